"""Parameter-holding nn.Modules whose forward runs HIP kernels.  They keep torch's parameter names,
shapes, default initialisation and state_dict format, so reference checkpoints load unchanged."""
import math

import torch
import torch.nn as nn

from . import functional as HF
from . import lib as L


class Linear(nn.Module):
    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(self.in_features)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x, act=L.ACT_NONE):
        return HF.linear(x, self.weight, self.bias, act)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}"


class LayerNorm(nn.Module):
    def __init__(self, normalized_shape, eps=1e-5):
        super().__init__()
        self.normalized_shape = (int(normalized_shape),)
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))

    def forward(self, x):
        return HF.layer_norm(x, self.weight, self.bias, self.eps)


class _ConvNd(nn.Module):
    """Weights of a convolution that only ever runs inside an encoder launch plan."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, bias, nd):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *([kernel_size] * nd)))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1 / math.sqrt(in_channels * kernel_size ** nd)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        raise RuntimeError(f"{type(self).__name__} is executed by its parent encoder's fused launch plan; "
                           "call the encoder (e.g. model.image_encoder(x)), not the layer")

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, "
                f"padding={self.padding}, bias={self.bias is not None}")


class Conv2d(_ConvNd):
    def __init__(self, cin, cout, k, stride=1, padding=0, bias=True):
        super().__init__(cin, cout, k, stride, padding, bias, 2)


class Conv1d(_ConvNd):
    def __init__(self, cin, cout, kernel_size, stride=1, padding=0, bias=True):
        super().__init__(cin, cout, kernel_size, stride, padding, bias, 1)


class _BatchNorm(nn.Module):
    def __init__(self, num_features, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = num_features, eps, momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def extra_repr(self):
        return f"{self.num_features}, eps={self.eps}, momentum={self.momentum}"


class BatchNorm2d(_BatchNorm):
    def forward(self, x):
        raise RuntimeError("BatchNorm2d is executed by its parent encoder's fused launch plan")


class BatchNorm1d(_BatchNorm):
    """Stand-alone use is the [B, C] case of the clinical MLP (PMB:258); inside ResNet1D_SE it is
    executed by the encoder plan."""

    def forward(self, x, relu=False):
        if x.dim() != 2:
            raise RuntimeError("BatchNorm1d over [B, C, L] is executed by its parent encoder's fused launch plan")
        return HF.batch_norm1d(x, self.weight, self.bias, self.running_mean, self.running_var,
                               self.num_batches_tracked, self.training, self.momentum, self.eps, relu)


class Sequential(nn.Sequential):
    """nn.Sequential whose forward fuses (Linear, ReLU|Sigmoid) and (BatchNorm1d, ReLU) pairs into one
    kernel epilogue and routes Dropout / Flatten to the HIP ops."""

    def forward(self, x):
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            if isinstance(m, (Linear, nn.Linear)):
                act = L.ACT_NONE
                if isinstance(nxt, nn.ReLU):
                    act, i = L.ACT_RELU, i + 1
                elif isinstance(nxt, nn.Sigmoid):
                    act, i = L.ACT_SIGMOID, i + 1
                x = HF.linear(x, m.weight, m.bias, act)
            elif isinstance(m, BatchNorm1d):
                relu = isinstance(nxt, nn.ReLU)
                x = m(x, relu=relu)
                i += int(relu)
            elif isinstance(m, nn.Dropout):
                x = HF.dropout(x, m.p, self.training and m.training)
            elif isinstance(m, nn.Flatten):
                x = x.reshape(x.shape[0], -1)
            elif isinstance(m, nn.Identity):
                pass
            else:
                x = m(x)
            i += 1
        return x


class LSTM(nn.Module):
    """``torch.nn.LSTM`` on the HIP recurrence kernels (train_physionet2.py:75-76): same parameter names, shapes,
    registration order, initialisation and state_dict keys, so checkpoints move in both directions.  Train and eval modes
    compute the same function (there is no dropout).  ``compute_dtype`` (``"fp32"`` default, or ``"bf16"``: the recurrent
    products on bf16 operands, see :func:`ecgmm.hip.functional.lstm`) is a property of the module, not of its parameters:
    they stay fp32 and a checkpoint does not carry it."""

    def __init__(self, input_size, hidden_size, num_layers=1, bias=True, batch_first=False, dropout=0.0,
                 bidirectional=False, proj_size=0, compute_dtype="fp32"):
        super().__init__()
        HF._lstm_dtype_code(compute_dtype)   # ValueError on anything but fp32 / bf16
        self.compute_dtype = str(compute_dtype).lower()
        if dropout != 0:
            raise ValueError(f"LSTM: dropout={dropout} is not supported (only dropout=0)")
        if proj_size != 0:
            raise ValueError(f"LSTM: proj_size={proj_size} is not supported (only proj_size=0)")
        if not bias:
            raise ValueError("LSTM: bias=False is not supported (only bias=True)")
        if input_size < 1 or hidden_size < 1 or num_layers < 1:
            raise ValueError("LSTM: input_size, hidden_size and num_layers must be >= 1")
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.bias, self.batch_first, self.dropout, self.bidirectional, self.proj_size = True, batch_first, 0.0, bidirectional, 0
        D = 2 if bidirectional else 1
        self._flat_names = []
        for layer in range(num_layers):
            for direction in range(D):
                In = input_size if layer == 0 else D * hidden_size
                sfx = f"_l{layer}" + ("_reverse" if direction else "")
                for name, shape in (("weight_ih", (4 * hidden_size, In)), ("weight_hh", (4 * hidden_size, hidden_size)),
                                    ("bias_ih", (4 * hidden_size,)), ("bias_hh", (4 * hidden_size,))):
                    setattr(self, name + sfx, nn.Parameter(torch.empty(*shape)))
                    self._flat_names.append(name + sfx)
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.hidden_size)
        for p in self.parameters():
            nn.init.uniform_(p, -bound, bound)

    def forward(self, x, hx=None, lengths=None):
        """``lengths`` (a list, a CPU or a device integer tensor, one per batch row): ``x`` stays padded and the result is
        torch's for the packed sequence, re-padded to ``T`` (:func:`ecgmm.hip.functional.lstm`)."""
        if isinstance(x, nn.utils.rnn.PackedSequence):
            raise TypeError("LSTM: a PackedSequence input is not supported: pass the padded tensor and lengths=")
        if x.dim() != 3:
            raise ValueError(f"LSTM: input must be 3-D (batched); unbatched {x.dim()}-D input is not supported")
        if x.shape[2] != self.input_size:
            raise ValueError(f"LSTM: input has {x.shape[2]} features, expected input_size={self.input_size}")
        params = [getattr(self, n) for n in self._flat_names]
        return HF.lstm(x, hx, params, self.hidden_size, self.num_layers, self.bidirectional, self.batch_first, lengths,
                       getattr(self, "compute_dtype", "fp32"))   # a module pickled before there was one: fp32

    def extra_repr(self):
        return (f"{self.input_size}, {self.hidden_size}, num_layers={self.num_layers}, batch_first={self.batch_first}, "
                f"bidirectional={self.bidirectional}")


class MultiheadAttention(nn.Module):
    """``torch.nn.MultiheadAttention`` restricted to what ``nn.TransformerEncoderLayer`` asks of it (train_physionet.py:219):
    self-attention with packed ``in_proj_weight`` / ``in_proj_bias`` and ``out_proj``, torch's names, shapes and
    initialisation.  ``forward(x)`` -> ``(output, None)``; the attention weights are never formed."""

    def __init__(self, embed_dim, num_heads, dropout=0.0, bias=True, add_bias_kv=False, add_zero_attn=False, kdim=None,
                 vdim=None, batch_first=False):
        super().__init__()
        for name, value, only in (("bias", bias, True), ("add_bias_kv", add_bias_kv, False),
                                  ("add_zero_attn", add_zero_attn, False)):
            if value != only:
                raise ValueError(f"MultiheadAttention: {name}={value} is not supported (only {name}={only})")
        for name, value in (("kdim", kdim), ("vdim", vdim)):
            if value is not None and value != embed_dim:
                raise ValueError(f"MultiheadAttention: {name}={value} is not supported (self-attention only: {name}=embed_dim)")
        if embed_dim < 1 or num_heads < 1 or embed_dim % num_heads:
            raise ValueError("MultiheadAttention: embed_dim must be divisible by num_heads")
        if embed_dim // num_heads not in (16, 32):
            raise ValueError(f"MultiheadAttention: head_dim={embed_dim // num_heads} is not supported (embed_dim / num_heads "
                             "must be 16 or 32)")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"MultiheadAttention: dropout={dropout} must lie in [0, 1)")
        self.embed_dim, self.num_heads, self.dropout, self.batch_first = embed_dim, num_heads, float(dropout), batch_first
        self.head_dim = embed_dim // num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        self.out_proj = Linear(embed_dim, embed_dim)
        self._reset_parameters()

    def _reset_parameters(self):
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.in_proj_bias, 0.0)
        nn.init.constant_(self.out_proj.bias, 0.0)

    def forward(self, query, key=None, value=None, key_padding_mask=None, need_weights=False, attn_mask=None,
                is_causal=False, *, lengths=None):
        """``lengths`` (keyword only; a list, a CPU or a device integer tensor, one per attention-batch element: dimension 0
        of the input with ``batch_first``, dimension 1 otherwise): positions at or behind an element's length are padding,
        torch's ``key_padding_mask[n, s] = s >= lengths[n]`` (:func:`ecgmm.hip.functional.multi_head_attention`).  The
        projections run over all rows, so PADDED INPUT MUST BE FINITE; the attention output is exactly zero at padded
        positions, the module's output there is ``out_proj.bias``."""
        for name, t in (("key", key), ("value", value)):
            if t is not None and t is not query:
                raise ValueError(f"MultiheadAttention: a separate {name} is not supported (self-attention only)")
        for name, t in (("key_padding_mask", key_padding_mask), ("attn_mask", attn_mask)):
            if t is not None:
                raise ValueError(f"MultiheadAttention: {name} is not supported (no masks; for padding pass lengths=)")
        if is_causal:
            raise ValueError("MultiheadAttention: is_causal=True is not supported (no masks)")
        if need_weights:
            raise ValueError("MultiheadAttention: need_weights=True is not supported (the weights are never formed)")
        if query.dim() != 3 or query.shape[2] != self.embed_dim:
            raise ValueError(f"MultiheadAttention: input must be 3-D with {self.embed_dim} features, got {tuple(query.shape)}")
        lengths = self._lengths(lengths, query)
        return self._attend(query.reshape(-1, self.embed_dim), query.shape, lengths).reshape(query.shape), None

    def _lengths(self, lengths, x):
        """``lengths`` of a 3-D input ``x`` -> ``None`` or the device ``int32 [N]`` tensor the kernels take, validated once
        (:func:`ecgmm.hip.functional.check_lengths`; a device tensor is taken as given)"""
        if lengths is None:
            return None
        S, N = (x.shape[1], x.shape[0]) if self.batch_first else (x.shape[0], x.shape[1])
        return HF.check_lengths(lengths, N, S).to(x.device)

    def _attend(self, x2, shape, lengths=None, sink=None):
        """x2 [rows, E], the rows of a tensor of ``shape`` -> [rows, E]; ``lengths``: as :meth:`_lengths` returns them.
        ``sink`` (a list): a record of this attention is appended -- detached ``qkv`` and ``lse`` and ``S``, ``N``, ``heads``,
        ``batch_first``, ``lengths``, the arguments of :func:`ecgmm.hip.functional.attention_weights`; the launches and the
        result are the same with and without it."""
        S, N = (shape[1], shape[0]) if self.batch_first else (shape[0], shape[1])
        qkv = HF.linear(x2, self.in_proj_weight, self.in_proj_bias)
        if sink is None:
            a = HF.multi_head_attention(qkv, S, N, self.num_heads, self.batch_first, self.dropout, self.training,
                                        lengths=lengths)
        else:
            a, lse = HF.multi_head_attention(qkv, S, N, self.num_heads, self.batch_first, self.dropout, self.training,
                                             lengths=lengths, return_lse=True)
            sink.append({"qkv": qkv.detach(), "lse": lse.detach(), "S": S, "N": N, "heads": self.num_heads,
                         "batch_first": self.batch_first, "lengths": lengths})
        return HF.linear(a, self.out_proj.weight, self.out_proj.bias)

    def attention_weights(self, x, *, lengths=None, average_attn_weights=True):
        """The attention weights of ``forward(x, lengths=lengths)``: ``[N, S, S]`` averaged over the heads, or
        ``[N, heads, S, S]`` with ``average_attn_weights=False`` -- what torch's ``need_weights=True`` returns, computed from
        the forward's stored log-sum-exp by ``ecgmm_mha_weights`` (``forward(need_weights=True)`` itself stays refused: the
        forward never forms them).  Always the probabilities BEFORE dropout, also in training mode.  With ``lengths`` the
        padded query rows and key columns are exact zeros.  Detached, no gradient."""
        if x.dim() != 3 or x.shape[2] != self.embed_dim:
            raise ValueError(f"MultiheadAttention: input must be 3-D with {self.embed_dim} features, got {tuple(x.shape)}")
        S, N = (x.shape[1], x.shape[0]) if self.batch_first else (x.shape[0], x.shape[1])
        lengths = self._lengths(lengths, x)
        with torch.no_grad():   # no dropout: the log-sum-exp does not depend on it, and no Philox offset is taken
            qkv = HF.linear(x.reshape(-1, self.embed_dim), self.in_proj_weight, self.in_proj_bias)
            _, lse = HF.multi_head_attention(qkv, S, N, self.num_heads, self.batch_first, lengths=lengths, return_lse=True)
        return HF.attention_weights(qkv, lse, S, N, self.num_heads, self.batch_first, lengths, average_attn_weights)


class TransformerEncoderLayer(nn.Module):
    """``torch.nn.TransformerEncoderLayer``, post-norm with ReLU (train_physionet.py:219): existing ops around the attention
    kernel -- ``linear`` (ReLU in ``linear1``'s epilogue), ``dropout``, the residual adds through ``ecgmm_ew``,
    ``layer_norm``.  torch's sub-module names, so ``state_dict``s move in both directions."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", layer_norm_eps=1e-5,
                 batch_first=False, norm_first=False, bias=True):
        super().__init__()
        if norm_first:
            raise ValueError("TransformerEncoderLayer: norm_first=True is not supported (only post-norm)")
        if not (activation == "relu" or activation is torch.relu or activation is nn.functional.relu or
                isinstance(activation, nn.ReLU)):
            raise ValueError(f"TransformerEncoderLayer: activation={activation!r} is not supported (only relu)")
        if not bias:
            raise ValueError("TransformerEncoderLayer: bias=False is not supported (only bias=True)")
        self.self_attn = MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=batch_first)
        self.linear1 = Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = Linear(dim_feedforward, d_model)
        self.norm_first = False
        self.norm1 = LayerNorm(d_model, eps=layer_norm_eps)
        self.norm2 = LayerNorm(d_model, eps=layer_norm_eps)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)

    def forward(self, src, src_mask=None, src_key_padding_mask=None, is_causal=False, *, lengths=None, attention_sink=None):
        """``attention_sink`` (keyword only; a list): the layer appends the record of its attention
        (:meth:`MultiheadAttention._attend`), from which ``ecgmm.explain`` rebuilds the maps; the output is bit-identical with
        and without it.  ``lengths`` (keyword only): one length per attention-batch element (dimension 0 of ``src`` with ``batch_first``,
        dimension 1 otherwise), as :meth:`MultiheadAttention.forward` takes them: padded positions are never keys.
        Everything around the attention (projections, residual adds, LayerNorm, feed-forward) runs over all rows, so
        PADDED ``src`` MUST BE FINITE and the padded rows of the output are not zero; nothing live depends on them, and
        their gradient is zero when the loss ignores them."""
        for name, t in (("src_mask", src_mask), ("src_key_padding_mask", src_key_padding_mask)):
            if t is not None:
                raise ValueError(f"TransformerEncoderLayer: {name} is not supported (no masks; for padding pass lengths=)")
        if is_causal:
            raise ValueError("TransformerEncoderLayer: is_causal=True is not supported (no masks)")
        E = self.self_attn.embed_dim
        if src.dim() != 3 or src.shape[2] != E:
            raise ValueError(f"TransformerEncoderLayer: input must be 3-D with {E} features, got {tuple(src.shape)}")
        lengths = self.self_attn._lengths(lengths, src)
        t = self.training
        x = src.reshape(-1, E)
        a = HF.dropout(self.self_attn._attend(x, src.shape, lengths, attention_sink), self.dropout1.p,
                       t and self.dropout1.training)
        x = self.norm1(HF.add(x, a))
        h = HF.dropout(self.linear1(x, act=L.ACT_RELU), self.dropout.p, t and self.dropout.training)
        f = HF.dropout(self.linear2(h), self.dropout2.p, t and self.dropout2.training)
        return self.norm2(HF.add(x, f)).reshape(src.shape)


class TransformerEncoder(nn.Module):
    """``torch.nn.TransformerEncoder``: ``num_layers`` deep copies of ``encoder_layer`` under ``layers.{i}`` (so, as in
    torch, every layer starts from the same initial weights)."""

    def __init__(self, encoder_layer, num_layers, norm=None, enable_nested_tensor=True, mask_check=True):
        super().__init__()
        import copy
        if not isinstance(encoder_layer, TransformerEncoderLayer):
            raise ValueError("TransformerEncoder: encoder_layer must be an ecgmm.hip.nn.TransformerEncoderLayer")
        if norm is not None:
            raise ValueError("TransformerEncoder: norm is not supported (only norm=None)")
        if num_layers < 1:
            raise ValueError("TransformerEncoder: num_layers must be >= 1")
        self.layers = nn.ModuleList([copy.deepcopy(encoder_layer) for _ in range(num_layers)])
        self.num_layers = num_layers
        self.norm = None

    def forward(self, src, mask=None, src_key_padding_mask=None, is_causal=None, *, lengths=None, attention_sink=None):
        """``lengths`` (keyword only): one length per attention-batch element, validated once and passed to every layer
        (:meth:`TransformerEncoderLayer.forward`: padded ``src`` must be finite, padded output rows are not zero).
        ``attention_sink`` (keyword only; a list): every layer appends the record of its attention, first layer first."""
        for name, t in (("mask", mask), ("src_key_padding_mask", src_key_padding_mask)):
            if t is not None:
                raise ValueError(f"TransformerEncoder: {name} is not supported (no masks; for padding pass lengths=)")
        if is_causal:
            raise ValueError("TransformerEncoder: is_causal=True is not supported (no masks)")
        if lengths is not None and src.dim() == 3:
            lengths = self.layers[0].self_attn._lengths(lengths, src)
        x = src
        for layer in self.layers:
            kw = {} if lengths is None else {"lengths": lengths}
            if attention_sink is not None:
                kw["attention_sink"] = attention_sink
            x = layer(x, **kw)
        return x
