"""Float64 reference of the TabNet eval forward for csrc/tabnet_infer.hip, shared by tests/test_tabnet_infer_*.py.

`reference` evaluates the UNFOLDED network -- oracle.tabnet_ref's modules cast to double: every BatchNorm as
(x - rm) / sqrt(rv + eps) * gamma + beta on the running statistics, every fc bias-free, the sparsemax by sorting -- and keeps
every intermediate the bounds of tests/tabnet_infer_bounds.py need (per-layer activations, sparsemax inputs, tau, masks, priors,
d, M_explain, row_entropy, out) next to the float64 FOLD of each layer (W' = s W, b' = beta - rm s), which is what the
kernel's blob is compared with.

`candidate` is the kernel's restatement -- fold first, then the folded chain -- evaluated with torch in fp32, with named slips.

Nothing here reads a file; the parameters come from oracle.fill.hash_fill_module (keyed by the state-dict name, so that all
BatchNorms differ)."""
import math
from types import SimpleNamespace as NS

import torch

from oracle import fill
from oracle import tabnet_ref as O

BN_EPS = 1e-5
SLIPS = ("shared_bn_of_another_use", "no_sqrt_half", "prior_never_updated", "previous_mask", "mask_on_raw_x",
         "importance_without_relu", "m_explain_plain_sum", "padded_features_counted")


def case(B, seed=0, **kw):
    """(cfg, B, seed) of the shape grid"""
    return cfg(**kw), B, seed


def grid():
    """The shapes the GPU tests run and the CPU tests vet: every tile capacity of the kernel (n_d + n_a <= 32 / 64 / 128 with
    D <= 16 / > 16), ragged D, a partial last tile of rows, more than one workgroup (B = 65, 130), one row, every
    (n_shared, n_independent) pattern, both gammas.  For every case with D >= 5 the seed is one for which each step of the
    float64 reference has a certain zero and a certain positive (tests/test_tabnet_infer_cpu.py checks that)."""
    return [case(33),                                                                        # the clinical encoder's shape
            case(17, D=5, n_d=16, n_a=16, n_steps=1, n_shared=0, n_independent=2),
            case(65, D=17, n_d=16, n_a=48, n_steps=5, n_shared=2, n_independent=0, out_dim=16, gamma=1.0),
            case(130, D=64, n_d=64, n_a=64, n_steps=3, n_shared=1, n_independent=1, out_dim=128),
            case(16, D=16, gamma=1.0),
            case(15, D=5, n_d=64, n_a=64, n_steps=1),
            case(1, D=2, n_d=16, n_a=16, n_steps=5, n_shared=1, n_independent=1, out_dim=16),
            case(33, D=64, n_d=16, n_a=48, n_steps=3, n_shared=0, n_independent=2, gamma=1.0),
            case(17, D=17, n_d=16, n_a=16, n_steps=3, n_shared=2, n_independent=0)]


def case_id(k):
    c, B, seed = k
    return "B%d-D%d-nd%d-na%d-s%d-sh%d-in%d-o%d-g%g" % (B, c.D, c.n_d, c.n_a, c.n_steps, c.n_shared, c.n_independent, c.out_dim,
                                                       c.gamma)


def cfg(D=2, n_d=32, n_a=32, n_steps=3, n_shared=2, n_independent=2, out_dim=32, gamma=1.5, epsilon=1e-15):
    return NS(D=D, n_d=n_d, n_a=n_a, n_steps=n_steps, n_shared=n_shared, n_independent=n_independent, out_dim=out_dim,
              gamma=gamma, epsilon=epsilon)


def build(c, tag="tn."):
    """oracle TabNetNoEmbeddings of configuration c, hash-filled, in eval mode (fp32 parameters)"""
    m = O.TabNetNoEmbeddings(c.D, c.out_dim, n_d=c.n_d, n_a=c.n_a, n_steps=c.n_steps, gamma=c.gamma,
                             n_independent=c.n_independent, n_shared=c.n_shared, epsilon=c.epsilon)
    return fill.hash_fill_module(m, tag).eval()


def param_table(model):
    """the C ABI's parameter table: every floating tensor of the state_dict in its order (num_batches_tracked left out)"""
    return [v for v in model.state_dict().values() if v.is_floating_point()]


def inputs(B, D, seed=0, scale=1.5):
    """B rows of D features; row 1 (if any) has all features equal, row 2 one dominant feature"""
    x = fill.hash_tensor((B, D), 7000 + seed, scale)
    if B > 1:
        x[1] = 0.75
    if B > 2:
        x[2] = 0.01 * x[2]
        x[2, (seed + D // 2) % D] = 6.0
    return x


def sparsemax_tau(z):
    """(p, tau, support size) of the sparsemax of the rows of z by sorting (Martins & Astudillo, Alg. 1), in z's dtype"""
    srt, _ = torch.sort(z, dim=-1, descending=True)
    cum = srt.cumsum(-1) - 1
    rho = torch.arange(1, z.shape[-1] + 1, dtype=z.dtype)
    k = (rho * srt > cum).sum(-1, keepdim=True)
    tau = cum.gather(-1, k - 1) / k.to(z.dtype)
    return torch.clamp(z - tau, min=0), tau, k


def _layers(ft):
    """the GLU layers of a FeatTransformer in execution order; the first one has no residual"""
    out = []
    for block in (ft.shared, ft.specifics):
        if isinstance(block, O.GLU_Block):
            out += list(block.glu_layers)
    return out


def _fold(fc_weight, bn, dtype):
    """(W', b', |rm s|, s) of a bias-free fc followed by BatchNorm `bn`, in `dtype` arithmetic"""
    w = fc_weight.detach().to(dtype)
    g, b, rm, rv = (t.detach().to(dtype) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    s = g / torch.sqrt(rv + torch.tensor(bn.eps, dtype=dtype))
    return s[:, None] * w, b - rm * s, (rm * s).abs(), s


def folds(model, dtype=torch.float64, slip=None):
    """the fold of every layer: NS(bn0=(scale, shift, |rm s|), ft[f][l] = (W', b', |rm s|), att[s] = ..., final=W)"""
    enc = model.encoder
    bn0 = enc.initial_bn
    g, b, rm, rv = (t.detach().to(dtype) for t in (bn0.weight, bn0.bias, bn0.running_mean, bn0.running_var))
    s0 = g / torch.sqrt(rv + torch.tensor(bn0.eps, dtype=dtype))
    fts = [enc.initial_splitter] + list(enc.feat_transformers)
    n_shared = len(enc.initial_splitter.shared.glu_layers) if isinstance(enc.initial_splitter.shared, O.GLU_Block) else 0
    ft = []
    for f, t in enumerate(fts):
        row = []
        for l, lay in enumerate(_layers(t)):
            bn = lay.bn.bn
            if slip == "shared_bn_of_another_use" and l < n_shared:     # the statistics of the NEXT use of the shared fc
                bn = _layers(fts[(f + 1) % len(fts)])[l].bn.bn
            row.append(_fold(lay.fc.weight, bn, dtype)[:3])
        ft.append(row)
    att = [_fold(a.fc.weight, a.bn.bn, dtype)[:3] for a in enc.att_transformers]
    return NS(bn0=(s0, b - rm * s0, (rm * s0).abs()), ft=ft, att=att, final=model.final_mapping.weight.detach().to(dtype))


def _chain(c, F, x, dtype, slip=None, keep=False, forced=None):
    """the folded chain on x in `dtype`; keep: record every intermediate.  forced [n_steps, B, D]: masks to carry on with --
    step s still computes ITS mask M (what `masks` returns and a candidate's mask is compared with) from what came before, but
    everything downstream of it (entropy, prior, masked input, M_explain) uses forced[s] (recorded as Mu)."""
    x = x.to(dtype)
    scale = 1.0 if slip == "no_sqrt_half" else math.sqrt(0.5)
    sc, sh, _ = F.bn0
    xn = x * sc + sh
    B, D = x.shape
    rec = NS(x=x, xn=xn, ft=[], steps=[])

    def feat(f, a):
        h, layers = None, []
        for l, (W, b, rms) in enumerate(F.ft[f]):
            z = a @ W.t() + b
            A, G = z[:, :c.n_d + c.n_a], z[:, c.n_d + c.n_a:]
            o = A * torch.sigmoid(G)
            hn = o if l == 0 else (h + o) * scale
            if keep:
                layers.append(NS(a=a, W=W, b=b, rms=rms, A=A, G=G, o=o, h_prev=h, h=hn))
            h = a = hn
        rec.ft.append(layers)
        return h

    h = feat(0, xn)
    prior = torch.ones(B, D, dtype=dtype)
    dsum = torch.zeros(B, c.n_d, dtype=dtype)
    mexp = torch.zeros(B, D, dtype=dtype)
    ent = torch.zeros(B, dtype=dtype)
    masks, M_prev = [], torch.ones(B, D, dtype=dtype) / D
    for s in range(c.n_steps):
        W, b, rms = F.att[s]
        att = h[:, c.n_d:]
        z = att @ W.t() + b
        zp = z * prior
        if slip == "padded_features_counted" and D % 16:
            pad = torch.zeros(B, (D + 15) // 16 * 16 - D, dtype=dtype)
            M, tau, k = sparsemax_tau(torch.cat([zp, pad], 1))
            M = M[:, :D]
        else:
            M, tau, k = sparsemax_tau(zp)
        Mu = M if forced is None else forced[s].to(dtype)
        term = Mu * torch.log(Mu + torch.tensor(c.epsilon, dtype=dtype))
        ent = ent + term.sum(1)
        prior_next = prior if slip == "prior_never_updated" else prior * (c.gamma - Mu)
        Mx = M_prev if slip == "previous_mask" else Mu
        mx = Mx * (x if slip == "mask_on_raw_x" else xn)
        h = feat(s + 1, mx)
        d = torch.relu(h[:, :c.n_d])
        imp = (h[:, :c.n_d] if slip == "importance_without_relu" else d).sum(1, keepdim=True)
        mexp = mexp + (Mu if slip == "m_explain_plain_sum" else Mu * imp)
        dsum = dsum + d
        if keep:
            rec.steps.append(NS(att=att, W=W, b=b, rms=rms, z=z, prior=prior, zp=zp, tau=tau, k=k, M=M, Mu=Mu, term=term,
                                prior_next=prior_next, mx=mx, d=d, imp=imp))
        masks.append(M)
        prior, M_prev = prior_next, Mu
    rec.forced = forced is not None
    rec.dsum, rec.m_explain, rec.row_entropy, rec.masks = dsum, mexp, ent, torch.stack(masks)
    rec.final = F.final
    rec.out = dsum @ F.final.t()
    return rec


def reference(c, model, x, forced=None):
    """float64, every intermediate kept.  The chain runs on the float64 fold, which in real arithmetic IS the unfolded
    network (s (W a) + beta - rm s = BN(W a)); `unfolded_out` evaluates the modules themselves for the CPU test of that.

    forced: the masks [n_steps, B, D] a candidate (the kernel, the fp32 restatement) returned.  They are outputs, so a check
    may take them as given: step s's mask is then the float64 function of the candidate's masks 0 .. s-1, and out, M_explain
    and row_entropy the float64 functions of all of them.  Every output element is still compared; what changes is that an
    error is propagated through ONE FeatTransformer and one attentive layer, not through n_steps + 1 of them -- the worst-case
    propagation by |W'| grows about 7x per layer on these weights and is vacuous over 16 layers."""
    rec = _chain(c, folds(model, torch.float64), x, torch.float64, keep=True, forced=forced)
    rec.folds = folds(model, torch.float64)
    return rec


@torch.no_grad()
def unfolded_out(model, x):
    """(out, M_loss) of oracle.tabnet_ref's own eval forward on a double copy of the modules"""
    import copy
    m = copy.deepcopy(model).double().eval()
    m.encoder.group_attention_matrix = m.encoder.group_attention_matrix.double()
    return m(x.double())


def candidate(c, model, x, slip=None):
    """the kernel's restatement in torch fp32: fold in fp32, then the folded chain in fp32"""
    return _chain(c, folds(model, torch.float32, slip), x, torch.float32, slip)
