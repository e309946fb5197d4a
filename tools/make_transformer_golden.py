"""Generate tests/golden/g11_transformer.npz -- run ONLY where the reference checkout exists (default /root/reference, or
ECGMM_REFERENCE), never on the GPU machine.

The expected values come from the reference's OWN ``ECGTransformer1D`` and ``FocalLoss`` (train_physionet.py:211-257).  The
file is not imported (it pulls in wfdb and tensorflow at import time): the two ``ClassDef`` nodes are taken out of it with
``ast`` and executed alone in a namespace holding ``torch``, ``nn`` and ``F``.  Stored: the ``state_dict`` as float32, the
input, and the float64 and torch-float32-CPU logits, loss and parameter gradients -- data only, no reference text.
To stay under the size limit of a committed file a float64 gradient g64 is stored as the float32 pair (g32, g64 - g32), g32
being torch-float32-CPU's own gradient, which the test needs anyway: g64 = g32 + lo to about 2^-24 |g64 - g32|, i.e. to
float64 precision (``gradients()`` below undoes it).

Configuration: ECGTransformer1D(seq_len=48, d_model=64, nhead=4, num_layers=2, dim_feedforward=128), a seeded non-zero
pos_embedding, B = 5, L = 48, every dropout 0, train mode (torch's eval-mode fused path is not the formula under test)."""
import ast
import copy
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ECGMM_REFERENCE", "/root/reference")
CONFIG = dict(seq_len=48, d_model=64, nhead=4, num_layers=2, dim_feedforward=128)
B, L = 5, 48
LABELS = [0, 1, 1, 0, 1]


def reference_classes(*names):
    path = os.path.join(REF, "train_physionet.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    ns = {"torch": torch, "nn": nn, "F": F}
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def no_dropout(model):
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
        if isinstance(m, nn.MultiheadAttention):
            m.dropout = 0.0
    return model


def run(model, criterion, x, labels):
    model.zero_grad()
    logits = model(x)
    loss = criterion(logits, labels)
    loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def gradients(z):
    """{parameter name: (float64 gradient, torch-float32-CPU gradient)} of a loaded golden file"""
    out = {}
    for k in z.files:
        if k.startswith("g32/"):
            g32 = torch.from_numpy(z[k])
            out[k[4:]] = (g32.double() + torch.from_numpy(z["g64lo/" + k[4:]]).double(), g32)
    return out


def main():
    Model, Focal = reference_classes("ECGTransformer1D", "FocalLoss")
    torch.manual_seed(11)
    model = no_dropout(Model(**CONFIG)).train()
    with torch.no_grad():
        model.pos_embedding.copy_(0.1 * torch.randn(model.pos_embedding.shape))
    x = torch.randn(B, 1, L)
    labels = torch.tensor(LABELS)
    criterion = Focal(alpha=1.0, gamma=2.0)
    m64 = copy.deepcopy(model).double()
    lg64, loss64, g64 = run(m64, criterion, x.double(), labels)
    lg32, loss32, g32 = run(model, criterion, x, labels)
    xp = x.clone()
    xp[0] += 1.0
    with torch.no_grad():
        lg64p = m64(xp.double())
    assert lg64.dtype == torch.float64 and float((lg64p[1:] - lg64[1:]).abs().max()) > 1e-6, "samples do not interact?"
    out = {"x": x.numpy(), "labels": labels.numpy(), "logits64": lg64.numpy(), "loss64": loss64.numpy(),
           "logits32": lg32.numpy(), "loss32": loss32.numpy(), "logits64_perturbed": lg64p.numpy(),
           "keys": np.array(list(model.state_dict()))}
    for k, v in model.state_dict().items():
        out["sd/" + k] = v.numpy().astype(np.float32)
    for k in g64:
        out["g32/" + k] = g32[k].numpy()
        out["g64lo/" + k] = (g64[k] - g32[k].double()).float().numpy()
    path = os.path.join(ROOT, "tests", "golden", "g11_transformer.npz")
    np.savez_compressed(path, **out)
    n = sum(v.numel() for v in model.state_dict().values())
    print(path, os.path.getsize(path), "bytes;", n, "parameters; max |dlogits| of samples 1.. after perturbing sample 0:",
          float((lg64p[1:] - lg64[1:]).abs().max()))


if __name__ == "__main__":
    main()
