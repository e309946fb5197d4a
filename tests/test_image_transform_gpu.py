"""SURVEY 8(f1), image half: the device transform is bit-identical to Pillow's BILINEAR resize (golden g8 = Pillow's
own outputs) followed by float32 ToTensor / Normalize -- integer work, so the bar is exact equality.

select() mirrors the host's choice of kernel in ecgmm_image_transform (csrc/image_transform.hip): the widest horizontal tap
count -> KMAX, the fast condition, the band-height loop.  Every oracle case names the variant it is here for and asserts it, so
a later change of the selection flags the list as stale instead of silently testing something else; together the cases run
every KMAX instantiation of the fast kernel, the general kernel, every band height, and both kernels above 64 KiB of LDS."""
import math

import numpy as np
import pytest
import torch

from ecgmm import image_transform as IT
from oracle import image_ref as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_matches_pillow_golden_bit_for_bit(golden_dir):
    g8 = np.load(f"{golden_dir}/g8_image.npz")
    for i, (h, w, oh, ow) in enumerate(g8["cases"]):
        img = IR.synthetic_ecg_picture(int(h), int(w), 31 + i)
        out = IT.image_transform(torch.from_numpy(img).to(DEV), (int(oh), int(ow)))
        want = IR.to_tensor_normalize(g8[f"resized_{i}"])
        assert out.shape == (3, oh, ow) and out.dtype == torch.float32
        assert np.array_equal(out.cpu().numpy(), want), f"case {i}"


def _axis_taps(in_size, out_size):
    """Pillow's precompute_coeffs for the bilinear filter: [(first source index, tap count)] per output index"""
    scale = in_size / out_size
    support = max(scale, 1.0)
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        out.append((xmin, xmax - xmin))
    return out


def _align16(n):
    return (n + 15) // 16 * 16


def select(H, W, OH, OW):
    """-> (kernel, KMAX or 0, band height, LDS bytes) as ecgmm_image_transform chooses them; ("copy", 0, 0, 0) without a resize"""
    if (H, W) == (OH, OW):
        return "copy", 0, 0, 0
    h, v = _axis_taps(W, OW), _axis_taps(H, OH)
    nmax = max(n for _, n in h)
    kmax = next((k for k in (4, 8, 16, 24, 32, 48) if nmax <= k), 0)
    fast = OW <= 256 and kmax != 0 and W * 3 + 31 <= 1024 * 16
    raw = _align16(W * 3 + 32 + (3 * kmax if fast else 0))
    ksh = math.ceil(max(W / OW, 1.0)) * 2 + 1
    hk = 768 * 4 if fast else OW * ksh * 4
    for ob in (16, 8, 4, 2, 1):
        rows = max(v[min(oy0 + ob, OH) - 1][0] + v[min(oy0 + ob, OH) - 1][1] - v[oy0][0] for oy0 in range(0, OH, ob))
        lds = raw + _align16(rows * OW * 3) + hk
        if lds <= 64 * 1024 or (ob == 1 and lds <= 160 * 1024):
            return ("fast" if fast else "general"), (kmax if fast else 0), ob, lds
    return "refused", 0, 0, lds


# (B, H, W, OH, OW) -> (kernel, KMAX, band height) the case selects
ORACLE_CASES = {
    (5, 250, 2500, 224, 224): ("fast", 24, 16), (3, 224, 224, 224, 224): ("copy", 0, 0), (2, 250, 2500, 250, 2500): ("copy", 0, 0),
    (4, 250, 2500, 125, 1250): ("general", 0, 2), (3, 64, 48, 224, 224): ("fast", 4, 16), (2, 7, 9, 5, 4): ("fast", 8, 16),
    (1, 1000, 31, 10, 30): ("fast", 4, 4), (2, 300, 5000, 224, 224): ("fast", 48, 16), (2, 40, 6000, 20, 100): ("general", 0, 1),
    (2, 100, 5461, 50, 224): ("general", 0, 1), (3, 30, 40, 30, 64): ("fast", 4, 16),
    # the instantiations and boundaries nothing above runs
    (2, 12, 100, 6, 16): ("fast", 16, 16),
    (2, 9, 130, 4, 10): ("fast", 32, 16),
    (2, 160, 300, 32, 256): ("fast", 4, 8),
    (2, 3000, 24, 3, 24): ("fast", 4, 1),            # 147200 B of LDS: the fast kernel above 64 KiB
    (2, 8, 5451, 4, 256): ("fast", 48, 16),          # W * 3 + 31 == 16384 exactly: the last width the fast kernel takes
    (2, 8, 5452, 4, 256): ("general", 0, 1),         # one column more: the general kernel, 65552 B of LDS
    (2, 33, 257, 16, 256): ("fast", 4, 16),          # OW = 256: the last output width the fast kernel takes
    (2, 33, 257, 16, 257): ("general", 0, 16),
    (2, 40, 12, 3, 12): ("fast", 4, 16),              # W == OW, H != OH: the horizontal pass is the identity
}
ORACLE_LDS = {(2, 3000, 24, 3, 24): 147200, (2, 8, 5452, 4, 256): 65552}


def test_the_cases_select_what_they_are_here_for():
    seen = set()
    for case, want in ORACLE_CASES.items():
        kernel, kmax, ob, lds = select(*case[1:])
        assert (kernel, kmax, ob) == want, (case, (kernel, kmax, ob, lds))
        if case in ORACLE_LDS:
            assert lds == ORACLE_LDS[case] > 64 * 1024, (case, lds)
        seen.add((kernel, kmax, ob))
    assert 5451 * 3 + 31 == 1024 * 16
    assert {k for kern, k, _ in seen if kern == "fast"} == {4, 8, 16, 24, 32, 48}
    assert {kern for kern, _, _ in seen} == {"fast", "general", "copy"}
    assert {ob for kern, _, ob in seen if kern != "copy"} == {16, 8, 4, 2, 1}
    assert {ob for kern, _, ob in seen if kern == "general"} >= {16, 1} and {ob for kern, _, ob in seen if kern == "fast"} >= {16, 8, 1}


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_batches_and_other_shapes_vs_oracle(case):
    B, h, w, oh, ow = case
    assert select(h, w, oh, ow)[:3] == ORACLE_CASES[case]
    imgs = np.stack([IR.synthetic_ecg_picture(h, w, 70 + b) for b in range(B)])
    tf = IT.Compose([IT.Resize((oh, ow)), IT.ToTensor(), IT.Normalize([0.5] * 3, [0.5] * 3)])
    out = tf(torch.from_numpy(imgs).to(DEV)).cpu().numpy()
    for b in range(B):
        assert np.array_equal(out[b], IR.image_transform(imgs[b], oh, ow)), f"picture {b}"


def test_unaligned_views_and_other_statistics():
    """a picture batch that does not start on a 16-byte boundary, and per-channel mean/std"""
    raw = np.concatenate([np.zeros(5, np.uint8), IR.synthetic_ecg_picture(60, 333, 3).reshape(-1)])
    dev = torch.from_numpy(raw).to(DEV)
    view = dev[5:].view(1, 60, 333, 3)
    assert view.data_ptr() % 16 != 0
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    out = IT.image_transform(view, (32, 100), mean, std).cpu().numpy()
    want = IR.to_tensor_normalize(IR.resize_bilinear_u8(raw[5:].reshape(60, 333, 3), 32, 100), mean, std)
    assert np.array_equal(out[0], want)


def test_feeds_the_model(golden_dir):
    """transform output is what ECGMultimodalModel.forward takes: [B, 3, 224, 224] float32 in [-1, 1]"""
    imgs = torch.from_numpy(np.stack([IR.synthetic_ecg_picture(250, 2500, b) for b in range(2)])).to(DEV)
    x = IT.image_transform(imgs, (224, 224))
    assert x.shape == (2, 3, 224, 224) and float(x.min()) >= -1.0 and float(x.max()) <= 1.0


def test_rejects_bad_arguments():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IT.image_transform(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(ValueError):
        IT.image_transform(torch.zeros(1, 8, 8, 3, device=DEV), (4, 4))
    with pytest.raises(ValueError):
        IT.Compose([IT.Normalize([0.5] * 3, [0.5] * 3)])
