"""Stand-alone rates of the BatchNorm element-wise passes at the ResNet18 layer shapes (batch 256, bf16): bn_act without / with
a residual, full BatchNorm backward (reduce + finalize + apply) and the apply-from-rows form.  Bytes = the tensors each pass must
move once; GB/s against the 6.29 TB/s a float4 copy reaches on this chip (MI355X_MICROARCH.md).
The passes that fold the finalize (bn_act from rows, both backward forms) are timed with the channel-sliced launch off and on
(ecgmm_bn_fold_slice) where it applies (C >= 256), alternating, in the same process.  At the output shapes of the three
downsample blocks: bn2's + the shortcut BatchNorm's backward as separate calls against ecgmm_bn_bwd_dual, alternating.
The stem's fused BatchNorm + ReLU + max-pool at the image and the signal shape (bytes: y read once, pooled and argmax bytes
written; the 2.25x window re-reads are cache traffic, not counted) and the SE gate pass ecgmm_se_gate_bn at the three widths of
the signal encoder (three tensors read, dz written).
--cases bn,pool,se picks the groups (default: all); ECGMM_LIB picks another build of the library for an A/B in one call."""
import argparse, ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="bn,pool,se")
cases = ap.parse_args().cases.split(",")
lib = L.lib()
B = 256
def timeit(fn, n=30):
    for _ in range(5): L.check(fn())
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): L.check(fn())
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda:0")
LAYERS = (("l1", 56 * 56, 64), ("l2", 28 * 28, 128), ("l3", 14 * 14, 256), ("l4", 7 * 7, 512))
for name, HW, Cn in (LAYERS if "bn" in cases else ()):
    M = B * HW
    n = M * Cn
    mk = lambda: torch.randn(n, device="cuda:0").to(torch.bfloat16)
    # rotate over several buffers so that the passes do not run out of the 256 MB Infinity Cache
    K = max(2, int(600e6 // (n * 2)))
    ys, rs, os_ = [mk() for _ in range(K)], [mk() for _ in range(K)], [torch.empty(n, device="cuda:0", dtype=torch.bfloat16) for _ in range(K)]
    coef = torch.rand(4 * Cn, device="cuda:0") + 0.5
    gamma = torch.rand(Cn, device="cuda:0") + 0.5
    dg, db = torch.empty(Cn, device="cuda:0"), torch.empty(Cn, device="cuda:0")
    scratch = torch.empty(lib.ecgmm_bn_bwd_scratch(L.BF16, M, Cn), dtype=torch.uint8, device="cuda:0")
    it = [0]
    def nxt():
        it[0] = (it[0] + 1) % K
        return it[0]
    def act(): i = nxt(); return lib.ecgmm_bn_act(L.BF16, ptr(ys[i]), ptr(coef), None, None, None, 1, 1, ptr(os_[i]), M, Cn, stream())
    def act_res(): i = nxt(); return lib.ecgmm_bn_act(L.BF16, ptr(ys[i]), ptr(coef), ptr(rs[i]), None, None, 1, 1, ptr(os_[i]), M, Cn, stream())
    def bwd(): i = nxt(); return lib.ecgmm_bn_bwd(L.BF16, ptr(rs[i]), ptr(ys[i]), None, None, 1, ptr(ys[i]), ptr(coef), ptr(gamma), ptr(dg), ptr(db), ptr(os_[i]), None, None, M, Cn, ptr(scratch), stream())
    rows = torch.rand(256 * 2 * Cn, device="cuda:0")
    def bwd_rows(): i = nxt(); return lib.ecgmm_bn_bwd_from_rows(L.BF16, ptr(rs[i]), ptr(ys[i]), ptr(ys[i]), ptr(coef), ptr(gamma), ptr(dg), ptr(db), ptr(os_[i]), ptr(rows), 256, M, Cn, ptr(scratch), stream())
    beta, rm, rv = torch.zeros(Cn, device="cuda:0"), torch.zeros(Cn, device="cuda:0"), torch.ones(Cn, device="cuda:0")
    nbt = torch.zeros((), dtype=torch.int64, device="cuda:0")
    coef_o = torch.empty(4 * Cn, device="cuda:0")
    srows = torch.rand(256 * 2 * Cn, device="cuda:0") + 1.0
    def act_rows(res):
        def f(): i = nxt(); return lib.ecgmm_bn_act_from_rows(L.BF16, ptr(ys[i]), ptr(srows), 256, float(M), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), 0.1, 1e-5, ptr(coef_o), ptr(rs[i]) if res else None, None, None, 1, 1, ptr(os_[i]), M, Cn, stream())
        return f
    def show(label, us, tensors):
        print(f"{name} C={Cn:3d} M={M:7d} {label:34s} {us:7.1f} us  {tensors * n * 2 / us / 1e6:6.2f} TB/s ({tensors} x {n * 2 / 1e6:.0f} MB, {K} buffer sets in rotation)")
    for label, fn, tensors in (("bn_act", act, 2), ("bn_act+residual", act_res, 3)):
        show(label, timeit(fn), tensors)
    for label, fn, tensors in (("bn_act from rows", act_rows(False), 2), ("bn_act+residual from rows", act_rows(True), 3),
                               ("bn_bwd reduce+apply", bwd, 5), ("bn_bwd apply from rows", bwd_rows, 3)):
        for sl in ((0, 1, 0, 1) if Cn >= 256 else (1,)):
            lib.ecgmm_bn_fold_slice(sl)
            show(label + (" [slice %d]" % sl if Cn >= 256 else ""), timeit(fn), tensors)
    lib.ecgmm_bn_fold_slice(1)
    if Cn < 128:
        continue
    # downsample blocks (their output shapes): bn2's backward with the bit mask and dz_out, then the shortcut BatchNorm's backward of
    # that dz -- two reduce + two apply launches, 11 tensor passes -- against ecgmm_bn_bwd_dual, one of each, 9 passes; alternating
    y2s, dzs, dyds = [mk() for _ in range(K)], [torch.empty_like(os_[0]) for _ in range(K)], [torch.empty_like(os_[0]) for _ in range(K)]
    mbits = torch.randint(0, 256, (n // 8,), dtype=torch.uint8, device="cuda:0")
    coefd, gammad = torch.rand(4 * Cn, device="cuda:0") + 0.5, torch.rand(Cn, device="cuda:0") + 0.5
    dgd, dbd = torch.empty(Cn, device="cuda:0"), torch.empty(Cn, device="cuda:0")
    scratch_d = torch.empty_like(scratch)
    def separate():
        i = nxt()
        rc = lib.ecgmm_bn_bwd_bits(L.BF16, ptr(rs[i]), ptr(mbits), None, None, 1, ptr(ys[i]), ptr(coef), ptr(gamma), ptr(dg), ptr(db), ptr(os_[i]), ptr(dzs[i]), None, M, Cn, ptr(scratch), stream())
        return rc or lib.ecgmm_bn_bwd(L.BF16, ptr(dzs[i]), None, None, None, 1, ptr(y2s[i]), ptr(coefd), ptr(gammad), ptr(dgd), ptr(dbd), ptr(dyds[i]), None, None, M, Cn, ptr(scratch_d), stream())
    def dual():
        i = nxt()
        return lib.ecgmm_bn_bwd_dual(L.BF16, ptr(rs[i]), None, ptr(mbits), None, None, ptr(ys[i]), ptr(coef), ptr(gamma), ptr(dg), ptr(db), ptr(os_[i]), ptr(y2s[i]), ptr(coefd), ptr(gammad), ptr(dgd), ptr(dbd), ptr(dyds[i]), ptr(dzs[i]), None, M, Cn, ptr(scratch), ptr(scratch_d), stream())
    for _ in range(2):
        show("bn2 + shortcut bn_bwd, separate", timeit(separate), 11)
        show("bn2 + shortcut bn_bwd, dual", timeit(dual), 9)

def rotating(n_bytes_per_set):
    return max(2, int(600e6 // n_bytes_per_set))
bf = torch.bfloat16
for name, H, W in ((("pool image", 112, 112), ("pool signal", 1, 2500)) if "pool" in cases else ()):
    Cn = 64
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    n_in, n_out = B * H * W * Cn, B * OH * OW * Cn
    K = rotating(n_in * 2 + n_out * 3)
    ys = [torch.randn(n_in, device="cuda:0").to(bf) for _ in range(K)]
    ps = [torch.empty(n_out, device="cuda:0", dtype=bf) for _ in range(K)]
    ix = [torch.empty(n_out, device="cuda:0", dtype=torch.uint8) for _ in range(K)]
    coef = torch.rand(4 * Cn, device="cuda:0") + 0.5
    it = [0]
    def pool():
        it[0] = (it[0] + 1) % K
        i = it[0]
        return lib.ecgmm_bnrelu_maxpool(L.BF16, ptr(ys[i]), ptr(coef), ptr(ps[i]), ptr(ix[i]), B, H, W, Cn, stream())
    nbytes = n_in * 2 + n_out * 3
    for _ in range(2):
        us = timeit(pool)
        print(f"{name} {B} x {H} x {W} x {Cn} bnrelu_maxpool            {us:7.1f} us  {nbytes / us / 1e6:6.2f} TB/s ({nbytes / 1e6:.0f} MB, {K} buffer sets in rotation)")
for R, Cn in (((1250, 64), (625, 128), (313, 256)) if "se" in cases else ()):
    n = B * R * Cn
    K = rotating(n * 2 * 4)
    mk = lambda: torch.randn(n, device="cuda:0").to(bf)
    ds, ms, ys, zs = [mk() for _ in range(K)], [mk() for _ in range(K)], [mk() for _ in range(K)], [torch.empty(n, device="cuda:0", dtype=bf) for _ in range(K)]
    coef = torch.rand(4 * Cn, device="cuda:0") + 0.5
    dg, a1, a2, a3 = (torch.empty(B * Cn, device="cuda:0") for _ in range(4))
    it = [0]
    def se():
        it[0] = (it[0] + 1) % K
        i = it[0]
        return lib.ecgmm_se_gate_bn(L.BF16, ptr(ds[i]), ptr(ms[i]), ptr(ys[i]), ptr(coef), ptr(zs[i]), ptr(dg), ptr(a1), ptr(a2), ptr(a3), B, R, Cn, stream())
    def gg():
        it[0] = (it[0] + 1) % K
        i = it[0]
        return lib.ecgmm_se_gate_grad(L.BF16, ptr(ds[i]), ptr(ms[i]), ptr(ys[i]), ptr(coef), ptr(dg), B, R, Cn, stream())
    for _ in range(2):
        us = timeit(se)
        print(f"se {B} x {R} x {Cn} se_gate_bn                          {us:7.1f} us  {4 * n * 2 / us / 1e6:6.2f} TB/s (4 x {n * 2 / 1e6:.0f} MB, {K} buffer sets in rotation)")
        us = timeit(gg)
        print(f"se {B} x {R} x {Cn} se_gate_grad                        {us:7.1f} us  {3 * n * 2 / us / 1e6:6.2f} TB/s (3 x {n * 2 / 1e6:.0f} MB, {K} buffer sets in rotation)")
