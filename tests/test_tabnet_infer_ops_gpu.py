"""ecgmm_tabnet_infer_prepare / ecgmm_tabnet_infer (csrc/tabnet_infer.hip) through the C ABI between sentinel zones
(tests/tabnet_infer_abi.py): the fold against the float64 fold element by element, every element of out, of each mask, of
M_explain and of row_entropy within its float64 bound (tests/tabnet_infer_bounds.py, nothing tuned), exact zeros outside the
support, and the bit identities: a row's bits independent of B and of its place in a tile, two calls the same, out the same
whichever optional outputs are requested, nothing written outside an output or past the blob.

The shapes are tests/tabnet_infer_ref.grid(): every tile capacity of the kernel, ragged D, B over 1, 15, 16, 17, 33, 65, 130."""
import pytest
import torch

from . import tabnet_infer_abi as A
from . import tabnet_infer_bounds as TB
from . import tabnet_infer_ref as R

pytestmark = pytest.mark.gpu
GRID = R.grid()
IDS = [R.case_id(k) for k in GRID]

_cache = {}


def _case(k):
    """(model, x, device x, blob, bytes, outputs of one full call) of a grid case, computed once"""
    key = R.case_id(k)
    if key not in _cache:
        c, B, seed = k
        with torch.no_grad():
            m = R.build(c)
            x = R.inputs(B, c.D, seed)
            blob, nb = A.prepare(c, A.to_dev(m))
            xd = x.to(A.DEV)
            _cache[key] = (m, x, xd, blob, nb, A.forward(c, blob, nb, xd))
    return _cache[key]


_refs = {}


def _ref(k):
    """(float64 reference forced with the kernel's masks, its bounds) of a grid case, computed once and left unchanged"""
    key = R.case_id(k)
    if key not in _refs:
        c = k[0]
        m, x, _, _, _, got = _case(k)
        with torch.no_grad():
            r = R.reference(c, m, x, forced=got["masks"].cpu())
            _refs[key] = (r, TB.Forward(c, r))
    return _refs[key]


# ---- the fold -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", GRID, ids=IDS)
def test_fold_matches_the_float64_fold_element_by_element(k):
    c = k[0]
    m, _, _, blob, nb, _ = _case(k)
    F, u = R.folds(m), A.unpack(c, blob, nb)
    worst = 0.0

    def judge(w, b, W, bb, rms, what):
        nonlocal worst
        rows, cols = W.shape
        rw = TB.ratio((w[:rows, :cols].double() - W).abs(), TB.fold_weight(W))
        rb = TB.ratio((b[:rows].double() - bb).abs(), TB.fold_bias(bb, rms))
        assert rw <= 1.0 and rb <= 1.0, "%s: weight %.3g x, bias %.3g x the bound" % (what, rw, rb)
        pad = torch.cat([w[:rows, cols:].reshape(-1), w[rows:].reshape(-1), b[rows:]])
        assert not bool((pad != 0).any()), what + ": the zero padding is not exact zeros"
        worst = max(worst, rw, rb)

    for f, row in enumerate(F.ft):
        for l, (W, bb, rms) in enumerate(row):
            judge(u.ft[f][l][0], u.ft[f][l][1], W, bb, rms, "FeatTransformer %d layer %d" % (f, l))
    for s, (W, bb, rms) in enumerate(F.att):
        judge(u.att[s][0], u.att[s][1], W, bb, rms, "attentive transformer %d" % s)
    sc, sh, rms0 = F.bn0
    assert TB.ratio((u.bn0[0][:c.D].double() - sc).abs(), TB.g_k(TB.K_FOLD) * sc.abs()) <= 1.0
    assert TB.ratio((u.bn0[1][:c.D].double() - sh).abs(), TB.fold_bias(sh, rms0)) <= 1.0
    assert not bool((u.bn0[0][c.D:] != 0).any()) and not bool((u.bn0[1][c.D:] != 0).any())
    assert torch.equal(u.final, m.final_mapping.weight.detach())
    print(R.case_id(k), "fold: worst error / bound %.3g" % worst)


def test_a_shared_fc_is_folded_with_each_uses_own_batchnorm():
    k = GRID[0]
    c = k[0]
    m, _, _, blob, nb, _ = _case(k)
    u = A.unpack(c, blob, nb)
    copies = [u.ft[f][0][0] for f in range(c.n_steps + 1)]
    for f in range(c.n_steps):
        assert not torch.equal(copies[f], copies[f + 1]), "FeatTransformers %d and %d hold the same fold of the shared fc" % (f, f + 1)


def test_a_gamma_of_zero_folds_to_exact_zeros():
    c = R.cfg(D=5, n_d=16, n_a=16, n_steps=1)
    with torch.no_grad():
        m = R.build(c, "tn0.")
        lay = m.encoder.feat_transformers[0].shared.glu_layers[0]
        lay.bn.bn.weight[3] = 0.0
        m.encoder.att_transformers[0].bn.bn.weight[1] = 0.0
        blob, nb = A.prepare(c, A.to_dev(m))
    u = A.unpack(c, blob, nb)
    w, b = u.ft[1][0]
    assert not bool((w[3] != 0).any()) and float(b[3]) == float(lay.bn.bn.bias.detach()[3])
    assert bool((w[2] != 0).any())
    assert not bool((u.att[0][0][1] != 0).any())


# ---- the forward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", GRID, ids=IDS)
def test_every_output_element_is_within_its_float64_bound(k):
    c, B, seed = k
    got = _case(k)[5]
    r, b = _ref(k)
    rr = TB.ratios(got, r, b)
    print(R.case_id(k), "error / bound:", {n: "%.3g" % v for n, v in rr.items()})
    assert set(rr) == {"out", "masks", "m_explain", "row_entropy"}
    for name, v in rr.items():
        assert v <= 1.0, "%s: error %.3g x its bound" % (name, v)
    mk = got["masks"].cpu()
    assert float(mk.min()) >= 0.0
    # exact zeros: outside the support, beyond the bound, the kernel stores 0.0 and nothing else
    zero, pos = TB.certain(r, b)
    assert not bool((mk[zero] != 0).any()), "a mask entry that float64 puts outside the support beyond the bound is not 0.0"
    assert bool((mk[pos] > 0).all()), "a mask entry that float64 puts inside the support beyond the bound is not positive"
    if c.D >= 5:
        for s in range(c.n_steps):
            assert int(zero[s].sum()) >= 1 and int(pos[s].sum()) >= 1, "step %d has no certain zero / positive" % s


def test_the_short_chain_is_within_the_bounds_without_taking_its_masks_as_given():
    """one step, two layers per FeatTransformer: there the plain propagation from x to every output still says something"""
    k = GRID[1]
    c = k[0]
    m, x, _, _, _, got = _case(k)
    with torch.no_grad():
        r = R.reference(c, m, x)
        b = TB.Forward(c, r)
    rr = TB.ratios(got, r, b)
    print(R.case_id(k), "unforced error / bound:", {n: "%.3g" % v for n, v in rr.items()})
    assert float(b.out.max()) < 1e-2 and max(rr.values()) <= 1.0, rr


def test_rows_with_equal_features_and_with_one_dominant_feature():
    """rows 1 and 2 of every case (tabnet_infer_ref.inputs); their elements are judged by the bound test -- here their masks are
    on the simplex as far as the element bounds allow"""
    for k in GRID:
        c, B, _ = k
        if B < 3:
            continue
        x, mk = _case(k)[1], _case(k)[5]["masks"].cpu().double()
        assert float(x[1].max() - x[1].min()) == 0.0 and float(x[2].abs().max()) == 6.0
        b = _ref(k)[1]
        assert bool(((mk[:, 1:3].sum(-1) - 1).abs() <= b.masks[:, 1:3].sum(-1)).all()), R.case_id(k)


# ---- bit identities -----------------------------------------------------------------------------------------------------
BITS = [GRID[0], GRID[2], GRID[3]]


@pytest.mark.parametrize("k", BITS, ids=[R.case_id(k) for k in BITS])
def test_a_rows_bits_depend_on_neither_the_batch_nor_its_place_in_a_tile(k):
    c, B, _ = k
    _, _, xd, blob, nb, full = _case(k)
    again = A.forward(c, blob, nb, xd)
    for name in full:
        assert torch.equal(full[name], again[name]), name + ": two identical calls differ"
    for r in (0, 15, 16, B - 1):                       # a row alone (B = 1) is that row of the batch
        one = A.forward(c, blob, nb, xd[r:r + 1].contiguous())
        assert torch.equal(one["out"], full["out"][r:r + 1]), "row %d alone differs from row %d of %d" % (r, r, B)
        assert torch.equal(one["masks"], full["masks"][:, r:r + 1]) and torch.equal(one["m_explain"], full["m_explain"][r:r + 1])
        assert torch.equal(one["row_entropy"], full["row_entropy"][r:r + 1])
    part = A.forward(c, blob, nb, xd[5:B - 3].contiguous())   # the same rows at other lanes, in other waves
    for name in ("out", "m_explain", "row_entropy"):
        assert torch.equal(part[name], full[name][5:B - 3]), name + ": a row's bits depend on its place in a tile"
    assert torch.equal(part["masks"], full["masks"][:, 5:B - 3])


@pytest.mark.parametrize("k", BITS, ids=[R.case_id(k) for k in BITS])
def test_out_has_the_same_bits_whichever_optional_outputs_are_requested(k):
    c = k[0]
    _, _, xd, blob, nb, full = _case(k)
    for want in ((), ("masks",), ("m_explain",), ("row_entropy",), ("m_explain", "row_entropy")):
        got = A.forward(c, blob, nb, xd, want=want)      # the absent outputs are null pointers; the sentinels are checked there
        assert torch.equal(got["out"], full["out"]), "out differs when %s is requested" % (want,)
        for name in want:
            assert torch.equal(got[name], full[name]), name
        assert all(got[name] is None for name in A.OPTIONAL if name not in want)
