"""CPU-side checks of TabNet's fused eval forward (csrc/tabnet_infer.hip, ecgmm.tabnet.forward_masks,
ecgmm.inference._TabNetPlan): the float64 reference of tests/tabnet_infer_ref.py is the oracle's own eval forward, its masks are
on the simplex and its M_explain is the definition; the bounds of tests/tabnet_infer_bounds.py accept the kernel's restatement
evaluated by torch in fp32 and reject named slips; ABI agreement, the size query and the refusals without a device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from ecgmm.hip import lib as L

from . import tabnet_infer_bounds as TB
from . import tabnet_infer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ecgmm_tabnet_infer_prepared_bytes", "ecgmm_tabnet_infer_prepare", "ecgmm_tabnet_infer")
GRID = R.grid()
IDS = [R.case_id(k) for k in GRID]
KEYS = ("out", "masks", "m_explain", "row_entropy")

# the slip -> the output that must leave its bound
SLIP_SHOWS_IN = dict(shared_bn_of_another_use="out", no_sqrt_half="out", prior_never_updated="masks", previous_mask="out",
                     mask_on_raw_x="out", importance_without_relu="m_explain", m_explain_plain_sum="m_explain",
                     padded_features_counted="masks")
SLIP_CASES = [GRID[0], GRID[2]]     # both have shared layers, several steps and a D that is no multiple of 16

_cache = {}


def _model(k):
    c, B, seed = k
    key = R.case_id(k)
    if key not in _cache:
        with torch.no_grad():
            m = R.build(c)
            x = R.inputs(B, c.D, seed)
            _cache[key] = (m, x, R.reference(c, m, x))
    return _cache[key]


def _outputs(rec):
    return dict(out=rec.out, masks=rec.masks, m_explain=rec.m_explain, row_entropy=rec.row_entropy)


def _judge(k, slip=None):
    """ratios of the fp32 restatement (with a slip) against the float64 reference forced with the restatement's own masks"""
    c, B, seed = k
    m, x, _ = _model(k)
    with torch.no_grad():
        cand = R.candidate(c, m, x, slip)
        r = R.reference(c, m, x, forced=cand.masks)
        return TB.ratios(_outputs(cand), r, TB.Forward(c, r))


def _err():
    return L.lib().ecgmm_last_error().decode()


# ---- the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", GRID, ids=IDS)
def test_reference_is_the_oracles_eval_forward_in_float64(k):
    c, B, seed = k
    m, x, r = _model(k)
    out, m_loss = R.unfolded_out(m, x)
    assert float((out - r.out).abs().max()) <= 1e-12 * max(1.0, float(out.abs().max()))
    assert abs(float(m_loss) - float(r.row_entropy.mean()) / c.n_steps) <= 1e-12
    assert r.out.dtype == torch.float64 and r.masks.shape == (c.n_steps, B, c.D)


@pytest.mark.parametrize("k", GRID, ids=IDS)
def test_reference_masks_are_on_the_simplex_and_m_explain_is_its_definition(k):
    c, B, seed = k
    _, _, r = _model(k)
    assert float(r.masks.min()) >= 0.0
    assert float((r.masks.sum(-1) - 1).abs().max()) <= 1e-13
    want = sum(st.M * torch.relu(st.d).sum(1, keepdim=True) for st in r.steps)
    assert torch.equal(want, r.m_explain)
    assert torch.equal(sum(st.d for st in r.steps) @ r.final.t(), r.out)
    for st in r.steps:       # tau is the threshold of the support
        assert torch.equal(torch.clamp(st.zp - st.tau, min=0), st.M)


# ---- the bounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", GRID, ids=IDS)
def test_bounds_accept_the_restatement_in_torch_fp32(k):
    rr = _judge(k)
    print(R.case_id(k), "torch fp32 / bound:", {n: "%.3g" % v for n, v in rr.items()})
    assert set(rr) == set(KEYS) and max(rr.values()) <= 1.0, rr


@pytest.mark.parametrize("k", GRID, ids=IDS)
def test_fold_bounds_accept_the_fold_in_torch_fp32(k):
    c, B, seed = k
    m, _, r = _model(k)
    got, worst = R.folds(m, torch.float32), 0.0
    pairs = [(g, w) for gr, wr in zip(got.ft, r.folds.ft) for g, w in zip(gr, wr)] + list(zip(got.att, r.folds.att))
    for (gw, gb, _), (W, b, rms) in pairs:
        worst = max(worst, TB.ratio((gw.double() - W).abs(), TB.fold_weight(W)), TB.ratio((gb.double() - b).abs(), TB.fold_bias(b, rms)))
    assert 0.0 < worst <= 1.0, worst


@pytest.mark.parametrize("slip", R.SLIPS)
@pytest.mark.parametrize("k", SLIP_CASES, ids=[R.case_id(k) for k in SLIP_CASES])
def test_bounds_reject_the_slip(k, slip):
    rr = _judge(k, slip)
    print(R.case_id(k), slip, {n: "%.3g" % v for n, v in rr.items()})
    assert rr[SLIP_SHOWS_IN[slip]] > 1.0, (slip, rr)
    if SLIP_SHOWS_IN[slip] == "m_explain":      # these two touch nothing else
        assert max(rr["out"], rr["masks"], rr["row_entropy"]) <= 1.0, (slip, rr)


def test_unforced_bounds_hold_too_where_they_say_something():
    """without taking the masks as given the same bounds hold, as long as the chain is short enough for them to stay small"""
    k = GRID[1]
    c, B, seed = k
    m, x, r = _model(k)
    with torch.no_grad():
        b = TB.Forward(c, r)
        rr = TB.ratios(_outputs(R.candidate(c, m, x)), r, b)
    assert float(b.out.max()) < 1e-2 and max(rr.values()) <= 1.0, rr


@pytest.mark.parametrize("k", [k for k in GRID if k[0].D >= 5], ids=[R.case_id(k) for k in GRID if k[0].D >= 5])
def test_every_step_has_a_certain_zero_and_a_certain_positive(k):
    """the condition of the exact-zero test on the GPU, for the reference alone (forced with its own masks rounded to fp32)"""
    c, B, seed = k
    m, x, r0 = _model(k)
    with torch.no_grad():
        r = R.reference(c, m, x, forced=r0.masks.float())
        zero, pos = TB.certain(r, TB.Forward(c, r))
    for s in range(c.n_steps):
        assert int(zero[s].sum()) >= 1 and int(pos[s].sum()) >= 1, (s, int(zero[s].sum()), int(pos[s].sum()))
    assert not bool((zero & (r.masks > 0)).any()) and not bool((pos & (r.masks <= 0)).any())


def test_inputs_hold_an_all_equal_row_and_a_dominant_feature_row():
    x = R.inputs(17, 5, 0)
    assert float(x[1].max() - x[1].min()) == 0.0
    assert float(x[2].abs().max()) == 6.0 and float(x[2].abs().sort().values[-2]) < 0.1


# ---- the C ABI without a device -----------------------------------------------------------------------------------------
def desc(D=2, n_d=32, n_a=32, steps=3, shared=2, indep=2, out=32, gamma=1.5, epsilon=1e-15, bn_eps=1e-5):
    return L.TabNetInferDesc(D, n_d, n_a, steps, shared, indep, out, gamma, epsilon, bn_eps)


def test_new_symbols_in_header_table_and_library():
    src = open(os.path.join(ROOT, "include", "ecgmm.h")).read()
    assert "state_dict ORDER" in src        # the header says which order the parameter table has
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ecgmm_[a-z0-9_]+)\s*\(", src))
    h = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared, name + " not declared in include/ecgmm.h"
        assert name in L.SIGNATURES, name + " not in the ctypes table"
        assert hasattr(h, name), name + " not exported"
    fields = re.search(r"typedef struct \{([^}]*)\} ecgmm_tabnet_infer_desc;", src).group(1)
    names = re.findall(r"\b([a-z_]+)\b(?=\s*[,;])", fields)
    assert names == [n for n, _ in L.TabNetInferDesc._fields_]
    assert L.lib().ecgmm_version() == 100


def _floats(D, n_d, n_a, steps, layers, out):
    W, Dp = n_d + n_a, (D + 15) // 16 * 16
    p64 = lambda n: (n + 63) // 64 * 64
    ft = 2 * W * Dp + p64(2 * W) + (layers - 1) * (2 * W * W + p64(2 * W))
    return 128 + (steps + 1) * ft + steps * (Dp * n_a + 64) + out * n_d


@pytest.mark.parametrize("k", GRID, ids=IDS)
def test_the_size_query_needs_no_device_and_holds_one_folded_copy_per_use(k):
    c = k[0]
    lib = L.lib()
    nb = lib.ecgmm_tabnet_infer_prepared_bytes(C.byref(desc(c.D, c.n_d, c.n_a, c.n_steps, c.n_shared, c.n_independent, c.out_dim)))
    assert nb == 4 * _floats(c.D, c.n_d, c.n_a, c.n_steps, c.n_shared + c.n_independent, c.out_dim), _err()
    # a shared fc is folded once per FeatTransformer: sharing does not shrink the blob
    swapped = lib.ecgmm_tabnet_infer_prepared_bytes(C.byref(desc(c.D, c.n_d, c.n_a, c.n_steps, c.n_independent, c.n_shared, c.out_dim)))
    assert swapped == nb
    more = lib.ecgmm_tabnet_infer_prepared_bytes(C.byref(desc(c.D, c.n_d, c.n_a, c.n_steps + 1, c.n_shared, c.n_independent, c.out_dim)))
    assert more > nb


def test_bad_descriptors_zero_the_query_and_name_the_limit():
    lib = L.lib()
    for kw, word in ((dict(D=65), "input_dim=65"), (dict(D=0), "input_dim=0"), (dict(n_d=8), "n_d=8"), (dict(n_a=24), "n_a=24"),
                     (dict(n_d=64, n_a=80), "<= 128"), (dict(steps=9), "n_steps=9"), (dict(steps=0), "n_steps=0"),
                     (dict(shared=0, indep=0), "n_shared=0"), (dict(shared=5, indep=4), "<= 8"), (dict(shared=-1), "n_shared=-1"),
                     (dict(out=40), "out_dim=40"), (dict(out=144), "out_dim=144"), (dict(out=0), "out_dim=0"),
                     (dict(gamma=-1.0), "gamma"), (dict(gamma=float("nan")), "gamma"), (dict(epsilon=-1.0), "epsilon"),
                     (dict(bn_eps=-1.0), "bn_eps")):
        assert lib.ecgmm_tabnet_infer_prepared_bytes(C.byref(desc(**kw))) == 0 and word in _err(), (kw, _err())
    assert lib.ecgmm_tabnet_infer_prepared_bytes(None) == 0 and "null" in _err()


def test_null_short_and_misaligned_buffers_are_errors_before_anything_is_written():
    lib = L.lib()
    d = desc()
    buf = C.create_string_buffer(256)
    base = (C.addressof(buf) + 15) // 16 * 16
    p1, odd = C.c_void_p(base), C.c_void_p(base + 4)
    n = 4 + 5 * 4 * 4 + 5 * 3 + 1
    tab = (C.c_void_p * n)(*[p1] * n)
    big = 1 << 40
    assert lib.ecgmm_tabnet_infer_prepare(C.byref(d), None, p1, big, None) == 1 and "null" in _err()
    assert lib.ecgmm_tabnet_infer_prepare(C.byref(d), tab, None, 0, None) == 3 and "blob" in _err()
    assert lib.ecgmm_tabnet_infer_prepare(C.byref(d), tab, p1, 64, None) == 3 and "blob" in _err()
    assert lib.ecgmm_tabnet_infer_prepare(C.byref(d), tab, odd, big, None) == 1 and "aligned" in _err()
    tab[n - 1] = None
    assert lib.ecgmm_tabnet_infer_prepare(C.byref(d), tab, p1, big, None) == 1 and "parameter %d" % (n - 1) in _err()
    assert lib.ecgmm_tabnet_infer_prepare(C.byref(desc(n_d=8)), tab, p1, big, None) == 1 and "n_d=8" in _err()
    run = lambda dd=d, x=p1, B=4, blob=p1, nb=big, out=p1: lib.ecgmm_tabnet_infer(C.byref(dd), x, B, blob, nb, out, None, None, None, None)
    assert run(x=None) == 1 and "null" in _err()
    assert run(out=None) == 1 and "null" in _err()
    assert run(B=0) == 1 and "B=0" in _err()
    assert run(B=1 << 31) == 1 and "B=" in _err()
    assert run(nb=64) == 3 and "blob" in _err()
    assert run(blob=None) == 3 and "blob" in _err()
    assert run(blob=odd) == 1 and "aligned" in _err()
    assert run(dd=desc(D=65)) == 1 and "input_dim=65" in _err()
    assert bytes(buf.raw) == bytes(256)


# ---- Python -------------------------------------------------------------------------------------------------------------
def test_forward_masks_refuses_training_mode_without_changing_it_and_names_the_fused_limits():
    from ecgmm.tabnet import FUSED_LIMITS, ClinicalTabNetEncoder, TabNetNoEmbeddings, fused_refusal
    m = ClinicalTabNetEncoder(2, 32)
    assert m.training
    with pytest.raises(RuntimeError, match="training mode"):
        m.forward_masks(torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="training mode"):
        m.visualize_masks(torch.zeros(4, 2).numpy(), save_dir=os.devnull)
    assert m.training and all(k.training for k in m.modules())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval().forward_masks(torch.zeros(4, 2))
    small = TabNetNoEmbeddings(4, 8, n_d=8, n_a=8).eval()
    with pytest.raises(ValueError, match=r"n_d=8.*multiples of 16"):
        small.forward_masks(torch.zeros(4, 4))
    with pytest.raises(ValueError, match=r"n_d=8.*multiples of 16"):
        small.encoder.forward_masks(torch.zeros(4, 4))
    assert fused_refusal(m.tabnet.encoder, 32) is None and "out" in fused_refusal(m.tabnet.encoder, 40)
    assert "n_d + n_a <= 128" in FUSED_LIMITS


def test_visualize_masks_keeps_the_reference_signature_and_the_model_has_its_wrapper():
    from ecgmm.multimodal import ECGMultimodalModel
    from ecgmm.tabnet import ClinicalTabNetEncoder
    p = inspect.signature(ClinicalTabNetEncoder.visualize_masks).parameters
    assert list(p) == ["self", "X", "feature_names", "save_dir", "base_filename"]
    assert (p["feature_names"].default, p["save_dir"].default, p["base_filename"].default) == (None, "./shap", "mask")
    q = inspect.signature(ECGMultimodalModel.visualize_clinical_masks).parameters
    assert list(q) == ["self", "clinical", "feature_names", "save_dir", "base_filename"]
    assert hasattr(ECGMultimodalModel, "extract_clinical_features")


def test_predictor_takes_the_clinical_encoder_and_keeps_its_eval_mode_message():
    from ecgmm import inference
    from ecgmm.tabnet import ClinicalTabNetEncoder
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.Predictor(ClinicalTabNetEncoder(2, 32).eval())
    with pytest.raises(ValueError, match="n_d=8"):
        inference._TabNetPlan(ClinicalTabNetEncoder(2, 8).eval())
    assert inspect.signature(inference.Predictor.__init__).parameters["clinical_plan"].default in (True, False)
    src = inspect.getsource(inference._MultimodalPlan.__call__)
    assert "Predictor: the clinical branch runs the model's own forward, which is in training mode " in src
    assert "ClinicalTabNetEncoder" in inference.Predictor.__doc__ and "clinical_plan" in inference.Predictor.__doc__
