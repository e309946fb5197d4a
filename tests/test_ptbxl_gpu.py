"""PTB-XL trainer on the device: ``ecgmm_signal_preprocess_i16`` against the reference's own function (golden g10) and, live,
against its scipy restatement; ``ecgmm_weighted_sample`` by exactness given the uniform each draw used, plus the distribution;
the dataset / weighted loader against the reference's ``__getitem__``; both entry points.

The bar of every pre-processing comparison is the project's own for this pipeline, 3e-6 * max(1, max|ref|)
(tests/test_preprocess_gpu.py).  The C entry points are called with NaN-filled outputs between sentinel zones
(tests/lstm_abi.py), and every call ends by checking the sentinels."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy.signal import butter

from ecgmm import evaluation_signal as ES
from ecgmm import preprocess as PP
from ecgmm import train_signal_only_ptb as TS
from ecgmm.config import Config
from ecgmm.hip import functional as HF
from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from ecgmm.signal_model import ResNet1D_SE
from oracle import ref_models as O

from . import lstm_abi
from . import ptbxl_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bar(ref):
    return 3e-6 * max(1.0, float(np.abs(ref).max()))


def _dbl(v):
    return (C.c_double * len(v))(*[float(t) for t in v])


def run_i16(d, chan, gain, base, step, out_len, order=5, window=200, expect_error=None):
    """the C entry point on frames d [R, T, nsig]; gain / base [R, nsig] (the channel columns are picked here).  The output is
    NaN-prefilled between sentinel zones.  -> fp32 numpy [R, nc, out_len]; or, with expect_error, asserts the refusal and that
    nothing was written at all."""
    R, T, nsig = d.shape
    nc = len(chan)
    cols = [c if 0 <= c < nsig else 0 for c in chan]
    raw = torch.from_numpy(np.ascontiguousarray(d)).to(DEV)
    g = torch.from_numpy(np.ascontiguousarray(gain[:, cols], dtype=np.float64)).to(DEV)
    bl = torch.from_numpy(np.ascontiguousarray(base[:, cols]).astype(np.int32)).to(DEV)
    b, a = PP.butter_lowpass(order, 40 / 125)
    zi = PP.lfilter_zi(b, a)
    ar = lstm_abi.Arena({"out": (R, nc, out_len)})
    rc = L.lib().ecgmm_signal_preprocess_i16(ptr(raw), R, T, nsig, (C.c_int * nc)(*chan), nc, ptr(g), ptr(bl), step,
                                             ptr(ar.views["out"]), out_len, window, _dbl(b), _dbl(a), _dbl(zi), order, stream())
    torch.cuda.synchronize()
    assert not ar.touched(), "written outside the output, next to: %s" % ar.touched()
    if expect_error is not None:
        assert rc == 1 and expect_error in L.lib().ecgmm_last_error(), (rc, L.lib().ecgmm_last_error())
        assert bool(torch.isnan(ar.views["out"]).all()), "a refused call wrote to its output"
        return None
    L.check(rc, "signal_preprocess_i16")
    return ar.views["out"].cpu().numpy()


def restated(d, chan, gain, base, step, out_len, order=5):
    out = np.empty((d.shape[0], len(chan), out_len))
    for r in range(d.shape[0]):
        for k, c in enumerate(chan):
            p = (d[r, :, c].astype(np.float64) - base[r, c]) / gain[r, c]
            out[r, k] = U.reference_item(p, out_len, step, order)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# preprocess_i16
# ---------------------------------------------------------------------------------------------------------------------
def test_matches_the_reference_function_golden(golden_dir):
    g = np.load(f"{golden_dir}/g10_ptbxl_preprocess.npz")
    lead = int(g["lead"])
    y = run_i16(g["frames"], [lead], g["gain"], g["baseline"], 2, 2476)
    assert y.dtype == np.float32 and y.shape == (4, 1, 2476)
    err = np.abs(y[:, 0].astype(np.float64) - g["y"]).max()
    ys = run_i16(g["frames_short"], [lead], g["gain_short"], g["baseline_short"], 2, 2476)
    errs = np.abs(ys[:, 0].astype(np.float64) - g["y_short"]).max()
    print(f"g10: max |diff| {err:.3g} (bar {bar(g['y']):.3g}); pad branch {errs:.3g} (bar {bar(g['y_short']):.3g})")
    assert err < bar(g["y"]) and errs < bar(g["y_short"])
    assert (ys[0, 0, 750:] == 0).all() and not np.signbit(ys[0, 0, 750:]).any()          # exact +0.0 behind the record
    # the host wrapper is the same launch
    w = PP.preprocess_i16(torch.from_numpy(g["frames"]).to(DEV), [lead], g["gain"][:, [lead]], g["baseline"][:, [lead]],
                          step=2, out_len=2476)
    assert np.array_equal(w.cpu().numpy(), y)


CASES = [  # R, T, nsig, chan, step, out_len, order
    (1, 5000, 12, [1], 2, 2476, 5),                    # the real shape
    (3, 1001, 3, [2, 0], 2, 501, 5),                   # odd T, reordered channels
    (2, 402, 1, [0], 2, 201, 5),                       # shortest legal: Lf = window + 1
    (2, 700, 2, [1], 2, 512, 5),                       # pad branch
    (5, 777, 12, list(range(12)), 1, 600, 5),          # no decimation, every channel, crop
    (5, 777, 12, list(range(12)), 1, 600, 3),          # ... and another instantiation
    (1, 9933, 1, [0], 1, 9933, 5),                     # the longest row that is accepted at order 5
]


@pytest.mark.parametrize("R,T,nsig,chan,step,out_len,order", CASES)
def test_matches_scipy_restatement_live(R, T, nsig, chan, step, out_len, order):
    d, gain, base = U.make_frames(T + R, R, T, nsig)
    ref = restated(d, chan, gain, base, step, out_len, order)
    y = run_i16(d, chan, gain, base, step, out_len, order)
    Lf = -(-T // step)
    err = np.abs(y.astype(np.float64) - ref).max()
    print(f"i16 R={R} T={T} nsig={nsig} chan={chan} step={step} out_len={out_len} order={order}: max |diff| {err:.3g} "
          f"(bar {bar(ref):.3g})")
    assert np.isfinite(y).all() and err < bar(ref)
    if out_len > Lf:
        tail = y[:, :, Lf:]
        assert (tail == 0).all() and not np.signbit(tail).any()


def test_crop_is_a_prefix():
    d, gain, base = U.make_frames(77, 2, 5000, 12)
    full = run_i16(d, [1, 4], gain, base, 2, 2500)
    crop = run_i16(d, [1, 4], gain, base, 2, 2476)
    assert np.array_equal(crop, full[:, :, :2476])


def test_invalid_sample_poisons_its_own_row_only():
    d, gain, base = U.make_frames(78, 3, 1200, 4)
    clean = run_i16(d, [3, 1], gain, base, 2, 600)
    d2 = d.copy()
    d2[1, 2 * 311, 3] = -32768                 # a frame the decimation keeps, of a channel the call reads
    d2[2, 2 * 100 + 1, 1] = -32768             # a frame the decimation skips: never read
    d2[0, 2 * 50, 2] = -32768                  # a channel the call does not read
    y = run_i16(d2, [3, 1], gain, base, 2, 600)
    assert np.isnan(y[1, 0]).all()
    mask = np.ones((3, 2), dtype=bool)
    mask[1, 0] = False
    assert np.array_equal(y[mask], clean[mask]) and np.isfinite(clean).all()


def test_refusals_launch_nothing():
    d, gain, base = U.make_frames(79, 1, 600, 2)
    run_i16(d, [2], gain, base, 2, 300, expect_error=b"channel")
    run_i16(d, [0, -1], gain, base, 2, 300, expect_error=b"channel")
    run_i16(d[:, :398], [0], gain, base, 2, 199, expect_error=b"window")                    # Lf = 199 < 200
    big = np.zeros((1, 9934, 1), dtype=np.int16)
    run_i16(big, [0], gain, base, 1, 64, expect_error=b"LDS")                               # Lf = 9934 at order 5
    with pytest.raises(RuntimeError, match="channel"):
        PP.preprocess_i16(torch.from_numpy(d).to(DEV), [5], gain[:, :1], base[:, :1])
    with pytest.raises(ValueError, match="int16"):
        PP.preprocess_i16(torch.zeros(1, 600, 2, device=DEV), [0], gain[:, :1], base[:, :1])


# ---------------------------------------------------------------------------------------------------------------------
# weighted_sample
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 64


def run_sampler(weights, count, seed=1234, offset=0, uniforms=True):
    """the C entry point with NaN / -1 prefilled outputs between sentinel zones -> (int64 indices, float64 uniforms, cdf)"""
    cdf, last = PP.weight_cdf(weights)
    cdf_d = torch.from_numpy(cdf).to(DEV)
    ibuf = torch.full((count + 2 * GUARD,), -777, dtype=torch.int64, device=DEV)
    ubuf = torch.full((count + 2 * GUARD,), -777.0, dtype=torch.float64, device=DEV)
    ibuf[GUARD:GUARD + count] = -1
    ubuf[GUARD:GUARD + count] = float("nan")
    out, u = ibuf[GUARD:GUARD + count], ubuf[GUARD:GUARD + count]
    L.check(L.lib().ecgmm_weighted_sample(ptr(cdf_d), len(cdf), last, ptr(out), ptr(u) if uniforms else None, count, seed, offset,
                                          stream()), "weighted_sample")
    torch.cuda.synchronize()
    for buf in (ibuf, ubuf):
        assert bool((buf[:GUARD] == -777).all()) and bool((buf[GUARD + count:] == -777).all()), "written outside an output"
    if not uniforms:
        assert bool(torch.isnan(u).all())
    return out.cpu().numpy(), u.cpu().numpy(), cdf


@pytest.fixture(scope="module")
def draws():
    labels = np.array([0] * 900 + [1] * 100)
    labels = labels[np.random.RandomState(3).permutation(1000)]
    w = TS.class_weights(labels)
    out, u, cdf = run_sampler(w, 4096)
    return labels, w, out, u, cdf


def test_every_draw_is_the_search_of_its_uniform(draws):
    labels, w, out, u, cdf = draws
    assert out.dtype == np.int64 and u.dtype == np.float64
    assert (out >= 0).all() and (out < 1000).all() and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(out, np.searchsorted(cdf, u * cdf[-1], "right"))          # every draw, no exceptions


def test_distribution(draws):
    labels, w, out, u, cdf = draws
    share = labels[out].mean()
    print(f"class-1 share {share:.4f}, mean u {u.mean():.4f}, distinct indices {len(np.unique(out))}")
    assert abs(share - 0.5) < 5 * np.sqrt(0.25 / 4096)
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / (12 * 4096))
    assert len(np.unique(u)) == 4096


def test_determinism_and_independence_of_count(draws):
    labels, w, out, u, cdf = draws
    again, u2, _ = run_sampler(w, 4096)
    assert np.array_equal(again, out) and np.array_equal(u2, u)
    first, u100, _ = run_sampler(w, 100)
    assert np.array_equal(first, out[:100]) and np.array_equal(u100, u[:100])
    nxt, u_next, _ = run_sampler(w, 4096, offset=1)
    assert not np.array_equal(nxt, out) and not np.array_equal(u_next, u)
    other, _, _ = run_sampler(w, 4096, seed=1235)
    assert not np.array_equal(other, out)
    no_u, _, _ = run_sampler(w, 300, uniforms=False)                                   # the uniforms are optional
    assert np.array_equal(no_u, out[:300])


def test_zero_weights_are_never_drawn():
    w = np.ones(40)
    w[17] = 0.0            # interior
    w[0] = 0.0             # first
    w[33:] = 0.0           # trailing
    out, u, cdf = run_sampler(w, 4096, seed=9)
    assert np.array_equal(out, np.searchsorted(cdf, u * cdf[-1], "right"))
    assert (w[out] > 0).all() and out.max() == 32 and out.min() == 1
    assert set(out.tolist()) == set(np.nonzero(w)[0].tolist())                         # 31 items, 4096 draws: all of them appear
    one, _, _ = run_sampler([2.5], 257)
    assert (one == 0).all()


def test_sampler_class_advances_the_stream():
    labels = np.array([0] * 90 + [1] * 10)
    s = TS.DeviceWeightedSampler(TS.class_weights(labels), 100, device=DEV)
    HF.manual_seed(7)
    a, b = s.sample().cpu().numpy(), s.sample().cpu().numpy()
    HF.manual_seed(7)
    a2, ua = s.sample(return_uniforms=True)
    assert np.array_equal(a, a2.cpu().numpy()) and not np.array_equal(a, b)
    assert np.array_equal(a, np.searchsorted(s.cdf_host, ua.cpu().numpy() * s.cdf_host[-1], "right"))
    pinned = s.sample(seed_offset=(7, 1)).cpu().numpy()
    assert np.array_equal(pinned, b)


# ---------------------------------------------------------------------------------------------------------------------
# dataset + loader
# ---------------------------------------------------------------------------------------------------------------------
def _config(root, **kw):
    return type("PtbCfg", (Config,), {"synthetic": False, "ptbxl_dir": str(root), "device": "cuda",
                                      "ptbxl_database": os.path.join(str(root), "ptbxl_database.csv"),
                                      "checkpoint_dir": os.path.join(str(root), "ck"), **kw})


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("ptbxl")
    kept = U.write_tree(str(root), n=24)
    return root, kept


def test_loader_matches_the_reference_pipeline(tree):
    from sklearn.model_selection import train_test_split
    root, kept = tree
    cfg = _config(root)
    records, labels = TS.load_ptbxl(cfg)
    by_path = {rec: k for rec, k in zip(records, kept)}
    X_train, X_temp, y_train, y_temp = train_test_split(records, labels, test_size=0.4, stratify=labels, random_state=42)
    X_val, X_test, y_val, y_test = train_test_split(X_temp, y_temp, test_size=0.5, stratify=y_temp, random_state=42)
    HF.manual_seed(cfg.seed)
    loaders = TS.get_ptbxl_dataloaders(cfg)
    worst = 0.0
    for loader, X, y in zip(loaders, (X_train, X_val, X_test), (y_train, y_val, y_test)):
        ds = loader.dataset
        assert ds.records == X and np.array_equal(ds.labels_host.numpy(), y)            # split membership and labels
        assert ds.signals.shape == (len(X), 1, 2476) and ds.signals.dtype == torch.float32
        ref = np.stack([U.reference_item((by_path[p][0][:, 1].astype(np.float64) - by_path[p][2][1]) / by_path[p][1][1]) for p in X])
        got = ds.signals[:, 0].cpu().numpy().astype(np.float64)
        worst = max(worst, np.abs(got - ref).max())
        assert np.abs(got - ref).max() < bar(ref)
    print(f"dataset rows vs the reference's __getitem__: max |diff| {worst:.3g}")
    short = [i for i, p in enumerate(X_train + X_val + X_test) if by_path[p][0].shape[0] == 3000]
    assert len(short) == 1                                                              # the pad branch is among them
    train = loaders[0]
    n = len(X_train)
    assert (n, len(X_val), len(X_test)) == (14, 5, 5) and len(train) == (n + 15) // 16 and train.sampler is not None
    seen = 0
    for k, (x, yb) in enumerate(train):
        order = train.last_order[k * 16:(k + 1) * 16]
        assert x.shape == (len(order), 1, 2476) and torch.equal(x, train.dataset.signals[order.to(DEV)])     # bit-equal rows
        assert torch.equal(yb.cpu(), train.dataset.labels_host[order])
        seen += x.shape[0]
    assert seen == n and train.last_order.shape == (n,) and int(train.last_order.min()) >= 0 and int(train.last_order.max()) < n
    first = train.last_order.clone()
    for _ in train:
        pass
    assert not torch.equal(first, train.last_order)                                     # the next epoch draws again
    val = loaders[1]
    xs = torch.cat([x for x, _ in val])
    assert torch.equal(val.last_order, torch.arange(len(X_val))) and torch.equal(xs, val.dataset.signals)


def test_twelve_lead_variant(tree):
    root, kept = tree
    recs = [dict(frames=k[0], gain=k[1], baseline=k[2]) for k in kept[4:10]]               # holds the 3000-frame record
    labels = [k[3] for k in kept[4:10]]
    one = TS.PTBXLSignalDataset(recs, labels, device=DEV)
    twelve = TS.PTBXLSignalDataset(recs, labels, leads=range(12), device=DEV, chunk=2)
    assert twelve.signals.shape == (6, 12, 2476) and torch.equal(twelve.signals[:, 1], one.signals[:, 0])
    ref = U.reference_item((kept[7][0][:, 9].astype(np.float64) - kept[7][2][9]) / kept[7][1][9])
    assert np.abs(twelve.signals[3, 9].cpu().numpy() - ref).max() < bar(ref) and (twelve.signals[3, :, 1500:] == 0).all()
    x, y = next(iter(TS.PTBXLLoader(twelve, 4)))
    assert x.shape == (4, 12, 2476) and torch.equal(x, twelve.signals[:4]) and torch.equal(y, twelve.labels[:4])


def test_evaluation_preprocess_signal():
    x = np.random.RandomState(11).randn(3, 2600).cumsum(axis=1) * 0.05
    for Ln in (2600, 1800):
        x32 = x[:, :Ln].astype(np.float32)
        ref = np.stack([U.reference_item(r.astype(np.float64), step=1) for r in x32])
        y = ES.preprocess_signal(torch.from_numpy(x32).to(DEV))
        assert y.shape == (3, 2476) and np.abs(y.cpu().numpy() - ref).max() < bar(ref)
        assert Ln > 2476 or bool((y[:, Ln:] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# entry points
# ---------------------------------------------------------------------------------------------------------------------
def _check_run(history, results, ckpt, epochs):
    assert len(history) == epochs
    assert all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in history)
    assert os.path.basename(os.path.dirname(ckpt)) == "signal" and os.listdir(ckpt) == ["best.pth"]
    assert all(np.isfinite(results[k]) for k in ("accuracy", "f1", "threshold")) and "AF" in results["report"]
    sd = torch.load(os.path.join(ckpt, "best.pth"), map_location="cpu")
    O.ResNet1D_SE(1, 2).load_state_dict(sd, strict=True)                  # same keys and shapes as the reference's class
    return sd


def test_entry_points_train_on_a_data_tree(tree, tmp_path, monkeypatch):
    import csv
    from ecgmm.inference import Predictor
    monkeypatch.chdir(tmp_path)
    root, kept = tree
    cfg = _config(root, checkpoint_dir=str(tmp_path / "ck"))
    history, results, ckpt = TS.main(cfg, num_epochs=2, quiet=True)
    sd = _check_run(history, results, ckpt, 2)
    model = ResNet1D_SE(compute_dtype="fp32")
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    x = TS.PTBXLSignalDataset([dict(frames=k[0], gain=k[1], baseline=k[2]) for k in kept[:8]], [k[3] for k in kept[:8]],
                              device=DEV).signals
    with torch.no_grad():
        want = model(x)
    got = Predictor(model)(x)
    assert (got - want).abs().max() < 1e-3 * max(1.0, float(want.abs().max()))   # the inference tests' fp32 bar
    # evaluation_signal.main on a written labels + signals pair, with that checkpoint
    rng = np.random.RandomState(21)
    with open(tmp_path / "labels.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["index", "label"])
        for i in range(14):
            w.writerow([i, "Borderline" if i == 3 else ("Abnormal" if i % 3 == 0 else "Normal")])
    with open(tmp_path / "ecg_signals.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow([""] + [str(t) for t in range(2600)])
        for i in range(1, 16):                                            # index 0 has no signal, 14 and 15 no label
            w.writerow([i] + [f"{v:.6f}" for v in rng.randn(2600).cumsum() * 0.05])
    ecfg = _config(root, label_file=str(tmp_path / "labels.csv"), ecg_csv=str(tmp_path / "ecg_signals.csv"), compute_dtype="fp32")
    loader = ES.get_digitized_test_loader(ecfg)
    assert len(loader.dataset) == 12 and loader.batch_size == 8 and loader.dataset.signals.shape == (12, 1, 2476)
    assert loader.dataset.labels_host.tolist() == [int(i % 3 == 0) for i in range(1, 14) if i != 3]
    res = ES.main(os.path.join(ckpt, "best.pth"), ecfg, quiet=True)
    assert all(np.isfinite(res[k]) for k in ("auc", "f1", "accuracy", "threshold")) and "Abnormal" in res["report"]
    res_p = ES.main(os.path.join(ckpt, "best.pth"), ecfg, quiet=True, use_predictor=True)
    assert all(np.isfinite(res_p[k]) for k in ("auc", "f1", "accuracy"))


def test_entry_point_runs_without_data(tmp_path, monkeypatch):
    """Config.synthetic: generated twelve-lead int16 records; validation and test through the Predictor"""
    monkeypatch.chdir(tmp_path)
    cfg = type("Synth", (Config,), {"synthetic": True, "synthetic_train_size": 24, "synthetic_val_size": 8,
                                    "synthetic_test_size": 8, "device": "cuda", "checkpoint_dir": str(tmp_path / "ck")})
    from ecgmm.inference import Predictor
    history, results, ckpt = TS.main(cfg, num_epochs=2, quiet=True, use_predictor=True)
    sd = _check_run(history, results, ckpt, 2)
    model = ResNet1D_SE(compute_dtype="fp32")
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    records, labels = TS.load_ptbxl(cfg)
    x = TS.PTBXLSignalDataset(records[:8], labels[:8], device=DEV).signals
    with torch.no_grad():
        want = model(x)
    got = Predictor(model)(x)
    assert (got - want).abs().max() < 1e-3 * max(1.0, float(want.abs().max()))   # the inference tests' fp32 bar
