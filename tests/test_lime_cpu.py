"""Host-side checks of the LIME path (no GPU): the quartile discretiser against direct numpy, the float64 restatement of
the ridge against sklearn, the numpy Philox against the Random123 known answers, the refusals, the workspace query and the
modality rows."""
import numpy as np
import pytest
import torch

from ecgmm import lime_fusion_modal_balance as LF
from ecgmm.hip import functional as HF
from ecgmm.hip import lib as L
from ecgmm.lime_tabular import LimeTabularExplainer, QuartileDiscretizer

from . import lime_ref as R
from .lime_ref import SEED, crafted_background


def direct(col, qs=(25, 50, 75)):
    col = col.astype(np.float64)
    qts = np.unique(np.percentile(col, qs))
    bins = np.searchsorted(qts, col)
    nb = len(qts) + 1
    mean = [col[bins == j].mean() if (bins == j).any() else 0.0 for j in range(nb)]
    std = [(np.std(col[bins == j]) if (bins == j).any() else 0.0) + 1e-11 for j in range(nb)]
    vals, counts = np.unique(bins, return_counts=True)
    return qts, bins, mean, std, [col.min()] + qts.tolist(), qts.tolist() + [col.max()], vals, counts / counts.sum()


def test_quartile_discretizer_matches_direct_numpy():
    bg = crafted_background()
    d = QuartileDiscretizer(bg)
    for f in range(bg.shape[1]):
        qts, bins, mean, std, lo, hi, vals, freq = direct(bg[:, f])
        assert np.array_equal(d.qts[f], qts)
        assert np.array_equal(d.discretize(bg)[:, f], bins)
        assert np.array_equal(d.means[f], mean) and np.array_equal(d.stds[f], std)
        assert np.array_equal(d.mins[f], lo) and np.array_equal(d.maxs[f], hi)
        assert np.array_equal(d.feature_values[f], vals) and np.array_equal(d.feature_frequencies[f], freq)
    assert len(d.qts[0]) == 3 and len(d.qts[1]) == 2                 # ties collapse bins
    # a constant column: its one distinct quantile is the value itself, every row falls in bin 0 and its std is the bare offset
    assert len(d.qts[2]) == 1 and list(d.feature_values[2]) == [0] and d.stds[2][0] == 1e-11 and d.means[2][0] == 0.75
    q = d.qts[3][0]
    assert d.discretize(np.array([[0, 0, 0, q, 0]]))[0, 3] == 0      # exactly on the first quartile: left side
    assert d.discretize(np.array([[0, 0, 0, np.nextafter(q, 99.0), 0]]))[0, 3] == 1
    empty = [j for j in range(len(d.qts[4]) + 1) if d.bin_counts[4][j] == 0]
    assert empty and all(d.means[4][j] == 0.0 and d.stds[4][j] == 1e-11 for j in empty)
    assert all(j not in d.feature_values[4] for j in empty)
    t = d.host_table()
    assert t["cdf"].shape == (5, 4) and np.allclose(t["cdf"][np.arange(5), t["nbins"] - 1], 1.0)
    j = empty[0]
    assert t["cdf"][4, j] == (t["cdf"][4, j - 1] if j else 0.0)       # zero frequency: no mass in the table
    dec = QuartileDiscretizer(bg, qs=(10, 20, 30, 40, 50, 60, 70, 80, 90))
    assert np.array_equal(dec.qts[0], direct(bg[:, 0], (10, 20, 30, 40, 50, 60, 70, 80, 90))[0])


@pytest.mark.parametrize("N,K,bins", [(37, 21, 4), (1000, 768, 4)])
def test_ridge_restatement_matches_sklearn(N, K, bins):
    Z, d2, y = R.ridge_case(N, K, 2, bins, seed=11)
    w = R.kernel_weights(d2, 0.75 * np.sqrt(K))
    for alpha in (1.0, 0.01) if N < 100 else (1.0,):
        ref = R.RidgeRef(Z, w, y, alpha)
        coef, icpt, score = R.sklearn_ridge(Z.astype(np.float64), w, y.astype(np.float64), alpha)
        assert np.abs(ref.beta - coef).max() <= 1e-12 and np.abs(ref.intercept - icpt).max() <= 1e-12
        assert np.abs(ref.score - score).max() <= 1e-10
        assert np.all(ref.beta[:, 1] == 0.0)                          # the all-ones column
    keep, fit = R.explain(Z.astype(np.float64), d2, y[0], 0.75 * np.sqrt(K), 10)
    assert len(keep) == 10 and fit.beta.shape == (1, 10)


def test_numpy_philox_known_answers_and_uniformity():
    kat = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for key, ctr, want in kat:                                        # Random123 kat_vectors, philox4x32 10 rounds
        assert tuple(int(v) for v in R.philox4x32_10(key, ctr)) == want
    # the counters tests/test_lime_ops_gpu.py uses at [1, 1000, 768]: row b0 = 5, offset (7 << 32) | 9; the first 1e5 elements
    n = np.arange(1, 132)[:, None]
    f = np.arange(768)[None, :]
    for u in R.perturb_uniforms(SEED, (7 << 32) | 9, 5, n, f):
        assert u.size >= 100000
        u = np.sort(u.reshape(-1)[:100000])
        assert u.min() >= 0.0 and u.max() < 1.0
        k = np.arange(1, u.size + 1)
        ks = max((k / u.size - u).max(), (u - (k - 1) / u.size).max())
        assert ks * np.sqrt(u.size) < 1.63


def test_refusals_say_what_is_not_implemented():
    bg = crafted_background()
    for kw in (dict(mode="regression"), dict(discretize_continuous=False), dict(sample_around_instance=True),
               dict(feature_selection="forward_selection"), dict(feature_selection="lasso_path"), dict(discretizer="entropy")):
        with pytest.raises(NotImplementedError, match="not implemented"):
            LimeTabularExplainer(bg, **kw)
    ex = LimeTabularExplainer(np.tile(bg, (1, 2)))
    assert ex.kernel_width == pytest.approx(0.75 * np.sqrt(10))
    assert ex.chunk_rows(2, 1 << 40) == 65535 and ex.chunk_rows(1000, 1) == 1      # one launch's limit; never below one row
    assert ex.chunk_rows(1000, 1 << 30) < (1 << 30) // (1000 * 4 * 128)            # predict_fn's hidden layer is counted
    with pytest.raises(ValueError, match="outside"):
        ex.explain_batch(torch.zeros(2, 10), lambda x: x, first_index=(1 << 18) - 1)
    row = torch.zeros(10)
    with pytest.raises(NotImplementedError, match="num_features <= 6"):
        ex.explain_instance(row, lambda x: x, num_features=6)
    with pytest.raises(NotImplementedError, match="top_labels"):
        ex.explain_instance(row, lambda x: x, top_labels=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ex.explain_instance(row, lambda x: x, num_features=10, num_samples=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.lime_perturb(torch.zeros(1, 10), ex.discretizer.table("cpu"), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.lime_ridge(torch.zeros(1, 4, 3, dtype=torch.uint8), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 1, 4), 1.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.lime_prob(torch.zeros(2, 2), 1)


def test_ridge_workspace_query_runs_without_a_gpu():
    q = L.lib().ecgmm_lime_ridge_workspace
    base = q(2, 100, 64)
    assert base >= 2 * 64 * 64 * 4
    assert q(3, 100, 64) > base and q(2, 101, 64) >= base and q(2, 1000, 64) > base and q(2, 100, 65) > base
    sizes = [q(4, 1000, d) for d in (1, 31, 32, 33, 64, 500, 768, 1024)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert [q(b, 1000, 768) for b in (1, 2, 64)] == sorted(q(b, 1000, 768) for b in (1, 2, 64))
    assert q(1, 10, 1100) == q(1, 10, 1024) == q(1, 10, 4096) > 0        # a fit keeps at most 1024 columns of a wider D
    for bad in ((0, 10, 10), (1, 0, 10), (1, 10, 0), (-1, 10, 10), (1, 10, 4097)):
        assert q(*bad) == 0
        assert b"lime_ridge_workspace" in L.lib().ecgmm_last_error()


def test_modality_rows():
    exp = [(0, 0.5), (1, -0.5), (2, 1.0), (3, -2.0), (4, 0.25), (5, 0.25), (6, -0.5)]
    row = LF.modality_row(exp, (2, 1, 4), label=1, sample_id=3)       # unequal blocks: [0, 2), [2, 3), [3, 7)
    assert row["Sample_ID"] == 3 and row["Label"] == 1
    assert row["Image_%"] == pytest.approx(20.0) and row["Signal_%"] == pytest.approx(20.0)
    assert row["Clinical_%"] == pytest.approx(60.0)
    assert row["Image_%"] + row["Signal_%"] + row["Clinical_%"] == pytest.approx(100.0)
    zero = LF.modality_row([(i, 0.0) for i in range(7)], (2, 1, 4), 0, 1)
    assert zero["Image_%"] == 0 and zero["Signal_%"] == 0 and zero["Clinical_%"] == 0
    part = LF.modality_row([(6, 1.0)], (2, 1, 4), 0, 1)               # a feature that was not kept counts as 0
    assert part["Clinical_%"] == pytest.approx(100.0) and part["Image_%"] == 0
