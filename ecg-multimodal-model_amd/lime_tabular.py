"""LIME for tabular data on the HIP ops (reference: lime_fusion_modal_balance.py:118-160 calls
``lime.lime_tabular.LimeTabularExplainer(training_data, feature_names, class_names, mode='classification')`` and
``explain_instance(row, predict_fn, num_features=768, num_samples=1000)``).

lime is not a dependency here (as shap is not, see shap_fusion_modal_balance.py), so this module restates lime 0.2.x with the
defaults that call hits: the quartile discretiser, perturbation in the discretised space with the instance as row 0, the
exponential kernel of width 0.75 sqrt(D) on the Euclidean distance of the binary rows, ``feature_selection='auto'`` and
``Ridge(alpha=1, fit_intercept=True)`` with the kernel weights as ``sample_weight``.  The discretiser is host float64 work done
once per background; perturbation and the fit run in csrc/lime.hip for a whole batch of rows (``explain_batch``).
lime's own random stream (numpy's) is not reproduced: draws come from the library's Philox stream, see DESIGN.md section 21.
"""
import numpy as np
import torch

from .hip import functional as HF

QUANTILES = {"quartile": (25, 50, 75), "decile": (10, 20, 30, 40, 50, 60, 70, 80, 90)}
STD_OFFSET = 1e-11


def _host64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


class QuartileDiscretizer:
    """lime.discretize.QuartileDiscretizer (``qs`` = the percentiles; DecileDiscretizer differs in nothing else).

    Per feature f: ``qts[f]`` the distinct percentiles, ``bin(x) = np.searchsorted(qts, x)`` in 0 .. len(qts), and per bin
    over the background values that fall in it ``means`` (0 when empty), ``stds`` (np.std + 1e-11), ``mins`` =
    [column min] + qts, ``maxs`` = qts + [column max]; ``feature_values[f]`` the bins that occur, sorted, and
    ``feature_frequencies[f]`` their relative counts."""

    def __init__(self, data, qs=QUANTILES["quartile"]):
        data = _host64(data)
        if data.ndim != 2 or data.shape[0] < 1 or data.shape[1] < 1:
            raise ValueError(f"the background must be [M, D], got {data.shape}")
        if not np.isfinite(data).all():
            raise ValueError("the background holds NaN / inf")
        self.qs = tuple(qs)
        self.num_features = data.shape[1]
        self.qts, self.means, self.stds, self.mins, self.maxs = [], [], [], [], []
        self.feature_values, self.feature_frequencies, self.bin_counts = [], [], []
        for f in range(self.num_features):
            col = data[:, f]
            qts = np.unique(np.percentile(col, self.qs))
            bins = np.searchsorted(qts, col)
            nb = len(qts) + 1
            counts = np.bincount(bins, minlength=nb)
            means, stds = np.zeros(nb), np.zeros(nb)
            for j in range(nb):
                sel = col[bins == j]
                means[j] = sel.mean() if len(sel) else 0.0
                stds[j] = (sel.std() if len(sel) else 0.0) + STD_OFFSET
            self.qts.append(qts)
            self.means.append(means)
            self.stds.append(stds)
            self.mins.append(np.concatenate([[col.min()], qts]))
            self.maxs.append(np.concatenate([qts, [col.max()]]))
            self.bin_counts.append(counts)
            self.feature_values.append(np.flatnonzero(counts))
            self.feature_frequencies.append(counts[counts > 0] / counts.sum())
        self.max_bins = max(len(q) + 1 for q in self.qts)

    def discretize(self, rows):
        rows = _host64(rows)
        single = rows.ndim == 1
        rows = np.atleast_2d(rows)
        out = np.stack([np.searchsorted(self.qts[f], rows[:, f]) for f in range(self.num_features)], axis=1)
        return out[0] if single else out

    def names(self, feature_names, bins):
        """lime's discretised feature names for the bins of one row"""
        out = []
        for f, j in enumerate(bins):
            n, q = feature_names[f], self.qts[f]
            if len(q) == 0:
                out.append(n)
            elif j == 0:
                out.append("%s <= %.2f" % (n, q[0]))
            elif j == len(q):
                out.append("%s > %.2f" % (n, q[-1]))
            else:
                out.append("%.2f < %s <= %.2f" % (q[j - 1], n, q[j]))
        return out

    def host_table(self):
        """the table ecgmm_lime_perturb reads, as numpy arrays padded to S = max_bins (see include/ecgmm.h)"""
        D, S = self.num_features, self.max_bins
        qts, cdf, stats = np.zeros((D, S)), np.zeros((D, S)), np.zeros((4, D, S))
        nbins = np.zeros(D, dtype=np.int32)
        for f in range(D):
            nb = len(self.qts[f]) + 1
            nbins[f] = nb
            qts[f, :nb - 1] = self.qts[f]
            c = np.cumsum(self.bin_counts[f] / self.bin_counts[f].sum())
            cdf[f, :nb], cdf[f, nb:] = c, c[-1]
            for i, v in enumerate((self.means[f], self.stds[f], self.mins[f], self.maxs[f])):
                stats[i, f, :nb] = v
            stats[1, f, nb:] = STD_OFFSET
        return {"qts": qts, "cdf": cdf, "stats": stats, "lim": stats[2:4].astype(np.float32), "nbins": nbins}

    def table(self, device):
        return {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in self.host_table().items()}


class Explanation:
    """what lime's Explanation carries for the reference's use: ``local_exp[label]`` = (feature, weight) pairs sorted by
    |weight| descending, ``intercept[label]``, ``score[label]`` (weighted R^2), ``local_pred[label]``"""

    def __init__(self, feature_names, class_names=None):
        self.domain_feature_names = feature_names
        self.class_names = class_names
        self.local_exp, self.intercept, self.score, self.local_pred = {}, {}, {}, {}

    def available_labels(self):
        return sorted(self.local_exp)

    def as_map(self):
        return self.local_exp

    def as_list(self, label=1):
        return [(self.domain_feature_names[f], w) for f, w in self.local_exp[label]]


def _refuse(what):
    raise NotImplementedError(what + " is not implemented by ecgmm.lime_tabular (only the path lime_fusion_modal_balance.py "
                              "takes: classification, quartile / decile discretiser, highest_weights selection)")


class LimeTabularExplainer:
    def __init__(self, training_data, feature_names=None, class_names=None, mode="classification", kernel_width=None,
                 discretize_continuous=True, discretizer="quartile", feature_selection="auto", random_state=None,
                 sample_around_instance=False, categorical_features=None):
        if mode != "classification":
            _refuse(f"mode={mode!r}")
        if not discretize_continuous:
            _refuse("discretize_continuous=False")
        if sample_around_instance:
            _refuse("sample_around_instance=True")
        if categorical_features:
            _refuse("categorical_features")
        if discretizer not in QUANTILES:
            _refuse(f"discretizer={discretizer!r}")
        if feature_selection not in ("auto", "highest_weights", "none"):
            _refuse(f"feature_selection={feature_selection!r}")
        self.discretizer = QuartileDiscretizer(training_data, QUANTILES[discretizer])
        D = self.discretizer.num_features
        self.feature_names = [str(i) for i in range(D)] if feature_names is None else list(feature_names)
        if len(self.feature_names) != D:
            raise ValueError(f"{len(self.feature_names)} feature names for {D} features")
        self.class_names = class_names
        self.feature_selection = feature_selection
        self.kernel_width = float(np.sqrt(D) * 0.75 if kernel_width is None else kernel_width)
        # random_state: an integer seeds a Philox stream of this explainer's own; None takes offsets of the library's
        self._seed = None if random_state is None else int(random_state)
        self._offset = 0
        self._tables = {}

    def _take(self):
        if self._seed is None:
            return HF._PhiloxState.take(4)
        off = self._offset
        self._offset += 1
        return self._seed, off

    def _table(self, device):
        key = str(device)
        if key not in self._tables:
            self._tables[key] = self.discretizer.table(device)
        return self._tables[key]

    MAX_CHUNK = 65535              # ecgmm_lime_ridge: one grid row per sample
    MAX_ROWS = 1 << 18             # ecgmm_lime_perturb: the row index takes 18 bits of the Philox counter
    PREDICT_FLOATS_PER_ROW = 256   # allowance for predict_fn's own buffers (fusion_classifier: 128 hidden + logits + probabilities)

    def chunk_rows(self, num_samples, byte_budget):
        """rows per chunk such that Z, inverse, d2, y, predict_fn's activations and the ridge workspace stay within
        ``byte_budget``, and within what one launch takes"""
        D, N = self.discretizer.num_features, int(num_samples)
        from .hip import lib as L
        ws = L.lib().ecgmm_lime_ridge_workspace(1, N, D)
        if ws == 0:
            L.check(1, "lime_ridge workspace query")
        per_row = N * D * 5 + N * 4 * (2 + self.PREDICT_FLOATS_PER_ROW) + ws
        return max(1, min(self.MAX_CHUNK, int(byte_budget) // per_row))

    def explain_batch(self, rows, predict_fn, labels=(1,), num_features=10, num_samples=5000, top_labels=None,
                      byte_budget=1 << 30, first_index=0, return_data=False):
        """One Explanation per row of ``rows`` [B, D] (a device tensor).  ``predict_fn`` gets a device tensor [M, D] and
        returns [M, C] probabilities.  The batch is cut into chunks that keep the device buffers within ``byte_budget``
        bytes; the draws of row b depend on (seed, offset, first_index + b) alone, so the chunking changes nothing.
        return_data: also a list, per chunk, of dict(Z, inverse, d2, probs, y, fits)."""
        if top_labels:
            _refuse("top_labels")
        D = self.discretizer.num_features
        labels = tuple(int(l) for l in labels)
        num_features, N = int(num_features), int(num_samples)
        if num_features < 1 or N < 2:
            raise ValueError("need num_features >= 1 and num_samples >= 2")
        select = num_features < D and self.feature_selection != "none"
        if select and self.feature_selection == "auto" and num_features <= 6:
            _refuse("feature_selection='auto' with num_features <= 6 (forward_selection)")
        if not isinstance(rows, torch.Tensor):
            raise TypeError("rows must be a torch tensor on the ROCm device")
        if first_index < 0 or first_index + len(rows) > self.MAX_ROWS:
            raise ValueError(f"rows {first_index} .. {first_index + len(rows)} outside the {self.MAX_ROWS} a batch may number")
        HF._require_cuda(rows, "lime explain")
        if rows.dim() != 2 or rows.shape[1] != D:
            raise ValueError(f"rows must be [B, {D}], got {tuple(rows.shape)}")
        rows = HF.f32c(rows)
        table = self._table(rows.device)
        seed_offset = self._take()
        bins = self.discretizer.discretize(rows)
        step = self.chunk_rows(N, byte_budget)
        out, data = [], []
        for lo in range(0, rows.shape[0], step):
            x = rows[lo:lo + step]
            Bc = x.shape[0]
            Z, inverse, d2 = HF.lime_perturb(x, table, N, b0=first_index + lo, seed_offset=seed_offset)
            with torch.no_grad():
                probs = predict_fn(inverse.view(Bc * N, D))
            if not isinstance(probs, torch.Tensor) or probs.dim() != 2 or probs.shape[0] != Bc * N:
                raise ValueError("predict_fn must return a [M, C] tensor of class probabilities")
            HF._require_cuda(probs, "lime predict_fn output")
            C = probs.shape[1]
            if max(labels) >= C or min(labels) < 0:
                raise ValueError(f"labels {labels} outside the {C} classes predict_fn returns")
            y = probs.float().view(Bc, N, C)[:, :, list(labels)].permute(0, 2, 1).contiguous()
            fits = {}
            if not select:
                fit = HF.lime_ridge(Z, d2, y, self.kernel_width, 1.0)
                host = {k: v.cpu().numpy() for k, v in fit.items() if k != "w"}
                for li, label in enumerate(labels):
                    fits[label] = (None, {k: v[:, li] for k, v in host.items()})
            else:
                first = HF.lime_ridge(Z, d2, y, self.kernel_width, 0.01, want=())
                # highest_weights: the num_features columns of largest |coef * Z[0]| (Z[0] = 1), per label
                keep = first["coef"].abs().topk(num_features, dim=2).indices.sort(dim=2).values.int()
                for li, label in enumerate(labels):
                    cols = keep[:, li].contiguous()
                    fit = HF.lime_ridge(Z, d2, y[:, li:li + 1].contiguous(), self.kernel_width, 1.0, cols=cols)
                    fits[label] = (cols.cpu().numpy(), {k: v[:, 0].cpu().numpy() for k, v in fit.items() if k != "w"})
            for b in range(Bc):
                exp = Explanation(self.discretizer.names(self.feature_names, bins[lo + b]), self.class_names)
                for label in labels:
                    cols, fit = fits[label]
                    coef = fit["coef"][b]
                    feats = np.arange(D) if cols is None else cols[b]
                    order = np.argsort(-np.abs(coef), kind="stable")
                    exp.local_exp[label] = [(int(feats[i]), float(coef[i])) for i in order]
                    exp.intercept[label] = float(fit["intercept"][b])
                    exp.score[label] = float(fit["score"][b])
                    exp.local_pred[label] = float(fit["local_pred"][b])
                out.append(exp)
            if return_data:
                data.append(dict(Z=Z, inverse=inverse, d2=d2, probs=probs, y=y, fits=fits))
        return (out, data) if return_data else out

    def explain_instance(self, data_row, predict_fn, labels=(1,), top_labels=None, num_features=10, num_samples=5000,
                         sample_index=0):
        """lime's explain_instance for one row [D] (a device tensor).  ``sample_index``: the position the row would have in
        ``explain_batch`` -- with it and the same seed the result equals that row of the batch."""
        if not isinstance(data_row, torch.Tensor):
            raise TypeError("data_row must be a torch tensor on the ROCm device")
        return self.explain_batch(data_row.reshape(1, -1), predict_fn, labels=labels, num_features=num_features,
                                  num_samples=num_samples, top_labels=top_labels, first_index=sample_index)[0]
