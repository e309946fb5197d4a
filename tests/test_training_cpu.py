"""ecgmm.training on the CPU: the epoch loop's policy (strict improvement, patience, LR / 10, file names), one pass over a
loader, the checkpoint test loop, the resident loader's order and length, and the NaN-guarded AUC.  A ``torch.nn.Linear``, SGD
and a scripted ``step`` that returns preset validation losses stand in for a trainer; the HIP library is never loaded."""
import math
import os

import pytest
import torch

import ecgmm.training as T


class _Rig:
    """model + optimizer + the two passes of a trainer whose validation losses are ``val_losses``; ``events`` records the
    order of what happened"""

    def __init__(self, val_losses, train_batches=3, val_batches=2):
        torch.manual_seed(0)
        self.model = torch.nn.Linear(4, 2)
        self.optimizer = torch.optim.SGD(self.model.parameters(), lr=0.1)
        self.scheduler = torch.optim.lr_scheduler.LambdaLR(self.optimizer, lambda k: 1.0)
        self.val_losses, self.events, self.sched_steps = list(val_losses), [], 0
        self.scheduler.step = self._sched_step
        self.train_loader = [(torch.randn(5, 4), torch.randint(0, 2, (5,))) for _ in range(train_batches)]
        self.val_loader = [(torch.randn(5, 4), torch.randint(0, 2, (5,))) for _ in range(val_batches)]
        self.epoch = 0

    def _sched_step(self):
        self.sched_steps += 1

    def step(self, batch):
        x, y = batch
        out = self.model(x)
        return torch.nn.functional.cross_entropy(out, y), out, y

    def val_step(self, batch):
        _, out, y = self.step(batch)
        assert not torch.is_grad_enabled()
        return torch.tensor(self.val_losses[self.epoch]), out, y      # the same loss for every batch: the mean is that loss

    def train_pass(self):
        self.events.append("train")
        return T.run_epoch(self.train_loader, self.step, self.optimizer, self.scheduler)

    def val_pass(self):
        self.events.append("val")
        result = T.run_epoch(self.val_loader, self.val_step, scheduler=self.scheduler)
        self.epoch += 1
        return result

    def refresh(self):
        self.events.append("refresh")

    def fit(self, tmp_path, **kw):
        return T.fit(self.model, self.optimizer, self.train_pass, self.val_pass, str(tmp_path), len(self.val_losses), **kw)


def _weights(path):
    return torch.load(path, map_location="cpu")["weight"]


def test_history_records_and_a_lower_loss_overwrites_best(tmp_path):
    rig = _Rig([0.5, 0.75, 0.25])
    seen, weights = [], []

    def on_epoch(record, extras):
        seen.append(dict(record))
        weights.append(rig.model.weight.detach().clone())
        assert extras == {}

    history = rig.fit(tmp_path, on_epoch=on_epoch)
    assert seen == history and [h["epoch"] for h in history] == [1, 2, 3] and [h["val_loss"] for h in history] == [0.5, 0.75, 0.25]
    assert all(set(h) == {"epoch", "train_loss", "train_acc", "val_loss", "val_acc"} for h in history)
    assert all(math.isfinite(h["train_loss"]) and 0.0 <= h["train_acc"] <= 1.0 and 0.0 <= h["val_acc"] <= 1.0 for h in history)
    assert torch.equal(_weights(tmp_path / "best.pth"), weights[2]) and torch.equal(_weights(tmp_path / "last.pth"), weights[2])
    assert not torch.equal(weights[0], weights[2])


def test_equal_loss_keeps_the_earlier_best(tmp_path):
    rig = _Rig([0.5, 0.5])
    kept = []
    rig.fit(tmp_path, on_epoch=lambda record, extras: kept.append(rig.model.weight.detach().clone()))
    assert torch.equal(_weights(tmp_path / "best.pth"), kept[0]) and not torch.equal(kept[0], kept[1])
    assert torch.equal(_weights(tmp_path / "last.pth"), kept[1])


def test_nan_loss_never_writes_a_best_file(tmp_path):
    rig = _Rig([float("nan"), float("nan")])
    history = rig.fit(tmp_path)
    assert len(history) == 2 and all(math.isnan(h["val_loss"]) for h in history)
    assert sorted(os.listdir(tmp_path)) == ["last.pth"]
    assert T.test_checkpoints(rig.model, str(tmp_path), ("best", "last"), lambda: "scored") == {"last": "scored"}
    with pytest.raises(FileNotFoundError):
        T.test_checkpoints(rig.model, str(tmp_path), ("best", "last"), lambda: "scored", skip_missing=False)


@pytest.mark.parametrize("patience", [1, 3])
def test_patience_stops_after_exactly_that_many_misses(tmp_path, patience):
    rig = _Rig([0.5] + [0.75] * 6)
    history = rig.fit(tmp_path, patience=patience)
    assert len(history) == 1 + patience
    assert len(_Rig([0.5] + [0.75] * 6).fit(tmp_path)) == 7          # no patience: every epoch runs


def test_lr_decay_after_two_misses_resets_on_improvement_and_after_a_decay(tmp_path):
    #        improve miss  improve miss  miss->/10  miss  miss->/10  improve
    losses = [0.5, 0.75, 0.25, 0.5, 0.5, 0.5, 0.5, 0.125]
    rig = _Rig(losses)
    lrs = []
    # on_epoch runs before the epoch's policy, so it sees the lr the epoch trained with
    rig.fit(tmp_path, lr_decay_after=2, on_epoch=lambda record, extras: lrs.append(rig.optimizer.param_groups[0]["lr"]))
    want = [0.1, 0.1, 0.1, 0.1, 0.1, 0.1 / 10, 0.1 / 10, 0.1 / 10 / 10]
    assert lrs == want and rig.optimizer.param_groups[0]["lr"] == want[-1]
    lrs.clear()
    rig = _Rig(losses)
    rig.fit(tmp_path, on_epoch=lambda record, extras: lrs.append(rig.optimizer.param_groups[0]["lr"]))
    assert lrs == [0.1] * 8                                            # off by default


def test_best_names_carry_the_one_based_epoch_and_last_is_optional(tmp_path):
    rig = _Rig([0.5, 0.75, 0.25])
    rig.fit(tmp_path, save_last=None, best_names=("epoch{epoch}.pth", "best.pth", "best_inner.pth"))
    assert sorted(os.listdir(tmp_path)) == ["best.pth", "best_inner.pth", "epoch1.pth", "epoch3.pth"]


def test_scheduler_steps_once_per_training_batch_and_never_in_validation(tmp_path):
    rig = _Rig([0.5, 0.25], train_batches=3, val_batches=2)
    rig.fit(tmp_path)
    assert rig.sched_steps == 2 * 3


def test_predictor_is_refreshed_between_training_and_validation_and_once_per_tag(tmp_path):
    rig = _Rig([0.5, 0.25])
    rig.fit(tmp_path, predictor=rig)
    assert rig.events == ["train", "refresh", "val"] * 2
    rig.events.clear()
    results = T.test_checkpoints(rig.model, str(tmp_path), ("best", "last"), lambda: rig.events.append("evaluate"), predictor=rig)
    assert rig.events == ["refresh", "evaluate"] * 2 and set(results) == {"best", "last"}


def test_run_epoch_means_accuracy_and_extras():
    rig = _Rig([0.5])
    logits = torch.tensor([[2.0, 0.0], [0.0, 2.0], [2.0, 0.0], [0.0, 2.0]])
    batches = [(logits, torch.tensor([0, 1, 1, 1])), (logits[:2], torch.tensor([1, 0]))]     # 3 of 4, then 0 of 2

    def step(batch):
        assert not torch.is_grad_enabled()
        out, y = batch
        return torch.tensor(float(len(y))), out, y, {"extra": torch.tensor(2.0 * len(y))}

    loss, acc, extras = T.run_epoch(batches, step)
    assert loss == (4 + 2) / 2 and acc == 3 / 6 and extras == {"extra": (8 + 4) / 2}
    loss, acc, extras = T.run_epoch(batches, lambda b: step(b)[:3], count_correct=False)
    assert loss == 3.0 and acc is None and extras == {}
    assert T.run_epoch([], step) == (0.0, 0.0, {})
    before = rig.model.weight.detach().clone()
    T.run_epoch(rig.train_loader, rig.step, rig.optimizer)
    assert not torch.equal(before, rig.model.weight)                     # with an optimizer the pass trains


# ---------------------------------------------------------------------------------------------------- ResidentLoader
class _Rows:
    def __init__(self, n):
        self.labels = torch.arange(n)

    def __len__(self):
        return self.labels.numel()


class _Loader(T.ResidentLoader):
    def batch(self, idx):
        return self.dataset.labels[idx]


class _Sampler:
    def __init__(self, n, count):
        self.n, self.count, self.draws = n, count, 0

    def __len__(self):
        return self.count

    def sample(self):
        self.draws += 1
        return torch.arange(self.count) % self.n


def test_resident_loader_length():
    ds = _Rows(37)
    assert len(_Loader(ds, 16)) == 3 and len(_Loader(ds, 16, drop_last=True)) == 2
    assert len(_Loader(ds, 16, sampler=_Sampler(37, 40))) == 3 and len(_Loader(ds, 16, drop_last=True, sampler=_Sampler(37, 40))) == 2
    assert [b.numel() for b in _Loader(ds, 16)] == [16, 16, 5]                  # the last partial batch is kept
    assert [b.numel() for b in _Loader(ds, 16, drop_last=True)] == [16, 16]
    with pytest.raises(ValueError, match="mutually exclusive"):
        _Loader(ds, 16, shuffle=True, sampler=_Sampler(37, 40))


@pytest.mark.parametrize("seed", [0, 42])
def test_resident_loader_order_is_one_randperm_per_epoch(seed):
    n = 37
    loader = _Loader(_Rows(n), 16, shuffle=True, generator=torch.Generator().manual_seed(seed))
    assert loader.last_order is None
    want = torch.Generator().manual_seed(seed)
    for _epoch in range(2):
        seen = torch.cat(list(loader))
        order = torch.randperm(n, generator=want)
        assert torch.equal(loader.last_order, order) and torch.equal(seen, order)
    plain = _Loader(_Rows(n), 16)
    assert torch.equal(torch.cat(list(plain)), torch.arange(n)) and torch.equal(plain.last_order, torch.arange(n))


def test_resident_loader_draws_from_its_sampler_once_per_epoch():
    sampler = _Sampler(37, 40)
    loader = _Loader(_Rows(37), 16, sampler=sampler)
    for epoch in (1, 2):
        seen = torch.cat(list(loader))
        assert sampler.draws == epoch
        assert torch.equal(seen, torch.arange(40) % 37) and torch.equal(loader.last_order, seen)


# ---------------------------------------------------------------------------------------------------------- metrics
def test_auc_or_nan_and_binary_metrics():
    assert math.isnan(T.auc_or_nan([1, 1, 1], [0.2, 0.5, 0.9]))
    assert T.auc_or_nan([0, 1, 0, 1], [0.1, 0.9, 0.2, 0.8]) == 1.0
    m = T.binary_metrics([0, 1, 0, 1], [0.1, 0.9, 0.6, 0.8], [0, 1, 1, 1])
    assert m == {"accuracy": 0.75, "f1": 0.8, "auc": 1.0}
    one_class = T.binary_metrics([0, 0], [0.1, 0.2], [0, 0])
    assert one_class["accuracy"] == 1.0 and one_class["f1"] == 0.0 and math.isnan(one_class["auc"])


def test_predict_collects_device_side_softmax_and_argmax():
    torch.manual_seed(1)
    net = torch.nn.Linear(4, 3)
    batches = [(torch.randn(5, 4), torch.randint(0, 3, (5,))) for _ in range(2)]
    y_true, y_prob, y_pred, loss = T.predict(net, batches, criterion=torch.nn.functional.cross_entropy)
    with torch.no_grad():
        logits = torch.cat([net(x) for x, _ in batches])
        want_loss = sum(torch.nn.functional.cross_entropy(net(x), y).item() for x, y in batches) / 2
    assert torch.equal(torch.from_numpy(y_prob), torch.softmax(logits, 1)) and y_prob.dtype.name == "float32"
    assert y_pred.tolist() == logits.argmax(1).tolist() and y_true.tolist() == torch.cat([y for _, y in batches]).tolist()
    assert loss == want_loss
    assert T.predict(lambda x: net(x[:, :4]), [(torch.randn(2, 6), torch.zeros(2))], prepare=None)[3] is None
    shaped = T.predict(net, [(torch.randn(2, 2, 2), torch.zeros(2))], prepare=lambda x: x.reshape(2, 4))
    assert shaped[1].shape == (2, 3)


def test_module_level_imports_are_torch_numpy_os_and_time():
    """so importing it loads neither the HIP library nor sklearn"""
    import ast
    with open(T.__file__) as f:
        tree = ast.parse(f.read())
    names = set()
    for node in tree.body:
        if isinstance(node, ast.Import):
            names |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add("." * node.level + (node.module or ""))
    assert names == {"os", "time", "numpy", "torch"}
