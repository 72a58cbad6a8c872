"""mmvae.downstream.cross_validate and SiteClassifier.fit on the MI355X against the reference's protocol run in stock torch on the CPU
(tools/make_downstream_fixture.py; results recorded in tests/golden/downstream.npz)."""
import os

import numpy as np
import pytest
import torch

from mmvae import downstream

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "downstream.npz")
DEV = "cuda"
EPOCHS = 25           # the recorded runs may take 100; most stop early, and the test has seconds


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return dict(X=z["fit_X"], y=z["fit_y"], acc=z["fit_acc"], f1=z["fit_f1"])


def test_the_recorded_runs_reach_090(gold):
    assert gold["X"].shape == (600, 40) and sorted(np.bincount(gold["y"])) == [3, 37, 60, 100, 150, 250]
    assert len(gold["acc"]) >= 3 and gold["acc"].min() >= 0.9 and gold["f1"].min() >= 0.88


def test_five_folds_do_not_fall_below_the_recorded_runs(gold):
    names = [f"site{c}" for c in range(6)]
    X, y = torch.from_numpy(gold["X"]).to(DEV), torch.from_numpy(gold["y"]).to(DEV)
    r = downstream.cross_validate(X, y, names, 5, epochs=EPOCHS, seed=42)
    print(f"device: accuracy {r['accuracy']:.4f} weighted F1 {r['weighted avg']['f1-score']:.4f}; recorded accuracy {gold['acc']}, F1 {gold['f1']}")
    for got, rec in ((r["accuracy"], gold["acc"]), (r["weighted avg"]["f1-score"], gold["f1"])):
        assert got >= rec.min() - (rec.max() - rec.min())
    # the aggregated dict of run_classification_scenario
    assert set(r) == {"accuracy", "accuracy_std", "weighted avg", *names}
    keys = {"precision", "precision_std", "recall", "recall_std", "f1-score", "f1-score_std"}
    assert set(r["weighted avg"]) == keys and all(set(r[n]) == keys for n in names)
    assert 0 <= r["accuracy_std"] < 0.1


class Scripted(downstream.SiteClassifier):
    """evaluate() answers from a contrived validation sequence; training is skipped"""

    def script(self, losses, accs, rows):
        self._script, self._rows, self.lrs = list(zip(losses, accs)), rows, []

    def train_epoch(self, generator=None):
        self.lrs.append(float(self._lr.item()))                   # what the step would read from the device

    def evaluate(self, x, labels, class_weights=None, batch_size=None):
        loss, acc = self._script[len(self.lrs) - 1]
        conf = torch.zeros(self.n_classes, self.n_classes, dtype=torch.int32, device=self.device)
        conf[0, 0] = len(self.lrs)
        return torch.tensor([loss, acc * self._rows / 100.0, 0.0], dtype=torch.float64, device=self.device), None, conf


def test_early_stopping_and_the_plateau_scheduler_act():
    X = torch.zeros(50, 8, device=DEV)
    y = torch.zeros(50, dtype=torch.int64, device=DEV)
    # the loss stalls from epoch 2 on: patience 5 -> the rate halves after 6 bad epochs; accuracy peaks at epoch 3: 10 epochs later the run stops
    losses = [1.0, 0.8] + [0.8] * 30
    accs = [50, 60, 70, 80] + [80] * 28
    net = Scripted(8, 2, (16,), True, (0.1,), device=DEV)
    net.script(losses, accs, 50)
    out = net.fit(X, y, X, y, None, epochs=32)
    assert out["epochs"] == 14 and out["best_epoch"] == 3 and out["best_acc"] == 80
    assert net.lrs[:8] == [pytest.approx(1e-3)] * 8 and net.lrs[8:14] == [pytest.approx(5e-4)] * 6
    assert out["confusion"][0, 0] == 14                            # restore_best=False: the last epoch's model is the one reported
    net.script(losses, accs, 50)
    out = net.fit(X, y, X, y, None, epochs=32, restore_best=True)
    assert out["confusion"][0, 0] == 4 and out["epochs"] == 14
    # without a stall neither acts
    net.script(list(np.linspace(1, 0.1, 20)), list(np.linspace(50, 90, 20)), 50)
    out = net.fit(X, y, X, y, None, epochs=20)
    assert out["epochs"] == 20 and net.lrs == [pytest.approx(1e-3)] * 20


def test_fit_learns_one_fold_and_reads_back_once_per_epoch(gold, monkeypatch):
    X, y = torch.from_numpy(gold["X"]).to(DEV), torch.from_numpy(gold["y"]).to(DEV)
    from mmvae.clustering import standardize
    z = standardize(X)
    net = downstream.SiteClassifier(40, 6, device=DEV, seed=3)
    reads = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.append(1), real(self))[1])
    out = net.fit(z[:480], y[:480], z[480:], y[480:], None, epochs=6, generator=torch.Generator().manual_seed(1))
    assert len(reads) == out["epochs"] == 6
    assert out["confusion"].sum() == 120 and np.trace(out["confusion"]) / 120 >= 0.8
    assert out["history"][-1][0] < out["history"][0][0]            # the validation loss fell
