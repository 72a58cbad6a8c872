"""mmvae.crossval on the MI355X at the tiny dims of tests/test_evaluate_knn_gpu.py (RNA 40, DNA 24, 5 sites, latent 8, 300 rows),
5 folds, k in {5, 10}: the neighbours of the one fold-masked search are the float64 restatement's (every query of every fold is
decided under tests/knn_bounds.py, so the device must return the same sets), the per-fold metrics of the mean baseline, the kNN and
the site-conditioned kNN lie within the derived metric bounds (tests/metrics_bounds.py) of the restatement, the VAE folds are
reproducible functions of the seed, and the comparison block is the restatement's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crossval_ref as CR  # noqa: E402
import knn_bounds as KB  # noqa: E402
import knn_ref as KR  # noqa: E402
import metrics_bounds as MB  # noqa: E402
import trainer  # noqa: E402
from mmvae import crossval as CV  # noqa: E402
from src.config import Config  # noqa: E402

A, D, S, L, N, FOLDS, KS = 40, 24, 5, 8, 300, 5, (5, 10)
DEV = "cuda"
DIRS = {"DNA -> RNA": ("b", "a"), "RNA -> DNA": ("a", "b")}


@pytest.fixture(scope="module")
def data():
    tpm, beta_v, site = trainer.synthetic_dataset(N, A, D, S, Config.RANDOM_SEED)
    return dict(a=tpm.numpy(), b=beta_v.numpy(), site=site.numpy(), fold=CV.kfold_assignments(N, FOLDS),
                da=tpm.to(DEV), db=beta_v.to(DEV), dsite=site.to(DEV))


def shift_of(X):
    return X.astype(np.float64).mean(axis=0).astype(np.float32)


def exact_neighbours(X, fold, k, site=None):
    """(N, k) int64, -1 behind a short list: the float64 neighbours per (fold, site) group of queries, every one asserted decided"""
    out = np.full((len(X), k), -1, np.int64)
    shift = shift_of(X)
    site = np.zeros(len(X), np.int64) if site is None else site
    for f in np.unique(fold):
        for s in np.unique(site):
            q, cand = np.flatnonzero((fold == f) & (site == s)), np.flatnonzero((fold != f) & (site == s))
            kk = min(k, len(cand))
            if len(q) == 0 or kk == 0:
                continue
            an = KB.analyse(X[q], X[cand], kk, shift)
            assert an["decided"].all(), (f, s, "an undecided query: the exact set cannot be required")
            out[q, :kk] = cand[an["order"][:, :kk]]
    return out


def predictions_f32(idx, Y):
    """what knn_predictions must produce from these lists: the fp32 mean over a row's c >= 1 entries, zeros for c = 0"""
    out = np.zeros((idx.shape[0], Y.shape[1]), np.float32)
    c = (idx >= 0).sum(axis=1)
    for cv in np.unique(c):
        if cv > 0:
            out[c == cv] = KR.mean_rows_f32(idx[c == cv][:, :cv], Y)
    return out


def check_fold_metrics(result, Y, pred_of_fold, fold, label):
    """every fold's six metrics against the restatement on (Y[fold rows], pred) within metrics_tol"""
    assert list(result["fold_metrics"]) == list(CR.KEYS)
    for f in range(int(fold.max()) + 1):
        rows = np.flatnonzero(fold == f)
        y, p = Y[rows].astype(np.float64), np.asarray(pred_of_fold(f, rows), np.float64)
        want, tol = CR.metric_dict(y, p), MB.metrics_tol(y, p, y[0])
        for key, src in CR.KEYS.items():
            got = result["fold_metrics"][key][f]
            print(f"{label} fold {f} {key}: {got!r} want {want[key]!r} bound {tol[src]:.3e}")
            assert np.isfinite(tol[src]) and abs(got - want[key]) <= tol[src], (label, f, key, got, want[key], tol[src])
    for key in CR.KEYS:
        assert result[f"mean_{key}"] == float(np.mean(result["fold_metrics"][key])) and result[f"std_{key}"] == float(np.std(result["fold_metrics"][key]))


@pytest.mark.parametrize("direction", list(DIRS))
def test_mean_and_knn_folds_equal_the_restatement(direction, data):
    src, tgt = DIRS[direction]
    X, Y, fold = data[src], data[tgt], data["fold"]
    fold32 = torch.from_numpy(fold).to(DEV)
    exact = exact_neighbours(X, fold, max(KS))
    idx = CV.masked_neighbours(data["d" + src], fold32, max(KS)).cpu().numpy().astype(np.int64)
    for k in KS:
        assert np.array_equal(np.sort(idx[:, :k], axis=1), np.sort(exact[:, :k], axis=1)), (k, "the neighbour sets differ from the float64 sets")
    preds = {}
    results = CV.cross_validate(data["d" + src], data["d" + tgt], data["dsite"], fold, direction, ("mean", "knn"), KS, predictions=preds)
    assert [(r["direction"], r["model"], r["param_name"], r["param_value"]) for r in results] == \
        [(direction, "mean", "dummy", 0), (direction, "knn", "k", 5), (direction, "knn", "k", 10)]
    total = Y.astype(np.float64).sum(axis=0)
    check_fold_metrics(results[0], Y, lambda f, rows: np.broadcast_to(((total - Y[rows].astype(np.float64).sum(axis=0)) / (N - len(rows))).astype(np.float32),
                                                                      (len(rows), Y.shape[1])), fold, f"{direction} mean")
    for r, k in zip(results[1:], KS):
        want = predictions_f32(idx[:, :k], Y)                                   # averaged in the device's neighbour order
        assert np.array_equal(preds[("knn", k)].cpu().numpy().view(np.uint32), want.view(np.uint32))
        check_fold_metrics(r, Y, lambda f, rows: want[rows], fold, f"{direction} knn k={k}")
        assert r["time"] > 0


def test_knn_by_site_folds_equal_the_restatement(data):
    X, Y, fold, site = data["b"], data["a"], data["fold"], data["site"]
    for s in range(S):
        for f in range(FOLDS):
            assert ((site == s) & (fold != f)).sum() >= 37
    exact = exact_neighbours(X, fold, max(KS), site)
    idx = CV.masked_neighbours(data["db"], torch.from_numpy(fold).to(DEV), max(KS), data["dsite"].int()).cpu().numpy().astype(np.int64)
    assert (idx >= 0).all() and np.array_equal(np.sort(idx, axis=1), np.sort(exact, axis=1))
    assert (site[idx] == site[:, None]).all() and (fold[idx] != fold[:, None]).all()
    preds = {}
    results = CV.cross_validate(data["db"], data["da"], data["dsite"], fold, "DNA -> RNA", ("knn_site",), KS, predictions=preds)
    assert [(r["model"], r["param_value"]) for r in results] == [("knn_site", 5), ("knn_site", 10)]
    for r, k in zip(results, KS):
        want = predictions_f32(idx[:, :k], Y)
        assert np.array_equal(preds[("knn_site", k)].cpu().numpy().view(np.uint32), want.view(np.uint32))
        check_fold_metrics(r, Y, lambda f, rows: want[rows], fold, f"knn_site k={k}")


def test_knn_by_site_with_short_and_empty_lists(data):
    """a site of 3 rows, two of them in one fold: lists of 1, 1 and 2 entries; a site of 2 rows in one fold: no candidate, zero rows"""
    X, Y, fold = data["b"], data["a"], data["fold"]
    site = data["site"].copy()
    f0, f1 = np.flatnonzero(fold == 0), np.flatnonzero(fold == 1)
    site[[f0[0], f0[1], f1[0]]] = S
    site[[f1[1], f1[2]]] = S + 1
    exact = exact_neighbours(X, fold, max(KS), site)
    c = (exact >= 0).sum(axis=1)
    assert c[[f0[0], f0[1], f1[0]]].tolist() == [1, 1, 2] and c[[f1[1], f1[2]]].tolist() == [0, 0]
    dsite = torch.from_numpy(site).to(DEV)
    idx = CV.masked_neighbours(data["db"], torch.from_numpy(fold).to(DEV), max(KS), dsite.int()).cpu().numpy().astype(np.int64)
    assert np.array_equal((idx >= 0).sum(axis=1), c) and np.array_equal(np.sort(idx, axis=1), np.sort(exact, axis=1))
    assert ((idx >= 0) == (np.arange(max(KS))[None, :] < c[:, None])).all(), "entries first, -1 behind them"
    preds = {}
    results = CV.cross_validate(data["db"], data["da"], dsite, fold, "DNA -> RNA", ("knn_site",), KS, predictions=preds)
    for r, k in zip(results, KS):
        want = predictions_f32(idx[:, :k], Y)
        got = preds[("knn_site", k)].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (got[[f1[1], f1[2]]] == 0).all() and np.array_equal(got[f1[0]], KR.mean_rows_f32(idx[f1[0]:f1[0] + 1, :2], Y)[0])
        check_fold_metrics(r, Y, lambda f, rows: want[rows], fold, f"short lists k={k}")
    with pytest.raises(ValueError, match="fewer than"):                          # the plain kNN refuses short lists, as sklearn does
        CV.knn_predictions(data["db"][:12], data["da"][:12], torch.from_numpy(CV.kfold_assignments(12, 3)).to(DEV), (10,))


@pytest.fixture(scope="module")
def vae_runs(data):
    """3 folds, 2 epochs, batch 32: all models once, the VAE again with the same seed and once with another"""
    fold = CV.kfold_assignments(N, 3)
    kw = dict(epochs=2, batch_size=32, latent_dim=L, n_sites=S)
    preds, preds_again, preds_other = {}, {}, {}
    full = CV.cross_validate(data["db"], data["da"], data["dsite"], fold, "DNA -> RNA", ("mean", "knn", "vae"), KS, seed=42, predictions=preds, **kw)
    again = CV.cross_validate(data["db"], data["da"], data["dsite"], fold, "DNA -> RNA", ("vae",), KS, seed=42, predictions=preds_again, **kw)
    other = CV.cross_validate(data["db"], data["da"], data["dsite"], fold, "DNA -> RNA", ("vae",), KS, seed=43, predictions=preds_other, **kw)
    return dict(fold=fold, full=full, again=again[0], other=other[0], preds=preds, preds_again=preds_again, preds_other=preds_other)


def test_vae_folds_are_finite_and_functions_of_the_seed(vae_runs, data):
    vae = vae_runs["full"][-1]
    assert (vae["model"], vae["param_name"], vae["param_value"]) == ("vae", "epochs", 2) and list(vae["fold_metrics"]) == list(CR.KEYS)
    for key, scores in vae["fold_metrics"].items():
        assert len(scores) == 3 and np.isfinite(scores).all(), key
    # the same seed gives the same models: every prediction bit for bit (the metrics launch adds with float64 atomics, so the metrics
    # of two runs agree within their bounds, which check_fold_metrics asserts for both runs against the one prediction)
    pred = vae_runs["preds"][("vae", 2)]
    assert torch.equal(pred.view(torch.int32), vae_runs["preds_again"][("vae", 2)].view(torch.int32)), "the same seed must give the same folds"
    assert not torch.equal(pred, vae_runs["preds_other"][("vae", 2)]), "another seed must give another model"
    assert vae["fold_metrics"] != vae_runs["other"]["fold_metrics"]
    # every row predicted exactly once: the assembled prediction reproduces every fold's metrics, and no row is left at zero
    assert pred.shape == (N, A) and bool((pred != 0).any(dim=1).all())
    host = pred.cpu().numpy()
    for run, label in ((vae, "vae"), (vae_runs["again"], "vae again")):
        check_fold_metrics(run, data["a"], lambda f, rows: host[rows], vae_runs["fold"], label)


def test_comparisons_equal_the_restatement(vae_runs):
    pytest.importorskip("scipy.stats")
    results = vae_runs["full"]
    assert [r["model"] for r in results] == ["mean", "knn", "knn", "vae"]
    for metric in ("Mean R2", "MSE", "Pearson"):
        got = CV.compare(results, metric)
        assert len(got) == 1 and {"knn_vs_vae", "vae_vs_mean"} <= set(got[0])
        CR.same_comparison(got, CR.compare(results, metric), rel=1e-9)


@pytest.mark.parametrize("eager", [False, True])
def test_the_restored_state_is_the_best_epochs(eager, data):
    """the validation losses are stubbed as 3, 1, 2: the state after the second epoch must come back, not the last one"""
    seen = []

    def val_loss(model, epoch):
        seen.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        return [3.0, 1.0, 2.0][epoch]

    model, best = CV.fit_vae("dna2rna", data["da"][:200], data["db"][:200], data["dsite"][:200], (A, D, S, L), epochs=3, batch_size=32,
                             eager=eager, val_loss_fn=val_loss)
    assert len(seen) == 3 and best.best_epoch == 1 and best.best == 1.0 and best.trigger == 1 and not model.training
    now = model.state_dict()
    assert all(torch.equal(now[k], seen[1][k]) for k in now)
    assert any(not torch.equal(seen[2][k], seen[1][k]) for k in now), "the third epoch must have moved the weights"
    assert any(not torch.equal(seen[0][k], seen[1][k]) for k in now)


def test_early_stop_bookkeeping_counts_patience():
    b = CV.BestState(2)
    m = torch.nn.Linear(2, 2)
    assert [b.update(v, m, e) for e, v in enumerate([5.0, 4.0, 4.0, 4.5])] == [False, False, False, True] and b.best_epoch == 1


def test_refusals(data):
    with pytest.raises(ValueError):
        CV.cross_validate(data["db"], data["da"], data["dsite"], data["fold"], "DNA -> protein")
    with pytest.raises(ValueError):
        CV.cross_validate(data["db"], data["da"], data["dsite"], data["fold"], "DNA -> RNA", ("ae",))
    with pytest.raises(ValueError):
        CV.cross_validate(data["db"], data["da"], data["dsite"], data["fold"] + 1, "DNA -> RNA", ("mean",))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CV.cross_validate(torch.zeros(10, 3), torch.zeros(10, 2), torch.zeros(10), CV.kfold_assignments(10, 2), "DNA -> RNA", ("mean",))
