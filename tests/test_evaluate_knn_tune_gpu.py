"""evaluate.py --knn-tune [--knn-by-site] [--knn-tune-out] on the MI355X at small dims: the tuned rows are those of
mmvae.knn.optimize_knn called directly on the same split, the JSON carries the 16-point grids, and the tuned row is no worse than the
--knn 5 row, whose point the grid contains."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate  # noqa: E402
import metrics_bounds as MB  # noqa: E402
import metrics_ref as MR  # noqa: E402
import trainer  # noqa: E402
from mmvae.knn import optimize_knn  # noqa: E402
from src.config import Config  # noqa: E402
from src.models import RNA2DNAVAE  # noqa: E402

A, D, S, L, N = 40, 24, 5, 8, 2048
DIMS = ["--samples", str(N), "--input-dim-a", str(A), "--input-dim-b", str(D), "--n-sites", str(S), "--latent-dim", str(L)]
SCALARS = ("MAE", "MSE", "RMSE", "R2", "MeanR2", "CosineSimilarity", "PearsonMean", "PearsonStd")


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    torch.manual_seed(3)
    path = str(tmp_path_factory.mktemp("ckpt") / "rna2dna.pt")
    torch.save(RNA2DNAVAE(A, D, S, L).state_dict(), path)
    return path


@pytest.fixture(scope="module")
def tables(checkpoint, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("out") / "tune.json")
    common = DIMS + ["--batch-size", "128", "--precision", "fp32", "--checkpoint", checkpoint]
    plain = evaluate.run("rna2dna", common)
    rows = evaluate.run("rna2dna", common + ["--knn", "5", "--knn-tune", "--knn-by-site", "--knn-tune-out", out])
    with open(out) as f:
        return plain, rows, json.load(f)


@pytest.fixture(scope="module")
def direct():
    """optimize_knn on the split evaluate.py uses: {conditioned: (best, params, grid, validation targets, prediction)}"""
    tpm, beta_v, site = trainer.synthetic_dataset(N, A, D, S, Config.RANDOM_SEED)
    val_idx, train_idx = trainer.split_indices(N)
    tr = [t[train_idx].cuda().contiguous() for t in (tpm, beta_v, site)]
    va = [t[val_idx].cuda().contiguous() for t in (tpm, beta_v, site)]
    out = {}
    for cond in (False, True):
        best, params, grid = optimize_knn(tr[0], tr[1], va[0], va[1], tr[2] if cond else None, va[2] if cond else None, conditioned=cond)
        pred = best.predict(va[0], va[2]) if cond else best.predict(va[0])
        out[cond] = (best, params, grid, va[1].cpu().numpy(), pred.cpu().numpy())
    return out


def key(r):
    return r["Route"], r["Modality"], r["Model"]


def test_the_tuned_rows_are_those_of_optimize_knn(tables, direct):
    plain, rows, _ = tables
    assert [key(r) for r in rows[:len(plain)]] == [key(r) for r in plain] and len(plain) == 2
    names = []
    for cond in (False, True):
        p = direct[cond][1]
        names.append(("a+site->b" if cond else "a->b", "DNA", f"kNN-{'site-' if cond else ''}tuned(k={p['n_neighbors']},w={p['weights']},m={p['metric']})"))
    assert [key(r) for r in rows[len(plain):]] == [("a->b", "DNA", "kNN(k=5)"), ("a+site->b", "DNA", "kNN-site(k=5)"), names[0], names[1]]
    got = {key(r): r for r in rows}
    for cond in (False, True):
        _, _, grid, y, pred = direct[cond]
        row = got[names[cond]]
        y64, p64 = y.astype(np.float64), pred.astype(np.float64)
        want, tol = MR.metrics(y64, p64), MB.metrics_tol(y64, p64, y64[0])
        for k in SCALARS:
            assert np.isfinite(tol[k]) and abs(row[k] - want[k]) <= tol[k], (cond, k, row[k], want[k], tol[k])
        assert abs(row["MSE"] - min(m for _, m in grid)) <= tol["MSE"]
    # the grid contains (5, uniform, euclidean): the winner's MSE cannot exceed that row's
    assert got[names[0]]["MSE"] <= got[("a->b", "DNA", "kNN(k=5)")]["MSE"]
    assert got[names[1]]["MSE"] <= got[("a+site->b", "DNA", "kNN-site(k=5)")]["MSE"]


def test_the_json_carries_the_grids_the_winners_and_the_box_plot_numbers(tables, direct):
    _, rows, js = tables
    assert [t["conditioned"] for t in js] == [False, True]
    for t in js:
        _, params, grid, _, _ = direct[t["conditioned"]]
        assert t["best"] == params and key(t) in {key(r) for r in rows}
        assert len(t["grid"]) == 16 and [dict(g) for g in t["grid"]] == [dict(p, mse=m) for p, m in grid]          # the same bits
        assert t["best_mse"] == min(m for _, m in grid) == dict((json.dumps(p, sort_keys=True), m) for p, m in grid)[json.dumps(params, sort_keys=True)]
        assert set(t["per_sample_mse"]) == {t["Model"], "RNA2DNAVAE"}
        for s in t["per_sample_mse"].values():
            assert s["min"] <= s["q1"] <= s["median"] <= s["q3"] <= s["max"] and s["min"] <= s["mean"] <= s["max"]
        # rows of equal length: the mean of the per-sample MSEs is the MSE over all elements
        assert t["per_sample_mse"][t["Model"]]["mean"] == pytest.approx(t["best_mse"], rel=1e-12)


def test_the_flags_that_need_another_are_refused(checkpoint):
    for flags in (["--knn-by-site"], ["--knn-tune-out", "x.json"]):
        with pytest.raises(SystemExit):
            evaluate.run("rna2dna", DIMS + ["--checkpoint", checkpoint] + flags)
