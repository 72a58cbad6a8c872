"""tests/knn_tune_ref.py on the CPU against tests/golden/knn_tuned.npz (sklearn's KNeighborsRegressor and the reference's
ConditionedKNeighborsRegressor over the reference's grid, tools/make_knn_tune_fixture.py) and against sklearn directly where it
imports; and the two conditions the fixture's seed was chosen for, which the GPU tests rely on."""
import importlib.util
import os

import numpy as np
import pytest

import knn_tune_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "knn_tuned.npz")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def test_the_fixture_has_the_stated_sizes(fx):
    assert fx["X"].shape == (300, 37) and fx["Xq"].shape == (77, 37) and fx["Y"].shape == (300, 23) and fx["Yq"].shape == (77, 23)
    assert all(fx[n].dtype == np.float32 for n in ("X", "Y", "Xq", "Yq"))
    rows = np.bincount(fx["site"])
    assert len(rows) == 5 and len(set(rows)) == 5 and (rows < 50).any() and (rows < 5).any()
    assert set(np.unique(fx["site_q"])) == set(range(5))
    assert fx["mse"].shape == fx["cond_mse"].shape == (16,) and fx["pred"].shape == fx["cond_pred"].shape == (16, 77, 23)
    assert os.path.getsize(GOLDEN) <= max(os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f)) for f in os.listdir(os.path.dirname(GOLDEN))
                                          if f != "knn_tuned.npz")


def test_the_grid_order_is_that_of_itertools_product():
    c = TR.combinations()
    assert len(c) == 16 and c[0] == {"n_neighbors": 5, "weights": "uniform", "metric": "euclidean"}
    assert c[1]["metric"] == "manhattan" and c[2]["weights"] == "distance" and c[4]["n_neighbors"] == 10


@pytest.mark.parametrize("cond", [False, True])
def test_the_restatement_equals_the_records(fx, cond):
    X, Y, Xq, Yq, site, site_q = (fx[n] for n in ("X", "Y", "Xq", "Yq", "site", "site_q"))
    fn = (lambda **p: TR.conditioned_regress(X, Y, site, Xq, site_q, **p)) if cond else (lambda **p: TR.knn_regress(X, Y, Xq, **p))
    mses, best, preds = TR.optimize(fn, Yq)
    pre = "cond_" if cond else ""
    assert np.abs(preds - fx[pre + "pred"]).max() <= 1e-12
    assert np.abs(mses - fx[pre + "mse"]).max() <= 1e-13 and best == int(fx[pre + "best"])
    assert best == int(np.argmin(fx[pre + "mse"]))


def test_the_restatement_equals_sklearn(fx):
    neighbors = pytest.importorskip("sklearn.neighbors")
    X, Y, Xq = (fx[n].astype(np.float64) for n in ("X", "Y", "Xq"))
    for p in TR.combinations():
        want = neighbors.KNeighborsRegressor(**p).fit(X, Y).predict(Xq)
        assert np.abs(TR.knn_regress(X, Y, Xq, **p) - want).max() <= 1e-12, p


def test_every_query_is_decided_and_the_winner_is_clear(fx):
    spec = importlib.util.spec_from_file_location("make_knn_tune_fixture", os.path.join(ROOT, "tools", "make_knn_tune_fixture.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert TR.conditions(fx, fx) == (True, True)
    regen = tool.inputs(int(fx["seed"]))
    assert all(np.array_equal(regen[n], fx[n]) for n in ("X", "Y", "Xq", "Yq", "site", "site_q"))
