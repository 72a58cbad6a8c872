"""mmvae.knn on the MI355X with weights in {uniform, distance} and metric in {euclidean, manhattan}, and optimize_knn, against the
records of sklearn and the reference's ConditionedKNeighborsRegressor in tests/golden/knn_tuned.npz, within the derived bounds of
tests/knn_l1_bounds.py.  On the fixture every query is decided at every k of the grid and the winner is clear of the bounds
(tests/test_knn_tune_ref_cpu.py asserts both), so every case is compared and the winner must be the reference's.  Regressors of
the grid's points are built with from_params(): the constructors keep refusing weights other than 'uniform' (tests/test_knn_gpu.py)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import knn_bounds as KB  # noqa: E402
import knn_l1_bounds as LB  # noqa: E402
import knn_tune_ref as TR  # noqa: E402
from mmvae import ops  # noqa: E402
from mmvae.knn import ConditionedKNeighborsRegressor, KNeighborsRegressor, optimize_knn  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_tuned.npz")
REF_EPS = 1e-12       # the float64 reference's own roundoff: 37-term sums of O(1) values, 2^-53 each, with a wide margin


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def dev():
    return {n: torch.from_numpy(v).to(DEV) for n, v in fixture().items() if n in ("X", "Y", "Xq", "Yq", "site", "site_q")}


@functools.lru_cache(maxsize=None)
def tol(i, cond):
    return TR.prediction_tol(fixture(), TR.combinations()[i], cond)


POINTS = [i for i, p in enumerate(TR.combinations()) if p["n_neighbors"] in (5, 50)]       # the four (weights, metric) at the grid's ends


@pytest.mark.parametrize("i", POINTS)
def test_regressor_against_sklearn(i):
    f, d, p = fixture(), dev(), TR.combinations()[i]
    reg = KNeighborsRegressor.from_params(**p).fit(d["X"], d["Y"])
    idx, dist = reg.kneighbors(d["Xq"])
    dist64 = TR.distances(f["Xq"], f["X"], p["metric"])
    want = np.argsort(dist64, axis=1, kind="stable")[:, :p["n_neighbors"]]
    assert np.array_equal(np.sort(idx.cpu().numpy(), axis=1), np.sort(want, axis=1))      # decided: the exact set
    inp = idx.cpu().numpy().astype(np.int64)
    if p["metric"] == "manhattan":                                                      # the distance itself, not its square
        LB.check_dist(LB.analyse(f["Xq"], f["X"], p["n_neighbors"]), inp, dist.cpu().numpy(), label=str(p))
    else:
        shift = reg.shift.cpu().numpy()
        err = np.abs(dist.double().cpu().numpy() - np.take_along_axis(dist64, inp, axis=1) ** 2)
        assert (err <= np.take_along_axis(KB.dist2_tol(f["Xq"], f["X"], shift), inp, axis=1) + REF_EPS).all()
    for bs in (None, 16):
        pred = reg.predict(d["Xq"], batch_size=bs).double().cpu().numpy()
        err = np.abs(pred - f["pred"][i])
        assert (err <= tol(i, False) + REF_EPS).all(), (p, float((err / (tol(i, False) + REF_EPS)).max()))


@pytest.mark.parametrize("i", POINTS)
def test_conditioned_regressor_against_the_reference(i):
    f, d, p = fixture(), dev(), TR.combinations()[i]
    reg = ConditionedKNeighborsRegressor.from_params(**p).fit(d["X"], d["Y"], d["site"])
    pred = reg.predict(d["Xq"], d["site_q"]).double().cpu().numpy()
    err = np.abs(pred - f["cond_pred"][i])
    assert (err <= tol(i, True) + REF_EPS).all(), (p, float((err / (tol(i, True) + REF_EPS)).max()))


@pytest.mark.parametrize("cond", [False, True])
def test_optimize_knn_returns_the_references_winner_and_mses(cond):
    f, d = fixture(), dev()
    pre = "cond_" if cond else ""
    best, params, grid = optimize_knn(d["X"], d["Y"], d["Xq"], d["Yq"], d["site"] if cond else None, d["site_q"] if cond else None, conditioned=cond)
    assert [p for p, _ in grid] == TR.combinations()
    for i, (p, mse) in enumerate(grid):
        bound = LB.mse_tol(f[pre + "pred"][i], f["Yq"], tol(i, cond) + REF_EPS)
        print(f"{'conditioned ' if cond else ''}{p}: mse {mse:.9f} reference {f[pre + 'mse'][i]:.9f} bound {bound:.2e}")
        assert abs(mse - f[pre + "mse"][i]) <= bound, (p, mse, f[pre + "mse"][i], bound)
    assert params == TR.combinations()[int(f[pre + "best"])]
    assert isinstance(best, ConditionedKNeighborsRegressor if cond else KNeighborsRegressor)
    assert (best.n_neighbors, best.weights, best.metric) == (params["n_neighbors"], params["weights"], params["metric"])
    pred = best.predict(d["Xq"], d["site_q"]) if cond else best.predict(d["Xq"])
    assert float(((pred.double() - d["Yq"].double()) ** 2).mean()) == dict((tuple(p.items()), m) for p, m in grid)[tuple(params.items())]
    # every grid point is a prefix of one search: its MSE is, bit for bit, that of an independent fit
    for p, mse in grid[::5]:
        reg = (ConditionedKNeighborsRegressor if cond else KNeighborsRegressor).from_params(**p)
        single = reg.fit(d["X"], d["Y"], d["site"]).predict(d["Xq"], d["site_q"]) if cond else reg.fit(d["X"], d["Y"]).predict(d["Xq"])
        assert float(((single.double() - d["Yq"].double()) ** 2).mean()) == mse, p


def test_optimize_knn_with_a_smaller_grid_and_its_refusals():
    d = dev()
    _, params, grid = optimize_knn(d["X"], d["Y"], d["Xq"], d["Yq"], params={"n_neighbors": [7], "weights": ["distance"], "metric": ["manhattan", "euclidean"]})
    assert [p["metric"] for p, _ in grid] == ["manhattan", "euclidean"] and params["n_neighbors"] == 7
    for bad in (lambda: optimize_knn(d["X"], d["Y"], d["Xq"], d["Yq"], conditioned=True),
                lambda: optimize_knn(d["X"], d["Y"], d["Xq"], d["Yq"], params={"n_neighbors": [5], "weights": ["rank"], "metric": ["euclidean"]}),
                lambda: optimize_knn(d["X"], d["Y"], d["Xq"], d["Yq"], params={"n_neighbors": [301], "weights": ["uniform"], "metric": ["euclidean"]}),
                lambda: KNeighborsRegressor.from_params(5, weights="rank"), lambda: KNeighborsRegressor(5, metric="cosine"),
                lambda: KNeighborsRegressor(5, weights="distance"),                     # the constructor's refusal stays; from_params builds it
                lambda: ConditionedKNeighborsRegressor.from_params(5, weights="rank"), lambda: ConditionedKNeighborsRegressor(5, metric="chebyshev")):
        with pytest.raises(ValueError):
            bad()


def test_the_default_regressor_gives_the_bits_of_the_uniform_euclidean_path():
    d = dev()
    reg = KNeighborsRegressor(5).fit(d["X"], d["Y"])
    assert (reg.weights, reg.metric) == ("uniform", "euclidean")
    idx, _ = ops.knn_search(d["Xq"], d["X"], 5, ops._column_means(d["X"]), dist2=False)
    want = ops.knn_mean_rows(idx, d["Y"])
    assert torch.equal(reg.predict(d["Xq"]).view(torch.int32), want.view(torch.int32))
    assert torch.equal(reg.kneighbors(d["Xq"])[0], idx)
