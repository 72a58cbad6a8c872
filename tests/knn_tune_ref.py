"""float64 restatement of the tuned k-NN baseline (mmvae.knn.optimize_knn): sklearn's KNeighborsRegressor with weights in {uniform,
distance} and metric in {euclidean, manhattan}, the reference's ConditionedKNeighborsRegressor (src/models/conditioned_knn.py) over
them, and the grid loop of its optimize_knn (src/knn_comparison/run_comparison.py:56-94, restated here because that module imports
plotting libraries): every combination in itertools.product order, validation MSE over all elements, the first strict minimum wins.
Neighbours are ranked by (distance, training index)."""
import itertools

import numpy as np

import knn_l1_bounds as LB
import knn_ref as KR

GRID = {"n_neighbors": [5, 10, 20, 50], "weights": ["uniform", "distance"], "metric": ["euclidean", "manhattan"]}


def combinations(params=None):
    params = GRID if params is None else params
    keys, values = zip(*params.items())
    return [dict(zip(keys, v)) for v in itertools.product(*values)]


def distances(Xq, X, metric):
    """(Mq, Nt) float64 distances in the metric's own unit"""
    return LB.dist1(Xq, X) if metric == "manhattan" else np.sqrt(KR.dist2(Xq, X))


def knn_regress(X, Y, Xq, n_neighbors=5, weights="uniform", metric="euclidean"):
    Y = np.asarray(Y, np.float64)
    Y = Y[:, None] if Y.ndim == 1 else Y
    d = distances(Xq, X, metric)
    idx = np.argsort(d, axis=1, kind="stable")[:, :n_neighbors]
    if weights == "uniform":
        return Y[idx].mean(axis=1)
    return LB.weighted_rows(idx, np.take_along_axis(d, idx, axis=1), Y, False)


def conditioned_regress(X, Y, site, Xq, site_q, n_neighbors=5, weights="uniform", metric="euclidean"):
    X, Xq, Y = np.asarray(X, np.float64), np.asarray(Xq, np.float64), np.asarray(Y, np.float64)
    site, site_q = np.asarray(site).astype(int), np.asarray(site_q).astype(int)
    out = np.zeros((Xq.shape[0], Y.shape[1]))
    for s in np.unique(site_q):
        m = site == s
        if m.any():
            out[site_q == s] = knn_regress(X[m], Y[m], Xq[site_q == s], min(n_neighbors, int(m.sum())), weights, metric)
    return out


def mse(y, pred):
    return float(np.mean((np.asarray(y, np.float64) - np.asarray(pred, np.float64)) ** 2))


def optimize(predict, y_val, params=None):
    """the loop of run_comparison.py:73-91 over predict(**p) -> (mses, index of the winner, predictions)"""
    best, best_i, mses, preds = float("inf"), -1, [], []
    for i, p in enumerate(combinations(params)):
        pred = predict(**p)
        m = mse(y_val, pred)
        mses.append(m)
        preds.append(pred)
        if m < best:
            best, best_i = m, i
    return np.array(mses), best_i, np.stack(preds)


# ---------------------------------------------------------------------------------------------------------------------------
# what the fixture's seed is chosen for (tools/make_knn_tune_fixture.py) and the device tests rely on
# ---------------------------------------------------------------------------------------------------------------------------
def conditions(d, ref=None):
    """(every query decided at every grid k, both metrics, plain and per site; MSE gap of the two best > their bounds, both grids).
    ref: dict(mse, cond_mse, pred, cond_pred) of the records, or None to use the restatement"""
    import knn_bounds as KB
    X, Y, Xq, Yq, site, site_q = (d[n] for n in ("X", "Y", "Xq", "Yq", "site", "site_q"))
    groups = [(np.ones(len(X), bool), np.ones(len(Xq), bool))] + [(site == s, site_q == s) for s in np.unique(site_q) if (site == s).any()]
    decided = True
    for mt, mq in groups:
        shift = X[mt].astype(np.float64).mean(axis=0).astype(np.float32)
        for k in GRID["n_neighbors"]:
            k = min(k, int(mt.sum()))
            decided &= bool(KB.analyse(Xq[mq], X[mt], k, shift)["decided"].all()) and bool(LB.analyse(Xq[mq], X[mt], k)["decided"].all())
    if not decided:
        return False, False
    clear = True
    for cond in (False, True):
        if ref is None:
            fn = (lambda **p: conditioned_regress(X, Y, site, Xq, site_q, **p)) if cond else (lambda **p: knn_regress(X, Y, Xq, **p))
            mses, _, preds = optimize(fn, Yq)
        else:
            mses, preds = (ref["cond_mse"], ref["cond_pred"]) if cond else (ref["mse"], ref["pred"])
        tol = np.array([LB.mse_tol(preds[i], Yq, prediction_tol(d, p, cond)) for i, p in enumerate(combinations())])
        a, b = np.argsort(mses, kind="stable")[:2]
        clear &= bool(mses[b] - mses[a] > tol[a] + tol[b])
    return True, clear


def prediction_tol(d, p, cond):
    """elementwise bound on |device prediction - float64 reference| at grid point p (tests/knn_l1_bounds.py: predict_tol)"""
    X, Y, Xq, site, site_q = (d[n] for n in ("X", "Y", "Xq", "site", "site_q"))
    if not cond:
        shift = X.astype(np.float64).mean(axis=0).astype(np.float32)
        return LB.predict_tol(X, Y, Xq, p["n_neighbors"], p["weights"], p["metric"], shift)
    out = np.zeros((Xq.shape[0], Y.shape[1]))
    for s in np.unique(site_q):
        m = site == s
        if m.any():
            shift = X[m].astype(np.float64).mean(axis=0).astype(np.float32)
            out[site_q == s] = LB.predict_tol(X[m], Y[m], Xq[site_q == s], min(p["n_neighbors"], int(m.sum())), p["weights"], p["metric"], shift)
    return out
