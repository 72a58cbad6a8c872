"""k-NN imputation baselines and the neighbourhood hit on the device: the reference's KNeighborsRegressor(n_neighbors=5) rows
(compare_directional_imputation.py:235-254, vae_cross_modality_cv.py:320, cluster_imputation_methods.py:297-403), its
ConditionedKNeighborsRegressor (src/models/conditioned_knn.py:18-93) and calculate_neighborhood_hit
(src/clustering_evaluation/metrics_utils.py:19-38) on ONE search kernel (mmvae_knn_search: a fp32 MFMA GEMM whose epilogue is a running
top-k, the queries x training rows score matrix never exists) and one streaming gather (mmvae_knn_mean_rows); and the reference's tuned
baseline, optimize_knn (src/knn_comparison/run_comparison.py:56-94): a grid over n_neighbors x weights {uniform, distance} x metric
{euclidean, manhattan}, with the manhattan search (mmvae_knn_search_l1) and the inverse-distance regression (mmvae_knn_weighted_rows).

    reg = KNeighborsRegressor(5).fit(X_train, Y_train)             # device tensors, fp32 or bf16 rows; nothing is copied
    Y_hat = reg.predict(X_val)                                     # fp32 (rows, outputs) on the device
    creg = ConditionedKNeighborsRegressor(5).fit(X_train, Y_train, site_train)
    Y_hat = creg.predict(X_val, site_val)
    nh = neighborhood_hit(latent, labels, k=5)
    best, params, grid = optimize_knn(X_train, Y_train, X_val, Y_val)         # 16 grid points from two searches

Neighbours are ordered by (distance key, training index): among exactly equal distances the smaller training index wins, where
sklearn's order is unspecified.  weights: 'uniform' or 'distance', metric: 'euclidean' or 'manhattan' -- the grid of the reference's
optimize_knn; its other scripts use the defaults.  The constructors take both metrics but keep refusing every weights but 'uniform',
as they always have (callers rely on that ValueError); a regressor of any grid point comes from the classmethod

    reg = KNeighborsRegressor.from_params(n_neighbors=20, weights="distance", metric="manhattan").fit(X_train, Y_train)

which is what optimize_knn returns.  kneighbors() returns squared distances for euclidean and the L1 distances themselves for
manhattan."""
import itertools

import torch

from . import ops


WEIGHTS, METRICS = ("uniform", "distance"), ("euclidean", "manhattan")
GRID = {"n_neighbors": [5, 10, 20, 50], "weights": list(WEIGHTS), "metric": list(METRICS)}      # run_comparison.py:63-67


def _check_kind(weights, metric, constructor=False):
    if constructor and weights != "uniform":
        raise ValueError(f"weights={weights!r}: the constructor takes 'uniform' only; from_params() builds a regressor with any of {WEIGHTS}")
    if weights not in WEIGHTS:
        raise ValueError(f"weights={weights!r}: one of {WEIGHTS}")
    if metric not in METRICS:
        raise ValueError(f"metric={metric!r}: one of {METRICS}")


def _search(Xq, X, k, metric, shift, dist=True):
    """(idx, dist): squared distances for euclidean, the distances themselves for manhattan"""
    if metric == "manhattan":
        return ops.knn_search_l1(Xq, X, k, dist=dist)
    return ops.knn_search(Xq, X, k, shift, dist2=dist)


def _regress(idx, dist, Y, k, weights, metric, out=None):
    """the regression rows from the first k columns of a search's (idx, dist)"""
    if weights == "uniform":
        return ops.knn_mean_rows(idx[:, :k], Y, out)
    return ops.knn_weighted_rows(idx[:, :k], dist[:, :k], Y, metric == "euclidean", out)


def _from_params(cls, n_neighbors=5, weights="uniform", metric="euclidean"):
    """A regressor with any weights of WEIGHTS and metric of METRICS: the parameters of sklearn's class, as optimize_knn's grid
    spells them (cls.from_params(**params))."""
    _check_kind(weights, metric)
    reg = cls(n_neighbors, "uniform", metric)
    reg.weights = weights
    return reg


def _device_matrix(t, name):
    return ops._device_matrix(t, name, "mmvae.knn")


class KNeighborsRegressor:
    def __init__(self, n_neighbors=5, weights="uniform", metric="euclidean"):
        _check_kind(weights, metric, constructor=True)
        if int(n_neighbors) < 1:
            raise ValueError(f"n_neighbors={n_neighbors}")
        self.n_neighbors, self.weights, self.metric = int(n_neighbors), weights, metric
        self.X = self.Y = self.shift = None

    from_params = classmethod(_from_params)

    def fit(self, X, Y):
        """Keeps references to X (rows, features) and Y (rows, outputs); the training column means become the search's shift."""
        X, Y = _device_matrix(X, "X"), _device_matrix(Y, "Y")
        if X.shape[0] != Y.shape[0] or X.shape[0] < 1:
            raise ValueError(f"fit: X {tuple(X.shape)} against Y {tuple(Y.shape)}")
        if self.n_neighbors > X.shape[0]:
            raise ValueError(f"n_neighbors={self.n_neighbors} > {X.shape[0]} training rows")       # sklearn raises at predict
        self.X, self.Y, self.shift = X, Y, ops._column_means(X) if self.metric == "euclidean" else None
        return self

    def kneighbors(self, Xq, dist2=True):
        if self.X is None:
            raise RuntimeError("kneighbors() before fit()")
        return _search(_device_matrix(Xq, "Xq"), self.X, self.n_neighbors, self.metric, self.shift, dist=dist2)

    def predict(self, Xq, batch_size=None):
        """fp32 (rows, outputs); batch_size bounds the queries per search (the result does not depend on it)."""
        Xq = _device_matrix(Xq, "Xq")
        out = torch.empty(Xq.shape[0], self.Y.shape[1], dtype=torch.float32, device=Xq.device)
        step = Xq.shape[0] if not batch_size else int(batch_size)
        for i in range(0, Xq.shape[0], max(step, 1)):
            idx, dist = self.kneighbors(Xq[i:i + step], dist2=self.weights == "distance")
            _regress(idx, dist, self.Y, self.n_neighbors, self.weights, self.metric, out[i:i + step])
        return out


class ConditionedKNeighborsRegressor:
    """One KNeighborsRegressor per site over that site's training rows (conditioned_knn.py).  `site` is an explicit int64 vector here,
    not the last column of X."""

    def __init__(self, n_neighbors=5, weights="uniform", metric="euclidean"):
        _check_kind(weights, metric, constructor=True)
        self.n_neighbors, self.weights, self.metric = int(n_neighbors), weights, metric
        self.models = {}
        self.n_outputs_ = None

    from_params = classmethod(_from_params)

    @staticmethod
    def _sites(site, rows):
        if not isinstance(site, torch.Tensor) or site.dim() != 1 or site.shape[0] != rows or site.dtype != torch.int64:
            raise ValueError(f"site must be an int64 ({rows},) tensor")
        return site

    def fit(self, X, Y, site):
        X, Y = _device_matrix(X, "X"), _device_matrix(Y, "Y")
        site = self._sites(site, X.shape[0]).to(X.device)
        order = torch.argsort(site, stable=True)            # the training rows by site, once; a site's rows keep their order
        Xs, Ys = X[order], Y[order]
        values, counts = torch.unique_consecutive(site[order], return_counts=True)
        self.models, self.n_outputs_ = {}, Y.shape[1]
        lo = 0
        for v, c in zip(values.tolist(), counts.tolist()):
            k = min(self.n_neighbors, c)
            if k >= 1:
                self.models[v] = KNeighborsRegressor.from_params(k, self.weights, self.metric).fit(Xs[lo:lo + c], Ys[lo:lo + c])
            lo += c
        return self

    def predict(self, Xq, site):
        Xq = _device_matrix(Xq, "Xq")
        site = self._sites(site, Xq.shape[0]).to(Xq.device)
        out = torch.zeros(Xq.shape[0], self.n_outputs_, dtype=torch.float32, device=Xq.device)
        order = torch.argsort(site, stable=True)
        values, counts = torch.unique_consecutive(site[order], return_counts=True)
        Xs = Xq[order]
        lo = 0
        for v, c in zip(values.tolist(), counts.tolist()):
            if v in self.models:                             # a site without training rows keeps its zero rows
                out[order[lo:lo + c]] = self.models[v].predict(Xs[lo:lo + c])
            lo += c
        return out


def neighborhood_hit(features, labels, k=5):
    """Mean over rows of the share of a row's k nearest other rows that carry its label (calculate_neighborhood_hit): the k + 1 nearest
    of every row among all rows, the first column (the row itself) dropped.  0.0 for fewer than k + 1 rows."""
    if len(features) < k + 1:
        return 0.0
    features = _device_matrix(features, "features")
    labels = torch.as_tensor(labels).to(features.device)
    if labels.dim() != 1 or labels.shape[0] != features.shape[0]:
        raise ValueError(f"labels must be ({features.shape[0]},)")
    idx, _ = ops.knn_search(features, features, k + 1, ops._column_means(features), dist2=False)
    hits = labels[idx[:, 1:].long()] == labels[:, None]
    return float(hits.double().mean(dim=1).mean())


def _by_site(site, rows, dev):
    """(order, [(site value, lo, count)]): the rows grouped by site, a site's rows in their order"""
    site = ConditionedKNeighborsRegressor._sites(site, rows).to(dev)
    order = torch.argsort(site, stable=True)
    values, counts = torch.unique_consecutive(site[order], return_counts=True)
    los = [0]
    for c in counts.tolist():
        los.append(los[-1] + c)
    return order, list(zip(values.tolist(), los[:-1], counts.tolist()))


def optimize_knn(X_train, Y_train, X_val, Y_val, site_train=None, site_val=None, *, params=None, conditioned=False):
    """The reference's optimize_knn (run_comparison.py:56-94): every combination of `params` (default GRID: 4 x 2 x 2, in
    itertools.product order, n_neighbors outermost, metric innermost) is fitted on the training rows and scored by the validation MSE
    (mean over all elements, float64); the first strict minimum wins.  Returns (best_model, best_params, grid), grid a list of
    (params, mse) in that order; best_model is fitted and its predict() reproduces the winning prediction.
    One search per metric at max(n_neighbors) serves the whole grid: neighbours come ascending by (key, index), so the k nearest are
    the first k columns of any wider answer, bit for bit.  conditioned: ConditionedKNeighborsRegressor -- one such search per site and
    metric, with min(n_neighbors, rows of the site) neighbours; needs site_train / site_val (int64 vectors)."""
    params = dict(GRID if params is None else params)
    if set(params) != set(GRID) or not all(len(v) for v in params.values()):
        raise ValueError(f"params must list {sorted(GRID)}")
    for w, m in itertools.product(params["weights"], params["metric"]):
        _check_kind(w, m)
    ks = [int(k) for k in params["n_neighbors"]]
    X, Y, Xq, Yq = (_device_matrix(t, n) for t, n in ((X_train, "X_train"), (Y_train, "Y_train"), (X_val, "X_val"), (Y_val, "Y_val")))
    if X.shape[0] != Y.shape[0] or Xq.shape[0] != Yq.shape[0] or Yq.shape[1] != Y.shape[1] or min(ks) < 1:
        raise ValueError(f"optimize_knn: train {tuple(X.shape)} / {tuple(Y.shape)}, validation {tuple(Xq.shape)} / {tuple(Yq.shape)}, n_neighbors {ks}")
    kmax = max(ks)
    if conditioned:
        if site_train is None or site_val is None:
            raise ValueError("optimize_knn(conditioned=True) needs site_train and site_val")
        order_t, groups_t = _by_site(site_train, X.shape[0], X.device)
        order_q, groups_q = _by_site(site_val, Xq.shape[0], X.device)
        Xs, Ys, Xqs = X[order_t], Y[order_t], Xq[order_q]
        train = {v: (lo, c) for v, lo, c in groups_t}
        parts = []                                   # (validation rows, the site's Y, rows of the site, {metric: (idx, dist)})
        for v, lo, c in groups_q:
            if v not in train:
                continue                             # a site without training rows keeps its zero rows
            tlo, tc = train[v]
            Xt = Xs[tlo:tlo + tc]
            found = {m: _search(Xqs[lo:lo + c], Xt, min(kmax, tc), m, ops._column_means(Xt) if m == "euclidean" else None) for m in params["metric"]}
            parts.append((order_q[lo:lo + c], Ys[tlo:tlo + tc], tc, found))
    else:
        if kmax > X.shape[0]:
            raise ValueError(f"n_neighbors={kmax} > {X.shape[0]} training rows")
        shift = ops._column_means(X)
        parts = [(None, Y, X.shape[0], {m: _search(Xq, X, kmax, m, shift if m == "euclidean" else None) for m in params["metric"]})]
    Yq64 = Yq.double()
    pred = torch.empty(Xq.shape[0], Y.shape[1], dtype=torch.float32, device=X.device)
    grid, best_mse, best_params = [], float("inf"), {}
    for k, w, m in itertools.product(ks, params["weights"], params["metric"]):
        if conditioned:
            pred.zero_()
        for rows, Yt, tc, found in parts:
            idx, dist = found[m]
            if rows is None:
                _regress(idx, dist, Yt, k, w, m, pred)
            else:
                pred[rows] = _regress(idx, dist, Yt, min(k, tc), w, m)
        p = {"n_neighbors": k, "weights": w, "metric": m}
        mse = float(((pred.double() - Yq64) ** 2).mean())
        grid.append((p, mse))
        if mse < best_mse:                           # run_comparison.py:88: the first strict minimum
            best_mse, best_params = mse, p
    if conditioned:
        best = ConditionedKNeighborsRegressor.from_params(**best_params).fit(X, Y, site_train)
    else:
        best = KNeighborsRegressor.from_params(**best_params).fit(X, Y)
    return best, best_params, grid
