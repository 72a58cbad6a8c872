"""k-NN imputation baselines and the neighbourhood hit on the device: the reference's KNeighborsRegressor(n_neighbors=5) rows
(compare_directional_imputation.py:235-254, vae_cross_modality_cv.py:320, cluster_imputation_methods.py:297-403), its
ConditionedKNeighborsRegressor (src/models/conditioned_knn.py:18-93) and calculate_neighborhood_hit
(src/clustering_evaluation/metrics_utils.py:19-38) on ONE search kernel (mmvae_knn_search: a fp32 MFMA GEMM whose epilogue is a running
top-k, the queries x training rows score matrix never exists) and one streaming gather (mmvae_knn_mean_rows).

    reg = KNeighborsRegressor(5).fit(X_train, Y_train)             # device tensors, fp32 or bf16 rows; nothing is copied
    Y_hat = reg.predict(X_val)                                     # fp32 (rows, outputs) on the device
    creg = ConditionedKNeighborsRegressor(5).fit(X_train, Y_train, site_train)
    Y_hat = creg.predict(X_val, site_val)
    nh = neighborhood_hit(latent, labels, k=5)

Neighbours are ordered by (distance key, training index): among exactly equal distances the smaller training index wins, where
sklearn's order is unspecified.  Uniform weights and the euclidean metric only (nothing in the reference uses another)."""
import torch

from . import ops


def _check_kind(weights, metric):
    if weights != "uniform":
        raise ValueError(f"weights={weights!r}: only 'uniform' is implemented")
    if metric != "euclidean":
        raise ValueError(f"metric={metric!r}: only 'euclidean' is implemented")


def _device_matrix(t, name):
    return ops._device_matrix(t, name, "mmvae.knn")


class KNeighborsRegressor:
    def __init__(self, n_neighbors=5, weights="uniform", metric="euclidean"):
        _check_kind(weights, metric)
        if int(n_neighbors) < 1:
            raise ValueError(f"n_neighbors={n_neighbors}")
        self.n_neighbors, self.weights, self.metric = int(n_neighbors), weights, metric
        self.X = self.Y = self.shift = None

    def fit(self, X, Y):
        """Keeps references to X (rows, features) and Y (rows, outputs); the training column means become the search's shift."""
        X, Y = _device_matrix(X, "X"), _device_matrix(Y, "Y")
        if X.shape[0] != Y.shape[0] or X.shape[0] < 1:
            raise ValueError(f"fit: X {tuple(X.shape)} against Y {tuple(Y.shape)}")
        if self.n_neighbors > X.shape[0]:
            raise ValueError(f"n_neighbors={self.n_neighbors} > {X.shape[0]} training rows")       # sklearn raises at predict
        self.X, self.Y, self.shift = X, Y, ops._column_means(X)
        return self

    def kneighbors(self, Xq, dist2=True):
        if self.X is None:
            raise RuntimeError("kneighbors() before fit()")
        return ops.knn_search(_device_matrix(Xq, "Xq"), self.X, self.n_neighbors, self.shift, dist2=dist2)

    def predict(self, Xq, batch_size=None):
        """fp32 (rows, outputs); batch_size bounds the queries per search (the result does not depend on it)."""
        Xq = _device_matrix(Xq, "Xq")
        out = torch.empty(Xq.shape[0], self.Y.shape[1], dtype=torch.float32, device=Xq.device)
        step = Xq.shape[0] if not batch_size else int(batch_size)
        for i in range(0, Xq.shape[0], max(step, 1)):
            idx, _ = self.kneighbors(Xq[i:i + step], dist2=False)
            ops.knn_mean_rows(idx, self.Y, out[i:i + step])
        return out


class ConditionedKNeighborsRegressor:
    """One KNeighborsRegressor per site over that site's training rows (conditioned_knn.py).  `site` is an explicit int64 vector here,
    not the last column of X."""

    def __init__(self, n_neighbors=5, weights="uniform", metric="euclidean"):
        _check_kind(weights, metric)
        self.n_neighbors, self.weights, self.metric = int(n_neighbors), weights, metric
        self.models = {}
        self.n_outputs_ = None

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
                self.models[v] = KNeighborsRegressor(k).fit(Xs[lo:lo + c], Ys[lo:lo + c])
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
