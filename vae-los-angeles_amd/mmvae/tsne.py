"""t-SNE in two dimensions on the device: the subset of sklearn.manifold.TSNE that the reference's perform_dimensionality_reduction
uses (src/clustering_evaluation/cluster_imputation_methods.py:140-187: TSNE(n_components=2, random_state=42, perplexity=min(30, n - 1))
on a PCA(50) of the standardised features).

    Y = TSNE(n_components=2, perplexity=30.0, random_state=42).fit_transform(Z)      # Z: fp32 or bf16 (N, F) on the device

It is sklearn's method="barnes_hut" at angle = 0: the sparse P comes from the int(3 perplexity + 1) nearest neighbours and the
repulsion runs over every pair, exactly, with no tree (mmvae_tsne_gradient).  The neighbour search is mmvae_knn_search, the perplexity
search mmvae_tsne_affinities, the step mmvae_tsne_update; the symmetrisation of P between them is a sort of 64-bit keys in torch.  The
schedule is sklearn's: learning_rate = max(N / early_exaggeration / 4, 50), 250 iterations with P exaggerated at momentum 0.5, then
momentum 0.8; error and gradient norm are read every 50 iterations (the only host synchronisations of the loop) for sklearn's two
stopping rules.  Euclidean metric and n_components = 2 only."""
import math

import torch

from . import _lib as L
from . import ops
from .pca import PCA

__all__ = ["TSNE", "conditional_neighbours", "joint_probabilities"]

_EXPLORATION_MAX_ITER = 250         # sklearn's TSNE._EXPLORATION_MAX_ITER
_N_ITER_CHECK = 50                  # sklearn's TSNE._N_ITER_CHECK
_FLOAT64_MAX = 1.7976931348623157e308


def conditional_neighbours(X, n_neighbors):
    """(idx int32 (N, n_neighbors), dist2 fp32 (N, n_neighbors)): every row's nearest other rows, ascending.  The search takes
    n_neighbors + 1 with the column means as shift and drops the entry that is the row itself, or the last entry where duplicates of the
    row pushed it out of its own list."""
    N = X.shape[0]
    k = int(n_neighbors)
    if not 1 <= k <= min(N - 1, L.KNN_MAXK - 1):
        raise ValueError(f"t-SNE: {k} neighbours outside [1, min(N - 1 = {N - 1}, {L.KNN_MAXK - 1})] (MMVAE_KNN_MAXK - 1)")
    idx, d2 = ops.knn_search(X, X, k + 1, ops._column_means(X))
    me = torch.arange(N, device=X.device, dtype=torch.int32).unsqueeze(1)
    is_self = idx == me
    drop = torch.where(is_self.any(dim=1), is_self.int().argmax(dim=1), torch.full((N,), k, device=X.device))
    keep = torch.arange(k + 1, device=X.device).unsqueeze(0) != drop.unsqueeze(1)
    return idx[keep].view(N, k).contiguous(), d2[keep].view(N, k).contiguous()


def joint_probabilities(idx, p_cond):
    """P = (P_cond + P_cond^T) / sum as CSR (row_ptr int32 (N + 1,), col int32 (nnz,), val fp32 (nnz,)), columns ascending within a row.
    The 64-bit keys (i << 32 | j) of both orientations are sorted and equal keys merged; a slot has at most two addends, so its sum has
    one set of bits whatever order they arrive in.  The total is accumulated in float64."""
    N, k = idx.shape
    dev = idx.device
    i = torch.arange(N, device=dev, dtype=torch.int64).unsqueeze(1).expand(N, k).reshape(-1)
    j = idx.reshape(-1).to(torch.int64)
    v = p_cond.reshape(-1)
    keys, perm = torch.sort(torch.cat([(i << 32) | j, (j << 32) | i]))
    vals = torch.cat([v, v])[perm]
    first = torch.ones_like(keys, dtype=torch.bool)
    first[1:] = keys[1:] != keys[:-1]
    pos = torch.nonzero(first).squeeze(1)
    nxt = (pos + 1).clamp_max(keys.numel() - 1)
    pair = (~first[nxt]) & (pos + 1 < keys.numel())
    val = vals[pos] + torch.where(pair, vals[nxt], torch.zeros_like(vals[nxt]))
    ukeys = keys[pos]
    total = val.double().sum().clamp_min(torch.finfo(torch.float64).eps)
    val = (val.double() / total).float().contiguous()
    row_ptr = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    row_ptr[1:] = torch.cumsum(torch.bincount(ukeys >> 32, minlength=N), 0)
    return row_ptr, (ukeys & 0xFFFFFFFF).to(torch.int32).contiguous(), val


class TSNE:
    """sklearn.manifold.TSNE(n_components=2) on device tensors.  init: "pca" (mmvae.pca.PCA(2) scaled to 1e-4 / std of its first column,
    as sklearn scales it), "random" (1e-4 N(0, 1) from a torch generator on the device seeded with random_state: NOT numpy's stream, so
    not sklearn's draw for the same seed) or an fp32 (N, 2) tensor.  After fit_transform: embedding_ fp32 (N, 2) on the device,
    kl_divergence_ (float), n_iter_, learning_rate_; history_ lists (iteration, error, gradient norm, exaggeration) of every check."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, n_iter_without_progress=300,
                 min_grad_norm=1e-7, init="pca", random_state=None, metric="euclidean"):
        if n_components != 2:
            raise ValueError(f"n_components={n_components!r}: only 2 is implemented")
        if metric != "euclidean":
            raise ValueError(f"metric={metric!r}: only 'euclidean' is implemented")
        if not float(perplexity) > 0:
            raise ValueError(f"perplexity={perplexity!r} must be positive")
        if not float(early_exaggeration) >= 1:
            raise ValueError(f"early_exaggeration={early_exaggeration!r} must be at least 1")
        if learning_rate != "auto" and not float(learning_rate) > 0:
            raise ValueError(f"learning_rate={learning_rate!r} must be 'auto' or positive")
        if int(max_iter) < _EXPLORATION_MAX_ITER:
            raise ValueError(f"max_iter={max_iter!r} must be at least {_EXPLORATION_MAX_ITER}")
        if not (isinstance(init, torch.Tensor) or init in ("pca", "random")):
            raise ValueError(f"init={init!r} must be 'pca', 'random' or an (N, 2) tensor")
        self.n_components, self.perplexity, self.early_exaggeration = 2, float(perplexity), float(early_exaggeration)
        self.learning_rate, self.max_iter, self.n_iter_without_progress = learning_rate, int(max_iter), int(n_iter_without_progress)
        self.min_grad_norm, self.init, self.random_state, self.metric = float(min_grad_norm), init, random_state, metric
        self.embedding_ = self.kl_divergence_ = self.n_iter_ = self.learning_rate_ = None

    def _initial(self, X):
        N = X.shape[0]
        if isinstance(self.init, torch.Tensor):
            if not self.init.is_cuda or tuple(self.init.shape) != (N, 2):
                raise ValueError(f"init must be a device tensor of shape ({N}, 2)")
            return self.init.detach().float().contiguous().clone()
        if self.init == "pca":
            if X.shape[1] < 2:
                raise ValueError("init='pca' needs at least 2 features")
            Y = PCA(2).fit_transform(X)
            return (Y / Y[:, 0].double().std(unbiased=False).float() * 1e-4).contiguous()
        gen = torch.Generator(device=X.device)
        gen.manual_seed(0 if self.random_state is None else int(self.random_state))
        return (1e-4 * torch.randn(N, 2, generator=gen, device=X.device, dtype=torch.float32)).contiguous()

    def _descend(self, Y, P, it, max_iter, momentum, exaggeration, n_iter_without_progress, work):
        """sklearn's _gradient_descent from iteration `it`: fresh update and gains, (error, last iteration).  The kernel's error takes P as
        stored; under exaggeration sklearn's takes x P inside the logarithm too: sum x p log(x p / q) = x (KL + log x) with sum p = 1."""
        update, gains = torch.zeros_like(Y), torch.ones_like(Y)
        grad = torch.empty_like(Y)
        error, best_error = None, _FLOAT64_MAX
        best_iter = i = it
        for i in range(it, max_iter):
            check = (i + 1) % _N_ITER_CHECK == 0
            want_error = check or i == max_iter - 1
            _, _, err, _ = ops.tsne_gradient(Y, *P, exaggeration, error=want_error, grad_out=grad, work=work[0])
            gn = ops.tsne_update(Y, update, gains, grad, momentum, self.learning_rate_, grad_norm=check, work=work[1])
            if want_error:
                error = float(err.double().sum())                  # the host synchronisation of every 50th iteration
                if exaggeration != 1.0:
                    error = exaggeration * (error + math.log(exaggeration))
            if check:
                grad_norm = float(gn)
                self.history_.append((i + 1, error, grad_norm, exaggeration))
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > n_iter_without_progress:
                    break
                if grad_norm <= self.min_grad_norm:
                    break
        return error, i

    def fit_transform(self, X):
        if not isinstance(X, torch.Tensor) or not X.is_cuda:
            raise RuntimeError("mmvae.tsne: X must be a CUDA/HIP tensor; there is no CPU fallback")
        X = ops._device_matrix(X, "X", "mmvae.tsne")
        N = X.shape[0]
        if not self.perplexity < N:
            raise ValueError(f"perplexity ({self.perplexity}) must be less than n_samples ({N})")
        if self.learning_rate == "auto":
            self.learning_rate_ = max(N / self.early_exaggeration / 4, 50.0)
        else:
            self.learning_rate_ = float(self.learning_rate)
        k = min(N - 1, int(3.0 * self.perplexity + 1))
        if not self.perplexity < k:
            raise ValueError(f"perplexity ({self.perplexity}) must be below the {k} neighbours of {N} samples")
        idx, d2 = conditional_neighbours(X, k)
        p_cond, self.beta_ = ops.tsne_affinities(d2, self.perplexity)
        P = joint_probabilities(idx, p_cond)
        Y = self._initial(X)
        work = (ops._workspace(ops.tsne_gradient_work_bytes(N), X.device), ops._workspace(ops.tsne_update_work_bytes(N), X.device))
        self.history_ = []
        error, it = self._descend(Y, P, 0, _EXPLORATION_MAX_ITER, 0.5, self.early_exaggeration, _EXPLORATION_MAX_ITER, work)
        if it < _EXPLORATION_MAX_ITER or self.max_iter - _EXPLORATION_MAX_ITER > 0:
            last, it = self._descend(Y, P, it + 1, self.max_iter, 0.8, 1.0, self.n_iter_without_progress, work)
            error = error if last is None else last          # max_iter = 250: no iteration is left (sklearn reports the largest float64)
        self.n_iter_, self.kl_divergence_, self.embedding_ = it, error, Y
        return Y

    def fit(self, X):
        self.fit_transform(X)
        return self
