"""Exact PCA on the device: the subset of sklearn.decomposition.PCA that the reference's perform_dimensionality_reduction uses
(src/clustering_evaluation/cluster_imputation_methods.py:140-187: PCA(n_components=2, random_state=42) on the standardised features,
and a PCA(50) in front of t-SNE).

    pca = PCA(n_components=2, random_state=42)
    Y = pca.fit_transform(Z)                       # Z: fp32 or bf16 (N, F) on the device; Y: fp32 (N, 2) on the device
    pca.components_, pca.explained_variance_ratio_

The two passes over the data are this project's kernels: the centred F x F scatter matrix (mmvae_pca_scatter, O(N F^2), the
fp32-rounded column mean subtracted on load) and the projection onto the components (mmvae_pca_project, O(N F k)).  No centred and no
double copy of X exists.  Between them the F x F scatter matrix is eigen-decomposed in float64 by torch.linalg.eigh on the device: a
library call on purpose.  Exact solver only (sklearn's "full" / "covariance_eigh"); no whiten, no inverse_transform."""
import torch

from . import _lib as L
from . import ops

__all__ = ["PCA"]

_EXACT = ("auto", "full", "covariance_eigh")


class PCA:
    def __init__(self, n_components, *, svd_solver="auto", whiten=False, random_state=None):
        if isinstance(n_components, bool) or not isinstance(n_components, int):
            raise ValueError(f"n_components={n_components!r} must be an int")
        if not 1 <= n_components <= L.PCA_MAXK:
            raise ValueError(f"n_components={n_components} outside [1, {L.PCA_MAXK}] (MMVAE_PCA_MAXK)")
        if svd_solver not in _EXACT:
            raise ValueError(f"svd_solver={svd_solver!r}: only the exact solver is implemented ({', '.join(map(repr, _EXACT))})")
        if whiten:
            raise ValueError("whiten=True is not implemented")
        self.n_components, self.svd_solver, self.whiten = n_components, svd_solver, False
        self.random_state = random_state                    # accepted and ignored: the exact solver draws nothing
        self.mean_ = self.components_ = None

    def fit(self, X):
        X = ops._device_matrix(X, "X", "mmvae.pca")
        N, F = X.shape
        k = self.n_components
        if N < 2:
            raise ValueError(f"PCA needs at least 2 samples, got n_samples={N}")
        if k > min(N, F):
            raise ValueError(f"n_components={k} must be between 0 and min(n_samples, n_features)={min(N, F)} with svd_solver='full'")
        self.mean_ = ops._column_means(X)
        S = ops.pca_scatter(X, self.mean_)
        lam, vec = torch.linalg.eigh(S.double())            # ascending
        lam = lam.clamp_min(0.0).flip(0)[:k]
        comp = vec.flip(1)[:, :k].T                         # (k, F), descending
        # sklearn >= 1.5's svd_flip(u_based_decision=False): a component's entry of largest magnitude is positive
        big = comp.gather(1, comp.abs().argmax(dim=1, keepdim=True))
        comp = comp * torch.where(big < 0, -torch.ones_like(big), torch.ones_like(big))
        self.components_ = comp.float().contiguous()
        self.explained_variance_ = lam / (N - 1)
        self.explained_variance_ratio_ = lam / S.diagonal().double().sum()
        self.singular_values_ = lam.sqrt()
        self.n_samples_, self.n_features_in_, self.n_components_ = N, F, k
        return self

    def transform(self, X):
        if self.components_ is None:
            raise RuntimeError("transform() before fit()")
        X = ops._device_matrix(X, "X", "mmvae.pca")
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, PCA was fitted with {self.n_features_in_}")
        return ops.pca_project(X, self.mean_, self.components_)

    def fit_transform(self, X):
        return self.fit(X).transform(X)
