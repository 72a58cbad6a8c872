"""The two numbers the reference judges a clustering with, on the device: silhouette_score(StandardScaler().fit_transform(features),
labels) and calculate_neighborhood_hit (src/clustering_evaluation/cluster_imputation_methods.py:478-504, cluster_reconstructed.py:299-317).

    Z = standardize(features)                      # StandardScaler().fit_transform, fp32 on the device
    Z = StandardScaler().fit_transform([original, imputed])    # the same on mmvae_standardize_fit / _apply: the matrix is assembled from
                                                   # its column blocks while it is standardised (an imputed mean row stays one row)
    s = silhouette_samples(Z, labels)              # fp32 (N,) on the device
    score = silhouette_score(Z, labels)            # Python float
    nh = neighborhood_hit(Z, labels, k=5)
    Y = PCA(n_components=2).fit_transform(Z)       # mmvae.pca: the table's second part, the same two numbers on Y
    T = TSNE(n_components=2, perplexity=30.0, random_state=42).fit_transform(PCA(50).fit_transform(Z))    # mmvae.tsne: its third

The silhouette runs on mmvae_silhouette_samples (a fp32 MFMA distance GEMM whose epilogue is a square root and a per-class row sum: the
N x N distances never exist).  Euclidean metric only, no sample_size (nothing in the reference uses either)."""
import torch

from . import _lib as L
from . import ops
from .knn import neighborhood_hit  # noqa: F401  (neighborhood_hit: re-exported)
from .pca import PCA  # noqa: F401  (re-exported: the table's PCA columns)
from .tsne import TSNE  # noqa: F401  (re-exported: the table's t-SNE columns)

__all__ = ["silhouette_samples", "silhouette_score", "standardize", "StandardScaler", "neighborhood_hit", "PCA", "TSNE", "judge_matrix",
           "can_judge", "tsne_embedding", "CLUSTERING_COLUMNS", "PCA_COLUMNS", "TSNE_COLUMNS", "TSNE_PCA_K", "NH_K"]

CLUSTERING_COLUMNS = ("Silhouette", "NeighborhoodHit")
PCA_COLUMNS = ("PCASilhouette", "PCANeighborhoodHit", "PCAExplained")
TSNE_COLUMNS = ("TSNESilhouette", "TSNENeighborhoodHit")
TSNE_PCA_K = 50                                              # the reference reduces to 50 components in front of t-SNE
NH_K = 5


def _encode(labels, N, device):
    """(order int32 (N,), class_start int32 (C + 1,)) of any integer labels: codes by torch.unique, a class's rows in their own order"""
    labels = torch.as_tensor(labels)
    if labels.dim() != 1 or labels.shape[0] != N or labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
        raise ValueError(f"labels must be an integer ({N},) tensor or array")
    values, codes, counts = torch.unique(labels.to(device), return_inverse=True, return_counts=True)
    n_labels = values.shape[0]
    if not 1 < n_labels < N:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % n_labels)
    if n_labels > L.SIL_MAXC:
        raise ValueError(f"Number of labels is {n_labels}: at most {L.SIL_MAXC} (MMVAE_SIL_MAXC) are supported")
    order = torch.argsort(codes, stable=True).to(torch.int32)
    class_start = torch.zeros(n_labels + 1, dtype=torch.int32, device=device)
    class_start[1:] = torch.cumsum(counts, 0)
    return order, class_start


def silhouette_samples(X, labels, metric="euclidean"):
    """sklearn.metrics.silhouette_samples(X, labels) as an fp32 (N,) device tensor."""
    if metric != "euclidean":
        raise ValueError(f"metric={metric!r}: only 'euclidean' is implemented")
    if not isinstance(X, torch.Tensor) or not X.is_cuda:
        raise RuntimeError("mmvae.clustering: X must be a CUDA/HIP tensor; there is no CPU fallback")
    X = ops._device_matrix(X, "X", "mmvae.clustering")
    order, class_start = _encode(labels, X.shape[0], X.device)
    return ops.silhouette_samples(X, order, class_start, ops._column_means(X))[0]


def silhouette_score(X, labels, metric="euclidean"):
    """sklearn.metrics.silhouette_score(X, labels): the mean of the samples, in float64."""
    return float(silhouette_samples(X, labels, metric).double().mean())


def standardize(X):
    """StandardScaler().fit_transform(X): float64 column mean and population variance, a zero-variance (constant) column keeps scale 1; fp32,
    contiguous, on X's device."""
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError("standardize: X must be a 2-D tensor")
    Xd = X.detach().double()
    mean = Xd.mean(dim=0)
    var = Xd.var(dim=0, unbiased=False)
    # a constant column's variance is zero up to the rounding of its mean: sklearn's bound (_is_constant_feature)
    n, eps = Xd.shape[0], torch.finfo(torch.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = torch.where(constant, torch.ones_like(var), var.sqrt())
    return ((Xd - mean) / scale).float().contiguous()


class StandardScaler:
    """sklearn.preprocessing.StandardScaler() (with_mean, with_std) on mmvae_standardize_fit / mmvae_standardize_apply.  `parts` is one
    tensor or a sequence of up to four column blocks of the feature matrix: each a 2-D fp32 / bf16 device matrix, or a 1-D tensor, one
    row that stands for every sample (a mean imputation); the row count is that of the matrix parts, of which there is at least one.
    mean_, var_, scale_: float64 (F,) device tensors; transform gives fp32 (rows, F), contiguous."""

    def __init__(self):
        self.mean_ = self.var_ = self.scale_ = self.n_samples_seen_ = None

    @staticmethod
    def _parts(parts):
        """the parts detached; what they must be is checked in one place, ops._std_parts"""
        parts = (parts,) if isinstance(parts, torch.Tensor) else tuple(parts)
        return tuple(t.detach() if isinstance(t, torch.Tensor) else t for t in parts)

    def fit(self, parts):
        parts = self._parts(parts)
        self.mean_, self.var_, self.scale_ = ops.standardize_fit(parts)
        self.n_samples_seen_ = next(t.shape[0] for t in parts if t.dim() == 2)
        return self

    def transform(self, parts):
        if self.mean_ is None:
            raise RuntimeError("StandardScaler.transform before fit")
        return ops.standardize_apply(self._parts(parts), self.mean_, self.scale_)

    def fit_transform(self, parts):
        return self.fit(parts).transform(parts)


def tsne_embedding(z, perplexity, iters, seed):
    """The reference's t-SNE of a standardised matrix: PCA(50) first when it has more than 50 columns, perplexity capped at rows - 1."""
    if z.shape[1] > TSNE_PCA_K:
        z = PCA(TSNE_PCA_K).fit_transform(z)
    return TSNE(2, perplexity=min(perplexity, z.shape[0] - 1), max_iter=iters, random_state=seed).fit_transform(z)


def can_judge(n_labels, rows):                              # the silhouette's label-count guard
    return 2 <= n_labels <= min(rows - 1, L.SIL_MAXC)


def judge_matrix(z, labels, *, pca_k=0, tsne=None, k=NH_K, embeddings=None):
    """One table row of a standardised matrix z, computed in column order: silhouette and neighbourhood hit (k) on z; pca_k > 0: on its
    first pca_k principal components, with their explained-variance share; tsne = (perplexity, iterations, seed): on tsne_embedding(z).
    embeddings: a dict that receives "pca" / "tsne" (host arrays).  labels=None: nothing is judged, z is only embedded."""
    def judged(y):
        return () if labels is None else (silhouette_score(y, labels), neighborhood_hit(y, labels, k=k))

    row = dict(zip(CLUSTERING_COLUMNS, judged(z)))
    if pca_k > 0:
        pca = PCA(pca_k)
        y = pca.fit_transform(z)
        row.update(zip(PCA_COLUMNS, judged(y) + (float(pca.explained_variance_ratio_.sum()),)))
        if embeddings is not None:
            embeddings["pca"] = y.cpu().numpy()
    if tsne is not None:
        y = tsne_embedding(z, *tsne)
        row.update(zip(TSNE_COLUMNS, judged(y)))
        if embeddings is not None:
            embeddings["tsne"] = y.cpu().numpy()
    return row
