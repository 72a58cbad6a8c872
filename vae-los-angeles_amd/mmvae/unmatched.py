"""Clustering of the UNMATCHED samples on the device: the reference's src/clustering_evaluation/cluster_imputation_methods.py and
cluster_reconstructed.py without the plotting.  An RNA-only sample gets its DNA imputed, a DNA-only sample its RNA; the [original |
imputed] feature matrix is standardised (mmvae.clustering.StandardScaler assembles it from its two column blocks) and judged by the
silhouette and the neighbourhood hit on the features, on their PCA(2) and on the t-SNE of their PCA(50).

    imputed = impute("knn", train_rna, train_dna, train_site, query, query_site, "rna2dna", k=5)   # "mean": a 1-D row
    parts = feature_parts("RNA-only", original, imputed, scaling="consistent")
    row = judge(parts, labels, tsne=(250, 42))                                                      # one table row, or None + message

Scaling of RNA.  processed_data.pkl holds log1p(TPM), the unmatched RNA file raw TPM.  scaling="consistent" (default): unmatched RNA is
log1p'd as reconstruct.py does, before it queries the training set and before it is clustered, and imputed RNA stays on the training
(log) scale: the four methods are comparable.  scaling="reference": the reference's arithmetic verbatim -- raw TPM queries the
log-scale training set and is clustered raw, and imputed RNA of mean / knn / cond_knn gets a log1p on top of the log scale
(cluster_imputation_methods.py:290,333,408); the VAE's reconstructed RNA is clustered as written (cluster_reconstructed.py:130).
Every log1p is numpy's on the host, on float32, as in reconstruct.py."""
import numpy as np
import torch

from . import _lib as L
from . import clustering, ops
from .knn import ConditionedKNeighborsRegressor, KNeighborsRegressor

METHODS = ("mean", "knn", "cond_knn", "vae")
IMPUTERS = METHODS[:3]
DIRECTIONS = ("rna2dna", "dna2rna")
SAMPLE_TYPES = {"RNA-only": "rna2dna", "DNA-only": "dna2rna"}
SCALINGS = ("consistent", "reference")

__all__ = ["impute", "query_features", "feature_parts", "judge", "log1p_host", "METHODS", "SCALINGS", "SAMPLE_TYPES"]


def log1p_host(t):
    """numpy's log1p of a float32 device tensor, on the host (no device transcendental enters any bound)"""
    return torch.from_numpy(np.log1p(t.detach().float().cpu().numpy())).to(t.device)


def _check(value, allowed, what):
    if value not in allowed:
        raise ValueError(f"{what}={value!r}: one of {tuple(allowed)}")


def query_features(sample_type, original, scaling="consistent"):
    """What an imputer (or a model) is queried with: unmatched RNA is raw TPM -- log1p'd under "consistent", as it is under "reference"."""
    _check(sample_type, SAMPLE_TYPES, "sample_type")
    _check(scaling, SCALINGS, "scaling")
    return log1p_host(original) if sample_type == "RNA-only" and scaling == "consistent" else original


def impute(method, train_a, train_b, train_site, query, query_site, direction, k=5):
    """The missing modality of `query` from the matched training set (a = RNA, b = DNA; direction "rna2dna": features a, targets b).
    "mean": a 1-D fp32 row, the fp32 rounding of the float64 column mean of the training target (SimpleImputer(strategy="mean")
    .statistics_.astype(float32)), from mmvae_standardize_fit.  "knn": KNeighborsRegressor(k).  "cond_knn":
    ConditionedKNeighborsRegressor(k) on the int64 site vectors; a query whose site has no training rows gets zeros
    (conditioned_knn.py:78-85)."""
    _check(method, IMPUTERS, "method")
    _check(direction, DIRECTIONS, "direction")
    X, Y = (train_a, train_b) if direction == "rna2dna" else (train_b, train_a)
    ops._no_cpu(Y, "train", "mmvae.unmatched")
    if method == "mean":
        return ops.standardize_fit(ops._device_matrix(Y, "train", "mmvae.unmatched"))[0].float()
    ops._no_cpu(query, "query", "mmvae.unmatched")
    if method == "knn":
        return KNeighborsRegressor(k).fit(X, Y).predict(query)
    if train_site is None or query_site is None:
        raise ValueError("cond_knn needs train_site and query_site")
    return ConditionedKNeighborsRegressor(k).fit(X, Y, train_site).predict(query, query_site)


def feature_parts(sample_type, original, imputed, scaling="consistent", method="knn"):
    """[original | imputed] as the two column blocks StandardScaler takes.  `imputed` is a matrix, or a 1-D row (mean imputation)."""
    _check(sample_type, SAMPLE_TYPES, "sample_type")
    _check(scaling, SCALINGS, "scaling")
    _check(method, METHODS, "method")
    if sample_type == "RNA-only":
        return [query_features(sample_type, original, scaling), imputed]
    if scaling == "reference" and method != "vae":
        imputed = log1p_host(imputed)
    return [original, imputed]


def judge(parts, labels, pca=True, tsne=None, k=clustering.NH_K, embeddings=None):
    """One table row of the feature matrix whose column blocks are `parts`, or None with a printed message where the labels allow no
    silhouette.  Z = StandardScaler().fit_transform(parts); silhouette and neighbourhood hit (k) on Z; with pca on PCA(2) of Z, with
    the explained-variance sum; with tsne = (iterations, seed) on the t-SNE of Z by perform_dimensionality_reduction's rule (PCA(50) first
    only above 50 columns, perplexity min(30, rows - 1)).  embeddings: a dict that receives "pca" / "tsne" (host arrays).  labels=None
    (a DNA-only frame without primary_site): the samples are embedded, nothing is judged, None is returned."""
    parts = (parts,) if isinstance(parts, torch.Tensor) else tuple(parts)
    rows = next((t.shape[0] for t in parts if isinstance(t, torch.Tensor) and t.dim() == 2), 0)
    if labels is not None:
        labels = torch.as_tensor(labels)
        if labels.dim() != 1 or labels.shape[0] != rows:
            raise ValueError(f"labels must be ({rows},)")
        n_labels = int(torch.unique(labels).numel())
        if not clustering.can_judge(n_labels, rows):
            print(f"  not judged: {n_labels} distinct label(s) among {rows} rows (need 2 .. min(rows - 1, {L.SIL_MAXC}))")
            return None
        if rows < k + 1:
            print(f"  not judged: {rows} rows, the neighbourhood hit needs {k + 1}")
            return None
    z = clustering.StandardScaler().fit_transform(parts)
    labels = None if labels is None else labels.to(z.device)
    wanted = labels is not None or embeddings is not None          # without labels the projections only serve `embeddings`
    row = clustering.judge_matrix(z, labels, pca_k=min(2, z.shape[1]) if pca and wanted else 0,
                                  tsne=(30, *tsne) if tsne is not None and rows >= 2 and wanted else None, k=k, embeddings=embeddings)
    return row if labels is not None else None
