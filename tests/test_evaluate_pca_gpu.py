"""evaluate.py --clustering-pca on the MI355X at the tiny dims of tests/test_evaluate_clustering_gpu.py: without the flag the clustering
rows are what they were, with --clustering-pca 2 every row gains PCASilhouette, PCANeighborhoodHit and PCAExplained, and for the rows
that need no model -- the true features and the mean imputation -- PCAExplained matches the float64 restatement (tests/pca_ref.py)
within the eigenvalue bound of tests/pca_bounds.py and the two PCA numbers equal, bit for bit, what mmvae.clustering gives on
PCA(2).fit_transform(standardize(features)) recomputed by the test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate  # noqa: E402
import pca_bounds as PB  # noqa: E402
import trainer  # noqa: E402
from mmvae import clustering  # noqa: E402
from src.config import Config  # noqa: E402
from src.models import MultiModalVAE, RNA2DNAVAE  # noqa: E402

A, D, S, L, N, K = 40, 24, 5, 8, 300, 5
DIMS = ["--samples", str(N), "--input-dim-a", str(A), "--input-dim-b", str(D), "--n-sites", str(S), "--latent-dim", str(L)]
PLAIN_KEYS = {"Features", "Model", "Silhouette", "NeighborhoodHit"}
PCA_KEYS = {"PCASilhouette", "PCANeighborhoodHit", "PCAExplained"}


@pytest.fixture(scope="module")
def data():
    tpm, beta_v, site = trainer.synthetic_dataset(N, A, D, S, Config.RANDOM_SEED)
    val_idx, train_idx = trainer.split_indices(N)
    x = {"a": tpm, "b": beta_v}
    return dict(val={m: x[m][val_idx] for m in x}, train={m: x[m][train_idx] for m in x}, site_val=site[val_idx])


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt")
    torch.manual_seed(3)
    out = {}
    for kind, cls in (("rna2dna", RNA2DNAVAE), ("multimodal", MultiModalVAE)):
        out[kind] = str(d / f"{kind}.pt")
        torch.save(cls(A, D, S, L).state_dict(), out[kind])
    return out


def check_row(row, feats, site, label):
    """feats: fp32 (rows, A + D) host tensor, the matrix evaluate.py filled for this row"""
    z = clustering.standardize(feats.to("cuda"))
    labels = site.to("cuda")
    pca = clustering.PCA(2)
    y = pca.fit_transform(z)
    want = (clustering.silhouette_score(y, labels), clustering.neighborhood_hit(y, labels, k=evaluate.NH_K))
    print(f"{label}: PCASilhouette {row['PCASilhouette']!r} want {want[0]!r}, PCANeighborhoodHit {row['PCANeighborhoodHit']!r} want {want[1]!r}")
    assert (row["PCASilhouette"], row["PCANeighborhoodHit"]) == want                 # the kernels are bit-reproducible
    assert row["PCAExplained"] == float(pca.explained_variance_ratio_.sum())
    # against the float64 restatement on the same standardised fp32 matrix
    an = PB.analyse(z.cpu().numpy(), 2)
    lam, t = an["ref"]["lam_all"][:2], np.trace(an["ref"]["S"])
    t_lo = t - an["trace_err"]
    bound = (an["eig"] / t_lo + lam * an["trace_err"] / (t * t_lo)).sum() + 1e-15
    ref = an["ref"]["explained_variance_ratio"].sum()
    print(f"{label}: PCAExplained {row['PCAExplained']!r} want {ref!r} bound {bound:.3e}")
    assert abs(row["PCAExplained"] - ref) <= bound


@pytest.mark.parametrize("kind", ["rna2dna", "multimodal"])
def test_clustering_table_with_pca_columns(kind, data, checkpoints):
    common = DIMS + ["--batch-size", "32", "--precision", "fp32", "--checkpoint", checkpoints[kind], "--clustering"]
    _, plain = evaluate.run(kind, common, return_clustering=True)
    assert plain and all(set(r) == PLAIN_KEYS for r in plain)                        # without the flag: what the rows were
    _, zero = evaluate.run(kind, common + ["--clustering-pca", "0"], return_clustering=True)
    assert all(set(r) == PLAIN_KEYS for r in zero)
    _, crows = evaluate.run(kind, common + ["--clustering-pca", "2"], return_clustering=True)
    assert [(r["Features"], r["Model"]) for r in crows] == [(r["Features"], r["Model"]) for r in plain]
    assert all(set(r) == PLAIN_KEYS | PCA_KEYS for r in crows)
    assert all(-1.0 <= r["PCASilhouette"] <= 1.0 and 0.0 <= r["PCANeighborhoodHit"] <= 1.0 and 0.0 < r["PCAExplained"] <= 1.0 for r in crows)
    got = {(r["Features"], r["Model"]): r for r in crows}
    base = {(r["Features"], r["Model"]): r for r in plain}
    for key in (("a|b", "original"),):                                               # rows without a sampled eps: the flag changes nothing else
        assert all(got[key][c] == base[key][c] for c in evaluate.CLUSTERING_COLUMNS)
    val = data["val"]
    check_row(got[("a|b", "original")], torch.cat([val["a"], val["b"]], dim=1), data["site_val"], f"{kind} original")
    imputations = {"rna2dna": [("rna+site->dna", "b")], "multimodal": [("a->b", "b"), ("b->a", "a")]}[kind]
    for route, tgt in imputations:
        mean = data["train"][tgt].double().mean(dim=0).float()
        parts = dict(val)
        parts[tgt] = mean.expand(val[tgt].shape[0], -1)
        check_row(got[(route, "MeanImputation")], torch.cat([parts["a"], parts["b"]], dim=1), data["site_val"], f"{kind} {route} mean")


def test_the_flag_needs_clustering(checkpoints):
    with pytest.raises(SystemExit):
        evaluate.run("rna2dna", DIMS + ["--checkpoint", checkpoints["rna2dna"], "--clustering-pca", "2"])
    with pytest.raises(SystemExit):
        evaluate.run("rna2dna", DIMS + ["--checkpoint", checkpoints["rna2dna"], "--clustering", "--clustering-pca", "65"])
