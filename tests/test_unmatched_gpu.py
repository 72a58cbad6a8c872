"""mmvae.unmatched on the MI355X against what the reference recorded in tests/golden/unmatched_clustering.npz
(tools/make_unmatched_fixture.py), with scaling="reference": every assembled and standardised matrix within the z bound of the recorded
one, widened by the imputed block's own bound (tests/unmatched_bounds.py); the neighbourhood hit EQUAL to the record (the fixture's
seed decides every neighbour); the silhouette inside silhouette_bounds' interval with the Lipschitz term in max_i |dZ_i|; the PCA /
t-SNE numbers of a row bit-equal to clustering.PCA / TSNE / silhouette_score / neighborhood_hit called directly on that row's Z (the
pipeline is a composition: its pieces have their own tests).  With scaling="consistent": the RNA block is host log1p of the raw block
bit for bit and the table has the same rows."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import unmatched_bounds as UB  # noqa: E402
import unmatched_ref as UR  # noqa: E402
from evaluate import CLUSTERING_COLUMNS, PCA_COLUMNS, TSNE_COLUMNS, tsne_embedding  # noqa: E402
from mmvae import clustering, ops  # noqa: E402
from mmvae import unmatched as U  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unmatched_clustering.npz")
ROWS = [(st, m) for st in UR.SAMPLE_TYPES for m in UR.IMPUTERS]
TSNE = (250, 42)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_parts(fx, st, method, scaling):
    d = {k: fx[k] for k in ("train_rna", "train_dna", "train_site", "rna_only", "rna_only_site", "dna_only", "dna_only_site")}
    x, site = UR.known(d, st)
    original, site_t = dev(x), dev(site)
    block = U.impute(method, dev(d["train_rna"]), dev(d["train_dna"]), dev(d["train_site"]), U.query_features(st, original, scaling), site_t,
                     U.SAMPLE_TYPES[st], k=UR.K)
    return d, original, block, U.feature_parts(st, original, block, scaling, method), site


@pytest.mark.parametrize("st,method", ROWS)
def test_reference_scaling_against_the_record(fx, st, method):
    key = f"{st}/{method}/"
    F_rec, labels = fx[key + "features"], fx[key + "labels"]
    d, original, block, parts, site = device_parts(fx, st, method, "reference")
    assert np.array_equal(site, labels)
    n0 = original.shape[1]
    if method == "mean":                      # the fp32 rounding of the float64 column mean: within one fp32 ulp of the restatement's
        assert block.dim() == 1 and block.dtype == torch.float32
        want = UR.impute(d, st, "mean", "reference")[0]
        assert np.all(np.abs(block.cpu().numpy().astype(np.float64) - want) <= UB.ulp32(want))
    T = np.concatenate([np.zeros((len(F_rec), n0)), UB.block_tol(F_rec[:, n0:], method, UR.K, log1p_on_top=st == "DNA-only")], axis=1)
    rows, F = F_rec.shape
    z64, tol = UB.z_tol_record(F_rec, T, ops.standardize_fit_splits(rows, F))
    Z = clustering.StandardScaler().fit_transform(parts)
    err = np.abs(Z.cpu().numpy().astype(np.float64) - fx[key + "Z"].astype(np.float64))
    print(f"{key} Z against the record: max err {err.max():.3e}, max err / tol {np.max(err / tol):.3f}")
    assert np.all(err <= tol)

    e = {}
    row = U.judge(parts, dev(labels), tsne=TSNE, embeddings=e)
    assert tuple(row) == CLUSTERING_COLUMNS + PCA_COLUMNS + TSNE_COLUMNS
    # equal as a count of hits among the rows x 5 neighbours: the two means of means are float64 sums in different orders (torch on the
    # device, numpy in the reference) and may differ in the last bit
    hits = float(fx[key + "nh"]) * 5 * rows
    assert abs(hits - round(hits)) < 1e-9 and abs(row["NeighborhoodHit"] * 5 * rows - round(hits)) < 1e-9
    # the silhouette: rows of the device's Z lie within |tol_i| (euclidean) of the float64 z of the recorded features, plus the record's
    # own distance from it
    row_err = np.sqrt((tol ** 2).sum(axis=1))
    lo, hi = UB.silhouette_interval(z64, labels, row_err, ops.silhouette_splits(rows, len(np.unique(labels))))
    print(f"{key} silhouette {row['Silhouette']:.6f} in [{lo:.6f}, {hi:.6f}], recorded {float(fx[key + 'sil']):.6f}")
    assert lo <= row["Silhouette"] <= hi and lo <= float(fx[key + "sil"]) <= hi

    # the composition, bit for bit
    lab = dev(labels)
    p = clustering.PCA(2)
    Y = p.fit_transform(Z)
    assert row["PCASilhouette"] == clustering.silhouette_score(Y, lab) and row["PCANeighborhoodHit"] == clustering.neighborhood_hit(Y, lab, k=5)
    assert row["PCAExplained"] == float(p.explained_variance_ratio_.sum())
    assert row["Silhouette"] == clustering.silhouette_score(Z, lab)
    Yt = tsne_embedding(Z, 30, *TSNE)
    assert row["TSNESilhouette"] == clustering.silhouette_score(Yt, lab) and row["TSNENeighborhoodHit"] == clustering.neighborhood_hit(Yt, lab, k=5)
    assert np.array_equal(e["pca"], Y.cpu().numpy()) and np.array_equal(e["tsne"], Yt.cpu().numpy()) and e["tsne"].shape == (rows, 2)


def test_consistent_scaling(fx):
    for st, method in ROWS:
        d, original, block, parts, site = device_parts(fx, st, method, "consistent")
        want = UR.features(d, st, method, "consistent")
        n0 = original.shape[1]
        assert np.array_equal(parts[0].cpu().numpy().view(np.int32), want[:, :n0].view(np.int32))             # host log1p, bit for bit
        if st == "RNA-only":
            assert np.array_equal(parts[0].cpu().numpy(), np.log1p(original.cpu().numpy()))
        row = U.judge(parts, dev(site), tsne=None)
        assert tuple(row) == CLUSTERING_COLUMNS + PCA_COLUMNS


def test_judge_skips_with_a_message_and_embeds_without_labels(fx, capsys):
    x = dev(fx["dna_only"])
    assert U.judge([x], torch.zeros(len(x), dtype=torch.int64), tsne=None) is None                         # one label
    assert U.judge([x[:4]], torch.tensor([0, 1, 0, 1]), tsne=None) is None                                 # rows < k + 1
    assert U.judge([x], torch.arange(len(x)), tsne=None) is None                                           # as many labels as rows
    assert capsys.readouterr().out.count("not judged") == 3
    e = {}
    assert U.judge([x], None, tsne=None, embeddings=e) is None and e["pca"].shape == (len(x), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.impute("mean", x.cpu(), x.cpu(), None, x.cpu(), None, "rna2dna")
    with pytest.raises(ValueError):
        U.impute("median", x, x, None, x, None, "rna2dna")
