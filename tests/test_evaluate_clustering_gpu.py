"""evaluate.py --clustering on the MI355X at the tiny dims of tests/test_evaluate_knn_gpu.py: without the flag run() returns what it
returned before, with it the expected (Features, Model) rows appear in order, and the rows that need no model -- the true features and
the mean imputation -- carry the silhouette of the float64 restatement (tests/silhouette_ref.py on float64 standardised features)
within the derived bounds (tests/silhouette_bounds.py) and the neighbourhood hit of tests/knn_ref.py (every query decided under
tests/knn_bounds.py)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate  # noqa: E402
import knn_bounds as KB  # noqa: E402
import knn_ref as KR  # noqa: E402
import silhouette_bounds as SB  # noqa: E402
import silhouette_ref as SR  # noqa: E402
import trainer  # noqa: E402
from mmvae import ops  # noqa: E402
from src.config import Config  # noqa: E402
from src.models import MultiModalVAE, RNA2DNAVAE  # noqa: E402

A, D, S, L, N, K = 40, 24, 5, 8, 300, 5
DIMS = ["--samples", str(N), "--input-dim-a", str(A), "--input-dim-b", str(D), "--n-sites", str(S), "--latent-dim", str(L)]
U = 2.0 ** -24


@pytest.fixture(scope="module")
def data():
    tpm, beta_v, site = trainer.synthetic_dataset(N, A, D, S, Config.RANDOM_SEED)
    val_idx, train_idx = trainer.split_indices(N)
    x = {"a": tpm.numpy(), "b": beta_v.numpy()}
    return dict(val={m: x[m][val_idx] for m in x}, train={m: x[m][train_idx] for m in x}, site_val=site[val_idx].numpy())


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt")
    torch.manual_seed(3)
    out = {}
    for kind, cls in (("rna2dna", RNA2DNAVAE), ("multimodal", MultiModalVAE)):
        out[kind] = str(d / f"{kind}.pt")
        torch.save(cls(A, D, S, L).state_dict(), out[kind])
    return out


def keys(rows, *names):
    return [tuple(r[n] for n in names) for r in rows]


def check_numbers(row, feats, site, label):
    """feats: float64 (rows, A + D) features before standardisation"""
    z = SR.standardize(feats)
    z32 = z.astype(np.float32)
    values, codes = np.unique(site, return_inverse=True)
    n, C = len(z), len(values)
    # the device standardises in float64 as well and rounds to fp32: its rows lie within 2 u |z_i| of z (u for the rounding, u for
    # the order of the float64 sums, which is of the order of 1e-16)
    an = SB.analyse(z, codes, C, SR.column_means(z32), ops.silhouette_splits(n, C, 0), row_perturbation=2.0 * U * np.sqrt((z * z).sum(axis=1)))
    width = np.maximum(an["s_hi"] - an["s"], an["s"] - an["s_lo"]).mean()
    want = SR.silhouette_score(z, site)
    print(f"{label}: Silhouette {row['Silhouette']!r} want {want!r} bound {width:.3e}")
    assert abs(row["Silhouette"] - want) <= width
    shift = z32.astype(np.float64).mean(axis=0).astype(np.float32)
    assert KB.analyse(z32, z32, K + 1, shift)["decided"].all()                     # then the hit is a count of exact sets
    nh = KR.neighborhood_hit(z32, site, K)
    print(f"{label}: NeighborhoodHit {row['NeighborhoodHit']!r} want {nh!r}")
    assert row["NeighborhoodHit"] == pytest.approx(nh, abs=1e-12)


@pytest.mark.parametrize("kind", ["rna2dna", "multimodal"])
def test_clustering_table(kind, data, checkpoints, tmp_path):
    common = DIMS + ["--batch-size", "32", "--precision", "fp32", "--checkpoint", checkpoints[kind]]
    plain = evaluate.run(kind, common)
    assert isinstance(plain, list) and len(plain) == {"rna2dna": 2, "multimodal": 6}[kind]   # what run() returned before the flag existed
    assert all(set(r) == {"Route", "Modality", "Model"} | set(evaluate.COLUMNS) for r in plain)
    again, none = evaluate.run(kind, common, return_clustering=True)
    assert none == [] and keys(again, "Route", "Modality", "Model") == keys(plain, "Route", "Modality", "Model")
    out = tmp_path / "clustering.json"
    rows, crows = evaluate.run(kind, common + ["--clustering", "--knn", str(K), "--knn-by-site", "--clustering-out", str(out)], return_clustering=True)
    assert keys(rows[:len(plain)], "Route", "Modality", "Model") == keys(plain, "Route", "Modality", "Model")
    title = trainer.KINDS[kind]["title"]
    imputations = {"rna2dna": [("rna+site->dna", "a", "b")], "multimodal": [("a->b", "a", "b"), ("b->a", "b", "a")]}[kind]
    expect = [("a|b", "original")]
    for route, src, tgt in imputations:
        expect += [(route, title), (route, "MeanImputation"), (f"{src}->{tgt}", f"kNN(k={K})"), (f"{src}+site->{tgt}", f"kNN-site(k={K})")]
    assert keys(crows, "Features", "Model") == expect
    assert all(set(r) == {"Features", "Model", "Silhouette", "NeighborhoodHit"} for r in crows)
    assert all(-1.0 <= r["Silhouette"] <= 1.0 and 0.0 <= r["NeighborhoodHit"] <= 1.0 for r in crows)
    assert json.loads(out.read_text()) == crows
    got = {(r["Features"], r["Model"]): r for r in crows}
    val = {m: data["val"][m].astype(np.float64) for m in "ab"}
    check_numbers(got[("a|b", "original")], np.hstack([val["a"], val["b"]]), data["site_val"], f"{kind} original")
    for route, src, tgt in imputations:
        mean = torch.from_numpy(data["train"][tgt]).double().mean(dim=0).float().numpy().astype(np.float64)
        parts = dict(val)
        parts[tgt] = np.broadcast_to(mean, val[tgt].shape)
        check_numbers(got[(route, "MeanImputation")], np.hstack([parts["a"], parts["b"]]), data["site_val"], f"{kind} {route} mean")


def test_flags_that_need_clustering(checkpoints, tmp_path):
    with pytest.raises(SystemExit):
        evaluate.run("rna2dna", DIMS + ["--checkpoint", checkpoints["rna2dna"], "--clustering-out", str(tmp_path / "x.json")])


def test_one_site_skips_the_table(checkpoints, capsys):
    dims = ["--samples", str(N), "--input-dim-a", str(A), "--input-dim-b", str(D), "--n-sites", "1", "--latent-dim", str(L)]
    torch.manual_seed(3)
    path = checkpoints["rna2dna"].replace("rna2dna.pt", "one_site.pt")
    torch.save(RNA2DNAVAE(A, D, 1, L).state_dict(), path)
    rows, crows = evaluate.run("rna2dna", dims + ["--batch-size", "32", "--precision", "fp32", "--checkpoint", path, "--clustering"], return_clustering=True)
    assert crows == [] and len(rows) == 2
    assert "clustering table skipped" in capsys.readouterr().out
