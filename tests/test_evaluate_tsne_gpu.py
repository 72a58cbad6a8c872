"""evaluate.py --clustering-tsne on the MI355X at the tiny dims of tests/test_evaluate_pca_gpu.py (64 features: the PCA(50) in front of
t-SNE runs): every clustering row gains TSNESilhouette and TSNENeighborhoodHit, finite; for the rows that need no model they equal, bit
for bit, what mmvae.clustering gives on the test's own TSNE(PCA(50)(standardize(features))); every other cell of both tables is what a
run without the flag prints."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate  # noqa: E402
import trainer  # noqa: E402
from mmvae import clustering, engine  # noqa: E402
from src.config import Config  # noqa: E402
from src.models import MultiModalVAE  # noqa: E402

A, D, S, L, N, ITERS = 40, 24, 5, 8, 2048, 300
DIMS = ["--samples", str(N), "--input-dim-a", str(A), "--input-dim-b", str(D), "--n-sites", str(S), "--latent-dim", str(L)]
TSNE_KEYS = {"TSNESilhouette", "TSNENeighborhoodHit"}


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ckpt") / "multimodal.pt")
    torch.manual_seed(3)
    torch.save(MultiModalVAE(A, D, S, L).state_dict(), path)
    return path


@pytest.fixture(scope="module")
def tables(checkpoint):
    common = DIMS + ["--batch-size", "128", "--precision", "fp32", "--checkpoint", checkpoint, "--clustering", "--clustering-pca", "2"]
    # each run from the same position of the Philox stream that eps is drawn from, as two invocations of the tool start: otherwise the
    # model's rows differ between any two runs of one process, with or without the flag
    dev = torch.device("cuda", torch.cuda.current_device())
    start = engine.GLOBAL_NOISE.state_dict(dev)
    plain = evaluate.run("multimodal", common, return_clustering=True)
    engine.GLOBAL_NOISE.load_state_dict(start, dev)
    with_tsne = evaluate.run("multimodal", common + ["--clustering-tsne", "--tsne-iters", str(ITERS)], return_clustering=True)
    return plain, with_tsne


def test_new_columns_are_present_and_finite_and_nothing_else_changes(tables):
    (rows0, crows0), (rows1, crows1) = tables
    # the imputation table does not know the flag.  Its float columns come from float64 sums that mmvae_recon_metrics accumulates with
    # atomics: the order of at most 410 additions per sum differs between any two runs (410 x 2^-53 = 5e-14 of the sum of magnitudes;
    # 1e-15 was seen), so those compare to 1e-10 -- far below anything a changed input would do -- and everything else exactly
    assert len(rows1) == len(rows0) == 6
    for r0, r1 in zip(rows0, rows1):
        assert set(r1) == set(r0) and all(r1[k] == r0[k] for k in ("Route", "Modality", "Model", "PearsonValid"))
        assert all(r1[k] == pytest.approx(r0[k], rel=1e-10, abs=1e-10) for k in evaluate.COLUMNS), (r0, r1)
    assert len(crows1) == len(crows0) == 5
    for r0, r1 in zip(crows0, crows1):
        assert set(r1) == set(r0) | TSNE_KEYS and not TSNE_KEYS & set(r0)
        assert all(r1[k] == r0[k] for k in r0), (r0, r1)
        assert all(math.isfinite(r1[k]) for k in TSNE_KEYS)
        assert -1.0 <= r1["TSNESilhouette"] <= 1.0 and 0.0 <= r1["TSNENeighborhoodHit"] <= 1.0


def test_new_columns_equal_the_tests_own_recomputation(tables):
    crows = {(r["Features"], r["Model"]): r for r in tables[1][1]}
    tpm, beta_v, site = trainer.synthetic_dataset(N, A, D, S, Config.RANDOM_SEED)
    val_idx, train_idx = trainer.split_indices(N)
    val = {"a": tpm[val_idx], "b": beta_v[val_idx]}
    labels = site[val_idx].to("cuda")
    cases = [(("a|b", "original"), dict(val))]
    for route, tgt, src in (("a->b", "b", beta_v), ("b->a", "a", tpm)):
        parts = dict(val)
        parts[tgt] = src[train_idx].double().mean(dim=0).float().expand(val[tgt].shape[0], -1)
        cases.append(((route, "MeanImputation"), parts))
    for key, parts in cases:
        z = clustering.standardize(torch.cat([parts["a"], parts["b"]], dim=1).to("cuda"))
        assert z.shape[1] == 64 > evaluate.TSNE_PCA_K
        y = clustering.TSNE(2, perplexity=30.0, max_iter=ITERS, random_state=Config.RANDOM_SEED).fit_transform(clustering.PCA(50).fit_transform(z))
        want = (clustering.silhouette_score(y, labels), clustering.neighborhood_hit(y, labels, k=evaluate.NH_K))
        print(f"{key}: TSNESilhouette {crows[key]['TSNESilhouette']!r} want {want[0]!r}, TSNENeighborhoodHit {crows[key]['TSNENeighborhoodHit']!r} "
              f"want {want[1]!r}")
        assert (crows[key]["TSNESilhouette"], crows[key]["TSNENeighborhoodHit"]) == want     # every kernel on the way is bit-reproducible


def test_the_flags_are_checked(checkpoint):
    base = DIMS + ["--checkpoint", checkpoint]
    for extra in (["--clustering-tsne"], ["--clustering", "--clustering-tsne", "--tsne-iters", "100"],
                  ["--clustering", "--clustering-tsne", "--tsne-perplexity", "0"]):
        with pytest.raises(SystemExit):
            evaluate.run("multimodal", base + extra)
