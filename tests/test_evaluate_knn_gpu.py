"""evaluate.py --knn K [--knn-by-site] on the MI355X at the tiny dims of tests/test_evaluate_gpu.py: exactly the new rows are added,
their metrics are those of the float64 restatement's neighbours (tests/knn_ref.py; every query of this data is decided under
tests/knn_bounds.py, so the device must return the same sets) within the derived metric bounds (tests/metrics_bounds.py), and without
the flags the table is what it was."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate  # noqa: E402
import knn_bounds as KB  # noqa: E402
import knn_ref as KR  # noqa: E402
import metrics_bounds as MB  # noqa: E402
import metrics_ref as MR  # noqa: E402
import trainer  # noqa: E402
from src.config import Config  # noqa: E402
from src.models import MultiModalVAE, RNA2DNAVAE  # noqa: E402

A, D, S, L, N, K = 40, 24, 5, 8, 300, 5
DIMS = ["--samples", str(N), "--input-dim-a", str(A), "--input-dim-b", str(D), "--n-sites", str(S), "--latent-dim", str(L)]
SCALARS = ("MAE", "MSE", "RMSE", "R2", "MeanR2", "CosineSimilarity", "PearsonMean", "PearsonStd")


@pytest.fixture(scope="module")
def data():
    tpm, beta_v, site = trainer.synthetic_dataset(N, A, D, S, Config.RANDOM_SEED)
    val_idx, train_idx = trainer.split_indices(N)
    x = {"a": tpm.numpy(), "b": beta_v.numpy()}
    return dict(val={m: x[m][val_idx] for m in x}, train={m: x[m][train_idx] for m in x},
                site_val=site[val_idx].numpy(), site_train=site[train_idx].numpy())


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt")
    torch.manual_seed(3)
    out = {}
    for kind, cls in (("rna2dna", RNA2DNAVAE), ("multimodal", MultiModalVAE)):
        out[kind] = str(d / f"{kind}.pt")
        torch.save(cls(A, D, S, L).state_dict(), out[kind])
    return out


def by_key(rows):
    return {(r["Route"], r["Modality"], r["Model"]): r for r in rows}


def check_row(row, y, p, label):
    y, p = np.asarray(y, np.float64), np.asarray(p, np.float64)
    want, tol = MR.metrics(y, p), MB.metrics_tol(y, p, y[0])
    for k in SCALARS:
        print(f"{label} {k}: {row[k]!r} want {want[k]!r} bound {tol[k]:.3e}")
        assert np.isfinite(tol[k]) and abs(row[k] - want[k]) <= tol[k], (label, k, row[k], want[k], tol[k])
    assert row["PearsonValid"] == want["PearsonValid"]


def reference_prediction(data, src, tgt, by_site):
    """the fp32 rows the device path must produce: float64 neighbours (all decided), averaged as the kernel averages"""
    Xt, Yt, Xq = data["train"][src], data["train"][tgt], data["val"][src]
    if not by_site:
        an = KB.analyse(Xq, Xt, K, Xt.astype(np.float64).mean(axis=0).astype(np.float32))
        assert an["decided"].all()
        return KR.mean_rows_f32(an["order"][:, :K], Yt)
    out = np.zeros((Xq.shape[0], Yt.shape[1]), np.float32)
    for s in np.unique(data["site_val"]):
        m, mq = data["site_train"] == s, data["site_val"] == s
        if m.any():
            k = min(K, int(m.sum()))
            an = KB.analyse(Xq[mq], Xt[m], k, Xt[m].astype(np.float64).mean(axis=0).astype(np.float32))
            assert an["decided"].all()
            out[mq] = KR.mean_rows_f32(an["order"][:, :k], Yt[m])
    return out


@pytest.mark.parametrize("kind", ["rna2dna", "multimodal"])
def test_knn_rows_are_added_and_equal_the_reference(kind, data, checkpoints):
    common = DIMS + ["--batch-size", "32", "--precision", "fp32", "--checkpoint", checkpoints[kind]]
    plain = evaluate.run(kind, common)
    rows = evaluate.run(kind, common + ["--knn", str(K), "--knn-by-site"])
    base_keys = [(r["Route"], r["Modality"], r["Model"]) for r in plain]
    assert [(r["Route"], r["Modality"], r["Model"]) for r in rows[:len(plain)]] == base_keys
    assert len(plain) == {"rna2dna": 2, "multimodal": 6}[kind]                       # what the table held before the flags existed
    targets = {"rna2dna": ["b"], "multimodal": ["a", "b"]}[kind]
    names = {"a": "RNA", "b": "DNA"}
    expect = []
    for tgt in targets:
        src = "b" if tgt == "a" else "a"
        expect += [(f"{src}->{tgt}", names[tgt], f"kNN(k={K})", src, tgt, False), (f"{src}+site->{tgt}", names[tgt], f"kNN-site(k={K})", src, tgt, True)]
    assert [(r["Route"], r["Modality"], r["Model"]) for r in rows[len(plain):]] == [e[:3] for e in expect]
    got = by_key(rows)
    for route, modality, model, src, tgt, by_site in expect:
        r = got[(route, modality, model)]
        assert set(r) == {"Route", "Modality", "Model"} | set(evaluate.COLUMNS)
        check_row(r, data["val"][tgt], reference_prediction(data, src, tgt, by_site), f"{kind} {route} {model}")
    # the mean-imputation rows are still the training means' (the metrics launch sums with f64 atomics: equal within its bounds, not bitwise)
    for tgt in targets:
        mean = torch.from_numpy(data["train"][tgt]).double().mean(dim=0).float().numpy()
        pred = np.broadcast_to(mean, data["val"][tgt].shape)
        for table in (plain, rows):
            check_row(by_key(table)[("train mean", names[tgt], "MeanImputation")], data["val"][tgt], pred, f"{kind} mean {tgt}")


def test_knn_by_site_alone_is_refused(checkpoints):
    with pytest.raises(SystemExit):
        evaluate.run("rna2dna", DIMS + ["--checkpoint", checkpoints["rna2dna"], "--knn-by-site"])
