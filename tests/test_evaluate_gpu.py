"""evaluate.py on the MI355X at tiny dims: the JSON it writes, the split it evaluates, the mean-imputation row and the model rows
against the float64 restatement (tests/metrics_ref.py) within the derived bounds (tests/metrics_bounds.py)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate  # noqa: E402
import metrics_bounds as MB  # noqa: E402
import metrics_ref as MR  # noqa: E402
import trainer  # noqa: E402
from mmvae import engine  # noqa: E402
from src.config import Config  # noqa: E402
from src.models import MultiModalVAE, RNA2DNAVAE  # noqa: E402

DEV = "cuda"
A, D, S, L, N = 40, 24, 5, 8, 300
DIMS = ["--samples", str(N), "--input-dim-a", str(A), "--input-dim-b", str(D), "--n-sites", str(S), "--latent-dim", str(L)]
SCALARS = ("MAE", "MSE", "RMSE", "R2", "MeanR2", "CosineSimilarity", "PearsonMean", "PearsonStd")


@pytest.fixture(scope="module")
def data():
    """the synthetic dataset of the trainers and THEIR validation split, built here from the trainer's own pieces"""
    tpm, beta_v, site = trainer.synthetic_dataset(N, A, D, S, Config.RANDOM_SEED)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(Config.RANDOM_SEED))
    n_val = int(N * Config.TRAIN_TEST_SPLIT)
    val_idx, train_idx = trainer.split_indices(N)
    assert torch.equal(val_idx, perm[:n_val]) and torch.equal(train_idx, perm[n_val:])       # the split trainer.run used before the helper
    return dict(a=tpm[val_idx].numpy(), b=beta_v[val_idx].numpy(), site=site[val_idx],
                mean_a=tpm[train_idx].double().mean(dim=0).float().numpy(), mean_b=beta_v[train_idx].double().mean(dim=0).float().numpy())


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt")
    torch.manual_seed(3)
    out = {}
    for kind, cls in (("rna2dna", RNA2DNAVAE), ("multimodal", MultiModalVAE)):
        out[kind] = str(d / f"{kind}.pt")
        torch.save(cls(A, D, S, L).state_dict(), out[kind])
    return out


def check_row(row, y, p, label):
    y, p = np.asarray(y, np.float64), np.asarray(p, np.float64)
    want, tol = MR.metrics(y, p), MB.metrics_tol(y, p, y[0])
    for k in SCALARS:
        print(f"{label} {k}: {row[k]!r} want {want[k]!r} bound {tol[k]:.3e}")
        assert np.isfinite(tol[k]) and abs(row[k] - want[k]) <= tol[k], (label, k, row[k], want[k], tol[k])
    assert row["PearsonValid"] == want["PearsonValid"]


def by_key(rows):
    return {(r["Route"], r["Modality"], r["Model"]): r for r in rows}


@pytest.mark.parametrize("kind", ["rna2dna", "multimodal"])
def test_json_rows_and_mean_baseline(kind, data, checkpoints, tmp_path):
    out = tmp_path / "results.json"
    rows = evaluate.run(kind, DIMS + ["--batch-size", "32", "--precision", "fp32", "--checkpoint", checkpoints[kind], "--out", str(out)])
    with open(out) as f:
        stored = json.load(f)
    assert stored == json.loads(json.dumps(rows))
    expect = {"rna2dna": 1 + 1, "multimodal": 4 + 2}[kind]                 # routes x target modalities + one baseline per modality
    assert len(stored) == expect
    for r in stored:
        assert set(r) == {"Route", "Modality", "Model"} | set(evaluate.COLUMNS)
        assert all(np.isfinite(r[k]) for k in evaluate.COLUMNS), r
        assert r["PearsonValid"] == data["a"].shape[0]
    got = by_key(stored)
    check_row(got[("train mean", "DNA", "MeanImputation")], data["b"], data["mean_b"], f"{kind} mean DNA")      # two batches: 32 + 28
    if kind == "multimodal":
        check_row(got[("train mean", "RNA", "MeanImputation")], data["a"], data["mean_a"], f"{kind} mean RNA")


def test_bf16_inputs_evaluate_the_stored_values(data, checkpoints):
    rows = evaluate.run("rna2dna", DIMS + ["--batch-size", "64", "--input-dtype", "bf16", "--checkpoint", checkpoints["rna2dna"]])
    stored_b = torch.from_numpy(data["b"]).to(torch.bfloat16).double().numpy()
    check_row(by_key(rows)[("train mean", "DNA", "MeanImputation")], stored_b, data["mean_b"], "bf16 inputs, mean DNA")


@pytest.mark.parametrize("kind", ["rna2dna", "multimodal"])
def test_model_rows_equal_the_reference_on_the_models_reconstruction(kind, data, checkpoints):
    """eps injected: evaluate.run and a forward of the same checkpoint here see the same noise, so the model rows must be the
    metrics of exactly the reconstruction this forward returns."""
    n_val = data["a"].shape[0]
    eps = torch.randn(n_val, L, generator=torch.Generator().manual_seed(4))
    engine.GLOBAL_NOISE.inject([], eps)
    try:
        rows = by_key(evaluate.run(kind, DIMS + ["--batch-size", "64", "--precision", "fp32", "--checkpoint", checkpoints[kind]]))
        cls = RNA2DNAVAE if kind == "rna2dna" else MultiModalVAE
        model = cls(A, D, S, L)
        model.load_state_dict(torch.load(checkpoints[kind], map_location="cpu"))
        model.to(DEV).set_precision("fp32").eval()
        a, b, s = torch.from_numpy(data["a"]).to(DEV), torch.from_numpy(data["b"]).to(DEV), data["site"].to(DEV)
        with torch.no_grad():
            if kind == "rna2dna":
                rec = model(rna=a, site=s)[0].double().cpu().numpy()
                check_row(rows[("rna+site->dna", "DNA", "RNA2DNAVAE")], data["b"], rec, "rna2dna")
            else:
                rec_b = model(a=a)[1].double().cpu().numpy()
                check_row(rows[("a->b", "DNA", "MultiModalVAE")], data["b"], rec_b, "a->b")
                rec_a = model(b=b)[0].double().cpu().numpy()
                check_row(rows[("b->a", "RNA", "MultiModalVAE")], data["a"], rec_a, "b->a")
                full = model(a=a, b=b, site=s)
                ra, rb = full[0].double().cpu().numpy(), full[1].double().cpu().numpy()
                check_row(rows[("a+b+site->a,b", "RNA", "MultiModalVAE")], data["a"], ra, "full a")
                check_row(rows[("a+b+site->a,b", "DNA", "MultiModalVAE")], data["b"], rb, "full b")
    finally:
        engine.GLOBAL_NOISE.clear()


def test_checkpoint_of_other_dimensions_is_named(checkpoints):
    argv = [a if a != str(L) else "12" for a in DIMS]                      # latent 12 against the checkpoint's 8
    with pytest.raises(SystemExit) as e:
        evaluate.run("rna2dna", argv + ["--checkpoint", checkpoints["rna2dna"]])
    assert "checkpoint (" in str(e.value) and "latent 12" in str(e.value)


def test_missing_checkpoint_is_an_error(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                                            # no latest_rna2dna_run_id.txt here
    with pytest.raises(SystemExit):
        evaluate.run("rna2dna", DIMS)
