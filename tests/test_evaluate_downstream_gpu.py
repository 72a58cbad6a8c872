"""evaluate.py --downstream on the MI355X with a tiny checkpoint (the pattern of tests/test_evaluate_tsne_gpu.py): eight scenarios for the
MultiModalVAE and five for a directional model, the JSON with the reference's keys, both other tables untouched by the flag, and a
validation split that cannot carry the task skipped with a message."""
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate  # noqa: E402
from mmvae import engine  # noqa: E402
from src.models import MultiModalVAE, RNA2DNAVAE  # noqa: E402

A, D, S, L, N = 40, 24, 5, 8, 2048
DIMS = ["--samples", str(N), "--input-dim-a", str(A), "--input-dim-b", str(D), "--n-sites", str(S), "--latent-dim", str(L)]
FLAGS = ["--downstream", "--downstream-folds", "2", "--downstream-epochs", "3"]
KEYS = {"precision", "precision_std", "recall", "recall_std", "f1-score", "f1-score_std"}


def save(tmp_path_factory, cls, name):
    path = str(tmp_path_factory.mktemp("ckpt") / name)
    torch.manual_seed(3)
    torch.save(cls(A, D, S, L).state_dict(), path)
    return path


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    return save(tmp_path_factory, MultiModalVAE, "multimodal.pt")


@pytest.fixture(scope="module")
def runs(checkpoint, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("out") / "downstream.json")
    common = DIMS + ["--batch-size", "128", "--precision", "fp32", "--checkpoint", checkpoint, "--clustering"]
    dev = torch.device("cuda", torch.cuda.current_device())
    start = engine.GLOBAL_NOISE.state_dict(dev)                    # each run from the same position of the stream eps is drawn from
    plain = evaluate.run("multimodal", common, return_clustering=True)
    engine.GLOBAL_NOISE.load_state_dict(start, dev)
    flagged = evaluate.run("multimodal", common + FLAGS + ["--downstream-out", out], return_clustering=True)
    with open(out) as f:
        return plain, flagged, json.load(f)


def check_table(table, scenarios):
    assert list(table) == scenarios
    for name, r in table.items():
        assert {"accuracy", "accuracy_std", "weighted avg"} <= set(r) and set(r["weighted avg"]) == KEYS, name
        classes = set(r) - {"accuracy", "accuracy_std", "weighted avg"}
        assert classes == {str(c) for c in range(S)} and all(set(r[c]) == KEYS for c in classes)
        assert 0.0 <= r["accuracy"] <= 1.0 and all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in r["weighted avg"].values())


def test_eight_scenarios_with_the_references_keys(runs):
    check_table(runs[2], ["Orig. RNA", "Orig. DNA", "Orig. RNA + Est. DNA", "Orig. DNA + Est. RNA", "Orig. RNA + Orig. DNA", "Est. DNA", "Est. RNA",
                          "Est. RNA + Est. DNA"])


def test_the_other_tables_do_not_depend_on_the_flag(runs):
    (rows0, crows0), (rows1, crows1), _ = runs
    assert len(rows1) == len(rows0) == 6 and len(crows1) == len(crows0) > 0
    for r0, r1 in zip(rows0, rows1):                              # float64 atomics: see tests/test_evaluate_tsne_gpu.py
        assert set(r1) == set(r0) and all(r1[k] == r0[k] for k in ("Route", "Modality", "Model", "PearsonValid"))
        assert all(r1[k] == pytest.approx(r0[k], rel=1e-10, abs=1e-10) for k in evaluate.COLUMNS), (r0, r1)
    assert crows1 == crows0


def test_a_directional_model_fills_five_scenarios(tmp_path_factory, capsys):
    path = save(tmp_path_factory, RNA2DNAVAE, "rna2dna.pt")
    out = str(tmp_path_factory.mktemp("out") / "downstream.json")
    # bf16 input storage here, fp32 in the MultiModalVAE runs above: the estimated modality is drawn from either
    evaluate.run("rna2dna", DIMS + ["--batch-size", "128", "--precision", "fp32", "--input-dtype", "bf16", "--checkpoint", path] + FLAGS
                 + ["--downstream-out", out])
    with open(out) as f:
        check_table(json.load(f), ["Orig. RNA", "Orig. DNA", "Orig. RNA + Est. DNA", "Est. DNA", "Orig. RNA + Orig. DNA"])
    printed = capsys.readouterr().out
    assert "downstream task: site classification, 2 stratified folds" in printed and printed.count(" +- ") == 5 * 4 + 1          # four cells a row, and the heading


def test_a_split_without_two_usable_classes_is_skipped_with_a_message(capsys):
    va = [torch.zeros(5, 4, device="cuda"), torch.zeros(5, 3, device="cuda"), torch.arange(5, device="cuda")]
    assert evaluate.downstream_table("multimodal", None, va, 4, 2, 3, 42) == {}
    va[2] = torch.tensor([0, 0, 0, 1, 2], device="cuda")           # one site with two rows or more
    assert evaluate.downstream_table("multimodal", None, va, 4, 2, 3, 42) == {}
    assert capsys.readouterr().out.count("downstream table skipped") == 2


def test_the_flags_are_checked(checkpoint):
    base = DIMS + ["--checkpoint", checkpoint]
    for extra in (["--downstream-out", "x.json"], ["--downstream", "--downstream-folds", "1"], ["--downstream", "--downstream-epochs", "0"]):
        with pytest.raises(SystemExit):
            evaluate.run("multimodal", base + extra)
