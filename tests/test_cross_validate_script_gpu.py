"""cross_validate.py on the MI355X at the tiny dims of tests/test_crossval_gpu.py: the JSON it writes has the reference's
aggregated_results rows for both directions and the three comparisons, and the flags it cannot serve are refused."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cross_validate  # noqa: E402
import crossval_ref as CR  # noqa: E402

DIMS = ["--samples", "300", "--input-dim-a", "40", "--input-dim-b", "24", "--n-sites", "5", "--latent-dim", "8", "--subset", "1.0"]
RESULT_KEYS = {"direction", "model", "param_name", "param_value", "time", "fold_metrics"} | {f"{p}_{k}" for p in ("mean", "std") for k in CR.KEYS}


def test_the_json_has_the_references_schema(tmp_path):
    pytest.importorskip("scipy.stats")
    path = tmp_path / "cv.json"
    out = cross_validate.run(DIMS + ["--folds", "3", "--neighbors", "5", "10", "--epochs", "1", "--batch-size", "32", "--knn-by-site", "--out", str(path)])
    disk = json.loads(path.read_text())
    assert disk["rows"] == 300 and disk["folds"] == 3 and disk["neighbors"] == [5, 10]
    want = [(d, m, p) for d in ("DNA -> RNA", "RNA -> DNA") for m, p in (("mean", 0), ("knn", 5), ("knn", 10), ("knn_site", 5), ("knn_site", 10), ("vae", 1))]
    assert [(r["direction"], r["model"], r["param_value"]) for r in disk["results"]] == want
    for r in disk["results"]:
        assert set(r) == RESULT_KEYS and list(r["fold_metrics"]) == list(CR.KEYS)
        for k, scores in r["fold_metrics"].items():
            assert len(scores) == 3 and np.isfinite(scores).all()
            assert r[f"mean_{k}"] == float(np.mean(scores)) and r[f"std_{k}"] == float(np.std(scores))
    assert list(disk["comparisons"]) == ["Mean R2", "MSE", "Pearson"]
    for metric, entries in disk["comparisons"].items():
        assert [e["direction"] for e in entries] == ["DNA -> RNA", "RNA -> DNA"]
        CR.same_comparison(entries, CR.compare(disk["results"], metric), rel=1e-9)
        for e in entries:
            assert {"knn_vs_vae", "vae_vs_mean", "knn_site_vs_vae"} <= set(e) and e["knn_vs_vae"]["df"] == 2
    assert out["results"] == disk["results"]


def test_subset_takes_the_sampled_rows():
    out = cross_validate.run(DIMS[:-2] + ["--subset", "0.5", "--folds", "3", "--neighbors", "5", "--models", "mean", "knn"])
    assert out["rows"] == 150 and [r["model"] for r in out["results"]] == ["mean", "knn"] * 2
    assert out["comparisons"] == {"Mean R2": [], "MSE": [], "Pearson": []}               # nothing to compare without the VAE


def test_flags_that_cannot_be_served_are_refused():
    with pytest.raises(SystemExit, match="the project has no AE models"):
        cross_validate.run(DIMS + ["--models", "mean", "ae"])
    with pytest.raises(SystemExit, match="--knn-by-site needs knn"):
        cross_validate.run(DIMS + ["--models", "mean", "vae", "--knn-by-site"])
    with pytest.raises(SystemExit):
        cross_validate.run(DIMS + ["--models", "forest"])
    with pytest.raises(SystemExit):
        cross_validate.run(DIMS + ["--folds", "1"])
    with pytest.raises(SystemExit):
        cross_validate.run(["--samples", "20", "--input-dim-a", "40", "--input-dim-b", "24", "--n-sites", "5", "--subset", "1.0", "--folds", "2", "--neighbors", "15",
                            "--models", "knn"])
