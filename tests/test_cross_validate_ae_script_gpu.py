"""cross_validate.py --autoencoder on the MI355X at the tiny dims of tests/test_cross_validate_script_gpu.py: the JSON has both
directions' AE rows (model "ae", param_name "epochs") behind the VAE rows and the two new comparison pairs, consistent with compare()
on the file's own results; --models ae is still refused."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cross_validate  # noqa: E402
from mmvae import crossval as CV  # noqa: E402
from test_cross_validate_script_gpu import DIMS, RESULT_KEYS  # noqa: E402


def test_autoencoder_rows_and_pairs(tmp_path, capsys):
    path = tmp_path / "cv.json"
    out = cross_validate.run(DIMS + ["--folds", "3", "--neighbors", "5", "--epochs", "1", "--batch-size", "32", "--autoencoder", "--out", str(path)])
    disk = json.loads(path.read_text())
    want = [(d, m, p) for d in ("DNA -> RNA", "RNA -> DNA") for m, p in (("mean", 0), ("knn", 5), ("vae", 1), ("ae", 1))]
    assert [(r["direction"], r["model"], r["param_value"]) for r in disk["results"]] == want
    for r in disk["results"]:
        assert set(r) == RESULT_KEYS
        if r["model"] == "ae":
            assert r["param_name"] == "epochs" and all(len(s) == 3 and np.isfinite(s).all() for s in r["fold_metrics"].values())
    for metric, entries in disk["comparisons"].items():
        assert [e["direction"] for e in entries] == ["DNA -> RNA", "RNA -> DNA"]
        again = json.loads(json.dumps(CV.compare(disk["results"], metric)))
        assert entries == again                                                     # consistent with compare() on the file's own results
        for e in entries:
            assert e["best_ae"] == 1 and e["ae_vs_vae"]["a"] == e["ae_vs_knn"]["a"] == "AE" and e["ae_vs_vae"]["df"] == 2
            assert (e["ae_vs_vae"]["b"], e["ae_vs_knn"]["b"]) == ("VAE", "kNN")
    assert out["results"] == disk["results"]
    text = capsys.readouterr().out
    assert "Best AE: epochs=1" in text and "AE vs VAE: t=" in text and "AE vs kNN: t=" in text


def test_models_ae_is_still_refused():
    with pytest.raises(SystemExit, match="the project has no AE models"):
        cross_validate.run(DIMS + ["--models", "mean", "ae", "--autoencoder"])
