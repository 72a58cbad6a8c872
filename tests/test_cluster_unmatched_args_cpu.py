"""cluster_unmatched.py without a GPU: the parser, the file lookup, the synthetic inputs and the message."""
import numpy as np
import pytest

import cluster_unmatched as CU
from mmvae import unmatched as U


def test_parser_defaults_and_choices():
    a = CU.build_parser().parse_args([])
    assert a.methods is None and a.neighbors == 5 and a.scaling == "consistent" and a.data_dir == "data" and a.from_reconstruction is None
    assert not a.no_tsne and a.tsne_iters == 1000 and a.out is None and a.embeddings_out is None and a.synthetic == 0
    a = CU.build_parser().parse_args(["--methods", "mean", "vae", "--neighbors", "7", "--scaling", "reference", "--no-tsne", "--seed", "3",
                                      "--from-reconstruction", "20250101_000000", "--out", "o.json", "--embeddings-out", "e.npz", "--synthetic", "9"])
    assert a.methods == ["mean", "vae"] and a.neighbors == 7 and a.scaling == "reference" and a.no_tsne and a.seed == 3 and a.synthetic == 9
    for bad in (["--methods", "median"], ["--scaling", "raw"], ["--neighbors", "x"]):
        with pytest.raises(SystemExit):
            CU.build_parser().parse_args(bad)
    assert U.METHODS == ("mean", "knn", "cond_knn", "vae") and U.SCALINGS == ("consistent", "reference")


def test_newest_reconstruction_files(tmp_path):
    for name in ("rna_with_reconstructed_dna_20250101_000000.pkl", "rna_with_reconstructed_dna_20250301_120000.pkl",
                 "dna_with_reconstructed_rna_20250101_000000.pkl"):
        (tmp_path / name).write_bytes(b"")
    got = CU.find_latest_reconstruction_files(str(tmp_path))
    assert got["RNA-only"].endswith("dna_20250301_120000.pkl") and got["DNA-only"].endswith("rna_20250101_000000.pkl")
    got = CU.find_latest_reconstruction_files(str(tmp_path), "20250301_120000")
    assert got["RNA-only"].endswith("dna_20250301_120000.pkl") and got["DNA-only"] is None


def test_synthetic_inputs_have_sites_on_both_frames():
    a = CU.build_parser().parse_args(["--synthetic", "30", "--input-dim-a", "6", "--input-dim-b", "4"])
    train, classes, rna, dna = CU.synthetic_inputs(a)
    assert train[0].shape == (30, 6) and train[1].shape == (30, 4) and len(classes) == 24
    assert "primary_site" in rna.columns and "primary_site" in dna.columns and len(rna) == len(dna) == 30
    raw = np.array(rna["tpm_unstranded"].tolist())
    assert raw.shape == (30, 6) and (raw >= 0).all()                                    # raw TPM: expm1 of the log-scale draw
    df, codes = CU.known_sites(rna.assign(primary_site=["nowhere"] + list(rna["primary_site"][1:])), classes, "RNA-only")
    assert len(df) == 29 and codes.dtype == np.int64 and (classes[codes] == df["primary_site"].to_numpy()).all()


def test_feature_parts_and_messages_need_no_device():
    import torch
    x, y = torch.tensor([[0.0, 1.0]]), torch.tensor([[3.0]])
    assert torch.equal(U.feature_parts("RNA-only", x, y, "consistent")[0], torch.from_numpy(np.log1p(x.numpy()))) and U.feature_parts("RNA-only", x, y, "reference")[0] is x
    assert U.feature_parts("DNA-only", x, y, "consistent")[1] is y
    assert torch.equal(U.feature_parts("DNA-only", x, y, "reference", "knn")[1], torch.from_numpy(np.log1p(y.numpy())))
    assert U.feature_parts("DNA-only", x, y, "reference", "vae")[1] is y
    for bad in (dict(sample_type="both"), dict(scaling="raw"), dict(method="median")):
        with pytest.raises(ValueError):
            U.feature_parts(**{**dict(sample_type="RNA-only", original=x, imputed=y), **bad})


def test_says_that_it_needs_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="cluster_unmatched.py needs an MI355X"):
        CU.main(["--synthetic", "50"])
    with pytest.raises(SystemExit, match="--neighbors must be at least 1"):
        CU.main(["--neighbors", "0"])
