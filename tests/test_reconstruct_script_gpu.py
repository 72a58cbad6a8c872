"""vae-los-angeles_amd/reconstruct.py as a fresh child process on tiny synthetic pickles: the reference's file names, columns, filter
and stats keys; the reconstructed columns equal mmvae.reconstruct.Reconstructor on np.log1p of the input at the same seed; --draws
adds the std columns; a direction without a checkpoint is skipped and the exit status stays 0."""
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvae import engine  # noqa: E402
from mmvae.reconstruct import Reconstructor  # noqa: E402
from src.models import DNA2RNAVAE, RNA2DNAVAE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "vae-los-angeles_amd", "reconstruct.py")
DEV = torch.device("cuda", 0)
RNA, DNA, LATENT, SEED = 40, 24, 8, 77
CLASSES = np.array(["Brain", "Breast", "Colon", "Kidney", "Lung"])


def write_inputs(tmp_path):
    rng = np.random.default_rng(3)
    data = tmp_path / "data"
    data.mkdir()
    with open(data / "label_encoder.pkl", "wb") as f:
        pickle.dump(types.SimpleNamespace(classes_=CLASSES), f)
    sites = list(rng.choice(CLASSES, 9))
    sites[2], sites[6] = "Thymus", "Adrenal gland"                       # two rows the label encoder does not know
    rna = pd.DataFrame({"case_barcode": [f"R{i}" for i in range(9)],
                        "tpm_unstranded": list(rng.gamma(1.0, 20.0, (9, RNA))), "primary_site": sites})
    dna = pd.DataFrame({"case_barcode": [f"D{i}" for i in range(7)], "beta_value": list(rng.random((7, DNA)))})
    rna.to_pickle(data / "rna_only_unmatched.pkl")
    dna.to_pickle(data / "dna_only_unmatched.pkl")
    models = {}
    for tag, cls in (("rna2dna", RNA2DNAVAE), ("dna2rna", DNA2RNAVAE)):
        torch.manual_seed(5)
        models[tag] = cls(RNA, DNA, len(CLASSES), LATENT)
        torch.save(models[tag].state_dict(), tmp_path / f"{tag}.pt")
        models[tag].to(DEV).set_precision("bf16").eval()
    return data, rna, dna, models


def run_script(tmp_path, *extra):
    cmd = [sys.executable, SCRIPT, "--data-dir", str(tmp_path / "data"), "--input-dim-a", str(RNA), "--input-dim-b", str(DNA),
           "--latent-dim", str(LATENT), "--seed", str(SEED), "--checkpoint-dir", str(tmp_path), *extra]
    return subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=240)


def reconstructed(model, x, site, **kw):
    """Reconstructor from the script's Philox position: (--seed, offset 0); the process's own position is put back"""
    seed0, pos0 = torch.initial_seed(), engine.GLOBAL_NOISE.state_dict(DEV)
    try:
        torch.manual_seed(SEED)
        engine.GLOBAL_NOISE.load_state_dict({"offset": 0}, DEV)
        m, s = Reconstructor(model).reconstruct(torch.from_numpy(x).to(DEV), None if site is None else torch.from_numpy(site).to(DEV), **kw)
        return m.cpu().numpy(), (None if s is None else s.cpu().numpy())
    finally:
        torch.manual_seed(seed0)
        engine.GLOBAL_NOISE.load_state_dict(pos0, DEV)


def test_script_writes_the_reference_files(tmp_path):
    data, rna, dna, models = write_inputs(tmp_path)
    r = run_script(tmp_path, "--timestamp", "T0", "--checkpoint-rna2dna", str(tmp_path / "rna2dna.pt"),
                   "--checkpoint-dna2rna", str(tmp_path / "dna2rna.pt"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(data)) == sorted(["label_encoder.pkl", "rna_only_unmatched.pkl", "dna_only_unmatched.pkl",
                                               "rna_with_reconstructed_dna_T0.pkl", "dna_with_reconstructed_rna_T0.pkl",
                                               "reconstruction_stats_T0.pkl"])
    out_r, out_d = pd.read_pickle(data / "rna_with_reconstructed_dna_T0.pkl"), pd.read_pickle(data / "dna_with_reconstructed_rna_T0.pkl")
    assert list(out_r.columns) == ["case_barcode", "tpm_unstranded", "primary_site", "reconstructed_beta_value", "primary_site_encoded"]
    assert list(out_d.columns) == ["case_barcode", "beta_value", "reconstructed_tpm_unstranded"]
    kept = rna[rna["primary_site"].isin(CLASSES)]
    assert len(kept) == 7 and list(out_r["case_barcode"]) == list(kept["case_barcode"]) and list(out_d["case_barcode"]) == list(dna["case_barcode"])
    labels = np.searchsorted(CLASSES, kept["primary_site"].to_numpy()).astype(np.int64)
    assert np.array_equal(out_r["primary_site_encoded"].to_numpy(), labels)
    with open(data / "reconstruction_stats_T0.pkl", "rb") as f:
        stats = pickle.load(f)
    assert stats == {"timestamp": "T0", "rna_only_samples": 7, "dna_only_samples": 7,
                     "rna_only_primary_sites": kept["primary_site"].value_counts().to_dict()}
    x = np.log1p(np.array(kept["tpm_unstranded"].tolist()).astype(np.float32))
    want, _ = reconstructed(models["rna2dna"], x, labels)
    assert np.array_equal(np.stack(out_r["reconstructed_beta_value"].to_numpy()), want)
    want, _ = reconstructed(models["dna2rna"], np.array(dna["beta_value"].tolist()).astype(np.float32), None, sites="none")
    assert np.array_equal(np.stack(out_d["reconstructed_tpm_unstranded"].to_numpy()), want)


def test_draws_add_std_columns_and_a_missing_checkpoint_skips_its_direction(tmp_path):
    data, rna, dna, models = write_inputs(tmp_path)
    (tmp_path / "latest_rna2dna_run_id.txt").write_text("run9\n")          # the run-id route: best_rna2dna_run9.pt in --checkpoint-dir
    os.replace(tmp_path / "rna2dna.pt", tmp_path / "best_rna2dna_run9.pt")
    os.remove(tmp_path / "dna2rna.pt")                                     # and no run id for the other direction
    r = run_script(tmp_path, "--timestamp", "T1", "--draws", "3")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Warning: No DNA2RNAVAE run ID found." in r.stdout
    assert not os.path.exists(data / "dna_with_reconstructed_rna_T1.pkl")
    out_r = pd.read_pickle(data / "rna_with_reconstructed_dna_T1.pkl")
    assert list(out_r.columns) == ["case_barcode", "tpm_unstranded", "primary_site", "reconstructed_beta_value",
                                   "reconstructed_beta_value_std", "primary_site_encoded"]
    kept = rna[rna["primary_site"].isin(CLASSES)]
    labels = np.searchsorted(CLASSES, kept["primary_site"].to_numpy()).astype(np.int64)
    x = np.log1p(np.array(kept["tpm_unstranded"].tolist()).astype(np.float32))
    mean, std = reconstructed(models["rna2dna"], x, labels, draws=3, return_std=True)
    assert np.array_equal(np.stack(out_r["reconstructed_beta_value"].to_numpy()), mean)
    assert np.array_equal(np.stack(out_r["reconstructed_beta_value_std"].to_numpy()), std)
    with open(data / "reconstruction_stats_T1.pkl", "rb") as f:
        stats = pickle.load(f)
    assert stats["rna_only_samples"] == 7 and stats["dna_only_samples"] == 0
