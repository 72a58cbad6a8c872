"""vae-los-angeles_amd/cluster_unmatched.py as a fresh child process on synthetic samples: two sample types times the four methods
give the expected rows and columns in --out and arrays of the right shapes in --embeddings-out; a second run takes the vae rows from the
files reconstruct.py --synthetic wrote into the same directory (its DNA-only frame has no primary_site: embedded, not judged)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from evaluate import CLUSTERING_COLUMNS, PCA_COLUMNS, TSNE_COLUMNS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vae-los-angeles_amd")
N = 600
COMMON = ["--synthetic", str(N), "--tsne-iters", "250"]


def run(tmp_path, script, *args):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), "--data-dir", str(tmp_path / "data"), *args], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_synthetic_table_and_embeddings(tmp_path):
    out, emb = tmp_path / "rows.json", tmp_path / "emb.npz"
    run(tmp_path, "cluster_unmatched.py", *COMMON, "--out", str(out), "--embeddings-out", str(emb))
    rows = json.loads(out.read_text())
    assert [(r["SampleType"], r["Method"]) for r in rows] == [(st, m) for st in ("RNA-only", "DNA-only") for m in ("mean", "knn", "cond_knn", "vae")]
    for r in rows:
        assert list(r) == ["SampleType", "Method", "Samples"] + list(CLUSTERING_COLUMNS + PCA_COLUMNS + TSNE_COLUMNS) and r["Samples"] == N
        assert all(np.isfinite(r[c]) for c in CLUSTERING_COLUMNS + PCA_COLUMNS + TSNE_COLUMNS)
        assert -1 <= r["Silhouette"] <= 1 and 0 <= r["NeighborhoodHit"] <= 1 and 0 < r["PCAExplained"] <= 1
    e = np.load(emb)
    for r in rows:
        key = f"{r['SampleType']}/{r['Method']}"
        assert e[key + "/pca"].shape == (N, 2) and e[key + "/tsne"].shape == (N, 2) and e[key + "/labels"].shape == (N,)


def test_vae_rows_from_reconstruction_files(tmp_path):
    run(tmp_path, "reconstruct.py", "--synthetic", str(N), "--timestamp", "T7")
    out, emb = tmp_path / "rows.json", tmp_path / "emb.npz"
    text = run(tmp_path, "cluster_unmatched.py", *COMMON, "--methods", "vae", "--from-reconstruction", "T7", "--out", str(out),
               "--embeddings-out", str(emb))
    assert "rna_with_reconstructed_dna_T7.pkl" in text and "dna_with_reconstructed_rna_T7.pkl" in text
    assert "don't have primary_site information: embedded, not judged" in text
    rows = json.loads(out.read_text())
    assert [(r["SampleType"], r["Method"], r["Samples"]) for r in rows] == [("RNA-only", "vae", N)]
    e = np.load(emb)
    assert e["DNA-only/vae/tsne"].shape == (N, 2) and "DNA-only/vae/labels" not in e.files and e["RNA-only/vae/labels"].shape == (N,)
