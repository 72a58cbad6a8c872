"""Clustering of the unmatched samples on the MI355X: the reference's cluster_imputation_methods.py and cluster_reconstructed.py as one
table, without the plots (mmvae.unmatched).

  RNA-only samples (data/rna_only_unmatched.pkl) get their DNA, DNA-only samples (data/dna_only_unmatched.pkl) their RNA from
    mean / knn / cond_knn   fitted on the matched training set (data/processed_data.pkl), and from
    vae                     RNA2DNAVAE / DNA2RNAVAE: the columns reconstructed_beta_value / reconstructed_tpm_unstranded of the files
                            reconstruct.py wrote (--from-reconstruction TS, or the newest pair in --data-dir), else the models themselves
  one table row per (sample type, method): silhouette and neighbourhood hit on the standardised [original | imputed] features, on their
  PCA(2) (with the explained variance) and on the t-SNE of their PCA(50).

The reference's rules: samples are filtered to the sites label_encoder.pkl knows; cond_knn covers the samples with a known site; a
DNA-only frame without primary_site is embedded (--embeddings-out) but not judged.  --scaling: see mmvae.unmatched."""
import argparse
import glob
import json
import os
import pickle
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmvae.unmatched import METHODS, SAMPLE_TYPES, SCALINGS  # noqa: E402
from src.config import Config  # noqa: E402

RECON = {"RNA-only": ("rna_with_reconstructed_dna_", "reconstructed_beta_value"),
         "DNA-only": ("dna_with_reconstructed_rna_", "reconstructed_tpm_unstranded")}
ORIGINAL = {"RNA-only": "tpm_unstranded", "DNA-only": "beta_value"}


def build_parser():
    ap = argparse.ArgumentParser(description="cluster the unmatched samples with imputed / reconstructed modalities on MI355X")
    ap.add_argument("--methods", nargs="+", choices=METHODS, default=None, help="default: all that can run")
    ap.add_argument("--neighbors", type=int, default=5, help="k of knn / cond_knn")
    ap.add_argument("--scaling", choices=SCALINGS, default="consistent")
    ap.add_argument("--data-dir", default="data")
    ap.add_argument("--from-reconstruction", default=None, metavar="TS", help="the <ts> of reconstruct.py's output files (default: the newest)")
    ap.add_argument("--no-tsne", action="store_true")
    ap.add_argument("--tsne-iters", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=Config.RANDOM_SEED)
    ap.add_argument("--out", default=None, metavar="FILE", help="table rows as JSON")
    ap.add_argument("--embeddings-out", default=None, metavar="FILE.npz", help="PCA / t-SNE coordinates and labels per row")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N synthetic matched, RNA-only and DNA-only samples of 24 sites instead "
                    "of the input files; vae then runs freshly initialised models where no checkpoint exists")
    # the models of the vae method, as reconstruct.py names them
    ap.add_argument("--checkpoint-dir", default=Config.CHECKPOINT_DIR)
    ap.add_argument("--checkpoint-rna2dna", default=None)
    ap.add_argument("--checkpoint-dna2rna", default=None)
    ap.add_argument("--input-dim-a", type=int, default=int(os.getenv("INPUT_DIM_A", 782)))
    ap.add_argument("--input-dim-b", type=int, default=int(os.getenv("INPUT_DIM_B", 572)))
    ap.add_argument("--latent-dim", type=int, default=int(os.getenv("LATENT_DIM", Config.LATENT_DIM)))
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    return ap


def find_latest_reconstruction_files(data_dir, ts=None):
    """{sample type: path or None}: the files of run `ts`, or the newest of each kind (names sort by timestamp)"""
    out = {}
    for kind, (prefix, _) in RECON.items():
        if ts is not None:
            p = os.path.join(data_dir, f"{prefix}{ts}.pkl")
            out[kind] = p if os.path.exists(p) else None
        else:
            found = sorted(glob.glob(os.path.join(data_dir, f"{prefix}*.pkl")))
            out[kind] = found[-1] if found else None
    return out


def synthetic_inputs(args):
    """-> (train (rna, dna, site) tensors, classes, RNA-only frame with RAW TPM, DNA-only frame), sites on both frames"""
    import pandas as pd
    from trainer import synthetic_dataset
    n, n_sites = args.synthetic, 24
    classes = np.array([f"site_{i:02d}" for i in range(n_sites)])
    train = synthetic_dataset(n, args.input_dim_a, args.input_dim_b, n_sites, args.seed)
    tpm, _, site_r = synthetic_dataset(n, args.input_dim_a, args.input_dim_b, n_sites, args.seed + 1)
    _, beta, site_d = synthetic_dataset(n, args.input_dim_a, args.input_dim_b, n_sites, args.seed + 2)
    rna = pd.DataFrame({"case_barcode": [f"RNA-{i:06d}" for i in range(n)], "tpm_unstranded": list(np.expm1(tpm.numpy())),
                        "primary_site": classes[site_r.numpy()]})
    dna = pd.DataFrame({"case_barcode": [f"DNA-{i:06d}" for i in range(n)], "beta_value": list(beta.numpy()),
                        "primary_site": classes[site_d.numpy()]})
    return train, classes, rna, dna


def load_inputs(args):
    import pandas as pd
    from trainer import load_pickled_dataset
    path = lambda name: os.path.join(args.data_dir, name)
    with open(path("label_encoder.pkl"), "rb") as f:
        classes = np.asarray(pickle.load(f).classes_)
    train = load_pickled_dataset(path("processed_data.pkl")) if os.path.exists(path("processed_data.pkl")) else None
    if train is None:
        print(f"Training data not found: {path('processed_data.pkl')}: mean / knn / cond_knn cannot run")
    frames = []
    for name, what in (("rna_only_unmatched.pkl", "RNA-only"), ("dna_only_unmatched.pkl", "DNA-only")):
        if os.path.exists(path(name)):
            frames.append(pd.read_pickle(path(name)))
        else:
            print(f"{what} data file not found: {path(name)} (the reference's scripts/prepare_data.py writes it)")
            frames.append(None)
    return train, classes, frames[0], frames[1]


def known_sites(df, classes, what):
    """the frame filtered to the sites the label encoder knows, and their codes (None without primary_site)"""
    if df is None or "primary_site" not in df.columns:
        return df, None
    known = df["primary_site"].isin(classes)
    if not known.all():
        print(f"  {what}: filtered out {int((~known).sum())} samples with primary_site not in label_encoder")
    df = df[known]
    return df, np.searchsorted(classes, df["primary_site"].to_numpy()).astype(np.int64)


def column(df, name, dev):
    return torch.from_numpy(np.array(df[name].tolist()).astype(np.float32)).to(dev)


def vae_block(kind, df, sites, args, n_classes, dev):
    """the reconstructed modality of the frame's samples from the directional model, as reconstruct.py computes it; None without a model"""
    import types
    import reconstruct as R
    direction = SAMPLE_TYPES[kind]
    model = R.load_model(direction, args, n_classes, dev)
    if model is None:
        return None
    run = types.SimpleNamespace(seed=args.seed, draws=1, batch_size=args.batch_size)
    x = np.array(df[ORIGINAL[kind]].tolist()).astype(np.float32)
    if kind == "RNA-only":
        mean, _ = R.run_batches(model, np.log1p(x), sites, run, "given", dev)
    else:
        mean, _ = R.run_batches(model, x, None, run, "none", dev)
    return torch.from_numpy(mean).to(dev)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.neighbors < 1:
        raise SystemExit("--neighbors must be at least 1")
    if not torch.cuda.is_available():
        raise SystemExit("cluster_unmatched.py needs an MI355X: the product path has no CPU fallback")
    from mmvae import unmatched as U
    dev = torch.device("cuda", 0)
    if args.synthetic:
        train, classes, rna_df, dna_df = synthetic_inputs(args)
    else:
        train, classes, rna_df, dna_df = load_inputs(args)
    if rna_df is None and dna_df is None:
        print("No unmatched samples found: run the reference's scripts/prepare_data.py first")
        return
    print(f"Label encoder: {len(classes)} classes; scaling {args.scaling}; k = {args.neighbors}")
    if train is not None:
        train = tuple(t.to(dev) for t in train)
    recon_files = find_latest_reconstruction_files(args.data_dir, args.from_reconstruction)
    methods = list(args.methods or METHODS)
    tsne = None if args.no_tsne else (args.tsne_iters, args.seed)
    rows, emb = [], {}

    for kind, df in (("RNA-only", rna_df), ("DNA-only", dna_df)):
        if df is None or not len(df):
            continue
        for method in methods:
            frame, block = df, None
            if method == "vae" and recon_files[kind] is not None:
                import pandas as pd
                frame = pd.read_pickle(recon_files[kind])
                print(f"{kind} / vae: {recon_files[kind]}")
            frame, sites = known_sites(frame, classes, kind)
            if not len(frame):
                print(f"{kind} / {method}: no samples with a valid primary_site")
                continue
            original = column(frame, ORIGINAL[kind], dev)
            site_t = None if sites is None else torch.from_numpy(sites).to(dev)
            if method == "vae":
                block = column(frame, RECON[kind][1], dev) if RECON[kind][1] in frame.columns else vae_block(kind, frame, sites, args, len(classes), dev)
                if block is None:
                    print(f"{kind} / vae: no reconstruction file and no model: skipped")
                    continue
            elif train is None:
                continue
            elif method == "cond_knn" and sites is None:
                print(f"{kind} samples don't have primary_site information: cond_knn skipped")
                continue
            else:
                block = U.impute(method, train[0], train[1], train[2], U.query_features(kind, original, args.scaling), site_t,
                                 SAMPLE_TYPES[kind], k=args.neighbors)
            parts = U.feature_parts(kind, original, block, args.scaling, method)
            key, e = f"{kind}/{method}", {}
            if sites is None:
                print(f"{kind} samples don't have primary_site information: embedded, not judged ({method})")
                U.judge(parts, None, tsne=tsne, embeddings=e)
            else:
                row = U.judge(parts, site_t, tsne=tsne, embeddings=e)
                if row is not None:
                    rows.append({"SampleType": kind, "Method": method, "Samples": len(frame), **row})
                    print(f"{kind:<10}{method:<10}" + "".join(f"  {c} {v:.4f}" for c, v in row.items()))
                emb[f"{key}/labels"] = sites
            for name, y in e.items():
                emb[f"{key}/{name}"] = y
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    if args.embeddings_out:
        np.savez_compressed(args.embeddings_out, **emb)
    print(f"{len(rows)} table rows")


if __name__ == "__main__":
    main()
