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
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hostlib  # noqa: E402
from hostlib import ORIGINAL, RECON  # noqa: E402
from mmvae.data import load_pickled_dataset, synthetic_dataset  # noqa: E402
from mmvae.reconstruct import Reconstructor  # noqa: E402
from mmvae.unmatched import METHODS, SAMPLE_TYPES, SCALINGS  # noqa: E402
from src.config import Config  # noqa: E402


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
    hostlib.add_model_args(ap)
    ap.add_argument("--batch-size", type=int, default=4096)
    hostlib.add_precision_args(ap, input_dtype=False)
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
    n, classes = args.synthetic, hostlib.SYNTHETIC_CLASSES
    train = synthetic_dataset(n, args.input_dim_a, args.input_dim_b, len(classes), args.seed)
    tpm, _, site_r = synthetic_dataset(n, args.input_dim_a, args.input_dim_b, len(classes), args.seed + 1)
    _, beta, site_d = synthetic_dataset(n, args.input_dim_a, args.input_dim_b, len(classes), args.seed + 2)
    return train, classes, hostlib.synthetic_frame("RNA-only", np.expm1(tpm.numpy()), classes[site_r.numpy()]), \
        hostlib.synthetic_frame("DNA-only", beta.numpy(), classes[site_d.numpy()])


def load_inputs(args):
    classes = hostlib.read_classes(args.data_dir)
    matched = os.path.join(args.data_dir, "processed_data.pkl")
    train = load_pickled_dataset(matched) if os.path.exists(matched) else None
    if train is None:
        print(f"Training data not found: {matched}: mean / knn / cond_knn cannot run")
    return (train, classes, *hostlib.read_unmatched_frames(args.data_dir))


def known_sites(df, classes, what):
    """the frame filtered to the sites the label encoder knows, and their codes (None without primary_site)"""
    return hostlib.known_sites(df, classes, f"  {what}: filtered out {{n}} samples with primary_site not in label_encoder")


def column(df, name, dev):
    return torch.from_numpy(hostlib.column_matrix(df, name)).to(dev)


def vae_block(kind, df, sites, args, n_classes, dev):
    """the reconstructed modality of the frame's samples from the directional model, as reconstruct.py computes it; None without a model"""
    direction = SAMPLE_TYPES[kind]
    model = hostlib.load_directional(direction, getattr(args, f"checkpoint_{direction}"), args.checkpoint_dir,
                                     (args.input_dim_a, args.input_dim_b, n_classes, args.latent_dim), args.precision, args.seed, args.synthetic, dev)
    if model is None:
        return None
    x = hostlib.column_matrix(df, ORIGINAL[kind])
    x, sites, how = (np.log1p(x), sites, "given") if kind == "RNA-only" else (x, None, "none")
    mean, _ = Reconstructor(model).reconstruct_batched(x, sites, draws=1, sites=how, batch_size=args.batch_size, seed=args.seed)
    return torch.from_numpy(mean).to(dev)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.neighbors < 1:
        raise SystemExit("--neighbors must be at least 1")
    hostlib.require_device("cluster_unmatched.py")
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
