"""Reconstruction of unmatched samples with the trained directional VAEs on the MI355X: the reference's reconstruct_unmatched.py.

  RNA-only samples  (data/rna_only_unmatched.pkl: case_barcode, tpm_unstranded, primary_site)  -> DNA methylation by RNA2DNAVAE
  DNA-only samples  (data/dna_only_unmatched.pkl: case_barcode, beta_value)                    -> RNA expression by DNA2RNAVAE
  -> data/rna_with_reconstructed_dna_<ts>.pkl, data/dna_with_reconstructed_rna_<ts>.pkl, data/reconstruction_stats_<ts>.pkl

File names, columns, the filter on unknown primary sites, log1p on float32 and the stats keys are the reference's; the
preprocessing runs on the host in numpy, so the model sees the reference's inputs bit for bit.  What is added:

  --draws K          K draws of z per sample: the reconstructed column is their mean and a `<column>_std` column their spread (the
                     reference writes ONE random draw: vae.py:73 samples in eval mode too)
  --dna-sites all    DNA-only samples carry no primary site; the reference reconstructs them with site=None (the default here,
                     "none") and names "iterate through all possible sites and average" as the alternative: this is it

Both go through mmvae.reconstruct.Reconstructor, whose last decoder layer reduces the draws x sites on chip.  Every direction starts
from the same Philox position (--seed, offset 0), so a direction's output does not depend on whether the other one ran.
"""
import argparse
import os
import pickle
from datetime import datetime

import numpy as np
import torch

import hostlib
from mmvae.data import synthetic_dataset
from mmvae.reconstruct import Reconstructor
from src.config import Config


def build_parser():
    ap = argparse.ArgumentParser(description="reconstruct unmatched samples with RNA2DNAVAE / DNA2RNAVAE on MI355X")
    ap.add_argument("--data-dir", default="data", help="where label_encoder.pkl and the *_only_unmatched.pkl files are, and where the outputs go")
    ap.add_argument("--timestamp", default=None, help="the <ts> of the output names (default: now, %%Y%%m%%d_%%H%%M%%S)")
    ap.add_argument("--checkpoint-dir", default=Config.CHECKPOINT_DIR)
    ap.add_argument("--checkpoint-rna2dna", default=None, help="state_dict (default: best_rna2dna_<id>.pt of latest_rna2dna_run_id.txt)")
    ap.add_argument("--checkpoint-dna2rna", default=None, help="state_dict (default: best_dna2rna_<id>.pt of latest_dna2rna_run_id.txt)")
    hostlib.add_model_args(ap)
    ap.add_argument("--draws", type=int, default=1, metavar="K", help="draws of z per sample; K > 1: mean and *_std columns")
    ap.add_argument("--dna-sites", default="none", choices=["none", "all"], help="site of the DNA-only samples: none, or the mean over all sites")
    ap.add_argument("--batch-size", type=int, default=4096)
    hostlib.add_precision_args(ap, input_dtype=False)
    ap.add_argument("--seed", type=int, default=Config.RANDOM_SEED, help="Philox stream of eps")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N synthetic samples per direction and 24 synthetic sites instead of "
                    "the input files; a direction without a checkpoint then runs a freshly initialised model")
    return ap


def reconstructed(model, df, column, x, site, args, sites):
    """the frame plus `column`, the reconstruction of the rows of x (and `column`_std, their spread, where there is one)"""
    mean, std = Reconstructor(model).reconstruct_batched(x, site, draws=args.draws, sites=sites, batch_size=args.batch_size, seed=args.seed)
    out = df.copy()
    out[column] = list(mean)
    if std is not None:
        out[column + "_std"] = list(std)
    return out


def synthetic_inputs(args):
    """-> (classes, RNA-only frame with RAW TPM, DNA-only frame without sites): ONE synthetic dataset's RNA and DNA"""
    classes = hostlib.SYNTHETIC_CLASSES
    tpm, beta, site = synthetic_dataset(args.synthetic, args.input_dim_a, args.input_dim_b, len(classes), args.seed)
    return classes, hostlib.synthetic_frame("RNA-only", np.expm1(tpm.numpy()), classes[site.numpy()]), hostlib.synthetic_frame("DNA-only", beta.numpy())


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.draws < 1:
        raise SystemExit("--draws must be at least 1")
    hostlib.require_device("reconstruct.py")
    dev = torch.device("cuda", 0)
    ts = args.timestamp or datetime.now().strftime("%Y%m%d_%H%M%S")
    path = lambda name: os.path.join(args.data_dir, name)
    print(f"Unmatched data reconstruction, run timestamp {ts} (draws {args.draws}, DNA-only sites: {args.dna_sites}, {args.precision})")

    if args.synthetic:
        classes, rna_df, dna_df = synthetic_inputs(args)
        os.makedirs(args.data_dir, exist_ok=True)
    else:
        classes = hostlib.read_classes(args.data_dir)
        rna_df, dna_df = hostlib.read_unmatched_frames(args.data_dir)
    print(f"Label encoder: {len(classes)} classes")
    dims = (args.input_dim_a, args.input_dim_b, len(classes), args.latent_dim)
    models = {kind: hostlib.load_directional(kind, getattr(args, f"checkpoint_{kind}"), args.checkpoint_dir, dims, args.precision, args.seed,
                                             args.synthetic, dev) for kind in ("rna2dna", "dna2rna")}

    rna_out = dna_out = None
    if rna_df is not None and models["rna2dna"] is not None:
        rna_df, labels = hostlib.known_sites(rna_df, classes, "  Filtered out {n} samples with unknown primary_site")
        if len(rna_df):
            rna = np.log1p(hostlib.column_matrix(rna_df, hostlib.ORIGINAL["RNA-only"]))         # the training normalisation, on float32
            rna_out = reconstructed(models["rna2dna"], rna_df, hostlib.RECON["RNA-only"][1], rna, labels, args, "given")
            rna_out["primary_site_encoded"] = labels
            rna_out.to_pickle(path(f"rna_with_reconstructed_dna_{ts}.pkl"))
            print(f"RNA->DNA: {len(rna_out)} samples -> {path(f'rna_with_reconstructed_dna_{ts}.pkl')}")
        else:
            print("  No samples to reconstruct (all filtered out)")
    if dna_df is not None and models["dna2rna"] is not None and len(dna_df):
        dna_out = reconstructed(models["dna2rna"], dna_df, hostlib.RECON["DNA-only"][1], hostlib.column_matrix(dna_df, hostlib.ORIGINAL["DNA-only"]), None, args,
                                args.dna_sites)
        dna_out.to_pickle(path(f"dna_with_reconstructed_rna_{ts}.pkl"))
        print(f"DNA->RNA: {len(dna_out)} samples -> {path(f'dna_with_reconstructed_rna_{ts}.pkl')}")

    if rna_out is not None or dna_out is not None:
        stats = {"timestamp": ts,
                 "rna_only_samples": len(rna_out) if rna_out is not None else 0,
                 "dna_only_samples": len(dna_out) if dna_out is not None else 0}
        if rna_out is not None:
            stats["rna_only_primary_sites"] = rna_out["primary_site"].value_counts().to_dict()
        with open(path(f"reconstruction_stats_{ts}.pkl"), "wb") as f:
            pickle.dump(stats, f)
        print(f"Statistics -> {path(f'reconstruction_stats_{ts}.pkl')}")
    for what, out in (("RNA->DNA", rna_out), ("DNA->RNA", dna_out)):
        print(f"{what} reconstruction {'completed' if out is not None else 'not performed'}")


if __name__ == "__main__":
    main()
