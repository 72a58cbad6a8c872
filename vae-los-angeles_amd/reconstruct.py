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
import types
from datetime import datetime

import numpy as np
import torch

from mmvae import engine
from mmvae.reconstruct import Reconstructor
from src.config import Config
from trainer import KINDS, make_model


def build_parser():
    ap = argparse.ArgumentParser(description="reconstruct unmatched samples with RNA2DNAVAE / DNA2RNAVAE on MI355X")
    ap.add_argument("--data-dir", default="data", help="where label_encoder.pkl and the *_only_unmatched.pkl files are, and where the outputs go")
    ap.add_argument("--timestamp", default=None, help="the <ts> of the output names (default: now, %%Y%%m%%d_%%H%%M%%S)")
    ap.add_argument("--checkpoint-dir", default=Config.CHECKPOINT_DIR)
    ap.add_argument("--checkpoint-rna2dna", default=None, help="state_dict (default: best_rna2dna_<id>.pt of latest_rna2dna_run_id.txt)")
    ap.add_argument("--checkpoint-dna2rna", default=None, help="state_dict (default: best_dna2rna_<id>.pt of latest_dna2rna_run_id.txt)")
    ap.add_argument("--input-dim-a", type=int, default=int(os.getenv("INPUT_DIM_A", 782)))
    ap.add_argument("--input-dim-b", type=int, default=int(os.getenv("INPUT_DIM_B", 572)))
    ap.add_argument("--latent-dim", type=int, default=int(os.getenv("LATENT_DIM", Config.LATENT_DIM)))
    ap.add_argument("--draws", type=int, default=1, metavar="K", help="draws of z per sample; K > 1: mean and *_std columns")
    ap.add_argument("--dna-sites", default="none", choices=["none", "all"], help="site of the DNA-only samples: none, or the mean over all sites")
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--seed", type=int, default=Config.RANDOM_SEED, help="Philox stream of eps")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N synthetic samples per direction and 24 synthetic sites instead of "
                    "the input files; a direction without a checkpoint then runs a freshly initialised model")
    return ap


def checkpoint_path(kind, args):
    """The direction's state_dict: the override, or the run named by latest_<tag>_run_id.txt -> (path or None, why not)"""
    tag = KINDS[kind]["tag"]
    given = getattr(args, f"checkpoint_{tag}")
    if given:
        return (given, None) if os.path.exists(given) else (None, f"Model file {given} not found!")
    id_file = f"latest_{tag}_run_id.txt"
    if not os.path.exists(id_file):
        return None, f"No {KINDS[kind]['title']} run ID found."
    with open(id_file) as f:
        run_id = f.read().strip()
    path = os.path.join(args.checkpoint_dir, f"best_{tag}_{run_id}.pt")
    return (path, None) if os.path.exists(path) else (None, f"Model file {path} not found!")


def load_model(kind, args, n_sites, dev):
    path, why = checkpoint_path(kind, args)
    if path is None and not args.synthetic:
        print(f"Warning: {why}")
        return None
    torch.manual_seed(args.seed)
    model = make_model(kind, types.SimpleNamespace(input_dim_a=args.input_dim_a, input_dim_b=args.input_dim_b, n_sites=n_sites,
                                                   latent_dim=args.latent_dim))
    if path is not None:
        model.load_state_dict(torch.load(path, map_location="cpu"))
        print(f"{KINDS[kind]['title']} loaded from {path}")
    else:
        print(f"{KINDS[kind]['title']}: no checkpoint ({why}) -- synthetic run on a freshly initialised model")
    return model.to(dev).set_precision(args.precision).eval()


def column_matrix(df, column):
    return np.array(df[column].tolist()).astype(np.float32)


def run_batches(model, x, site, args, sites, dev):
    """Reconstructor over the rows of x in batches -> (mean, std or None) as host float32 arrays"""
    torch.manual_seed(args.seed)
    engine.GLOBAL_NOISE.load_state_dict({"offset": 0}, dev)
    rec = Reconstructor(model)
    want_std = rec.group_size(args.draws, sites) > 1
    means, stds = [], []
    for i in range(0, x.shape[0], args.batch_size):
        xb = torch.from_numpy(x[i:i + args.batch_size]).to(dev)
        sb = torch.from_numpy(site[i:i + args.batch_size]).to(dev) if site is not None else None
        m, s = rec.reconstruct(xb, sb, draws=args.draws, sites=sites, return_std=want_std)
        means.append(m.cpu().numpy())
        if want_std:
            stds.append(s.cpu().numpy())
    return np.concatenate(means), (np.concatenate(stds) if want_std else None)


def reconstruct_dna_from_rna(model, rna_df, classes, args, dev):
    """RNA-only samples -> their frame plus reconstructed_beta_value (and _std) and primary_site_encoded"""
    rna = np.log1p(column_matrix(rna_df, "tpm_unstranded"))                 # the training normalisation, on float32
    labels = np.searchsorted(classes, rna_df["primary_site"].to_numpy()).astype(np.int64)       # LabelEncoder.transform on sorted classes_
    mean, std = run_batches(model, rna, labels, args, "given", dev)
    out = rna_df.copy()
    out["reconstructed_beta_value"] = list(mean)
    if std is not None:
        out["reconstructed_beta_value_std"] = list(std)
    out["primary_site_encoded"] = labels
    return out


def reconstruct_rna_from_dna(model, dna_df, args, dev):
    """DNA-only samples -> their frame plus reconstructed_tpm_unstranded (and _std)"""
    mean, std = run_batches(model, column_matrix(dna_df, "beta_value"), None, args, args.dna_sites, dev)
    out = dna_df.copy()
    out["reconstructed_tpm_unstranded"] = list(mean)
    if std is not None:
        out["reconstructed_tpm_unstranded_std"] = list(std)
    return out


def synthetic_inputs(args):
    """-> (classes, RNA-only frame with RAW TPM, DNA-only frame)"""
    import pandas as pd
    from trainer import synthetic_dataset
    n, n_sites = args.synthetic, 24
    tpm, beta, site = synthetic_dataset(n, args.input_dim_a, args.input_dim_b, n_sites, args.seed)
    classes = np.array([f"site_{i:02d}" for i in range(n_sites)])
    rna = pd.DataFrame({"case_barcode": [f"RNA-{i:06d}" for i in range(n)], "tpm_unstranded": list(np.expm1(tpm.numpy())),
                        "primary_site": classes[site.numpy()]})
    dna = pd.DataFrame({"case_barcode": [f"DNA-{i:06d}" for i in range(n)], "beta_value": list(beta.numpy())})
    return classes, rna, dna


def main(argv=None):
    import pandas as pd
    args = build_parser().parse_args(argv)
    if args.draws < 1:
        raise SystemExit("--draws must be at least 1")
    if not torch.cuda.is_available():
        raise SystemExit("reconstruct.py needs an MI355X: the product path has no CPU fallback")
    dev = torch.device("cuda", 0)
    ts = args.timestamp or datetime.now().strftime("%Y%m%d_%H%M%S")
    path = lambda name: os.path.join(args.data_dir, name)
    print(f"Unmatched data reconstruction, run timestamp {ts} (draws {args.draws}, DNA-only sites: {args.dna_sites}, {args.precision})")

    rna_df = dna_df = None
    if args.synthetic:
        classes, rna_df, dna_df = synthetic_inputs(args)
        os.makedirs(args.data_dir, exist_ok=True)
    else:
        with open(path("label_encoder.pkl"), "rb") as f:
            classes = np.asarray(pickle.load(f).classes_)                   # any object with a sorted classes_
        for name, what in (("rna_only_unmatched.pkl", "RNA-only"), ("dna_only_unmatched.pkl", "DNA-only")):
            if not os.path.exists(path(name)):
                print(f"{what} data file not found: {path(name)} (the reference's scripts/prepare_data.py writes it)")
        if os.path.exists(path("rna_only_unmatched.pkl")):
            rna_df = pd.read_pickle(path("rna_only_unmatched.pkl"))
        if os.path.exists(path("dna_only_unmatched.pkl")):
            dna_df = pd.read_pickle(path("dna_only_unmatched.pkl"))
    print(f"Label encoder: {len(classes)} classes")
    models = {kind: load_model(kind, args, len(classes), dev) for kind in ("rna2dna", "dna2rna")}

    rna_out = dna_out = None
    if rna_df is not None and models["rna2dna"] is not None:
        known = rna_df["primary_site"].isin(classes)
        if not known.all():
            print(f"  Filtered out {int((~known).sum())} samples with unknown primary_site")
        rna_df = rna_df[known]
        if len(rna_df):
            rna_out = reconstruct_dna_from_rna(models["rna2dna"], rna_df, classes, args, dev)
            rna_out.to_pickle(path(f"rna_with_reconstructed_dna_{ts}.pkl"))
            print(f"RNA->DNA: {len(rna_out)} samples -> {path(f'rna_with_reconstructed_dna_{ts}.pkl')}")
        else:
            print("  No samples to reconstruct (all filtered out)")
    if dna_df is not None and models["dna2rna"] is not None and len(dna_df):
        dna_out = reconstruct_rna_from_dna(models["dna2rna"], dna_df, args, dev)
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
