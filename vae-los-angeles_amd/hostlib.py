"""What the command-line tools beside this file share: their common arguments, the device guard, where a checkpoint is and the unmatched
samples' files.  The tools import this module, never each other (train*.py -> trainer excepted); mmvae and src import neither."""
import os
import pickle

import numpy as np
import torch

from src.config import Config
from src.models import KINDS, make_model

INPUT_DTYPE_HELP = "storage of the device-resident RNA / DNA matrices"


def add_dataset_args(ap):
    ap.add_argument("--data", default=None, help="processed_data.pkl produced by the reference's prepare scripts (default: synthetic)")
    ap.add_argument("--samples", type=int, default=262144, help="synthetic dataset size")


def add_model_args(ap, n_sites=False):
    ap.add_argument("--input-dim-a", type=int, default=int(os.getenv("INPUT_DIM_A", 782)))      # env overrides as train_dna2rna.py:172-174
    ap.add_argument("--input-dim-b", type=int, default=int(os.getenv("INPUT_DIM_B", 572)))
    if n_sites:
        ap.add_argument("--n-sites", type=int, default=24)
    ap.add_argument("--latent-dim", type=int, default=int(os.getenv("LATENT_DIM", Config.LATENT_DIM)))


def add_precision_args(ap, input_dtype=True, input_dtype_help=INPUT_DTYPE_HELP):
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    if input_dtype:
        ap.add_argument("--input-dtype", default="fp32", choices=["fp32", "bf16"], help=input_dtype_help)


def require_device(script_name):
    if not torch.cuda.is_available():
        raise SystemExit(f"{script_name} needs an MI355X: the product path has no CPU fallback")


NO_RUN_ID, NOT_FOUND = "no run id", "not found"


def resolve_checkpoint(kind, given, checkpoint_dir):
    """The override `given`, else the run the trainer named in latest_<tag>_run_id.txt -> (path, None), or (None, (why, the missing file))"""
    tag, path = KINDS[kind]["tag"], given
    if not path:
        id_file = f"latest_{tag}_run_id.txt"
        if not os.path.exists(id_file):
            return None, (NO_RUN_ID, id_file)
        with open(id_file) as f:
            path = os.path.join(checkpoint_dir, f"best_{tag}_{f.read().strip()}.pt")
    return (path, None) if os.path.exists(path) else (None, (NOT_FOUND, path))


def load_directional(kind, given, checkpoint_dir, dims, precision, seed, synthetic, dev):
    """The directional model of dims (input_dim_a, input_dim_b, n_sites, latent_dim) in eval mode, constructed after torch.manual_seed(seed);
    without a checkpoint: None and a warning, or under `synthetic` the freshly initialised model."""
    title = KINDS[kind]["title"]
    path, cause = resolve_checkpoint(kind, given, checkpoint_dir)
    why = None if cause is None else f"No {title} run ID found." if cause[0] == NO_RUN_ID else f"Model file {cause[1]} not found!"
    if path is None and not synthetic:
        print(f"Warning: {why}")
        return None
    torch.manual_seed(seed)
    model = make_model(kind, *dims)
    if path is not None:
        model.load_state_dict(torch.load(path, map_location="cpu"))
        print(f"{title} loaded from {path}")
    else:
        print(f"{title}: no checkpoint ({why}) -- synthetic run on a freshly initialised model")
    return model.to(dev).set_precision(precision).eval()


# the unmatched samples: the files of the reference's scripts/prepare_data.py and of reconstruct.py
UNMATCHED = {"RNA-only": "rna_only_unmatched.pkl", "DNA-only": "dna_only_unmatched.pkl"}
ORIGINAL = {"RNA-only": "tpm_unstranded", "DNA-only": "beta_value"}
RECON = {"RNA-only": ("rna_with_reconstructed_dna_", "reconstructed_beta_value"),       # (file prefix, column) reconstruct.py writes
         "DNA-only": ("dna_with_reconstructed_rna_", "reconstructed_tpm_unstranded")}
SYNTHETIC_CLASSES = np.array([f"site_{i:02d}" for i in range(24)])


def read_classes(data_dir):
    with open(os.path.join(data_dir, "label_encoder.pkl"), "rb") as f:
        return np.asarray(pickle.load(f).classes_)                          # any object with a sorted classes_


def read_unmatched_frames(data_dir):
    """-> [RNA-only frame, DNA-only frame]; None, and a line that says so, for a file that is not there"""
    import pandas as pd
    paths = {what: os.path.join(data_dir, name) for what, name in UNMATCHED.items()}
    for what, p in paths.items():
        if not os.path.exists(p):
            print(f"{what} data file not found: {p} (the reference's scripts/prepare_data.py writes it)")
    return [pd.read_pickle(p) if os.path.exists(p) else None for p in paths.values()]


def known_sites(df, classes, filtered):
    """the frame filtered to the label encoder's sites, and their codes (None without primary_site); filtered: what to print for {n} dropped rows"""
    if df is None or "primary_site" not in df.columns:
        return df, None
    known = df["primary_site"].isin(classes)
    if not known.all():
        print(filtered.format(n=int((~known).sum())))
    df = df[known]
    return df, np.searchsorted(classes, df["primary_site"].to_numpy()).astype(np.int64)


def column_matrix(df, name):
    return np.array(df[name].tolist()).astype(np.float32)


def synthetic_frame(what, values, sites=None):
    """a frame of the `what` ("RNA-only" / "DNA-only") file's columns: values (a host matrix) and, where given, the site names"""
    import pandas as pd
    cols = {"case_barcode": [f"{what[:3]}-{i:06d}" for i in range(len(values))], ORIGINAL[what]: list(values)}
    if sites is not None:
        cols["primary_site"] = sites
    return pd.DataFrame(cols)
