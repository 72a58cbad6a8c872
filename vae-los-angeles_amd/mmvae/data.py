"""The matched dataset (RNA, DNA, site) on the host: processed_data.pkl or its synthetic stand-in, the validation split, class weights."""
import numpy as np
import torch

from src.config import Config


def balanced_class_weights(site, n_sites):
    """compute_class_weights of the reference (optimize_hyperparameters.py:33-44): sklearn's 'balanced' weights over the classes
    PRESENT in the training labels, n / (k_present * count_c); classes that do not occur keep weight 1."""
    counts = torch.bincount(site.reshape(-1), minlength=n_sites).double()
    present = counts > 0
    w = torch.ones(n_sites, dtype=torch.float64)
    w[present] = site.numel() / (present.sum().double() * counts[present])
    return w.float()


def synthetic_dataset(n, a_dim, d_dim, n_sites, seed):
    g = torch.Generator().manual_seed(seed)
    tpm = torch.log1p(torch.exp(1.5 * torch.randn(n, a_dim, generator=g)))          # log1p(TPM)-like, >= 0 (prepare_data.py:123-125)
    beta = torch.rand(n, d_dim, generator=g)                                          # methylation beta values in [0, 1]
    site = torch.randint(0, n_sites, (n,), generator=g, dtype=torch.int64)
    return tpm, beta, site


def load_pickled_dataset(path):
    """Same columns as the reference's processed_data.pkl (src/data/dataset.py:20-30)."""
    import pandas as pd
    df = pd.read_pickle(path)          # a file the USER produced with the reference's own scripts -- never one from the reference tree
    tpm = torch.tensor(np.stack(df["tpm_unstranded"].values), dtype=torch.float32)
    beta = torch.tensor(np.stack(df["beta_value"].values), dtype=torch.float32)
    site = torch.tensor(df["primary_site_encoded"].values, dtype=torch.int64)
    return tpm, beta, site


def split_indices(n):
    """(val_idx, train_idx) of n samples: the one validation split of the trainers and of evaluate.py."""
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(Config.RANDOM_SEED))       # train_test_split(random_state=42) stand-in
    n_val = int(n * Config.TRAIN_TEST_SPLIT)
    return perm[:n_val], perm[n_val:]


def load_matched(data, samples, input_dim_a, input_dim_b, n_sites, seed):
    """(tpm, beta, site, (input_dim_a, input_dim_b, n_sites)): the pickled `data`, which sets the dims, else `samples` synthetic rows"""
    if data:
        tpm, beta, site = load_pickled_dataset(data)
        input_dim_a, input_dim_b, n_sites = tpm.shape[1], beta.shape[1], int(site.max()) + 1
    else:
        tpm, beta, site = synthetic_dataset(samples, input_dim_a, input_dim_b, n_sites, seed)
    # class indices are validated ONCE, on the host, before any rank trains: in the loop a bad label only shows up in the loss read of the rank that
    # holds it and the other ranks would wait in the all-reduce.  -100 (F.cross_entropy's ignore_index) has no row in the site Embedding either.
    lo, hi = int(site.min()), int(site.max())
    if lo < 0 or hi >= n_sites:
        raise SystemExit(f"site labels must lie in [0, {n_sites}); found [{lo}, {hi}]")
    return tpm, beta, site, (input_dim_a, input_dim_b, n_sites)
