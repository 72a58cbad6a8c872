"""Imputation metrics on the device: the dictionary of the reference's compute_metrics (compare_directional_imputation.py:167-210)
and calculate_metrics (vae_cross_modality_cv.py:71-108) from ONE streaming launch per batch (mmvae_recon_metrics) instead of an
N x N cosine_similarity matrix, a Python loop of scipy.stats.pearsonr and a host copy of every reconstruction.

    m = ImputationMetrics(n_features, device)
    for y_true, y_pred in batches:          # any number of batches; y_pred (F,) = one row for every sample (mean imputation)
        m.update(y_true, y_pred)
    result = m.compute()

The kernel leaves four float64 sums per feature (additive over batches) and the per-sample Pearson r / cosine similarity; compute()
finishes in float64 on the host from one 32 * n_features byte copy.  Keys (one spelling for both reference routines):
MAE, MSE, RMSE, R2 (flat), MeanR2 (uniform average of the per-feature R^2), CosineSimilarity, PearsonMean, PearsonStd (population),
PearsonValid (rows whose r is not NaN), _pearson_all (per-row tensor on the device, NaN kept in place).
"""
import numpy as np
import torch

from . import ops


def _r2(ss_res, ss_tot):
    """1 - SS_res / SS_tot with sklearn's force_finite default: where SS_tot == 0, 1.0 if SS_res == 0 else 0.0."""
    ss_res, ss_tot = np.asarray(ss_res, np.float64), np.asarray(ss_tot, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 1.0 - ss_res / ss_tot
    return np.where(ss_tot == 0, np.where(ss_res == 0, 1.0, 0.0), out)


def finalize_columns(col_acc, col_shift, rows):
    """MAE, MSE, RMSE, R2, MeanR2 in float64 from the (4, F) column sums of `rows` samples taken about col_shift (F,):
    y_ij = c_j + t_ij, so  sum_i (y_ij - m)^2 = S1_j + 2 (c_j - m) S0_j + rows (c_j - m)^2  for any m (the column mean: S1 - S0^2 / rows)."""
    s0, s1, ss_res, s_abs = np.asarray(col_acc, np.float64)
    c = np.asarray(col_shift, np.float64)
    F = s0.shape[0]
    count = float(rows) * F
    mse = ss_res.sum() / count
    gmean = (rows * c + s0).sum() / count
    dc = c - gmean
    ss_tot_flat = (s1 + 2.0 * dc * s0 + rows * dc * dc).sum()
    if not s1.any() and (c == c[0]).all():
        # every target element equals c[0]: S1 is a sum of exact zeros (a difference of two distinct fp32 values squares to a normal
        # float64), while gmean above may have rounded and left a tiny positive value where SS_tot is exactly 0
        ss_tot_flat = 0.0
    ss_tot_col = np.maximum(s1 - s0 * s0 / rows, 0.0)
    return {"MAE": float(s_abs.sum() / count), "MSE": float(mse), "RMSE": float(np.sqrt(mse)),
            "R2": float(_r2(ss_res.sum(), ss_tot_flat)), "MeanR2": float(_r2(ss_res, ss_tot_col).mean())}


class ImputationMetrics:
    def __init__(self, n_features, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"ImputationMetrics: the MI355X path needs a CUDA/HIP device (got {device}); there is no CPU fallback")
        self.n_features = int(n_features)
        self.device = device
        self.reset()

    def reset(self):
        self.col_acc = torch.zeros(4, self.n_features, dtype=torch.float64, device=self.device)
        self.col_shift = None            # fixed by the first batch: its first target row
        self.rows = 0
        self._pearson, self._cosine = [], []

    def update(self, y_true, y_pred):
        one_row = isinstance(y_pred, torch.Tensor) and y_pred.dim() == 1          # (F,): the same prediction for every sample
        y_true = ops._device_matrix(y_true, "y_true", "ImputationMetrics")
        y_pred = ops._device_matrix(y_pred[None] if one_row else y_pred, "y_pred", "ImputationMetrics")     # copies e.g. an expanded row
        if one_row:
            y_pred = y_pred[0]
        if y_true.shape[1] != self.n_features:
            raise ValueError(f"ImputationMetrics: y_true is {tuple(y_true.shape)}, need (rows, {self.n_features})")
        M = y_true.shape[0]
        if M == 0:
            return self
        if self.col_shift is None:
            self.col_shift = y_true[0].float().contiguous().clone()
        rp = torch.empty(M, dtype=torch.float32, device=self.device)
        rc = torch.empty(M, dtype=torch.float32, device=self.device)
        ops.recon_metrics(y_pred, y_true, self.col_shift, self.col_acc, rp, rc)
        self._pearson.append(rp)
        self._cosine.append(rc)
        self.rows += M
        return self

    def compute(self):
        if self.rows == 0:
            raise ValueError("ImputationMetrics.compute() before any update()")
        out = finalize_columns(self.col_acc.cpu().numpy(), self.col_shift.cpu().numpy(), self.rows)
        pearson = torch.cat(self._pearson)
        p64 = pearson.double()
        valid = ~torch.isnan(p64)
        n_valid = int(valid.sum())
        if n_valid:
            v = p64[valid]
            mean = v.mean()
            out["PearsonMean"] = float(mean)
            out["PearsonStd"] = float(((v - mean) ** 2).mean().sqrt())             # np.std: population
        else:
            out["PearsonMean"] = out["PearsonStd"] = 0.0                           # compute_metrics:192-193
        out["PearsonValid"] = n_valid
        out["CosineSimilarity"] = float(torch.cat(self._cosine).double().mean())
        out["_pearson_all"] = pearson
        return out


def imputation_metrics(y_true, y_pred):
    """One-shot form: the metrics of y_pred ((rows, F), or (F,) for every row) against y_true (rows, F), both on the device."""
    if not isinstance(y_true, torch.Tensor) or not y_true.is_cuda:
        raise RuntimeError("imputation_metrics: the MI355X path needs CUDA/HIP tensors; there is no CPU fallback")
    return ImputationMetrics(y_true.shape[1], y_true.device).update(y_true, y_pred).compute()
