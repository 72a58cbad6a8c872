"""Bounds of the unmatched-sample clustering (mmvae.unmatched) against the records of tests/golden/unmatched_clustering.npz, composed
from the pieces' own derived bounds: standardize_bounds (StandardScaler), knn_bounds.mean_rows_tol (the imputed kNN rows),
silhouette_bounds (the silhouette, with its row_perturbation term as the Lipschitz term in max_i |dZ_i|).  Nothing is tuned.

block_tol: how far an element of the device's imputed block may lie from the recorded one.
  mean row   one fp32 ulp between the device's row and the restatement's: both are the fp32 rounding of a float64 column mean, formed
             in different orders.  The RECORDED row is further away: SimpleImputer takes np.ma.mean of the float32 training matrix,
             which accumulates in float32 over the n training rows (measured on the fixture: up to 3 fp32 ulps at n = 96), so against
             the record the bound is sklearn's own, gamma(n) |value| for positive data (train_rows=n).  It never reaches Z: a
             mean-imputed column is constant, and z = 0 exactly on both sides.
  kNN rows   knn_bounds.mean_rows_tol for the device's fp32 mean over the k neighbours PLUS the same for sklearn's own float32 mean
             (the neighbour sets are equal: the fixture's seed decides every query).  The fixture's targets are positive, so the mean
             of magnitudes mean_rows_tol uses IS the value: gamma(k) |value| + 2^-149, twice.
  log1p on top (scaling="reference", DNA-only): |d log1p| <= |dx| for x >= 0, plus half an fp32 ulp of the result on either side.
z_tol_record: |Z_device - Z_recorded|.  The block's tolerance T moves the column mean by at most max T and the scale by at most 2 max T
  (a standard deviation is 1-Lipschitz in the rms of the centred perturbation); the rest is standardize_bounds.z_tol around the float64
  z of the recorded features, T / scale for the element itself, and sklearn's in-place float32 transform (a second rounding: half an
  fp32 ulp of (x - mean) over scale, and half an fp32 ulp of z)."""
import numpy as np

import knn_bounds as KB
import silhouette_bounds as SB
import standardize_bounds as B
import standardize_ref as StdR


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a)).astype(np.float32)).astype(np.float64)


def block_tol(block, method, k, log1p_on_top, train_rows=None):
    """(rows, cols) bound on |device block - recorded block|; block: the recorded block (after its log1p, if any).  train_rows: add
    the float32 accumulation of sklearn's own mean row over that many rows (comparisons of a mean row with the RECORD)"""
    b = np.abs(np.asarray(block, np.float64))
    raw = np.expm1(b) if log1p_on_top else b
    t = ulp32(raw) if method == "mean" else 2.0 * (KB.gamma(k) * raw + 2.0 ** -149)
    if method == "mean" and train_rows:
        t = t + KB.gamma(train_rows) * raw
    return t + ulp32(b) if log1p_on_top else t


def z_tol_record(F, T, splits):
    """F (rows, cols) recorded float32 features, T (rows, cols) elementwise tolerance of the device's features -> (z64, tol)"""
    mean, var, scale = StdR.fit(F)
    z64 = StdR.apply64(np.asarray(F, np.float32), mean, scale)
    mt, vt, st = B.fit_tol(F, splits)
    exact = np.ptp(np.asarray(F), axis=0) == 0
    Tc = np.where(exact, 0.0, T.max(axis=0))
    mt2, st2 = mt + Tc, st + 2.0 * Tc
    tol = B.z_tol(z64, scale, mt2, st2) + np.where(exact, 0.0, T) / (scale - st2)
    tol = tol + 0.5 * ulp32(np.asarray(F, np.float64) - mean) / scale + 0.5 * ulp32(z64)
    return z64, tol


def silhouette_interval(Z, labels, row_err, nsplit):
    """[lo, hi] of the device's silhouette_score of rows within row_err (N,) of Z (float64) in the euclidean norm"""
    values, codes = np.unique(np.asarray(labels), return_inverse=True)
    shift = np.asarray(Z, np.float64).mean(axis=0).astype(np.float32)
    an = SB.analyse(Z, codes, len(values), shift, nsplit, row_perturbation=row_err)
    slack = len(codes) * 2.0 ** -53
    return float(an["s_lo"].mean()) - slack, float(an["s_hi"].mean()) + slack
