"""Derived error bounds of mmvae_standardize_fit / mmvae_standardize_apply against tests/standardize_ref.py.  Nothing here is tuned: every
term is a count of float64 roundings times the magnitude it acts on, taken from the data.

The kernel's form (include/mmvae_hip.h).  Per column, with n rows, shift c = x_0 (the column's first row, an fp32 value):
    a_i = fl(x_i - c)                                  one rounding (exact unless the exponents of x_i and c are > 29 bits apart)
    S0 = sum a_i,  S1 = sum fl(a_i^2)                  any order with at most P = n + 3 + splits additions on a path
                                                       (rows of a wave of a split, 3 to join the waves, splits - 1 to join the splits)
    d = fl(S0 / n),  mean = fl(c + d),  var = fl(fl(S1 / n) - fl(d^2)),  scale = sqrt(var)
U = 2^-53, gamma(k) = k U / (1 - k U) (Higham, Accuracy and Stability, lemma 3.1).  With A1 = mean |x_i - c|, A2 = mean (x_i - c)^2,
dx = mean(x) - c (exact values):
    |S0/n - dx|     <= gamma(P + 1) A1                  (1 rounding of a_i + P additions)
    |d - dx|        <= gamma(P + 1) A1 + U |dx|  =: Ed  (the division)
    |mean - mean*|  <= Ed + U |mean*|                   (the last addition)               + U |mean*|  the yardstick's own rounding
    |S1/n - A2|     <= gamma(P + 3) A2                  (2 roundings in a_i^2 from a_i, 1 from the product, P additions)
    |var - var*|    <= gamma(P + 3) A2 + U A2           (the division)
                       + 2 |dx| Ed + Ed^2 + U dx^2      (d^2 against dx^2, and its rounding)
                       + U var*                         (the subtraction)                  + U var*     the yardstick's own rounding
var* = A2 - dx^2, so the terms in A2 and dx^2 carry the amplification (mean - shift)^2 / var of the shifted one-pass form: for the column
whose first row is the only outlier, dx^2 / var* ~ n.  A fused multiply-add in place of a product and a sum only removes roundings.
The clamp var = max(var, 0) moves var towards var* >= 0.  A constant column has a_i = 0: every term but the roundings of mean* is zero.
    |scale - scale*| <= |var - var*| / sqrt(var*)  (|sqrt(v + e) - sqrt(v)| = |e| / (sqrt(v + e) + sqrt(v)) <= |e| / sqrt(v), v + e >= 0)
                        + 4 U scale*               (the kernel's square root: at most 1 ulp = 2 U; the yardstick's: 1 ulp)
    scale = scale* = 1 exactly where the column is constant; the cases keep every other column 1e6 above the constant rule's threshold.

z after a device fit.  z* = (x - mean*) / scale* in exact arithmetic of the yardstick's mean*, scale*; the kernel forms
fl32(fl(fl(x - mean) / scale)):
    E = (|dmean| + |z*| |dscale|) / (scale* - |dscale|)      propagation of the fit's errors
        + 3 U (|z*| + that)                                  the subtraction, the division, and the yardstick's z64 (2 roundings)
    |z - z*| <= E + half an fp32 ulp at (|z*| + E)
With the yardstick's own mean and scale the kernel is bit-equal to numpy's expression: no bound is involved."""
import numpy as np

U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def fit_tol(X, splits):
    """(mean_tol, var_tol, scale_tol), float64 (F,), for the matrix X (rows, F) of fp32-representable values and `splits` row splits.
    Also returns nothing else: the yardstick values come from standardize_ref.fit."""
    Xl = np.asarray(X).astype(np.longdouble)
    n = Xl.shape[0]
    a = Xl - Xl[0]
    A1 = np.abs(a).mean(axis=0).astype(np.float64)
    A2 = (a * a).mean(axis=0).astype(np.float64)
    dx = a.mean(axis=0).astype(np.float64)
    mean = (Xl[0] + a.mean(axis=0)).astype(np.float64)
    var = np.maximum(((a - a.mean(axis=0)) ** 2).mean(axis=0).astype(np.float64), 0.0)
    P = n + 3 + splits
    Ed = gamma(P + 1) * A1 + U * np.abs(dx)
    mean_tol = Ed + 2 * U * np.abs(mean)
    var_tol = gamma(P + 3) * A2 + U * A2 + 2 * np.abs(dx) * Ed + Ed * Ed + U * dx * dx + 2 * U * var
    nonconst = A2 > 0
    scale = np.sqrt(var)
    scale_tol = np.where(nonconst, var_tol / np.where(nonconst, scale, 1.0) + 4 * U * scale, 0.0)
    return mean_tol, var_tol, scale_tol


def z_tol(z64, scale, mean_tol, scale_tol):
    """elementwise bound of |z_device - z64| after a fit whose mean / scale are within mean_tol / scale_tol of the yardstick's"""
    az = np.abs(z64)
    prop = (mean_tol + az * scale_tol) / (scale - scale_tol)
    E = prop + 3 * U * (az + prop)
    return E + 0.5 * np.spacing((az + E).astype(np.float32)).astype(np.float64)
