"""sklearn.preprocessing.StandardScaler restated in numpy, the yardstick of mmvae_standardize_fit / mmvae_standardize_apply
(include/mmvae_hip.h) and of mmvae.clustering.StandardScaler.

    mean, var, scale = fit(X)          # float64 (F,): two-pass column mean and population variance, sklearn's constant-feature rule
    z = apply(X32, mean, scale)        # ((x.astype(f8) - mean) / scale).astype(f4): the expression the kernel is bit-equal to
    z64 = apply64(X32, mean, scale)    # the same before the rounding to fp32

The results are float64.  The two passes ACCUMULATE in numpy's longdouble (64 mantissa bits here) so that the yardstick's own error is
one rounding of the result -- U |mean|, U var -- and not the 16 + log2(n) roundings of a float64 pairwise sum, which for a column
1e4 +- 1e-2 would be ten times the error the kernel is allowed (tests/standardize_bounds.py)."""
import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "standardize_ref needs an extended-precision longdouble for its accumulators"

EPS = np.finfo(np.float64).eps


def constant_threshold(n, mean, var):
    """sklearn.utils.extmath._is_constant_feature's bound: var <= this means 'constant'"""
    return n * EPS * var + (n * mean * EPS) ** 2


def fit(X):
    """X: (rows, F), any float dtype holding fp32-representable values"""
    Xl = np.asarray(X).astype(np.longdouble)
    n = Xl.shape[0]
    mean_l = Xl.sum(axis=0) / n
    var_l = ((Xl - mean_l) ** 2).sum(axis=0) / n
    mean, var = mean_l.astype(np.float64), var_l.astype(np.float64)
    constant = var <= constant_threshold(n, mean, var)
    scale = np.where(constant, 1.0, np.sqrt(var))
    return mean, var, scale


def apply64(X32, mean, scale):
    X32 = np.asarray(X32)
    assert X32.dtype == np.float32
    return (X32.astype(np.float64) - mean) / scale


def apply(X32, mean, scale):
    return apply64(X32, mean, scale).astype(np.float32)


def splits_used(rows, F, splits=0):
    """(splits_used, rows_per_split): the header's planner formula of mmvae_standardize_fit_splits"""
    ctiles = -(-F // 64)
    want = splits if splits > 0 else max(1, min(2048 // ctiles, rows // 32))
    want = min(want, 64, rows)
    rps = -(-rows // want)
    return -(-rows // rps), rps


def work_bytes(rows, F, splits=0):
    return 16 * F * splits_used(rows, F, splits)[0]
