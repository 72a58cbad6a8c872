"""Restatement of the imputation metrics (mmvae.metrics / mmvae_recon_metrics) in numpy, shared by tests/test_metrics_ref_cpu.py
(against sklearn / scipy and a stored fixture), tests/test_metrics_gpu.py and tests/test_evaluate_gpu.py (device against float64).

Every function takes `dt` like tests/elementwise_bounds.py: np.float64 gives the reference.  The inputs are float32 (or bfloat16)
values held in float arrays and count as exact.  Edge rules, as scipy 1.15 / sklearn 1.7 behave on float64 input:
  Pearson r   NaN when every element of the target row, or of the prediction row, compares equal to the row's first element
              (decided on the values, not on a variance that came out as 0); clipped to [-1, 1]
  cosine      a zero norm is replaced by 1 (sklearn.preprocessing.normalize inside cosine_similarity): a zero row gives 0
  R^2         force_finite: where SS_tot == 0 the score is 1.0 if SS_res == 0 else 0.0 (per feature and flat)
  PearsonMean / PearsonStd are 0.0 when no row is valid; PearsonStd is the population value (np.std)
"""
import numpy as np

KEYS = ("MAE", "MSE", "RMSE", "R2", "MeanR2", "CosineSimilarity", "PearsonMean", "PearsonStd", "PearsonValid", "_pearson_all")


def _a(x, dt):
    return np.asarray(x).astype(dt)


def _pred2d(y, p):
    return np.broadcast_to(p, y.shape) if p.ndim == 1 else p


def constant_rows(y, p):
    """rows on which scipy.stats.pearsonr returns NaN: (x == x[0]).all() for either input"""
    y = np.asarray(y); p = _pred2d(y, np.asarray(p))
    return (y == y[:, :1]).all(axis=1) | (p == p[:, :1]).all(axis=1)


def _sum(x, perm):
    """row sums; perm: a column order in which the terms are added one by one (the kernel's order is not fixed)"""
    if perm is None:
        return x.sum(axis=1)
    s = np.zeros(x.shape[0], x.dtype)
    for j in perm:
        s = s + x[:, j]
    return s


def row_pearson(y, p, dt=np.float64, form="centred", perm=None):
    """form: 'centred' = the two-sweep reference; 'shifted' = the kernel's arithmetic, moments of the row shifted by its own first
    element; 'raw' = moments of the unshifted row (what the kernel must NOT do)."""
    y = _a(y, dt); p = _a(_pred2d(y, np.asarray(p)), dt)
    n = dt(y.shape[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        if form == "centred":
            a, b = y - y.mean(axis=1, keepdims=True), p - p.mean(axis=1, keepdims=True)
            r = _sum(a * b, perm) / (np.sqrt(_sum(a * a, perm)) * np.sqrt(_sum(b * b, perm)))
        else:
            a, b = (y - y[:, :1], p - p[:, :1]) if form == "shifted" else (y, p)
            sa, sb = _sum(a, perm), _sum(b, perm)
            cov = _sum(a * b, perm) - sa * sb / n
            vy, vp = _sum(a * a, perm) - sa * sa / n, _sum(b * b, perm) - sb * sb / n
            r = cov / (np.sqrt(vy) * np.sqrt(vp))
        r = np.where(r > 1, dt(1), np.where(r < -1, dt(-1), r))
    return np.where(constant_rows(y, p), dt(np.nan), r)


def row_cosine(y, p, dt=np.float64, perm=None):
    y = _a(y, dt); p = _a(_pred2d(y, np.asarray(p)), dt)
    ny, npn = np.sqrt(_sum(y * y, perm)), np.sqrt(_sum(p * p, perm))
    ny, npn = np.where(ny == 0, dt(1), ny), np.where(npn == 0, dt(1), npn)
    return _sum(y * p, perm) / (ny * npn)


def col_sums(y, p, shift=None, dt=np.float64):
    """(4, F): sum (y - c), sum (y - c)^2, sum (p - y)^2, sum |p - y| over the rows; c = shift or 0"""
    y = _a(y, dt); p = _a(_pred2d(y, np.asarray(p)), dt)
    t = y - (_a(shift, dt) if shift is not None else dt(0))
    d = p - y
    return np.stack([t.sum(axis=0), (t * t).sum(axis=0), (d * d).sum(axis=0), np.abs(d).sum(axis=0)])


def r2(ss_res, ss_tot):
    ss_res, ss_tot = np.asarray(ss_res), np.asarray(ss_tot)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 1 - ss_res / ss_tot
    return np.where(ss_tot == 0, np.where(ss_res == 0, 1.0, 0.0), out)


def metrics(y, p, dt=np.float64):
    """All ten outputs, two-sweep (centred) forms throughout: what sklearn.metrics / scipy.stats compute on float64 casts."""
    y = _a(y, dt); p = _a(_pred2d(y, np.asarray(p)), dt)
    d = p - y
    mse = (d * d).mean()
    out = {"MAE": np.abs(d).mean(), "MSE": mse, "RMSE": np.sqrt(mse)}
    # SS_tot of constant data is exactly 0 (a rounded mean of a non-dyadic constant would leave a tiny positive value)
    tot = 0.0 if (y == y.flat[0]).all() else ((y - y.mean()) ** 2).sum()
    tot_j = np.where((y == y[:1]).all(axis=0), 0.0, ((y - y.mean(axis=0)) ** 2).sum(axis=0))
    out["R2"] = r2((d * d).sum(), tot)
    out["MeanR2"] = r2((d * d).sum(axis=0), tot_j).mean()
    out["CosineSimilarity"] = row_cosine(y, p, dt).mean()
    r = row_pearson(y, p, dt)
    v = r[~np.isnan(r)]
    out["PearsonMean"] = v.mean() if v.size else 0.0
    out["PearsonStd"] = v.std() if v.size else 0.0
    out["PearsonValid"] = int(v.size)
    out["_pearson_all"] = r
    return {k: (float(v) if np.ndim(v) == 0 and k != "PearsonValid" else v) for k, v in out.items()}


def edge_case(seed=0):
    """The 67 x 45 case of tests/golden/imputation_metrics.npz (tools/make_metrics_fixture.py writes exactly this): float32 (y, p)."""
    g = np.random.default_rng(seed)
    y = np.abs(g.standard_normal((67, 45)))
    p = y + 0.3 * g.standard_normal((67, 45))
    row20 = 1000.0 + 1e-3 * g.standard_normal((2, 45))
    y[:, 11] = 0.75
    y[:, 13] = 0.125; p[:, 13] = 0.125
    y[20], p[20] = row20[0], row20[1]              # the rows after the columns: rows 3, 5, 7 and 9 stay constant
    y[3] = 0.5
    p[5] = 0.25
    y[7] = 0.0
    p[9] = 0.0
    return y.astype(np.float32), p.astype(np.float32)
