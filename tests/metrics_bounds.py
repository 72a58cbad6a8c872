"""DERIVED error bounds of mmvae_recon_metrics (csrc/metrics.hip) and of the dictionary mmvae.metrics builds on it, against the
float64 restatement tests/metrics_ref.py.  Style and constants of tests/elementwise_bounds.py; nothing is fitted to kernel output.

The roundings that are counted:
  loads    fp32 / bf16 values widened to float64: exact.  A product of two such values is exact in float64 (48 significant bits).
  F64      2^-53: one float64 operation (a difference y - c, a square of a rounded value, one addition of a sum, a multiply).
  sums     n terms added in ANY order (registers, wave exchanges, LDS and global atomics, several launches): (n - 1) F64 sum |terms|.
           A fused multiply-add drops one rounding; the uncontracted count covers both forms.
  E64_DIV, E64_SQRT   float64 division / square root on the device: 2.5 ulp / 1 ulp, the same ulp counts elementwise_bounds assumes
           for fp32 (not taken as correctly rounded).
  U        2^-24: the fp32 store of r and of the cosine.
  REF      the reference is a float64 sum in an order of its own, so a difference "kernel - reference" carries the any-order bound
           twice: every float64 term below is doubled.  (The fp32 store is the kernel's alone.)
  SECOND   first-order analysis: every relative term that enters is kept below 2^-10; where the data do not allow that
           (a variance or an SS_tot not clearly above its own error) the bound says so with +inf instead of pretending.
Errors are relative to the magnitude of the TERMS (sums of absolute values), never to a result that may have cancelled.
"""
import numpy as np

from elementwise_bounds import U, F64, SECOND

ULP64 = 2 * F64
E64_DIV = 2.5 * ULP64
E64_SQRT = 1 * ULP64
REF = 2.0
SMALL = 2.0 ** -10


def _pred2d(y, p):
    return np.broadcast_to(p, y.shape) if p.ndim == 1 else p


def col_tol(y, p, shift=None, prior=None):
    """(4, F) bound of col_acc after adding the M rows of (y, p) to `prior` (None = zeros).
    t = y - c: one rounding per term; M terms and the prior are added in any order: M additions -> (M + 1) F64 (sum |t| + |prior|).
    t^2 and d^2 = (p - y)^2: the rounded difference enters twice and the square rounds once: 3 F64 per term -> (M + 3) F64.
    |d|: as t."""
    y = np.asarray(y, np.float64); p = np.asarray(_pred2d(y, np.asarray(p)), np.float64)
    M = y.shape[0]
    t = y - (np.asarray(shift, np.float64) if shift is not None else 0.0)
    d = p - y
    pr = np.zeros((4, y.shape[1])) if prior is None else np.abs(np.asarray(prior, np.float64))
    mags = np.stack([np.abs(t).sum(0), (t * t).sum(0), (d * d).sum(0), np.abs(d).sum(0)]) + pr
    n = np.array([M + 1, M + 3, M + 3, M + 1], np.float64)[:, None]
    return REF * SECOND * n * F64 * mags


def pearson_tol(y, p):
    """(M,) bound of row_pearson; 0 on the rows where the reference is NaN (NaN positions are compared exactly, not within a bound).
    With a = y - y[0], b = p - p[0] (one rounding each) and n = F terms per row:
      Sa, Sb          n F64 sum |a|                      (n - 1 additions + the rounding of a)
      Sab, Saa, Sbb   (n + 2) F64 sum |a b|              (a, b, the product, n - 1 additions)
      cov = Sab - Sa Sb / n:   dSab + (|Sb| dSa + |Sa| dSb) / n + (F64 + E64_DIV) |Sa Sb| / n + F64 (|Sab| + |Sa Sb| / n)
      vy  = Saa - Sa^2 / n:    dSaa + 2 |Sa| dSa / n + (F64 + E64_DIV) Sa^2 / n + F64 (Saa + Sa^2 / n);  vp likewise
      r = cov / (sqrt vy * sqrt vp):  dcov / (sy sp) + |r| (dvy / 2 vy + dvp / 2 vp + 2 E64_SQRT + F64 + E64_DIV)
    the clamp to [-1, 1] moves r towards the true value; then the fp32 store: U |r|.
    +inf where dvy > 2^-10 vy (or vp): the row's variance is not clearly above its own rounding."""
    y = np.asarray(y, np.float64); p = np.asarray(_pred2d(y, np.asarray(p)), np.float64)
    n = float(y.shape[1])
    a, b = y - y[:, :1], p - p[:, :1]
    sa, sb = a.sum(1), b.sum(1)
    A1, B1 = np.abs(a).sum(1), np.abs(b).sum(1)
    saa, sbb, sab, sab_abs = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1), np.abs(a * b).sum(1)
    dsa, dsb = n * F64 * A1, n * F64 * B1
    dcov = ((n + 2) * F64 * sab_abs + (np.abs(sb) * dsa + np.abs(sa) * dsb) / n + (F64 + E64_DIV) * np.abs(sa * sb) / n
            + F64 * (np.abs(sab) + np.abs(sa * sb) / n))

    def dvar(s1, s2, ds1):
        return (n + 2) * F64 * s2 + 2 * np.abs(s1) * ds1 / n + (F64 + E64_DIV) * s1 * s1 / n + F64 * (s2 + s1 * s1 / n)
    dvy, dvp = dvar(sa, saa, dsa), dvar(sb, sbb, dsb)
    yc, pc = y - y.mean(1, keepdims=True), p - p.mean(1, keepdims=True)
    vy, vp, cov = (yc * yc).sum(1), (pc * pc).sum(1), (yc * pc).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.clip(cov / np.sqrt(vy * vp), -1, 1)
        tol = REF * SECOND * (dcov / np.sqrt(vy * vp) + np.abs(r) * (dvy / (2 * vy) + dvp / (2 * vp) + 2 * E64_SQRT + F64 + E64_DIV))
        tol = tol * (1 + U) + U * np.abs(r)
        tol = np.where((dvy > SMALL * vy) | (dvp > SMALL * vp), np.inf, tol)
    const = (y == y[:, :1]).all(1) | (p == p[:, :1]).all(1)
    return np.where(const, 0.0, tol)


def cosine_tol(y, p):
    """(M,) bound of row_cosine.  The products y p, y y, p p are exact; Syp: (n - 1) F64 sum |y p|; Syy, Spp (positive terms):
    relative (n - 1) F64, halved by the square root; two square roots, their product and the division; the fp32 store.
    A zero norm is replaced by 1 and the numerator is then a sum of exact zeros: the bound is 0."""
    y = np.asarray(y, np.float64); p = np.asarray(_pred2d(y, np.asarray(p)), np.float64)
    n = float(y.shape[1])
    ny, npn = np.sqrt((y * y).sum(1)), np.sqrt((p * p).sum(1))
    zero = (ny == 0) | (npn == 0)
    ny, npn = np.where(ny == 0, 1.0, ny), np.where(npn == 0, 1.0, npn)
    cos = (y * p).sum(1) / (ny * npn)
    tol = REF * SECOND * ((n - 1) * F64 * np.abs(y * p).sum(1) / (ny * npn)
                          + np.abs(cos) * ((n - 1) * F64 + 2 * E64_SQRT + F64 + E64_DIV))
    tol = tol * (1 + U) + U * np.abs(cos)
    return np.where(zero, 0.0, tol)


def _r2_tol(ss_res, ss_tot, d_res, d_tot):
    """1 - res / tot: d_res / tot + res d_tot / tot^2 + (division, subtraction) 2 F64 (1 + res / tot).  Where tot == 0 the branch of
    the force_finite rule is the reference's own only if the computed tot is exactly 0 too, i.e. d_tot == 0 (every term an exact 0); res, a sum of squares
    without cancellation, is 0 on both sides or on neither."""
    ss_res, ss_tot, d_res, d_tot = (np.asarray(v, np.float64) for v in (ss_res, ss_tot, d_res, d_tot))
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = SECOND * (d_res / ss_tot + ss_res * d_tot / ss_tot ** 2 + 2 * F64 * (1 + ss_res / ss_tot))
    tol = np.where(d_tot > SMALL * ss_tot, np.inf, tol)
    return np.where(ss_tot == 0, np.where(d_tot == 0, 0.0, np.inf), tol)


def metrics_tol(y, p, shift):
    """Bounds of the scalar entries of ImputationMetrics.compute() on the rows (y, p) with column shift `shift` (the first target
    row the accumulator saw), host finalisation in float64 included (sums of F column values: F F64 sum |values|).
    Flat R^2: the global mean g from the column sums rows c_j + S0_j, then SS_tot = sum_j S1_j + 2 (c_j - g) S0_j + rows (c_j - g)^2,
    every term with the bound of its factors; per-feature: SS_tot_j = S1_j - S0_j^2 / rows.
    Row aggregates: a mean of values moves by at most the mean of their bounds; a population standard deviation (the norm of the
    centred vector / sqrt n, centring being a projection) by at most the root mean square of their bounds."""
    y = np.asarray(y, np.float64); p = np.asarray(_pred2d(y, np.asarray(p)), np.float64)
    M, F = y.shape
    c = np.asarray(shift, np.float64)
    T = col_tol(y, p, shift)
    t, d = y - c, p - y
    s0, s1, s2, s3 = t.sum(0), (t * t).sum(0), (d * d).sum(0), np.abs(d).sum(0)
    count = float(M) * F
    out = {}
    out["MAE"] = SECOND * (T[3].sum() + (F + 1) * F64 * s3.sum()) / count
    d_mse = SECOND * (T[2].sum() + (F + 1) * F64 * s2.sum()) / count
    mse = s2.sum() / count
    out["MSE"] = d_mse
    out["RMSE"] = d_mse / (2 * np.sqrt(mse)) + F64 * np.sqrt(mse) if mse > 0 and d_mse < SMALL * mse else np.sqrt(d_mse)
    # flat R^2
    colsum = M * c + s0
    d_colsum = T[0] + F64 * (2 * M * np.abs(c) + np.abs(s0))
    g = colsum.sum() / count
    dg = (d_colsum.sum() + (F + 1) * F64 * np.abs(colsum).sum()) / count
    dc = c - g
    d_dc = dg + F64 * np.abs(dc)
    mag = s1 + 2 * np.abs(dc * s0) + M * dc * dc
    d_term = T[1] + 2 * (np.abs(dc) * T[0] + np.abs(s0) * d_dc) + 2 * M * np.abs(dc) * d_dc + 4 * F64 * mag
    ss_tot = (s1 + 2 * dc * s0 + M * dc * dc).sum()
    ss_tot = ((y - y.mean()) ** 2).sum() if ss_tot != 0 else 0.0
    d_res = T[2].sum() + F * F64 * s2.sum()
    d_tot = d_term.sum() + F * F64 * mag.sum()
    if (y == y.flat[0]).all() and (c == c[0]).all():
        ss_tot, d_tot = 0.0, 0.0         # constant data about a constant shift: finalize_columns decides SS_tot == 0 on exact zeros
    out["R2"] = float(_r2_tol(s2.sum(), ss_tot, d_res, d_tot))
    # per-feature R^2
    tot_j = np.where((y == y[:1]).all(0), 0.0, ((y - y.mean(0)) ** 2).sum(0))
    d_tot_j = T[1] + 2 * np.abs(s0) * T[0] / M + (3 * F64 + E64_DIV) * (s1 + s0 * s0 / M)
    tol_j = _r2_tol(s2, tot_j, T[2], d_tot_j)
    with np.errstate(divide="ignore", invalid="ignore"):
        r2_j = np.where(tot_j == 0, 1.0, 1 - s2 / tot_j)
    out["MeanR2"] = float(tol_j.mean() + (F + 1) * F64 * np.abs(r2_j).mean())
    # row aggregates
    tp, tc = pearson_tol(y, p), cosine_tol(y, p)
    valid = ~((y == y[:, :1]).all(1) | (p == p[:, :1]).all(1))
    nv = int(valid.sum())
    out["CosineSimilarity"] = float(tc.mean() + (M + 1) * F64)                  # |cos| <= 1
    out["PearsonMean"] = float(tp[valid].mean() + (nv + 1) * F64) if nv else 0.0
    out["PearsonStd"] = float(np.sqrt((tp[valid] ** 2).mean()) + (nv + 4) * F64) if nv else 0.0
    return {k: float(v) for k, v in out.items()}
