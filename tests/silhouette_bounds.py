"""Derived bounds for mmvae_silhouette_samples (include/mmvae_hip.h), nothing tuned.  u = 2^-24 (fp32 unit roundoff),
gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1: n roundings of any nesting).

The kernel forms  d2_ij = fl(fl(qn_i + tn_j) - 2 dot_ij),  qn_i = fl(sum (x_i - c)~^2),  dot_ij = fl(sum (x_i - c)~ (x_j - c)~),
x~ = fl(x - c), all fp32, sums of F terms in some fixed order (bf16 storage is widened exactly).  Against d2*_ij = |x_i - x_j|^2:
  - every x~ carries one rounding, a product of two one more, a sum of F terms at most F - 1 nested ones, the sum of the two norms one
    and the final difference one (the product by 2 none): every term of qn_i, tn_j and 2 dot_ij carries at most 2 + 1 + (F - 1) + 2
    = F + 4 roundings, so
        |d2 - d2*| <= tol2_ij = gamma(F + 4) (Q2_i + Q2_j + 2 QT_ij),     Q2_i = sum (x_i - c)^2,  QT_ij = sum |x_i - c| |x_j - c|
    (c: the fp32 shift values, exactly; the clamp at 0 moves d2 towards d2* >= 0).
  - d = sqrt(d2), correctly rounded up to 2 u:  |sqrt(d2) - d*| = |d2 - d2*| / (sqrt(d2) + d*) <= min(sqrt(tol2), tol2 / d*), so
        |d - d*| <= delta_ij = min(sqrt(tol2_ij), tol2_ij / d*_ij) (1 + 2 u) + 2 u d*_ij,      delta_ii = 0 (the diagonal is forced to 0).
  - S_ic = the fp32 sum of the class's d_ij in the kernel's order.  The longest chain of additions one term passes through: the lane's
    four columns (3), the butterfly over 16 lanes (4), the pair of column waves (1), the tiles of the class a split owns (at most
    the class's tiles, including the first addition to 0), the splits (nsplit - 1):  depth_c = 8 + tiles_c + nsplit - 1, and
        |S_ic - S*_ic| <= dS_ic = sum_j delta_ij + gamma(depth_c) sum_j (d*_ij + delta_ij).
  - a = S / (n - 1), b = min_c S_c / n_c: a correctly rounded division each, budgeted 2 u (n is exact in fp32 below 2^24):
        |a - a*| <= da = (dS / (n - 1)) (1 + 2 u) + 2 u a*,    |mean_c - mean*_c| likewise, and the minimum over classes is 1-Lipschitz in
    the maximum norm:  |b - b*| <= db = max_c of the classes' bounds.
  - s = (b - a) / max(a, b) is increasing in b and decreasing in a (for a, b >= 0), and the kernel's own s is formed from its a and b with
    one subtraction and one division (3 u with the 2 u division budget, |s| <= 1):
        s(a* + da, max(b* - db, 0)) - 3 u <= s <= s(max(a* - da, 0), b* + db) + 3 u.
    A row alone in its class has s = 0 and a = 0 exactly.
  - row_perturbation p (N,): the rows the kernel reads are not x but rows within p_i of x_i in the euclidean norm (x rounded to fp32
    by the caller, say); every distance then moves by at most p_i + p_j, which is added to delta_ij off the diagonal."""
import numpy as np

import silhouette_ref as SR

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def analyse(x, codes, C, shift=None, nsplit=1, row_perturbation=None):
    """dict(a, b, s: float64 reference, da, db, s_lo, s_hi (N,), single (N,) bool, dD (N, N) bound on every distance) in row order"""
    x = np.asarray(x, np.float64)
    codes = np.asarray(codes).astype(np.int64)
    N, F = x.shape
    ref = SR.parts(x, codes, C)
    D = ref["D"]
    xc = x if shift is None else x - np.asarray(shift, np.float64)
    Q2 = (xc * xc).sum(axis=1)
    QT = np.abs(xc) @ np.abs(xc).T
    tol2 = gamma(F + 4) * (Q2[:, None] + Q2[None, :] + 2.0 * QT)
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.minimum(np.sqrt(tol2), np.where(D > 0, tol2 / np.where(D > 0, D, 1.0), np.inf)) * (1.0 + 2.0 * U) + 2.0 * U * D
    if row_perturbation is not None:
        p = np.asarray(row_perturbation, np.float64)
        delta = delta + p[:, None] + p[None, :]
    np.fill_diagonal(delta, 0.0)
    _, start = SR.grouping(codes, C)
    tiles = SR.tiles_of(start)
    n = ref["n"]
    dS = np.zeros((N, C))
    for c in range(C):
        m = codes == c
        depth = 8 + int(tiles[c]) + nsplit - 1
        dS[:, c] = delta[:, m].sum(axis=1) + gamma(depth) * (D[:, m] + delta[:, m]).sum(axis=1)
    rows = np.arange(N)
    own = n[codes]
    single = own == 1
    da = np.where(single, 0.0, dS[rows, codes] / np.maximum(own - 1, 1) * (1.0 + 2.0 * U) + 2.0 * U * ref["a"])
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(n[None, :] > 0, ref["S"] / np.maximum(n, 1)[None, :], 0.0)
        dmean = np.where(n[None, :] > 0, dS / np.maximum(n, 1)[None, :] * (1.0 + 2.0 * U) + 2.0 * U * mean, 0.0)
    dmean[rows, codes] = 0.0
    db = dmean.max(axis=1)
    a, b = ref["a"], ref["b"]
    s_lo = np.where(single, 0.0, SR.s_of(a + da, np.maximum(b - db, 0.0)) - 3.0 * U)
    s_hi = np.where(single, 0.0, SR.s_of(np.maximum(a - da, 0.0), b + db) + 3.0 * U)
    return dict(a=a, b=b, s=ref["s"], da=da, db=db, s_lo=s_lo, s_hi=s_hi, single=single, dD=delta, D=D)


def outside(an, a, b, s):
    """number of rows whose a, b or s lies outside its bound (a NaN lies outside)"""
    a, b, s = (np.asarray(v, np.float64) for v in (a, b, s))
    bad = ~(np.abs(a - an["a"]) <= an["da"]) | ~(np.abs(b - an["b"]) <= an["db"]) | ~((s >= an["s_lo"]) & (s <= an["s_hi"]))
    return int(bad.sum())


def check(an, a, b, s, label=""):
    """asserts a, b, s (N,) within their bounds; returns the largest error of a and b relative to its bound"""
    a, b, s = (np.asarray(v, np.float64) for v in (a, b, s))
    ea, eb = np.abs(a - an["a"]), np.abs(b - an["b"])
    assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(s).all(), (label, "non-finite")
    assert (ea <= an["da"]).all(), (label, "a", np.flatnonzero(~(ea <= an["da"]))[:5], float(ea.max()), float(an["da"].max()))
    assert (eb <= an["db"]).all(), (label, "b", np.flatnonzero(~(eb <= an["db"]))[:5], float(eb.max()), float(an["db"].max()))
    ok = (s >= an["s_lo"]) & (s <= an["s_hi"])
    assert ok.all(), (label, "s", np.flatnonzero(~ok)[:5], s[~ok][:5], an["s_lo"][~ok][:5], an["s_hi"][~ok][:5])
    assert (s[an["single"]] == 0).all() and (a[an["single"]] == 0).all(), (label, "a row alone in its class")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(an["da"] > 0, ea / an["da"], 0.0))), float(np.nanmax(np.where(an["db"] > 0, eb / an["db"], 0.0)))
