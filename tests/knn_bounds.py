"""Derived bounds for mmvae_knn_search / mmvae_knn_mean_rows (include/mmvae_hip.h), nothing tuned.  u = 2^-24 (fp32 unit roundoff),
gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1: n roundings of any nesting).

The kernel ranks candidate j for query i by  key = fl(tn_j - 2 dot_ij),  tn_j = fl(sum (t_j - c)~^2),  dot_ij = fl(sum (q_i - c)~ (t_j - c)~),
x~ = fl(x - c), all fp32, sums of F terms in some fixed order (bf16 storage is widened exactly).  Against the exact
key* = |t - c|^2 - 2 (q - c).(t - c) (c: the fp32 shift values, exactly):
  - each x~ carries one rounding, each product one, each sum of F terms at most F - 1 nested ones, the final fl one, and the product
    by 2 none: every term of tn_j and of 2 dot_ij carries at most 2 + 1 + (F - 1) + 1 = F + 3 roundings, so
        |key - key*| <= tol_ij = gamma(F + 3) (T2_j + 2 QT_ij),      T2_j = sum (t_j - c)^2,  QT_ij = sum |q_i - c| |t_j - c|.
    By Cauchy-Schwarz QT <= |q - c| |t - c|: no looser than (F + 6) u (|t|^2 + 2 |q| |t|).
  - d2 = max(fl(key + qn_i), 0), qn_i = fl(sum (q_i - c)~^2): |qn - Q2_i| <= gamma(F + 2) Q2_i, and the final sum rounds once more:
        |d2 - |q - t|^2| <= tol_ij + gamma(F + 2) Q2_i + u (1 + gamma(F + 3)) (T2_j + 2 QT_ij + Q2_i)      (the clamp moves d2 towards the exact value).
The same |q - c|^2 is added to every key of a query, so the ranking by key is the ranking by d2* = key* + Q2 up to tol.  With E the exact
k nearest of query i (by (d2*, j)), D_k their largest d2*, tau_E = max_{e in E} tol_ie:
  - a row m outside E is only returned in place of some e in E, i.e. with key_m <= key_e, so d2*_m - tol_im <= D_k + tau_E.  C = the set
    of rows satisfying that (it contains E and every row the kernel can return), tau_C = max_{m in C} tol_im, band = 2 tau_C.
  - every returned row has d2* <= D_k + tau_E + tol_im <= D_k + band; a row j with d2*_j < D_k - band that was left out would have lost
    to a returned m with d2*_m >= D_k, i.e. D_k <= d2*_j + tol_im + tol_ij <= d2*_j + band: it is returned; two consecutive returned
    rows (m1 before m2) have key_m1 <= key_m2, so d2*_m1 <= d2*_m2 + band.
  - if the (k+1)-th distance exceeds D_k by more than band, no m outside E can replace an e in E: the query is DECIDED and the
    returned set is E.
mean_rows: k terms summed in ascending order (k - 1 roundings) and one correctly rounded division:
        |out - mean| <= gamma(k) mean |y|."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def pair_terms(q, t, shift=None):
    """T2 (Nt,), Q2 (Mq,), QT (Mq, Nt) in float64 of the values the kernel reads"""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    if shift is not None:
        c = np.asarray(shift, np.float64)
        q, t = q - c, t - c
    return (t * t).sum(axis=1), (q * q).sum(axis=1), np.abs(q) @ np.abs(t).T


def key_tol(q, t, shift=None):
    """tol_ij (Mq, Nt)"""
    T2, _, QT = pair_terms(q, t, shift)
    return gamma(q.shape[1] + 3) * (T2[None, :] + 2.0 * QT)


def dist2_tol(q, t, shift=None):
    T2, Q2, QT = pair_terms(q, t, shift)
    F = q.shape[1]
    base = T2[None, :] + 2.0 * QT
    return gamma(F + 3) * base + gamma(F + 2) * Q2[:, None] + U * (1.0 + gamma(F + 3)) * (base + Q2[:, None])


def analyse(q, t, k, shift=None):
    """dict(d (Mq, Nt) exact d2, order (Mq, Nt) exact ranking, Dk (Mq,), band (Mq,), decided (Mq,) bool, tol (Mq, Nt))"""
    import knn_ref
    d = knn_ref.dist2(q, t)
    tol = key_tol(q, t, shift)
    order = np.argsort(d, axis=1, kind="stable")
    Mq, Nt = d.shape
    Dk = np.take_along_axis(d, order[:, k - 1:k], axis=1)[:, 0]
    tau_e = np.take_along_axis(tol, order[:, :k], axis=1).max(axis=1)
    in_c = d - tol <= (Dk + tau_e)[:, None]
    tau_c = np.where(in_c, tol, 0.0).max(axis=1)
    band = 2.0 * tau_c
    if k < Nt:
        gap = np.take_along_axis(d, order[:, k:k + 1], axis=1)[:, 0] - Dk
        decided = gap > band
    else:
        decided = np.ones(Mq, bool)
    return dict(d=d, order=order, Dk=Dk, band=band, decided=decided, tol=tol)


def check_search(q, t, k, idx, dist2=None, shift=None, label="", an=None):
    """Asserts that idx (Mq, k) (and dist2) is a valid answer; returns the analysis with the count of undecided queries."""
    an = analyse(q, t, k, shift) if an is None else an
    d, Dk, band = an["d"], an["Dk"], an["band"]
    Mq, Nt = d.shape
    idx = np.asarray(idx).astype(np.int64)
    assert idx.shape == (Mq, k), (label, idx.shape)
    assert ((idx >= 0) & (idx < Nt)).all(), (label, "index out of range", np.argwhere((idx < 0) | (idx >= Nt))[:5])
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), (label, "repeated index", np.flatnonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))[:5])
    got = np.take_along_axis(d, idx, axis=1)
    assert (got <= (Dk + band)[:, None]).all(), (label, "a returned row lies beyond the band", np.argwhere(got > (Dk + band)[:, None])[:5])
    member = np.zeros((Mq, Nt), bool)
    np.put_along_axis(member, idx, True, axis=1)
    must = d < (Dk - band)[:, None]
    assert not (must & ~member).any(), (label, "a row closer than the band was left out", np.argwhere(must & ~member)[:5])
    assert (got[:, :-1] <= got[:, 1:] + band[:, None]).all(), (label, "not ascending", np.argwhere(got[:, :-1] > got[:, 1:] + band[:, None])[:5])
    exact = np.sort(an["order"][:, :k], axis=1)
    dec = an["decided"]
    assert (srt[dec] == exact[dec]).all(), (label, "a decided query differs from the float64 set", np.flatnonzero(dec)[(srt[dec] != exact[dec]).any(axis=1)][:5])
    if dist2 is not None:
        dist2 = np.asarray(dist2, np.float64)
        tol_d = np.take_along_axis(dist2_tol(q, t, shift), idx, axis=1)
        err = np.abs(dist2 - got)
        assert np.isfinite(dist2).all() and (err <= tol_d).all(), (label, "dist2", np.argwhere(~(err <= tol_d))[:5], float(np.nanmax(err / tol_d)))
    an["undecided"] = int((~dec).sum())
    return an


def mean_rows_tol(idx, y):
    """bound (Mq, Fy) on |out - float64 mean over the given indices|"""
    a = np.abs(np.asarray(y, np.float64))[np.asarray(idx)]
    return gamma(a.shape[1]) * a.mean(axis=1) + 2.0 ** -149
