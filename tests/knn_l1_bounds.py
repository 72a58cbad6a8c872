"""Derived bounds for mmvae_knn_search_l1 / mmvae_knn_weighted_rows (include/mmvae_hip.h) and float32 emulations of both kernels with
switches for the mistakes a kernel could make; nothing tuned.  u = 2^-24, gamma(n) = n u / (1 - n u) as in tests/knn_bounds.py.

Search.  The kernel's key is ONE fp32 chain  key = fl(..fl(fl(|d_0| + |d_1|) + |d_2|).. + |d_{F-1}|),  d_c = fl(q_c - t_c)  (bf16
storage is widened exactly; |.| and 0 + |d_0| are exact).  Every term carries the rounding of its subtraction and at most F - 1
roundings of the additions it passes through, 1 + (F - 1) = F in all, so against key* = sum |q_c - t_c|:
        |key - key*| <= tol_ij = gamma(F) key*_ij.
The returned distance is the key, so it obeys the same bound.  (key* is formed here in float64 from fp32 values: its own error,
F 2^-53 key*, is 2^-29 of the bound and is ignored.)  From d = key* and tol, the candidate set, band = 2 tau_C and DECIDED follow word
for word as in tests/knn_bounds.py (the argument there uses nothing about the key but |key - key*| <= tol); analyse() returns the
dictionary knn_bounds.check_search(..., an=) accepts.

Weighted rows.  Given (idx, dist) -- the kernel's own inputs -- let d_n = dist_n (or sqrt(dist_n) when squared), w*_n = 1 / d_n exactly
(or the 0 / 1 indicator when a d_n is 0, which the kernel forms exactly), p_n = w*_n / sum_m w*_m, ref = sum_n p_n y_n in float64.
The kernel's weight carries 1 rounding (the division) plus 1 for the square root; a term of the numerator then 1 for the product and at
most k - 1 for the sum: k + 2.  The denominator's terms carry 2 + (k - 1) = k + 1; all weights are >= 0, so the denominator is
(sum w*) (1 + theta_{k+1}).  The final division adds 1.  Every term of out = N^ / D^ is therefore p_n y_n (1 + theta_{(k+2)+(k+1)+1}):
        |out - ref| <= gamma(2 k + 4) sum_n p_n |y_n|      (+ 2^-149 for a result in the subnormal range).

Regressor against a float64 reference (sklearn on float64 copies).  When the neighbour SET is the exact one (decided queries) the device
differs from the reference by the bound above plus the effect of its fp32 distances on the weights: d^_n = d_n (1 + e_n) with
|e_n| <= rho, so w^_n = w_n (1 + eta_n), |eta_n| <= rho / (1 - rho) =: rho'.  Normalised weights then move by the factor
(1 + eta_n) / sum_m p_m (1 + eta_m) in [(1 - rho') / (1 + rho'), (1 + rho') / (1 - rho')]: |p^_n - p_n| <= kappa p_n, kappa = 2 rho' / (1 - rho').
        |pred - ref| <= (kappa + gamma(2 k + 4) (1 + kappa)) sum_n p_n |y_n|.
rho: manhattan gamma(F) (above); euclidean from |d2^ - d2| <= knn_bounds.dist2_tol: d^ / d = sqrt(1 + e / d2) within
1 -+ r / (2 (1 - r)) for r = tol / d2 < 1, and one more rounding for the kernel's square root is already counted in gamma(2 k + 4).
Uniform weights: knn_bounds.mean_rows_tol.  MSE: |mse^ - mse| <= mean(2 |ref - y| b + b^2) for an elementwise prediction bound b."""
import numpy as np

from knn_bounds import U, gamma  # noqa: F401

CHUNK = 32            # columns per chunk of the kernel's pipeline


# ---------------------------------------------------------------------------------------------------------------------------
# search
# ---------------------------------------------------------------------------------------------------------------------------
def dist1(q, t):
    """exact-form L1 distances (Mq, Nt) in float64"""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    out = np.empty((q.shape[0], t.shape[0]))
    for i in range(q.shape[0]):
        out[i] = np.abs(t - q[i]).sum(axis=1)
    return out


def key_tol(q, t):
    return gamma(np.shape(q)[1]) * dist1(q, t)


def analyse(q, t, k):
    """the analysis of knn_bounds.analyse for the L1 key: dict(d, order, Dk, band, decided, tol)"""
    d = dist1(q, t)
    tol = gamma(np.shape(q)[1]) * d
    order = np.argsort(d, axis=1, kind="stable")
    Mq, Nt = d.shape
    Dk = np.take_along_axis(d, order[:, k - 1:k], axis=1)[:, 0]
    tau_e = np.take_along_axis(tol, order[:, :k], axis=1).max(axis=1)
    in_c = d - tol <= (Dk + tau_e)[:, None]
    band = 2.0 * np.where(in_c, tol, 0.0).max(axis=1)
    decided = np.take_along_axis(d, order[:, k:k + 1], axis=1)[:, 0] - Dk > band if k < Nt else np.ones(Mq, bool)
    return dict(d=d, order=order, Dk=Dk, band=band, decided=decided, tol=tol)


def check_dist(an, idx, dist, label=""):
    """the returned distances against the float64 distances of the returned rows"""
    idx = np.asarray(idx).astype(np.int64)
    want, tol = np.take_along_axis(an["d"], idx, axis=1), np.take_along_axis(an["tol"], idx, axis=1)
    err = np.abs(np.asarray(dist, np.float64) - want)
    assert np.isfinite(np.asarray(dist)).all() and (err <= tol).all(), (label, "distance", np.argwhere(~(err <= tol))[:5])


def keys_f32(q, t, mistake=None):
    """(Mq, Nt) float32 keys as the header specifies them: one sequential chain over the columns in ascending order.
    mistake: 'squares' | 'drop_last_column' | 'drop_tail_chunk'"""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    F = q.shape[1]
    if mistake == "drop_last_column":
        F -= 1
    if mistake == "drop_tail_chunk" and F > CHUNK:
        F -= F % CHUNK
    acc = np.zeros((q.shape[0], t.shape[0]), np.float32)
    for c in range(F):
        d = q[:, c, None] - t[None, :, c]
        acc = acc + (d * d if mistake == "squares" else np.abs(d))
    return acc


def emulate(q, t, k, mistake=None):
    """(idx (Mq, k) int64, dist (Mq, k) float32) of the kernel, bit for bit: keys_f32 ranked by (key, index), NaN last.
    mistake: those of keys_f32 | 'tie_larger' | 'unsorted' (the k best in arrival order, not ascending)"""
    key = keys_f32(q, t, mistake)
    Nt = key.shape[1]
    if mistake == "tie_larger":
        idx = (Nt - 1 - np.argsort(key[:, ::-1], axis=1, kind="stable"))[:, :k]
    else:
        idx = np.argsort(key, axis=1, kind="stable")[:, :k]
    if mistake == "unsorted":
        idx = np.sort(idx, axis=1)
    return idx, np.take_along_axis(key, idx, axis=1)


# ---------------------------------------------------------------------------------------------------------------------------
# weighted rows
# ---------------------------------------------------------------------------------------------------------------------------
def weights64(dist, squared):
    """(Mq, k) float64 weights of sklearn's _get_weights(dist, 'distance') for the given distances"""
    d = np.asarray(dist, np.float64)
    d = np.sqrt(d) if squared else d
    zero = d == 0
    with np.errstate(divide="ignore"):
        w = 1.0 / d
    rows = zero.any(axis=1)
    w[rows] = zero[rows]
    return w


def weighted_rows(idx, dist, y, squared):
    """float64 weighted mean over the given indices and distances (Mq, Fy)"""
    w = weights64(dist, squared)
    return np.einsum("ik,ikf->if", w, np.asarray(y, np.float64)[np.asarray(idx)]) / w.sum(axis=1)[:, None]


def weighted_rows_tol(idx, dist, y, squared):
    """bound (Mq, Fy) on |out - weighted_rows(idx, dist, y, squared)|"""
    w = weights64(dist, squared)
    p = w / w.sum(axis=1)[:, None]
    k = p.shape[1]
    return gamma(2 * k + 4) * np.einsum("ik,ikf->if", p, np.abs(np.asarray(y, np.float64))[np.asarray(idx)]) + 2.0 ** -149


def weighted_rows_f32(idx, dist, y, squared, mistake=None):
    """the fp32 rows of the kernel.  mistake: 'inv_d2' | 'no_sqrt' | 'no_zero_rule' | 'zero_rule_first_only' | 'divide_by_k'"""
    idx, y = np.asarray(idx), np.asarray(y, np.float32)
    d = np.asarray(dist, np.float32)
    if squared and mistake != "no_sqrt":
        d = np.sqrt(d)
    zero = d == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (np.float32(1) / d).astype(np.float32)
        if mistake == "inv_d2":
            w = (w * w).astype(np.float32)
        if mistake != "no_zero_rule":
            rows = zero.any(axis=1)
            ind = zero.astype(np.float32)
            if mistake == "zero_rule_first_only":
                ind[:, 1:] = 0
            w[rows] = ind[rows]
        s = np.zeros((idx.shape[0], y.shape[1]), np.float32)
        ws = np.zeros(idx.shape[0], np.float32)
        for n in range(idx.shape[1]):
            s = s + w[:, n, None] * y[idx[:, n]]
            ws = ws + w[:, n]
        return s / (np.float32(idx.shape[1]) if mistake == "divide_by_k" else ws[:, None])


# ---------------------------------------------------------------------------------------------------------------------------
# regressors against a float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def predict_tol(X, Y, Xq, k, weights, metric, shift=None):
    """bound (Mq, Fy) on |device prediction - float64 reference| for queries whose neighbour set is the exact one"""
    import knn_bounds as KB
    import knn_ref as KR
    Y = np.asarray(Y, np.float64)
    F = np.shape(X)[1]
    if metric == "manhattan":
        d = dist1(Xq, X)
        idx = np.argsort(d, axis=1, kind="stable")[:, :k]
        dk = np.take_along_axis(d, idx, axis=1)
        rho = np.full(len(dk), gamma(F))
    else:
        idx, d2 = KR.search(Xq, X, k)
        dk = np.sqrt(d2)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.take_along_axis(KB.dist2_tol(Xq, X, shift), idx, axis=1) / d2
        assert (r < 0.5).all(), "a neighbour at distance ~0: the weight bound does not apply"
        rho = (r / (2.0 * (1.0 - r))).max(axis=1)
    if weights == "uniform":
        return KB.mean_rows_tol(idx, Y)
    rho1 = rho / (1.0 - rho)
    kappa = (2.0 * rho1 / (1.0 - rho1))[:, None]
    w = weights64(dk, False)
    p = w / w.sum(axis=1)[:, None]
    return (kappa + gamma(2 * k + 4) * (1.0 + kappa)) * np.einsum("ik,ikf->if", p, np.abs(Y)[idx]) + 2.0 ** -149


def mse_tol(ref_pred, y, b):
    """bound on |mean((pred - y)^2) - mean((ref_pred - y)^2)| given |pred - ref_pred| <= b elementwise"""
    return float(np.mean(2.0 * np.abs(np.asarray(ref_pred, np.float64) - np.asarray(y, np.float64)) * b + b * b))
