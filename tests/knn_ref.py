"""float64 restatement of the k-NN baselines (mmvae.knn, include/mmvae_hip.h: mmvae_knn_search / mmvae_knn_mean_rows): the search
under the (d^2, training index) order, sklearn's uniform KNeighborsRegressor, the reference's ConditionedKNeighborsRegressor
(src/models/conditioned_knn.py) and calculate_neighborhood_hit (src/clustering_evaluation/metrics_utils.py); the test cases the CPU
and the GPU tests share; and a float32 emulation of the kernel's arithmetic with switches for the mistakes a kernel could make."""
import numpy as np

TILE = 128            # query rows per workgroup and training rows per tile of the kernel


# ---------------------------------------------------------------------------------------------------------------------------
# float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------
def dist2(q, t):
    """exact-form squared distances (Mq, Nt) in float64: sum of squared differences, no GEMM form"""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    out = np.empty((q.shape[0], t.shape[0]))
    for i in range(q.shape[0]):
        d = t - q[i]
        out[i] = np.einsum("jf,jf->j", d, d)
    return out


def search(q, t, k):
    """(idx (Mq, k) int64, d2 (Mq, k) float64): the k smallest d^2 per query, ascending by (d^2, training index)"""
    d = dist2(q, t)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(d, idx, axis=1)


def mean_rows(idx, y):
    return np.asarray(y, np.float64)[np.asarray(idx)].mean(axis=1)


def knn_regress(X, Y, Xq, k=5):
    """KNeighborsRegressor(n_neighbors=k).fit(X, Y).predict(Xq), uniform weights, euclidean"""
    Y = np.asarray(Y, np.float64)
    Y = Y[:, None] if Y.ndim == 1 else Y
    return mean_rows(search(Xq, X, k)[0], Y)


def conditioned_regress(X, Y, site, Xq, site_q, k=5):
    """ConditionedKNeighborsRegressor(n_neighbors=k).fit([X | site], Y).predict([Xq | site_q]): one regressor per training site with
    min(k, rows of the site) neighbours; a query whose site was not trained keeps a zero row"""
    X, Xq = np.asarray(X, np.float64), np.asarray(Xq, np.float64)
    Y = np.asarray(Y, np.float64)
    Y = Y[:, None] if Y.ndim == 1 else Y
    site, site_q = np.asarray(site).astype(int), np.asarray(site_q).astype(int)
    out = np.zeros((Xq.shape[0], Y.shape[1]))
    for s in np.unique(site_q):
        m = site == s
        if not m.any():
            continue
        out[site_q == s] = knn_regress(X[m], Y[m], Xq[site_q == s], min(k, int(m.sum())))
    return out


def neighborhood_hit(features, labels, k=5):
    features, labels = np.asarray(features, np.float64), np.asarray(labels)
    if len(features) < k + 1:
        return 0.0
    idx = search(features, features, k + 1)[0][:, 1:]
    return float(np.mean(np.mean(labels[idx] == labels[:, None], axis=1)))


# ---------------------------------------------------------------------------------------------------------------------------
# storage
# ---------------------------------------------------------------------------------------------------------------------------
def to_bf16(x):
    """float32 values rounded to the nearest bf16 (ties to even), returned as float32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


# ---------------------------------------------------------------------------------------------------------------------------
# cases: name -> dict(q, t (float32; bf16-representable where bf16 is set), k, shift (float32 or None), bf16)
# ---------------------------------------------------------------------------------------------------------------------------
def _omics(g, rows, F):
    return np.abs(g.standard_normal((rows, F))).astype(np.float32)


def make_case(name):
    if name in ("p77_f32", "p77_bf16"):                     # partial query block, partial training tile, F no multiple of 4
        g = np.random.default_rng(1)
        q, t = _omics(g, 77, 45), _omics(g, 333, 45)
        if name.endswith("bf16"):
            q, t = to_bf16(q), to_bf16(t)
        return dict(q=q, t=t, k=5, shift=None, bf16=name.endswith("bf16"))
    if name.startswith("t1000_k"):                          # several tiles per row block
        g = np.random.default_rng(2)
        return dict(q=_omics(g, 200, 100), t=_omics(g, 1000, 100), k=int(name[7:]), shift=None, bf16=False)
    if name == "split":                                     # few query rows: the training rows are split across workgroups
        g = np.random.default_rng(3)
        return dict(q=g.random((3, 20), np.float32), t=g.random((5000, 20), np.float32), k=6, shift=None, bf16=False)
    if name == "nt_eq_k":
        g = np.random.default_rng(4)
        return dict(q=_omics(g, 10, 7), t=_omics(g, 5, 7), k=5, shift=None, bf16=False)
    if name == "nt1":
        g = np.random.default_rng(5)
        return dict(q=_omics(g, 4, 3), t=_omics(g, 1, 3), k=1, shift=None, bf16=False)
    if name == "mq1":
        g = np.random.default_rng(6)
        return dict(q=_omics(g, 1, 33), t=_omics(g, 300, 33), k=5, shift=None, bf16=False)
    if name in ("ill_shift", "ill_noshift"):                # 100 + N(0, 1): the GEMM form cancels 1e4 against 1e4 without the shift
        g = np.random.default_rng(7)
        q = (100.0 + g.standard_normal((77, 45))).astype(np.float32)
        t = (100.0 + g.standard_normal((333, 45))).astype(np.float32)
        shift = t.astype(np.float64).mean(axis=0).astype(np.float32) if name == "ill_shift" else None
        return dict(q=q, t=t, k=5, shift=shift, bf16=False)
    raise KeyError(name)


MATCH_CASES = ("p77_f32", "p77_bf16", "t1000_k1", "t1000_k5", "t1000_k50", "split", "nt_eq_k", "nt1", "mq1", "ill_shift")


def duplicates_case(Nt):
    """training rows 5 and 200 identical and query 0 equal to them (Nt 5000 with 3 queries: the two rows fall into different splits)"""
    g = np.random.default_rng(8)
    t = g.random((Nt, 20), np.float32)
    q = g.random((3, 20), np.float32)
    t[200] = t[5]
    q[0] = t[5]
    return q, t


# ---------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernel's arithmetic: key = |t - c|^2 - 2 (q - c).(t - c) in float32, selection by (key, index)
# ---------------------------------------------------------------------------------------------------------------------------
def emulate(q, t, k, shift=None, mistake=None, pad=None):
    """(idx (Mq, k) int64, dist2 (Mq, k) float32) as the kernel computes them, up to the summation order of float32.  mistake:
    None | 'drop_train_tail' | 'drop_query_tail' | 'tie_larger' | 'k_minus_1' | 'read_pads' | 'shift_one' | 'bf16_products'.
    pad: values of pad columns next to the data ('read_pads' multiplies them in)."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    Mq, Nt = q.shape[0], t.shape[0]
    if mistake == "read_pads":
        padq = np.full((Mq, 3), pad, np.float32)
        q, t = np.hstack([q, padq]), np.hstack([t, np.full((Nt, 3), pad, np.float32)])
        if shift is not None:
            shift = np.concatenate([shift, np.zeros(3, np.float32)])
    c = np.zeros(q.shape[1], np.float32) if shift is None else np.asarray(shift, np.float32)
    qs = q - c if mistake != "shift_one" else q.copy()
    ts = t - c
    if mistake == "bf16_products":
        qs, ts = to_bf16(qs), to_bf16(ts)
    tn = np.einsum("jf,jf->j", ts, ts, dtype=np.float32)
    qn = np.einsum("if,if->i", qs, qs, dtype=np.float32)
    key = (tn[None, :] - np.float32(2) * (qs @ ts.T)).astype(np.float32)
    key = np.where(np.isnan(key), np.float32(np.inf), key) + np.float32(0)
    nt_used = Nt
    if mistake == "drop_train_tail" and Nt % TILE and Nt > TILE:
        nt_used = Nt - Nt % TILE
    keep = k - 1 if mistake == "k_minus_1" and k > 1 else k
    if mistake == "tie_larger":
        order = (nt_used - 1 - np.argsort(key[:, :nt_used][:, ::-1], axis=1, kind="stable"))[:, :keep]
    else:
        order = np.argsort(key[:, :nt_used], axis=1, kind="stable")[:, :keep]
    idx = np.full((Mq, k), -1, np.int64)
    idx[:, :keep] = order
    if keep < k:
        idx[:, keep:] = order[:, -1:]
    d2 = np.maximum(np.take_along_axis(key, np.maximum(idx, 0), axis=1) + qn[:, None], np.float32(0)).astype(np.float32)
    if mistake == "drop_query_tail" and Mq % TILE:
        idx[Mq - Mq % TILE:] = -1
    return idx, d2


def mean_rows_f32(idx, y):
    """the fp32 rows mmvae_knn_mean_rows writes for these indices: fp32 sums in ascending neighbour order, one fp32 division"""
    y, idx = np.asarray(y, np.float32), np.asarray(idx)
    s = np.zeros((idx.shape[0], y.shape[1]), np.float32)
    for n in range(idx.shape[1]):
        s = s + y[idx[:, n]]
    return s / np.float32(idx.shape[1])
