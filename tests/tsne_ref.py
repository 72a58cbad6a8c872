"""float64 restatement of what mmvae.tsne computes (sklearn's TSNE(2, method="barnes_hut") at angle = 0), in numpy: the perplexity
search of _binary_search_perplexity, the symmetric CSR P of _joint_probabilities_nn, the gradient / Z / KL of _kl_divergence_bh with an
exact repulsion, one step of _gradient_descent, the whole fit, and trustworthiness.  tests/test_tsne_ref_cpu.py holds it to sklearn's
own records (tests/golden/tsne.npz)."""
import numpy as np

N_STEPS, TOL = 100, 1e-5            # sklearn's n_steps and PERPLEXITY_TOLERANCE
MACHINE_EPSILON = np.finfo(np.double).eps


# ---------------------------------------------------------------------------------------------------------------------------
# affinities
# ---------------------------------------------------------------------------------------------------------------------------
def entropy(d, beta):
    """(H, p) of one row (k,) or of rows (N, k) of squared distances at precision beta (scalar or (N,)): p_j = exp(-beta d_j) / sum,
    H = log(sum) + beta sum_j d_j p_j, evaluated on d - min(d) (neither depends on the shift)."""
    d = np.asarray(d, np.float64)
    x = d - d.min(axis=-1, keepdims=True)
    b = np.asarray(beta, np.float64)[..., None]
    e = np.exp(-x * b)
    s = e.sum(axis=-1, keepdims=True)
    p = e / s
    return np.log(s[..., 0]) + b[..., 0] * (x * p).sum(axis=-1), p


def binary_search(d, perplexity):
    """(p (N, k), beta (N,), converged (N,) bool): sklearn's search per row -- beta = 1, doubled while no upper bracket exists, halved while
    no lower one does, bisected otherwise, at most 100 evaluations, done at |H - log perplexity| <= 1e-5.  beta is the precision p was
    evaluated at."""
    d = np.asarray(d, np.float64)
    N, k = d.shape
    target = np.log(perplexity)
    P, B, ok = np.empty((N, k)), np.empty(N), np.zeros(N, bool)
    for i in range(N):
        beta, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(N_STEPS):
            H, p = entropy(d[i], beta)
            at = beta
            diff = H - target
            if abs(diff) <= TOL:
                ok[i] = True
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        P[i], B[i] = p, at
    return P, B, ok


def neighbours(X, k):
    """(idx (N, k), dist2 (N, k)) of every row's k nearest OTHER rows in float64, ascending by (distance, index)"""
    X = np.asarray(X, np.float64)
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(D, np.inf)
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(D, idx, axis=1)


def symmetric_csr(idx, p_cond):
    """(row_ptr (N + 1,), col (nnz,), val (nnz,)) of P = (P_cond + P_cond^T) / sum, columns ascending within a row"""
    idx = np.asarray(idx).astype(np.int64)
    N, k = idx.shape
    i = np.repeat(np.arange(N, dtype=np.int64), k)
    j = idx.ravel()
    v = np.asarray(p_cond, np.float64).ravel()
    keys = np.concatenate([i * N + j, j * N + i])
    uk, inv = np.unique(keys, return_inverse=True)
    val = np.bincount(inv, weights=np.concatenate([v, v]), minlength=len(uk))
    val = val / max(val.sum(), MACHINE_EPSILON)
    row_ptr = np.zeros(N + 1, np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(uk // N, minlength=N))
    return row_ptr, uk % N, val


def joint_probabilities(X, perplexity):
    """the CSR P of the rows X: int(3 perplexity + 1) neighbours (at most N - 1), search, symmetrisation"""
    X = np.asarray(X, np.float64)
    k = min(X.shape[0] - 1, int(3.0 * perplexity + 1))
    idx, d2 = neighbours(X, k)
    return symmetric_csr(idx, binary_search(d2, perplexity)[0])


def dense(row_ptr, col, val, N):
    P = np.zeros((N, N))
    rows = np.repeat(np.arange(N), np.diff(row_ptr))
    np.add.at(P, (rows, col), val)
    return P


# ---------------------------------------------------------------------------------------------------------------------------
# gradient
# ---------------------------------------------------------------------------------------------------------------------------
def gradient(Y, row_ptr, col, val, exaggeration=1.0):
    """dict(grad (N, 2), Z, kl, A (N, 2), R (N, 2), z (N,), err (N,)): w_ij = 1 / (1 + |y_i - y_j|^2), A_i = sum_j p_ij w_ij (y_i - y_j) over
    the stored entries, R_i = sum_{j != i} w_ij^2 (y_i - y_j), z_i = sum_{j != i} w_ij, Z = sum z, grad = 4 (exaggeration A - R / Z),
    err_i = sum_{j, p_ij > 0} p_ij log(p_ij / (w_ij / Z)), kl = sum err."""
    Y = np.asarray(Y, np.float64)
    N = Y.shape[0]
    val = np.asarray(val, np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    W = 1.0 / (1.0 + (diff ** 2).sum(axis=2))
    np.fill_diagonal(W, 0.0)
    z = W.sum(axis=1)
    Z = z.sum()
    R = ((W * W)[:, :, None] * diff).sum(axis=1)
    rows = np.repeat(np.arange(N), np.diff(row_ptr))
    d = Y[rows] - Y[col]
    q = 1.0 + (d ** 2).sum(axis=1)
    A = np.zeros((N, 2))
    np.add.at(A, rows, (val / q)[:, None] * d)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(val > 0, val * (np.log(np.where(val > 0, val, 1.0)) + np.log(q) + np.log(Z)), 0.0)
    err = np.bincount(rows, weights=terms, minlength=N)
    return dict(grad=4.0 * (exaggeration * A - R / Z), Z=Z, kl=err.sum(), A=A, R=R, z=z, err=err)


# ---------------------------------------------------------------------------------------------------------------------------
# update and fit
# ---------------------------------------------------------------------------------------------------------------------------
def update(y, upd, gains, grad, momentum, learning_rate):
    """one step of sklearn's _gradient_descent: (y, update, gains, |gains * grad|_2), nothing in place"""
    y, upd, gains, grad = (np.asarray(v, np.float64) for v in (y, upd, gains, grad))
    inc = upd * grad < 0.0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), 0.01)
    g = grad * gains
    upd = momentum * upd - learning_rate * g
    return y + upd, upd, gains, float(np.sqrt((g * g).sum()))


def fit(P, Y0, early_exaggeration=12.0, max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7, learning_rate=None):
    """sklearn's TSNE._tsne in float64 from the CSR P and the initial embedding: dict(Y, kl, n_iter, learning_rate, checks) -- 250
    iterations with P exaggerated at momentum 0.5, then momentum 0.8; error and gradient norm every 50 iterations and the two
    stopping rules."""
    row_ptr, col, val = P
    Y = np.array(Y0, np.float64)
    N = Y.shape[0]
    lr = max(N / early_exaggeration / 4, 50.0) if learning_rate is None else learning_rate
    checks = []

    def descend(Y, it, max_it, momentum, ex, patience):
        upd, gains = np.zeros_like(Y), np.ones_like(Y)
        error, best, best_it, i = None, np.finfo(float).max, it, it
        for i in range(it, max_it):
            check = (i + 1) % 50 == 0
            g = gradient(Y, row_ptr, col, val, ex)
            if check or i == max_it - 1:
                error = g["kl"] if ex == 1.0 else ex * (g["kl"] + np.log(ex))
            Y, upd, gains, gn = update(Y, upd, gains, g["grad"], momentum, lr)
            if check:
                checks.append((i + 1, error, gn, ex))
                if error < best:
                    best, best_it = error, i
                elif i - best_it > patience:
                    break
                if gn <= min_grad_norm:
                    break
        return Y, error, i

    Y, error, it = descend(Y, 0, 250, 0.5, early_exaggeration, 250)
    if it < 250 or max_iter - 250 > 0:
        Y, last, it = descend(Y, it + 1, max_iter, 0.8, 1.0, n_iter_without_progress)
        error = error if last is None else last
    return dict(Y=Y, kl=error, n_iter=it, learning_rate=lr, checks=checks)


def kl_of(P, Y):
    """the KL divergence of the embedding Y against the CSR P"""
    return gradient(Y, *P)["kl"]


def trustworthiness(X, Y, n_neighbors=5):
    """sklearn.manifold.trustworthiness(X, Y, n_neighbors=k), euclidean: 1 - 2 / (n k (2 n - 3 k - 1)) sum_i sum_{j in the k nearest of i
    in Y} max(0, rank of j among i's neighbours in X - k), ranks from 1 and without the row itself"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    n, k = X.shape[0], n_neighbors
    DX = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(DX, np.inf)
    order = np.argsort(DX, axis=1, kind="stable")
    rank = np.empty((n, n), np.int64)
    np.put_along_axis(rank, order, np.arange(1, n + 1)[None, :].repeat(n, axis=0), axis=1)
    idx_y = neighbours(Y, k)[0]
    t = np.maximum(np.take_along_axis(rank, idx_y, axis=1) - k, 0).sum()
    return 1.0 - t * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


# ---------------------------------------------------------------------------------------------------------------------------
# shared inputs
# ---------------------------------------------------------------------------------------------------------------------------
def blobs(n=600, f=10, classes=6, seed=0):
    """(X fp32 (n, f), labels (n,)): `classes` centres N(0, 4^2), noise N(0, 1)"""
    g = np.random.default_rng(seed)
    centres = 4.0 * g.standard_normal((classes, f))
    labels = np.arange(n) % classes
    return (centres[labels] + g.standard_normal((n, f))).astype(np.float32), labels


def silhouette(Y, labels):
    """mean silhouette coefficient of Y by class, float64"""
    Y = np.asarray(Y, np.float64)
    D = np.sqrt(((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2))
    cls = np.unique(labels)
    S = np.stack([D[:, labels == c].sum(axis=1) for c in cls], axis=1)
    n = np.array([(labels == c).sum() for c in cls])
    own = np.searchsorted(cls, labels)
    rows = np.arange(len(Y))
    a = S[rows, own] / np.maximum(n[own] - 1, 1)
    M = S / n[None, :]
    M[rows, own] = np.inf
    b = M.min(axis=1)
    return float(np.mean(np.where(n[own] > 1, (b - a) / np.maximum(a, b), 0.0)))
