"""float64 numpy restatement of what mmvae.pca.PCA computes -- sklearn.decomposition.PCA(n_components=k, svd_solver="full") as the
reference uses it (src/clustering_evaluation/cluster_imputation_methods.py:140-187) -- the test inputs with a planted spectrum, and a
float32 emulation of the kernels' arithmetic (with a list of mistakes the bounds of tests/pca_bounds.py must catch)."""
import numpy as np

CHUNK = 32          # rows per chunk of mmvae_pca_scatter (include/mmvae_hip.h)
TILE = 128
TARGET_WG = 512
MIN_CHUNKS = 8
MAX_SPLITS = 64


def column_means(x):
    """the shift mmvae.pca passes: the float64 column mean rounded to fp32"""
    return np.asarray(x, np.float64).mean(axis=0).astype(np.float32)


def scatter(x, c=None):
    """(x - c)^T (x - c) in float64; c = None: no centring"""
    xc = np.asarray(x, np.float64) - (0.0 if c is None else np.asarray(c, np.float64))
    return xc.T @ xc


def sign_fix(comp):
    """sklearn >= 1.5's svd_flip(u_based_decision=False): every row's entry of largest magnitude is positive"""
    comp = np.array(comp, np.float64)
    big = comp[np.arange(len(comp)), np.abs(comp).argmax(axis=1)]
    return comp * np.where(big < 0, -1.0, 1.0)[:, None]


def decompose(S, N, k):
    """the attributes of a fitted PCA from the F x F scatter matrix S of N rows"""
    lam, vec = np.linalg.eigh(np.asarray(S, np.float64))
    lam_all = np.maximum(lam, 0.0)[::-1]
    lam = lam_all[:k]
    return dict(lam_all=lam_all, components=sign_fix(vec[:, ::-1][:, :k].T), explained_variance=lam / (N - 1),
                explained_variance_ratio=lam / np.trace(S), singular_values=np.sqrt(lam))


def fit(x, k, mean=None):
    """mean: None = the exact float64 column mean (sklearn's), else the centre to use"""
    x = np.asarray(x, np.float64)
    m = x.mean(axis=0) if mean is None else np.asarray(mean, np.float64)
    S = scatter(x, m)
    out = decompose(S, x.shape[0], k)
    out.update(mean=m, S=S)
    return out


def transform(x, mean, components):
    return (np.asarray(x, np.float64) - np.asarray(mean, np.float64)) @ np.asarray(components, np.float64).T


def planted(N, F, lam_top, offset, seed, bf16=False):
    """float32 (N, F) with sample covariance W diag(lam) W^T before the rounding to fp32: lam = lam_top followed by ones, r = min(F,
    N - 1) of them non-zero; U: Q factor of a column-centred Gaussian N x r matrix, W: Q factor of a Gaussian F x F matrix"""
    g = np.random.default_rng(seed)
    r = min(F, N - 1)
    G = g.standard_normal((N, r))
    U = np.linalg.qr(G - G.mean(axis=0))[0]
    W = np.linalg.qr(g.standard_normal((F, F)))[0]
    lam = np.ones(r)
    lam[:len(lam_top)] = lam_top
    x = ((U * np.sqrt(lam * (N - 1))) @ W[:, :r].T + offset).astype(np.float32)
    if bf16:                                                 # values that bf16 holds exactly (round to nearest even on the upper 16 bits)
        b = x.view(np.uint32).astype(np.uint64)
        x = (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    return x


_CASES = {
    # name: (N, F, planted lambda, offset, seed, k, bf16)
    "n40": (40, 77, (40.0, 20.0, 10.0), 0.0, 11, 3, False),             # N < F
    "n300": (300, 77, (40.0, 20.0, 10.0), 100.0, 12, 3, False),
    "s77": (77, 37, (40.0, 20.0, 10.0), 100.0, 13, 3, False),           # one partial tile, a partial row chunk, odd width
    "s1000": (1000, 129, (400.0, 200.0, 100.0), 100.0, 14, 3, False),    # a tile plus one column; several splits
    "k50": (300, 200, tuple(np.arange(80.0, 30.0, -1.0)), 0.5, 15, 50, False),   # neighbouring gaps of 1: eigenvalues and span only
    "b77": (77, 37, (40.0, 20.0, 10.0), 2.0, 16, 2, True),              # values exact in bf16
}
CASES = tuple(_CASES)
COMPONENT_CASES = ("n40", "n300", "s77", "s1000", "b77")                 # k <= 3: per-component checks


def make_case(name):
    N, F, lam, offset, seed, k, bf16 = _CASES[name]
    x = planted(N, F, lam, offset, seed, bf16)
    return dict(name=name, x=x, k=k, bf16=bf16, offset=offset, shift=column_means(x), per_component=name in COMPONENT_CASES)


def splits_used(N, F, splits=0):
    """mmvae_pca_scatter_splits, restated from the header's formula"""
    T = (F + TILE - 1) // TILE
    P = T * (T + 1) // 2
    chunks = (N + CHUNK - 1) // CHUNK
    want = splits if splits > 0 else max(1, min(TARGET_WG // P, chunks // MIN_CHUNKS))
    want = min(want, MAX_SPLITS, chunks)
    cps = -(-chunks // want)
    return -(-chunks // cps), cps


# ---------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
SCATTER_MISTAKES = ("no_centring", "lower_unwritten", "lower_not_mirrored", "tail_rows_minus_shift", "tail_rows_dropped",
                    "partial_twice", "partial_skipped")
FIT_MISTAKES = ("n_for_n_minus_1", "ratio_over_top_k", "ascending", "sign_not_fixed", "uncentred_components")


def emulate_scatter(x, shift, splits=1, order="ascending", mistake=None):
    """S float32 (F, F) as mmvae_pca_scatter computes it up to the order of the sums inside a split: operands centred in fp32, products
    and sums in fp32 per split (order: 'ascending' / 'descending' rows one at a time, or 'blas': numpy's float32 matrix product), the
    splits' partial sums added in ascending order, the upper triangle mirrored."""
    f = np.float32
    x = np.asarray(x, f)
    N, F = x.shape
    c = np.zeros(F, f) if shift is None or mistake == "no_centring" else np.asarray(shift, f)
    xc = (x - c).astype(f)
    ns, cps = splits_used(N, F, splits)
    rows = N
    if mistake == "tail_rows_minus_shift":                   # the rows that pad the last chunk staged as 0 - shift
        xc = np.vstack([xc, np.tile(-c, (-N % CHUNK, 1))]).astype(f)
        rows = len(xc)
    if mistake == "tail_rows_dropped":                       # the partial last chunk left out
        rows = N // CHUNK * CHUNK
    parts = []
    for s in range(ns):
        blk = xc[s * cps * CHUNK:min((s + 1) * cps * CHUNK, rows)]
        if order == "blas":
            acc = (blk.T @ blk).astype(f)
        else:
            acc = np.zeros((F, F), f)
            for r in (blk if order == "ascending" else blk[::-1]):
                acc = acc + np.outer(r, r).astype(f)
        parts.append(acc)
    if mistake == "partial_twice" and ns > 1:
        parts.insert(1, parts[1])
    if mistake == "partial_skipped" and ns > 1:
        del parts[1]
    S = parts[0]
    for p in parts[1:]:
        S = (S + p).astype(f)
    up = np.triu(S)
    if mistake == "lower_unwritten":
        return up
    if mistake == "lower_not_mirrored":                      # the lower triangle summed in another order
        lo = emulate_scatter(x, shift, splits, "descending" if order != "descending" else "ascending")
        return up + np.tril(lo, -1)
    return up + np.triu(S, 1).T


def emulate_project(x, shift, v):
    f = np.float32
    xc = (np.asarray(x, f) - (f(0) if shift is None else np.asarray(shift, f))).astype(f)
    return (xc @ np.asarray(v, f).T).astype(f)


def emulate_fit(x, k, splits=0, order="ascending", mistake=None):
    """what mmvae.pca.PCA.fit computes from the emulated scatter matrix: float64 eigh, clamp, descending order, sign rule, the three
    variance vectors; components rounded to fp32.  mistake: None, one of SCATTER_MISTAKES or of FIT_MISTAKES."""
    x = np.asarray(x, np.float32)
    N = x.shape[0]
    c = column_means(x)
    S = emulate_scatter(x, c, splits, order, mistake if mistake in SCATTER_MISTAKES else None)
    lam, vec = np.linalg.eigh((emulate_scatter(x, None, splits, order) if mistake == "uncentred_components" else S).astype(np.float64))
    lam = np.maximum(lam, 0.0)
    if mistake != "ascending":
        lam, vec = lam[::-1], vec[:, ::-1]
    lam, comp = lam[:k], vec[:, :k].T
    if mistake != "sign_not_fixed":
        comp = sign_fix(comp)
    trace = lam.sum() if mistake == "ratio_over_top_k" else np.diag(S).astype(np.float64).sum()
    return dict(S=S, mean=c, components=comp.astype(np.float32), explained_variance=lam / (N if mistake == "n_for_n_minus_1" else N - 1),
                explained_variance_ratio=lam / trace, singular_values=np.sqrt(lam))
