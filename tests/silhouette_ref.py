"""float64 restatement of the silhouette coefficient (mmvae.clustering, include/mmvae_hip.h: mmvae_silhouette_samples) with direct
differences (no GEMM form): sklearn's silhouette_samples / silhouette_score (euclidean) and StandardScaler().fit_transform; the test
cases the CPU and the GPU tests share; and a float32 emulation of the kernel's arithmetic with switches for the mistakes a kernel
could make."""
import numpy as np

from knn_ref import to_bf16

TILE = 128            # query positions per workgroup and column positions per tile of the kernel


# ---------------------------------------------------------------------------------------------------------------------------
# float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------
def pair_dist(x):
    """euclidean distances (N, N) in float64: square root of the sum of squared differences; the diagonal is exactly 0"""
    x = np.asarray(x, np.float64)
    out = np.empty((x.shape[0], x.shape[0]))
    for i in range(x.shape[0]):
        d = x - x[i]
        out[i] = np.sqrt(np.einsum("jf,jf->j", d, d))
    return out


def s_of(a, b):
    """(b - a) / max(a, b), 0 where the maximum is 0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(m > 0, (b - a) / np.where(m > 0, m, 1.0), 0.0)


def parts(x, codes, C=None, D=None):
    """dict(S (N, C) class sums, n (C,) class sizes, a, b, s (N,)) for class codes in [0, C); classes without rows are skipped in b"""
    codes = np.asarray(codes).astype(np.int64)
    C = int(codes.max()) + 1 if C is None else C
    D = pair_dist(x) if D is None else D
    N = D.shape[0]
    n = np.bincount(codes, minlength=C)
    S = np.stack([D[:, codes == c].sum(axis=1) for c in range(C)], axis=1)
    rows = np.arange(N)
    own = n[codes]
    a = np.where(own > 1, S[rows, codes] / np.maximum(own - 1, 1), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(n[None, :] > 0, S / np.maximum(n, 1)[None, :], np.inf)
    mean[rows, codes] = np.inf
    b = mean.min(axis=1)
    s = np.where(own > 1, s_of(a, b), 0.0)
    return dict(S=S, n=n, a=a, b=b, s=s, D=D)


def silhouette_samples(x, labels):
    """sklearn.metrics.silhouette_samples(x, labels, metric='euclidean') in float64"""
    values, codes = np.unique(np.asarray(labels), return_inverse=True)
    if not 1 < len(values) < len(codes):
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % len(values))
    return parts(x, codes, len(values))["s"]


def silhouette_score(x, labels):
    return float(np.mean(silhouette_samples(x, labels)))


def standardize(x):
    """StandardScaler().fit_transform(x) in float64: population variance; a constant column (its variance is zero up to the rounding
    of its mean: sklearn's _is_constant_feature bound) keeps scale 1"""
    x = np.asarray(x, np.float64)
    mean, var = x.mean(axis=0), x.var(axis=0)
    n, eps = x.shape[0], np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    return (x - mean) / np.where(constant, 1.0, np.sqrt(var))


# ---------------------------------------------------------------------------------------------------------------------------
# cases: name -> dict(x float32 (bf16-representable where bf16 is set), codes (N,) class of every row, C, shift (float32 or None),
#                     bf16, grouped: the rows are already in class order and no `order` is passed)
# ---------------------------------------------------------------------------------------------------------------------------
def grouping(codes, C):
    """(order int32 (N,), class_start int32 (C + 1,)): the stable grouping of the rows by class"""
    codes = np.asarray(codes).astype(np.int64)
    order = np.argsort(codes, kind="stable").astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))]).astype(np.int32)
    return order, start


def column_means(x):
    return np.asarray(x, np.float64).mean(axis=0).astype(np.float32)


def _blobs(g, codes, F, C, sep=1.5):
    """class centres sep apart per coordinate scale, unit noise: overlapping clusters with silhouettes of both signs"""
    centres = sep * g.standard_normal((C, F))
    return (centres[codes] + g.standard_normal((len(codes), F))).astype(np.float32)


def _sizes_to_codes(g, sizes, shuffle=True):
    codes = np.repeat(np.arange(len(sizes)), sizes)
    return g.permutation(codes) if shuffle else codes


def make_case(name):
    if name in ("p77_f32", "p77_bf16", "grouped"):          # partial row block, partial tiles, F no multiple of 4
        g = np.random.default_rng(31)
        codes = _sizes_to_codes(g, [30, 19, 28])
        x = _blobs(g, codes, 45, 3, sep=0.4)
        if name == "p77_bf16":
            x = to_bf16(x)
        if name == "grouped":
            o = np.argsort(codes, kind="stable")
            x, codes = x[o], codes[o]
        return dict(x=x, codes=codes, C=3, shift=column_means(x), bf16=name == "p77_bf16", grouped=name == "grouped")
    if name == "c1000":                                     # a singleton, an exact tile, a tile + 1, several tiles; 8 row blocks
        g = np.random.default_rng(32)
        codes = _sizes_to_codes(g, [1, 128, 129, 300, 442])
        x = _blobs(g, codes, 33, 5, sep=0.5)
        return dict(x=x, codes=codes, C=5, shift=column_means(x), bf16=False, grouped=False)
    if name in ("pairs_shift", "pairs_noshift"):            # 60 classes of 2 rows, 100 + N(0, 1): a is ONE distance, a leaking diagonal halves it
        g = np.random.default_rng(33)
        codes = _sizes_to_codes(g, [2] * 60)
        x = (100.0 + g.standard_normal((120, 45))).astype(np.float32)
        return dict(x=x, codes=codes, C=60, shift=column_means(x) if name == "pairs_shift" else None, bf16=False, grouped=False)
    if name == "empty_class":                               # class 1 of 4 has no rows
        g = np.random.default_rng(34)
        codes = g.permutation(np.repeat([0, 2, 3], [30, 40, 20]))
        x = _blobs(g, codes, 20, 4, sep=0.5)
        return dict(x=x, codes=codes, C=4, shift=column_means(x), bf16=False, grouped=False)
    if name == "identical":                                 # every row equal: all d* = 0
        g = np.random.default_rng(35)
        x = np.tile((3.0 + g.standard_normal(29)).astype(np.float32), (70, 1))
        return dict(x=x, codes=_sizes_to_codes(g, [40, 30]), C=2, shift=None, bf16=False, grouped=False)
    if name == "near_dup":                                  # rows that differ in their last bits around 100, no shift: the GEMM form of
        g = np.random.default_rng(36)                       # d^2 is rounding noise of either sign and must be clamped before the root
        base = (100.0 + g.standard_normal(45)).astype(np.float32)
        x = (base[None, :] + 1e-5 * g.standard_normal((90, 45))).astype(np.float32)
        return dict(x=x, codes=_sizes_to_codes(g, [50, 40]), C=2, shift=None, bf16=False, grouped=False)
    if name == "cmax":                                      # C = 64 classes on 200 rows
        g = np.random.default_rng(37)
        sizes = np.full(64, 3)
        sizes[:8] += 1
        codes = _sizes_to_codes(g, sizes)
        x = _blobs(g, codes, 17, 64, sep=0.7)
        return dict(x=x, codes=codes, C=64, shift=column_means(x), bf16=False, grouped=False)
    if name == "n3":                                        # the smallest problem the public interface accepts: sizes 2 / 1
        g = np.random.default_rng(38)
        codes = np.array([1, 0, 0])
        return dict(x=_blobs(g, codes, 5, 2), codes=codes, C=2, shift=None, bf16=False, grouped=False)
    raise KeyError(name)


CASES = ("p77_f32", "p77_bf16", "grouped", "c1000", "pairs_shift", "pairs_noshift", "empty_class", "identical", "near_dup", "cmax", "n3")
SKLEARN_CASES = tuple(c for c in CASES if c != "identical")       # recorded in tests/golden/silhouette.npz


def tiles_of(class_start):
    """column tiles per class: a tile never crosses a class boundary"""
    n = np.diff(np.asarray(class_start).astype(np.int64))
    return (n + TILE - 1) // TILE


# ---------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernel's arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
MISTAKES = ("diag", "a_div_n", "own_in_b", "b_sum", "empty_in_min", "single_not_zero", "beyond_segment", "shift_one", "no_sqrt",
            "max_is_b", "drop_last_split", "no_clamp")


def emulate(x, codes, C, shift=None, nsplit=1, mistake=None):
    """(a, b, s) float32 (N,) in row order as the kernel computes them, up to the summation order of the float32 dot products and norms:
    GEMM form on the shifted values, clamp, square root, diagonal and segment masks, tile sums in the kernel's order (a lane's four
    columns, the butterfly over 16 lanes, the two column waves), tiles of a class in ascending order per split, splits in ascending
    order, then a, b, s.  mistake: None or one of MISTAKES."""
    f = np.float32
    x = np.asarray(x, f)
    N = x.shape[0]
    order, start = grouping(codes, C)
    c = np.zeros(x.shape[1], f) if shift is None else np.asarray(shift, f)
    xp = x[order]
    ts = xp - c
    qs = xp.copy() if mistake == "shift_one" else ts
    tn = np.einsum("jf,jf->j", ts, ts, dtype=f)
    qn = np.einsum("if,if->i", qs, qs, dtype=f)
    dot = (qs @ ts.T).astype(f)
    ntile = tiles_of(start)
    total = int(ntile.sum())
    nsplit = max(1, min(nsplit, total))
    tps = (total + nsplit - 1) // nsplit
    part = np.zeros((nsplit, N, C), f)
    lane = np.arange(16)
    pos = np.arange(N)
    t_global = 0
    with np.errstate(invalid="ignore"):
        for cl in range(C):
            lo, hi = int(start[cl]), int(start[cl + 1])
            for k in range(int(ntile[cl])):
                j0 = lo + TILE * k
                cols = j0 + np.arange(TILE)
                ok = cols < hi
                jj = np.where(ok, cols, 0)
                tnj = np.where(ok, tn[jj], f(0))
                dj = np.where(ok[None, :], dot[:, jj], f(0))
                d2 = ((qn[:, None] + tnj[None, :]).astype(f) - f(2) * dj).astype(f)
                if mistake != "no_clamp":
                    d2 = np.maximum(d2, f(0))
                d = d2 if mistake == "no_sqrt" else np.sqrt(d2).astype(f)
                if mistake != "diag":
                    d = np.where(pos[:, None] == cols[None, :], f(0), d)
                if mistake != "beyond_segment":
                    d = np.where(ok[None, :], d, f(0))
                d = d.reshape(N, 2, 4, 16)                                     # column = 64 wc + 16 ni + li
                v = ((d[:, :, 0] + d[:, :, 1]) + d[:, :, 2]) + d[:, :, 3]
                for o in (8, 4, 2, 1):
                    v = v + v[:, :, lane ^ o]
                tile_sum = v[:, 0, 0] + v[:, 1, 0]
                part[t_global // tps, :, cl] += tile_sum
                t_global += 1
    used = nsplit - 1 if mistake == "drop_last_split" and nsplit > 1 else nsplit
    S = part[0].copy()
    for s_ in range(1, used):
        S = S + part[s_]
    n = np.diff(start).astype(np.int64)
    a = np.zeros(N, f)
    b = np.full(N, np.inf, f)
    sv = np.zeros(N, f)
    pcode = np.asarray(codes)[order]
    with np.errstate(invalid="ignore", divide="ignore"):
        for cl in range(C):
            if n[cl] <= 0 and mistake != "empty_in_min":
                continue
            own = pcode == cl
            if n[cl] > 0:
                den = n[cl] if mistake == "a_div_n" else n[cl] - 1
                a = np.where(own, (S[:, cl] / f(den)).astype(f) if den > 0 else f(0), a)
            m = S[:, cl] if mistake == "b_sum" else (S[:, cl] / f(n[cl])).astype(f) if n[cl] > 0 else np.zeros(N, f)
            other = np.ones(N, bool) if mistake == "own_in_b" else ~own
            b = np.where(other & ~(m >= b), m, b).astype(f)
        mx = b if mistake == "max_is_b" else np.where(a > b, a, b)
        sv = np.where(mx > 0, ((b - a).astype(f) / mx).astype(f), f(0)).astype(f)
    if mistake != "single_not_zero":
        sv = np.where(n[pcode] > 1, sv, f(0))
    out = [np.empty(N, f) for _ in range(3)]
    for o, v in zip(out, (a, b, sv)):
        o[order] = v
    return tuple(out)
