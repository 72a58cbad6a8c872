"""The cases of the StandardScaler tests (CPU bounds test and GPU tests share them): rows and column blocks, with planted columns.

A part is (cols, dtype, ld, one_row): dtype "f32" / "bf16", ld None = cols, one_row = one row of values standing for every sample.
Planted into the first part where it has at least five columns (fp32 everywhere):
    column 0: mean 1e4, standard deviation 1e-2        (raw moments would lose every digit of the variance in fp32 and six in fp64)
    column 1: first row 1e6, the others near 0         (the kernel's shift, the first row, is the worst possible here)
    column 2: constant 0.1f;  column 3: constant 0     (sklearn's constant rule: scale 1)
bf16 parts hold multiples of 1/8 below 8 in magnitude: exactly representable, so the fp32 image the yardstick sees is what the kernel reads."""
from collections import namedtuple

import numpy as np

Part = namedtuple("Part", "cols dtype ld one_row")
Case = namedtuple("Case", "name rows parts")


def P(cols, dtype="f32", ld=None, one_row=False):
    return Part(cols, dtype, ld, one_row)


CASES = (
    Case("r1", 1, (P(5),)),
    Case("r2", 2, (P(1),)),
    Case("r65", 65, (P(7), P(5, "bf16"))),
    Case("r257", 257, (P(13), P(11, one_row=True))),
    Case("r1000", 1000, (P(782, ld=784), P(572, ld=576))),
    Case("r4099", 4099, (P(33, ld=40), P(3, "bf16", ld=8), P(1), P(2, "bf16", one_row=True))),
)
BY_NAME = {c.name: c for c in CASES}
SPLIT_CASE = "r4099"            # 4099 is prime: every forced split count above 1 leaves the last split short


def _seed(case):
    return 1000 + CASES.index(case)


def arrays(case):
    """list of fp32 arrays, (rows, cols) or (cols,) for a one-row part, in part order"""
    rng = np.random.default_rng(_seed(case))
    out = []
    for i, p in enumerate(case.parts):
        rows = 1 if p.one_row else case.rows
        if p.dtype == "bf16":
            a = rng.integers(-63, 64, size=(rows, p.cols)).astype(np.float32) / 8
        else:
            mu = rng.normal(0.0, 3.0, size=p.cols)
            sd = np.exp(rng.normal(0.0, 1.0, size=p.cols))
            a = (mu + sd * rng.normal(size=(rows, p.cols))).astype(np.float32)
            if i == 0 and p.cols >= 5 and not p.one_row:
                a[:, 0] = (1e4 + 1e-2 * rng.normal(size=rows)).astype(np.float32)
                a[:, 1] = (0.1 * rng.normal(size=rows)).astype(np.float32)
                a[0, 1] = 1e6
                a[:, 2] = np.float32(0.1)
                a[:, 3] = 0.0
        out.append(a[0] if p.one_row else a)
    return out


def full(case, arrs=None):
    """the assembled (rows, F) fp32 matrix"""
    arrs = arrays(case) if arrs is None else arrs
    return np.concatenate([np.broadcast_to(a, (case.rows, a.shape[-1])) for a in arrs], axis=1).astype(np.float32)


def tie_problem(per_scale=16):
    """(X fp32 (3, n), mean (n,), scale (n,)) for apply alone, on which a multiplication by the float64 reciprocal of scale is VISIBLE after
    the rounding to fp32 -- on ordinary data it is not: one float64 ulp moves an fp32 rounding once in 2^29 elements.  Here
    (x - mean) = s t exactly, t an odd 25-bit integer just below 2^25 (an exact tie between two fp32 values, half a float64 ulp relative
    2^-54) and s an odd integer whose reciprocal is rounded by nearly 2^-53: the division gives t and rounds to even, the product
    (s t) fl(1 / s) misses t by one float64 ulp and rounds to the other neighbour.  Found by search, asserted here."""
    xs, ms, ss = [], [], []
    t = np.arange(2 ** 25 - 2 ** 12 + 1, 2 ** 25, 2, dtype=np.float64)
    for s in (49.0, 75.0, 77.0, 91.0):
        y = s * t                                                    # exact: below 2^32
        k = np.nonzero((y / s).astype(np.float32) != (y * (1.0 / s)).astype(np.float32))[0][:per_scale]
        assert k.size == per_scale
        x = y[k].astype(np.float32)
        m = x.astype(np.float64) - y[k]                              # exact: both are integers below 2^32
        assert np.all(x.astype(np.float64) - m == y[k])
        xs.append(x), ms.append(m), ss.append(np.full(per_scale, s))
    X = np.tile(np.concatenate(xs), (3, 1)).astype(np.float32)
    return X, np.concatenate(ms), np.concatenate(ss)


def other_rows(case, rows):
    """`rows` further samples of the same columns (for transform with a fitted scaler): the case's values, rows permuted and perturbed"""
    rng = np.random.default_rng(_seed(case) + 500)
    out = []
    for a, p in zip(arrays(case), case.parts):
        if p.one_row:
            out.append(a)
        else:
            pick = a[rng.integers(0, case.rows, size=rows)]
            out.append(pick if p.dtype == "bf16" else (pick * np.float32(1.25)).astype(np.float32))
    return out
