"""The StandardScaler yardsticks tested on themselves, without a GPU: a numpy emulation of the arithmetic of standardize.hip (memory
images of the parts, the first-row shift, float64 sums per wave and split in the header's order) stays inside tests/standardize_bounds.py
on every case in three summation orders and several split counts; eleven plausible mistakes of such a kernel leave them; the restatement
equals sklearn's StandardScaler."""
import numpy as np
import pytest

import standardize_bounds as B
import standardize_cases as SC
import standardize_ref as R

PAD = np.float32(777.0)
ORDERS = ("kernel", "reverse", "pairwise")


# ---- memory images: what the kernel is handed ----------------------------------------------------------------------------------
def memories(case, arrs):
    """per part: (flat element array, stride in elements): fp32 as float32, bf16 as its uint16 bit patterns; pad columns hold PAD"""
    out = []
    for a, p in zip(arrs, case.parts):
        if p.one_row:
            img, stride = a.copy(), 0
        else:
            ld = p.ld or p.cols
            img = np.full((case.rows, ld), PAD, dtype=np.float32)
            img[:, :p.cols] = a
            img, stride = img.reshape(-1), ld
        if p.dtype == "bf16":
            bits = (img.view(np.uint32) >> 16).astype(np.uint16)          # PAD is not representable: its pad image is simply another value
            img = bits
        out.append((img, stride))
    return out


def read(case, mems, mistake=None):
    """the (rows, F) float64 matrix a kernel with this addressing sees"""
    cols, rows = [], np.arange(case.rows)[:, None]
    for i, ((img, stride), p) in enumerate(zip(mems, case.parts)):
        c = np.arange(p.cols)[None, :]
        if mistake == "offset" and i >= 1:
            c = c + case.parts[i - 1].cols                                # local column from the previous part's first column
        if mistake == "one_row_stride" and p.one_row:
            stride = p.cols                                               # rows 1 .. are whatever lies behind the one row
            img = np.concatenate([img, np.full(p.cols * (case.rows - 1), 16000 if p.dtype == "bf16" else PAD, dtype=img.dtype)])
        if p.dtype == "bf16" and mistake == "bf16_halves":
            f = img[:img.size // 2 * 2].view(np.float32)
            v = f[(rows * stride + c) % f.size]
        else:
            e = img[(rows * stride + c) % img.size]
            v = (e.astype(np.uint32) << 16).view(np.float32) if p.dtype == "bf16" else e
        cols.append(np.broadcast_to(v, (case.rows, p.cols)).astype(np.float64))
    return np.concatenate(cols, axis=1)


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def seq_sum(A, dtype):
    s = np.zeros(A.shape[1], dtype)
    for row in A:
        s = (s + row).astype(dtype)
    return s


def emu_fit(X, used, rps, order="kernel", mistake=None):
    n = X.shape[0]
    acc = np.float32 if mistake == "fp32_acc" else np.float64
    c = np.zeros(X.shape[1]) if mistake == "no_shift_fp32_products" else X[0]
    S0, S1 = np.zeros(X.shape[1], acc), np.zeros(X.shape[1], acc)
    nsp = used - 1 if (mistake == "drop_last" and used > 1) else used
    for s in range(nsp):
        a = (X[s * rps:min((s + 1) * rps, n)] - c).astype(acc)
        sq = (a.astype(np.float32) * a.astype(np.float32)).astype(acc) if mistake == "no_shift_fp32_products" else (a * a).astype(acc)
        if order == "pairwise":
            t0, t1 = a.sum(axis=0, dtype=acc), sq.sum(axis=0, dtype=acc)
        else:
            t0, t1 = np.zeros(X.shape[1], acc), np.zeros(X.shape[1], acc)
            for w in range(4):
                aw, qw = a[w::4], sq[w::4]
                if order == "reverse":
                    aw, qw = aw[::-1], qw[::-1]
                t0, t1 = (t0 + seq_sum(aw, acc)).astype(acc), (t1 + seq_sum(qw, acc)).astype(acc)
        S0, S1 = (S0 + t0).astype(acc), (S1 + t1).astype(acc)
    S0, S1 = S0.astype(np.float64), S1.astype(np.float64)
    d = S0 / n
    mean = c + d
    var = np.maximum((S1 - n * d * d) / (n - 1) if (mistake == "unbiased" and n > 1) else S1 / n - d * d, 0.0)
    constant = var <= R.constant_threshold(n, mean, var)
    if mistake == "no_constant_rule":
        constant = np.zeros_like(constant)
    with np.errstate(invalid="ignore"):
        scale = np.where(constant, 1.0, var if mistake == "scale_is_var" else np.sqrt(var))
    return mean, var, scale


def emu_apply(X32, mean, scale, ldz, mistake=None):
    """the z buffer (rows, ldz) pre-filled with NaN"""
    rows, F = X32.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        z = ((X32.astype(np.float64) - mean) * (1.0 / scale) if mistake == "reciprocal" else (X32.astype(np.float64) - mean) / scale).astype(np.float32)
    buf = np.full(rows * ldz, np.nan, np.float32)
    ld = F if mistake == "ldz_is_F" else ldz
    buf[(np.arange(rows)[:, None] * ld + np.arange(F)[None, :]).reshape(-1)] = z.reshape(-1)
    return buf.reshape(rows, ldz)


def inside(got, want, tol):
    return bool(np.all(np.abs(got - want) <= tol))           # a NaN is outside


def verdict(case, splits, order="kernel", mistake=None):
    """does the emulation, with this mistake, pass everything tests/test_standardize_gpu.py asserts?"""
    arrs = SC.arrays(case)
    X32 = SC.full(case, arrs)
    F = X32.shape[1]
    used, rps = R.splits_used(case.rows, F, splits)
    mean_r, var_r, scale_r = R.fit(X32)
    mt, vt, st = B.fit_tol(X32, used)
    Xk = read(case, memories(case, arrs), mistake)
    mean, var, scale = emu_fit(Xk, used, rps, order, mistake)
    ok = inside(mean, mean_r, mt) and inside(var, var_r, vt) and inside(scale, scale_r, st)
    # apply with the yardstick's mean / scale: bit-equal, guard columns untouched
    zb = emu_apply(Xk.astype(np.float32), mean_r, scale_r, F + 3, mistake)
    ok = ok and np.array_equal(zb[:, :F].view(np.int32), R.apply(X32, mean_r, scale_r).view(np.int32)) and bool(np.isnan(zb[:, F:]).all())
    # apply after the emulated fit
    z64 = R.apply64(X32, mean_r, scale_r)
    with np.errstate(all="ignore"):
        zd = ((Xk - mean) / scale).astype(np.float32)
        ok = ok and inside(zd.astype(np.float64), z64, B.z_tol(z64, scale_r, mt, st))
    return ok


# ---- tests -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_cases_stay_out_of_the_constant_rules_fuzzy_zone(case):
    X = SC.full(case)
    mean, var, scale = R.fit(X)
    exact = np.ptp(X, axis=0) == 0
    thr = R.constant_threshold(case.rows, mean, var)
    assert np.all(exact | (var >= 1e6 * thr)), "a column is neither exactly constant nor far above sklearn's constant threshold"
    assert np.all(var[exact] == 0) and np.all(scale[exact] == 1.0) and np.all(scale[~exact] == np.sqrt(var[~exact]))
    for splits in (1, 64):
        _, vt, st = B.fit_tol(X, splits)
        assert np.all(vt[~exact] < 1e-6 * var[~exact]) and np.all(vt[exact] == 0) and np.all(st[exact] == 0)
    if case.name == "r1":
        assert exact.all()
    # the planted columns are where the docstring says
    if case.parts[0].cols >= 5 and case.rows >= 65:
        assert abs(mean[0] - 1e4) < 1 and 1e-5 < var[0] < 1e-3 and X[0, 1] == 1e6 and np.abs(X[1:, 1]).max() < 1 and exact[2] and exact[3]
        assert mean[2] == np.float64(np.float32(0.1)) and mean[3] == 0


def test_bf16_parts_are_exactly_representable():
    for case in SC.CASES:
        for a, p in zip(SC.arrays(case), case.parts):
            if p.dtype == "bf16":
                assert np.all((a.view(np.uint32) & 0xFFFF) == 0)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_the_kernels_arithmetic_stays_inside_the_bounds(case, order):
    for splits in (0, 1, 3, 64):
        assert verdict(case, splits, order), (case.name, order, splits)


MISTAKES = {
    "unbiased": "r4099", "scale_is_var": "r4099", "no_constant_rule": "r4099", "fp32_acc": "r4099", "no_shift_fp32_products": "r4099",
    "offset": "r4099", "one_row_stride": "r257", "drop_last": "r4099", "bf16_halves": "r65", "reciprocal": "r4099", "ldz_is_F": "r65",
}


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_each_mistake_leaves_the_bounds(mistake):
    case = SC.BY_NAME[MISTAKES[mistake]]
    assert verdict(case, 3, "kernel")
    if mistake == "reciprocal":         # visible on the tie problem alone: test_reciprocal_multiply_breaks_only_the_bit_equality
        assert verdict(case, 3, "kernel", mistake)
    else:
        assert not verdict(case, 3, "kernel", mistake)


def test_reciprocal_multiply_breaks_only_the_bit_equality():
    """on the cases a float64 reciprocal is invisible after the rounding to fp32; the tie problem (standardize_cases.tie_problem) shows it"""
    X, mean, scale = SC.tie_problem()
    F = X.shape[1]
    want = R.apply(X, mean, scale)
    good, bad = emu_apply(X, mean, scale, F + 3), emu_apply(X, mean, scale, F + 3, "reciprocal")
    assert np.array_equal(good[:, :F].view(np.int32), want.view(np.int32))
    assert not np.array_equal(bad[:, :F].view(np.int32), want.view(np.int32))
    z64 = R.apply64(X, mean, scale)
    assert inside(bad[:, :F].astype(np.float64), z64, B.z_tol(z64, scale, 0 * mean, 0 * scale))           # still within the z bound


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_the_restatement_is_sklearns_standard_scaler(case):
    """sklearn accumulates float32 data in float64 (pairwise np.sum over x, then over (x - mean)^2): its mean carries up to
    16 + log2(n) roundings of sum |x| / n, its variance the same of mean (x - mean)^2 plus the mean's error squared.  Its transform
    works IN PLACE on the float32 copy -- X -= mean_; X /= scale_ -- which is TWO roundings to fp32 where the restatement (and the kernel)
    has one: the difference is at most half an fp32 ulp of (x - mean), divided by scale, on top of half an fp32 ulp of z."""
    sk = pytest.importorskip("sklearn.preprocessing")
    X = SC.full(case)
    n = case.rows
    mean, var, scale = R.fit(X)
    s = sk.StandardScaler().fit(X.copy())
    k = 16 + int(np.ceil(np.log2(n))) + 3
    X64 = X.astype(np.float64)
    mt = B.gamma(k) * np.abs(X64).mean(axis=0) + 2 * B.U * np.abs(mean)
    dev2 = ((X64 - mean) ** 2).mean(axis=0)
    vt = B.gamma(k + 3) * dev2 + 2 * mt * np.abs(X64 - mean).mean(axis=0) + mt * mt + 2 * B.U * var
    assert s.mean_.dtype == np.float64 and inside(s.mean_, mean, mt) and inside(s.var_, var, vt)
    exact = np.ptp(X, axis=0) == 0
    assert np.all(s.scale_[exact] == 1.0) and inside(s.scale_[~exact], scale[~exact], vt[~exact] / scale[~exact] + 4 * B.U * scale[~exact])
    z_sk = s.transform(X.copy())
    assert z_sk.dtype == np.float32
    z64 = R.apply64(X, mean, scale)
    diff = X64 - mean
    st = np.where(exact, 0.0, vt / scale + 4 * B.U * scale)
    tol = (0.5 * np.spacing(np.abs(diff).astype(np.float32)).astype(np.float64) + mt) / (scale - st) + B.z_tol(z64, scale, mt, st)
    assert inside(z_sk.astype(np.float64), z64, tol)
    assert s.n_samples_seen_ == n
