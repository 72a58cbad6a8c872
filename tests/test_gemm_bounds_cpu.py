"""The derived bounds of tests/gemm_bounds.py on the CPU, both ways:

(a) THEY HOLD: a float32 numpy restatement of each operation stays inside its bound against float64, under adversarial summation
    orders -- strictly sequential fp32 accumulation, pairwise accumulation, split-then-reduce -- with the operand formed in fp32 and
    then rounded to bf16, at the shapes of tests/test_gemm_folded_gpu.py.  (The dW restatements keep the GPU cases' batch sizes
    and take a block of the output columns: the bound is per element, so a block shows what the whole matrix would.)
(b) THEY BITE: each deliberate mistake in the restatement puts at least one element outside the same bound.  Where a bound cannot
    see a mistake at some shape the docstring of that test records why and which shape is used instead; no bound is tightened by hand.

No GPU is needed.
"""
import numpy as np
import pytest

import np_oracle as O
import elementwise_bounds as E
import gemm_bounds as G

F32, F64 = np.float32, np.float64


def rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(F32)


def worst(got, ref, tol):
    """max err / bound over all elements (inf when an element with a zero bound is off)."""
    err = np.abs(np.asarray(got, F64) - np.asarray(ref, F64))
    tol = np.broadcast_to(np.asarray(tol, F64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / tol, 0.0)
    return float(r.max()) if r.size else 0.0


def holds(got, ref, tol, what):
    w = worst(got, ref, tol)
    assert w <= 1.0, f"{what}: float32 restatement outside the bound: err / bound {w:.3f}"


def bites(got, ref, tol, what):
    w = worst(got, ref, tol)
    assert w > 1.0, f"{what}: the mistake stays inside the bound (worst err / bound {w:.3f}): the bound cannot see it at this shape"


# ---------------------------------------------------------------------------------------------
# float32 sums of products in a chosen order.  a [R][T], b [C][T] -> [R][C] = sum_t a[r][t] b[c][t], started from `init`
# ---------------------------------------------------------------------------------------------
def dot_seq(a, b, init=None):
    acc = np.zeros((a.shape[0], b.shape[0]), F32) if init is None else np.broadcast_to(init, (a.shape[0], b.shape[0])).astype(F32)
    for t in range(a.shape[1]):
        acc = acc + a[:, t, None] * b[None, :, t]
    return acc


def dot_pair(a, b):
    T = a.shape[1]
    if T == 1:
        return a[:, 0, None] * b[None, :, 0]
    return dot_pair(a[:, :T // 2], b[:, :T // 2]) + dot_pair(a[:, T // 2:], b[:, T // 2:])


def dot_split(a, b, step, init=None):
    """chunks of `step` terms summed sequentially each, the partial sums then added in order (K steps / batch splits + slab reduce)."""
    parts = [dot_seq(a[:, t:t + step], b[:, t:t + step]) for t in range(0, a.shape[1], step)]
    s = parts[0]
    for p in parts[1:]:
        s = s + p
    return s if init is None else np.broadcast_to(init, s.shape).astype(F32) + s


ORDERS = ["sequential", "pairwise", "split"]


def nt32(a, w, bias, order, step=64):
    a, w = np.asarray(a, F32), np.asarray(w, F32)
    b = np.zeros(w.shape[0], F32) if bias is None else np.asarray(bias, F32)
    if order == "sequential":
        return dot_seq(a, w, b[None, :])
    if order == "pairwise":
        return dot_pair(a, w) + b[None, :]
    return dot_split(a, w, step) + b[None, :]


def dw32(p, q, old_dw, old_db, order, rps):
    """dW / db in float32: `sequential` adds every row onto the old value in turn, `pairwise` sums a tree and adds it, `split` sums
    splits of rps rows (a short last one) and reduces them in order onto the old value."""
    pt, qt = np.ascontiguousarray(np.asarray(p, F32).T), np.ascontiguousarray(np.asarray(q, F32).T)
    ones = np.ones((1, pt.shape[1]), F32)
    if order == "sequential":
        return dot_seq(pt, qt, old_dw), dot_seq(pt, ones, old_db[:, None])[:, 0]
    if order == "pairwise":
        return old_dw + dot_pair(pt, qt), old_db + dot_pair(pt, ones)[:, 0]
    return dot_split(pt, qt, rps, old_dw), dot_split(pt, ones, rps, old_db[:, None])[:, 0]


# ---------------------------------------------------------------------------------------------
# the operands as the kernels form them, in float32
# ---------------------------------------------------------------------------------------------
def prologue32(y, scale, shift, inv_keep, mask, bf16, scale_only=False):
    v = np.maximum(G.prologue_value(y, scale, shift, inv_keep, F32, scale_only), F32(0))
    assert v.dtype == F32
    if mask is not None:
        v = v * mask.astype(F32)
    return O.bf16_round(v) if bf16 else v


def fma32(a, b, c):
    """One fused multiply-add of float32 values: the exact product and sum formed in float64, rounded once."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def bn_bwd_p32(d, y, mean, rstd, sd, sdx, M, gamma, eval_mode, unzeroed=False):
    """gemm_src.h: BnBwdCols::column from the f64 sums (the four per-column constants) + bn_bwd_apply's two fused multiply-adds, rounded to bf16."""
    k0 = gamma * rstd
    k1 = np.zeros_like(k0) if eval_mode and not unzeroed else (np.asarray(sd, F64) / M).astype(F32)
    k2 = np.zeros_like(k0) if eval_mode else (np.asarray(sdx, F64) / M).astype(F32)
    c2, c1 = k0 * k2 * rstd, k0 * k1
    assert c2.dtype == F32 and c1.dtype == F32
    t = fma32(y - mean, c2, c1)
    return O.bf16_round(fma32(k0, d, -t.astype(F64)))


def pro_case(rng, M, K, bf16, masked):
    y = rnd(rng, M, K, scale=1.5)
    y = O.bf16_round(y) if bf16 else y
    scale, shift = (rng.uniform(0.5, 1.5, K)).astype(F32), rnd(rng, K, scale=0.3)
    mask = (rng.random((M, K)) < 0.9).astype(np.uint8) if masked else None
    return y, scale, shift, (1.0 / 0.9 if masked else 1.0), mask


NT_SHAPES = [(2, 40, 64), (389, 40, 128), (389, 256, 512), (4096, 40, 256), (130, 512, 256)]


# =============================================================================================
# (a) the bounds hold
# =============================================================================================
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_nt_bound_holds(M, N, K, bf16, order):
    rng = np.random.default_rng(M + N + K)
    y, scale, shift, ik, mask = pro_case(rng, M, K, bf16, masked=(N == 40))
    w = rnd(rng, N, K, scale=K ** -0.5)
    w = O.bf16_round(w) if bf16 else w
    bias = rnd(rng, N)
    h, dh = G.prologue_operand(y, scale, shift, ik, mask, bf16)
    if bf16:
        assert (dh > 0).mean() < 0.02 and ((dh > 0).any() or M * K < 10000)      # the at-risk set is small, and exists at any real size
    ref = G.nt_ref(h, w, bias)
    got = nt32(prologue32(y, scale, shift, ik, mask, bf16), w, bias, order)
    assert got.dtype == F32
    holds(got, ref, G.nt_tol(h, w, bias, dh), "NT")
    if bf16:
        holds(O.bf16_round(np.maximum(got, 0)), np.maximum(ref, 0), G.nt_tol(h, w, bias, dh, out_bf16=True, ref=np.maximum(ref, 0)), "NT, ReLU, bf16 out")
    # the column statistics of the stored values: fp32 partial sums over `rows` rows, then float64
    c = O.bf16_round(got) if bf16 else got
    for rows in (G.ROWS_TILE, G.ntp_rows(M, N)):
        s = np.zeros((2, N))
        for r0 in range(0, M, rows):
            blk = c[r0:r0 + rows]
            s1, s2 = np.zeros(N, F32), np.zeros(N, F32)
            for r in range(blk.shape[0]):
                s1, s2 = s1 + blk[r], s2 + blk[r] * blk[r]
            s += np.stack([s1, s2]).astype(F64)
        holds(s, G.stats_ref(c), G.stats_tol(c, rows), f"statistics over {rows} rows")


def test_ntp_rows_counts_the_tiles_of_a_persistent_workgroup():
    assert G.ntp_rows(4096, 256) == 128 and G.ntp_rows(32768, 256) == 128        # at most 256 tiles: one each
    assert G.ntp_rows(65536, 256) == 256 and G.ntp_rows(65536, 128) == 256       # 512 tiles on 256 workgroups
    assert G.ntp_rows(65536, 384) == 128 * 6                                     # 3 column tiles of 128: 1536 tiles


def test_q_bf16_is_round_to_nearest_even_without_a_float32_detour():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e-3, 0.0, 1000.0 + 1.0 / 3.0, 255.5, 2.0 ** -20])
    assert np.array_equal(G.q_bf16(x), O.bf16_round(x.astype(F32)).astype(F64))   # these are exact in float32
    assert G.q_bf16(1.00390625) == 1.0 and G.q_bf16(1.01171875) == 1.015625        # ties go to the even neighbour
    v = 1.00390625 + 2.0 ** -40                     # above the tie by less than float32 resolves: a float32 detour rounds down
    assert G.q_bf16(v) == 1.0078125 and O.bf16_round(np.array([v], F32))[0] == 1.0


DW_CASES = [  # M, N, K (a block of the GPU case's columns), rps, kind
    (8192, 48, 40, 1024, "bn"), (8192 + 96, 32, 46, 544, "bn"), (16384, 24, 36, 2048, "bn"),
    (130, 40, 128, 32, "pro"), (4096, 40, 256, 512, "pro"), (2, 24, 72, 32, "plain"), (4096, 64, 20, 128, "plain")]


def dw_case(rng, M, N, K, kind, eval_mode=False):
    """-> (the float64 operands p, q; allowances dp, dq; the float32 operands as the kernel forms them; extra)"""
    old_dw, old_db = rnd(rng, N, K), rnd(rng, N)
    if kind == "bn":
        d, y = O.bf16_round(rnd(rng, M, N) + rnd(rng, N, scale=0.5)), O.bf16_round(rnd(rng, M, N, scale=2.0) + F32(0.3))
        mean, rstd, gamma = rnd(rng, N, scale=0.2), rng.uniform(0.5, 1.5, N).astype(F32), rnd(rng, N) + 1.5
        xh = (y.astype(F64) - mean) * rstd
        sd, sdx = d.astype(F64).sum(0), (d * xh).sum(0)
        q = O.bf16_round(rnd(rng, M, K) + F32(0.5))                    # the fp32 input batch, rounded on load
        p, dp = G.bn_bwd_operand(d, y, mean, rstd, sd, sdx, M, gamma, eval_mode)
        extra = (d, y, mean, rstd, sd, sdx, gamma)
        return p, q, dp, None, bn_bwd_p32(d, y, mean, rstd, sd, sdx, M, gamma, eval_mode), q, old_dw, old_db, extra
    if kind == "pro":
        y, scale, shift, ik, mask = pro_case(rng, M, K, True, True)
        p = rnd(rng, M, N)                                             # fp32 P: rounded to bf16 on load
        q, dq = G.prologue_operand(y, scale, shift, ik, mask, True)
        return O.bf16_round(p), q, None, dq, O.bf16_round(p), prologue32(y, scale, shift, ik, mask, True), old_dw, old_db, None
    p, q = O.bf16_round(rnd(rng, M, N)), O.bf16_round(rnd(rng, M, K))
    return p, q, None, None, p, q, old_dw, old_db, None


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N,K,rps,kind", DW_CASES)
def test_dw_bound_holds(M, N, K, rps, kind, order):
    rng = np.random.default_rng(M + N + K)
    for eval_mode in ((False, True) if kind == "bn" else (False,)):
        p, q, dp, dq, p32, q32, old_dw, old_db, _ = dw_case(rng, M, N, K, kind, eval_mode)
        rw, rb = G.dw_ref(p, q, old_dw, old_db)
        tw, tb = G.dw_tol(p, q, old_dw, old_db, dp, dq)
        gw, gb = dw32(p32, q32, old_dw, old_db, order, rps)
        assert gw.dtype == F32 and gb.dtype == F32
        holds(gw, rw, tw, f"dW {kind} eval{int(eval_mode)}")
        holds(gb, rb, tb, f"db {kind} eval{int(eval_mode)}")
        # two orders of the same operands: inside the order-only bound of each other
        ow, ob = dw32(p32, q32, old_dw, old_db, "split" if order != "split" else "sequential", rps)
        ot = G.dw_order_tol(p32, q32, old_dw, old_db)
        holds(gw, ow, ot[0], "dW between two orders"); holds(gb, ob, ot[1], "db between two orders")


@pytest.mark.parametrize("M", [130, 4096])
def test_chained_statistics_bound_holds(M):
    """The hand-off of the forward: a GEMM's atomically accumulated statistics (fp32 partial sums over 128 rows) finalised, against a
    finalisation of the float64 sums of the data, inside E.bn_finalize_tol with sums_rel from the statistics bound."""
    rng = np.random.default_rng(M)
    N = 64
    c = O.bf16_round(rnd(rng, M, N, scale=1.3) + rnd(rng, N))
    c[:, 0] = O.bf16_round(F32(1000.0 + 1.0 / 3.0))
    s = np.zeros((2, N))
    for r0 in range(0, M, 128):
        blk = c[r0:r0 + 128]
        s1, s2 = np.zeros(N, F32), np.zeros(N, F32)
        for r in range(blk.shape[0]):
            s1, s2 = s1 + blk[r], s2 + blk[r] * blk[r]
        s += np.stack([s1, s2]).astype(F64)
    gamma, beta, rm, rv = rnd(rng, N) + 1.5, rnd(rng, N), rnd(rng, N), rng.uniform(0.5, 2, N).astype(F32)
    exact = G.stats_ref(c)
    ref = E.bn_finalize(exact[0], exact[1], M, gamma, beta, 1e-5, 0.1, rm, rv, F64)
    got = E.bn_finalize(s[0], s[1], M, gamma, beta, 1e-5, 0.1, rm, rv, F32)
    tol = E.bn_finalize_tol(exact[0], exact[1], M, gamma, beta, 1e-5, 0.1, rm, rv, sums_rel=G.sums_rel(c, 128))
    for k in tol:
        holds(got[k], ref[k], tol[k], "chained " + k)


# =============================================================================================
# (b) the bounds bite
# =============================================================================================
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_nt_bound_sees_a_dropped_last_k_chunk(M, N, K, bf16):
    rng = np.random.default_rng(M + N + K)
    y, scale, shift, ik, mask = pro_case(rng, M, K, bf16, masked=(N == 40))
    w = rnd(rng, N, K, scale=K ** -0.5)
    w = O.bf16_round(w) if bf16 else w
    bias = rnd(rng, N)
    h, dh = G.prologue_operand(y, scale, shift, ik, mask, bf16)
    a32 = prologue32(y, scale, shift, ik, mask, bf16)
    bites(nt32(a32[:, :K - 8], w[:, :K - 8], bias, "split"), G.nt_ref(h, w, bias), G.nt_tol(h, w, bias, dh), "last 8-element K chunk dropped")


@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_nt_bound_sees_inv_keep_on_the_scale_only(M, N, K):
    rng = np.random.default_rng(M + N + K)
    y, scale, shift, ik, mask = pro_case(rng, M, K, True, True)
    w, bias = O.bf16_round(rnd(rng, N, K, scale=K ** -0.5)), rnd(rng, N)
    h, dh = G.prologue_operand(y, scale, shift, ik, mask, True)
    wrong = prologue32(y, scale, shift, ik, mask, True, scale_only=True)
    bites(nt32(wrong, w, bias, "split"), G.nt_ref(h, w, bias), G.nt_tol(h, w, bias, dh), "inv_keep on the scale only")


@pytest.mark.parametrize("K", [64, 128, 256, 512])
def test_nt_bound_sees_one_ulp_in_a_row_of_small_magnitude(K):
    """One operand element that is NOT at risk moved by one bf16 ulp, in a row whose terms are 1000 times smaller than the other
    rows': a bound relative to the largest element of the matrix -- the form of every check in test_gemm_gpu.py -- passes this by a
    factor of about 1000, the per-element bound does not.  The moved element is the row's largest: at K = 512 a typical element's ulp
    (2^-8 of ONE term) is below (K + 1) U of the K terms' magnitudes, which is what the accumulation alone may cost."""
    rng = np.random.default_rng(K)
    M, N = 389, 40
    y, scale, shift, ik, mask = pro_case(rng, M, K, True, False)
    m = 77
    y[m] = O.bf16_round(y[m] * F32(1e-3)); shift = shift * F32(1e-3)     # every row keeps its formula; row m is small once shift is
    y[:m] = O.bf16_round(y[:m] + F32(2.0)); y[m + 1:] = O.bf16_round(y[m + 1:] + F32(2.0))
    w, bias = O.bf16_round(rnd(rng, N, K, scale=K ** -0.5)), np.zeros(N, F32)
    h, dh = G.prologue_operand(y, scale, shift, ik, mask, True)
    a32 = prologue32(y, scale, shift, ik, mask, True)
    ref, tol = G.nt_ref(h, w, bias), G.nt_tol(h, w, bias, dh)
    holds(nt32(a32, w, bias, "split"), ref, tol, "unperturbed")
    k = int(np.argmax(np.where(dh[m] == 0, np.abs(a32[m]), 0)))
    assert dh[m, k] == 0 and a32[m, k] != 0
    moved = a32.copy()
    moved[m, k] = F32(float(a32[m, k]) + 2.0 ** (np.frexp(float(a32[m, k]))[1] - 8))   # the next bf16 value away from zero (a > 0: ReLU)
    assert moved[m, k] != a32[m, k] and O.bf16_round(moved[m, k]) == moved[m, k]
    got = nt32(moved, w, bias, "split")
    bites(got, ref, tol, "one bf16 ulp in a small row")
    # ... which the max-scaled tolerance of test_gemm_gpu.py (2e-5 sqrt(K) max |ref|) passes a hundred times over
    assert np.abs(got[m].astype(F64) - ref[m]).max() <= 1e-2 * 2e-5 * np.sqrt(K) * np.abs(ref).max()


@pytest.mark.parametrize("M,N,K,rps,kind", [c for c in DW_CASES if c[0] < 16384])
def test_dw_bound_sees_a_dropped_last_row_of_a_short_split(M, N, K, rps, kind):
    """The last split is short (or the only one); its last row never enters the sum.  At M ~ 8192 the accumulation bound of a TYPICAL
    element, (M - 1) U sum |p q| ~ 4 mean |p q|, is above one typical term: the elements that see the mistake are those where the
    dropped row's own product is large, and every shape here has some; db is checked where M <= 4096.
    RECORDED: at M = 16 384 the bound cannot see ONE dropped row -- (M - 1) U of 16 384 terms is 16 mean terms, more than any
    product of two roughly normal values in the block (worst err / bound 0.75 on the 24 x 36 block) -- so that batch size is left
    to the shapes above; the bound is not tightened."""
    rng = np.random.default_rng(M + N + K)
    p, q, dp, dq, p32, q32, old_dw, old_db, _ = dw_case(rng, M, N, K, kind)
    rw, rb = G.dw_ref(p, q, old_dw, old_db)
    tw, tb = G.dw_tol(p, q, old_dw, old_db, dp, dq)
    gw, gb = dw32(p32[:-1], q32[:-1], old_dw, old_db, "split", rps)
    bites(gw, rw, tw, "dW, last row dropped")
    if M <= 4096:
        bites(gb, rb, tb, "db, last row dropped")


@pytest.mark.parametrize("M,N,K,rps,kind", [c for c in DW_CASES if c[4] == "bn"])
def test_dw_bound_sees_coef1_left_unzeroed_in_eval_mode(M, N, K, rps, kind):
    """Eval mode with c1 = sum_d / M instead of 0: every P element moves by c0 c1, about one bf16 ulp of a typical P.  db collects it
    M times over and is far outside; dW sees it because the fp32 input batch Q has a column mean (as real inputs do) -- against a
    centred Q the mistake would average out inside the accumulation bound, which is why the cases draw Q around 0.5."""
    rng = np.random.default_rng(M + N + K)
    p, q, dp, dq, p32, q32, old_dw, old_db, (d, y, mean, rstd, sd, sdx, gamma) = dw_case(rng, M, N, K, kind, eval_mode=True)
    assert np.allclose(p, G.q_bf16((gamma * rstd).astype(F64) * d), rtol=0, atol=0)        # eval mode: gamma rstd d exactly
    rw, rb = G.dw_ref(p, q, old_dw, old_db)
    tw, tb = G.dw_tol(p, q, old_dw, old_db, dp, dq)
    wrong = bn_bwd_p32(d, y, mean, rstd, sd, sdx, M, gamma, True, unzeroed=True)
    gw, gb = dw32(wrong, q32, old_dw, old_db, "split", rps)
    bites(gb, rb, tb, "db, coef[1] unzeroed"); bites(gw, rw, tw, "dW, coef[1] unzeroed")


@pytest.mark.parametrize("N", [128, 384, 512])
def test_accum_bound_sees_dgamma_added_once_per_k_tile(N):
    rng = np.random.default_rng(N)
    old, s = rnd(rng, N), rng.standard_normal(N) * 30
    once = E.accum(old, s, F32)
    holds(once, E.accum(old, s, F64), E.accum_tol(old, s), "dgamma")
    twice = once + s.astype(F32)                                            # two K tiles, each adding
    bites(twice, E.accum(old, s, F64), E.accum_tol(old, s), "dgamma added twice")


@pytest.mark.parametrize("M", [2, 389, 65536])
def test_finalize_bound_sees_the_running_statistics_updated_twice(M):
    rng = np.random.default_rng(M)
    N = 64
    x = rng.standard_normal((min(M, 4096), N)) * rng.uniform(0.1, 3.0, N) + rng.uniform(-2, 2, N)
    s1, s2 = x.sum(0) * (M / x.shape[0]), (x * x).sum(0) * (M / x.shape[0])
    gamma, beta, rm, rv = rnd(rng, N) + 1.5, rnd(rng, N), rnd(rng, N), rng.uniform(0.5, 2, N).astype(F32)
    args = (s1, s2, M, gamma, beta, 1e-5, 0.1)
    ref, tol = E.bn_finalize(*args, rm, rv, F64), E.bn_finalize_tol(*args, rm, rv)
    one = E.bn_finalize(*args, rm, rv, F32)
    two = E.bn_finalize(*args, one["running_mean"], one["running_var"], F32)             # a second workgroup (or tile) stepping again
    for k in ("running_mean", "running_var"):
        holds(one[k], ref[k], tol[k], k)
        bites(two[k], ref[k], tol[k], k + " stepped twice")


# =============================================================================================
# the statistics comparisons of tests/test_gemm_gpu.py that now use the derived bound
# =============================================================================================
NT_STORE = [(300, 128, 782, False), (257, 512, 572, False), (128, 40, 77, False), (1000, 600, 256, True), (64, 24, 64, True), (31, 130, 20, True)]


@pytest.mark.parametrize("bf16_mode", [False, True], ids=["fp32", "bf16"])
def test_derived_statistics_bound_is_below_the_tolerance_it_replaces_in_test_gemm_gpu(bf16_mode):
    """test_nt_store and test_nt_wide_tiles compared stat1 / stat2 with the sums of the stored values at rtol = 1e-4, atol = 1e-2.
    On their inputs (drawn here as they draw them) the derived bound of one 128-row tile is below that in every column, for every
    activation and output type, so those comparisons were replaced.  The comparisons of test_gemm_gpu.py that stay as they were
    hold the BatchNorm-backward sums against float64 values that were never stored (another reference), or two kernels against
    each other."""
    import torch
    r16 = lambda x: x.to(torch.bfloat16).to(torch.float32) if bf16_mode else x
    cases = [(M * 7 + N, M, N, K) for M, N, K, a_bf16 in NT_STORE if bf16_mode or not a_bf16]
    if bf16_mode:
        cases += [(N + K, 389, N, K) for N, K in ((256, 512), (512, 572), (512, 256))]              # test_nt_wide_tiles
    worst_ratio = 0.0
    for seed, M, N, K in cases:
        g = torch.Generator().manual_seed(seed)
        A = r16(torch.randn(M, K, generator=g))
        W = torch.randn(N, K, generator=g) / np.sqrt(K)
        b = torch.randn(N, generator=g)
        ref = A.double() @ r16(W).double().t() + b.double()
        for r in (ref, ref.clamp_min(0), torch.sigmoid(ref)):
            for stored in ([r.float().double()] + ([r.float().to(torch.bfloat16).double()] if bf16_mode else [])):
                c = stored.numpy()
                present = 1e-2 + 1e-4 * np.abs(G.stats_ref(c))
                worst_ratio = max(worst_ratio, float((G.stats_tol(c, G.ROWS_TILE) / present).max()))
    assert worst_ratio <= 1.0, worst_ratio


# =============================================================================================
# the epilogue rules of tests/gemm_bounds.py (sigmoid / accumulate, ReLU mask, BatchNorm backward, loss epilogues, f32-atomic dW,
# row blocks): float32 restatements hold under the three summation orders, deliberate mistakes fall outside.  The inputs come from
# tests/gemm_cases.py, the generators of the GPU tests, at GPU shapes.
# =============================================================================================
import gemm_cases as GC  # noqa: E402

EPI_SHAPES = [(31, 130, 20), (128, 40, 77), (389, 136, 256), (333, 200, 128)]


def nt_setup(M, N, K, bf16=True, w_scale=None):
    rng = np.random.default_rng(M + 3 * N + 7 * K)
    a, w, bias = GC.nt_case(rng, M, N, K, w_scale)
    if bf16:
        a, w = O.bf16_round(a), O.bf16_round(w)
    return rng, a, w, bias, G.nt_ref(a, w, bias), G.nt_tol(a, w, bias)


def sigmoid32(x):
    with np.errstate(over="ignore"):
        return F32(1) / (F32(1) + np.exp2(-np.asarray(x, F32) * F32(G.LOG2E32)))


def ln32(x):
    with np.errstate(divide="ignore"):
        return np.log2(np.asarray(x, F32)) * F32(0.6931471805599453)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N,K", EPI_SHAPES)
def test_sigmoid_and_accumulate_bounds_hold_and_see_the_activation_before_the_bias(M, N, K, order):
    rng, a, w, bias, ref, tol = nt_setup(M, N, K, w_scale=6.0 * K ** -0.5)           # saturated logits included
    assert np.abs(ref).max() > 17
    x32 = nt32(a, w, bias, order)
    p, tp = G.sigmoid(ref), G.sigmoid_tol(ref, tol)
    holds(sigmoid32(x32), p, tp, "sigmoid")
    holds(O.bf16_round(sigmoid32(x32)), p, G.bf16_out(tp, p), "sigmoid, bf16 out")
    old = rnd(rng, M, N)
    holds(old + x32, old.astype(F64) + ref, G.accumulate_tol(tol, ref, old), "C += acc + bias")
    wrong = sigmoid32(nt32(a, w, None, order)) + bias[None, :]
    bites(wrong, p, tp, "sigmoid applied before the bias")
    # tail-only columns and the small rows are held by their own terms: a dropped last K chunk is outside in exactly those columns
    drop = nt32(a[:, :K - 8], w[:, :K - 8], bias, order)
    for j in GC.nt_tail_rows(N, K):
        bites(drop[:, j], ref[:, j], tol[:, j], f"tail-only column {j}, last K chunk dropped")
    bites(sigmoid32(drop)[GC.small_rows(M)], p[GC.small_rows(M)], tp[GC.small_rows(M)], "small rows through the sigmoid, last K chunk dropped")


def epi_setup(M, N, K):
    rng, a, w, bias, ref, tol = nt_setup(M, N, K)
    e = GC.epi_case(rng, M, N)
    e["h"], e["y"] = O.bf16_round(e["h"]), O.bf16_round(e["y"])
    acc, tol = G.nt_ref(a, w, None), G.nt_tol(a, w, None)
    return rng, a, w, acc, tol, e


def bn_bwd32(acc32, e, masked, gate_y=False, no_inv_keep=False):
    """EpiBnBwd::compute in float32 -> (d, xhat)."""
    y = e["y"]
    keep = e["mask"].astype(F32) * (F32(1) if no_inv_keep else F32(1.0 / 0.9)) if masked else F32(1)
    gate = (y > 0) if gate_y else (y * e["scale"] + e["shift"] > 0)
    d = np.where(gate, acc32 * keep, F32(0)).astype(F32)
    return d, (y - e["mean"]) * e["rstd"]


def colsums32(v, rows=G.ROWS_TILE):
    """fp32 partial sums over `rows` rows, added in float64."""
    s = np.zeros(v.shape[1])
    for r0 in range(0, v.shape[0], rows):
        part = np.zeros(v.shape[1], F32)
        for r in range(r0, min(r0 + rows, v.shape[0])):
            part = part + v[r]
        s += part.astype(F64)
    return s


def shifted(x, by):
    """Rows read one row block early: row r holds what belongs to row r - by (the first block is read correctly)."""
    out = x.copy()
    out[by:] = x[:-by]
    return out


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N,K", EPI_SHAPES)
def test_relu_mask_bound_holds_and_bites(M, N, K, order):
    rng, a, w, acc, tol, e = epi_setup(M, N, K)
    acc32 = nt32(a, w, None, order)
    ref, t = G.relu_mask(acc, tol, e["h"])
    tb = G.bf16_out(t, ref)
    holds(O.bf16_round(np.where(e["h"] > 0, acc32, F32(0))), ref, tb, "ReLU mask")
    assert (e["h"] == 0).any() and (tb[e["h"] == 0] == 0).all()
    bites(O.bf16_round(np.where(e["h"] >= 0, acc32, F32(0))), ref, tb, "h >= 0 for h > 0")
    if M > 64:
        bites(O.bf16_round(np.where(shifted(e["h"], 32) > 0, acc32, F32(0))), ref, tb, "h read one row block early")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("M,N,K", EPI_SHAPES)
def test_bn_bwd_epilogue_bounds_hold_and_bite(M, N, K, masked, order):
    rng, a, w, acc, tol, e = epi_setup(M, N, K)
    acc32 = nt32(a, w, None, order)
    mask = e["mask"] if masked else None
    ik = 1.0 / 0.9 if masked else 1.0
    dref, dtol, share = G.bn_bwd_d(acc, tol, e["y"], e["scale"], e["shift"], mask, ik)
    assert share < 0.02                                                     # the at-risk cap of the GPU cases, same generator
    d32, xh32 = bn_bwd32(acc32, e, masked)
    holds(d32, dref, dtol, "d"); holds(O.bf16_round(d32), dref, G.bf16_out(dtol, dref), "d, bf16 out (phase 2)")
    sref, stol = G.bn_bwd_stats(dref, e["y"], e["mean"], e["rstd"]), G.bn_bwd_stats_tol(dref, dtol, e["y"], e["mean"], e["rstd"])
    holds(np.stack([colsums32(d32), colsums32(d32 * xh32)]), sref, stol, "sum d, sum d xhat")
    c = e["coef"]
    p1ref, p1tol = E.bn_bwd_apply(dref, e["y"], e["mean"], e["rstd"], c, F64), G.bn_bwd_phase1_tol(dref, dtol, e["y"], e["mean"], e["rstd"], c)
    holds(c[0] * (d32 - c[1] - xh32 * c[2]), p1ref, p1tol, "phase 1")
    holds(O.bf16_round(c[0] * (d32 - c[1] - xh32 * c[2])), p1ref, G.bf16_out(p1tol, p1ref), "phase 1, bf16 out")
    # the mistakes
    bites(bn_bwd32(acc32, e, masked, gate_y=True)[0], dref, dtol, "gate on y > 0")
    if masked:
        bites(bn_bwd32(acc32, e, masked, no_inv_keep=True)[0], dref, dtol, "keep without inv_keep")
        if M > 64:
            wrong = np.where(e["y"] * e["scale"] + e["shift"] > 0, acc32 * shifted(e["mask"], 32).astype(F32) * F32(1.0 / 0.9), F32(0))
            bites(wrong, dref, dtol, "mask read one row block early")
    bites(colsums32(d32 * e["y"]), sref[1], stol[1], "sum d y for sum d xhat")
    bites(c[0] * (d32 - xh32 * c[2]), p1ref, p1tol, "phase 1 without c1")


def test_bn_bwd_gate_marks_the_elements_within_its_own_rounding_of_zero():
    """y sc + sh exactly 0 in float64 and one float32 ulp to either side: at risk, allowance the whole |acc keep|; 1e-3 away: not."""
    sc, sh = np.array([1.5], F32), np.array([-0.75], F32)
    y = np.array([[0.5], [np.nextafter(F32(0.5), F32(1))], [np.nextafter(F32(0.5), F32(0))], [0.501], [0.499]], F32)
    gate, risk = G.bn_bwd_gate(y, sc, sh)
    assert risk[:3, 0].all() and not risk[3:, 0].any() and gate[3, 0] and not gate[4, 0]
    acc = np.full((5, 1), 3.0)
    d, tol, share = G.bn_bwd_d(acc, 1e-6, y, sc, sh, None, 1.0)
    assert (tol[:3] >= 3.0).all() and (tol[3] < 1e-5) and tol[4] == 0 and share == 0.6


LOSS_SHAPES = [(300, 333, 128), (389, 782, 128), (130, 572, 256)]


def loss32(x32, t, bce, clamp=True, wrt_p=False):
    """EpiLoss::term in float32 -> (gradient, terms)."""
    t = np.asarray(t, F32)
    if not bce:
        d = x32 - t
        return F32(2) * d, d * d
    pe = sigmoid32(x32)
    om = F32(1) - pe
    lp, l1p = ln32(pe), ln32(om)
    if clamp:
        lp, l1p = np.maximum(lp, F32(-100)), np.maximum(l1p, F32(-100))
    d = pe - t
    with np.errstate(invalid="ignore", over="ignore"):
        g = d / np.maximum(om * pe, F32(1e-12)) if wrt_p else d * np.minimum(om * pe * F32(1e12), F32(1))
        term = -(t * lp + (F32(1) - t) * l1p)
    return g, term


def loss_sum32(terms):
    """fp32 partial sums of G.LOSS_TERMS terms in sequence, added in float64."""
    v = terms.reshape(-1)
    s = 0.0
    for i in range(0, v.size, G.LOSS_TERMS):
        s += float(np.add.accumulate(v[i:i + G.LOSS_TERMS], dtype=F32)[-1])
    return s


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("bce", [False, True], ids=["mse", "bce"])
@pytest.mark.parametrize("M,N,K", LOSS_SHAPES)
def test_loss_epilogue_bounds_hold_and_bite(M, N, K, bce, order):
    rng, a, w, bias, ref, tol = nt_setup(M, N, K, w_scale=(8.0 if bce else 1.0) * K ** -0.5)
    t = GC.loss_case(rng, M, N, bce)
    if bce:      # logits saturate on both sides of both hard target values
        hard = ref[:M // 2]
        assert all(((hard * s > 17.5) & (t[:M // 2] == v)).any() for s in (1, -1) for v in (0, 1))
    gref, gtol, lref, ltol = (G.bce_epilogue if bce else G.mse_epilogue)(ref, tol, t)
    gtol = G.bf16_out(gtol, gref)
    x32 = nt32(a, w, bias, order)
    g32, l32 = loss32(x32, t, bce)
    holds(O.bf16_round(g32), gref, gtol, "gradient")
    holds(l32, lref, ltol, "terms")
    sref, stol = float(lref.sum()), G.loss_sum_tol(lref, ltol)
    assert abs(loss_sum32(l32) - sref) <= stol
    # the target read one row block early
    gw, lw = loss32(x32, shifted(t, 32), bce)
    bites(O.bf16_round(gw), gref, gtol, "target read one row block early (gradient)")
    # BCE: the sum cannot see this mistake at any shape.  Its bound carries, for every saturated logit, the distance of L1P (or LP) at
    # fl32(p +- tol_p) to the clamp -- tens per element -- while a row shift of targets that are independent of the logits changes
    # the sum only by the scatter of its terms; the gradient rows above carry the bite for BCE.
    if not bce:
        assert abs(loss_sum32(lw) - sref) > stol, "target read one row block early (MSE sum)"
    if bce:
        gw, lw = loss32(x32, t, True, clamp=False)
        bites(lw, lref, ltol, "log clamp missing")
        assert not abs(loss_sum32(lw) - sref) <= stol
        bites(O.bf16_round(loss32(x32, t, True, wrt_p=True)[0]), gref, gtol, "gradient with respect to p")
        # float64 mathematics is the wrong reference: a saturated wrong prediction costs 100, not |x|
        sat = (ref > 17.5) & (t == 0)
        assert (lref[sat] == 100).all() and (np.log1p(np.exp(ref[sat])) < 60).all()


DW_EDGE = [(130, 24, 64, None), (333, 128, 96, None), (1000, 40, 128, 352), (16384, 24, 36, 2048)]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N,K,rps", DW_EDGE)
def test_dw_atomics_bound_holds_and_the_tail_only_columns_see_a_dropped_row_at_any_batch_size(M, N, K, rps, order):
    """The f32-atomics form (no slab; row blocks): the old value is one of the terms.  The tail-only columns of tests/gemm_cases.py are
    zero outside the last 32-row step of the last split, so their bound counts 32 rows' terms at most: the dropped last row that
    test_dw_bound_sees_a_dropped_last_row_of_a_short_split records as invisible at M = 16 384 is outside here."""
    rng = np.random.default_rng(M + N + K)
    tail = GC.dw_tail(M, rps)
    p, q = (O.bf16_round(x) for x in GC.dw_case(rng, M, N, K, tail))
    old_dw, old_db = rnd(rng, N, K), rnd(rng, N)
    rw, rb = G.dw_ref(p, q, old_dw, old_db)
    tw, tb = G.dw_tol(p, q, old_dw, old_db, atomics=True)
    slab = G.dw_tol(p, q, old_dw, old_db)
    assert (tw >= slab[0]).all() and (tb >= slab[1]).all()
    gw, gb = dw32(p, q, old_dw, old_db, order, rps or 64)
    holds(gw, rw, tw, "dW, atomics"); holds(gb, rb, tb, "db")
    # row blocks: every block adds onto what the earlier ones left
    half = M // 2
    w1, b1 = dw32(p[:half], q[:half], old_dw, old_db, order, rps or 64)
    w2, b2 = dw32(p[half:], q[half:], w1, b1, order, rps or 64)
    holds(w2, rw, tw, "dW in two row blocks"); holds(b2, rb, tb, "db in two row blocks")
    # mistakes
    dw_, db_ = dw32(p[:-1], q[:-1], old_dw, old_db, order, rps or 64)
    for c in (1 % N, N - 1):
        bites(dw_[c], rw[c], tw[c], f"dW row {c} (tail-only P column), last row dropped")
    for c in (2 % K, K - 1):
        bites(dw_[:, c], rw[:, c], tw[:, c], f"dW column {c} (tail-only Q column), last row dropped")
    bites(db_[[1 % N, N - 1]], rb[[1 % N, N - 1]], tb[[1 % N, N - 1]], "db of the tail-only P columns, last row dropped")
    pad = gb.copy()
    pad[N - 1] += F32(7.0 * M)                                              # the 7.0 pad column of P summed into the last db element
    bites(pad, rb, tb, "db that includes a pad column")
    # P read one row block early in the second block
    w3, _ = dw32(shifted(p, 32)[half:], q[half:], w1, b1, order, rps or 64)
    bites(w3, rw, tw, "P read one row block early")


@pytest.mark.parametrize("M", [389, 1000])
def test_at_risk_cap_of_the_gpu_operand_prologues(M):
    """The at-risk share that tests/test_gemm_gpu.py asserts (< 2 %) on the inputs of its own generators: the BatchNorm + ReLU +
    Dropout prologue of the NT row-block case (dh) and the BatchNorm-corrected P of the dW row-block case (dp)."""
    K = 256
    rng = np.random.default_rng(M)
    y, _, _ = GC.nt_case(rng, M, 136, K)
    scale, shift = rng.uniform(0.5, 1.5, K).astype(F32), GC.rnd(rng, K, scale=0.3)
    mask = (rng.random((M, K)) < 0.9).astype(np.uint8)
    _, dh = G.prologue_operand(G.q_bf16(y), scale, shift, 1.0 / 0.9, mask, True)
    assert (dh > 0).mean() < 0.02
    Mw, N, Kw = 1000, 256, 150
    rng = np.random.default_rng(17)
    d, _ = GC.dw_case(rng, Mw, N, Kw)
    y = GC.rnd(rng, Mw, N, scale=2.0) + F32(0.3)
    mean, rstd = GC.rnd(rng, N, scale=0.2), rng.uniform(0.5, 1.5, N).astype(F32)
    coef = np.stack([rng.uniform(0.5, 1.5, N), rng.standard_normal(N) * 0.1, rng.standard_normal(N) * 0.1]).astype(F32)
    d, y = G.q_bf16(d), G.q_bf16(y)
    _, dp = G.operand_risk(E.bn_bwd_apply(d, y, mean, rstd, coef, np.float64), E.bn_bwd_apply_tol(d, y, mean, rstd, coef), True)
    assert (dp > 0).mean() < 0.02
