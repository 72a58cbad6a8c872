"""DERIVED per-element error bounds of the GEMM kernels (csrc/gemm_nt.hip, gemm_nt2.h, gemm_ntp.h, gemm_nt_epi.h, gemm_tn.hip,
gemm_tn_wide.hip), shared by tests/test_gemm_gpu.py, tests/test_gemm_folded_gpu.py and the loss-epilogue test of
tests/test_loss_gpu.py (device against float64) and tests/test_gemm_bounds_cpu.py (a float32 numpy restatement must stay
inside every bound, and a set of deliberate mistakes must fall outside).  The model of one float32 operation and the constants are
those of tests/elementwise_bounds.py; nothing below was fitted to what a kernel returns.  Every bound is PER ELEMENT and relative
to the magnitude of that element's own terms (sum of absolute values), never to the largest element of the matrix: one wrong
element of small magnitude -- a tail column, a row of a short last split -- is outside it.

Rules

  NT output element      C[m][j] = sum_k a[m][k] w[j][k] + bias[j]: K products accumulated in fp32 in ANY order (MFMA K steps,
                         fragment order) plus the bias.  A bf16 x bf16 product is exact in fp32; the fp32 MFMA is an fma chain with
                         one rounding per term.  Either way  (K + 1) U (sum_k |a_k| |w_k| + |bias|) SECOND   (nt_tol).  A bf16
                         output goes through bf16_out; ReLU is exact (monotone, and it keeps 0).
  dW element             dW[n][k] = old + sum_m p[m][n] q[m][k]: M terms summed in any order (batch splits, slab reduce, atomics):
                         (M - 1) U sum_m |p_m| |q_m|, plus ONE rounding for the add of the sum onto the old value,
                         U (|old| + sum |p q|)   (dw_tol).  That is the slab form (tn_reduce_kernel sums the splits' partial tiles
                         and adds the sum onto dW once).  Without a slab every split adds its partial tile onto dW with f32 atomics
                         (gemm_tn.hip, tn_body: "f32 atomics straight into dW"): the old value is one of M + 1 terms summed in any
                         order,  M U (|old| + sum |p q|)   (dw_tol(atomics=True)); it is never below the slab form.  db[n] = old + sum_m p[m][n] likewise over |p_m|, except that the kernels add every split's
                         column sum onto db with f32 atomics: the old value is one of M + 1 terms summed in any order,
                         M U (|old| + sum |p|)   (db_tol).
  row blocks             (for_row_blocks in common.h: mmvae_gemm_nt / mmvae_gemm_tn re-enter themselves for consecutive blocks of rows.)
                         NT outputs: rows are independent, every element is computed by exactly one block with the same K terms:
                         nothing changes.  Column statistics: every block's workgroups add their fp32 partial sums (still at most
                         ROWS_TILE rows each) with f64 atomics: stats_tol / bn_bwd_stats_tol as they are.  The loss sum likewise.
                         dW / db: every block adds onto what the previous blocks left, through atomics or through the reduce's
                         `+=`: the old value and the earlier blocks' sums are terms of ONE sum of M + 1 terms in some order,
                         which is exactly the atomics form above: dw_tol(atomics=True) and db_tol, with the M of the whole call.
  operands formed in the kernel, then rounded to the compute type
                         (the BatchNorm + ReLU + Dropout prologue, the BatchNorm-backward correction.)  The reference forms the
                         value in float64 and rounds it; the kernel forms it in fp32 with the roundings its expression counts, so
                         its value v' lies within tol_v of the float64 value v.  Rounding to bf16 (q) and ReLU are monotone, hence
                         both q(relu(v')) and q(relu(v)) lie in  [q(relu(v - tol_v)), q(relu(v + tol_v))]:  the two differ by at
                         most the width `dh` of that interval, which is 0 unless v lies within tol_v of a rounding boundary (then one
                         ulp of the compute type) or of the ReLU's boundary 0 (then the whole value).  operand_risk() returns dh
                         for every element, computed on the CPU; the AT-RISK SET is dh > 0.  An at-risk operand element (m, k)
                         adds dh[m][k] |w[j][k]| to the bound of the outputs it feeds: the allowance is dh |W|^T (NT),
                         dh^T |Q| or |P|^T dh (dW), the column sums of dh (db).  No element is excluded anywhere.
                         In fp32 mode the operand is not rounded and keeps its fp32 error: dh = tol_v for every element.
  prologue value         v = y (sc ik) + sh ik with sc ik and sh ik rounded once per workgroup (gemm_src.h SrcBnReluDrop::init),
                         then one fused multiply-add (or a product and a sum): the scaled term carries U (sc ik) + U (product) + U
                         (sum), the shift term U + U:  tol_v = 3 U (|y sc ik| + |sh ik|) SECOND.  The keep byte multiplies exactly.
  BatchNorm-backward P   E.bn_bwd_apply_tol with coef_tol = E.bn_bwd_coefs_tol: the kernels' form  c0 d - ((y - mean) (c0 c2 rstd) +
                         c0 c1)  with its two explicit fused multiply-adds counts 5 U on the xhat term, 3 U on the c1 term and U on
                         the d term -- inside 5 U |c0| T.
  sigmoid, C += ...      (EpiStore::compute, gemm_nt_epi.h.)  p = rcp(1 + exp2(-x log2 e)) on an x that carries tol_x (nt_tol).  The
                         sigmoid is monotone: the x of the kernel lies in [x - tol_x, x + tol_x], so the exact sigmoid of it lies in
                         [s(x - tol_x), s(x + tol_x)].  Arithmetic on top: the argument product -x * fl32(log2 e) carries U (the
                         constant) + U (the product) relative to |x| log2 e, i.e. 2 U |x| RELATIVE in e = exp(-x) -- it grows with
                         |x|; v_exp_f32 E_EXP; 1 + e one rounding U; v_rcp_f32 one ulp (ULP).  d p / p = -(1 - p) d e / e:
                           tol_p = max(s(x + tol_x) - p, p - s(x - tol_x)) + p ((1 - p) (2 U |x| + E_EXP) + U + ULP) + FLUSH,
                         FLUSH = 2^-126: the hardware transcendentals flush denormal results to zero (x < -87).   (sigmoid_tol)
                         Accumulate form C = old + v (v already rounded to the output type): one more rounding over |old| + |v|
                         (accumulate_tol).
  ReLU-mask epilogue     dH = h > 0 ? acc : 0 with the STORED h: the select is exact.  Where h <= 0 the bound is 0 (the element must be
                         exactly 0), elsewhere nt_tol (then bf16_out in bf16 mode)   (relu_mask).
  BatchNorm-backward epilogue   (EpiBnBwd in gemm_nt_epi.h; EpiBnBwdStream / nt2_bnbwd_epilogue in gemm_nt2.h: the same expressions.)
                         gate     y sc + sh > 0 is formed in fp32: a product and a sum (or one fma) of exact inputs, 2 U (|y sc| + |sh|)
                                  SECOND.  An element whose float64 gate value lies within that of 0 is AT RISK: the kernel may take
                                  either side, and its allowance is its whole |acc keep| (on top of the bound below).  No element is
                                  excluded   (bn_bwd_gate).
                         d        acc * keep: one rounding onto nt_tol:  tol_d = keep tol_acc + U |acc keep|   (bn_bwd_d).
                         phase 1  c0 (d - c1 - xhat c2): E.bn_bwd_apply_tol (5 U |c0| (|d| + |c1| + |xhat c2|)) plus |c0| tol_d, then
                                  bf16_out in bf16 mode   (bn_bwd_phase1_tol).
                         sums     sum d and sum d xhat over the UNROUNDED fp32 d: every d enters with its own tol_d (times |xhat| for
                                  the second sum); xhat = (y - mean) rstd and the product d xhat add 3 U per term of the second sum;
                                  fp32 partial sums over the rows one workgroup reduces before its f64 atomic, then f64 atomics.  Rows:
                                  accumulator-layout form 128 (one tile: nt_epilogue adds the two 64-row wave rows red[0] + red[2] in
                                  fp32 in front of the atomic); stream form 128 as well -- nt2_bnbwd_epilogue: a thread sums its 16 rows
                                  (r0 + 8 i), the 8 row groups are added in fp32 (`for g < 8: v += part[...]`) in front of the atomic,
                                  and every tile does its own atomic: ROWS_TILE for both   (bn_bwd_stats_tol).
  loss epilogues         (EpiLoss::term / term2, nt2_loss_epilogue in gemm_nt2.h.)  x = acc + bias carries nt_tol.
                         MSE      d = x - t: tol_d = tol_x + U (|x| + |t|); gradient 2 d (exact doubling) through bf16_out, pad columns
                                  exactly 0; term d d: 2 |d| tol_d + tol_d^2 + U d^2.
                         BCE      p = sigmoid(x) with sigmoid_tol.  torch, like the kernel, evaluates the logs on the FP32 p: the
                                  reference is  -(t LP(p32) + (1 - t) L1P(p32)),  p32 = fl32(s(x)),  LP(p) = max(ln p, -100),
                                  L1P(p) = max(ln fl32(1 - p), -100)  in float64 (the subtraction 1 - p of two fp32 values is correctly
                                  rounded: the kernel's 1 - pe IS fl32(1 - pe)).  The kernel's pe is an fp32 value within tol_p of s(x),
                                  hence in [fl32(p - tol_p), fl32(p + tol_p)] (rounding is monotone); LP rises and L1P falls with p:
                                  evaluate both at the two ends.  v_log_f32 one ulp, the constant ln 2 and its product U each:
                                  (ULP + 2 U) |log|.  Near saturation the interval contains p = 1 (or 0) and the bound is as wide as
                                  the clamp: that is the operation's own sensitivity, not slack.  Term: 1 - t, the product and the fma
                                  3 U (|t lp| + |(1 - t) l1p|).  Gradient (p - t) f, f = min(p (1 - p) 1e12, 1): d = p - t carries
                                  tol_p + U (|p| + |t|); f is exactly 1 unless p (1 - p) 1e12 comes within its own error of 1
                                  (|x| > 27); one rounding for the product; bf16_out.
                         sum      fp32 partial sums of one tile: a thread adds its 64 terms, wave_sum the 64 lanes: LOSS_TERMS = 4096
                                  terms per fp32 sum; the 4 waves and the tiles are added in f64   (loss_sum_tol).
  column statistics      stat1 / stat2 are fp32 partial sums over the rows ONE workgroup reduces before its f64 atomic, then f64
                         atomics.  The row count is read off each kernel's epilogue:
                           tile kernels (gemm_nt.hip, 128 x 128 and 128 x 256): one 128-row tile -- red[...] in gemm_nt_epi.h holds
                              the sums of the two 64-row wave rows, added once more in fp32 in front of the atomic: ROWS_TILE = 128;
                           wave-specialised kernel (gemm_ntp.h): st_sum1 / wgstat accumulate over ALL row tiles a persistent
                              workgroup owns in one column tile before flush_stats: 128 ceil(row tiles / workgroups per column
                              tile) rows, with a grid of min(256, tiles) workgroups (launch_ntp): ntp_rows().
                         Bound: (rows - 1) U sum |stored values| for the sums; the squares carry one more rounding each (v * v):
                         rows U sum v^2; plus M F64 of the same magnitudes for the f64 atomics   (stats_tol).
"""
import numpy as np

from elementwise_bounds import (U, ULP, E_EXP, SECOND, BF16, F64, bf16_out, accum_tol, bn_finalize_tol,  # noqa: F401  (re-exported)
                                bn_bwd_coefs, bn_bwd_coefs_tol, bn_bwd_apply, bn_bwd_apply_tol)

ROWS_TILE = 128


def _f(x):
    return np.asarray(x, np.float64)


def q_bf16(x):
    """float64 -> the nearest bf16 value (ties to even), as float64.  No detour through float32 (that would round twice)."""
    m, e = np.frexp(_f(x))
    return np.ldexp(np.rint(m * 256.0), e - 8)


def ntp_rows(M, N):
    """Rows behind one fp32 partial sum of the wave-specialised kernel: gx row tiles (padded to a multiple of 8) times gy column
    tiles over min(256, tiles) persistent workgroups; a workgroup's tiles of one column tile are summed before the atomic."""
    bn = 256 if N % 256 == 0 else 128
    gx, gy = (M + 127) // 128, (N + bn - 1) // bn
    ntiles = (gx + 7) // 8 * 8 * gy
    return 128 * -(-ntiles // min(256, ntiles))


# ---------------------------------------------------------------------------------------------
# operands formed in the kernel
# ---------------------------------------------------------------------------------------------
def prologue_value(y, scale, shift, inv_keep, dt, scale_only=False):
    """relu's argument y (scale ik) + shift ik in `dt` (float32: the kernel's table and a product + sum).  scale_only: the deliberate
    mistake of applying inv_keep to the scale alone."""
    ik = dt(np.float32(inv_keep))
    sc = np.asarray(scale, np.float32).astype(dt) * ik
    sh = np.asarray(shift, np.float32).astype(dt) * (dt(1) if scale_only else ik)
    return np.asarray(y).astype(dt) * sc + sh


def prologue_tol(y, scale, shift, inv_keep):
    ik = float(np.float32(inv_keep))
    return SECOND * 3 * U * (np.abs(_f(y) * _f(scale) * ik) + np.abs(_f(shift) * ik))


def operand_risk(v, tol_v, bf16, relu=False, keep=None):
    """-> (h, dh): the reference operand q(relu(v)) * keep and the width of the interval in which the kernel's operand lies (module
    docstring).  bf16 False (fp32 mode): no rounding, dh = tol_v."""
    v, tol_v = _f(v), _f(tol_v)
    r = (lambda x: np.maximum(x, 0.0)) if relu else (lambda x: x)
    if bf16:
        h, dh = q_bf16(r(v)), q_bf16(r(v + tol_v)) - q_bf16(r(v - tol_v))
    else:
        h, dh = r(v), np.broadcast_to(tol_v, v.shape).copy()
    if keep is not None:
        k = _f(keep)
        h, dh = h * k, dh * k
    return h, dh


def prologue_operand(y, scale, shift, inv_keep, mask, bf16):
    """The A / Q operand behind the BatchNorm + ReLU + Dropout prologue from the fp32 tables: (h float64 reference, dh allowance)."""
    return operand_risk(prologue_value(y, scale, shift, inv_keep, np.float64), prologue_tol(y, scale, shift, inv_keep), bf16, relu=True, keep=mask)


def bn_bwd_operand(d, y, mean, rstd, sd, sdx, M, gamma, eval_mode, bf16=True):
    """The P operand behind the BatchNorm-backward correction with the finalisation folded in: float64 from the f64 sums (eval mode:
    gamma rstd d exactly), E.bn_bwd_apply_tol with the coefficients' own bounds for the value before rounding.  -> (p, dp)"""
    coef = bn_bwd_coefs(sd, sdx, M, gamma, rstd, eval_mode, np.float64)
    ctol = bn_bwd_coefs_tol(sd, sdx, M, gamma, rstd, eval_mode)
    return operand_risk(bn_bwd_apply(d, y, mean, rstd, coef, np.float64), bn_bwd_apply_tol(d, y, mean, rstd, coef, ctol), bf16)


# ---------------------------------------------------------------------------------------------
# products
# ---------------------------------------------------------------------------------------------
def nt_ref(a, w, bias):
    return _f(a) @ _f(w).T + (0.0 if bias is None else _f(bias))


def nt_tol(a, w, bias, dh=None, out_bf16=False, ref=None):
    """Bound of C = a w^T + bias (module docstring); dh: allowance of the operand a; out_bf16: C stored as bf16 (needs ref)."""
    K = np.shape(a)[1]
    aw = np.abs(_f(a)) @ np.abs(_f(w)).T
    tol = SECOND * (K + 1) * U * (aw + (0.0 if bias is None else np.abs(_f(bias))))
    if dh is not None:
        tol = tol + _f(dh) @ np.abs(_f(w)).T
    return bf16_out(tol, ref) if out_bf16 else tol


def dw_ref(p, q, old_dw, old_db, mm=np.matmul):
    """mm: the float64 matrix product (the GPU tests hand in a device float64 matmul where the host would take more than seconds)."""
    p = _f(p)
    return _f(old_dw) + mm(p.T, _f(q)), _f(old_db) + p.sum(0)


def dw_tol(p, q, old_dw, old_db, dp=None, dq=None, atomics=False, mm=np.matmul):
    """-> (bound of dW, bound of db) (module docstring); dp / dq: allowances of the operands P / Q; atomics: no slab, or row blocks."""
    p, q = np.abs(_f(p)), np.abs(_f(q))
    M = p.shape[0]
    pq, ps = mm(p.T, q), p.sum(0)
    if atomics:
        tw = SECOND * M * U * (np.abs(_f(old_dw)) + pq)
    else:
        tw = SECOND * ((M - 1) * U * pq + U * (np.abs(_f(old_dw)) + pq))
    tb = SECOND * M * U * (np.abs(_f(old_db)) + ps)
    if dp is not None:
        tw, tb = tw + mm(_f(dp).T, q), tb + _f(dp).sum(0)
    if dq is not None:
        tw = tw + mm(p.T, _f(dq))
    return tw, tb


def dw_order_tol(p, q, old_dw, old_db, atomics=False):
    """Two launches that multiply the SAME operands differ only by the order of the fp32 sums: each is inside dw_tol (without
    allowances) of the exact sum, so they are within twice that of each other."""
    tw, tb = dw_tol(p, q, old_dw, old_db, atomics=atomics)
    return 2 * tw, 2 * tb


# ---------------------------------------------------------------------------------------------
# column statistics
# ---------------------------------------------------------------------------------------------
def stats_ref(c):
    c = _f(c)
    return np.stack([c.sum(0), (c * c).sum(0)])


def stats_tol(c, rows):
    """[2][N] bound of (stat1, stat2) against the float64 sums of the stored values c [M][N]; rows: see the module docstring."""
    c = _f(c)
    M = c.shape[0]
    rows = min(rows, M)
    a1, a2 = np.abs(c).sum(0), (c * c).sum(0)
    return np.stack([SECOND * ((rows - 1) * U + M * F64) * a1, SECOND * (rows * U + M * F64) * a2])


def sums_rel(c, rows):
    """The statistics bound as the `sums_rel` of E.bn_finalize_tol, per column, for a finalisation whose sums came from a GEMM's
    atomics and whose reference is computed from the data: the variance s2 / M - mean^2 moves by tol2 / M + 2 |mean| tol1 / M
    <= (tol2 / s2 + 2 tol1 / |s1|) (s2 / M + mean^2), and the mean by tol1 / |s1| of itself."""
    s, t = stats_ref(c), stats_tol(c, rows)
    tiny = np.finfo(np.float64).tiny
    return t[1] / np.maximum(s[1], tiny) + 2 * t[0] / np.maximum(np.abs(s[0]), tiny)


# ---------------------------------------------------------------------------------------------
# epilogues of the NT GEMM (module docstring)
# ---------------------------------------------------------------------------------------------
FLUSH = 2.0 ** -126
LOSS_TERMS = 4096
LOG2E32 = float(np.float32(1.4426950408889634))


def f32r(x):
    """float64 -> the nearest float32 value, as float64."""
    return _f(x).astype(np.float32).astype(np.float64)


def sigmoid(x):
    x = _f(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sigmoid_tol(x, tol_x):
    x, tol_x = _f(x), _f(tol_x)
    p = sigmoid(x)
    prop = np.maximum(sigmoid(x + tol_x) - p, p - sigmoid(x - tol_x))
    return SECOND * (prop + p * (sigmoid(-x) * (2 * U * np.abs(x) + E_EXP) + U + ULP)) + FLUSH


def accumulate_tol(tol_v, v, old):
    """C = old + v."""
    return SECOND * (_f(tol_v) + U * (np.abs(_f(old)) + np.abs(_f(v))))


def relu_mask(acc, tol_acc, h):
    """-> (reference, bound) of dH = h > 0 ? acc : 0 from the stored h."""
    on = _f(h) > 0
    return np.where(on, _f(acc), 0.0), np.where(on, _f(tol_acc), 0.0)


def bn_bwd_gate(y, scale, shift):
    """-> (gate open in float64, at risk)."""
    y, sc, sh = _f(y), _f(scale), _f(shift)
    g = y * sc + sh
    return g > 0, np.abs(g) <= SECOND * 2 * U * (np.abs(y * sc) + np.abs(sh))


def bn_bwd_d(acc, tol_acc, y, scale, shift, mask, inv_keep):
    """d = acc keep (gate) -> (reference, bound incl. the at-risk allowance, share of elements at risk)."""
    keep = float(np.float32(inv_keep)) * _f(mask) if mask is not None else np.ones(np.shape(acc))
    gate, risk = bn_bwd_gate(y, scale, shift)
    full = _f(acc) * keep
    tol = SECOND * (keep * _f(tol_acc) + U * np.abs(full))
    return np.where(gate, full, 0.0), np.where(gate | risk, tol, 0.0) + np.where(risk, np.abs(full), 0.0), float(risk.mean())


def bn_bwd_phase1_tol(d, tol_d, y, mean, rstd, coef):
    return bn_bwd_apply_tol(d, y, mean, rstd, coef) + SECOND * np.abs(_f(coef)[0]) * _f(tol_d)


def bn_bwd_stats(d, y, mean, rstd):
    d = _f(d)
    xh = (_f(y) - _f(mean)) * _f(rstd)
    return np.stack([d.sum(0), (d * xh).sum(0)])


def bn_bwd_stats_tol(d, tol_d, y, mean, rstd, rows=ROWS_TILE):
    d, tol_d = _f(d), _f(tol_d)
    M = d.shape[0]
    rows = min(rows, M)
    xh = np.abs((_f(y) - _f(mean)) * _f(rstd))
    a1, a2 = (np.abs(d) + tol_d).sum(0), ((np.abs(d) + tol_d) * xh).sum(0)
    return np.stack([SECOND * (tol_d.sum(0) + ((rows - 1) * U + M * F64) * a1),
                     SECOND * ((tol_d * xh).sum(0) + (3 * U + (rows - 1) * U + M * F64) * a2)])


def mse_epilogue(x, tol_x, t):
    """-> (gradient 2 (x - t), its bound before bf16_out, terms (x - t)^2, their bounds)."""
    x, t = _f(x), _f(t)
    d = x - t
    tol_d = _f(tol_x) + U * (np.abs(x) + np.abs(t))
    return 2 * d, SECOND * 2 * tol_d, d * d, SECOND * (2 * np.abs(d) * tol_d + tol_d ** 2 + U * d * d)


def _clog(p):
    with np.errstate(divide="ignore"):
        return np.maximum(np.log(p), -100.0)


def bce_lp(p, clamp=True):
    with np.errstate(divide="ignore"):
        return _clog(p) if clamp else np.log(p)


def bce_l1p(p, clamp=True):
    return bce_lp(f32r(1.0 - _f(p)), clamp)


def bce_epilogue(x, tol_x, t):
    """-> (gradient w.r.t. the logit, its bound before bf16_out, loss terms, their bounds) (module docstring)."""
    x, t = _f(x), _f(t)
    p, q, tol_p = sigmoid(x), sigmoid(-x), sigmoid_tol(x, tol_x)
    p32, lo, hi = f32r(p), f32r(np.maximum(p - tol_p, 0.0)), f32r(np.minimum(p + tol_p, 1.0))
    e_log = ULP + 2 * U
    lp, l1p = bce_lp(p32), bce_l1p(p32)
    tol_lp = np.maximum(bce_lp(hi) - lp, lp - bce_lp(lo)) + e_log * np.abs(lp)
    tol_l1p = np.maximum(bce_l1p(lo) - l1p, l1p - bce_l1p(hi)) + e_log * np.abs(l1p)
    term = -(t * lp + (1 - t) * l1p)
    mag = np.abs(t * lp) + np.abs((1 - t) * l1p)
    tol_term = SECOND * (np.abs(t) * tol_lp + np.abs(1 - t) * tol_l1p + 3 * U * mag)
    fraw = p * q * 1e12
    e_f = 1e12 * (tol_p * (p + q) + 4 * U * p * q)
    f = np.minimum(fraw, 1.0)
    tol_f = np.maximum(np.minimum(fraw + e_f, 1.0) - f, f - np.clip(fraw - e_f, 0.0, 1.0))
    d = p - t
    tol_d = tol_p + U * (np.abs(p) + np.abs(t))
    return d * f, SECOND * (f * tol_d + np.abs(d) * tol_f + tol_d * tol_f + U * np.abs(d * f)), term, tol_term


def loss_sum_tol(terms, tol_terms):
    """Bound of the f64 loss accumulator against the float64 sum of the reference terms."""
    a = float((np.abs(_f(terms)) + _f(tol_terms)).sum())
    return SECOND * (float(_f(tol_terms).sum()) + ((LOSS_TERMS - 1) * U + np.size(terms) * F64) * a)
