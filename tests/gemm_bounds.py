"""DERIVED per-element error bounds of the GEMM kernels (csrc/gemm_nt.hip, gemm_ntp.h, gemm_tn.hip, gemm_tn_wide.hip), shared by
tests/test_gemm_folded_gpu.py (device against float64) and tests/test_gemm_bounds_cpu.py (a float32 numpy restatement must stay
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
                         U (|old| + sum |p q|)   (dw_tol).  That is the slab form, which every test here uses (a slab is always
                         handed in).  db[n] = old + sum_m p[m][n] likewise over |p_m|, except that the kernels add every split's
                         column sum onto db with f32 atomics: the old value is one of M + 1 terms summed in any order,
                         M U (|old| + sum |p|)   (db_tol).
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

from elementwise_bounds import (U, SECOND, BF16, F64, bf16_out, accum_tol, bn_finalize_tol,  # noqa: F401  (re-exported)
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


def dw_ref(p, q, old_dw, old_db):
    p = _f(p)
    return _f(old_dw) + p.T @ _f(q), _f(old_db) + p.sum(0)


def dw_tol(p, q, old_dw, old_db, dp=None, dq=None):
    """-> (bound of dW, bound of db) (module docstring); dp / dq: allowances of the operands P / Q."""
    p, q = np.abs(_f(p)), np.abs(_f(q))
    M = p.shape[0]
    pq, ps = p.T @ q, p.sum(0)
    tw = SECOND * ((M - 1) * U * pq + U * (np.abs(_f(old_dw)) + pq))
    tb = SECOND * M * U * (np.abs(_f(old_db)) + ps)
    if dp is not None:
        tw, tb = tw + _f(dp).T @ q, tb + _f(dp).sum(0)
    if dq is not None:
        tw = tw + p.T @ _f(dq)
    return tw, tb


def dw_order_tol(p, q, old_dw, old_db):
    """Two launches that multiply the SAME operands differ only by the order of the fp32 sums: each is inside dw_tol (without
    allowances) of the exact sum, so they are within twice that of each other."""
    tw, tb = dw_tol(p, q, old_dw, old_db)
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
