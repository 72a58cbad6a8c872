"""Formulas and DERIVED error bounds of the stand-alone loss kernel (vae_loss_kernel in csrc/elementwise.hip, the class / KL
arithmetic of csrc/loss_terms.h), shared by tests/test_loss_kernel_gpu.py (device against float64, every element) and
tests/test_loss_bounds_cpu.py (a float32 numpy restatement of each expression must stay inside the same bound, and a set of deliberate
mistakes must fall outside).  The inputs come from tests/loss_cases.py.

Every formula takes `dt`: np.float64 gives the reference, np.float32 the restatement of the kernel's expression.  The inputs are
float32 (or bf16 targets, widened exactly) and count as exact.  The model of one float32 operation and the constants U, ULP, E_EXP,
E_DIV, SECOND, BF16, F64, bf16_out are those of tests/elementwise_bounds.py; FLUSH, mse_epilogue, bce_lp / bce_l1p and the interval
evaluation at a clamp are those of tests/gemm_bounds.py.  Nothing below was fitted to what the kernel returns, and every bound is per
element, relative to the magnitude of that element's own terms.

  E_LOG    libm logf (the class term's logf(se) on every path): 2 ulp.  An ASSUMPTION, exactly as E_EXP is one: the ulp table of the HIP
           math functions is not part of this tree or of the toolchain's installed documentation.  DESIGN.md records how much of it
           the device uses.
  E_RCP    v_rcp_f32: one ulp (ULP).
  E_VLOG   v_log_f32 times the constant ln 2: ULP for the instruction, U for the constant, U for the product: ULP + 2 U of |ln|.

MSE       mse_epilogue with tol_x = 0: d = x - t carries U (|x| + |t|), the gradient 2 d is an exact doubling, the term d d one more
          rounding.
BCE       The kernel takes the fp32 p as an EXACT input (the GEMM epilogue's rule starts from the logit; this one from p).
          term   -(t LP + (1 - t) L1P), LP = max(ln p, -100), L1P = max(ln fl32(1 - p), -100): the subtraction 1 - p of two fp32 values
                 is correctly rounded, so the kernel's 1 - p IS fl32(1 - p) and the reference takes its log in float64.  Each log E_VLOG
                 of its own clamped magnitude (the clamp is monotone and 1-Lipschitz; a log below -100 stays clamped unless it lies
                 within its own error of -100, which SECOND covers).  A p below 2^-126 takes the scaled form ln(p 2^32) - 32 ln 2 (the
                 instruction does not read denormal inputs): the scaling is exact, the log of the scaled value is smaller in magnitude,
                 the constant 32 ln 2 and the subtraction add one U of |ln p| between them: E_VLOG + U there.  Then 1 - t, two
                 products and a sum: 3 U (|t LP| + |(1 - t) L1P|).
          pq     fl(fl(1 - p) p): 2 U pq, and where the product is denormal half a denormal ulp, U FLUSH, absolute.
          d      p - t: U (|p| + |t|) (the convention of bce_epilogue).
          w.r.t. the logit   d min(pq 1e12, 1).  fraw = pq 1e12 carries the error of pq times 1e12, U for the fp32 constant and U for the
                 product; f = min(fraw, 1) is evaluated at BOTH ENDS of that error, as bce_epilogue does at this clamp; then the product.
          w.r.t. p   d rcp(max(pq, 1e-12)).  max is monotone: the larger of two values that each carry at most 2 U (pq) or U (the fp32
                 constant 1e-12) carries at most 2 U; v_rcp_f32 E_RCP; the product U.  All RELATIVE: the value reaches 1e12.
          Either product may underflow (a denormal p against the target 0): U FLUSH absolute, as for pq.  A bf16 gradient goes
          through bf16_out.
class     w = class weight of the label (0 for -100, class 0 for a label outside [0, S)), gw = fl(gamma w): U.
          e_j    expf(fl(x_j - m)), m the exact row maximum: the rounding of x - m is U |x - m| RELATIVE in e, expf E_EXP, and FLUSH
                 absolute where the exponential underflows.
          se     S - 1 additions in ANY order (ascending on the row-per-thread and scalar paths, a butterfly on the half-wave path):
                 sum tol_e + (S - 1) U se.
          term   w (m + logf(se) - x_y): logf carries tol_se / se from its argument and E_LOG |ln se|; two additions over the magnitude
                 M = |m| + |ln se| + |x_y|, one product: |w| (tol_log + 3 U M).  ONE bound for all three paths: they state this
                 expression alike (the scalar path names m + logf(se) `lse` first).
          g_c    TWO bounds, one per expression:
                 softmax form (row-per-thread, half-wave)   gw (e / se - onehot): the quotient r carries tol_e / se + r (tol_se / se +
                     E_DIV); the subtraction, the product and gw itself 3 U (r + onehot).
                 scalar form   gw (expf(x - lse) - onehot): lse carries tol_log + U (|m| + |ln se|) ABSOLUTE, which with the rounding of
                     x - lse, U |x - lse|, is relative in the exponential; E_EXP; FLUSH; then 3 U (r + onehot) as above.
                 Both are multiples of |gw|: the gradient row of an ignored label or of a zero class weight must be EXACTLY 0.
KL        ex = expf(lv): E_EXP ex + FLUSH.  Contraction is off (loss_terms.h), every operation rounds:
          term   -0.5 (((1 + lv) - mu mu) - ex): 1 + lv U (1 + |lv|); mu mu U mu^2; the two subtractions U each over what they have
                 collected: 0.5 (tol_ex + U (3 (1 + |lv|) + 3 mu^2 + ex)).
          g_mu   beta mu: U |beta mu|.       g_lv   (-0.5 beta) (1 - ex): 0.5 |beta| (tol_ex + U (1 + ex)) + U |g_lv|.
sums      sums[k] against the float64 sum of the reference terms: every term's own bound, plus "n terms in any order" over the FP32
          part of the chain -- (n32 - 1) U sum (|term| + tol) with n32 the number of terms one fp32 partial sum can hold -- plus
          n F64 for the f64 part (the four waves, the atomics).  n32 is read off the kernel (fp32_chain):
             not TAIL   a thread adds its own terms in fp32, wave_sum the 64 lanes: 64 x (terms of one thread).
             TAIL       the row-per-thread class term and the KL term widen EVERY term before adding it: n32 = 1, only the terms'
                        bounds and n F64 remain.  The half-wave and scalar class paths still add a thread's own rows in fp32
                        (`s[2] += ...`) and widen that sum: n32 = rows of one thread.
          The grid that decides these counts is restated below (launch) from launch_loss in csrc/elementwise.hip; if the launcher
          changes, that function is the one place to update.
          sums[4], the count of labels outside [0, S), is EXACT.
"""
import numpy as np

from elementwise_bounds import U, ULP, E_EXP, E_DIV, SECOND, BF16, F64, bf16_out  # noqa: F401  (re-exported)
from gemm_bounds import FLUSH, mse_epilogue, bce_lp, bce_l1p, f32r, q_bf16  # noqa: F401

E_LOG = 2 * ULP
E_RCP = ULP
E_VLOG = ULP + 2 * U
LN2_32 = np.float32(0.6931471805599453)
C1E12_32, C1EM12_32 = np.float32(1e12), np.float32(1e-12)


def _a(x, dt):
    return np.asarray(x).astype(dt)


def _f(x):
    return np.asarray(x, np.float64)


# ---------------------------------------------------------------------------------------------
# the launcher's choices (launch_loss, csrc/elementwise.hip), restated
# ---------------------------------------------------------------------------------------------
def vec_width(W, operands):
    """The vector width of one streaming part: the widest of 4, 2 that divides W and, for every operand (pointer, leading dimension,
    element size; pointer None = absent), its leading dimension and its address in units of v elements; else 1."""
    for v in (4, 2):
        if W % v == 0 and all(p is None or (ld % v == 0 and p % (v * es) == 0) for p, ld, es in operands):
            return v
    return 1


def ce_path(S, ld_logits, p_logits, ld_gc=0, p_gc=None):
    """'thread' (one row per thread, 16-byte accesses), 'half' (one row per half wave) or 'scalar' (S > 32)."""
    if S <= 32 and S % 4 == 0 and ld_logits % 4 == 0 and p_logits % 16 == 0 and (p_gc is None or (ld_gc % 4 == 0 and p_gc % 16 == 0)):
        return "thread"
    return "half" if S <= 32 else "scalar"


def grid_for(items, per_block, cap):
    return int(min(max(-(-items // per_block), 1), cap))


def launch(B, A=0, va=1, D=0, vd=1, S=0, path=None, L=0):
    """-> (workgroups of 256 threads, TAIL form?).  A / D / S / L = 0: that part is absent."""
    work = B * ((A // va if A else 0) + (D // vd if D else 0) + (4 * S if S else 0) + L + 1)
    grid = grid_for(work, 256 * 4, 1024)
    tail = not A and not D
    if tail:
        grid = min(512, -(-B // 256)) if path == "thread" else min(grid, 512)
    return grid, tail


def fp32_chain(part, grid, tail, B, W=0, V=1, path=None):
    """Terms one fp32 partial sum of sums[k] can hold (module docstring).  part: 'stream' (W columns in V-wide vectors), 'class', 'kl'
    (W = L)."""
    threads = grid * 256
    if part == "stream":
        return 64 * V * -(-(B * (W // V)) // threads)
    if part == "kl":
        return 1 if tail else 64 * -(-(B * W) // threads)
    if path == "thread":
        return 1 if tail else 64 * -(-B // threads)
    own = -(-B // (grid * 8)) if path == "half" else -(-B // threads)        # half wave: 2 rows per wave and pass
    return own if tail else 64 * own


def sum_tol(terms, tol_terms, n32):
    """Bound of one f64 accumulator against the float64 sum of the reference terms."""
    a = float((np.abs(_f(terms)) + _f(tol_terms)).sum())
    return SECOND * (float(_f(tol_terms).sum()) + ((n32 - 1) * U + np.size(terms) * F64) * a)


# ---------------------------------------------------------------------------------------------
# MSE
# ---------------------------------------------------------------------------------------------
def mse(x, t, dt, mistake=None):
    """-> (gradient 2 (x - t), term (x - t)^2)"""
    d = _a(x, dt) - _a(t, dt)
    return (dt(1) if mistake == "factor 1" else dt(2)) * d, d * d


def mse_tol(x, t):
    """-> (bound of the gradient before bf16_out, bound of the term)"""
    _, tg, _, tt = mse_epilogue(x, 0.0, t)
    return tg, tt


# ---------------------------------------------------------------------------------------------
# BCE on a given p
# ---------------------------------------------------------------------------------------------
def bce(p, t, wrt_logit, dt, mistake=None):
    """-> (gradient, term).  float64: the reference (logs of the fp32 p and of fl32(1 - p), exact p (1 - p), the constants 1e12 and
    1e-12).  float32: the kernel's expression -- v_log_f32 restated as log2 times the fp32 ln 2, its fp32 constants, rcp as 1 / x.
    mistake: 'clamp -88', 'no min factor', 'clamp 1e-6'."""
    p, t = _a(p, dt), _a(t, dt)
    one = dt(1)
    if dt == np.float64:
        lp, l1p = bce_lp(p), bce_l1p(p)
        c12, cm12 = 1e12, 1e-12
    else:
        floor = dt(-88) if mistake == "clamp -88" else dt(-100)
        with np.errstate(divide="ignore"):
            tiny = p < dt(FLUSH)                              # scaled by 2^32, 32 ln 2 taken off again (bce_part_g)
            lnp = np.log2(np.where(tiny, p * dt(2.0 ** 32), p)) * LN2_32 - np.where(tiny, dt(32 * np.log(2.0)), dt(0))
            lp, l1p = np.maximum(lnp, floor), np.maximum(np.log2(one - p) * LN2_32, floor)
        c12, cm12 = C1E12_32, (dt(1e-6) if mistake == "clamp 1e-6" else C1EM12_32)
    pq, d = (one - p) * p, p - t
    if wrt_logit:
        g = d if mistake == "no min factor" else d * np.minimum(pq * c12, one)
    else:
        g = d * (one / np.maximum(pq, cm12))
    return g, -(t * lp + (one - t) * l1p)


def bce_tol(p, t, wrt_logit):
    """-> (bound of the gradient before bf16_out, bound of the term) (module docstring)."""
    p, t = _f(p), _f(t)
    lp, l1p = bce_lp(p), bce_l1p(p)
    tol_lp = (E_VLOG + np.where(p < FLUSH, U, 0.0)) * np.abs(lp)
    tol_l1p = E_VLOG * np.abs(l1p)
    mag = np.abs(t * lp) + np.abs((1 - t) * l1p)
    tol_term = SECOND * (np.abs(t) * tol_lp + np.abs(1 - t) * tol_l1p + 3 * U * mag)
    pq, d = (1 - p) * p, p - t
    tol_pq = 2 * U * pq + U * FLUSH
    tol_d = U * (np.abs(p) + np.abs(t))
    if wrt_logit:
        fraw = pq * 1e12
        e_f = 1e12 * tol_pq + 2 * U * fraw
        f = np.minimum(fraw, 1.0)
        tol_f = np.maximum(np.minimum(fraw + e_f, 1.0) - f, f - np.clip(fraw - e_f, 0.0, 1.0))
        return SECOND * (f * tol_d + np.abs(d) * tol_f + tol_d * tol_f + U * np.abs(d * f)) + U * FLUSH, tol_term
    r = 1.0 / np.maximum(pq, 1e-12)
    return SECOND * (r * tol_d + np.abs(d) * r * (2 * U + E_RCP) + U * np.abs(d) * r) + U * FLUSH, tol_term


# ---------------------------------------------------------------------------------------------
# class term
# ---------------------------------------------------------------------------------------------
def ce_labels(y, S, cw, dt, mistake=None):
    """-> (class used [B], weight [B], labels outside [0, S)).  mistake: 'wrong weight', 'ignore as class 0', 'bad label kept'."""
    y = np.asarray(y, np.int64)
    ign = y == -100
    bad = ~ign & ((y < 0) | (y >= S))
    yy = np.where(bad | ign, 0, y)
    if mistake == "bad label kept":
        yy = np.where(bad, np.clip(y, 0, S - 1), yy)            # clamped into range instead of class 0
    wy = (yy + 1) % S if mistake == "wrong weight" else yy
    w = np.ones(len(y), dt) if cw is None else _a(cw, dt)[wy]
    if mistake != "ignore as class 0":
        w = np.where(ign, dt(0), w)
    elif cw is not None:
        w = np.where(ign, dt(1), w)
    return yy, w.astype(dt), int(bad.sum())


def _row_sum(e, order):
    """Sum over the columns: 'seq' ascending (the row-per-thread and scalar paths), 'tree' the half wave's xor butterfly over 32 lanes."""
    if order == "seq":
        se = e[:, 0].copy()
        for j in range(1, e.shape[1]):
            se = se + e[:, j]
        return se
    v = np.zeros((e.shape[0], 32), e.dtype)
    v[:, :e.shape[1]] = e
    lane = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return v[:, 0]


def ce(x, y, cw, gamma, form, dt, order="seq", mistake=None):
    """-> (terms [B], gradient [B][S], labels outside [0, S)).  form: 'softmax' (row-per-thread, half-wave) or 'scalar'.
    mistake: the three of ce_labels, 'onehot y+1', 'gamma dropped', 'no max'."""
    x = _a(x, dt)
    B, S = x.shape
    yy, w, n_bad = ce_labels(y, S, cw, dt, mistake)
    hit = (np.arange(S)[None, :] == ((yy + 1) % S if mistake == "onehot y+1" else yy)[:, None]).astype(dt)
    m = np.zeros(B, dt) if mistake == "no max" else x.max(1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(x - m[:, None])
        se = _row_sum(e, order)
        lse = m + np.log(se)
        term = w * (lse - x[np.arange(B), yy])
        gw = w if mistake == "gamma dropped" else dt(np.float32(gamma)) * w
        r = e / se[:, None] if form == "softmax" else np.exp(x - lse[:, None])
        g = gw[:, None] * (r - hit)
    return term, g, n_bad


def ce_tol(x, y, cw, gamma, form):
    """-> (bound of the terms [B], bound of the gradient [B][S]) (module docstring)."""
    x = _f(x)
    B, S = x.shape
    yy, w, _ = ce_labels(y, S, cw, np.float64)
    hit = (np.arange(S)[None, :] == yy[:, None]).astype(np.float64)
    m = x.max(1)
    xm = x - m[:, None]
    e = np.exp(xm)
    tol_e = e * (U * np.abs(xm) + E_EXP) + FLUSH
    se = e.sum(1)
    tol_se = tol_e.sum(1) + (S - 1) * U * se
    L = np.log(se)
    tol_log = tol_se / se + E_LOG * np.abs(L)
    M = np.abs(m) + np.abs(L) + np.abs(x[np.arange(B), yy])
    tol_term = SECOND * np.abs(w) * (tol_log + 3 * U * M)
    gw = np.abs(float(np.float32(gamma)) * w)[:, None]
    if form == "softmax":
        r = e / se[:, None]
        tol_r = tol_e / se[:, None] + r * (tol_se / se + E_DIV)[:, None]
    else:
        lse = m + L
        r = np.exp(x - lse[:, None])
        tol_lse = tol_log + U * (np.abs(m) + np.abs(L))
        tol_r = r * (tol_lse[:, None] + U * np.abs(x - lse[:, None]) + E_EXP) + FLUSH
    return tol_term, SECOND * gw * (tol_r + 3 * U * (r + hit))


# ---------------------------------------------------------------------------------------------
# KL term
# ---------------------------------------------------------------------------------------------
def kl(mu, lv, beta, dt, mistake=None):
    """-> (terms, g_mu, g_lv), kl_elem of csrc/loss_terms.h.  mistake: 'g_lv sign', 'exp half'."""
    mu, lv, beta = _a(mu, dt), _a(lv, dt), dt(np.float32(beta))
    with np.errstate(under="ignore"):
        ex = np.exp(dt(0.5) * lv if mistake == "exp half" else lv)
    g_lv = dt(-0.5) * beta * (dt(1) - ex)
    return dt(-0.5) * (dt(1) + lv - mu * mu - ex), beta * mu, -g_lv if mistake == "g_lv sign" else g_lv


def kl_tol(mu, lv, beta):
    """-> bounds of (terms, g_mu, g_lv) (module docstring)."""
    mu, lv, b = _f(mu), _f(lv), abs(float(np.float32(beta)))
    ex = np.exp(lv)
    tol_ex = E_EXP * ex + FLUSH
    tol_t = 0.5 * (tol_ex + U * (3 * (1 + np.abs(lv)) + 3 * mu * mu + ex))
    g_lv = 0.5 * b * np.abs(1 - ex)
    return SECOND * tol_t, SECOND * U * b * np.abs(mu), SECOND * (0.5 * b * (tol_ex + U * (1 + ex)) + U * g_lv)
