"""Formulas and DERIVED error bounds of the memory-bound kernels of csrc/elementwise.hip, shared by tests/test_elementwise_gpu.py
(device against float64) and tests/test_elementwise_ref_cpu.py (a float32 numpy restatement of each formula must stay inside the
same bound, which shows that no bound is tighter than float32 arithmetic itself).

Every formula takes `dt`: np.float64 gives the reference, np.float32 the restatement.  The inputs are float32 values (or float64
sums) and count as exact.  No bound below was fitted to what the kernels return; the model of one float32 operation is

  U        2^-24: the relative error of one correctly rounded operation (add, multiply, fused multiply-add, conversion).
  ULP      2 U: one ulp relative to the value, at worst (just above a power of two).
  E_EXP, E_POW   expf / powf: 2 ulp.  An ASSUMPTION: the ulp table of the HIP math functions is not part of this tree or of the
           toolchain's installed documentation; if a ROCm release documents more, these two constants are the place to change.
  E_DIV    fp32 division 2.5 ulp, E_SQRT sqrtf 1 ulp: the library is built without -fhip-fp32-correctly-rounded-divide-sqrt and
           without fast-math, so neither is taken as correctly rounded.
  sums     n terms summed in ANY order (loops, trees, LDS or global atomics): (n - 1) U sum |terms|.
  fma      a contracted a * b + c drops one rounding: every bound counts the uncontracted roundings, which covers both forms.
  SECOND   the analysis is first order; every relative error term that enters is below 2^-10 (the largest: the bias corrections
           of AdamW at t = 1, 4 U * 999), so the neglected products of two terms are below 2^-10 of the bound.
  BF16     a bf16 output adds 2^-8 of the value (one bf16 ulp).

Errors are taken relative to the MAGNITUDE OF THE TERMS (sum of absolute values), never of a result that may have cancelled.
"""
import numpy as np

U = 2.0 ** -24
ULP = 2 * U
E_EXP = 2 * ULP
E_POW = 2 * ULP
E_DIV = 2.5 * ULP
E_SQRT = 1 * ULP
SECOND = 1.0 + 2.0 ** -10
BF16 = 2.0 ** -8
F64 = 2.0 ** -53


def _a(x, dt):
    return np.asarray(x).astype(dt)


def bf16_out(tol, ref):
    """Bound of a value stored as bf16: the fp32 bound, then one bf16 ulp of the (fp32-perturbed) value."""
    return tol * (1 + BF16) + BF16 * np.abs(ref)


# ---------------------------------------------------------------------------------------------
# mean fusion + reparameterisation
# ---------------------------------------------------------------------------------------------
def fuse_fwd(mu_terms, lv_terms, eps, dt):
    """mu = mean of the terms, logvar likewise, z = mu + eps exp(logvar / 2); terms: the [B][L] halves of every modality present
    (EncoderC's already gathered), in the kernel's order a, b, table."""
    n = len(mu_terms)
    mu, lv = _a(mu_terms[0], dt), _a(lv_terms[0], dt)
    for k in range(1, n):
        mu = mu + _a(mu_terms[k], dt)
        lv = lv + _a(lv_terms[k], dt)
    if n > 1:
        inv = dt(1) / dt(n)
        mu, lv = mu * inv, lv * inv
    z = mu + _a(eps, dt) * np.exp(dt(0.5) * lv)
    return mu, lv, z


def fuse_fwd_tol(mu_terms, lv_terms, eps):
    """mean: one term is a copy (0 + x is exact): bound 0.  n terms: n - 1 additions, 1 / n (one division: E_DIV), one multiply,
    all relative to sum |terms| / n.
    z: the error of mu; exp's argument 0.5 * lv (exact scaling) carries the error of lv, which exp turns into the RELATIVE error
    0.5 * tol_lv; expf itself E_EXP; eps * exp one rounding; the final addition one rounding of |mu| + |eps| std."""
    n = len(mu_terms)
    out = []
    for terms in (mu_terms, lv_terms):
        mag = sum(np.abs(_a(t, np.float64)) for t in terms)
        out.append(np.zeros_like(mag) if n == 1 else SECOND * ((n - 1) + 1) * U * mag / n + SECOND * E_DIV * mag / n)
    mu, lv, _ = fuse_fwd(mu_terms, lv_terms, eps, np.float64)
    es = np.abs(_a(eps, np.float64)) * np.exp(0.5 * lv)
    tol_z = SECOND * (out[0] + es * (0.5 * out[1] + E_EXP + U) + U * (np.abs(mu) + es))
    return out[0], out[1], tol_z


def fuse_bwd(g_mu, g_lv, dzs, eps, logvar, n_mod, dt):
    """d_mu = (g_mu + sum dz) / n ; d_logvar = (g_lv + sum dz * eps * exp(logvar / 2) / 2) / n   (g_* None = 0)."""
    dz = _a(dzs[0], dt)
    for d in dzs[1:]:
        dz = dz + _a(d, dt)
    gm = _a(g_mu, dt) if g_mu is not None else np.zeros_like(dz)
    gl = _a(g_lv, dt) if g_lv is not None else np.zeros_like(dz)
    dmu = gm + dz
    dlv = gl + dz * _a(eps, dt) * np.exp(dt(0.5) * _a(logvar, dt)) * dt(0.5)
    if n_mod > 1:
        inv = dt(1) / dt(n_mod)
        dmu, dlv = dmu * inv, dlv * inv
    return dmu, dlv


def fuse_bwd_tol(g_mu, g_lv, dzs, eps, logvar, n_mod):
    """k = number of dz operands, D = sum |dz_i|.
    d_mu: k - 1 additions of the dz, + g_mu one rounding: k U (|g_mu| + D); times 1 / n: E_DIV + U more when n > 1.
    d_logvar: the product P = D |eps| std / 2 carries (k - 1) U (the dz sum) + U (* eps) + E_EXP + U (* exp) + 0 (* 0.5 is exact);
    + g_lv one rounding of |g_lv| + P; times 1 / n as above."""
    k = len(dzs)
    D = sum(np.abs(_a(d, np.float64)) for d in dzs)
    gm = np.abs(_a(g_mu, np.float64)) if g_mu is not None else 0.0
    gl = np.abs(_a(g_lv, np.float64)) if g_lv is not None else 0.0
    inv_err = (E_DIV + U) if n_mod > 1 else 0.0
    P = D * np.abs(_a(eps, np.float64)) * np.exp(0.5 * _a(logvar, np.float64)) * 0.5
    tol_mu = SECOND * (k * U + inv_err) * (gm + D) / n_mod
    tol_lv = SECOND * (((k - 1) * U + 2 * U + E_EXP) * P + (U + inv_err) * (gl + P)) / n_mod
    return tol_mu, tol_lv


def scatter_tol(rows_ref, rows_tol, site, S):
    """d_table[s] = sum of the rows with site == s: the rows' own bounds add up, and the summation (LDS atomics per workgroup, global
    atomics per workgroup or per element, the sum over the scatter copies: count_s - 1 additions of non-zero values in some order)
    adds count_s U sum |rows|.  Labels outside [0, S) scatter nothing.  -> (reference [S][W], bound [S][W])"""
    W = rows_ref.shape[1]
    ref, tol, mag = np.zeros((S, W)), np.zeros((S, W)), np.zeros((S, W))
    ok = (site >= 0) & (site < S)
    np.add.at(ref, site[ok], rows_ref[ok])
    np.add.at(tol, site[ok], rows_tol[ok])
    np.add.at(mag, site[ok], np.abs(rows_ref[ok]) + rows_tol[ok])
    count = np.bincount(site[ok], minlength=S).astype(np.float64)[:, None]
    return ref, SECOND * (tol + count * U * mag)


# ---------------------------------------------------------------------------------------------
# EncoderC table
# ---------------------------------------------------------------------------------------------
def embed_fwd(emb, w_mu, b_mu, w_lv, b_lv, dt):
    """T[S][2L] = emb [S][E] x [w_mu; w_lv]^T + [b_mu; b_lv], accumulated from the bias over e ascending."""
    W, b = np.concatenate([_a(w_mu, dt), _a(w_lv, dt)], 0), np.concatenate([_a(b_mu, dt), _a(b_lv, dt)])
    emb = _a(emb, dt)
    acc = np.broadcast_to(b, (emb.shape[0], b.shape[0])).copy()
    for e in range(emb.shape[1]):
        acc = acc + emb[:, e, None] * W[None, :, e]
    return acc


def embed_fwd_tol(emb, w_mu, b_mu, w_lv, b_lv):
    """E products (one rounding each) and E additions onto the bias: (E + 1) U (|b| + |emb| |W|^T)."""
    W, b = np.abs(np.concatenate([w_mu, w_lv], 0)).astype(np.float64), np.abs(np.concatenate([b_mu, b_lv])).astype(np.float64)
    E = emb.shape[1]
    return SECOND * (E + 1) * U * (b[None, :] + np.abs(emb).astype(np.float64) @ W.T)


def embed_bwd(d_table_copies, emb, w_mu, w_lv, old, dt):
    """dT = sum of the copies; d_emb += dT x Wcat; d_Wcat += dT^T x emb; d_bcat += column sums of dT.  old = (d_emb, d_Wcat, d_bcat)."""
    dT = _a(d_table_copies[0], dt)
    for c in d_table_copies[1:]:
        dT = dT + _a(c, dt)
    W, emb = np.concatenate([_a(w_mu, dt), _a(w_lv, dt)], 0), _a(emb, dt)
    return _a(old[0], dt) + dT @ W, _a(old[1], dt) + dT.T @ emb, _a(old[2], dt) + dT.sum(0, dtype=dt)


def embed_bwd_tol(d_table_copies, emb, w_mu, w_lv, old):
    """A term |dT| |w| carries (c - 1) U from the sum of the c copies and U from its product; n of them are summed ((n - 1) U) and
    added to the old gradient (U): (c + n) U (|old| + A |B|) with A = sum_c |copy|; n = 2L for d_emb, S for d_Wcat and d_bcat."""
    A = sum(np.abs(_a(c, np.float64)) for c in d_table_copies)
    W, emb = np.abs(np.concatenate([w_mu, w_lv], 0)).astype(np.float64), np.abs(emb).astype(np.float64)
    c, S, L2 = len(d_table_copies), A.shape[0], A.shape[1]
    o = [np.abs(_a(x, np.float64)) for x in old]
    return (SECOND * (c + L2) * U * (o[0] + A @ W), SECOND * (c + S) * U * (o[1] + A.T @ emb), SECOND * (c + S) * U * (o[2] + A.sum(0)))


# ---------------------------------------------------------------------------------------------
# BatchNorm pieces
# ---------------------------------------------------------------------------------------------
def bn_finalize(s1, s2, M, gamma, beta, eps, momentum, rm, rv, dt):
    """From the f64 column sums: mean, biased variance (clamped at 0), rstd, scale = gamma rstd, shift = beta - mean scale, and the
    running statistics (momentum form, UNBIASED variance).  The kernel forms mean / var / rstd / the unbiased variance in f64 and
    rounds them to f32; the reference (dt = float64) forms the variance in extended precision so that the one-pass cancellation
    is the kernel's alone.  -> dict"""
    wide = np.longdouble if dt == np.float64 else np.float64
    mean = _a(s1, wide) / wide(M)
    var = np.maximum(_a(s2, wide) / wide(M) - mean * mean, wide(0))
    rstd = (wide(1) / np.sqrt(var + wide(np.float32(eps)))).astype(dt)
    meanf, unb = mean.astype(dt), (var * (wide(M) / wide(M - 1))).astype(dt)
    scale = _a(gamma, dt) * rstd
    out = dict(mean=meanf, rstd=rstd, scale=scale, shift=_a(beta, dt) - meanf * scale, var=var.astype(np.float64))
    if rm is not None:
        m = dt(np.float32(momentum))
        out["running_mean"] = (dt(1) - m) * _a(rm, dt) + m * meanf
        out["running_var"] = (dt(1) - m) * _a(rv, dt) + m * unb
    return out


def bn_finalize_tol(s1, s2, M, gamma, beta, eps, momentum, rm, rv, sums_rel=0.0):
    """var = s2 / M - mean^2 in f64: two divisions, a square and a subtraction: 4 * 2^-53 (s2 / M + mean^2) absolute -- small against
    eps except where the column has a large mean (the constant-column case) -- plus `sums_rel` (s2 / M + mean^2) when the reference
    was not computed from these sums (torch's batch_norm from the data: the sums carry M * 2^-53).
    rstd: 0.5 dvar / (var + eps) relative from the variance, U from the rounding to f32.  mean: U.  scale = gamma * rstd: + U.
    shift = beta - mean * scale: the product carries mean (U) + scale + U; the subtraction U (|beta| + |mean scale|).
    running = (1 - m) * old + m * new: 1 - m one rounding, two products, one addition, `new` rounded to f32:
    3 U (|(1 - m) old| + |m new|), and m * M / (M - 1) * dvar for the variance."""
    r = bn_finalize(s1, s2, M, gamma, beta, eps, momentum, rm, rv, np.float64)
    m2 = np.asarray(s2, np.float64) / M + r["mean"] ** 2
    dvar = (4 * F64 + sums_rel) * m2
    e_rstd = 0.5 * dvar / (r["var"] + float(np.float32(eps))) + U
    g, b = np.abs(_a(gamma, np.float64)), np.abs(_a(beta, np.float64))
    ms = np.abs(r["mean"] * r["scale"])
    tol = dict(mean=SECOND * (U + sums_rel) * np.abs(r["mean"]), rstd=SECOND * e_rstd * r["rstd"], scale=SECOND * (e_rstd + U) * g * r["rstd"],
               shift=SECOND * ((U + sums_rel + e_rstd + U + U) * ms + U * (b + ms)))
    if rm is not None:
        m = float(np.float32(momentum))
        tol["running_mean"] = SECOND * (3 * U + sums_rel) * (np.abs((1 - m) * _a(rm, np.float64)) + np.abs(m * r["mean"]))
        unb = r["var"] * M / (M - 1.0)
        tol["running_var"] = SECOND * (3 * U * (np.abs((1 - m) * _a(rv, np.float64)) + m * unb) + m * M / (M - 1.0) * dvar)
    return tol


def bn_eval(gamma, beta, rm, rv, eps, dt):
    """Eval mode: rstd = 1 / sqrt(running_var + eps), scale = gamma rstd, shift = beta - running_mean scale."""
    rstd = dt(1) / np.sqrt(_a(rv, dt) + dt(np.float32(eps)))
    scale = _a(gamma, dt) * rstd
    return dict(rstd=rstd, scale=scale, shift=_a(beta, dt) - _a(rm, dt) * scale, mean=_a(rm, dt))


def bn_eval_tol(gamma, beta, rm, rv, eps):
    """rstd: the addition U, halved by the square root; sqrtf E_SQRT; the division E_DIV.  scale: + U.  shift: product + U, then the
    subtraction U (|beta| + |rm scale|).  mean is a copy."""
    r = bn_eval(gamma, beta, rm, rv, eps, np.float64)
    e_rstd = 0.5 * U + E_SQRT + E_DIV
    ms = np.abs(r["mean"] * r["scale"])
    return dict(rstd=SECOND * e_rstd * r["rstd"], scale=SECOND * (e_rstd + U) * np.abs(r["scale"]),
                shift=SECOND * ((e_rstd + 2 * U) * ms + U * (np.abs(_a(beta, np.float64)) + ms)), mean=0.0 * ms)


def bn_bwd_coefs(sd, sdx, M, gamma, rstd, eval_mode, dt):
    """coef[3][N] = {gamma rstd, sum_d / M, sum_dx / M} (eval mode: {gamma rstd, 0, 0}); the divisions are f64, rounded once."""
    c0 = _a(gamma, dt) * _a(rstd, dt)
    z = np.zeros_like(c0)
    return np.stack([c0, z if eval_mode else (np.asarray(sd, np.float64) / M).astype(dt), z if eval_mode else (np.asarray(sdx, np.float64) / M).astype(dt)])


def bn_bwd_coefs_tol(sd, sdx, M, gamma, rstd, eval_mode):
    """One rounding each (the f64 division is exact to 2^-53)."""
    return SECOND * U * np.abs(bn_bwd_coefs(sd, sdx, M, gamma, rstd, eval_mode, np.float64))


def accum(old, s, dt):
    """old += (float) s for an f64 sum s (dgamma / dbeta)."""
    return _a(old, dt) + np.asarray(s, np.float64).astype(dt)


def accum_tol(old, s):
    """The conversion U |s| and the addition U (|old| + |s|)."""
    return SECOND * U * (np.abs(_a(old, np.float64)) + 2 * np.abs(np.asarray(s, np.float64)))


def bn_bwd_apply(d, y, mean, rstd, coef, dt):
    """dy = c0 (d - c1 - xhat c2), xhat = (y - mean) rstd."""
    xh = (_a(y, dt) - _a(mean, dt)) * _a(rstd, dt)
    c = _a(coef, dt)
    return c[0] * (_a(d, dt) - c[1] - xh * c[2])


def bn_bwd_apply_tol(d, y, mean, rstd, coef, coef_tol=0.0):
    """xhat: a subtraction of two exact inputs and a product: 2 U relative.  xhat * c2: + U.  d - c1: U (|d| + |c1|); - xhat c2:
    U (|d| + |c1| + |xhat c2|).  Times c0: U.  Relative to the magnitude T = |d| + |c1| + |xhat c2|:
    |c0| (2 U (|d| + |c1|) + 4 U |xhat c2|) + U |c0| T  <=  5 U |c0| T.
    coef_tol [3][N]: bounds of the coefficients themselves when the reference uses exact ones (the fused finalize + apply)."""
    c = _a(coef, np.float64)
    xh = np.abs((_a(y, np.float64) - _a(mean, np.float64)) * _a(rstd, np.float64))
    T = np.abs(_a(d, np.float64)) + np.abs(c[1]) + xh * np.abs(c[2])
    tol = 5 * U * np.abs(c[0]) * T
    if np.ndim(coef_tol):
        tol = tol + coef_tol[0] * T + np.abs(c[0]) * (coef_tol[1] + xh * coef_tol[2])
    return SECOND * tol


# ---------------------------------------------------------------------------------------------
# small element-wise launches
# ---------------------------------------------------------------------------------------------
def sigmoid_bwd(g, p, dt):
    """g * p * (1 - p)"""
    return _a(g, dt) * _a(p, dt) * (dt(1) - _a(p, dt))


def sigmoid_bwd_tol(g, p):
    """1 - p of an exact input: U; two products: 3 U |g p (1 - p)|."""
    return SECOND * 3 * U * np.abs(sigmoid_bwd(g, p, np.float64))


def scale_tol(x, s):
    """x * s: one rounding."""
    return SECOND * U * np.abs(_a(x, np.float64) * float(s))


def loss_finalize(sums, beta, gamma, dt):
    """{recon + gamma class + beta kld, recon, class, kld, bad labels}: f64 arithmetic on the f64 sums and the f32 hyper-parameters,
    one rounding to f32 each."""
    s = np.asarray(sums, np.float64)
    recon = s[0] + s[1]
    return np.array([recon + float(np.float32(gamma)) * s[2] + float(np.float32(beta)) * s[3], recon, s[2], s[3], s[4]]).astype(dt)


def loss_finalize_tol(sums, beta, gamma):
    """U of each value from the conversion; the f64 operations before it (at most five) 5 * 2^-53 of the sum of the terms."""
    s = np.abs(np.asarray(sums, np.float64))
    ref = np.abs(loss_finalize(sums, beta, gamma, np.float64))
    return SECOND * (U * ref + 5 * F64 * (s[0] + s[1] + abs(gamma) * s[2] + abs(beta) * s[3]))


# ---------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------
def adamw(p, g, m, v, t, lr, b1, b2, eps, wd, maximize, dt, device_bc=False):
    """One step at step count t (1-based) in `dt`, the kernel's expression: p *= 1 - lr wd ; m, v updated ;
    p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).  dt = float32: the bias corrections as the launch forms them -- rounded f32
    arguments (host form) or 1 - powf(b, t) in f32 (device_bc).  The float64 REFERENCE is oracle/np_oracle.adamw_step; this function
    in float64 is only used to show that it states the same formula."""
    lr, b1, b2, eps, wd = (dt(np.float32(x)) for x in (lr, b1, b2, eps, wd))
    g = -_a(g, dt) if maximize else _a(g, dt)
    if dt == np.float32 and device_bc:
        bc1 = dt(1) - np.power(b1, dt(t))
        rs = dt(1) / np.sqrt(dt(1) - np.power(b2, dt(t)))
    else:
        bc1 = dt(1.0 - float(b1) ** t)
        rs = dt(1) / np.sqrt(dt(1.0 - float(b2) ** t))
    pp = _a(p, dt) * (dt(1) - lr * wd)
    mm = b1 * _a(m, dt) + (dt(1) - b1) * g
    vv = b2 * _a(v, dt) + (dt(1) - b2) * g * g
    pp = pp - (lr / bc1) * mm / (np.sqrt(vv) * rs + eps)
    return pp, mm, vv


def adamw_tol(p, g, m, v, t, lr, b1, b2, eps, wd, maximize, device_bc):
    """m' = b1 m + (1 - b1) g: 1 - b1 one rounding, two products, one addition: 3 U (|b1 m| + |(1 - b1) g|) = dm.
    v' = b2 v + (1 - b2) g g: one more product: 4 U v' (all terms are positive) = dv.
    p * (1 - lr wd): lr wd and 1 - x are roundings of a factor next to 1 (2 U), the product U: 3 U |p|.
    Bias corrections, relative:
       host form    bc1, bc2 arrive rounded to f32: U each.
       device form  b^t from powf: E_POW relative to b^t, which is b^t / (1 - b^t) relative to 1 - b^t (499 at b2 = 0.999, t = 2:
                    4 U * 499 = 1.2e-4), and the subtraction U:  e_bc = E_POW b^t / (1 - b^t) + U.
       step = lr / bc1: e_bc1 in full + E_DIV.   rs = 1 / sqrtf(bc2): e_bc2 by HALF (square root) + E_SQRT + E_DIV.
    denom = sqrtf(v') rs + eps: sqrt(v') carries dv / (2 v') = 2 U and E_SQRT, the product e_rs + U, the addition U:
       e_den = 2 U + E_SQRT + e_rs + 2 U (relative to denom: eps > 0 only lowers the share of the first term).
    update = step * m' / denom: dm * step / denom absolute from m', and |update| (e_step + U + E_DIV + e_den).
    p' = p (1 - lr wd) - update: the subtraction U (|p| + |update|)."""
    f = lambda x: float(np.float32(x))
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    p, g, m, v = (_a(x, np.float64) for x in (p, g, m, v))
    g = -g if maximize else g                     # exact
    mm = b1 * m + (1 - b1) * g
    vv = b2 * v + (1 - b2) * g * g
    dm = 3 * U * (np.abs(b1 * m) + np.abs((1 - b1) * g))
    dv = 4 * U * vv
    if device_bc:
        e_bc1 = E_POW * b1 ** t / (1 - b1 ** t) + U
        e_bc2 = E_POW * b2 ** t / (1 - b2 ** t) + U
    else:
        e_bc1 = e_bc2 = U
    e_step = e_bc1 + E_DIV
    e_rs = 0.5 * e_bc2 + E_SQRT + E_DIV
    e_den = 2 * U + E_SQRT + e_rs + 2 * U
    step, denom = lr / (1 - b1 ** t), np.sqrt(vv) / np.sqrt(1 - b2 ** t) + eps
    upd = np.abs(step * mm / denom)
    d_upd = dm * step / denom + upd * (e_step + U + E_DIV + e_den)
    return SECOND * (3 * U * np.abs(p) + d_upd + U * (np.abs(p) + upd)), SECOND * dm, SECOND * dv
