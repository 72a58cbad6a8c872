"""Formulas and DERIVED per-element error bounds of the site classifier's kernels (csrc/classifier.hip and mmvae_adam_step), in the
manner of tests/elementwise_bounds.py and with its model of one float32 operation (U, ULP, E_EXP, E_POW, E_DIV, E_SQRT, SECOND; sums of
n terms in any order: (n - 1) U sum |terms|; a contracted multiply-add drops a rounding, the bounds count the uncontracted ones).
E_LOG, logf: 2 ulp, the same ASSUMPTION as E_EXP.  Errors are relative to the magnitude of the terms, nothing is fitted to kernel output.

Every formula takes `dt` (np.float64: the reference, np.float32: the emulation that tests/test_downstream_bounds_cpu.py shows to stay
inside the bound) and `wrong`: the name of one plausible mistake, which the same test shows to leave the bound.  The inputs are float32
values and count as exact; mean and rstd of the backward are inputs (the forward's fp32 outputs)."""
import numpy as np

from elementwise_bounds import E_DIV, E_EXP, E_POW, E_SQRT, SECOND, U, ULP

E_LOG = 2 * ULP


def _a(x, dt):
    return np.asarray(x).astype(dt)


def _inv_keep(p, dt):
    return dt(np.float32(1.0 / (1.0 - p))) if dt == np.float32 else dt(1.0 / (1.0 - p))


# ---------------------------------------------------------------------------------------------
# LayerNorm + ReLU + Dropout
# ---------------------------------------------------------------------------------------------
def ln_fwd(z, gamma, beta, keep, p, eps, dt, wrong=None):
    """-> (y, mean, rstd).  gamma None: y = relu(z) keep / (1 - p)."""
    z = _a(z, dt)
    N = z.shape[1]
    k = dt(1) if keep is None else _a(keep, dt) * _inv_keep(p, dt)
    if wrong == "scale_twice" and keep is not None:
        k = k * _inv_keep(p, dt)
    if gamma is None:
        return np.maximum(z, dt(0)) * k, None, None
    mean = z.sum(axis=1, dtype=dt) / dt(N)
    d = z - mean[:, None]
    var = (d * d).sum(axis=1, dtype=dt) / dt(N - 1 if wrong == "unbiased" else N)
    rstd = dt(1) / (np.sqrt(var) + dt(eps)) if wrong == "eps_outside" else dt(1) / np.sqrt(var + dt(eps))
    pre = d * rstd[:, None] * _a(gamma, dt) + _a(beta, dt)
    return np.maximum(pre, dt(0)) * k, mean, rstd


def ln_fwd_tol(z, gamma, beta, keep, p, eps):
    """mean: N - 1 additions, one division.  d = z - mean: the error of mean and one rounding of |z| + |mean|.  var: d^2 carries
    2 |d| dd and one rounding, N - 1 additions, one division.  rstd = 1 / sqrt(var + eps): the argument's error by half, E_SQRT, E_DIV.
    xhat = d rstd, pre = xhat gamma + beta: the errors carried and one rounding per operation.  y = relu(pre) k: k = fl(1 / (1 - p)) one
    rounding, the product one; where |pre| is below its own bound the gate may fall either way and the error is |pre| k, which the
    carried term dpre k covers.  A dropped element is exactly 0.  -> (tol_y, tol_mean, tol_rstd)"""
    z = _a(z, np.float64)
    N = z.shape[1]
    kk = 1.0 if keep is None else _a(keep, np.float64) / (1.0 - p)
    if gamma is None:
        return 2 * U * np.maximum(z, 0) * kk, None, None
    gamma, beta = _a(gamma, np.float64), _a(beta, np.float64)
    mean = z.mean(axis=1)
    t_mean = SECOND * ((N - 1) * U * np.abs(z).sum(axis=1) / N + E_DIV * np.abs(mean))
    d = z - mean[:, None]
    dd = t_mean[:, None] + U * (np.abs(z) + np.abs(mean)[:, None])
    var = (d * d).mean(axis=1)
    t_var = ((2 * np.abs(d) * dd + U * d * d).sum(axis=1) + (N - 1) * U * (d * d).sum(axis=1)) / N + E_DIV * var
    a = var + eps
    rstd = 1 / np.sqrt(a)
    t_rstd = SECOND * rstd * (0.5 * (t_var + U * a) / a + E_SQRT + E_DIV)
    xhat = d * rstd[:, None]
    dx = dd * rstd[:, None] + np.abs(d) * t_rstd[:, None] + U * np.abs(xhat)
    pre = xhat * gamma + beta
    dpre = dx * np.abs(gamma) + U * np.abs(xhat * gamma) + U * (np.abs(xhat * gamma) + np.abs(beta))
    t_y = SECOND * kk * (dpre * (1 + 2 * U) + 2 * U * np.maximum(pre, 0))
    return t_y, t_mean, t_rstd


def ln_bwd(dy, z, mean, rstd, gamma, beta, keep, p, dt, wrong=None):
    """-> (dz, dgamma, dbeta) from the forward's operands; mean, rstd: the forward's fp32 outputs (inputs here)"""
    dy, z = _a(dy, dt), _a(z, dt)
    N = z.shape[1]
    k = dt(1) if keep is None else _a(keep, dt) * _inv_keep(p, dt)
    if wrong == "no_scale_bwd" and keep is not None:
        k = _a(keep, dt)
    if wrong == "scale_twice" and keep is not None:
        k = k * _inv_keep(p, dt)
    if gamma is None:
        return np.where(z > 0, dy * k, dt(0)), None, None
    gamma, beta = _a(gamma, dt), _a(beta, dt)
    xhat = (z - _a(mean, dt)[:, None]) * _a(rstd, dt)[:, None]
    gate = xhat > 0 if wrong == "gate_xhat" else xhat * gamma + beta > 0
    g = np.where(gate, dy * k, dt(0))
    gg = g * gamma
    s1 = gg.sum(axis=1, dtype=dt) * (dt(1) / dt(N))
    s2 = (gg * xhat).sum(axis=1, dtype=dt) * (dt(1) / dt(N))
    third = dt(0) if wrong == "drop_term" else xhat * s2[:, None]
    dz = (gg - s1[:, None] - third) * _a(rstd, dt)[:, None]
    return dz, (g * xhat).sum(axis=0, dtype=dt), g.sum(axis=0, dtype=dt)


def ln_bwd_tol(dy, z, mean, rstd, gamma, beta, keep, p):
    """xhat = (z - mean) rstd: two roundings.  pre as in the forward.  g = dy k [pre > 0]: two roundings (k, the product); where |pre| is
    below its bound the gate may fall either way: the whole |dy k| joins the bound of g there.  gg = g gamma one rounding more.
    s1 = sum gg / N, s2 = sum gg xhat / N: the terms' errors, N - 1 additions, 1 / N (E_DIV) and a product.  dz = rstd (gg - s1 - xhat s2):
    the errors carried, two subtractions and the product relative to |gg| + |s1| + |xhat s2|.  dgamma, dbeta: the terms' errors and
    M - 1 additions.  -> (tol_dz, tol_dgamma, tol_dbeta)"""
    dy, z = _a(dy, np.float64), _a(z, np.float64)
    M, N = z.shape
    kk = 1.0 if keep is None else _a(keep, np.float64) / (1.0 - p)
    if gamma is None:
        return 2 * U * np.abs(dy * kk), None, None
    gamma, beta, mean, rstd = (_a(x, np.float64) for x in (gamma, beta, mean, rstd))
    xhat = (z - mean[:, None]) * rstd[:, None]
    dx = U * (np.abs(z) + np.abs(mean)[:, None]) * rstd[:, None] + U * np.abs(xhat)
    pre = xhat * gamma + beta
    dpre = dx * np.abs(gamma) + U * np.abs(xhat * gamma) + U * (np.abs(xhat * gamma) + np.abs(beta))
    g = np.where(pre > 0, dy * kk, 0.0)
    dg = 2 * U * np.abs(g) + np.where(np.abs(pre) <= SECOND * dpre, np.abs(dy * kk), 0.0)
    gg = g * gamma
    dgg = dg * np.abs(gamma) + U * np.abs(gg)
    inv = E_DIV + U
    s1, s2 = gg.mean(axis=1), (gg * xhat).mean(axis=1)
    ds1 = (dgg.sum(axis=1) + (N - 1) * U * np.abs(gg).sum(axis=1)) / N + inv * np.abs(gg).sum(axis=1) / N
    t = gg * xhat
    dt_ = dgg * np.abs(xhat) + np.abs(gg) * dx + U * np.abs(t)
    ds2 = (dt_.sum(axis=1) + (N - 1) * U * np.abs(t).sum(axis=1)) / N + inv * np.abs(t).sum(axis=1) / N
    c = xhat * s2[:, None]
    dc = dx * np.abs(s2)[:, None] + np.abs(xhat) * ds2[:, None] + U * np.abs(c)
    mag = np.abs(gg) + np.abs(s1)[:, None] + np.abs(c)
    t_dz = SECOND * rstd[:, None] * (dgg + ds1[:, None] + dc + 3 * U * mag)
    gx = g * xhat
    dgx = dg * np.abs(xhat) + np.abs(g) * dx + U * np.abs(gx)
    t_dgamma = SECOND * (dgx.sum(axis=0) + (M - 1) * U * np.abs(gx).sum(axis=0))
    t_dbeta = SECOND * (dg.sum(axis=0) + (M - 1) * U * np.abs(g).sum(axis=0))
    return t_dz, t_dgamma, t_dbeta


# ---------------------------------------------------------------------------------------------
# mean-reduced weighted cross-entropy
# ---------------------------------------------------------------------------------------------
def wce(logits, labels, w, dt, wrong=None):
    """-> dict(sum_wnll, sum_w (float64 sums of the dt row terms), nll, g, pred, confusion)"""
    x = _a(logits, dt)
    M, C = x.shape
    y = np.asarray(labels, np.int64)
    w = np.ones(C, dt) if w is None else _a(w, dt)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    se = e.sum(axis=1, keepdims=True, dtype=dt)
    nll = (m + np.log(se))[:, 0] - x[np.arange(M), y]
    wy = w[y]
    total = dt(M) if wrong == "div_M" else dt(wy.astype(np.float64).sum())
    onehot = np.zeros((M, C), dt)
    onehot[np.arange(M), y] = 1
    gw = np.ones(M, dt) if wrong == "no_weight_grad" else wy
    g = gw[:, None] * (e / se - onehot) / total
    pred = C - 1 - x[:, ::-1].argmax(axis=1) if wrong == "last_max" else x.argmax(axis=1)
    confusion = np.zeros((C, C), np.int64)
    np.add.at(confusion, (pred, y) if wrong == "transposed" else (y, pred), 1)
    return dict(sum_wnll=(wy.astype(np.float64) * nll.astype(np.float64)).sum(), sum_w=wy.astype(np.float64).sum(), nll=nll, g=g, pred=pred,
                confusion=confusion)


def wce_tol(logits, labels, w):
    """e = exp(x - m): the subtraction's rounding U |x - m| becomes a relative error of e, expf E_EXP.  se: the terms' errors and C - 1
    additions.  log se: dse / se and E_LOG |log se|.  nll = (m + log se) - x_y: two roundings of the terms.  sum w nll (float64): the
    rows' bounds times w.  softmax = e / se: de / e + dse / se + E_DIV.  g = w (softmax - onehot) / W: the subtraction, the product,
    W = fl(float64 sum) and the division.  pred and confusion are exact.  -> (tol_nll, tol_sum_wnll, tol_g)"""
    x = _a(logits, np.float64)
    M, C = x.shape
    y = np.asarray(labels, np.int64)
    w = np.ones(C) if w is None else _a(w, np.float64)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    de = e * (U * np.abs(x - m) + E_EXP)
    se = e.sum(axis=1, keepdims=True)
    dse = de.sum(axis=1, keepdims=True) + (C - 1) * U * se
    lse = np.log(se)
    dl = dse / se + E_LOG * np.abs(lse)
    xy = x[np.arange(M), y]
    t_nll = SECOND * (dl[:, 0] + U * (np.abs(m) + np.abs(lse))[:, 0] + U * ((np.abs(m) + np.abs(lse))[:, 0] + np.abs(xy)))
    wy = w[y]
    soft = e / se
    dsoft = soft * (de / e + dse / se + E_DIV)
    onehot = np.zeros((M, C))
    onehot[np.arange(M), y] = 1
    diff = soft - onehot
    W = wy.sum()
    t_g = SECOND * wy[:, None] / W * (dsoft + U * np.abs(diff) + np.abs(diff) * (2 * U + E_DIV))
    return t_nll, SECOND * (wy * t_nll).sum(), t_g


# ---------------------------------------------------------------------------------------------
# Adam with coupled decay
# ---------------------------------------------------------------------------------------------
def adam(p, g, m, v, t, lr, b1, b2, eps, wd, dt, device_bc=True, wrong=None):
    """One step at step count t (1-based): g' = g + wd p ; m, v ; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), the kernel's expression.
    dt = float32: the bias corrections as the launch forms them (device_bc: 1 - powf(b, t) in fp32; else rounded host values)."""
    lr, b1, b2, eps, wd = (dt(np.float32(x)) for x in (lr, b1, b2, eps, wd))
    p, g = _a(p, dt), _a(g, dt)
    if dt == np.float32 and device_bc:
        bc1 = dt(1) - np.power(b1, dt(t))
        rs = dt(1) / np.sqrt(dt(1) - np.power(b2, dt(t)))
    else:
        bc1 = dt(1.0 - float(b1) ** t)
        rs = dt(1) / np.sqrt(dt(1.0 - float(b2) ** t))
    pp = p
    if wrong == "decoupled":
        pp = p * (dt(1) - lr * wd)
    else:
        g = g + wd * p
    mm = b1 * _a(m, dt) + (dt(1) - b1) * g
    vv = b2 * _a(v, dt) + (dt(1) - b2) * g * g
    denom = (np.sqrt(vv) + eps) * rs if wrong == "bc2_inside" else np.sqrt(vv) * rs + eps
    return pp - (lr / bc1) * mm / denom, mm, vv


def adam_tol(p, g, m, v, t, lr, b1, b2, eps, wd, device_bc=True):
    """g' = g + wd p: a product and an addition, dg = 2 U (|g| + |wd p|).  From there tests/elementwise_bounds.adamw_tol's chain with dg
    carried: m' = b1 m + (1 - b1) g': 3 U of the terms and (1 - b1) dg.  v' = b2 v + (1 - b2) g'^2: 4 U v' and (1 - b2) 2 |g'| dg.
    denom = sqrt(v') rs + eps: sqrt carries dv / (2 sqrt v') ABSOLUTE (v' may be tiny next to eps, so not taken relative) and E_SQRT,
    rs = 1 / sqrt(bc2) its own e_rs, the product and the addition a rounding each.  update = step m' / denom; p' = p - update: one
    rounding of |p| + |update|.  -> (tol_p, tol_m, tol_v)"""
    f = lambda x: float(np.float32(x))
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    p, g, m, v = (_a(x, np.float64) for x in (p, g, m, v))
    dg = 2 * U * (np.abs(g) + np.abs(wd * p))
    g = g + wd * p
    mm = b1 * m + (1 - b1) * g
    vv = b2 * v + (1 - b2) * g * g
    dm = 3 * U * (np.abs(b1 * m) + np.abs((1 - b1) * g)) + (1 - b1) * dg
    dv = 4 * U * vv + (1 - b2) * 2 * np.abs(g) * dg
    if device_bc:
        e_bc1 = E_POW * b1 ** t / (1 - b1 ** t) + U
        e_bc2 = E_POW * b2 ** t / (1 - b2 ** t) + U
    else:
        e_bc1 = e_bc2 = U
    e_step = e_bc1 + E_DIV
    e_rs = 0.5 * e_bc2 + E_SQRT + E_DIV
    rs = 1 / np.sqrt(1 - b2 ** t)
    root = np.sqrt(vv)
    d_root = np.where(vv > 0, dv / (2 * np.maximum(root, 1e-300)), np.sqrt(dv)) + E_SQRT * root
    denom = root * rs + eps
    d_den = d_root * rs + root * rs * (e_rs + U) + U * denom
    step = lr / (1 - b1 ** t)
    upd = np.abs(step * mm / denom)
    d_upd = dm * step / denom + upd * (e_step + U + E_DIV + d_den / denom)
    return SECOND * (d_upd + U * (np.abs(p) + upd)), SECOND * dm, SECOND * dv
