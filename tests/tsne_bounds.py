"""Derived bounds for mmvae_tsne_affinities / mmvae_tsne_gradient / mmvae_tsne_update (include/mmvae_hip.h), nothing tuned.
u = 2^-24 (fp32 unit roundoff), gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1: n roundings of
any nesting).  A quantity with a star is the float64 value of tests/tsne_ref.py on the fp32 inputs the kernel reads.  The device
library's expf and logf are documented at 1 ulp and budgeted at 2 ulp = 4 u relative (LIB); v_rcp_f32 is documented at 1 ulp = 2 u
relative (RCP); divisions and the fused multiply-add are correctly rounded.

Gradient.  dx = fl(x_i - x_j) carries one rounding.  q = fl(dy^2 + fl(dx^2 + 1)): the term dx^2 carries 2 (dx twice) + 2, dy^2 2 + 1, the
one 2: q = q* (1 + t), |t| <= gamma(4), q* = 1 + |y_i - y_j|^2.  w = rcp(q):
    |w - w*| <= REL_W w*,   REL_W = gamma(4) / (1 - gamma(4)) + RCP (1 + gamma(4) / (1 - gamma(4))) <= gamma(7).
  - R_i: a term fl(w w) dx entering a chain of fused multiply-adds carries 2 x 7 + 1 (w^2) + 1 (dx) = 16 roundings before the chain.  The
    chain of a split is its L columns (L <= 64 chunks_per_split) in ascending order, then the splits in ascending order (splits - 1):
        |R_i - R*_i| <= dR_i = gamma(16 + L + splits) sum_{j != i} w*^2 |y_i - y_j|      (per component; the diagonal adds exactly 0)
  - z_i likewise with 7 roundings per term:  |z_i - z*_i| <= gamma(7 + L + splits) z*_i.
  - Z: a workgroup's sum takes the z_i of a split (7 + L), the lane's two rows (1), the butterfly (6), the four waves (3); the workgroup
    sums are added in float64 (its 2^-53 roundings are covered by one more fp32 rounding) and Z is rounded to fp32 (1): all terms positive,
        |Z - Z*| <= REL_Z Z*,   REL_Z = gamma(L + 19).
  - A_i: a term fl(p w) dx carries 7 + 1 + 1 = 9 roundings before its lane's chain of ceil(len_i / 64) fused multiply-adds and the
    butterfly (6):   |A_i - A*_i| <= dA_i = gamma(15 + ceil(len_i / 64)) sum_j p_ij w*_ij |y_i - y_j|.
  - grad = fl(4 fl(fl(x A) - fl(R / Z))) (the 4 is exact; a contraction of x A into the subtraction only removes a rounding):
        |R / Z - R* / Z*| <= dRZ = (dR + |R*| rz) / Z* / (1 - REL_Z),  rz = REL_Z,  and three roundings on top:
        |grad - grad*| <= 4 (x dA + dRZ) (1 + gamma(3)) + gamma(3) 4 (x |A*| + |R*| / Z*).
  - err_i = sum_j p (fl(fl(logf p + logf q) + logf Z)): logf p within LIB |log p|; logf q within LIB |log q*| + gamma(4) / (1 - gamma(4))
    (its argument's error); logf Z within LIB |log Z*| + REL_Z / (1 - REL_Z); the two additions round once and twice:
        e_L = (LIB + 2 u) (|log p| + |log q*| + |log Z*|) (1 + LIB) + gamma(5) + 2 REL_Z
    (2 REL_Z >= REL_Z / (1 - REL_Z) (1 + 2 u) for REL_Z < 1 / 4), and a term p L enters its lane's chain (ceil(len_i / 64)) and the butterfly (6);
    the rows are added in float64:
        |KL - KL*| <= sum_ij p e_L (1 + gamma(len)) + gamma(7 + ceil(len_max / 64)) sum_ij p |L*|.
Affinities, at the returned beta (a fp32 value, taken exactly).  x_j = fl(d_j - m) and a_j = fl(x_j beta): a_j = a*_j (1 + t), |t| <= gamma(2);
e_j = expf(-a_j) = exp(-a*_j) (1 + eps_j),  1 + eps_j <= exp(a*_j gamma(2)) (1 + LIB) (and the mirror image below).  s = sum e_j in lane
chains of ceil(k / 64) and the butterfly (6): all terms positive,  1 + eps_s <= (1 + max-weighted eps) (1 + gamma(D)),  D = ceil(k / 64) + 6,
with the weighted mean of eps_j over e*_j.  p_j = fl(e_j / s):
        |p_j - p*_j| <= p*_j ((1 + eps_j) (1 + u) / (1 - eps_s) - 1) + 2^-126 / s*           (the last: an exponential flushed to zero)
  - H = fl(fl(logf s) + fl(beta fl(sd / s))), sd = the fused chain of x_j e_j (each term eps_j + u before the chain, D in it):
        dsd = sum x*_j e*_j ((1 + eps_j) (1 + gamma(D + 1)) - 1),   r* = sd* / s*
        |H - H*| <= dH = eps_s / (1 - eps_s) + LIB |log s*| + beta ((dsd + sd* eps_s / (1 - eps_s)) / s* (1 + gamma(2)) + gamma(2) r*)
                         + u (1 + LIB) (|log s*| + beta r*) (1 + gamma(3)) + dH-terms' second order, covered by the factor (1 + gamma(8)).
    The kernel stops on |fl(H - fl(log perplexity))| <= fl(1e-5), so at a converged row
        |H* - log perplexity| <= 1e-5 (1 + 2 u) + dH + (LIB + u) |log perplexity| + u.
Update, per element, the fp32 inputs taken exactly; momentum, learning rate and the constants 0.2, 0.8, 0.01 are rounded to fp32 (u each):
        |gains' - gains*'| <= dg = 2 u (|gains| + 0.2) (one rounding of the constant, one of the operation; the floor 0.01 within 0.01 u)
        |update' - update*'| <= du = (u |m update| + |lr grad| (dg + 3 u gains*')) (1 + gamma(4)) + u |update*'|
        |y' - y*'| <= du + u |y*'|.
  The branch reads the sign of fl(update grad): exact unless 0 < |update grad| < 2^-126, where the product may be flushed to zero; such
  elements are exempt from the comparison of gains (and of what follows from it).
  |gains grad|_2: a square carries 2 (dg / gains' + u) + 1, the butterfly 6, the waves 3, float64 then, the root and its rounding 1 + 1:
        relative bound  (max_e (dg / gains*' + u) + gamma(12) / 2) (1 + gamma(12)) + 2 u."""
import numpy as np

import tsne_ref as TR

U = 2.0 ** -24
LIB = 4.0 * U
RCP = 2.0 * U
TINY = 2.0 ** -126


def gamma(n):
    return n * U / (1.0 - n * U)


REL_Q = gamma(4) / (1.0 - gamma(4))
REL_W = REL_Q + RCP * (1.0 + REL_Q)
assert REL_W <= gamma(7)


def splits_used(N, want):
    """mmvae_tsne_gradient_splits for a forced count `want` >= 1"""
    chunks = -(-N // 64)
    want = min(want, 64, chunks)
    per = -(-chunks // want)
    return -(-chunks // per)


def split_columns(N, splits_used):
    """columns of the longest split: 64 ceil(ceil(N / 64) / splits_used), at most N"""
    chunks = -(-N // 64)
    return min(N, 64 * -(-chunks // splits_used))


# ---------------------------------------------------------------------------------------------------------------------------
# gradient
# ---------------------------------------------------------------------------------------------------------------------------
def gradient_bounds(Y, row_ptr, col, val, exaggeration, splits_used):
    """dict(ref = tsne_ref.gradient(...), d_grad (N, 2), d_Z, d_kl, d_z (N,), d_R (N, 2), d_A (N, 2))"""
    Y = np.asarray(Y, np.float64)
    val = np.asarray(val, np.float64)
    N = Y.shape[0]
    ref = TR.gradient(Y, row_ptr, col, val, exaggeration)
    L = split_columns(N, splits_used)
    diff = np.abs(Y[:, None, :] - Y[None, :, :])
    W = 1.0 / (1.0 + (diff ** 2).sum(axis=2))
    np.fill_diagonal(W, 0.0)
    d_R = gamma(16 + L + splits_used) * ((W * W)[:, :, None] * diff).sum(axis=1)
    d_z = gamma(7 + L + splits_used) * ref["z"]
    rel_Z = gamma(L + 19)
    lens = np.diff(row_ptr)
    rows = np.repeat(np.arange(N), lens)
    d = np.abs(Y[rows] - Y[col])
    q = 1.0 + (d ** 2).sum(axis=1)
    absA = np.zeros((N, 2))
    np.add.at(absA, rows, (val / q)[:, None] * d)
    d_A = gamma(15 + -(-lens // 64))[:, None] * absA
    Z = ref["Z"]
    d_RZ = (d_R + np.abs(ref["R"]) * rel_Z) / Z / (1.0 - rel_Z)
    d_grad = 4.0 * (exaggeration * d_A + d_RZ) * (1.0 + gamma(3)) + gamma(3) * 4.0 * (exaggeration * np.abs(ref["A"]) + np.abs(ref["R"]) / Z)
    pos = val > 0
    lp, lq, lZ = np.log(np.where(pos, val, 1.0)), np.log(q), np.log(Z)
    e_L = (LIB + 2.0 * U) * (np.abs(lp) + np.abs(lq) + abs(lZ)) * (1.0 + LIB) + gamma(5) + 2.0 * rel_Z
    lmax = int(lens.max()) if len(lens) else 0
    d_kl = float((val * e_L)[pos].sum() * (1.0 + gamma(max(lmax, 1))) + gamma(7 + -(-lmax // 64)) * (val * np.abs(lp + lq + lZ))[pos].sum())
    return dict(ref=ref, d_grad=d_grad, d_Z=rel_Z * Z, d_kl=d_kl, d_z=d_z, d_R=d_R, d_A=d_A)


def gradient_outside(b, grad, Z, kl, z_row=None):
    """names of the outputs that lie outside their bounds (a NaN lies outside)"""
    ref, bad = b["ref"], []
    if not (np.abs(np.asarray(grad, np.float64) - ref["grad"]) <= b["d_grad"]).all():
        bad.append("grad")
    if not abs(float(Z) - ref["Z"]) <= b["d_Z"]:
        bad.append("Z")
    if kl is not None and not abs(float(kl) - ref["kl"]) <= b["d_kl"]:
        bad.append("kl")
    if z_row is not None and not (np.abs(np.asarray(z_row, np.float64) - ref["z"]) <= b["d_z"]).all():
        bad.append("z_row")
    return bad


def check_gradient(b, grad, Z, kl, z_row=None, label=""):
    """asserts every output within its bound; returns the largest error relative to its bound, per output"""
    ref = b["ref"]
    eg = np.abs(np.asarray(grad, np.float64) - ref["grad"])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = dict(grad=float(np.nanmax(np.where(b["d_grad"] > 0, eg / b["d_grad"], 0.0))), Z=abs(float(Z) - ref["Z"]) / b["d_Z"],
                     kl=None if kl is None else abs(float(kl) - ref["kl"]) / b["d_kl"])
    bad = gradient_outside(b, grad, Z, kl, z_row)
    assert not bad, (label, bad, worst, np.argwhere(~(eg <= b["d_grad"]))[:5])
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# affinities
# ---------------------------------------------------------------------------------------------------------------------------
def affinity_bounds(d2, beta, perplexity):
    """at the returned beta (N,): dict(p, H: float64 at that beta, d_p (N, k), d_H (N,), h_tol (N,): bound on |H* - log perplexity| of a row
    the kernel's search converged on)"""
    d = np.asarray(d2, np.float64)
    beta = np.asarray(beta, np.float64)
    N, k = d.shape
    H, p = TR.entropy(d, beta)
    x = d - d.min(axis=1, keepdims=True)
    a = x * beta[:, None]
    e = np.exp(-a)
    s = e.sum(axis=1)
    D = -(-k // 64) + 6
    eps = np.exp(a * gamma(2)) * (1.0 + LIB) - 1.0
    eps_s = ((e * eps).sum(axis=1) / s + 1.0) * (1.0 + gamma(D)) - 1.0
    d_p = p * ((1.0 + eps) * (1.0 + U) / (1.0 - eps_s)[:, None] - 1.0) + (TINY / s)[:, None]
    sd = (x * e).sum(axis=1)
    dsd = (x * e * ((1.0 + eps) * (1.0 + gamma(D + 1)) - 1.0)).sum(axis=1)
    r = sd / s
    ls = np.abs(np.log(s))
    rs = eps_s / (1.0 - eps_s)
    d_H = (rs + LIB * ls + beta * ((dsd + sd * rs) / s * (1.0 + gamma(2)) + gamma(2) * r)
           + U * (1.0 + LIB) * (ls + beta * r) * (1.0 + gamma(3))) * (1.0 + gamma(8))
    lp = abs(np.log(perplexity))
    return dict(p=p, H=H, d_p=d_p, d_H=d_H, h_tol=TR.TOL * (1.0 + 2.0 * U) + d_H + (LIB + U) * lp + U)


# ---------------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------------
def update_bounds(y, upd, gains, grad, momentum, learning_rate):
    """dict(y, update, gains, norm: float64 step; d_y, d_update, d_gains (elementwise), rel_norm, exempt (bool): elements whose branch the
    kernel may take the other way)"""
    y, upd, gains, grad = (np.asarray(v, np.float64) for v in (y, upd, gains, grad))
    y1, u1, g1, norm = TR.update(y, upd, gains, grad, momentum, learning_rate)
    prod = np.abs(upd * grad)
    exempt = (prod > 0) & (prod < TINY)
    d_g = 2.0 * U * (np.abs(gains) + 0.2)
    d_u = (U * np.abs(momentum * upd) + np.abs(learning_rate * grad) * (d_g + 3.0 * U * g1)) * (1.0 + gamma(4)) + U * np.abs(u1)
    d_y = d_u + U * np.abs(y1)
    rel_norm = (float((d_g / g1 + U).max()) + gamma(12) / 2.0) * (1.0 + gamma(12)) + 2.0 * U
    return dict(y=y1, update=u1, gains=g1, norm=norm, d_y=d_y, d_update=d_u, d_gains=d_g, rel_norm=rel_norm, exempt=exempt)


def update_outside(b, y, upd, gains, norm=None):
    keep = ~b["exempt"]
    bad = []
    for name, got, tol in (("y", y, b["d_y"]), ("update", upd, b["d_update"]), ("gains", gains, b["d_gains"])):
        if not (np.abs(np.asarray(got, np.float64) - b[name]) <= tol)[keep].all():
            bad.append(name)
    if norm is not None and not b["exempt"].any() and not abs(float(norm) - b["norm"]) <= b["rel_norm"] * b["norm"]:
        bad.append("norm")
    return bad
