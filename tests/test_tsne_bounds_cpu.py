"""The bounds of tests/tsne_bounds.py hold an fp32 emulation of the kernels' arithmetic in several summation orders and split counts, and
reject a dozen mistakes.  The emulation forms every value the way tsne.hip does (fused multiply-adds through float64 products rounded
once, a correctly rounded reciprocal, which lies inside v_rcp_f32's 1 ulp), up to the order of the sums."""
import functools

import numpy as np
import pytest
import torch

import tsne_bounds as TB
import tsne_ref as TR
from mmvae import tsne

f32, f64 = np.float32, np.float64


def fma(a, b, c):
    """fl32(a b + c) for fp32 a, b, c: the product of two fp32 values is exact in float64"""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def ssum(terms, order):
    """fp32 sum of (..., n) along the last axis: 'chain' ascending, 'reverse' descending, 'pairwise' numpy's blocked pairwise sum"""
    terms = terms.astype(f32)
    if order == "pairwise":
        return terms.sum(axis=-1, dtype=f32)
    if order == "reverse":
        terms = terms[..., ::-1]
    return np.cumsum(terms, axis=-1, dtype=f32)[..., -1] if terms.shape[-1] else np.zeros(terms.shape[:-1], f32)


# ---------------------------------------------------------------------------------------------------------------------------
# gradient
# ---------------------------------------------------------------------------------------------------------------------------
def emulate_gradient(Y, row_ptr, col, val, exaggeration, splits_used, order="chain", mistake=None):
    """(grad (N, 2), Z, kl, z_row) in fp32 as mmvae_tsne_gradient forms them.  mistake: None | 'diag_in_Z' | 'pad_columns' | 'w_for_w2' |
    'no_factor_4' | 'exaggerate_repulsion' | 'split_twice' | 'split_skipped'"""
    Y = np.asarray(Y, f32)
    N = Y.shape[0]
    Yc = Y
    if mistake == "pad_columns":                                                     # the columns up to the next multiple of 64, read as zeros
        Yc = np.vstack([Y, np.zeros((-N % 64 or 64, 2), f32)])
    dx, dy = Y[:, None, 0] - Yc[None, :, 0], Y[:, None, 1] - Yc[None, :, 1]
    q = fma(dy, dy, fma(dx, dx, np.ones_like(dx)))
    w = (f32(1) / q).astype(f32)
    if mistake != "diag_in_Z":
        w[np.arange(N), np.arange(N)] = 0
    w2 = w if mistake == "w_for_w2" else w * w
    L = TB.split_columns(N, splits_used)
    cuts = [(s * L, min((s + 1) * L, Yc.shape[0] if s == splits_used - 1 else N)) for s in range(splits_used)]
    parts = []
    for lo, hi in cuts:
        tx, ty = (w2[:, lo:hi].astype(f64) * dx[:, lo:hi]), (w2[:, lo:hi].astype(f64) * dy[:, lo:hi])
        if order == "chain":                                                         # the kernel's: one fused chain per split
            rx, ry, z = np.zeros(N, f32), np.zeros(N, f32), np.zeros(N, f32)
            for j in range(hi - lo):
                rx, ry, z = (rx + tx[:, j]).astype(f32), (ry + ty[:, j]).astype(f32), z + w[:, lo + j]
        else:
            rx, ry, z = ssum(tx, order), ssum(ty, order), ssum(w[:, lo:hi], order)
        parts.append((rx, ry, z))
    if mistake == "split_twice":
        parts.append(parts[0])
    if mistake == "split_skipped" and len(parts) > 1:
        parts = parts[:-1]
    rx, ry, zr = (ssum(np.stack([p[i] for p in parts], axis=1), "chain") for i in range(3))
    Z = f32(np.sum([p[2].astype(f64).sum() for p in parts]))
    lens = np.diff(row_ptr)
    rows = np.repeat(np.arange(N), lens)
    ex, ey = Y[rows, 0] - Y[col, 0], Y[rows, 1] - Y[col, 1]
    qe = fma(ey, ey, fma(ex, ex, np.ones_like(ex)))
    val = np.asarray(val, f32)
    pw = val * (f32(1) / qe).astype(f32)
    pos = val > 0
    lterm = np.zeros_like(val)
    lterm[pos] = ((np.log(val[pos]) + np.log(qe[pos])).astype(f32) + np.log(Z)).astype(f32)
    ax, ay, err = np.zeros(N, f32), np.zeros(N, f32), np.zeros(N, f32)
    for i in range(N):
        e = slice(row_ptr[i], row_ptr[i + 1])
        ax[i], ay[i] = ssum(pw[e].astype(f64) * ex[e], order), ssum(pw[e].astype(f64) * ey[e], order)
        err[i] = ssum(val[e].astype(f64) * lterm[e], order)
    x = f32(exaggeration)
    rep = (f32(1) if mistake != "exaggerate_repulsion" else x)
    c = f32(4) if mistake != "no_factor_4" else f32(1)
    grad = np.stack([c * (x * ax - rep * (rx / Z)), c * (x * ay - rep * (ry / Z))], axis=1).astype(f32)
    return grad, Z, float(err.astype(f64).sum()), zr


@functools.lru_cache(maxsize=None)
def case(N, scale):
    g = np.random.default_rng(N)
    X = g.standard_normal((N, 4)) + 2.0 * g.standard_normal((3, 4))[np.arange(N) % 3]
    r, c, v = TR.joint_probabilities(X, min(10.0, (N - 1) / 4.0))
    Y = (scale * g.standard_normal((N, 2))).astype(f32)
    return Y, r, c, v.astype(f32)


GRADIENT_CASES = [(2, 1.0), (65, 1e-4), (130, 1.0), (200, 50.0)]


@pytest.mark.parametrize("order", ["chain", "reverse", "pairwise"])
@pytest.mark.parametrize("N,scale", GRADIENT_CASES)
def test_emulation_stays_inside_every_gradient_bound(N, scale, order):
    Y, r, c, v = case(N, scale)
    for exaggeration in (1.0, 12.0):
        for used in sorted({TB.splits_used(N, want) for want in (1, 2, 3)}):
            b = TB.gradient_bounds(Y, r, c, v, exaggeration, used)
            got = emulate_gradient(Y, r, c, v, exaggeration, used, order)
            worst = TB.check_gradient(b, *got, label=(N, scale, order, exaggeration, used))
            assert worst["grad"] <= 1.0 and worst["Z"] <= 1.0 and worst["kl"] <= 1.0


GRADIENT_MISTAKES = ["diag_in_Z", "pad_columns", "w_for_w2", "no_factor_4", "exaggerate_repulsion", "split_twice", "split_skipped"]


@pytest.mark.parametrize("mistake", GRADIENT_MISTAKES)
def test_gradient_mistakes_fall_outside_a_bound(mistake):
    caught = []
    for N, scale in GRADIENT_CASES[1:]:
        Y, r, c, v = case(N, scale)
        for exaggeration in (1.0, 12.0):
            used = TB.splits_used(N, 3)
            b = TB.gradient_bounds(Y, r, c, v, exaggeration, used)
            assert not TB.gradient_outside(b, *emulate_gradient(Y, r, c, v, exaggeration, used))
            bad = TB.gradient_outside(b, *emulate_gradient(Y, r, c, v, exaggeration, used, mistake=mistake))
            if bad:
                caught.append((N, scale, exaggeration, bad))
    print(mistake, caught)
    assert caught, f"{mistake} passes every bound on every case"


# ---------------------------------------------------------------------------------------------------------------------------
# symmetrisation
# ---------------------------------------------------------------------------------------------------------------------------
def test_symmetrisation_mistakes_fall_outside_the_bound():
    """the stored value of a slot: one fp32 addition, the division by the float64 total, the rounding to fp32: 3 u relative"""
    g = np.random.default_rng(4)
    N, k = 57, 9
    idx = np.stack([g.permutation(np.delete(np.arange(N), i))[:k] for i in range(N)]).astype(np.int32)
    p = g.random((N, k)).astype(f32)
    p /= p.sum(axis=1, keepdims=True)
    p[5] *= f32(0.5)                                                                 # a row whose sum is not 1
    r, c, v = TR.symmetric_csr(idx, p)

    def outside(row_ptr, col, val):
        if len(val) != len(v) or not np.array_equal(col, c):
            return True
        return not (np.abs(np.asarray(val, f64) - v) <= 3 * TB.U * v).all()
    got = tsne.joint_probabilities(torch.from_numpy(idx), torch.from_numpy(p))
    assert not outside(*(t.numpy() for t in got))
    dense = np.zeros((N, N))
    dense[np.repeat(np.arange(N), k), idx.ravel()] = p.ravel()
    one_sided = (dense / dense.sum())[np.repeat(np.arange(N), np.diff(r)), c]         # P_cond / sum alone, over the same slots
    assert outside(r, c, one_sided.astype(f32))
    by_2n = (dense + dense.T)[np.repeat(np.arange(N), np.diff(r)), c] / (2.0 * N)
    assert outside(r, c, by_2n.astype(f32))


# ---------------------------------------------------------------------------------------------------------------------------
# affinities
# ---------------------------------------------------------------------------------------------------------------------------
def emulate_affinities(d2, perplexity, order="lanes", mistake=None):
    """(p (N, k), beta (N,), converged (N,)) in fp32 as mmvae_tsne_affinities forms them.  order: 'lanes' (64 strided chains and a butterfly),
    'chain', 'pairwise'.  mistake: None | 'perplexity_for_log'"""
    d = np.asarray(d2, f32)
    N, k = d.shape
    target = f32(perplexity) if mistake == "perplexity_for_log" else np.log(f32(perplexity))

    def total(t):
        if order != "lanes":
            return ssum(t, order)
        lanes = np.cumsum(np.concatenate([t, np.zeros(-len(t) % 64, f32)]).reshape(-1, 64), axis=0, dtype=f32)[-1]
        for dist in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[np.arange(64) ^ dist]
        return lanes[0]
    P, B, ok = np.empty((N, k), f32), np.empty(N, f32), np.zeros(N, bool)
    for i in range(N):
        x = d[i] - d[i].min()
        beta, lo, hi = f32(1), f32(-np.inf), f32(np.inf)
        for _ in range(100):
            e = np.exp(-(x * beta)).astype(f32)
            s, sd = total(e), total((x.astype(f64) * e).astype(f32))
            at, s_at = beta, s
            diff = (np.log(s) + beta * (sd / s)) - target
            if abs(diff) <= f32(1e-5):
                ok[i] = True
                break
            if diff > 0:
                lo = beta
                beta = beta * f32(2) if hi == np.inf else (beta + hi) * f32(0.5)
            else:
                hi = beta
                beta = beta * f32(0.5) if lo == -np.inf else (beta + lo) * f32(0.5)
        P[i], B[i] = np.exp(-(x * at)).astype(f32) / s_at, at
    return P, B, ok


def distances(N, k, scale, seed):
    g = np.random.default_rng(seed)
    d = np.sort(scale * (0.5 + g.random((N, k)) * 4.0), axis=1)
    d[0] = d[0, 0]
    if k > 1:
        d[1, 0] = d[1, 1] * 1e-3
    return d.astype(f32)


@pytest.mark.parametrize("order", ["lanes", "chain", "pairwise"])
@pytest.mark.parametrize("k,perplexity,scale", [(5, 2.5, 1.0), (91, 30.0, 1.0), (91, 45.5, 1e-6), (70, 20.0, 1e6)])
def test_emulated_affinities_stay_inside_their_bounds(k, perplexity, scale, order):
    d2 = distances(12, k, scale, k)
    p, beta, ok = emulate_affinities(d2, perplexity, order)
    ok64 = TR.binary_search(d2, perplexity)[2]
    assert ok64[1:].all() and not ok64[0] and ok[1:].all()
    b = TB.affinity_bounds(d2, beta, perplexity)
    assert (np.abs(p.astype(f64) - b["p"]) <= b["d_p"]).all()
    assert (np.abs(b["H"] - np.log(perplexity))[ok] <= b["h_tol"][ok]).all()
    assert b["h_tol"][ok].max() <= 2e-5                                              # the bound adds little to the search's own 1e-5


def test_perplexity_in_place_of_its_logarithm_falls_outside():
    d2 = distances(12, 91, 1.0, 91)
    p, beta, ok = emulate_affinities(d2, 30.0, mistake="perplexity_for_log")
    b = TB.affinity_bounds(d2, beta, 30.0)
    assert not (np.abs(b["H"] - np.log(30.0))[1:] <= b["h_tol"][1:]).any()


# ---------------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------------
def emulate_update(y, upd, gains, grad, momentum, lr, mistake=None):
    """mistake: None | 'gains_sign' | 'no_floor'"""
    y, upd, gains, grad = (np.asarray(v, f32) for v in (y, upd, gains, grad))
    inc = upd * grad < 0
    if mistake == "gains_sign":
        inc = ~inc
    gains = np.where(inc, gains + f32(0.2), gains * f32(0.8)).astype(f32)
    if mistake != "no_floor":
        gains = np.maximum(gains, f32(0.01))
    gg = grad * gains
    upd = fma(np.full_like(upd, momentum), upd, -(f32(lr) * gg))
    return y + upd, upd, gains, float(np.sqrt((gg.astype(f64) ** 2).sum()))


def update_inputs(seed=0, n=400):
    g = np.random.default_rng(seed)
    y = g.standard_normal((n, 2)).astype(f32)
    upd = (1e-2 * g.standard_normal((n, 2))).astype(f32)
    gains = (0.01 + 3.0 * g.random((n, 2)) ** 3).astype(f32)
    grad = (1e-4 * g.standard_normal((n, 2))).astype(f32)
    upd[g.random((n, 2)) < 0.2] = 0.0
    return y, upd, gains, grad


@pytest.mark.parametrize("momentum,lr", [(0.5, 1092.27), (0.8, 50.0)])
def test_emulated_update_stays_inside_and_its_mistakes_fall_outside(momentum, lr):
    y, upd, gains, grad = update_inputs()
    mf, lf = float(f32(momentum)), float(f32(lr))
    b = TB.update_bounds(y, upd, gains, grad, mf, lf)
    assert not b["exempt"].any()
    assert not TB.update_outside(b, *emulate_update(y, upd, gains, grad, mf, lf))
    assert "gains" in TB.update_outside(b, *emulate_update(y, upd, gains, grad, mf, lf, mistake="gains_sign"))
    assert (b["gains"] == 0.01).any(), "some gains must sit on the floor for its absence to show"
    assert "gains" in TB.update_outside(b, *emulate_update(y, upd, gains, grad, mf, lf, mistake="no_floor"))
