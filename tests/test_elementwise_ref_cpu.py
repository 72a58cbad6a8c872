"""Every derived bound of tests/elementwise_bounds.py holds for a float32 numpy restatement of its formula against the float64 one:
a bound that float32 arithmetic itself broke would be tighter than any kernel can be.  The bounds come from counting roundings
(see the module's header), so these checks are also the first place where a mis-counted one shows.  Inputs are drawn as the GPU
tests draw theirs (tests/test_elementwise_gpu.py); no GPU is needed.
"""
import numpy as np
import pytest

import np_oracle as O
import elementwise_bounds as E

F32, F64 = np.float32, np.float64


def rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(F32)


def inside(got, ref, tol, what):
    err = np.abs(np.asarray(got, F64) - np.asarray(ref, F64))
    tol = np.broadcast_to(np.asarray(tol, F64), err.shape)
    assert (err <= tol).all(), f"{what}: float32 restatement outside the bound: max err {err.max():.3e}, err/tol {np.max(err / np.maximum(tol, 1e-300)):.3f}"
    nz = tol > 0
    return float(np.max(err[nz] / tol[nz])) if nz.any() else 0.0


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("L", [4, 20, 128])
def test_fuse_fwd_bound(n, L):
    rng = np.random.default_rng(10 * n + L)
    B = 130
    mt, lt = [rnd(rng, B, L) for _ in range(n)], [rnd(rng, B, L, scale=0.7) for _ in range(n)]
    eps = rnd(rng, B, L)
    ref, got, tol = E.fuse_fwd(mt, lt, eps, F64), E.fuse_fwd(mt, lt, eps, F32), E.fuse_fwd_tol(mt, lt, eps)
    for k, name in enumerate(("mu", "logvar", "z")):
        assert got[k].dtype == F32
        inside(got[k], ref[k], tol[k], name)
    if n == 1:
        assert (tol[0] == 0).all() and (tol[1] == 0).all()          # one modality: mu / logvar are copies
    assert np.allclose(ref[2], O.reparameterize(ref[0], ref[1], eps.astype(F64)), rtol=1e-14, atol=0)


@pytest.mark.parametrize("n_mod", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("has_g", [True, False])
def test_fuse_bwd_bound(n_mod, k, has_g):
    rng = np.random.default_rng(100 * n_mod + 10 * k + has_g)
    B, L, S = 257, 20, 24
    dzs = [rnd(rng, B, L) for _ in range(k)]
    gm, gl = (rnd(rng, B, L), rnd(rng, B, L)) if has_g else (None, None)
    eps, lv = rnd(rng, B, L), rnd(rng, B, L, scale=0.7)
    ref, got, tol = E.fuse_bwd(gm, gl, dzs, eps, lv, n_mod, F64), E.fuse_bwd(gm, gl, dzs, eps, lv, n_mod, F32), E.fuse_bwd_tol(gm, gl, dzs, eps, lv, n_mod)
    inside(got[0], ref[0], tol[0], "d_mu"); inside(got[1], ref[1], tol[1], "d_logvar")
    # the scatter: float32 rows summed per label in float32, in row order
    site = rng.integers(0, S, B)
    rows32, rows64, rows_tol = np.concatenate(got, 1), np.concatenate(ref, 1), np.concatenate(tol, 1)
    tab32 = np.zeros((S, 2 * L), F32)
    np.add.at(tab32, site, rows32)
    tref, ttol = E.scatter_tol(rows64, rows_tol, site, S)
    inside(tab32, tref, ttol, "d_table")


@pytest.mark.parametrize("S,Ed,L", [(6, 8, 4), (24, 32, 20), (24, 32, 128), (5, 3, 7)])
def test_embed_table_bounds(S, Ed, L):
    rng = np.random.default_rng(S * 1000 + L)
    emb, wm, wl, bm, bl = rnd(rng, S, Ed), rnd(rng, L, Ed, scale=0.3), rnd(rng, L, Ed, scale=0.3), rnd(rng, L), rnd(rng, L)
    ref = E.embed_fwd(emb, wm, bm, wl, bl, F64)
    inside(E.embed_fwd(emb, wm, bm, wl, bl, F32), ref, E.embed_fwd_tol(emb, wm, bm, wl, bl), "table")
    P = {"encoder_c.embedding.weight": emb.astype(F64), "encoder_c.fc_mu.weight": wm.astype(F64), "encoder_c.fc_mu.bias": bm.astype(F64),
         "encoder_c.fc_logvar.weight": wl.astype(F64), "encoder_c.fc_logvar.bias": bl.astype(F64)}
    mu, lv, _ = O.encoder_c_fwd(P, np.arange(S))
    assert np.allclose(ref, np.concatenate([mu, lv], 1), rtol=1e-12, atol=1e-13)       # the same operation as the pinned oracle
    for copies in (1, 8, 11):
        dT = [rnd(rng, S, 2 * L) for _ in range(copies)]
        old = (rnd(rng, S, Ed), rnd(rng, 2 * L, Ed), rnd(rng, 2 * L))
        r, g, t = E.embed_bwd(dT, emb, wm, wl, old, F64), E.embed_bwd(dT, emb, wm, wl, old, F32), E.embed_bwd_tol(dT, emb, wm, wl, old)
        for k, name in enumerate(("d_emb", "d_W", "d_b")):
            assert g[k].dtype == F32
            inside(g[k], r[k], t[k], name)


@pytest.mark.parametrize("M", [2, 3, 1000])
@pytest.mark.parametrize("N", [1, 24, 257])
def test_bn_finalize_bounds(M, N):
    rng = np.random.default_rng(M * 7 + N)
    x = rng.standard_normal((M, N)) * rng.uniform(0.1, 3.0, N) + rng.uniform(-2, 2, N)
    x[:, 0] = 1000.0 + 1.0 / 3.0                                   # constant column with a large mean: the variance cancels
    s1, s2 = x.sum(0), (x * x).sum(0)
    gamma, beta, rm, rv = rnd(rng, N) + 1.5, rnd(rng, N), rnd(rng, N), (rng.uniform(0.5, 2, N)).astype(F32)
    args = (s1, s2, M, gamma, beta, 1e-5, 0.1, rm, rv)
    ref, got, tol = E.bn_finalize(*args, F64), E.bn_finalize(*args, F32), E.bn_finalize_tol(*args)
    for k in tol:
        assert got[k].dtype == F32
        inside(got[k], ref[k], tol[k], k)
    assert np.isfinite(got["rstd"]).all() and (got["rstd"] <= F32(1.0 / np.sqrt(np.float32(1e-5))) * (1 + 2 ** -23)).all()
    re, ge, te = E.bn_eval(gamma, beta, rm, rv, 1e-5, F64), E.bn_eval(gamma, beta, rm, rv, 1e-5, F32), E.bn_eval_tol(gamma, beta, rm, rv, 1e-5)
    for k in te:
        inside(ge[k], re[k], te[k], "eval " + k)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("eval_mode", [False, True])
def test_bn_bwd_bounds(dtype, eval_mode):
    rng = np.random.default_rng(5 + eval_mode)
    M, N = 133, 64
    d, y = rnd(rng, M, N), rnd(rng, M, N, scale=2.0)
    if dtype == "bf16":
        d, y = O.bf16_round(d).astype(F32), O.bf16_round(y).astype(F32)
    mean, rstd, gamma = rnd(rng, N), rng.uniform(0.3, 3, N).astype(F32), rnd(rng, N) + 1.5
    xh = (y.astype(F64) - mean) * rstd
    sd, sdx = d.astype(F64).sum(0), (d * xh).sum(0)
    old_g, old_b = rnd(rng, N), rnd(rng, N)
    inside(E.accum(old_g, sdx, F32), E.accum(old_g, sdx, F64), E.accum_tol(old_g, sdx), "dgamma")
    inside(E.accum(old_b, sd, F32), E.accum(old_b, sd, F64), E.accum_tol(old_b, sd), "dbeta")
    c64, c32 = E.bn_bwd_coefs(sd, sdx, M, gamma, rstd, eval_mode, F64), E.bn_bwd_coefs(sd, sdx, M, gamma, rstd, eval_mode, F32)
    ctol = E.bn_bwd_coefs_tol(sd, sdx, M, gamma, rstd, eval_mode)
    inside(c32, c64, ctol, "coef")
    # apply with the kernel's own (float32) coefficients as exact inputs, and the fused form against exact coefficients
    got = E.bn_bwd_apply(d, y, mean, rstd, c32, F32)
    inside(got, E.bn_bwd_apply(d, y, mean, rstd, c32, F64), E.bn_bwd_apply_tol(d, y, mean, rstd, c32), "apply")
    ref = E.bn_bwd_apply(d, y, mean, rstd, c64, F64)
    tol = E.bn_bwd_apply_tol(d, y, mean, rstd, c64, ctol)
    inside(got, ref, tol, "finalize + apply")
    if dtype == "bf16":
        inside(O.bf16_round(got), ref, E.bf16_out(tol, ref), "bf16 output")
    # the oracle's BatchNorm backward is this formula (training mode): dy = gamma rstd (d - dbeta / B - xhat dgamma / B)
    if not eval_mode:
        c = dict(keep=np.ones_like(xh), yh=np.ones_like(xh), xhat=xh, gamma=gamma.astype(F64), rstd=rstd.astype(F64))
        dy, dg, db = O._bn_relu_drop_bwd(d.astype(F64), c)
        assert np.allclose(dy, ref, rtol=1e-11, atol=1e-12) and np.allclose(dg, sdx) and np.allclose(db, sd)


def test_small_elementwise_bounds():
    rng = np.random.default_rng(3)
    g, p = rnd(rng, 37, 45), rng.uniform(0, 1, (37, 45)).astype(F32)
    p[0, :4] = [0.0, 1.0, 1e-7, 1 - 2 ** -24]
    ref, got, tol = E.sigmoid_bwd(g, p, F64), E.sigmoid_bwd(g, p, F32), E.sigmoid_bwd_tol(g, p)
    inside(got, ref, tol, "sigmoid_bwd")
    inside(O.bf16_round(got), ref, E.bf16_out(tol, ref), "sigmoid_bwd bf16")
    x, s = rnd(rng, 1000), F32(0.3712)
    inside(x * s, x.astype(F64) * float(s), E.scale_tol(x, s), "scale")
    xb = O.bf16_round(x).astype(F32)
    inside(O.bf16_round(xb * s), xb.astype(F64) * float(s), E.bf16_out(E.scale_tol(xb, s), xb.astype(F64) * float(s)), "scale bf16")
    sums = np.array([1234.5678, 987.654321, 3.14159, 42.4242, 2.0])
    inside(E.loss_finalize(sums, 1e-3, 0.7, F32), E.loss_finalize(sums, 1e-3, 0.7, F64), E.loss_finalize_tol(sums, 1e-3, 0.7), "loss_finalize")


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("device_bc", [False, True])
@pytest.mark.parametrize("wd,maximize", [(0.0, False), (1e-2, True)])
def test_adamw_bound(t, device_bc, wd, maximize):
    rng = np.random.default_rng(t + device_bc)
    n = 1 << 20
    p, g, m, v = rnd(rng, n), rnd(rng, n, scale=0.1), rnd(rng, n, scale=0.05), (rng.uniform(0, 1e-2, n)).astype(F32)
    g[:5] = 0.0; v[:3] = 0.0; m[:5] = F32(1e-6)   # sqrt(v') = 0: the update is bounded by eps alone
    g[n // 2:] *= 1e-3; m[n // 2:] *= 1e-3; v[n // 2:] *= 1e-6      # sqrt(v') of the order of eps
    hp = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-8, wd=wd)
    got = E.adamw(p, g, m, v, t, maximize=maximize, dt=F32, device_bc=device_bc, **hp)
    # the reference: oracle/np_oracle.adamw_step in float64 on the float32-rounded hyper-parameters
    f = lambda x: float(np.float32(x))
    P, st = {"w": p.astype(F64)}, {"w": dict(m=m.astype(F64), v=v.astype(F64))}
    O.adamw_step(P, {"w": (-g if maximize else g).astype(F64)}, st, t - 1, lr=f(hp["lr"]), wd=f(wd), b1=f(0.9), b2=f(0.999), eps=f(1e-8))
    ref = (P["w"], st["w"]["m"], st["w"]["v"])
    mine = E.adamw(p, g, m, v, t, maximize=maximize, dt=F64, **hp)
    tol = E.adamw_tol(p, g, m, v, t, maximize=maximize, device_bc=device_bc, **hp)
    for k, name in enumerate("pmv"):
        assert np.allclose(mine[k], ref[k], rtol=1e-12, atol=1e-300), name          # the same formula as the oracle
        assert got[k].dtype == F32
        inside(got[k], ref[k], tol[k], name)
