"""tests/ae_bounds.py on the CPU: the float32 restatement of the autoencoders' latent-path kernels stays inside the bounds the GPU tests
hold the kernels to around float64, and a handful of planted mistakes -- division by n_mod + 1, the table row skipped, the mean applied
twice, the bias missing, the wrong head column, z pads not zero -- do not.  The mean is held bit-equal: there a mistake only has to
change a bit.  The fused latent launch (head GEMM, mean, bf16 z, the decoder's first layer) is restated as a whole too."""
import numpy as np
import pytest

import ae_bounds as AB
import elementwise_bounds as E

F32, F64 = np.float32, np.float64


def rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(F32)


def outside(got, ref, tol):
    return bool((np.abs(np.asarray(got, F64) - np.asarray(ref, F64)) > tol).any())


@pytest.mark.parametrize("S,Ed,Ld", [(24, 32, 20), (5, 16, 7), (1, 32, 1)])
def test_projected_table_float32_is_inside_and_mistakes_are_not(S, Ed, Ld):
    rng = np.random.default_rng(S + Ld)
    emb, w, b = rnd(rng, S, Ed), rnd(rng, Ld, Ed, scale=0.3), rnd(rng, Ld, scale=0.5)
    ref, tol = AB.proj_fwd(emb, w, b, F64), AB.proj_fwd_tol(emb, w, b)
    assert np.allclose(ref, emb.astype(F64) @ w.astype(F64).T + b, rtol=1e-12, atol=1e-13)
    assert not outside(AB.proj_fwd(emb, w, b, F32), ref, tol)
    assert outside(AB.proj_fwd(emb, w, b, F32, mistake="no_bias"), ref, tol)
    if Ld > 1:
        assert outside(AB.proj_fwd(emb, w, b, F32, mistake="wrong_column"), ref, tol)
    for copies in (1, 8, 11):
        dT = [rnd(rng, S, Ld) for _ in range(copies)]
        old = (rnd(rng, S, Ed), rnd(rng, Ld, Ed), rnd(rng, Ld))
        r64, r32, tols = AB.proj_bwd(dT, emb, w, old, F64), AB.proj_bwd(dT, emb, w, old, F32), AB.proj_bwd_tol(dT, emb, w, old)
        for got, want, tl in zip(r32, r64, tols):
            assert not outside(got, want, tl)
        fresh = AB.proj_bwd(dT, emb, w, tuple(np.zeros_like(o) for o in old), F32)          # a backward that overwrites instead of accumulating
        assert all(outside(got, want, tl) for got, want, tl in zip(fresh, r64, tols))
        if copies > 1:
            assert all(outside(got, want, tl) for got, want, tl in zip(AB.proj_bwd(dT[:-1], emb, w, old, F32), r64, tols))     # a copy left out


@pytest.mark.parametrize("subset", [("head",), ("head", "site"), ("site",)])
@pytest.mark.parametrize("Ld", [4, 20, 128])
def test_mean_forward_is_exact_and_mistakes_change_it(Ld, subset):
    rng = np.random.default_rng(Ld + len(subset))
    B, S, ldz = 37, 24, Ld + 4
    head = rnd(rng, B, Ld + 5, scale=0.8) if "head" in subset else None
    table = rnd(rng, S, Ld, scale=0.8) if "site" in subset else None
    site = rng.integers(0, S, B) if table is not None else None
    lat32, z32 = AB.fuse_mean_fwd(head, table, site, Ld, ldz, F32)
    lat64, _ = AB.fuse_mean_fwd(head, table, site, Ld, ldz, F64)
    # one term: exact; two: the one addition rounds once, the factor 1 / 2 is exact -- the float32 chain is the only float32 answer
    assert (np.abs(lat32.astype(F64) - lat64) <= (E.U * np.abs(lat64) if len(subset) == 2 else 0.0)).all()
    assert (z32[:, Ld:] == 0).all() and np.array_equal(z32[:, :Ld], lat32)
    zb = AB.fuse_mean_fwd(head, table, site, Ld, ldz, F32, "bf16")[1]
    assert np.array_equal(zb[:, :Ld], AB.bf16(lat32)) and np.abs(zb[:, :Ld] - lat32).max() <= 2.0 ** -8 * np.abs(lat32).max()
    applicable = {"dirty_pads"} | ({"wrong_column"} if head is not None else set()) | ({"n_plus_one", "mean_twice", "no_table"} if len(subset) == 2 else set())
    for m in applicable:
        lat_m, z_m = AB.fuse_mean_fwd(head, table, site, Ld, ldz, F32, mistake=m)
        assert not (np.array_equal(lat_m, lat32) and np.array_equal(z_m, z32)), m


def test_mean_forward_label_out_of_range_poisons_its_row():
    rng = np.random.default_rng(1)
    head, table = rnd(rng, 9, 4), rnd(rng, 3, 4)
    site = np.array([0, 1, 2, -1, 3, 2 ** 40, 0, 1, 2])
    lat, z = AB.fuse_mean_fwd(head, table, site, 4, 8, F32)
    bad = np.array([False, False, False, True, True, True, False, False, False])
    assert np.isnan(lat[bad]).all() and np.isfinite(lat[~bad]).all() and np.isnan(z[bad, :4]).all() and (z[:, 4:] == 0).all()


@pytest.mark.parametrize("has_g", [True, False])
@pytest.mark.parametrize("n_mod", [1, 2])
def test_mean_backward_and_scatter(n_mod, has_g):
    rng = np.random.default_rng(10 * n_mod + has_g)
    B, Ld, S = 300, 20, 24
    dz, g = rnd(rng, B, Ld), (rnd(rng, B, Ld) if has_g else None)
    site = rng.integers(0, S, B)
    site[[3, 150]] = (-1, S)
    r64, r32, tol = AB.fuse_mean_bwd(dz, g, n_mod, F64), AB.fuse_mean_bwd(dz, g, n_mod, F32), AB.fuse_mean_bwd_tol(dz, g, n_mod)
    assert not outside(r32, r64, tol)
    if not has_g:
        assert np.array_equal(r32.astype(F64), r64)
    tref, ttol = E.scatter_tol(r64, tol, site, S)
    ok = (site >= 0) & (site < S)
    t32 = np.zeros((S, Ld), F32)
    np.add.at(t32, site[ok], r32[ok])                                  # a float32 scatter-add in row order
    assert not outside(t32, tref, ttol)
    everything = np.zeros((S, Ld), F32)
    np.add.at(everything, np.clip(site, 0, S - 1), r32)                # a scatter that clamps the labels instead of dropping them
    assert outside(everything, tref, ttol)
    if n_mod > 1:
        for m in ("n_plus_one", "mean_twice"):
            assert outside(AB.fuse_mean_bwd(dz, g, n_mod, F32, mistake=m), r64, tol), m


@pytest.mark.parametrize("has_enc,has_table", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("L,K,N", [(20, 128, 256), (7, 256, 128)])
def test_fused_latent_float32_is_inside_and_mistakes_are_not(L, K, N, has_enc, has_table):
    """the fused latent launch restated in float32 (head GEMM over k ascending, mean, bf16 z, the decoder's first layer) against float64"""
    rng = np.random.default_rng(L + K + has_enc + 2 * has_table)
    B, S = 37, 24
    x = AB.bf16(np.maximum(rnd(rng, B, K), 0)) if has_enc else None
    w, b = AB.bf16(rnd(rng, L, K, scale=K ** -0.5)), rnd(rng, L, scale=0.1)
    table, site = (rnd(rng, S, L, scale=0.5), rng.integers(0, S, B)) if has_table else (None, None)
    w0, b0 = AB.bf16(rnd(rng, N, L, scale=L ** -0.5)), rnd(rng, N, scale=0.1)
    args = (x, w, b, table, site, w0, b0)
    r64, r32, tols = AB.fused_latent(*args, F64), AB.fused_latent(*args, F32), AB.fused_latent_tol(*args)
    for name, got, want, tl in zip(("latent", "z", "h0"), r32, r64, tols):
        assert not outside(got, want, tl), name
    applicable = (["no_bias", "wrong_column"] if has_enc else []) + (["n_plus_one", "mean_twice", "no_table"] if has_enc and has_table else [])
    for m in applicable:
        bad = AB.fused_latent(*args, F32, mistake=m)
        assert outside(bad[0], r64[0], tols[0]) and outside(bad[2], r64[2], tols[2]), m
    dirty = AB.fuse_mean_fwd(r32[0], None, None, L, L + 4, F32, "bf16", mistake="dirty_pads")[1]
    assert (dirty[:, L:] != 0).all()                     # z pads not zero: caught by the exact pad check of the GPU tests
