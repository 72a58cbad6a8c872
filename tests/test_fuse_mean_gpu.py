"""mmvae_fuse_mean_fwd / _bwd -- the autoencoders' fusion, the plain mean of the encoder's head and the site's table row -- one launch
at a time through the C ABI.

The mean of one or two terms is exact after the one addition, so the forward (latent, z with its pads) and the backward's d_head (and
its bf16 copy) are held BIT-EQUAL to the float32 chain of tests/ae_bounds.py; the scatter-add into d_table is held to
elementwise_bounds.scatter_tol on both scatter paths.  (S, L) = (24, 20) and (64, 128) both scatter through LDS with one head
(32 KiB <= 48 KiB); (100, 128) is the global-atomics path.  No call hands the library a pointer or size that could make a kernel touch
memory outside its buffers."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ae_bounds as AB  # noqa: E402
import elementwise_bounds as E  # noqa: E402
from test_elementwise_gpu import dev, host, rnd, inside, bits, strided, stream, snapshot, unchanged, NAN, DEV, F32, F64, ERR_ARG  # noqa: E402
from mmvae import _lib as L  # noqa: E402
from mmvae import ops  # noqa: E402

SUBSETS = [("head",), ("head", "site"), ("site",)]
Z_FORMS = [("f32", 0), ("bf16", 0), ("bf16", 11)]           # (dtype, extra columns past ceil8(L))


def _same_bits(got, want, what):
    """float32 / bf16 device tensor against float64 values of that type: equal bit patterns, NaN where NaN"""
    g = got.detach().float().cpu().numpy()
    w = np.asarray(want, F64).astype(F32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: NaN pattern differs"
    ok = ~np.isnan(w)
    assert np.array_equal(g[ok].view(np.int32), w[ok].view(np.int32)), f"{what}: {int((g[ok] != w[ok]).sum())} elements differ in bits"


def _fwd(B, Ld, subset, zform, S=24, bad_rows=()):
    rng = np.random.default_rng(B * 1000 + Ld * 10 + len(subset) + (subset[0] == "site"))
    head_np = rnd(rng, B, Ld, scale=0.8) if "head" in subset else None
    if head_np is not None:
        head_np[0, 0], head_np[B - 1, Ld - 1] = -0.0, 0.0     # a head of -0 leaves as -0 when it is the only term (torch's mean of one)
    head = strided(head_np, 5) if head_np is not None else None
    table_np = rnd(rng, S, Ld, scale=0.8) if "site" in subset else None
    if table_np is not None:
        table_np[:, Ld - 1] = -0.0                             # ... and so does a table entry (site only); -0 + 0 = +0 with both
    site_np = rng.integers(0, S, B).astype(np.int64)
    for r, v in bad_rows:
        site_np[r] = v
    table, site = (dev(table_np), dev(site_np)) if table_np is not None else (None, None)
    zdt, extra = zform
    ldz = ops.ceil_to(Ld, 8) + extra
    latent = torch.full((B + 1, Ld), NAN, device=DEV)
    z = torch.full((B + 1, ldz), NAN, dtype=torch.float32 if zdt == "f32" else torch.bfloat16, device=DEV)
    ops.fuse_mean_fwd(B, Ld, head, table, site, latent[:B], z[:B])
    torch.cuda.synchronize()
    ref_lat, ref_z = AB.fuse_mean_fwd(head_np, table_np, site_np if table_np is not None else None, Ld, ldz, F32, zdt)
    tag = f"fuse_mean_fwd B{B} L{Ld} {subset} {zform}"
    _same_bits(latent[:B], ref_lat, tag + " latent")
    _same_bits(z[:B], ref_z, tag + " z")
    assert (bits(z[:B, Ld:]) == 0).all(), "pad columns of z must be +0"
    assert torch.isnan(latent[B]).all() and torch.isnan(z[B].float()).all(), "a row past B was written"
    return latent, ref_lat


@pytest.mark.parametrize("zform", Z_FORMS)
@pytest.mark.parametrize("subset", SUBSETS)
@pytest.mark.parametrize("Ld", [4, 20, 128])
def test_fuse_mean_fwd_bit_equal(Ld, subset, zform):
    for B in (1, 37, 1000):
        _fwd(B, Ld, subset, zform)


def test_fuse_mean_fwd_label_out_of_range_poisons_only_its_row():
    B, Ld, S = 37, 20, 24
    bad = [(3, -1), (17, S), (36, 2 ** 40)]
    latent, ref = _fwd(B, Ld, ("head", "site"), ("bf16", 0), S, bad)
    rows = np.zeros(B, bool)
    rows[[r for r, _ in bad]] = True
    got = latent[:B].cpu().numpy()
    assert np.isnan(got[rows]).all() and np.isfinite(got[~rows]).all()


def test_fuse_mean_fwd_refusals():
    B, Ld = 8, 4
    head, table, site = dev(np.ones((B, Ld), F32)), dev(np.ones((3, Ld), F32)), dev(np.zeros(B, np.int64))
    latent, z = torch.full((B, Ld), 5.0, device=DEV), torch.full((B, 8), 5.0, device=DEV)
    before = [snapshot(latent), snapshot(z)]

    def call(n_mod, h=head.data_ptr(), t=None, s=None, S=0, ldz=8, zdt=L.F32):
        a = L.FuseMeanFwdArgs(B, Ld, n_mod, h, Ld, t, s, S, latent.data_ptr(), z.data_ptr(), zdt, ldz)
        return L.load().mmvae_fuse_mean_fwd(C.byref(a), stream())
    assert call(2) == ERR_ARG and call(0) == ERR_ARG and call(0, h=None) == ERR_ARG          # n_mod is not the number present
    assert call(2, t=table.data_ptr(), s=None, S=3) == ERR_ARG                                  # a table without labels
    assert call(1, ldz=3) == ERR_ARG and call(1, zdt=7) == -2
    torch.cuda.synchronize()
    assert unchanged(latent, before[0]) and unchanged(z, before[1])


# =============================================================================================
# backward
# =============================================================================================
def _bwd(rng, B, Ld, n_mod, has_g, S=0, copies=None, ld_lp=None, bad_rows=()):
    """copies: None = no table; 0 / 1: d_table [S][L] with that table_copies argument; n: [n][S][L]."""
    dz_np = rnd(rng, B, Ld)
    dz = strided(dz_np, 3)
    g_np = rnd(rng, B, Ld) if has_g else None
    g = dev(g_np) if has_g else None
    ld_h = Ld + 4
    d_head = torch.full((B, ld_h), NAN, device=DEV)
    lp = torch.full((B, ld_lp), NAN, dtype=torch.bfloat16, device=DEV) if ld_lp else None
    site_np = rng.integers(0, max(S, 1), B)
    for r, v in bad_rows:
        site_np[r % B] = v
    site = dev(site_np.astype(np.int64)) if copies is not None else None
    d_table = torch.zeros((max(copies, 1), S, Ld), device=DEV) if copies is not None else None
    a = L.FuseMeanBwdArgs(B, Ld, n_mod, dz.data_ptr(), Ld + 3, ops._p(g), d_head.data_ptr(), ld_h, ops._p(lp), ld_lp or 0,
                          ops._p(d_table), ops._p(site), S, copies or 0)
    assert L.load().mmvae_fuse_mean_bwd(C.byref(a), stream()) == 0
    torch.cuda.synchronize()
    ref32 = AB.fuse_mean_bwd(dz_np, g_np, n_mod, F32)
    tag = f"fuse_mean_bwd B{B} L{Ld} n{n_mod} g{int(has_g)}"
    _same_bits(d_head[:, :Ld], ref32, tag + " d_head")
    assert torch.isnan(d_head[:, Ld:]).all(), "columns past L of d_head were written"
    if lp is not None:
        assert np.array_equal(bits(lp[:, :Ld]), bits(d_head[:, :Ld].to(torch.bfloat16))), "d_head_lp is not torch's bf16 rounding of d_head"
        assert (bits(lp[:, Ld:]) == 0).all(), "pad columns of d_head_lp must be +0"
    return d_table, site_np, AB.fuse_mean_bwd(dz_np, g_np, n_mod, F64), AB.fuse_mean_bwd_tol(dz_np, g_np, n_mod)


@pytest.mark.parametrize("has_g", [True, False])
@pytest.mark.parametrize("n_mod", [1, 2])
def test_fuse_mean_bwd_heads_bit_equal(n_mod, has_g):
    for Ld in (4, 20, 128):
        for B, ld_lp in ((1, None), (129, Ld), (1000, ops.ceil_to(Ld, 8) + 8)):
            _bwd(np.random.default_rng(n_mod * 100 + has_g + B + Ld), B, Ld, n_mod, has_g, ld_lp=ld_lp)


@pytest.mark.parametrize("copies", [0, 1, 8, 11])
@pytest.mark.parametrize("path,S,Ld", [("lds", 24, 20), ("lds", 64, 128), ("global", 100, 128)])
def test_fuse_mean_bwd_table_scatter(path, S, Ld, copies):
    assert (S * Ld * 4 > 48 * 1024) == (path == "global")               # the entry point's choice of scatter path
    variants = itertools.cycle([(1, True, None), (2, False, Ld), (2, True, ops.ceil_to(Ld, 8) + 8)])
    for B in (1, 127, 128, 129, 4099):                                  # around the 128 rows of one workgroup
        n_mod, has_g, ld_lp = next(variants)
        rng = np.random.default_rng(S * 7 + copies * 31 + B)
        bad = [(3, -1), (B // 2, S), (B - 1, 2 ** 40)] if B >= 127 else []
        d_table, site_np, ref, tol = _bwd(rng, B, Ld, n_mod, has_g, S, copies, ld_lp, bad)
        tag = f"fuse_mean_bwd {path} S{S} L{Ld} copies{copies} B{B}"
        tref, ttol = E.scatter_tol(ref, tol, site_np, S)
        got = host(d_table).sum(0)                                      # the copies, summed in float64
        inside(got, tref, ttol, tag + " d_table")
        seen = np.zeros(S, bool)
        seen[site_np[(site_np >= 0) & (site_np < S)]] = True
        assert (got[~seen] == 0).all(), "a class without rows (or a label out of range) received a gradient"
        used = min(max(copies, 1), (B + 127) // 128)                    # workgroup w adds into copy w % copies
        assert (host(d_table)[used:] == 0).all()


def test_fuse_mean_bwd_refusals():
    B, Ld = 16, 4
    rng = np.random.default_rng(3)
    dz = dev(rnd(rng, B, Ld))
    d_head, d_table = torch.full((B, Ld), 5.0, device=DEV), torch.full((6, Ld), 5.0, device=DEV)
    before = [snapshot(d_head), snapshot(d_table)]

    def call(n_mod=1, dzp=dz.data_ptr(), table=None, site=None, S=0):
        a = L.FuseMeanBwdArgs(B, Ld, n_mod, dzp, Ld, None, d_head.data_ptr(), Ld, None, 0, table, site, S, 1)
        return L.load().mmvae_fuse_mean_bwd(C.byref(a), stream())
    assert call(n_mod=0) == ERR_ARG and call(n_mod=3) == ERR_ARG and call(dzp=None) == ERR_ARG
    assert call(table=d_table.data_ptr(), site=None, S=6) == ERR_ARG        # a table without labels
    torch.cuda.synchronize()
    assert unchanged(d_head, before[0]) and unchanged(d_table, before[1])
