"""Every kernel of csrc/elementwise.hip that had no test of its own, one launch at a time through the C ABI, against float64:
mean fusion + reparameterisation (both directions, both scatter paths), the EncoderC table, the BatchNorm finalisations, weight
preparation, the small element-wise launches and multi-tensor AdamW.

Nothing here is a tolerance fitted to what the kernels return.  A check is either EXACT (copies, zero padding, bf16 rounding, counters,
refusals that must leave every output untouched) or held to a bound DERIVED by counting the float32 roundings of the kernel's
expression: tests/elementwise_bounds.py states each formula and its bound, tests/test_elementwise_ref_cpu.py shows on the CPU that a
float32 restatement stays inside it.  No element is excluded anywhere.  References: oracle/np_oracle.py where it has the
operation (reparameterize, encoder_c_fwd / _bwd, adamw_step), torch.nn.functional.batch_norm in float64 on the CPU for the running
statistics, float64 numpy otherwise.

No call hands the library a pointer or a size that could make a kernel touch memory outside its buffers: refusal tests use only
arguments the entry points reject before they launch, and every buffer is allocated at its full padded size.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import np_oracle as O  # noqa: E402
import elementwise_bounds as E  # noqa: E402
from mmvae import _lib as L  # noqa: E402
from mmvae import ops  # noqa: E402

DEV = "cuda"
F32, F64 = np.float32, np.float64
NAN = float("nan")
ERR_ARG = -1


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().double().cpu().numpy()


def rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(F32)


def stream():
    return torch.cuda.current_stream().cuda_stream


def strided(x, pad, fill=NAN):
    """Device copy of the 2-D array x as a view of a [rows][cols + pad] buffer whose pad columns hold `fill`."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), fill, dtype=torch.float32, device=DEV)
    buf[:, :x.shape[1]] = dev(x)
    return buf[:, :x.shape[1]]


def inside(got, ref, tol, what):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    tol = np.broadcast_to(np.asarray(tol, F64), ref.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = np.abs(got - ref)
    nz = tol > 0
    ratio = float(np.max(err[nz] / tol[nz])) if nz.any() else 0.0
    print(f"{what}: max err {err.max() if err.size else 0:.3e}, max err / bound {ratio:.3f}")
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements outside the derived bound; worst err {err[bad].max():.3e} (bound {tol[bad][np.argmax(err[bad])]:.3e})"


def bits(t):
    """Bit patterns of a float32 / bf16 tensor as a numpy integer array."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def ulps_apart(a, b):
    """Largest distance, in units of the last place of their type, between two finite tensors of one dtype."""
    def ordered(t):
        i = bits(t).astype(np.int64)
        mask = 0x7FFFFFFF if t.dtype == torch.float32 else 0x7FFF
        return np.where(i >= 0, i, -(i & mask))
    return int(np.abs(ordered(a) - ordered(b)).max())


def unchanged(t, before):
    return np.array_equal(bits(t) if t.is_floating_point() else t.cpu().numpy(), before)


def snapshot(t):
    return bits(t).copy() if t.is_floating_point() else t.cpu().numpy().copy()


# =============================================================================================
# mean fusion + reparameterisation, forward
# =============================================================================================
SUBSETS = [s for r in (1, 2, 3) for s in itertools.combinations(("a", "b", "table"), r)]
Z_FORMS = [("f32", 0), ("bf16", 0), ("bf16", 11)]           # (dtype, extra columns past ceil8(L); 11: ldz = L + 11)


def _fuse_fwd_case(rng, B, Ld, subset, S=24, bad_rows=()):
    ld_pad = 5
    ha = strided(rnd(rng, B, 2 * Ld, scale=0.8), ld_pad) if "a" in subset else None
    hb = strided(rnd(rng, B, 2 * Ld, scale=0.8), ld_pad) if "b" in subset else None
    table = dev(rnd(rng, S, 2 * Ld, scale=0.8)) if "table" in subset else None
    site_np = rng.integers(0, S, B)
    for r, v in bad_rows:
        site_np[r] = v
    site = dev(site_np.astype(np.int64)) if table is not None else None
    eps = dev(rnd(rng, B, Ld))
    return ha, hb, table, site, site_np, eps


def _fuse_fwd_reference(ha, hb, table, site_np, eps, Ld, ok):
    mt, lt = [], []
    for h in (ha, hb):
        if h is not None:
            x = h.cpu().numpy()
            mt.append(x[:, :Ld]); lt.append(x[:, Ld:])
    if table is not None:
        T = table.cpu().numpy()
        rows = T[np.where(ok, site_np, 0)]
        mt.append(rows[:, :Ld]); lt.append(rows[:, Ld:])
    e = eps.cpu().numpy()
    return E.fuse_fwd(mt, lt, e, F64), E.fuse_fwd_tol(mt, lt, e)


@pytest.mark.parametrize("zform", Z_FORMS, ids=lambda f: f"{f[0]}+{f[1]}")
@pytest.mark.parametrize("Ld", [4, 20, 128])
@pytest.mark.parametrize("subset", SUBSETS, ids="+".join)
def test_fuse_reparam_fwd(subset, Ld, zform):
    zt = torch.float32 if zform[0] == "f32" else torch.bfloat16
    ldz = Ld + 11 if zform[1] else ops.ceil_to(Ld, 8)
    for B in (1, 130, 4099):
        rng = np.random.default_rng(SUBSETS.index(subset) * 1000 + Ld * 10 + B % 7)
        ha, hb, table, site, site_np, eps = _fuse_fwd_case(rng, B, Ld, subset)
        mu, lv = (torch.full((B, Ld), NAN, device=DEV) for _ in range(2))
        zbuf = torch.full((B, ldz), NAN, dtype=zt, device=DEV)
        assert ops._ld(zbuf[:, :Ld]) == ldz and (ha is None or ops._ld(ha) == 2 * Ld + 5)     # the leading dimensions under test
        ops.fuse_reparam_fwd(B, Ld, ha, hb, table, site, eps, mu, lv, zbuf[:, :Ld])
        (rmu, rlv, rz), (tmu, tlv, tz) = _fuse_fwd_reference(ha, hb, table, site_np, eps, Ld, np.ones(B, bool))
        tag = f"fwd {'+'.join(subset)} L{Ld} B{B} {zform}"
        inside(host(mu), rmu, tmu, tag + " mu")
        inside(host(lv), rlv, tlv, tag + " logvar")
        inside(host(zbuf[:, :Ld]), rz, tz if zt == torch.float32 else E.bf16_out(tz, rz), tag + " z")
        assert np.allclose(rz, O.reparameterize(rmu, rlv, host(eps)), rtol=1e-14, atol=0)
        assert (bits(zbuf[:, Ld:]) == 0).all(), "pad columns of z must be +0"


def test_fuse_reparam_fwd_label_out_of_range_poisons_its_row_only():
    B, Ld, S = 130, 20, 24
    bad = [(0, -1), (7, S), (64, 2 ** 40), (129, -(2 ** 62))]
    rng = np.random.default_rng(1)
    ha, hb, table, site, site_np, eps = _fuse_fwd_case(rng, B, Ld, ("a", "table"), S, bad)
    ok = (site_np >= 0) & (site_np < S)
    assert (~ok).sum() == 4
    mu, lv = (torch.full((B, Ld), 5.0, device=DEV) for _ in range(2))
    zbuf = torch.full((B, 24), 5.0, dtype=torch.bfloat16, device=DEV)
    ops.fuse_reparam_fwd(B, Ld, ha, None, table, site, eps, mu, lv, zbuf[:, :Ld])
    (rmu, rlv, rz), (tmu, tlv, tz) = _fuse_fwd_reference(ha, None, table, site_np, eps, Ld, ok)
    for got, ref, tol, name in ((mu, rmu, tmu, "mu"), (lv, rlv, tlv, "logvar"), (zbuf[:, :Ld], rz, E.bf16_out(tz, rz), "z")):
        g = host(got)
        assert np.isnan(g[~ok]).all(), f"{name}: a row with a label outside [0, S) must be NaN"
        inside(g[ok], ref[ok], tol[ok], "bad label, other rows: " + name)
    assert (bits(zbuf[:, Ld:]) == 0).all()


def test_fuse_reparam_fwd_refuses_a_wrong_modality_count():
    B, Ld = 16, 4
    rng = np.random.default_rng(2)
    ha, eps = dev(rnd(rng, B, 2 * Ld)), dev(rnd(rng, B, Ld))
    mu, lv, z = (torch.full((B, Ld), 5.0, device=DEV) for _ in range(3))
    before = [snapshot(t) for t in (mu, lv, z)]
    for n_mod, heads_a in ((2, ha.data_ptr()), (0, ha.data_ptr()), (1, None)):
        a = L.FuseFwdArgs(B, Ld, n_mod, heads_a, None, 2 * Ld, None, None, 0, eps.data_ptr(), mu.data_ptr(), lv.data_ptr(), z.data_ptr(), L.F32, Ld)
        assert L.load().mmvae_fuse_reparam_fwd(C.byref(a), stream()) == ERR_ARG
    a = L.FuseFwdArgs(B, Ld, 1, ha.data_ptr(), None, 2 * Ld, None, None, 0, eps.data_ptr(), mu.data_ptr(), lv.data_ptr(), z.data_ptr(), L.F32, Ld - 1)
    assert L.load().mmvae_fuse_reparam_fwd(C.byref(a), stream()) == ERR_ARG           # ldz < L
    torch.cuda.synchronize()
    assert all(unchanged(t, b) for t, b in zip((mu, lv, z), before))


# =============================================================================================
# mean fusion + reparameterisation, backward
# =============================================================================================
def _fuse_bwd_run(rng, B, Ld, n_mod, k, has_g, S=0, copies=None, ld_lp=None, bad_rows=()):
    """One launch.  copies: None = no table; 0 / 1: d_table [S][2L] with that table_copies argument; n: [n][S][2L]."""
    dz_np = [rnd(rng, B, Ld) for _ in range(k)]
    dzs = [strided(d, 3) for d in dz_np]
    gm_np, gl_np = (rnd(rng, B, Ld), rnd(rng, B, Ld)) if has_g else (None, None)
    eps_np, lv_np = rnd(rng, B, Ld), rnd(rng, B, Ld, scale=0.7)
    ld_h = 2 * Ld + 4
    d_heads = torch.full((B, ld_h), NAN, device=DEV)
    lp = torch.full((B, ld_lp), NAN, dtype=torch.bfloat16, device=DEV) if ld_lp else None
    site_np = rng.integers(0, max(S, 1), B)
    for r, v in bad_rows:
        site_np[r % B] = v
    site = dev(site_np.astype(np.int64)) if copies is not None else None
    d_table = torch.zeros((max(copies, 1), S, 2 * Ld), device=DEV) if copies is not None else None
    keep = [dev(x) if x is not None else None for x in (gm_np, gl_np, eps_np, lv_np)]
    a = L.FuseBwdArgs(B, Ld, n_mod, ops._p(keep[0]), ops._p(keep[1]), dzs[0].data_ptr(), dzs[1].data_ptr() if k > 1 else None,
                      dzs[2].data_ptr() if k > 2 else None, Ld + 3, keep[2].data_ptr(), keep[3].data_ptr(), d_heads.data_ptr(), ld_h,
                      ops._p(d_table), ops._p(site), S, ops._p(lp), ld_lp or 0, copies or 0)
    assert L.load().mmvae_fuse_reparam_bwd(C.byref(a), stream()) == 0
    torch.cuda.synchronize()
    ref = E.fuse_bwd(gm_np, gl_np, dz_np, eps_np, lv_np, n_mod, F64)
    tol = E.fuse_bwd_tol(gm_np, gl_np, dz_np, eps_np, lv_np, n_mod)
    return d_heads, lp, d_table, site_np, np.concatenate(ref, 1), np.concatenate(tol, 1)


def _fuse_bwd_check(tag, Ld, d_heads, lp, ref, tol):
    inside(host(d_heads[:, :2 * Ld]), ref, tol, tag + " d_heads")
    assert torch.isnan(d_heads[:, 2 * Ld:]).all(), "columns past 2L of d_heads were written"
    if lp is not None:
        assert np.array_equal(bits(lp[:, :2 * Ld]), bits(d_heads[:, :2 * Ld].to(torch.bfloat16))), "d_heads_lp is not torch's bf16 rounding of d_heads"
        assert (bits(lp[:, 2 * Ld:]) == 0).all(), "pad columns of d_heads_lp must be +0"


@pytest.mark.parametrize("has_g", [True, False])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("n_mod", [1, 2, 3])
def test_fuse_reparam_bwd_heads(n_mod, k, has_g):
    Ld = 20
    for B, ld_lp in ((129, None), (4099, 2 * Ld), (127, ops.ceil_to(2 * Ld, 8) + 8)):
        rng = np.random.default_rng(n_mod * 100 + k * 10 + has_g + B)
        d_heads, lp, _, _, ref, tol = _fuse_bwd_run(rng, B, Ld, n_mod, k, has_g, ld_lp=ld_lp)
        _fuse_bwd_check(f"bwd n{n_mod} k{k} g{int(has_g)} B{B}", Ld, d_heads, lp, ref, tol)


@pytest.mark.parametrize("copies", [0, 1, 8, 11])
@pytest.mark.parametrize("path,S,Ld", [("lds", 24, 20), ("global", 64, 128)])
def test_fuse_reparam_bwd_table_scatter(path, S, Ld, copies):
    assert (S * 2 * Ld * 4 > 48 * 1024) == (path == "global")          # the entry point's choice of scatter path
    variants = itertools.cycle([(1, 1, True, None), (2, 2, False, 2 * Ld), (3, 3, True, ops.ceil_to(2 * Ld, 8) + 8)])
    for B in (1, 127, 128, 129, 4099):                                  # around the 128 rows of one workgroup
        n_mod, k, has_g, ld_lp = next(variants)
        rng = np.random.default_rng(S * 7 + copies * 31 + B)
        bad = [(3, -1), (B // 2, S), (B - 1, 2 ** 40)] if B >= 127 else []
        d_heads, lp, d_table, site_np, ref, tol = _fuse_bwd_run(rng, B, Ld, n_mod, k, has_g, S, copies, ld_lp, bad)
        tag = f"bwd {path} copies{copies} B{B}"
        _fuse_bwd_check(tag, Ld, d_heads, lp, ref, tol)
        tref, ttol = E.scatter_tol(ref, tol, site_np, S)
        got = host(d_table).sum(0)                                      # the copies, summed in float64
        inside(got, tref, ttol, tag + " d_table")
        seen = np.zeros(S, bool)
        seen[site_np[(site_np >= 0) & (site_np < S)]] = True
        assert (got[~seen] == 0).all(), "a class without rows (or a label out of range) received a gradient"
        used = min(max(copies, 1), (B + 127) // 128)                    # workgroup w adds into copy w % copies
        assert (host(d_table)[used:] == 0).all()


def test_fuse_reparam_bwd_refusals():
    B, Ld = 16, 4
    rng = np.random.default_rng(3)
    dz, eps, lv = dev(rnd(rng, B, Ld)), dev(rnd(rng, B, Ld)), dev(rnd(rng, B, Ld))
    d_heads, d_table = torch.full((B, 2 * Ld), 5.0, device=DEV), torch.full((6, 2 * Ld), 5.0, device=DEV)
    before = [snapshot(d_heads), snapshot(d_table)]

    def call(n_mod=1, dzp=dz.data_ptr(), table=None, site=None, S=0):
        a = L.FuseBwdArgs(B, Ld, n_mod, None, None, dzp, None, None, Ld, eps.data_ptr(), lv.data_ptr(), d_heads.data_ptr(), 2 * Ld,
                          table, site, S, None, 0, 1)
        return L.load().mmvae_fuse_reparam_bwd(C.byref(a), stream())
    assert call(n_mod=0) == ERR_ARG and call(dzp=None) == ERR_ARG
    assert call(table=d_table.data_ptr(), site=None, S=6) == ERR_ARG        # a table without labels
    torch.cuda.synchronize()
    assert unchanged(d_heads, before[0]) and unchanged(d_table, before[1])


# =============================================================================================
# EncoderC table
# =============================================================================================
# (32, 32, 128): 68 KiB of operands, the first size past the default dynamic-LDS limit (refused until the launch learnt to raise it);
# (24, 64, 100): the corner of the reference's hyperparameter search, 74.75 KiB; (76, 64, 128): 159 KiB, the last size the CU's LDS holds
EMBED_SHAPES = [(6, 8, 4), (24, 32, 20), (24, 32, 128), (5, 3, 7), (32, 32, 128), (24, 64, 100), (76, 64, 128)]
EMBED_LDS_MAX = 160 * 1024                       # mmvae_embed_table_bwd's capacity (include/mmvae_hip.h)


def embed_lds_bytes(S, Ed, Ld, heads=2):
    return (S * heads * Ld + S * Ed + heads * Ld * Ed) * 4


def _embed_params(rng, S, Ed, Ld):
    return rnd(rng, S, Ed), rnd(rng, Ld, Ed, scale=0.3), rnd(rng, Ld, scale=0.5), rnd(rng, Ld, Ed, scale=0.3), rnd(rng, Ld, scale=0.5)


@pytest.mark.parametrize("S,Ed,Ld", EMBED_SHAPES)
def test_embed_table_fwd(S, Ed, Ld):
    rng = np.random.default_rng(S * 100 + Ld)
    emb, wm, bm, wl, bl = _embed_params(rng, S, Ed, Ld)
    table = torch.full((S + 1, 2 * Ld), NAN, device=DEV)
    ops.embed_table_fwd(dev(emb), dev(wm), dev(bm), dev(wl), dev(bl), table)
    ref = E.embed_fwd(emb, wm, bm, wl, bl, F64)
    P = {"encoder_c.embedding.weight": emb.astype(F64), "encoder_c.fc_mu.weight": wm.astype(F64), "encoder_c.fc_mu.bias": bm.astype(F64),
         "encoder_c.fc_logvar.weight": wl.astype(F64), "encoder_c.fc_logvar.bias": bl.astype(F64)}
    mu, lv, _ = O.encoder_c_fwd(P, np.arange(S))
    assert np.allclose(ref, np.concatenate([mu, lv], 1), rtol=1e-12, atol=1e-13)
    inside(host(table[:S]), ref, E.embed_fwd_tol(emb, wm, bm, wl, bl), f"embed_table_fwd {S, Ed, Ld}")
    assert torch.isnan(table[S]).all()


@pytest.mark.parametrize("copies", [1, 8, 11])
@pytest.mark.parametrize("S,Ed,Ld", EMBED_SHAPES)
def test_embed_table_bwd(S, Ed, Ld, copies):
    rng = np.random.default_rng(S * 100 + Ld + copies)
    emb, wm, bm, wl, bl = _embed_params(rng, S, Ed, Ld)
    dT = [rnd(rng, S, 2 * Ld) for _ in range(copies)]
    old = (rnd(rng, S, Ed), rnd(rng, 2 * Ld, Ed), rnd(rng, 2 * Ld))               # the gradients are ACCUMULATED into
    d_emb, d_wm, d_wl = dev(old[0]), dev(old[1][:Ld]), dev(old[1][Ld:])
    d_bm, d_bl = dev(old[2][:Ld]), dev(old[2][Ld:])
    ops.embed_table_bwd(dev(emb), dev(wm), dev(wl), dev(np.stack(dT)), d_emb, d_wm, d_bm, d_wl, d_bl)
    ref, tol = E.embed_bwd(dT, emb, wm, wl, old, F64), E.embed_bwd_tol(dT, emb, wm, wl, old)
    # the pinned oracle on the table gradient as if every class were one sample
    P = {"encoder_c.embedding.weight": emb.astype(F64), "encoder_c.fc_mu.weight": wm.astype(F64), "encoder_c.fc_logvar.weight": wl.astype(F64)}
    G, dTs = {}, np.sum([d.astype(F64) for d in dT], 0)
    O.encoder_c_bwd(P, dict(pre="encoder_c", h=emb.astype(F64), site=np.arange(S)), dTs[:, :Ld], dTs[:, Ld:], G)
    assert np.allclose(ref[0] - old[0], G["encoder_c.embedding.weight"], rtol=1e-9, atol=1e-11)
    assert np.allclose(ref[1][:Ld] - old[1][:Ld], G["encoder_c.fc_mu.weight"], rtol=1e-9, atol=1e-11)
    assert np.allclose(ref[2][Ld:] - old[2][Ld:], G["encoder_c.fc_logvar.bias"], rtol=1e-9, atol=1e-11)
    tag = f"embed_table_bwd {S, Ed, Ld} copies {copies}"
    inside(host(d_emb), ref[0], tol[0], tag + " d_emb")
    inside(np.concatenate([host(d_wm), host(d_wl)]), ref[1], tol[1], tag + " d_W")
    inside(np.concatenate([host(d_bm), host(d_bl)]), ref[2], tol[2], tag + " d_b")


def test_embed_table_bwd_sizes_straddle_both_lds_limits():
    """EMBED_SHAPES holds the default dynamic-LDS limit (64 KiB) and the capacity (160 KiB) from both sides."""
    sizes = sorted(embed_lds_bytes(*s) for s in EMBED_SHAPES)
    assert any(b <= 64 * 1024 for b in sizes) and any(64 * 1024 < b <= EMBED_LDS_MAX for b in sizes)
    assert embed_lds_bytes(24, 32, 128) <= 64 * 1024 < embed_lds_bytes(32, 32, 128)
    assert embed_lds_bytes(76, 64, 128) <= EMBED_LDS_MAX < embed_lds_bytes(77, 64, 128)


def test_embed_table_bwd_refuses_operands_beyond_the_cu_lds():
    S, Ed, Ld = 77, 64, 128                       # (S 2L + S E + 2L E) floats = 160.25 KiB; 76 sites: 159 KiB, accepted above
    assert embed_lds_bytes(S, Ed, Ld) > EMBED_LDS_MAX >= embed_lds_bytes(S - 1, Ed, Ld)
    rng = np.random.default_rng(4)
    emb, wm, bm, wl, bl = _embed_params(rng, S, Ed, Ld)
    outs = [torch.full(s, 5.0, device=DEV) for s in ((S, Ed), (Ld, Ed), (Ld,), (Ld, Ed), (Ld,))]
    before = [snapshot(t) for t in outs]
    with pytest.raises(L.MMVAEArgError):
        ops.embed_table_bwd(dev(emb), dev(wm), dev(wl), dev(rnd(rng, S, 2 * Ld)), *outs)
    torch.cuda.synchronize()
    assert all(unchanged(t, b) for t, b in zip(outs, before))


# =============================================================================================
# BatchNorm pieces
# =============================================================================================
def _bn_data(rng, M, N):
    x = rng.standard_normal((M, N)) * rng.uniform(0.1, 3.0, N) + rng.uniform(-2, 2, N)
    x[:, 0] = 1000.0 + 1.0 / 3.0                 # a constant column with a large mean: s2 / M - mean^2 cancels to ~1e-10, either sign
    gamma, beta = rnd(rng, N) + 1.5, rnd(rng, N)
    rm, rv = rnd(rng, N), rng.uniform(0.5, 2.0, N).astype(F32)
    return x, gamma, beta, rm, rv


@pytest.mark.parametrize("running", [True, False], ids=["running", "no_running"])
@pytest.mark.parametrize("M", [2, 3, 1000])
@pytest.mark.parametrize("N", [1, 24, 128, 257, 512])
def test_bn_finalize(N, M, running):
    rng = np.random.default_rng(N * 10 + M)
    x, gamma, beta, rm, rv = _bn_data(rng, M, N)
    s1, s2 = x.sum(0), (x * x).sum(0)
    stats = dev(np.stack([s1, s2]))
    out = {k: torch.full((N + 3,), NAN, device=DEV) for k in ("mean", "rstd", "scale", "shift")}
    d_rm, d_rv, nbt = dev(rm), dev(rv), torch.tensor([41], dtype=torch.int64, device=DEV)
    ops.bn_finalize(M, N, stats, dev(gamma), dev(beta), d_rm if running else None, d_rv if running else None, nbt if running else None,
                    out["mean"], out["rstd"], out["scale"], out["shift"])
    args = (s1, s2, M, gamma, beta, ops.BN_EPS, ops.BN_MOMENTUM, rm if running else None, rv if running else None)
    ref, tol = E.bn_finalize(*args, F64), E.bn_finalize_tol(*args)
    for k in out:
        inside(host(out[k][:N]), ref[k], tol[k], f"bn_finalize N{N} M{M} {k}")
        assert torch.isnan(out[k][N:]).all()
    rstd = host(out["rstd"][:N])
    assert rstd[0] <= 1.0 / np.sqrt(float(F32(ops.BN_EPS))) * (1 + 2 * E.U), "constant column: rstd beyond 1 / sqrt(eps)"
    if not running:
        assert unchanged(d_rm, bits(dev(rm))) and unchanged(d_rv, bits(dev(rv))) and nbt.item() == 41
        return
    assert nbt.item() == 42                       # exactly one step
    inside(host(d_rm), ref["running_mean"], tol["running_mean"], "running_mean")
    inside(host(d_rv), ref["running_var"], tol["running_var"], "running_var")
    # torch's BatchNorm in float64 on the CPU from the DATA: momentum form and unbiased variance (biased: off by var / M * momentum)
    t_rm, t_rv = torch.from_numpy(rm.astype(F64)), torch.from_numpy(rv.astype(F64))
    y = torch.nn.functional.batch_norm(torch.from_numpy(x), t_rm, t_rv, torch.from_numpy(gamma.astype(F64)), torch.from_numpy(beta.astype(F64)),
                                       training=True, momentum=float(F32(ops.BN_MOMENTUM)), eps=float(F32(ops.BN_EPS)))
    tol_t = E.bn_finalize_tol(*args, sums_rel=(M + 1) * E.F64)
    inside(host(d_rm), t_rm.numpy(), tol_t["running_mean"], "running_mean against torch")
    inside(host(d_rv), t_rv.numpy(), tol_t["running_var"], "running_var against torch")
    # the normalisation the consumer GEMM applies, y = x scale + shift, against torch's output (not the constant column, whose
    # output is cancellation noise times rstd in either implementation)
    yk = x[:, 1:] * host(out["scale"][1:N]) + host(out["shift"][1:N])
    mag = np.abs(x[:, 1:]) * tol_t["scale"][1:] + tol_t["shift"][1:]
    inside(yk, y.numpy()[:, 1:], mag + 1e-12 * (1 + np.abs(yk)), "x scale + shift against torch")


def test_bn_finalize_refuses_one_row():
    N = 24
    rng = np.random.default_rng(5)
    stats, gamma, beta = dev(rng.standard_normal((2, N))), dev(rnd(rng, N)), dev(rnd(rng, N))
    outs = [torch.full((N,), 5.0, device=DEV) for _ in range(6)]
    nbt = torch.tensor([41], dtype=torch.int64, device=DEV)
    before = [snapshot(t) for t in outs]
    a = L.BnFinalizeArgs(1, N, stats[0].data_ptr(), stats[1].data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5, 0.1,
                         outs[4].data_ptr(), outs[5].data_ptr(), nbt.data_ptr(), *(t.data_ptr() for t in outs[:4]))
    assert L.load().mmvae_bn_finalize(C.byref(a), stream()) == ERR_ARG
    with pytest.raises(ValueError):
        ops.bn_finalize(1, N, stats, gamma, beta, outs[4], outs[5], nbt, *outs[:4])
    torch.cuda.synchronize()
    assert all(unchanged(t, b) for t, b in zip(outs, before)) and nbt.item() == 41


@pytest.mark.parametrize("with_stats", [True, False])
@pytest.mark.parametrize("N", [1, 24, 128, 257, 512])
def test_bn_eval_coeffs(N, with_stats):
    rng = np.random.default_rng(N)
    _, gamma, beta, rm, rv = _bn_data(rng, 4, N)
    rv[0] = 0.0                                   # rstd = 1 / sqrt(eps)
    out = {k: torch.full((N + 3,), NAN, device=DEV) for k in ("scale", "shift", "mean", "rstd")}
    ops.bn_eval_coeffs(dev(gamma), dev(beta), dev(rm), dev(rv), out["scale"], out["shift"], mean=out["mean"] if with_stats else None,
                       rstd=out["rstd"] if with_stats else None)
    ref, tol = E.bn_eval(gamma, beta, rm, rv, ops.BN_EPS, F64), E.bn_eval_tol(gamma, beta, rm, rv, ops.BN_EPS)
    for k in out:
        if k in ("mean", "rstd") and not with_stats:
            assert torch.isnan(out[k]).all()
            continue
        inside(host(out[k][:N]), ref[k], tol[k], f"bn_eval_coeffs N{N} {k}")
        assert torch.isnan(out[k][N:]).all()
    # eval-mode BatchNorm of torch in float64: y = x scale + shift
    x = rng.standard_normal((7, N))
    y = torch.nn.functional.batch_norm(torch.from_numpy(x), torch.from_numpy(rm.astype(F64)), torch.from_numpy(rv.astype(F64)),
                                       torch.from_numpy(gamma.astype(F64)), torch.from_numpy(beta.astype(F64)), training=False,
                                       eps=float(F32(ops.BN_EPS))).numpy()
    inside(x * host(out["scale"][:N]) + host(out["shift"][:N]), y, np.abs(x) * tol["scale"] + tol["shift"] + 1e-12 * (1 + np.abs(y)), "eval y against torch")


def _bn_bwd_case(rng, M, N, dt):
    d, y = rnd(rng, M, N), rnd(rng, M, N, scale=2.0)
    if dt == torch.bfloat16:
        d, y = O.bf16_round(d), O.bf16_round(y)
    mean, rstd, gamma = rnd(rng, N), rng.uniform(0.3, 3, N).astype(F32), rnd(rng, N) + 1.5
    xh = (y.astype(F64) - mean) * rstd
    sd, sdx = d.astype(F64).sum(0), (d * xh).sum(0)               # the f64 column sums of the statistics phase
    return d, y, mean, rstd, gamma, sd, sdx, rnd(rng, N), rnd(rng, N)


@pytest.mark.parametrize("eval_mode", [False, True], ids=["train", "eval"])
@pytest.mark.parametrize("M", [1, 24, 1000])
@pytest.mark.parametrize("N", [1, 24, 128, 257, 512])
def test_bn_bwd_finalize(N, M, eval_mode):
    rng = np.random.default_rng(N * 10 + M)
    d, y, mean, rstd, gamma, sd, sdx, old_g, old_b = _bn_bwd_case(rng, M, N, torch.float32)
    dgamma, dbeta, coef = dev(old_g), dev(old_b), torch.full((3, N), NAN, device=DEV)
    ops.bn_bwd_finalize(M, N, dev(np.stack([sd, sdx])), dev(gamma), dev(rstd), dgamma, dbeta, coef, eval_mode)
    inside(host(dgamma), E.accum(old_g, sdx, F64), E.accum_tol(old_g, sdx), "dgamma")
    inside(host(dbeta), E.accum(old_b, sd, F64), E.accum_tol(old_b, sd), "dbeta")
    inside(host(coef), E.bn_bwd_coefs(sd, sdx, M, gamma, rstd, eval_mode, F64), E.bn_bwd_coefs_tol(sd, sdx, M, gamma, rstd, eval_mode), "coef")
    if eval_mode:
        assert (bits(coef[1:]) == 0).all()


FIN_APPLY = [("bf16", n) for n in (64, 128, 256, 512)] + [("f32", n) for n in (32, 128, 512)]


@pytest.mark.parametrize("eval_mode", [False, True], ids=["train", "eval"])
@pytest.mark.parametrize("M", [1, 5, 4133])
@pytest.mark.parametrize("dtype,N", FIN_APPLY)
def test_bn_bwd_finalize_apply(dtype, N, M, eval_mode):
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    rng = np.random.default_rng(N * 10 + M)
    d, y, mean, rstd, gamma, sd, sdx, old_g, old_b = _bn_bwd_case(rng, M, N, dt)
    ld = N + 8
    def padded(x):
        buf = torch.full((M, ld), 3.0, dtype=dt, device=DEV)
        buf[:, :N] = dev(x).to(dt)
        return buf
    stats, t_mean, t_rstd, t_gamma = dev(np.stack([sd, sdx])), dev(mean), dev(rstd), dev(gamma)
    # the two-launch form on a copy
    d2, y2 = padded(d), padded(y)
    dg2, db2, coef = dev(old_g), dev(old_b), torch.empty((3, N), device=DEV)
    ops.bn_bwd_finalize(M, N, stats, t_gamma, t_rstd, dg2, db2, coef, eval_mode)
    ops.bn_bwd_apply(d2[:, :N], y2[:, :N], N, t_mean, t_rstd, coef)
    # the fused launch
    d1, y1 = padded(d), padded(y)
    dg1, db1 = dev(old_g), dev(old_b)
    ops.bn_bwd_finalize_apply(d1[:, :N], y1[:, :N], M, N, t_mean, t_rstd, stats, t_gamma, dg1, db1, eval_mode)
    torch.cuda.synchronize()
    tag = f"finalize_apply {dtype} N{N} M{M}"
    # dgamma / dbeta: added exactly once whatever the grid is, and bit-identical to the finalize launch.  (A kernel in which a SECOND
    # thread of a column added as well would race with the first -- both usually read the old value -- so this check catches that
    # fault only when their waves drift apart: seen at f32, N = 512, M = 1.)
    assert np.array_equal(bits(dg1), bits(dg2)) and np.array_equal(bits(db1), bits(db2)), tag + ": dgamma / dbeta differ from mmvae_bn_bwd_finalize"
    inside(host(dg1), E.accum(old_g, sdx, F64), E.accum_tol(old_g, sdx), tag + " dgamma")
    inside(host(db1), E.accum(old_b, sd, F64), E.accum_tol(old_b, sd), tag + " dbeta")
    assert (d1[:, N:] == 3.0).all() and (d2[:, N:] == 3.0).all(), "columns past N were written"
    apart = ulps_apart(d1[:, :N], d2[:, :N])
    print(f"{tag}: fused against two launches: {'bit-identical' if apart == 0 else f'{apart} ulp apart'}")
    assert apart <= 1
    c64 = E.bn_bwd_coefs(sd, sdx, M, gamma, rstd, eval_mode, F64)
    ctol = E.bn_bwd_coefs_tol(sd, sdx, M, gamma, rstd, eval_mode)
    ref, tol = E.bn_bwd_apply(d, y, mean, rstd, c64, F64), E.bn_bwd_apply_tol(d, y, mean, rstd, c64, ctol)
    for got, name in ((d1, "fused"), (d2, "two launches")):
        inside(host(got[:, :N]), ref, tol if dt == torch.float32 else E.bf16_out(tol, ref), f"{tag} {name} against float64")


def test_bn_bwd_finalize_apply_refuses_other_widths():
    M = 8
    for dt, code, N in ((torch.bfloat16, L.BF16, 192), (torch.float32, L.F32, 96), (torch.bfloat16, L.BF16, 60), (torch.float32, L.F32, 30)):
        d, y = torch.full((M, N), 2.0, dtype=dt, device=DEV), torch.full((M, N), 1.0, dtype=dt, device=DEV)
        vec = [torch.full((N,), 5.0, device=DEV) for _ in range(5)]          # mean, rstd, gamma, dgamma, dbeta
        stats = torch.ones((2, N), dtype=torch.float64, device=DEV)
        before = [snapshot(t) for t in [d] + vec]
        rc = L.load().mmvae_bn_bwd_finalize_apply(code, M, N, d.data_ptr(), N, y.data_ptr(), N, vec[0].data_ptr(), vec[1].data_ptr(),
                                                  stats[0].data_ptr(), stats[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(),
                                                  vec[4].data_ptr(), 0, stream())
        assert rc == ERR_ARG, (dt, N)
        torch.cuda.synchronize()
        assert all(unchanged(t, b) for t, b in zip([d] + vec, before))


# =============================================================================================
# weight preparation
# =============================================================================================
def test_prep_weights_table():
    rng = np.random.default_rng(6)
    items, checks, keep = [], [], []

    def source(rows, cols, pad):
        x = rnd(rng, rows, cols)
        flat = x.reshape(-1)
        ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** -100, 3.0e38, 0.0, -0.0, np.inf, -np.inf], F32)
        flat[:min(len(ties), flat.size)] = ties[:flat.size]          # bf16 rounding ties (to even), large and small magnitudes
        v = strided(x, pad, fill=7.0)                                # a wider source buffer: src_ld > src_cols
        keep.append(v)
        return x, v

    def dest(rows, cols, dt):
        buf = torch.full((rows + 2, cols + 8), NAN, dtype=dt, device=DEV)
        keep.append(buf)
        return buf

    def add(x, v, buf, r0, c0, dst_rows, dst_cols, transpose, expect):
        es = buf.element_size()
        items.append(L.PrepItem(v.data_ptr(), buf.data_ptr() + (r0 * buf.stride(0) + c0) * es, x.shape[0], x.shape[1], v.stride(0),
                                dst_rows, dst_cols, buf.stride(0), int(transpose), ops._dt(buf)))
        src = x.T if transpose else x
        blk = np.zeros((dst_rows, dst_cols), F32)
        blk[:min(src.shape[0], dst_rows), :min(src.shape[1], dst_cols)] = src[:dst_rows, :dst_cols]
        expect[r0:r0 + dst_rows, c0:c0 + dst_cols] = blk

    def expectation(buf):
        e = np.full(tuple(buf.shape), np.nan, F32)
        checks.append((buf, e))
        return e

    for dt in (torch.bfloat16, torch.float32):
        # plain and transposed copies of a 20 x 782 weight into its padded operands
        x, v = source(20, 782, 2)
        b = dest(128, 832, dt); add(x, v, b, 0, 0, 128, 832, False, expectation(b))
        b = dest(896, 64, dt); add(x, v, b, 0, 0, 896, 64, True, expectation(b))
        # two heads concatenated: rows [0, 20) and [20, 128) of one operand (the last item clears the padding rows); transposed:
        # columns [0, 20) and [20, 64) of the other
        (x1, v1), (x2, v2) = source(20, 33, 0), source(20, 33, 3)
        b = dest(128, 64, dt); e = expectation(b)
        add(x1, v1, b, 0, 0, 20, 64, False, e); add(x2, v2, b, 20, 0, 108, 64, False, e)
        b = dest(128, 64, dt); e = expectation(b)
        add(x1, v1, b, 0, 0, 128, 20, True, e); add(x2, v2, b, 0, 20, 128, 44, True, e)
        # 1 x 1 and 33 x 65: nothing is a multiple of the 32 x 32 tile; destinations smaller than a tile and smaller than the source
        x, v = source(1, 1, 0)
        b = dest(1, 1, dt); add(x, v, b, 0, 0, 1, 1, False, expectation(b))
        b = dest(3, 2, dt); add(x, v, b, 0, 0, 3, 2, True, expectation(b))
        x, v = source(33, 65, 1)
        b = dest(33, 65, dt); add(x, v, b, 0, 0, 33, 65, False, expectation(b))
        b = dest(65, 33, dt); add(x, v, b, 0, 0, 65, 33, True, expectation(b))
        b = dest(40, 30, dt); add(x, v, b, 0, 0, 40, 30, True, expectation(b))      # crops columns, pads rows
    arr = (L.PrepItem * len(items))(*items)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    assert L.load().mmvae_prep_weights(table.data_ptr(), len(items), stream()) == 0
    torch.cuda.synchronize()
    for buf, e in checks:
        want = torch.from_numpy(e).to(buf.dtype)                  # torch's own rounding to the destination type
        got = buf.cpu()
        written = ~np.isnan(e)
        assert torch.isnan(got[torch.from_numpy(~written)]).all(), "written outside [dst_rows][dst_cols]"
        assert np.array_equal(bits(got)[written], bits(want)[written]), f"prep_weights: {tuple(buf.shape)} {buf.dtype} differs from torch's rounding"
    assert L.load().mmvae_prep_weights(table.data_ptr(), 0, stream()) == ERR_ARG
    assert L.load().mmvae_prep_weights(None, 3, stream()) == ERR_ARG


# =============================================================================================
# sigmoid backward, scaling, loss finalisation
# =============================================================================================
@pytest.mark.parametrize("ldo_extra", [0, 3, 11])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_sigmoid_bwd(dtype, ldo_extra):
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    rng = np.random.default_rng(7)
    for M, N in ((37, 45), (1, 1), (130, 64)):
        g, p = rnd(rng, M, N), rng.uniform(0, 1, (M, N)).astype(F32)
        if p.size > 4:
            p.reshape(-1)[:4] = [0.0, 1.0, 1e-7, 1 - 2.0 ** -24]
        ldo = N + ldo_extra
        out = torch.full((M, ldo), NAN, dtype=dt, device=DEV)
        assert ops._ld(out[:, :N]) == ldo
        ops.sigmoid_bwd(strided(g, 3), strided(p, 5), out[:, :N])
        ref, tol = E.sigmoid_bwd(g, p, F64), E.sigmoid_bwd_tol(g, p)
        inside(host(out[:, :N]), ref, tol if dt == torch.float32 else E.bf16_out(tol, ref), f"sigmoid_bwd {dtype} {M}x{N} ldo {ldo}")
        Np = min(ops.ceil_to(N, 8), ldo)            # the GEMM operand contract: zeros up to the next multiple of 8, inside the row
        assert (bits(out[:, N:Np]) == 0).all() and torch.isnan(out[:, Np:]).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_scale_if_needed(dtype):
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    rng = np.random.default_rng(8)
    for n in (1, 255, 2048 * 256 + 77):             # the last: past one pass of the 2048-block grid
        x_np = rnd(rng, n)
        buf = torch.full((n + 16,), 3.0, dtype=dt, device=DEV)
        buf[:n] = dev(x_np).to(dt)
        idt = torch.int32 if dt == torch.float32 else torch.int16
        buf[:n].view(idt)[n // 2] = 0x7FC12345 if dt == torch.float32 else 0x7FC5          # a NaN with a payload
        before = snapshot(buf)
        ops.scale_if_needed(buf[:n], torch.ones(1, device=DEV))
        torch.cuda.synchronize()
        assert unchanged(buf, before), "*scale == 1 must leave every bit alone"
        buf[:n].view(idt)[n // 2] = 0
        x = host(buf[:n])
        s = F32(0.37123)
        ops.scale_if_needed(buf[:n], dev(np.array([s])))
        ref, tol = x * float(s), E.scale_tol(x, s)
        inside(host(buf[:n]), ref, tol if dt == torch.float32 else E.bf16_out(tol, ref), f"scale_if_needed {dtype} n{n}")
        assert (buf[n:] == 3.0).all()


def test_scale_many():
    rng = np.random.default_rng(9)
    sizes = [1, 7, 255, 256, 1000, 2048 * 256 + 5, 33, 4097]
    dts = [torch.float32, torch.bfloat16] * 4
    bufs = []
    for n, dt in zip(sizes, dts):
        b = torch.full((n + 8,), 3.0, dtype=dt, device=DEV)
        b[:n] = dev(rnd(rng, n)).to(dt)
        bufs.append(b)
    bufs[0].view(torch.int32)[0] = 0x7FC12345
    before = [snapshot(b) for b in bufs]
    views = [b[:n] for b, n in zip(bufs, sizes)]
    ops.scale_many(views, torch.ones(1, device=DEV))
    torch.cuda.synchronize()
    assert all(unchanged(b, s) for b, s in zip(bufs, before)), "*scale == 1 must leave every bit alone"
    bufs[0].view(torch.int32)[0] = 0x3F800000
    xs = [host(v) for v in views]
    s = F32(-1.7312)
    sc = dev(np.array([s]))
    ops.scale_many(views, sc)
    for v, x, b, n in zip(views, xs, bufs, sizes):
        ref, tol = x * float(s), E.scale_tol(x, s)
        inside(host(v), ref, tol if v.dtype == torch.float32 else E.bf16_out(tol, ref), f"scale_many {v.dtype} n{n}")
        assert (b[n:] == 3.0).all()
    # nine records, a null pointer, an empty tensor: refused, nothing scaled
    before = [snapshot(b) for b in bufs]
    nine = (L.ScaleItem * 9)(*[L.ScaleItem(views[i % 8].data_ptr(), sizes[i % 8], ops._dt(views[i % 8]), 0) for i in range(9)])
    assert L.load().mmvae_scale_many(nine, 9, sc.data_ptr(), stream()) == ERR_ARG
    two = (L.ScaleItem * 2)(L.ScaleItem(views[2].data_ptr(), sizes[2], L.F32, 0), L.ScaleItem(views[3].data_ptr(), 0, L.BF16, 0))
    assert L.load().mmvae_scale_many(two, 2, sc.data_ptr(), stream()) == ERR_ARG
    two[1] = L.ScaleItem(None, 5, L.BF16, 0)
    assert L.load().mmvae_scale_many(two, 2, sc.data_ptr(), stream()) == ERR_ARG
    assert L.load().mmvae_scale_many(two, 1, None, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert all(unchanged(b, s) for b, s in zip(bufs, before))


@pytest.mark.parametrize("on_device", [False, True], ids=["by_value", "beta_gamma_dev"])
def test_loss_finalize(on_device):
    sums_np = np.array([1234.56789012345, 987.654321, 3.14159265358979, 42.4242424242, 3.0])       # 3 labels out of range, passed through
    beta, gamma = F32(1e-3), F32(0.7)
    sums, out = dev(sums_np), torch.full((6,), NAN, device=DEV)
    bg = dev(np.array([beta, gamma])) if on_device else None
    ops.loss_finalize(sums, 123.0 if on_device else float(beta), -5.0 if on_device else float(gamma), out, beta_gamma_dev=bg)
    ref = E.loss_finalize(sums_np, beta, gamma, F64)
    assert ref[1] == sums_np[0] + sums_np[1] and ref[4] == 3.0       # {total, recon, class, kld, bad labels}: the order of the header
    want_total = sums_np[0] + sums_np[1] + float(gamma) * sums_np[2] + float(beta) * sums_np[3]
    assert abs(ref[0] - want_total) <= 1e-12 * want_total
    inside(host(out[:5]), ref, E.loss_finalize_tol(sums_np, beta, gamma), "loss_finalize")
    assert out[4].item() == 3.0 and torch.isnan(out[5])
    assert np.array_equal(sums.cpu().numpy(), sums_np)               # the sums are read, not consumed
    assert L.load().mmvae_loss_finalize(None, 1.0, 1.0, None, out.data_ptr(), stream()) == ERR_ARG


# =============================================================================================
# multi-tensor AdamW at the ABI
# =============================================================================================
ADAMW_SIZES = [1, 255, 1024, 1025, 262144 * 4 + 3]        # the last: past 256 blocks x 4 x 256 elements: the strided loop, clamped loads
HP = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-8)


class AdamWCase:
    """n_tensors tensors carved out of four flat buffers (p, g, m, v): the five sizes above, then small ones of unequal lengths.  Every
    fourth tensor has SMALL gradients and second moments (sqrt(v') of the order of eps ... 1e-4: the eps of the denominator decides the
    update), and a few elements have g = 0, v = 0 with m != 0 (the denominator is eps alone)."""

    def __init__(self, n_tensors, seed):
        rng = np.random.default_rng(seed)
        self.sizes = (ADAMW_SIZES + [1 + (37 * i) % 300 for i in range(n_tensors)])[:n_tensors]
        self.offs = np.concatenate([[0], np.cumsum(self.sizes)])
        n = int(self.offs[-1])
        p, g, m, v = rnd(rng, n), rnd(rng, n, scale=0.1), rnd(rng, n, scale=0.05), rng.uniform(1e-6, 1e-2, n).astype(F32)
        for i in range(3, n_tensors, 4):
            s = slice(self.offs[i], self.offs[i + 1])
            g[s] *= 1e-3; m[s] *= 1e-3; v[s] = rng.uniform(1e-12, 1e-8, s.stop - s.start).astype(F32)
        for i in range(0, n_tensors, 5):
            o = self.offs[i]
            g[o] = 0.0; v[o] = 0.0; m[o] = F32(1e-6)
        self.np = dict(p=p, g=g, m=m, v=v)
        self.t = {k: dev(x) for k, x in self.np.items()}

    def items(self, n=None):
        n = len(self.sizes) if n is None else n
        arr = (L.AdamWItem * n)()
        for i in range(n):
            o, sz = int(self.offs[i]), self.sizes[i]
            arr[i] = L.AdamWItem(*(self.t[k].data_ptr() + 4 * o for k in "pgmv"), sz)
        return arr

    def check(self, t, wd, maximize, device_bc, tag, lr=None):
        """Device state against oracle/np_oracle.adamw_step in float64 at step count t (1-based)."""
        f = lambda x: float(F32(x))
        hp = dict(HP, lr=HP["lr"] if lr is None else lr)
        n = int(self.offs[len(self.sizes)])
        P = {"w": self.np["p"].astype(F64)}
        st = {"w": dict(m=self.np["m"].astype(F64), v=self.np["v"].astype(F64))}
        g = self.np["g"].astype(F64)
        O.adamw_step(P, {"w": -g if maximize else g}, st, t - 1, lr=f(hp["lr"]), wd=f(wd), b1=f(hp["b1"]), b2=f(hp["b2"]), eps=f(hp["eps"]))
        tol = E.adamw_tol(self.np["p"], self.np["g"], self.np["m"], self.np["v"], t, wd=wd, maximize=maximize, device_bc=device_bc, **hp)
        for ref, tl, k in ((P["w"], tol[0], "p"), (st["w"]["m"], tol[1], "m"), (st["w"]["v"], tol[2], "v")):
            inside(host(self.t[k])[:n], ref[:n], tl[:n], f"adamw {tag} {k}")
        assert np.array_equal(self.t["g"].cpu().numpy(), self.np["g"]), "the gradients were written"


def _adamw_call(items, n, lr, wd, bc1, bc2, maximize, step_dev, advance, lr_dev):
    return L.load().mmvae_adamw_step(C.cast(items, C.c_void_p), n, lr, HP["b1"], HP["b2"], HP["eps"], wd, bc1, bc2, int(maximize),
                                     ops._p(step_dev), int(advance), ops._p(lr_dev), stream())


@pytest.mark.parametrize("wd,maximize", [(0.0, False), (1e-2, True)], ids=["plain", "wd+maximize"])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adamw_host_bias_corrections_70_tensors(t, wd, maximize):
    case = AdamWCase(70, seed=t)                  # two launches: 64 + 6 tensors
    bc1, bc2 = 1.0 - float(F32(HP["b1"])) ** t, 1.0 - float(F32(HP["b2"])) ** t
    assert _adamw_call(case.items(), 70, HP["lr"], wd, bc1, bc2, maximize, None, False, None) == 0
    case.check(t, wd, maximize, False, f"host t{t} wd{wd}")


@pytest.mark.parametrize("t0", [0, 1, 999])
def test_adamw_device_counter_without_advance_70_tensors(t0):
    case = AdamWCase(70, seed=10 + t0)
    ctr = torch.tensor([5, t0, 5], dtype=torch.int64, device=DEV)           # ONE word: read by every workgroup of both launches
    assert _adamw_call(case.items(), 70, HP["lr"], 1e-2, 0.0, -1.0, False, ctr[1:2], False, None) == 0      # bias_corr arguments ignored
    case.check(t0 + 1, 1e-2, False, True, f"device counter t0 {t0}")
    assert ctr.tolist() == [5, t0, 5], "without advance the counter is only read"
    ops.counter_add(ctr[1:2], 1)
    assert ctr.tolist() == [5, t0 + 1, 5]


@pytest.mark.parametrize("n_tensors", [5, 64])
@pytest.mark.parametrize("t0", [0, 1, 999])
def test_adamw_device_counter_with_advance(t0, n_tensors):
    case = AdamWCase(n_tensors, seed=20 + t0)
    ctr = torch.full((L.CTR_COPIES,), t0, dtype=torch.int64, device=DEV)
    lr_dev = dev(np.array([HP["lr"]], F32))
    assert _adamw_call(case.items(), n_tensors, 123.0, 0.0, 1.0, 1.0, True, ctr, True, lr_dev) == 0          # lr_dev overrides lr
    case.check(t0 + 1, 0.0, True, True, f"advance t0 {t0} n{n_tensors}")
    got = ctr.cpu().numpy()
    assert (got == t0 + 1).all(), f"{int((got != t0 + 1).sum())} of {L.CTR_COPIES} copies of the step count are not {t0 + 1}"


def test_adamw_through_ops_wrapper_keeps_the_copies_identical():
    for n_tensors in (5, 70):                     # <= 64: the launch ticks; beyond: the wrapper advances the copies after the launches
        case = AdamWCase(n_tensors, seed=30)
        ctr = torch.full((L.CTR_COPIES,), 999, dtype=torch.int64, device=DEV)
        ops.adamw_step(case.items(), HP["lr"], HP["b1"], HP["b2"], HP["eps"], 1e-2, 1.0, 1.0, step_dev=ctr)
        case.check(1000, 1e-2, False, True, f"ops wrapper n{n_tensors}")
        assert (ctr == 1000).all()


def test_adamw_refusal_enqueues_nothing():
    """A call that returns MMVAE_ERR_ARG has enqueued NOTHING (include/mmvae_hip.h): 65 records whose LAST one is invalid must not
    step the 64 tensors of the first launch."""
    for what in ("n = 0", "null pointer"):
        case = AdamWCase(65, seed=40)
        before = {k: snapshot(v) for k, v in case.t.items()}
        items = case.items()
        if what == "n = 0":
            items[64].n = 0
        else:
            items[64].m = None
        assert _adamw_call(items, 65, HP["lr"], 1e-2, 0.1, 0.001, False, None, False, None) == ERR_ARG, what
        torch.cuda.synchronize()
        for k, v in case.t.items():
            assert unchanged(v, before[k]), f"{what}: refused, but `{k}` of the first 64 tensors was stepped"
    # one launch = one tick: advance with more than 64 tensors is refused, the counter and the tensors stay
    case = AdamWCase(65, seed=41)
    before = {k: snapshot(v) for k, v in case.t.items()}
    ctr = torch.full((L.CTR_COPIES,), 7, dtype=torch.int64, device=DEV)
    assert _adamw_call(case.items(), 65, HP["lr"], 0.0, 1.0, 1.0, False, ctr, True, None) == ERR_ARG
    assert _adamw_call(case.items(), 5, HP["lr"], 0.0, 1.0, 1.0, False, None, True, None) == ERR_ARG         # advance without a counter
    assert _adamw_call(case.items(), 5, HP["lr"], 0.0, 0.0, 1.0, False, None, False, None) == ERR_ARG        # bias correction 0
    assert _adamw_call(case.items(), 0, HP["lr"], 0.0, 1.0, 1.0, False, None, False, None) == ERR_ARG
    torch.cuda.synchronize()
    assert (ctr == 7).all() and all(unchanged(v, before[k]) for k, v in case.t.items())
