"""mmvae.reconstruct.Reconstructor on both directional VAEs at small widths (inputs 40 / 24, latent 8, 5 sites, B = 37).

One draw is the plain forward, bit for bit.  Several draws / all sites are compared with the float64 mean and ddof-1 std of the G
separate model(...) calls, each fed its own slice of the injected eps and its site.  The tolerance is the derived bound of the last
GEMM (tests/group_moments_bounds.py): the encoder, the fusion and the decoder's hidden layers are the same kernels on the same row
values in both, so only the last layer differs -- the model's stored x_g and the fused kernel's x_g each lie within tol_x of the
exact product, i.e. within 2 tol_x of each other, and the moments' bound is taken at that."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_bounds as GB  # noqa: E402
import group_moments_bounds as MB  # noqa: E402
from gemm_gpu_util import DEV, host, within  # noqa: E402
from mmvae import _lib as L, engine, ops  # noqa: E402
from mmvae.reconstruct import Reconstructor  # noqa: E402
from src.models import DNA2RNAVAE, RNA2DNAVAE  # noqa: E402

RNA, DNA, SITES, LATENT, B = 40, 24, 5, 8, 37
KINDS = {"rna2dna": (RNA2DNAVAE, RNA), "dna2rna": (DNA2RNAVAE, DNA)}
_made = {}


def setup(kind):
    """(model, reconstructor, x, site), made once per kind"""
    if kind not in _made:
        cls, in_dim = KINDS[kind]
        torch.manual_seed(11)
        model = cls(RNA, DNA, SITES, LATENT).to(DEV).set_precision("bf16").eval()
        g = torch.Generator().manual_seed(12)
        x = torch.rand(B, in_dim, generator=g).to(DEV)
        site = torch.randint(0, SITES, (B,), generator=g).to(DEV)
        _made[kind] = (model, Reconstructor(model), x, site)
    return _made[kind]


def eps_for(rows, seed):
    return torch.randn(rows, LATENT, generator=torch.Generator().manual_seed(seed))


class injected:
    def __init__(self, eps):
        self.eps = eps

    def __enter__(self):
        engine.GLOBAL_NOISE.inject([], self.eps)

    def __exit__(self, *exc):
        engine.GLOBAL_NOISE.clear()
        return False


class last_layer_operand:
    """Records the operand of the decoder's last layer: of the fused launch, or (refuse=True: the launch answers MMVAE_ERR_ARG, as the
    library does for what it does not take) of the mmvae_gemm_nt with the fp32 output that replaces it."""

    def __init__(self, monkeypatch, refuse=False):
        self.a, real_gm, real_nt = None, ops.gemm_nt_group_moments, ops.gemm_nt

        def gm(prec, a, *args, **kw):
            if refuse:
                raise L.MMVAEArgError("mmvae_gemm_nt_group_moments failed: invalid argument")
            self.a = a
            return real_gm(prec, a, *args, **kw)

        def nt(prec, a, w, N, K, out, **kw):
            if out.dtype == torch.float32 and a.dtype == torch.bfloat16 and K >= 64:
                self.a = a
            return real_nt(prec, a, w, N, K, out, **kw)
        monkeypatch.setattr(ops, "gemm_nt_group_moments", gm)
        monkeypatch.setattr(ops, "gemm_nt", nt)


def last_layer_x(rec, a):
    """float64 x and tol_x of the last layer on the recorded operand"""
    pl = rec.dec.pl[-1]
    act = ops.ACT_SIGMOID if rec.dec.final_sigmoid else ops.ACT_NONE
    return MB.x_ref_tol(host(a[:, :pl.K]), host(pl.w[:pl.N, :pl.K]), host(pl.bias), act)


def separate_calls(model, x, site_of, eps, G):
    """x_g of the G separate forwards, stacked in the reconstructor's row order -> float64 [B G][N]"""
    outs = []
    for g in range(G):
        with injected(eps.view(B, G, LATENT)[:, g].contiguous()), torch.no_grad():
            outs.append(host(model(x, site_of(g))[0]))
    return np.stack(outs, axis=1).reshape(B * G, -1)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("sites", ["given", "none"])
def test_one_draw_is_the_plain_forward_bit_for_bit(kind, sites):
    model, rec, x, site = setup(kind)
    s = site if sites == "given" else None
    eps = eps_for(B, 3)
    with injected(eps), torch.no_grad():
        want = model(x, s)[0]
    with injected(eps):
        got, std = rec.reconstruct(x, s, draws=1, sites=sites)
    assert std is None and torch.equal(got, want)
    assert not model.training


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("sites,draws", [("given", 3), ("all", 2)])
def test_draws_and_all_sites_against_separate_forwards(kind, sites, draws, monkeypatch):
    model, rec, x, site = setup(kind)
    G = rec.group_size(draws, sites)
    eps = eps_for(B * G, 4)
    rec_op = last_layer_operand(monkeypatch)
    with injected(eps):
        mean, std = rec.reconstruct(x, site if sites == "given" else None, draws=draws, sites=sites, return_std=True)
    torch.cuda.synchronize()
    assert rec.last_fused, "the fused launch must take these shapes"
    _, tol_x = last_layer_x(rec, rec_op.a)
    monkeypatch.undo()
    site_of = (lambda g: site) if sites == "given" else (lambda g: torch.full((B,), g // draws, dtype=torch.int64, device=DEV))
    xs = separate_calls(model, x, site_of, eps, G)
    m, tm, s, ts = MB.moments_tol(xs, 2 * tol_x, G)
    within(host(mean), m, tm, f"reconstruct {kind} {sites} draws {draws} mean")
    within(host(std), s, ts, f"reconstruct {kind} {sites} draws {draws} std")


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fused_and_unfused_paths_agree_within_the_bounds(kind, monkeypatch):
    """both against the float64 moments of the last layer on the operand they multiplied (the same values in both runs)"""
    model, rec, x, site = setup(kind)
    draws, G = 4, 4
    eps = eps_for(B * G, 5)
    results = {}
    for refuse in (False, True):
        rec_op = last_layer_operand(monkeypatch, refuse=refuse)
        with injected(eps):
            mean, std = rec.reconstruct(x, site, draws=draws, return_std=True)
        torch.cuda.synchronize()
        assert rec.last_fused == (not refuse)
        results[refuse] = (host(mean), host(std), host(rec_op.a))
        monkeypatch.undo()
    assert np.array_equal(results[False][2], results[True][2]), "the two paths must multiply the same hidden activations"
    m, tm, s, ts = MB.moments_tol(*last_layer_x(rec, torch.from_numpy(results[False][2]).to(DEV)), G)
    for refuse, name in ((False, "fused"), (True, "unfused")):
        within(results[refuse][0], m, tm, f"reconstruct {kind} {name} mean")
        within(results[refuse][1], s, ts, f"reconstruct {kind} {name} std")


def test_a_group_above_128_goes_through_the_fallback(monkeypatch):
    model, rec, x, site = setup("dna2rna")
    draws = 129
    rec_op = last_layer_operand(monkeypatch)
    with injected(eps_for(B * draws, 6)):
        mean, std = rec.reconstruct(x, sites="none", draws=draws, return_std=True)
    torch.cuda.synchronize()
    assert rec.last_fused is False
    m, tm, s, ts = MB.moments_tol(*last_layer_x(rec, rec_op.a), draws)
    within(host(mean), m, tm, "reconstruct G 129 (fallback) mean")
    within(host(std), s, ts, "reconstruct G 129 (fallback) std")


@pytest.mark.parametrize("kind,sites,draws", [("rna2dna", "given", 1), ("rna2dna", "given", 3), ("dna2rna", "all", 2)])
def test_batched_is_the_batches_in_one_stream_bit_for_bit(kind, sites, draws):
    """reconstruct_batched over 9 rows in batches of 4 (two full, one ragged) = reconstruct() over the same slices, concatenated, in ONE
    Philox stream from (seed, offset 0): the position is set before the first batch, not per batch; and a second call repeats it."""
    model, rec, x, site = setup(kind)                           # the noise position is kept per device: x.device, cuda:0, not "cuda"
    rows, batch, seed = 9, 4, 77
    x, site = x[:rows], site[:rows]
    xh = x.cpu().numpy()
    sh = site.cpu().numpy() if sites == "given" else None
    want_std = rec.group_size(draws, sites) > 1
    assert rec.group_size(draws, sites) == {"given": draws, "all": 10}[sites]
    seed0, pos0 = torch.initial_seed(), engine.GLOBAL_NOISE.state_dict(x.device)
    try:
        got = [rec.reconstruct_batched(xh, sh, draws=draws, sites=sites, batch_size=batch, seed=seed) for _ in range(2)]
        torch.manual_seed(seed)
        engine.GLOBAL_NOISE.load_state_dict({"offset": 0}, x.device)
        parts = [rec.reconstruct(x[i:i + batch], site[i:i + batch] if sites == "given" else None, draws=draws, sites=sites, return_std=want_std)
                 for i in range(0, rows, batch)]
    finally:
        torch.manual_seed(seed0)
        engine.GLOBAL_NOISE.load_state_dict(pos0, x.device)
    assert [p[0].shape[0] for p in parts] == [4, 4, 1]
    mean = torch.cat([p[0] for p in parts]).cpu().numpy()
    for m, s in got:
        assert m.dtype == np.float32 and m.shape == (rows, mean.shape[1]) and np.array_equal(m, mean)
        if want_std:
            assert s.dtype == np.float32 and np.array_equal(s, torch.cat([p[1] for p in parts]).cpu().numpy())
        else:
            assert s is None
    # the stream moves from batch to batch: were the position set per batch, equal rows of two batches would reconstruct equally
    twice = np.concatenate([xh[:batch], xh[:batch]])
    st = None if sh is None else np.concatenate([sh[:batch], sh[:batch]])
    try:
        m2, _ = rec.reconstruct_batched(twice, st, draws=draws, sites=sites, batch_size=batch, seed=seed)
    finally:
        torch.manual_seed(seed0)
        engine.GLOBAL_NOISE.load_state_dict(pos0, x.device)
    assert np.array_equal(m2[:batch], mean[:batch]) and not np.array_equal(m2[batch:], m2[:batch])


def test_value_errors():
    model, rec, x, site = setup("rna2dna")
    with pytest.raises(ValueError):
        rec.reconstruct(x, site, draws=1, return_std=True)
    with pytest.raises(ValueError):
        rec.reconstruct(x, draws=2)                              # sites="given" without a site
    with pytest.raises(ValueError):
        rec.reconstruct(x, site, draws=2, sites="all")
    with pytest.raises(ValueError):
        rec.reconstruct(x, site, sites="none")
    with pytest.raises(ValueError):
        rec.reconstruct(x, site, sites="best")
    with pytest.raises(ValueError):
        rec.reconstruct(x, site, draws=0)
