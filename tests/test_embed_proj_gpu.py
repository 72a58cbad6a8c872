"""mmvae_embed_proj_fwd / _bwd -- the autoencoders' Embedding -> Linear(embed, latent) table, the one-head case of EncoderC's table
kernels -- one launch at a time against float64, held to the derived bounds of tests/ae_bounds.py (elementwise_bounds.embed_* with an
empty second head).  The backward runs with 1, 8 and 11 scatter copies onto non-zero old gradients, on both sides of the default
dynamic-LDS limit (64 KiB) and up to the capacity (160 KiB); what the entry point refuses (operands beyond that) must leave every
output untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ae_bounds as AB  # noqa: E402
import ae_oracle as AO  # noqa: E402
from test_elementwise_gpu import dev, host, rnd, inside, snapshot, unchanged, NAN, DEV, F64  # noqa: E402
from mmvae import _lib as L  # noqa: E402
from mmvae import ops  # noqa: E402

# (64, 32, 160): 68 KiB of operands, the first size past the default dynamic-LDS limit (refused until the launch learnt to raise it);
# (24, 64, 100): the corner of the reference's hyperparameter search; (76, 64, 256): 159 KiB, the last size the CU's LDS holds
SHAPES = [(24, 32, 20), (5, 16, 7), (1, 32, 1), (64, 32, 160), (24, 64, 100), (76, 64, 256)]


def _params(rng, S, Ed, Ld):
    return rnd(rng, S, Ed), rnd(rng, Ld, Ed, scale=0.3), rnd(rng, Ld, scale=0.5)


@pytest.mark.parametrize("S,Ed,Ld", SHAPES)
def test_embed_proj_fwd(S, Ed, Ld):
    rng = np.random.default_rng(S * 100 + Ld)
    emb, w, b = _params(rng, S, Ed, Ld)
    table = torch.full((S + 1, Ld), NAN, device=DEV)
    ops.embed_proj_fwd(dev(emb), dev(w), dev(b), table)
    ref = AB.proj_fwd(emb, w, b, F64)
    assert np.allclose(ref, emb.astype(F64) @ w.astype(F64).T + b, rtol=1e-12, atol=1e-13)
    inside(host(table[:S]), ref, AB.proj_fwd_tol(emb, w, b), f"embed_proj_fwd {S, Ed, Ld}")
    assert torch.isnan(table[S]).all()


@pytest.mark.parametrize("copies", [1, 8, 11])
@pytest.mark.parametrize("S,Ed,Ld", SHAPES)
def test_embed_proj_bwd(S, Ed, Ld, copies):
    rng = np.random.default_rng(S * 100 + Ld + copies)
    emb, w, b = _params(rng, S, Ed, Ld)
    dT = [rnd(rng, S, Ld) for _ in range(copies)]
    old = (rnd(rng, S, Ed), rnd(rng, Ld, Ed), rnd(rng, Ld))                       # the gradients are ACCUMULATED into
    d_emb, d_w, d_b = dev(old[0]), dev(old[1]), dev(old[2])
    ops.embed_proj_bwd(dev(emb), dev(w), dev(np.stack(dT)), d_emb, d_w, d_b)
    ref, tol = AB.proj_bwd(dT, emb, w, old, F64), AB.proj_bwd_tol(dT, emb, w, old)
    # the oracle's site path on the table gradient as if every class were one sample
    P = {"site_embedding.weight": emb.astype(F64), "site_projection.weight": w.astype(F64), "site_projection.bias": b.astype(F64)}
    dTs = np.sum([d.astype(F64) for d in dT], 0)
    de, gw, gb = AO.O._linear_bwd(dTs, P["site_embedding.weight"], P["site_projection.weight"])
    assert np.allclose(ref[0] - old[0], de, rtol=1e-9, atol=1e-11) and np.allclose(ref[1] - old[1], gw, rtol=1e-9, atol=1e-11)
    assert np.allclose(ref[2] - old[2], gb, rtol=1e-9, atol=1e-11)
    tag = f"embed_proj_bwd {S, Ed, Ld} copies {copies}"
    inside(host(d_emb), ref[0], tol[0], tag + " d_emb")
    inside(host(d_w), ref[1], tol[1], tag + " d_w")
    inside(host(d_b), ref[2], tol[2], tag + " d_b")


def test_embed_proj_bwd_refuses_operands_beyond_the_cu_lds():
    S, Ed, Ld = 77, 64, 256                       # (S L + S E + L E) floats = 160.25 KiB; 76 sites (159 KiB) and 48 (124 KiB) are accepted
    assert (S * Ld + S * Ed + Ld * Ed) * 4 > 160 * 1024 >= (76 * Ld + 76 * Ed + Ld * Ed) * 4
    rng = np.random.default_rng(4)
    emb, w, b = _params(rng, S, Ed, Ld)
    outs = [torch.full(s, 5.0, device=DEV) for s in ((S, Ed), (Ld, Ed), (Ld,))]
    before = [snapshot(t) for t in outs]
    with pytest.raises(L.MMVAEArgError):
        ops.embed_proj_bwd(dev(emb), dev(w), dev(rnd(rng, S, Ld)), *outs)
    torch.cuda.synchronize()
    assert all(unchanged(t, b_) for t, b_ in zip(outs, before))
    emb48 = emb[:48]
    ops.embed_proj_bwd(dev(emb48), dev(w), dev(rnd(rng, 48, Ld)), torch.zeros(48, Ed, device=DEV), outs[1], outs[2])      # accepted
    torch.cuda.synchronize()
