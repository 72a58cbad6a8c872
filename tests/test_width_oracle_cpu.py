"""The oracles at the widths of tests/width_cases.py, on the CPU.  oracle/np_oracle.py is pinned against the reference's recorded
vectors only at the fixture widths (24 / 40 / 5 / 4 / 8 and 782 / 572 / 24 / 20 / 32); the device tests of
tests/test_width_space_gpu.py lean on it at odd input widths, odd and large latents, 5 to 33 sites and embed widths 8 to 64.

For every row, B = 16:
  * one full step of np_oracle (forward, loss with class weights, backward, BatchNorm buffers) against float64 autograd of
    oracle/torch_ref.py (stock torch ops) on the same parameters, inputs, masks and eps, at the tolerances
    tests/test_oracle_vs_golden.py::test_partial_modality_backward_matches_autograd uses for that comparison: loss 1e-12, outputs
    1e-9 / 1e-12, every gradient 1e-9 Frobenius-relative, buffers 1e-12 (of the tensor's scale: _check_buffers);
  * the `q` code path with the identity hook against the fp64 path, as tests/test_oracle_q_vs_golden.py does (outputs 1e-12, the loss
    floats equal, gradients 1e-9).
The directional VAEs (np_oracle.directional_train_step) and the autoencoders (tests/ae_oracle.py) the same at the three rows they
run at on the device; the autoencoders' autograd side is restated here from stock torch ops (directional_ae.py:46-64).
Besides: the table's statements that need no device -- each row's limits against the library's documented ones, and the parameter
behind which the gradient arena loses its 8-byte alignment against VAEGraph.param_list()."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ae_oracle as AO
import np_oracle as O
import torch_ref as T
import width_cases as W

F64 = np.float64
CHAOTIC_BIASES = ("encoder_a.fc.0.bias", "encoder_b.fc.0.bias", "encoder_b.fc.4.bias")     # analytically zero gradients
BETA, GAMMA = 1e-3, 0.7
B = W.CPU_B
IDS = [r.id for r in W.ROWS]


def _data(row, seed=40):
    A, D, S, L, E = row.dims
    P, Bf = O.make_params(seed, A, D, S, L, E)
    a, b, site = O.make_batch(seed + 1, B, A, D, S)
    masks, eps = O.make_noise(seed + 2, B, L)
    cw = np.random.default_rng(seed + 3).uniform(0.5, 2.0, S)
    return O.cast_tree(P, F64), O.cast_tree(Bf, F64), a.astype(F64), b.astype(F64), site, masks, eps.astype(F64), cw


def _torch_state(P, Bf):
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in P.items()}
    bufs = {k: torch.tensor(np.asarray(v)) for k, v in Bf.items()}
    return p, bufs


def _check_grads(G, p, zero_scale):
    """np gradients G against the autograd gradients of the tensors p: the same set, each to 1e-9 Frobenius-relative."""
    assert {k for k, t_ in p.items() if t_.grad is not None} == set(G)
    worst = 0.0
    for k, g in G.items():
        want = p[k].grad.numpy()
        assert g.shape == want.shape, k
        if k in CHAOTIC_BIASES:             # analytically zero: rounding noise on both sides, measured against the layer's weight gradient
            assert np.abs(g - want).max() <= 1e-9 * zero_scale, k
            continue
        err = float(np.linalg.norm(g - want) / np.linalg.norm(want))
        worst = max(worst, err)
        assert err <= 1e-9, (k, err)
    return worst


def _check_buffers(Bf1, bufs):
    """BatchNorm buffers after the step: 1e-12 relative, or 1e-12 of the tensor's largest element -- an element of a running mean is
    a cancelling sum of up to 1211 products and may come out a thousand times smaller than them, so its rounding error (the order
    of the float64 additions differs between numpy and torch) is bounded against the tensor's scale, not against the element."""
    for k, v in Bf1.items():
        want = bufs[k].numpy()
        np.testing.assert_allclose(v, want, rtol=1e-12, atol=1e-12 * float(np.abs(want).max()), err_msg=k)


def _check_identity(r0, ri, out_keys, loss_keys, zero_scale):
    for k in out_keys:
        np.testing.assert_allclose(ri[k], r0[k], rtol=1e-12, atol=0)
    for k in loss_keys:
        assert abs(ri[k] - r0[k]) <= 1e-12 * abs(r0[k]), k
    assert set(ri["grads"]) == set(r0["grads"])
    for k, g in r0["grads"].items():
        if k in CHAOTIC_BIASES:
            assert np.abs(ri["grads"][k]).max() <= 1e-9 * max(1.0, zero_scale)
            continue
        assert np.linalg.norm(ri["grads"][k] - g) <= 1e-9 * np.linalg.norm(g), k


@pytest.mark.parametrize("rid", IDS)
def test_multimodal_step_matches_autograd(rid):
    row = W.BY_ID[rid]
    P, Bf, a, b, site, masks, eps, cw = _data(row)
    p, bufs = _torch_state(P, Bf)
    tm = {k: torch.from_numpy(v).double() for k, v in masks.items()}
    ta, tb, ts = torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(site)
    ra, rb, rc, mu, lv = T.forward(p, bufs, ta, tb, ts, True, tm, torch.from_numpy(eps))
    loss, rec, cls, kld = T.loss_fn(ra, ta, rb, tb, rc, ts, mu, lv, BETA, GAMMA, torch.from_numpy(cw))
    loss.backward()

    def step(q):
        P1, Bf1 = {k: v.copy() for k, v in P.items()}, dict(Bf)
        st, n = O.adamw_init(P1)
        return O.train_step(P1, Bf1, st, n, a, b, site, masks, eps, BETA, GAMMA, cw, q=q), Bf1
    r, Bf1 = step(None)
    np.testing.assert_allclose([r["total"], r["recon"], r["cls"], r["kld"]], [loss.item(), rec.item(), cls.item(), kld.item()], rtol=1e-12)
    for nm, t_ in (("out_a", ra), ("out_b", rb), ("out_c", rc), ("mu", mu), ("logvar", lv)):
        assert r[nm].shape == tuple(t_.shape)
        np.testing.assert_allclose(r[nm], t_.detach().numpy(), rtol=1e-9, atol=1e-12, err_msg=nm)
    assert len(r["grads"]) == 39
    worst = _check_grads(r["grads"], p, np.abs(r["grads"]["encoder_b.fc.0.weight"]).max())
    _check_buffers(Bf1, bufs)
    ri, _ = step(O._id)
    _check_identity(r, ri, ("out_a", "out_b", "out_c", "mu", "logvar"), ("total", "recon", "cls", "kld"),
                    np.abs(r["grads"]["encoder_b.fc.0.weight"]).max())
    print(f"{rid} {row.dims}: worst gradient Frobenius-rel against autograd {worst:.1e}")


@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
@pytest.mark.parametrize("rid", W.DIRECTIONAL_ROWS)
def test_directional_step_matches_autograd(rid, kind):
    row = W.BY_ID[rid]
    A, D, S, L, E = row.dims
    P, Bf, a, b, site, masks, eps, _ = _data(row, 50)
    x, tgt = (a, b) if kind == "rna2dna" else (b, a)
    ren = O.directional_param_names(kind, A, D, S, L, E)
    p, bufs = _torch_state({k: v for k, v in P.items() if k.split(".", 1)[0] in ren}, Bf)
    tm = {k: torch.from_numpy(v).double() for k, v in masks.items()}
    tx, tt, ts = torch.from_numpy(x), torch.from_numpy(tgt), torch.from_numpy(site)
    enc, idx = ("encoder_a", O.ENC_A_IDX) if kind == "rna2dna" else ("encoder_b", O.ENC_B_IDX)
    m1, l1 = T._encoder(tx, p, bufs, enc, idx, True, tm)
    h = F.embedding(ts, p["encoder_c.embedding.weight"])
    m2, l2 = F.linear(h, p["encoder_c.fc_mu.weight"], p["encoder_c.fc_mu.bias"]), F.linear(h, p["encoder_c.fc_logvar.weight"], p["encoder_c.fc_logvar.bias"])
    mu, lv = torch.stack([m1, m2]).mean(0), torch.stack([l1, l2]).mean(0)
    z = mu + torch.from_numpy(eps) * torch.exp(0.5 * lv)
    if kind == "rna2dna":
        out = T._decoder(z, p, "decoder_b", [0, 2, 4], True)
        rec = F.binary_cross_entropy(out, tt, reduction="sum")
    else:
        out = T._decoder(z, p, "decoder_a", [0, 2], False)
        rec = F.mse_loss(out, tt, reduction="sum")
    kld = -0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp())
    loss = rec + BETA * kld
    loss.backward()

    def step(q):
        P1, Bf1 = {k: v.copy() for k, v in P.items()}, dict(Bf)
        st, n = O.adamw_init(P1)
        return O.directional_train_step(kind, P1, Bf1, st, n, x, tgt, site, masks, eps, BETA, q=q), Bf1
    r, Bf1 = step(None)
    np.testing.assert_allclose([r["total"], r["recon"], r["kld"]], [loss.item(), rec.item(), kld.item()], rtol=1e-12)
    for nm, t_ in (("out", out), ("mu", mu), ("logvar", lv)):
        np.testing.assert_allclose(r[nm], t_.detach().numpy(), rtol=1e-9, atol=1e-12, err_msg=nm)
    wkey = enc + ".fc.0.weight"
    _check_grads(r["grads"], p, np.abs(r["grads"][wkey]).max())
    _check_buffers(Bf1, bufs)
    ri, _ = step(O._id)
    _check_identity(r, ri, ("out", "mu", "logvar"), ("total", "recon", "kld"), np.abs(r["grads"][wkey]).max())


def _ae_torch_forward(kind, p, bufs, x, site, masks):
    """RNA2DNAAE / DNA2RNAAE.forward (directional_ae.py:46-64) in training mode from stock torch ops, keyed by the state_dict names."""
    pre, bn_idx, head, dec, dec_idx, sig = AO.KINDS[kind]
    h = x
    for (li, bi, di) in bn_idx:
        y = F.linear(h, p[f"{pre}.{li}.weight"], p[f"{pre}.{li}.bias"])
        y = F.batch_norm(y, bufs[f"{pre}.{bi}.running_mean"], bufs[f"{pre}.{bi}.running_var"], p[f"{pre}.{bi}.weight"], p[f"{pre}.{bi}.bias"],
                         training=True, momentum=0.1, eps=1e-5)
        h = torch.relu(y) * masks[f"{pre}.{di}"] / (1.0 - O.DROP_P)
    lat_x = F.linear(h, p[f"{pre}.{head}.weight"], p[f"{pre}.{head}.bias"])
    lat_s = F.linear(F.embedding(site, p["site_embedding.weight"]), p["site_projection.weight"], p["site_projection.bias"])
    latent = torch.stack([lat_x, lat_s]).mean(0)
    h = latent
    for j, li in enumerate(dec_idx):
        h = F.linear(h, p[f"{dec}.fc.{li}.weight"], p[f"{dec}.fc.{li}.bias"])
        if j < len(dec_idx) - 1:
            h = torch.relu(h)
    return (torch.sigmoid(h) if sig else h), latent


@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
@pytest.mark.parametrize("rid", W.DIRECTIONAL_ROWS)
def test_autoencoder_step_matches_autograd(rid, kind):
    row = W.BY_ID[rid]
    A, D, S, L, E = row.dims
    P, Bf = AO.make_params(60, kind, A, D, S, L, E)
    a, b, site = O.make_batch(61, B, A, D, S)
    x, tgt = ((a, b) if kind == "rna2dna" else (b, a))
    x, tgt = x.astype(F64), tgt.astype(F64)
    rng = np.random.default_rng(62)
    masks = {n: (rng.random((B, w)) >= O.DROP_P).astype(np.uint8) for n, w in zip(AO.mask_names(kind), AO.HIDDEN[kind])}
    p, bufs = _torch_state(P, {k: v for k, v in Bf.items() if not k.endswith("num_batches_tracked")})
    out, latent = _ae_torch_forward(kind, p, bufs, torch.from_numpy(x), torch.from_numpy(site), {k: torch.from_numpy(v).double() for k, v in masks.items()})
    tt = torch.from_numpy(tgt)
    loss = F.binary_cross_entropy(out, tt, reduction="sum") if kind == "rna2dna" else F.mse_loss(out, tt, reduction="sum")
    loss.backward()

    def step(q):
        P1, Bf1 = {k: v.copy() for k, v in P.items()}, dict(Bf)
        st, n = O.adamw_init(P1)
        return AO.train_step(kind, P1, Bf1, st, n, x, tgt, site, masks, q=q), Bf1
    r, Bf1 = step(None)
    assert abs(r["total"] - loss.item()) <= 1e-12 * abs(loss.item())
    np.testing.assert_allclose(r["out"], out.detach().numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r["latent"], latent.detach().numpy(), rtol=1e-9, atol=1e-12)
    assert set(r["grads"]) == set(P)
    pre = AO.KINDS[kind][0]
    wscale = np.abs(r["grads"][pre + ".0.weight"]).max()
    zero = {f"{pre}.{li}.bias" for (li, _, _) in AO.KINDS[kind][1]}          # biases in front of a BatchNorm
    for k, g in r["grads"].items():
        want = p[k].grad.numpy()
        if k in zero:
            assert np.abs(g - want).max() <= 1e-9 * wscale, k
            continue
        assert np.linalg.norm(g - want) <= 1e-9 * np.linalg.norm(want), k
    _check_buffers({k: np.asarray(Bf1[k], F64) for k in bufs}, bufs)
    assert all(int(Bf1[k]) == 1 for k in Bf1 if k.endswith("num_batches_tracked"))
    ri, _ = step(O._id)
    np.testing.assert_allclose(ri["out"], r["out"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(ri["latent"], r["latent"], rtol=1e-12, atol=0)
    assert abs(ri["total"] - r["total"]) <= 1e-12 * abs(r["total"])
    for k, g in r["grads"].items():
        if k in zero:
            assert np.abs(ri["grads"][k]).max() <= 1e-9 * max(1.0, wscale)
            continue
        assert np.linalg.norm(ri["grads"][k] - g) <= 1e-9 * np.linalg.norm(g), k


# ----------------------------------------------------------------------------------------------------------------------------------
# the table's own statements
# ----------------------------------------------------------------------------------------------------------------------------------
def test_rows_are_what_the_table_says():
    assert len({r.id for r in W.ROWS}) == len(W.ROWS) == 11
    for r in W.ROWS:
        A, D, S, L, E = r.dims
        assert r.latent_fused == W.latent_fits(S, L), r.id
        assert r.class_tail == W.class_tail_fits(S, L), r.id
        assert r.B == 1000 or r.id == "big_batch"
    assert {r.misaligned_dw for r in W.ROWS} == {None, "decoder_a.fc.2.weight", "decoder_b.fc.2.weight"}
    d = {r.id: r.dims for r in W.ROWS}
    assert d["config"][:2] == (1177, 1211) and 1177 % 8 == 1 and 1211 % 8 == 3
    A, D, S, L, E = d["at_limits"]
    assert S * 2 * L == W.LAT_MAX_TABLE and S == 32 and W.latent_fits(S, L) and not W.latent_fits(S, L + 1) and not W.class_tail_fits(S + 4, L)
    A, D, S, L, E = d["past_table"]
    assert L <= W.LAT_MAX_L and S * 2 * L > W.LAT_MAX_TABLE >= (S - 4) * 2 * L
    assert d["past_latent"][3] == W.LAT_MAX_L + 1 and d["many_sites"][2] == 33 and d["many_sites"][3] == W.LAT_MAX_L
    A, D, S, L, E = d["corner"]
    assert (L, E) == (100, 64) and W.EMBED_RIDER_LDS < W.embed_bwd_lds(S, L, E) == 76544 <= W.EMBED_BWD_LDS
    # every other row's EncoderC backward fits the rider; the heads' dW is grouped exactly at the even latents
    assert all(W.embed_bwd_lds(r.dims[2], r.dims[3], r.dims[4]) <= W.EMBED_RIDER_LDS for r in W.ROWS if r.id != "corner")
    assert {r.id for r in W.ROWS if not W.heads_dw_grouped(r.dims[3])} == {"odd_latent", "past_latent", "odd_sites", "tiny_odd", "big_batch"}
    # the autoencoders at their three rows: fused below the limits only; the one head's dW grouped at L % 4 == 0 only
    assert [W.latent_fits(d[i][2], d[i][3], heads=1) for i in W.DIRECTIONAL_ROWS] == [True, False, False]
    assert [W.heads_dw_grouped(d[i][3], heads=1) for i in W.DIRECTIONAL_ROWS] == [False, False, True]
    # the reference's search space (optimize_hyperparameters.py:71-76) fits the enlarged EncoderC backward up to 106 sites
    assert W.embed_bwd_lds(106, 100, 64) <= W.EMBED_BWD_LDS < W.embed_bwd_lds(107, 100, 64)


@pytest.mark.parametrize("rid", IDS)
def test_arena_alignment_is_what_the_row_says(rid):
    """engine.carve_arena tiles the gradient arena by numel in VAEGraph.param_list() order: behind a parameter with an odd element
    count the gradient views are 4-byte aligned only, until the next odd one.  At least one row puts decoder_b's and one
    decoder_a's large dW targets there (test_rows_are_what_the_table_says)."""
    from src.models import MultiModalVAE
    row = W.BY_ID[rid]
    A, D, S, L, E = row.dims
    model = MultiModalVAE(A, D, S, L, embed_dim=E)
    names = {id(p): k for k, p in model.named_parameters()}
    plist = model._graph().param_list()
    assert len(plist) == 39
    order = [(names[id(p)], p.numel()) for p in plist]
    assert W.first_odd(order) == row.arena_odd_from, W.first_odd(order)
    off, odd_views = 0, []
    for k, n in order:
        if off % 2:
            odd_views.append(k)
        off += n
    big = next((k for k in odd_views if k.endswith("weight") and dict(order)[k] >= 16384), None)
    assert big == row.misaligned_dw, (big, odd_views)
    assert bool(odd_views) == (row.arena_odd_from is not None)
