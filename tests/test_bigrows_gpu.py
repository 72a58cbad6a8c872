"""Operands of 4 GiB and more: the scaled omics widths of BASELINE.json (RNA 20 000 / DNA 27 000 features) at the bench batch
of 65 536 rows per GPU put 5.2 GB and 7.1 GB fp32 inputs in front of kernels that address their row operands with 32-bit
offsets.  mmvae_gemm_nt / mmvae_gemm_tn process such operands in row blocks (include/mmvae_hip.h, mmvae_set_tuning key 3).

  * block invariance at a size the numpy oracle still covers elsewhere: a whole training step with the block size forced down to
    1 MiB (every GEMM of the step then runs in 256..2048-row blocks) against the same step unblocked;
  * the scaled widths at B = 65 536 themselves, through a size-independent property: in eval mode every row is independent and
    all loss terms are sums (src/utils/losses.py:8-46), so the gradient of the full batch (row-blocked path) must equal the sum
    of the gradients of its four quarters (each below 4 GiB: single-launch path); in train mode the first BatchNorm's batch mean
    must equal mean(a) W^T + b computed directly.
The numpy oracle cannot restate this size in seconds (1.8 TFLOP per big product); "parity at 4 GiB+" therefore rests on the block
invariance plus these properties, and is reported as such.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_model_gpu import report  # noqa: E402
from mmvae import engine, _lib  # noqa: E402
from src.models import MultiModalVAE  # noqa: E402
from src.utils import vae_loss  # noqa: E402

DEV = "cuda"


def _batch(B, A, D, S, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(B, A, device=DEV, generator=g)
    b = torch.rand(B, D, device=DEV, generator=g)
    site = torch.randint(0, S, (B,), device=DEV, generator=g)
    return a, b, site


def _step(model, a, b, site):
    for p in model.parameters():
        p.grad = None
    ra, rb, rc, mu, lv = model(a=a, b=b, site=site)
    loss, rec, cls, kld = vae_loss(ra, a, rb, b, rc, site, mu, lv, beta=1e-3, gamma=1.0)
    loss.backward()
    torch.cuda.synchronize()
    return (ra, rb, rc, mu, lv), np.array([loss.item(), float(rec), float(cls), float(kld)]), {k: p.grad.clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_row_blocks_do_not_change_a_training_step(prec):
    A, D, S, L, B = 782, 572, 24, 20, 4096
    torch.manual_seed(11)
    model = MultiModalVAE(A, D, S, L).to(DEV).set_precision(prec).train()
    a, b, site = _batch(B, A, D, S, 12)
    dev = torch.device(DEV, torch.cuda.current_device())
    lib = _lib.load()
    res = []
    for log2 in (0, 21):
        assert lib.mmvae_set_tuning(3, log2) == 0
        try:
            engine.GLOBAL_NOISE.offset_tensor(dev).zero_()                 # the same Philox draws in both runs
            for m in model.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.reset_running_stats()
            res.append(_step(model, a, b, site))
        finally:
            lib.mmvae_set_tuning(3, 0)
    (o0, l0, g0), (o1, l1, g1) = res
    # rows are independent in the forward products; the BatchNorm statistics are f64 atomic sums (order-free to ~1e-16), so the
    # outputs may move by an fp32 / bf16 rounding of a statistic at most
    tol = 1e-5 if prec == "fp32" else 2e-2
    for x, y in zip(o0, o1):
        assert (x - y).abs().max().item() <= tol * max(1.0, x.abs().max().item())
    np.testing.assert_allclose(l1, l0, rtol=1e-6 if prec == "fp32" else 1e-4)
    worst = 0.0
    for k in g0:
        if g0[k].abs().max().item() < 1e-3 * max(1e-30, max(v.abs().max().item() for v in g0.values())):
            continue                                                        # zero-by-construction biases in front of BatchNorm: rounding noise
        worst = max(worst, ((g0[k] - g1[k]).norm() / g0[k].norm().clamp_min(1e-30)).item())
    report(f"row blocks (1 MiB forced) vs single launches, B=4096 prec={prec}: loss rel {np.abs(l1 / l0 - 1).max():.2e}, grad Frobenius-rel max {worst:.2e}")
    assert worst <= (1e-4 if prec == "fp32" else 5e-3)


def test_row_blocks_do_not_change_the_fused_training_step():
    """The captured training step computes the reconstruction losses inside the decoders' last GEMMs (EPI_LOSS_MSE /
    EPI_LOSS_BCE_LOGIT): their epilogue operand is the fp32 TARGET, not an activation.  With the row-block path forced (1 MiB blocks)
    every block must read its own target rows -- a block advanced by the activation size read the targets of other rows (round-2
    advisor finding): loss sums and every gradient against the single-launch step."""
    from mmvae import functional as F_
    A, D, S, L, B = 782, 572, 24, 20, 4096
    torch.manual_seed(13)
    model = MultiModalVAE(A, D, S, L).to(DEV).set_precision("bf16").train()
    a, b, site = _batch(B, A, D, S, 14)
    dev = torch.device(DEV, torch.cuda.current_device())
    lib = _lib.load()
    res = []
    for log2 in (0, 21):
        assert lib.mmvae_set_tuning(3, log2) == 0
        try:
            engine.GLOBAL_NOISE.offset_tensor(dev).zero_()
            for m in model.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.reset_running_stats()
            gr = model._graph()
            gr.fused_recon = [a, b, None]
            try:
                ra, rb, rc, mu, lv = model(a=a, b=b, site=site)
            finally:
                gr.fused_recon = None
            assert ra.stride(0) == 0 and rb.stride(0) == 0
            total, out5 = F_.fused_loss({"a": (ra, a), "b": (rb, b), "c": (rc, site), "kl": (mu, lv)}, 1e-3, 1.0)
            for p in model.parameters():
                p.grad = None
            total.backward()
            torch.cuda.synchronize()
            res.append((out5.cpu().numpy().copy(), {k: p.grad.clone() for k, p in model.named_parameters()}))
        finally:
            lib.mmvae_set_tuning(3, 0)
    (l0, g0), (l1, g1) = res
    np.testing.assert_allclose(l1[:4], l0[:4], rtol=1e-4)
    worst = 0.0
    gmax = max(v.abs().max().item() for v in g0.values())
    for k in g0:
        if g0[k].abs().max().item() < 1e-3 * max(1e-30, gmax):
            continue
        worst = max(worst, ((g0[k] - g1[k]).norm() / g0[k].norm().clamp_min(1e-30)).item())
    report(f"fused step, row blocks (1 MiB forced) vs single launches, B=4096 bf16: loss rel {np.abs(l1[:4] / l0[:4] - 1).max():.2e}, grad Frobenius-rel max {worst:.2e}")
    assert worst <= 5e-3


def test_entry_points_reject_bad_block_size():
    lib = _lib.load()
    assert lib.mmvae_set_tuning(3, 8) == -1 and lib.mmvae_set_tuning(3, 40) == -1 and lib.mmvae_set_tuning(3, 0) == 0


def test_row_blocks_refuse_pro_out_before_the_first_block():
    """pro_out is written by the wave-specialised kernel only, which refuses a block with M % 128 != 0.  The row-block path must refuse
    pro_out before it enqueues any block: a refusal after the first blocks ran would leave their BatchNorm sums in the accumulators,
    and the engine's retry without pro_out would add them a second time.  Key 3 = 25 (32 MiB) splits M = 65 600 rows of 512 bytes
    into blocks of 22 016, 22 016 and 21 568 rows: the wave-specialised kernel would take the first two and refuse the last."""
    from mmvae import ops
    M, N, K = 16384 * 4 + 64, 256, 256
    g = torch.Generator(device=DEV).manual_seed(5)
    Y = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    scale = torch.rand(K, device=DEV, generator=g) + 0.5
    shift = torch.randn(K, device=DEV, generator=g) * 0.3
    mask = (torch.rand(M, K, device=DEV, generator=g) > 0.1).to(torch.uint8)
    pl = ops.PreparedLinear([torch.randn(N, K, device=DEV, generator=g) / K ** 0.5], [torch.zeros(N, device=DEV)], ops.PREC_BF16, DEV)
    ops.WeightPrep([pl], DEV).run()
    out = torch.full((M, N), 3.0, dtype=torch.bfloat16, device=DEV)
    H = torch.full((M, K), 7.0, dtype=torch.bfloat16, device=DEV)
    stats = torch.zeros(2, N, dtype=torch.float64, device=DEV)
    lib = _lib.load()
    assert lib.mmvae_set_tuning(3, 25) == 0
    try:
        with pytest.raises(_lib.MMVAEArgError, match="invalid argument"):
            ops.gemm_nt(ops.PREC_BF16, Y, pl.w, N, K, out, bias=pl.bias, prologue=(scale, shift, mask, 1.0 / 0.9), stats=stats, pro_out=H)
        torch.cuda.synchronize()
    finally:
        lib.mmvae_set_tuning(3, 0)
    assert torch.count_nonzero(stats).item() == 0
    assert bool((out == 3.0).all()) and bool((H == 7.0).all())


@pytest.mark.parametrize("prec,L", [("bf16", 128), ("fp32", 128), ("bf16", 20)])
def test_scaled_widths_at_batch_65536(prec, L):
    """BASELINE.json configs[4] on one GPU at the bench batch -- RNA = 20 000, DNA = 27 000, latent = 128, B = 65 536 (and latent 20,
    whose heads / decoder stems take the grouped tiny-dW path instead): a = 5.2 GB, b = 7.1 GB (fp32), both above 4 GiB.  The numpy
    oracle cannot restate 13 TFLOP in seconds; checked through size-independent properties: first BatchNorm batch means == mean(x) W^T + b,
    fused step == public call sequence, eval-mode gradients of the full batch == sum over its four quarters, outputs bit-identical per row."""
    A, D, S, B = 20000, 27000, 24, 65536
    free, _ = torch.cuda.mem_get_info()
    if free < 90 * 2 ** 30:
        pytest.skip("needs ~90 GB of free HBM")
    torch.manual_seed(21)
    model = MultiModalVAE(A, D, S, L).to(DEV).set_precision(prec)
    a, b, site = _batch(B, A, D, S, 22)
    assert a.numel() * 4 >= 2 ** 32 and b.numel() * 4 >= 2 ** 32

    # train mode: runs, finite, and the first BatchNorm batch means are what the inputs say they must be
    model.train()
    outs, losses, grads = _step(model, a, b, site)
    assert np.isfinite(losses).all() and all(torch.isfinite(g).all().item() for g in grads.values())
    for enc, x in (("encoder_a", a), ("encoder_b", b)):
        sd = dict(model.named_parameters())
        bufs = dict(model.named_buffers())
        W, bias = sd[f"{enc}.fc.0.weight"].double(), sd[f"{enc}.fc.0.bias"].double()
        want = x.double().mean(0) @ W.T + bias
        got = bufs[f"{enc}.fc.1.running_mean"].double() / 0.1                # momentum 0.1 from zero-initialised running_mean
        scale = want.abs().max().item()
        err = (got - want).abs().max().item() / scale
        report(f"scaled widths B=65536 latent={L} prec={prec}: {enc} first BatchNorm batch mean vs mean(x) W^T + b: {err:.2e} of scale")
        assert err <= (1e-4 if prec == "fp32" else 2e-3)
    del outs

    # the fused training step (reconstruction losses inside the decoders' last GEMMs: 5.2 / 7.1 GB fp32 targets behind 64-bit row offsets)
    # against the public call sequence above: same Philox draws, same running statistics
    from mmvae import functional as F_
    dev = torch.device(DEV, torch.cuda.current_device())
    def fused_or_not(fuse):
        engine.GLOBAL_NOISE.offset_tensor(dev).zero_()
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.reset_running_stats()
        g = model._graph()
        g.fused_recon = [a, b, None] if fuse else None
        try:
            ra, rb, rc, mu, lv = model(a=a, b=b, site=site)
        finally:
            g.fused_recon = None
        total, out5 = F_.fused_loss({"a": (ra, a), "b": (rb, b), "c": (rc, site), "kl": (mu, lv)}, 1e-3, 1.0)
        for p in model.parameters():
            p.grad = None
        total.backward()
        torch.cuda.synchronize()
        return np.array(F_.read_losses(out5)), {k: model.get_parameter(k).grad.clone() for k in ("decoder_a.fc.2.weight", "decoder_b.fc.4.weight", "encoder_b.fc.0.weight")}
    l0, g0 = fused_or_not(False)
    l1, g1 = fused_or_not(True)
    np.testing.assert_allclose(l1, l0, rtol=1e-6)
    for k in g0:
        e = float((g0[k] - g1[k]).norm() / g0[k].norm())
        assert e <= 1e-4, (k, e)
    report(f"scaled widths B=65536 latent={L} prec={prec}: fused step vs public call sequence: loss rel {np.abs(l1 / l0 - 1).max():.1e}")
    del grads, g0, g1

    # eval mode: full batch (row blocks) == sum over quarters (single launches)
    model.eval()
    eps = torch.randn(B, L, device=DEV)                    # reparameterize draws eps in eval mode too (src/models/vae.py:11-15): fix it
    engine.GLOBAL_NOISE.inject([], eps)
    outs, losses, grads = _step(model, a, b, site)
    rb_full = outs[1]
    Q = B // 4
    acc, lsum = None, 0.0
    for i in range(4):
        sl = slice(i * Q, (i + 1) * Q)
        engine.GLOBAL_NOISE.inject([], eps[sl])
        o, l, g = _step(model, a[sl], b[sl], site[sl])
        assert torch.equal(o[1], rb_full[sl]) and torch.equal(o[3], outs[3][sl])       # rows are independent: bit-identical outputs
        lsum = lsum + l
        acc = g if acc is None else {k: acc[k] + g[k] for k in g}
        del o
    engine.GLOBAL_NOISE.clear()
    np.testing.assert_allclose(lsum, losses, rtol=1e-6)
    worst, worst_k = 0.0, ""
    for k in grads:
        e = ((grads[k] - acc[k]).norm() / grads[k].norm().clamp_min(1e-30)).item()
        if e > worst:
            worst, worst_k = e, k
    report(f"scaled widths B=65536 latent={L} prec={prec} eval: full batch in row blocks vs sum of 4 quarters: loss rel {np.abs(lsum / losses - 1).max():.2e}, "
           f"grad Frobenius-rel max {worst:.2e} ({worst_k})")
    assert worst <= 1e-4
