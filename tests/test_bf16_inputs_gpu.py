"""Inputs in bf16 storage ("padded bf16 rows", mmvae.to_bf16_rows / mmvae_rows_to_bf16), end to end on the MI355X.

Kernel level: the conversion is bit-identical to torch's .to(torch.bfloat16) with zeroed pads; the loss epilogue of mmvae_gemm_nt and
mmvae_vae_loss with bf16 targets give the same gradient bits as with the fp32 copy of the same values, and loss sums equal to the f64
atomics' order.  Model level: bf16 storage against fp32 storage of the SAME bf16-rounded values (bf16 mode already rounds the inputs
inside the GEMM producers, so the two must agree to the run-to-run noise of the atomics), eager and captured, all three models.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvae import engine, ops, to_bf16_rows, is_bf16_rows  # noqa: E402
from mmvae import functional as F_  # noqa: E402
from mmvae.ops import PREC_BF16  # noqa: E402
from mmvae.optim import FusedAdamW  # noqa: E402
from src.models import MultiModalVAE, DNA2RNAVAE, RNA2DNAVAE  # noqa: E402
from src.utils import vae_loss  # noqa: E402
from src.utils.directional_losses import dna2rna_loss, rna2dna_loss  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, D, S, L = 782, 572, 24, 20
# biases of the Linear layers in front of a BatchNorm: their exact gradient is 0, what is computed is atomics-order noise
CHAOTIC = re.compile(r"encoder_\w+\.fc\.[04]\.bias$")


def bits(x):
    return x.contiguous().view(torch.int16)


def pads_of(x):
    """The pad columns F .. ld-1 of a padded-bf16-rows view."""
    ld = x.stride(0)
    return torch.as_strided(x, (x.shape[0], ld - x.shape[1]), (ld, 1), x.storage_offset() + x.shape[1])


def specials(n, g):
    """fp32 values that test the rounding: NaN (both signs, payloads), +-Inf, denormals, exact ties (even / odd), halfway+1, max."""
    u = torch.tensor([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF,
                      0x00008000, 0x00018000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,
                      0x00000000, 0x80000000, 0x3F800000], dtype=torch.int64)
    u = ((u + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)           # the same bits as int32
    base = torch.randn(n, generator=g) * 10.0 ** torch.randint(-40, 38, (n,), generator=g).float()
    base[: u.numel()] = u.view(torch.float32)
    return base


# ---------------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 7, 8, 572, 782])
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("strided", [False, True])
def test_to_bf16_rows_is_torch_rounding_with_zero_pads(F, src_dtype, strided):
    g = torch.Generator().manual_seed(F)
    N = 333
    x = specials(N * (F + 5), g).view(N, F + 5)
    x = x[:, 3:3 + F] if strided else x[:, :F].contiguous()
    x = x.to(DEV)
    if src_dtype == torch.bfloat16:
        x = x.to(torch.bfloat16) if not strided else torch.empty(N, F + 5, dtype=torch.bfloat16, device=DEV)[:, 2:2 + F].copy_(x)
    ref = x.to(torch.bfloat16)
    out = to_bf16_rows(x)
    assert is_bf16_rows(out) and tuple(out.shape) == (N, F) and out.stride(0) == ops.ceil_to(F, 8)
    assert torch.equal(bits(out), bits(ref))
    if out.stride(0) > F:
        assert int(bits(pads_of(out)).abs().max()) == 0
    # into a buffer that holds garbage (NaN bits): every pad is written
    buf = torch.full((N, ops.ceil_to(F, 8) + 8), -1, dtype=torch.int16, device=DEV).view(torch.bfloat16)[:, :F]
    ops.rows_to_bf16(x, buf)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(ref)) and int(bits(pads_of(buf)).abs().max()) == 0


@pytest.mark.parametrize("M", [65536, 1000])
@pytest.mark.parametrize("N,K,bce", [(782, 128, False), (572, 512, True), (300, 200, False), (131, 96, True)])
@pytest.mark.parametrize("padded", [True, False])
def test_loss_epilogue_bf16_target_equals_fp32_target(M, N, K, bce, padded):
    """gemm_nt EPI_LOSS_*: bf16 target (padded rows, or plain rows: narrower loads) == fp32 target h16.float(): gradient bits
    equal, loss sum to 1e-9 (f64 atomics)."""
    g = torch.Generator(device=DEV).manual_seed(M + N)
    Aop = to_bf16_rows(torch.randn(M, K, device=DEV, generator=g))
    W = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    bias = torch.randn(N, device=DEV, generator=g) * 0.1
    pl = ops.PreparedLinear([W], [bias], PREC_BF16, DEV)
    ops.WeightPrep([pl], DEV).run()
    T = torch.rand(M, N, device=DEV, generator=g) if bce else torch.randn(M, N, device=DEV, generator=g)
    T16 = to_bf16_rows(T) if padded else T.to(torch.bfloat16)
    T32 = T16.float()
    epi = ops.EPI_LOSS_BCE_LOGIT if bce else ops.EPI_LOSS_MSE
    res = []
    for tgt in (T32, T16):
        out = torch.full((M, ops.ceil_to(N, 8)), 3.0, dtype=torch.bfloat16, device=DEV)
        s = torch.zeros(1, dtype=torch.float64, device=DEV)
        ops.gemm_nt(PREC_BF16, Aop, pl.w, N, K, out, bias=pl.bias, epilogue=epi, h=tgt, loss_sum=s)
        res.append((out, s))
    torch.cuda.synchronize()
    assert torch.equal(bits(res[0][0]), bits(res[1][0]))
    l0, l1 = float(res[0][1]), float(res[1][1])
    assert abs(l1 - l0) <= 1e-9 * abs(l0), (l0, l1)


def _vae_loss_call(B, ra, a, rb, b, lg, site, mu, lv, gdt):
    sums = torch.zeros(5, dtype=torch.float64, device=DEV)
    ga = torch.empty(B, ops.ceil_to(ra.shape[1], 8), dtype=gdt, device=DEV)[:, :ra.shape[1]]
    gb = torch.empty(B, ops.ceil_to(rb.shape[1], 8), dtype=gdt, device=DEV)[:, :rb.shape[1]]
    gc, gm, gl = torch.empty_like(lg), torch.empty_like(mu), torch.empty_like(lv)
    ops.vae_loss(B, recon_a=ra, a=a, recon_b=rb, b=b, logits=lg, site=site, mu=mu, logvar=lv, beta=1e-3, gamma=1.0, sums=sums,
                 g_a=ga, g_b=gb, grad_b_wrt_logit=gdt == torch.bfloat16, g_c=gc, g_mu=gm, g_lv=gl)
    torch.cuda.synchronize()
    return sums[:4].cpu().numpy(), [ga, gb, gc, gm, gl]


def _check_vae_loss(B, ra, a32, rb, b32, lg, site, mu, lv):
    for gdt in (torch.float32, torch.bfloat16):
        ref_s, ref_g = _vae_loss_call(B, ra, a32.float(), rb, b32.float(), lg, site, mu, lv, gdt)
        for conv in (to_bf16_rows, lambda x: x.to(torch.bfloat16)):        # padded rows, plain rows
            s, gs = _vae_loss_call(B, ra, conv(a32), rb, conv(b32), lg, site, mu, lv, gdt)
            for x, y in zip(ref_g, gs):
                assert torch.equal(x.contiguous().view(torch.int8), y.contiguous().view(torch.int8))
            np.testing.assert_allclose(s, ref_s, rtol=1e-9, atol=0)


@pytest.mark.parametrize("B", [65536, 1000, 3])
def test_vae_loss_bf16_targets_equal_fp32_targets(B):
    g = torch.Generator(device=DEV).manual_seed(B)
    a32 = torch.randn(B, A, device=DEV, generator=g).abs().to(torch.bfloat16).float()
    b32 = torch.rand(B, D, device=DEV, generator=g).to(torch.bfloat16).float()
    ra = torch.randn(B, A, device=DEV, generator=g)
    rb = torch.rand(B, D, device=DEV, generator=g) * 0.98 + 0.01
    lg = torch.randn(B, S, device=DEV, generator=g)
    site = torch.randint(0, S, (B,), device=DEV, generator=g)
    mu, lv = torch.randn(B, L, device=DEV, generator=g), torch.randn(B, L, device=DEV, generator=g)
    _check_vae_loss(B, ra, a32, rb, b32, lg, site, mu, lv)


def test_vae_loss_bf16_targets_on_the_saturated_edges():
    d = np.load(os.path.join(ROOT, "tests", "golden", "loss_edges.npz"))
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).to(DEV) for k in ("recon_a", "a", "recon_b", "b", "recon_c", "site", "mu", "logvar")}
    f = {k: (v.float() if v.is_floating_point() else v.long()) for k, v in t.items()}
    a32, b32 = f["a"].to(torch.bfloat16).float(), f["b"].to(torch.bfloat16).float()
    sat = (f["b"] == 0) | (f["b"] == 1)
    assert bool(sat.any()) and torch.equal(b32[sat], f["b"][sat])       # the saturated 0 / 1 targets are exact in bf16
    _check_vae_loss(a32.shape[0], f["recon_a"], a32, f["recon_b"], b32, f["recon_c"], f["site"], f["mu"], f["logvar"])


# ---------------------------------------------------------------------------------------------------------------------------
# model level: bf16 storage == fp32 storage of the same values
# ---------------------------------------------------------------------------------------------------------------------------
def _data(B, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, A, generator=g).abs().to(torch.bfloat16).float().to(DEV)
    b = torch.rand(B, D, generator=g).to(torch.bfloat16).float().to(DEV)
    site = torch.randint(0, S, (B,), generator=g).to(DEV)
    return a, b, site


def _pair(cls, args, prec):
    torch.manual_seed(31)
    m0 = cls(*args).to(DEV).set_precision(prec)
    m1 = cls(*args).to(DEV).set_precision(prec)
    m1.load_state_dict(m0.state_dict())
    return m0, m1


def _rel(x, y):
    x, y = x.detach().double(), y.detach().double()
    return float((x - y).abs().max()) / (float(x.abs().max()) + 1e-30)


def _run(model, fwd, loss, train=True, fused=None):
    """One step from Philox offset 0: (outputs, losses, gradients, BatchNorm buffers)."""
    engine.GLOBAL_NOISE.offset_tensor(torch.device(DEV, torch.cuda.current_device())).zero_()
    model.train(train)
    g = model._graph()
    g.fused_recon = fused
    try:
        with torch.set_grad_enabled(train):
            outs = fwd(model)
            res = loss(outs)
    finally:
        g.fused_recon = None
    grads = {}
    if train:
        for p in model.parameters():
            p.grad = None
        res[0].backward()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    losses = np.array([float(res[0].detach())] + [float(v) for v in res[1:]])
    bufs = {k: v.clone() for k, v in model.state_dict().items() if "running" in k}
    return [o.detach().clone() for o in outs], losses, grads, bufs


def _compare(r0, r1, outs_idx, out_tol=1e-6):
    (o0, l0, g0, b0), (o1, l1, g1, b1) = r0, r1
    for i in outs_idx:
        assert _rel(o0[i], o1[i]) <= out_tol, (i, _rel(o0[i], o1[i]))
    np.testing.assert_allclose(l1, l0, rtol=1e-6)
    for k in b0:
        assert _rel(b0[k], b1[k]) <= out_tol, (k, _rel(b0[k], b1[k]))
    assert set(g0) == set(g1)
    big = max(float(v.abs().max()) for v in g0.values()) if g0 else 0.0
    worst = max([_rel(g0[k], g1[k]) for k in g0 if float(g0[k].abs().max()) > 1e-6 * big and not CHAOTIC.search(k)] or [0.0])
    assert worst <= 1e-3, worst


def _mm_fwd(xa, xb, site):
    return lambda m: m(a=xa, b=xb, site=site)


def _mm_loss(ta, tb, site):
    return lambda o: vae_loss(o[0], ta, o[1], tb, o[2], site, o[3], o[4], beta=1e-3, gamma=1.0)


@pytest.mark.parametrize("B,layout,fuse", [(65536, "padded", False), (65536, "padded", True), (1000, "padded", False),
                                           (1000, "padded", True), (1000, "plain", False), (1000, "plain", True)])
def test_multimodal_step_bf16_storage_equals_fp32_storage(B, layout, fuse):
    """bf16 mode.  fuse: the reconstruction losses inside the decoders' last GEMMs (the captured step's form) with bf16 targets.
    plain: a contiguous (B, F) bf16 tensor -- the per-call conversion path (fails on the code before bf16 storage)."""
    a, b, site = _data(B, B + 1)
    conv = to_bf16_rows if layout == "padded" else (lambda x: x.to(torch.bfloat16))
    a16, b16 = conv(a), conv(b)
    m0, m1 = _pair(MultiModalVAE, (A, D, S, L), "bf16")
    r0 = _run(m0, _mm_fwd(a, b, site), _mm_loss(a, b, site), fused=[a, b, None] if fuse else None)
    r1 = _run(m1, _mm_fwd(a16, b16, site), _mm_loss(a16, b16, site), fused=[a16, b16, None] if fuse else None)
    _compare(r0, r1, [2, 3, 4] if fuse else [0, 1, 2, 3, 4])


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_eval_and_single_modality_bf16_storage(prec):
    B = 1000
    a, b, site = _data(B, 5)
    a16, b16 = to_bf16_rows(a), to_bf16_rows(b)
    m0, m1 = _pair(MultiModalVAE, (A, D, S, L), prec)
    # eval mode, every modality
    _compare(_run(m0, _mm_fwd(a, b, site), _mm_loss(a, b, site), train=False),
             _run(m1, _mm_fwd(a16, b16, site), _mm_loss(a16, b16, site), train=False), [0, 1, 2, 3, 4])
    # a= only, b= only (site=None): outputs and latent statistics, training mode, with gradients through mu / logvar + recon
    for fa, fb in ((True, False), (False, True)):
        def fwd(x, y):
            return lambda m: m(a=x if fa else None, b=y if fb else None, site=None)

        def loss(x, y):
            def f(o):
                total, out5 = F_.fused_loss({"a": (o[0], x), "b": (o[1], y), "kl": (o[3], o[4])}, 1e-3, 1.0)
                return [total] + F_.read_losses(out5)[1:]
            return f
        _compare(_run(m0, fwd(a, b), loss(a, b)), _run(m1, fwd(a16, b16), loss(a16, b16)), [0, 1, 3, 4])


def test_fp32_mode_with_bf16_inputs_equals_float_inputs():
    B = 2048
    a, b, site = _data(B, 9)
    m0, m1 = _pair(MultiModalVAE, (A, D, S, L), "fp32")
    for conv in (to_bf16_rows, lambda x: x.to(torch.bfloat16)):
        m0.load_state_dict(m1.state_dict())
        r0 = _run(m0, _mm_fwd(a, b, site), _mm_loss(a, b, site))
        r1 = _run(m1, _mm_fwd(conv(a), conv(b), site), _mm_loss(conv(a), conv(b), site))
        _compare(r0, r1, [0, 1, 2, 3, 4])


@pytest.mark.parametrize("kind", ["dna2rna", "rna2dna"])
@pytest.mark.parametrize("fuse", [False, True])
def test_directional_models_bf16_storage(kind, fuse):
    B = 4096
    a, b, site = _data(B, 13)
    a16, b16 = to_bf16_rows(a), to_bf16_rows(b)
    cls = DNA2RNAVAE if kind == "dna2rna" else RNA2DNAVAE
    m0, m1 = _pair(cls, (A, D, S, L), "bf16")

    def fwd(x, y):
        return (lambda m: m(dna=y, site=site)) if kind == "dna2rna" else (lambda m: m(rna=x, site=site))

    def loss(x, y):
        if kind == "dna2rna":
            return lambda o: dna2rna_loss(o[0], x, o[1], o[2])
        return lambda o: rna2dna_loss(o[0], y, o[1], o[2])
    tgt = (lambda x, y: [x]) if kind == "dna2rna" else (lambda x, y: [y])
    r0 = _run(m0, fwd(a, b), loss(a, b), fused=tgt(a, b) if fuse else None)
    r1 = _run(m1, fwd(a16, b16), loss(a16, b16), fused=tgt(a16, b16) if fuse else None)
    _compare(r0, r1, [1, 2] if fuse else [0, 1, 2])


@pytest.mark.parametrize("kind", ["multimodal", "dna2rna", "rna2dna"])
def test_graphed_step_with_bf16_dataset(kind):
    """GraphedTrainStep(dataset=(A16, B16, S)) -- padded bf16 rows, gathered into padded static buffers -- against the same step on
    the fp32 dataset of the same values: losses step by step and parameters at the end (bounds of test_graphed_train_step_matches_eager).
    Fails on the code before bf16 storage: 'fused reconstruction loss: target must be fp32'."""
    from mmvae.graphs import GraphedTrainStep
    n, B, steps = 4096, 1024, 6
    a, b, site = _data(n, 17)
    cls = {"multimodal": MultiModalVAE, "dna2rna": DNA2RNAVAE, "rna2dna": RNA2DNAVAE}[kind]
    order = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(DEV)
    runs = []
    for ds in ((a, b, site), (to_bf16_rows(a), to_bf16_rows(b), site)):
        torch.manual_seed(123)
        m = cls(A, D, S, L).to(DEV).train()
        engine.GLOBAL_NOISE.offset_tensor(torch.device(DEV, torch.cuda.current_device())).zero_()
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
        gs = GraphedTrainStep(m, opt, kind=kind, dataset=ds, batch_size=B, warmup=2)
        if ds[0].dtype == torch.bfloat16:
            assert is_bf16_rows(gs.a) and is_bf16_rows(gs.b)
        losses = []
        for i in range(steps):
            gs.set_indices(order[(i % (n // B)) * B:(i % (n // B) + 1) * B])
            gs()
            losses.append(gs.losses()[0])
        runs.append((losses, m))
    np.testing.assert_allclose(runs[1][0], runs[0][0], rtol=2e-3)
    for (k, p0), (_, p1) in zip(runs[0][1].named_parameters(), runs[1][1].named_parameters()):
        if CHAOTIC.search(k):
            continue
        d = (p0 - p1).abs()
        assert float(d.max()) <= 10 * 1e-3 and float(d.mean()) <= 2e-4, (k, float(d.max()), float(d.mean()))


def test_graphed_step_with_static_bf16_buffers():
    """The static-buffer form: a= / b= padded bf16 buffers, batches copied in with copy_ (pads stay zero)."""
    from mmvae.graphs import GraphedTrainStep
    B = 1024
    a, b, site = _data(2 * B, 19)
    torch.manual_seed(5)
    m = MultiModalVAE(A, D, S, L).to(DEV).train()
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    sa, sb, ss = to_bf16_rows(a[:B]), to_bf16_rows(b[:B]), site[:B].clone()
    gs = GraphedTrainStep(m, opt, sa, sb, ss, warmup=1)
    got = []
    for i in range(4):
        lo = (i % 2) * B
        sa.copy_(a[lo:lo + B]); sb.copy_(b[lo:lo + B]); ss.copy_(site[lo:lo + B])
        gs()
        got.append(gs.losses()[0])
    assert all(np.isfinite(got)) and got[2] < got[0] and got[3] < got[1]
    assert int(bits(pads_of(sa)).abs().max()) == 0 and int(bits(pads_of(sb)).abs().max()) == 0


def test_trainer_with_bf16_input_storage(tmp_path):
    env = dict(os.environ, PYTHONPATH="")
    cmd = [sys.executable, os.path.join(ROOT, "vae-los-angeles_amd", "train.py"), "--samples", "16384", "--batch-size", "1024",
           "--checkpoint-dir", str(tmp_path), "--epochs", "2", "--input-dtype", "bf16"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "bf16 inputs" in out.stdout and "Epoch [2/2]" in out.stdout
    tl = [float(x) for x in re.findall(r"Train Loss: ([0-9.]+)", out.stdout)]
    assert len(tl) == 2 and tl[1] < tl[0], out.stdout
