"""The MFMA GEMM kernels (through the C ABI) against float64, element by element.

Every comparison with float64 is `within(got, ref, bound)` with a bound of tests/gemm_bounds.py: derived by counting the roundings of the
kernel's expression (tests/test_gemm_bounds_cpu.py shows that each bound holds for a float32 restatement under three summation orders
and that deliberate mistakes fall outside), per element and relative to that element's own terms, with no element excluded.  The
reference is computed from the values the device stores: the prepared weights read back, the rounded activations, the fp32 tables.
`within` reports each comparison's worst err / bound (the parity report of tests/test_model_gpu.py) before it asserts; those ratios are records.

The tests of the second half of the file (test_*_per_element, test_*_row_blocks_*) build the edges into their inputs -- rows of small
magnitude, columns that consist of a K (or batch) tail only, saturated logits, exact zeros, NaN pad columns, sentinel-filled output
buffers (tests/gemm_cases.py, tests/gemm_gpu_util.py) -- and assert the dispatch conditions of the kernel form they mean to run.

The older tests keep their max-scaled tolerances (_tol: 2e-5 sqrt(K) max|ref|, plus 2^-8 max|ref| for bf16 outputs; 2e-5 sqrt(M)
max|ref| for dW) BESIDE the derived bound, each marked `retained`: the dW worst-case bound exceeds them for typical elements from
M ~ 4096 on, and nothing an existing test asserts may get weaker.  Comparisons between two kernel forms stay as they were: bit
equality where the forms share their arithmetic, order-of-summation tolerances otherwise."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import elementwise_bounds as E  # noqa: E402
import gemm_bounds as G  # noqa: E402
from mmvae import ops  # noqa: E402
from mmvae.ops import PREC_BF16, PREC_F32  # noqa: E402
import gemm_cases as GC  # noqa: E402
from gemm_gpu_util import (NAN, NtCase, Out, a_operand, check_loss_epilogue, col_slice, dev, host, loss_target, prec_name, prep, row_blocks,  # noqa: E402
                           status, tn_plan_rows, tn_wide_plan, tuning, within, within_blocks)
from test_gemm_folded_gpu import Arena  # noqa: E402

DEV = "cuda"


def _round(x, prec):
    return x.to(torch.bfloat16).to(torch.float32) if prec == PREC_BF16 else x


def _prep(W, b, prec):
    pl = ops.PreparedLinear([W], [b], prec, DEV)
    ops.WeightPrep([pl], DEV).run()
    return pl


def _stats_inside(st, stored):
    """Column (sum, sum of squares) of a tile kernel against the float64 sums of the values it stored, inside the derived statistics
    bound of tests/gemm_bounds.py (fp32 partial sums over one 128-row tile, then f64 atomics).  tests/test_gemm_bounds_cpu.py shows
    that on these inputs the bound is below the rtol = 1e-4, atol = 1e-2 it replaces, column by column."""
    c = stored.numpy()
    err, tol = np.abs(st.cpu().numpy() - G.stats_ref(c)), G.stats_tol(c, G.ROWS_TILE)
    assert (err <= tol).all(), f"column statistics outside the derived bound: worst err / bound {np.max(err / np.maximum(tol, 1e-300)):.3f}"


def _tol(K, scale, out_bf16=False):
    """RETAINED: the max-scaled tolerance this file used before the derived bounds; it stays beside them wherever no CPU test shows
    the derived bound to be at or below it for every element."""
    return 2e-5 * np.sqrt(K) * scale + (scale * 2.0 ** -8 if out_bf16 else 0.0)


def _n(x):
    return x.detach().double().cpu().numpy()


def _act_bound(x_ref, x_tol, act, out_bf16):
    """Reference and derived bound of act(x) from those of x = a w^T + bias (tests/gemm_bounds.py)."""
    if act == ops.ACT_SIGMOID:
        r, t = G.sigmoid(x_ref), G.sigmoid_tol(x_ref, x_tol)
    else:
        r, t = (np.maximum(x_ref, 0) if act == ops.ACT_RELU else x_ref), x_tol
    return r, (G.bf16_out(t, r) if out_bf16 else t)


def _mm_dev(a, b):
    """float64 product on the device (rocBLAS: independent of this library), for the products the host would take seconds over."""
    return (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) @ torch.from_numpy(np.ascontiguousarray(b)).to(DEV)).cpu().numpy()


def _dw_within(dw, db, P, Q, old, atomics, what, dp=None, dq=None):
    """dW / db against float64 inside dw_tol; P, Q: the operands as the kernel multiplies them (float64 numpy), old: scalar."""
    N, K = P.shape[1], Q.shape[1]
    old_dw, old_db = np.full((N, K), float(old)), np.full(N, float(old))
    mm = _mm_dev if P.shape[0] * N * K > 5e8 else np.matmul
    rw, rb = G.dw_ref(P, Q, old_dw, old_db, mm=mm)
    tw, tb = G.dw_tol(P, Q, old_dw, old_db, dp=dp, dq=dq, atomics=atomics, mm=mm)
    within(_n(dw), rw, tw, what + " dW")
    within(_n(db), rb, tb, what + " db")


@pytest.mark.parametrize("prec", [PREC_F32, PREC_BF16])
@pytest.mark.parametrize("M,N,K,a_bf16", [(300, 128, 782, False), (257, 512, 572, False), (128, 40, 77, False),
                                          (1000, 600, 256, True), (64, 24, 64, True), (31, 130, 20, True)])
def test_nt_store(prec, M, N, K, a_bf16):
    if prec == PREC_F32 and a_bf16:
        pytest.skip("bf16 activations only exist in bf16 mode")
    g = torch.Generator().manual_seed(M * 7 + N)
    A = _round(torch.randn(M, K, generator=g), prec)
    W = torch.randn(N, K, generator=g) / np.sqrt(K)
    b = torch.randn(N, generator=g)
    Wd, bd = W.to(DEV), b.to(DEV)
    pl = _prep(Wd, bd, prec)
    np.testing.assert_array_equal(pl.w[:N, :K].float().cpu().numpy(), _round(W, prec).numpy())
    np.testing.assert_array_equal(pl.wt[:K, :N].float().cpu().numpy(), _round(W, prec).t().numpy())
    assert float(pl.w.float().abs().sum()) == pytest.approx(float(_round(W, prec).abs().sum()), rel=1e-5)
    if a_bf16:
        Ad = torch.zeros(M, ops.ceil_to(K, 8), dtype=torch.bfloat16, device=DEV)
        Ad[:, :K] = A.to(DEV)
        Ad[:, K:] = float("nan")          # a caller's pad elements may hold anything: the kernel masks a row's last chunk when K % 8 != 0
    else:
        Ad = A.to(DEV)
    ref = A.double() @ _round(W, prec).double().t() + b.double()
    a64, w64, b64 = _n(A), _n(pl.w[:N, :K]), _n(b)                   # the stored operands
    x_ref, x_tol = G.nt_ref(a64, w64, b64), G.nt_tol(a64, w64, b64)
    for out_dt in ([torch.float32] if prec == PREC_F32 else [torch.float32, torch.bfloat16]):
        for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_SIGMOID):
            out = torch.full((M, ops.ceil_to(N, 8)), 7.0, dtype=out_dt, device=DEV)
            st = torch.zeros(2, N, dtype=torch.float64, device=DEV)
            ops.gemm_nt(prec, Ad, pl.w, N, K, out, bias=pl.bias, act=act, stats=st)
            r = ref if act == 0 else (ref.clamp_min(0) if act == 1 else torch.sigmoid(ref))
            got = out[:, :N].float().cpu().double()
            within(got.numpy(), *_act_bound(x_ref, x_tol, act, out_dt == torch.bfloat16), f"test_nt_store {prec} M{M} N{N} K{K} act{act} {out_dt}")
            tol = _tol(K, float(r.abs().max()), out_dt == torch.bfloat16)
            assert float((got - r).abs().max()) <= tol, (act, out_dt)          # retained
            assert torch.all((out[:, N:].float() == 7.0) | (out[:, N:].float() == 0.0))   # pad columns: untouched or zeroed
            _stats_inside(st, got)
    # accumulate
    out = torch.ones(M, N, device=DEV)
    ops.gemm_nt(prec, Ad, pl.w, N, K, out, bias=pl.bias, accumulate=True)
    within(_n(out), x_ref + 1.0, G.accumulate_tol(x_tol, x_ref, np.ones_like(x_ref)), f"test_nt_store {prec} M{M} N{N} K{K} C += ...")
    assert float((out.cpu().double() - (ref + 1.0)).abs().max()) <= _tol(K, float(ref.abs().max()))          # retained


@pytest.mark.parametrize("prec", [PREC_F32, PREC_BF16])
@pytest.mark.parametrize("M,N,K", [(1000, 40, 128), (4096, 512, 572), (333, 128, 782), (2048, 782, 128), (130, 24, 64)])
def test_tn(prec, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    lp = prec == PREC_BF16
    P = _round(torch.randn(M, N, generator=g), prec)
    Q = _round(torch.randn(M, K, generator=g), prec)
    ref = P.double().t() @ Q.double()
    refb = P.double().sum(0)
    variants = [("f32", "f32")] + ([("bf16", "f32"), ("bf16", "bf16"), ("f32", "bf16")] if lp else [])
    for pk, qk in variants:
        def mk(X, kind):
            if kind == "f32":
                return X.to(DEV)
            t = torch.full((M, ops.ceil_to(X.shape[1], 8)), 7.0, dtype=torch.bfloat16, device=DEV)
            t[:, :X.shape[1]] = X.to(DEV)
            return t
        Pd, Qd = mk(P, pk), mk(Q, qk)
        for nsplit in (0, 1, 3):
            dw = torch.zeros(N, K, device=DEV)
            db = torch.zeros(N, device=DEV)
            ops.gemm_tn(prec, Pd, Qd, dw, db, N, K, nsplit=nsplit)
            # no slab: every split adds with f32 atomics (dw_tol(atomics=True)).  The derived worst-case bound exceeds the old tolerance
            # for typical elements from M ~ 4096 on (tests/test_gemm_bounds_cpu.py): both stay
            _dw_within(dw, db, _n(P), _n(Q), 0.0, True, f"test_tn {prec} M{M} N{N} K{K} P {pk} Q {qk} nsplit {nsplit}")
            tol = 2e-5 * np.sqrt(M) * float(ref.abs().max())
            assert float((dw.cpu().double() - ref).abs().max()) <= tol, (pk, qk, nsplit)          # retained
            assert float((db.cpu().double() - refb).abs().max()) <= 2e-5 * np.sqrt(M) * float(refb.abs().max()) + 1e-4          # retained
    # accumulation into non-zero dw
    dw = torch.ones(N, K, device=DEV); db = torch.ones(N, device=DEV)
    ops.gemm_tn(prec, P.to(DEV), Q.to(DEV), dw, db, N, K)
    _dw_within(dw, db, _n(P), _n(Q), 1.0, True, f"test_tn {prec} M{M} N{N} K{K} onto ones")
    assert float((dw.cpu().double() - ref - 1).abs().max()) <= 2e-5 * np.sqrt(M) * float(ref.abs().max())          # retained


@pytest.mark.parametrize("M,N,K", [(8192, 512, 256), (16384, 500, 250), (8192, 782, 128), (12288, 256, 512)])
def test_tn_two_wave_groups(M, N, K):
    """Plain bf16 x bf16 dW problems whose automatic split fills the chip with ONE 8-wave workgroup per CU (8 or 7 output tiles,
    batch >= 8192) run gemm_tn_kernel<.., DMA, NG = 2>: two wave groups, 4-buffer DMA ring, partial tiles added through LDS.
    Against the fp64 product of the same bf16 operands, and against the 4-wave form (an explicit split count selects it)."""
    g = torch.Generator().manual_seed(M + N + K)
    P = _round(torch.randn(M, N, generator=g), PREC_BF16)
    Q = _round(torch.randn(M, K, generator=g), PREC_BF16)
    ref = P.double().t() @ Q.double()
    refb = P.double().sum(0)
    def mk(X):
        t = torch.full((M, ops.ceil_to(X.shape[1], 8)), 7.0, dtype=torch.bfloat16, device=DEV)       # pad columns must not leak in
        t[:, :X.shape[1]] = X.to(DEV)
        return t
    Pd, Qd = mk(P), mk(Q)
    slab = torch.empty(1 << 24, device=DEV)
    got = {}
    for nsplit in (0, 64):
        dw = torch.ones(N, K, device=DEV); db = torch.ones(N, device=DEV)                            # accumulates into what is there
        ops.gemm_tn(PREC_BF16, Pd, Qd, dw, db, N, K, nsplit=nsplit, slab=slab)
        assert M % 64 == 0 and 64 * N * K <= slab.numel()                 # LDS-DMA form; the slab holds every split: the slab form of the bound
        if nsplit == 0:                                                   # launch_tn: the automatic split that selects the two wave groups
            ns2 = tn_plan_rows(M, 64, -(-N // 128) * -(-K // 128), 256)[0]
            assert ns2 % 8 == 0 and ns2 * (-(-N // 128) * -(-K // 128)) >= 224
        _dw_within(dw, db, _n(P), _n(Q), 1.0, False, f"test_tn_two_wave_groups M{M} N{N} K{K} nsplit {nsplit}")
        tol = 2e-5 * np.sqrt(M) * float(ref.abs().max())
        assert float((dw.cpu().double() - 1 - ref).abs().max()) <= tol, nsplit          # retained (the derived bound is wider at M >= 4096)
        assert float((db.cpu().double() - 1 - refb).abs().max()) <= 2e-5 * np.sqrt(M) * float(refb.abs().max()) + 1e-4, nsplit          # retained
        got[nsplit] = dw.clone()
        dw2 = torch.ones(N, K, device=DEV); db2 = torch.ones(N, device=DEV)
        ops.gemm_tn(PREC_BF16, Pd, Qd, dw2, db2, N, K, nsplit=nsplit, slab=slab)
        assert torch.equal(dw, dw2), nsplit                                                            # fixed-order sums: bitwise reproducible
    assert float((got[0] - got[64]).abs().max()) <= 1e-5 * np.sqrt(M) * float(ref.abs().max())


@pytest.mark.parametrize("prec", [PREC_F32, PREC_BF16])
@pytest.mark.parametrize("with_mask", [True, False])
def test_bn_relu_drop_prologue_and_bwd_epilogues(prec, with_mask):
    M, K, N = 700, 256, 136
    g = torch.Generator().manual_seed(5)
    adt = ops.act_dtype(prec)
    y = _round(torch.randn(M, K, generator=g), prec)
    scale = torch.rand(K, generator=g) + 0.5
    shift = torch.randn(K, generator=g) * 0.3
    mask = (torch.rand(M, K, generator=g) < 0.9).to(torch.uint8) if with_mask else None
    inv_keep = 1.0 / 0.9 if with_mask else 1.0
    W = torch.randn(N, K, generator=g) / np.sqrt(K)
    b = torch.randn(N, generator=g)
    pl = _prep(W.to(DEV), b.to(DEV), prec)
    # as the operand loader computes it: inv_keep folded into fp32 scale / shift, ONE fused multiply-add (exact product + one
    # rounding, emulated in float64), ReLU, times the keep byte -- so both sides round the same values to the compute type
    ik32 = torch.tensor(inv_keep, dtype=torch.float32)
    sc32, sh32 = scale * ik32, shift * ik32
    h = torch.relu((y.double() * sc32.double() + sh32.double()).float()) * (mask.float() if with_mask else 1.0)
    hq = _round(h, prec)
    ref = hq.double() @ _round(W, prec).double().t() + b.double()
    yd = y.to(DEV).to(adt)
    md = mask.to(DEV) if with_mask else None
    pro = (scale.to(DEV), shift.to(DEV), md, inv_keep)
    out = torch.zeros(M, N, device=DEV)
    ops.gemm_nt(prec, yd, pl.w, N, K, out, bias=pl.bias, prologue=pro)
    lp = prec == PREC_BF16
    name = f"test_bn_relu_drop_prologue_and_bwd_epilogues {prec} {'mask' if with_mask else 'nomask'}"
    w64, wt64 = _n(pl.w[:N, :K]), _n(pl.wt[:K, :N])
    h64, dh = G.prologue_operand(_n(yd), scale.numpy(), shift.numpy(), inv_keep, mask.numpy() if with_mask else None, lp)
    assert not lp or (dh > 0).mean() < 0.02
    within(_n(out), G.nt_ref(h64, w64, _n(b)), G.nt_tol(h64, w64, _n(b), dh), name + " prologue")
    assert float((out.cpu().double() - ref).abs().max()) <= _tol(K, float(ref.abs().max()))          # retained
    # TN with the same prologue on Q
    P = _round(torch.randn(M, 40, generator=g), prec)
    dw = torch.zeros(40, K, device=DEV); db = torch.zeros(40, device=DEV)
    ops.gemm_tn(prec, P.to(DEV), yd, dw, db, 40, K, q_prologue=pro)
    refw = P.double().t() @ hq.double()
    _dw_within(dw, db, _n(P), h64, 0.0, True, name + " prologue on Q", dq=dh)
    assert float((dw.cpu().double() - refw).abs().max()) <= 2e-5 * np.sqrt(M) * float(refw.abs().max())          # retained

    # dX GEMM with EPI_RELU_MASK:  dH = (dY @ W) * (H > 0)
    dY = _round(torch.randn(M, N, generator=g), prec)
    H = _round(torch.relu(torch.randn(M, K, generator=g)), prec)
    refd = (dY.double() @ _round(W, prec).double()) * (H > 0)
    outd = torch.zeros(M, K, dtype=adt, device=DEV)
    ops.gemm_nt(prec, dY.to(DEV).to(adt), pl.wt, K, N, outd, epilogue=ops.EPI_RELU_MASK, h=H.to(DEV).to(adt))
    acc, acc_tol = G.nt_ref(_n(dY), wt64, None), G.nt_tol(_n(dY), wt64, None)
    r_, t_ = G.relu_mask(acc, acc_tol, _n(H))
    within(_n(outd), r_, G.bf16_out(t_, r_) if lp else t_, name + " ReLU mask")
    assert float((outd.float().cpu().double() - refd).abs().max()) <= _tol(N, float(refd.abs().max()), prec == PREC_BF16)          # retained

    # dX GEMM with EPI_BN_BWD: d = (dY @ W) * keep * (y*scale+shift > 0); partials (sum d, sum d*xhat)
    mean = torch.randn(K, generator=g) * 0.1
    rstd = torch.rand(K, generator=g) + 0.5
    st = torch.zeros(2, K, dtype=torch.float64, device=DEV)
    bnargs = (scale.to(DEV), shift.to(DEV), mean.to(DEV), rstd.to(DEV), md, inv_keep)
    ops.gemm_nt(prec, dY.to(DEV).to(adt), pl.wt, K, N, None, epilogue=ops.EPI_BN_BWD, h=yd, bn=bnargs, stats=st)
    keep = mask.double() * inv_keep if with_mask else 1.0
    refd = (dY.double() @ _round(W, prec).double()) * keep * ((y * scale + shift) > 0)
    xhat = (y.double() - mean.double()) * rstd.double()
    d_, dt_, share = G.bn_bwd_d(acc, acc_tol, _n(y), scale.numpy(), shift.numpy(), mask.numpy() if with_mask else None, inv_keep)
    assert share < 0.02
    within(_n(st), G.bn_bwd_stats(d_, _n(y), mean.numpy(), rstd.numpy()), G.bn_bwd_stats_tol(d_, dt_, _n(y), mean.numpy(), rstd.numpy()), name + " BN backward sums")
    np.testing.assert_allclose(st[0].cpu(), refd.sum(0), rtol=1e-4, atol=1e-2)          # retained
    np.testing.assert_allclose(st[1].cpu(), (refd * xhat).sum(0), rtol=1e-4, atol=2e-2)          # retained
    # phase 1: dy = c0 * (d - c1 - xhat * c2), subtraction done on the f32 accumulators
    coef = torch.rand(3, K, generator=g) + 0.25
    ops.gemm_nt(prec, dY.to(DEV).to(adt), pl.wt, K, N, outd, epilogue=ops.EPI_BN_BWD, h=yd, bn=bnargs, bn_coef=coef.to(DEV))
    refy = coef[0].double() * (refd - coef[1].double() - xhat * coef[2].double())
    got = outd.float().cpu().double()
    r_ = E.bn_bwd_apply(d_, _n(y), mean.numpy(), rstd.numpy(), coef.numpy(), np.float64)
    t_ = G.bn_bwd_phase1_tol(d_, dt_, _n(y), mean.numpy(), rstd.numpy(), coef.numpy())
    within(got.numpy(), r_, G.bf16_out(t_, r_) if lp else t_, name + " BN backward phase 1")
    assert float((got - refy).abs().max()) <= _tol(N, float(refy.abs().max()), prec == PREC_BF16)          # retained


@pytest.mark.parametrize("N,K", [(256, 512), (512, 572), (512, 256)])
def test_nt_wide_tiles(N, K):
    """The 128x256-tile / 8-wave NT kernel (normally used from 256 row tiles up) at a small ragged M, all epilogues."""
    from mmvae import _lib
    lib = _lib.load()
    lib.mmvae_set_tuning(0, 1)
    try:
        prec, M = PREC_BF16, 389
        g = torch.Generator().manual_seed(N + K)
        A = _round(torch.randn(M, K, generator=g), prec)
        W = torch.randn(N, K, generator=g) / np.sqrt(K)
        b = torch.randn(N, generator=g)
        pl = _prep(W.to(DEV), b.to(DEV), prec)
        ref = A.double() @ _round(W, prec).double().t() + b.double()
        x_ref, x_tol = G.nt_ref(_n(A), _n(pl.w[:N, :K]), _n(b)), G.nt_tol(_n(A), _n(pl.w[:N, :K]), _n(b))          # the stored operands
        for Ad in (A.to(DEV), torch.nn.functional.pad(A, (0, ops.ceil_to(K, 8) - K)).to(DEV).bfloat16()):
            for out_dt in (torch.float32, torch.bfloat16):
                out = torch.full((M, N), 7.0, dtype=out_dt, device=DEV)
                st = torch.zeros(2, N, dtype=torch.float64, device=DEV)
                ops.gemm_nt(prec, Ad, pl.w, N, K, out, bias=pl.bias, act=ops.ACT_RELU, stats=st)
                r = ref.clamp_min(0)
                got = out.float().cpu().double()
                within(got.numpy(), *_act_bound(x_ref, x_tol, ops.ACT_RELU, out_dt == torch.bfloat16),
                       f"test_nt_wide_tiles N{N} K{K} A {Ad.dtype} {out_dt}")
                assert float((got - r).abs().max()) <= _tol(K, float(r.abs().max()), out_dt == torch.bfloat16)          # retained
                _stats_inside(st, got)
        # backward epilogues on the wide kernel: ReLU mask and both BatchNorm forms (output width N, reduction K)
        adt = torch.bfloat16
        dY = _round(torch.randn(M, K, generator=g), prec)
        Wt = torch.randn(N, K, generator=g) / np.sqrt(K)           # plays W^T: [N out][K red]
        plt = _prep(Wt.to(DEV), torch.zeros(N, device=DEV), prec)
        base = dY.double() @ _round(Wt, prec).double().t()
        H = _round(torch.relu(torch.randn(M, N, generator=g)), prec)
        outd = torch.zeros(M, N, dtype=adt, device=DEV)
        dYd = torch.nn.functional.pad(dY, (0, ops.ceil_to(K, 8) - K)).to(DEV).to(adt)      # activation buffers have 8-element rows
        ops.gemm_nt(prec, dYd, plt.w, N, K, outd, epilogue=ops.EPI_RELU_MASK, h=H.to(DEV).to(adt))
        refd = base * (H > 0)
        acc, acc_tol = G.nt_ref(_n(dY), _n(plt.w[:N, :K]), None), G.nt_tol(_n(dY), _n(plt.w[:N, :K]), None)
        r_, t_ = G.relu_mask(acc, acc_tol, _n(H))
        within(_n(outd), r_, G.bf16_out(t_, r_), f"test_nt_wide_tiles N{N} K{K} ReLU mask")
        assert float((outd.float().cpu().double() - refd).abs().max()) <= _tol(K, float(refd.abs().max()), True)          # retained
        y = _round(torch.randn(M, N, generator=g), prec)
        scale, shift = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.3
        mean, rstd = torch.randn(N, generator=g) * 0.1, torch.rand(N, generator=g) + 0.5
        mask = (torch.rand(M, N, generator=g) < 0.9).to(torch.uint8)
        bnargs = (scale.to(DEV), shift.to(DEV), mean.to(DEV), rstd.to(DEV), mask.to(DEV), 1.0 / 0.9)
        st = torch.zeros(2, N, dtype=torch.float64, device=DEV)
        ops.gemm_nt(prec, dYd, plt.w, N, K, outd, epilogue=ops.EPI_BN_BWD, h=y.to(DEV).to(adt), bn=bnargs, bn_phase=2, stats=st)
        d = base * (mask.double() / 0.9) * ((y * scale + shift) > 0)
        xhat = (y.double() - mean.double()) * rstd.double()
        d_, dt_, share = G.bn_bwd_d(acc, acc_tol, _n(y), scale.numpy(), shift.numpy(), mask.numpy(), 1.0 / 0.9)
        assert share < 0.02
        within(_n(outd), d_, G.bf16_out(dt_, d_), f"test_nt_wide_tiles N{N} K{K} BN backward d")
        within(_n(st), G.bn_bwd_stats(d_, _n(y), mean.numpy(), rstd.numpy()), G.bn_bwd_stats_tol(d_, dt_, _n(y), mean.numpy(), rstd.numpy()),
               f"test_nt_wide_tiles N{N} K{K} BN backward sums")
        assert float((outd.float().cpu().double() - d).abs().max()) <= _tol(K, float(d.abs().max()), True)          # retained
        np.testing.assert_allclose(st[0].cpu(), d.sum(0), rtol=1e-4, atol=2e-2)          # retained
        np.testing.assert_allclose(st[1].cpu(), (d * xhat).sum(0), rtol=1e-4, atol=4e-2)          # retained
        # BN prologue on the A operand with the wide kernel
        Kp = 256
        yp = _round(torch.randn(M, Kp, generator=g), prec)
        sc, sh = torch.rand(Kp, generator=g) + 0.5, torch.randn(Kp, generator=g) * 0.3
        mk = (torch.rand(M, Kp, generator=g) < 0.9).to(torch.uint8)
        W2 = torch.randn(N, Kp, generator=g) / 16
        pl2 = _prep(W2.to(DEV), b.to(DEV), prec)
        hq = _round(torch.relu(yp * sc + sh) * mk.float() / 0.9, prec)
        ref2 = hq.double() @ _round(W2, prec).double().t() + b.double()
        out2 = torch.zeros(M, N, device=DEV)
        ops.gemm_nt(prec, yp.to(DEV).to(adt), pl2.w, N, Kp, out2, bias=pl2.bias, prologue=(sc.to(DEV), sh.to(DEV), mk.to(DEV), 1.0 / 0.9))
        h64, dh = G.prologue_operand(_n(yp), sc.numpy(), sh.numpy(), 1.0 / 0.9, mk.numpy(), True)
        assert (dh > 0).mean() < 0.02
        w2 = _n(pl2.w[:N, :Kp])
        within(_n(out2), G.nt_ref(h64, w2, _n(b)), G.nt_tol(h64, w2, _n(b), dh), f"test_nt_wide_tiles N{N} Kp{Kp} prologue (register-staged 128 x 256)")
        assert float((out2.cpu().double() - ref2).abs().max()) <= _tol(Kp, float(ref2.abs().max()))          # retained
    finally:
        lib.mmvae_set_tuning(0, 256 * 128)


@pytest.mark.parametrize("prec", [PREC_F32, PREC_BF16])
@pytest.mark.parametrize("q_kind", ["f32", "act"])
def test_tn_bn_bwd_apply_prologue(prec, q_kind):
    """dW GEMM with the BatchNorm-backward correction on its P operand == mmvae_bn_bwd_apply followed by the plain dW GEMM
    (first layers: reference autograd native_batch_norm_backward + mm, optimize_hyperparameters.py:112)."""
    M, N, K = 1000, 256, 150
    g = torch.Generator().manual_seed(11)
    adt = ops.act_dtype(prec)
    d = _round(torch.randn(M, N, generator=g), prec)
    y = _round(torch.randn(M, N, generator=g) * 2 + 0.3, prec)
    mean, rstd = torch.randn(N, generator=g) * 0.2, torch.rand(N, generator=g) + 0.5
    coef = torch.stack([torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.1, torch.randn(N, generator=g) * 0.1])
    Q = torch.randn(M, K, generator=g)
    Qd = Q.to(DEV) if q_kind == "f32" else _round(Q, prec).to(DEV).to(adt)
    if q_kind == "act" and prec == PREC_BF16:
        t = torch.zeros(M, ops.ceil_to(K, 8), dtype=adt, device=DEV); t[:, :K] = Qd; Qd = t
    Qref = Q if q_kind == "f32" and prec == PREC_F32 else _round(Q, prec)
    xh = (y.double() - mean.double()) * rstd.double()
    dy = coef[0].double() * (d.double() - coef[1].double() - xh * coef[2].double())
    dyq = _round(dy.float(), prec).double()                       # the operand is rounded to the compute type once
    ref, refb = dyq.t() @ Qref.double(), dyq.sum(0)
    dd, yd = d.to(DEV).to(adt), y.to(DEV).to(adt)
    dw = torch.zeros(N, K, device=DEV); db = torch.zeros(N, device=DEV)
    ops.gemm_tn(prec, dd, Qd, dw, db, N, K, p_prologue=(yd, mean.to(DEV), rstd.to(DEV), coef.to(DEV).contiguous()))
    p_, dp_ = G.operand_risk(E.bn_bwd_apply(_n(d), _n(y), mean.numpy(), rstd.numpy(), coef.numpy(), np.float64),
                             E.bn_bwd_apply_tol(_n(d), _n(y), mean.numpy(), rstd.numpy(), coef.numpy()), prec == PREC_BF16)
    assert prec == PREC_F32 or (dp_ > 0).mean() < 0.02
    _dw_within(dw, db, p_, _n(Qref), 0.0, True, f"test_tn_bn_bwd_apply_prologue {prec} Q {q_kind}", dp=dp_)
    tol = (2e-5 if prec == PREC_F32 else 3e-3) * np.sqrt(M) * float(ref.abs().max())     # bf16: an operand rounding may flip
    assert float((dw.cpu().double() - ref).abs().max()) <= tol          # retained
    assert float((db.cpu().double() - refb).abs().max()) <= (2e-5 if prec == PREC_F32 else 3e-3) * np.sqrt(M) * float(refb.abs().max()) + 1e-3          # retained
    # and against the two-launch form it replaces
    d2 = dd.clone()
    ops.bn_bwd_apply(d2, yd, N, mean.to(DEV), rstd.to(DEV), coef.to(DEV).contiguous())
    dw2 = torch.zeros(N, K, device=DEV); db2 = torch.zeros(N, device=DEV)
    ops.gemm_tn(prec, d2, Qd, dw2, db2, N, K)
    assert float((dw - dw2).abs().max()) <= 1e-3 * float(dw2.abs().max())


@pytest.mark.parametrize("prec", [PREC_F32, PREC_BF16])
@pytest.mark.parametrize("M,N", [(1000, 256), (4133, 512), (77, 24), (5, 64)])
def test_bn_bwd_apply(prec, M, N):
    """mmvae_bn_bwd_apply (in place dy = c0 (d - c1 - xhat c2)) against float64, for widths that take the column-resident kernel
    (256 % (N / V) == 0) and one that takes the generic kernel (N = 24); the model test covers it inside the backward."""
    g = torch.Generator().manual_seed(M + N)
    adt = ops.act_dtype(prec)
    d = _round(torch.randn(M, N, generator=g), prec)
    y = _round(torch.randn(M, N, generator=g) * 2 + 0.3, prec)
    mean, rstd = torch.randn(N, generator=g) * 0.2, torch.rand(N, generator=g) + 0.5
    coef = torch.stack([torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.1, torch.randn(N, generator=g) * 0.1])
    xh = (y.double() - mean.double()) * rstd.double()
    ref = coef[0].double() * (d.double() - coef[1].double() - xh * coef[2].double())
    dd, yd = d.to(DEV).to(adt), y.to(DEV).to(adt)
    ops.bn_bwd_apply(dd, yd, N, mean.to(DEV), rstd.to(DEV), coef.to(DEV).contiguous())
    scale = float(ref.abs().max())
    tol = scale * (2.0 ** -8 if prec == PREC_BF16 else 1e-5)
    assert float((dd.float().cpu().double() - ref).abs().max()) <= tol


@pytest.mark.parametrize("case", ["store_f32_sigmoid", "store_bf16_stats", "relu_mask", "bn_bwd"])
def test_nt_kernel_generations_agree(case):
    """The two tile generations of the NT kernel (gemm_nt.hip register-staged; gemm_nt2.h LDS-DMA ring, persistent) on the SAME
    operands, switched inside one process with mmvae_set_tuning: identical products (the epilogue arithmetic is shared, the MFMA
    accumulation order over K is the same K-step order), at a size where both are eligible -- ragged N (572), K = 512, M not a
    multiple of the tile height."""
    from mmvae import _lib as L
    lib = L.load()
    dev = "cuda"
    M, N, K = 16384 + 300, (572 if case.startswith("store") else 512), (512 if case != "bn_bwd" else 256)
    g = torch.Generator().manual_seed(7)
    A = torch.randn(M, K, generator=g).to(dev).bfloat16()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    pl = ops.PreparedLinear([W], [bias], PREC_BF16, dev)
    ops.WeightPrep([pl], dev).run()
    H = torch.randn(M, ops.ceil_to(N, 8), generator=g).to(dev).bfloat16()
    mask = (torch.rand(M, N, generator=g) > 0.1).to(torch.uint8).to(dev)
    f = lambda: (torch.rand(N, generator=g) + 0.5).to(dev)
    bn = (f(), f() - 1.0, f() - 1.0, f(), mask, 1.0 / 0.9)

    def run():
        stats = torch.zeros(2, N, dtype=torch.float64, device=dev)
        if case == "store_f32_sigmoid":
            out = torch.empty(M, N, device=dev)
            ops.gemm_nt(PREC_BF16, A, pl.w, N, K, out, bias=pl.bias, act=ops.ACT_SIGMOID)
        elif case == "store_bf16_stats":
            out = torch.zeros(M, ops.ceil_to(N, 8), dtype=torch.bfloat16, device=dev)
            ops.gemm_nt(PREC_BF16, A, pl.w, N, K, out, bias=pl.bias, stats=stats)
        elif case == "relu_mask":
            out = torch.zeros(M, ops.ceil_to(N, 8), dtype=torch.bfloat16, device=dev)
            ops.gemm_nt(PREC_BF16, A, pl.w, N, K, out, epilogue=ops.EPI_RELU_MASK, h=H)
        else:
            out = torch.zeros(M, ops.ceil_to(N, 8), dtype=torch.bfloat16, device=dev)
            ops.gemm_nt(PREC_BF16, A, pl.w, N, K, out, epilogue=ops.EPI_BN_BWD, h=H, bn=bn, bn_phase=2, stats=stats)
        torch.cuda.synchronize()
        return out.float(), stats

    res = {}
    try:
        for name, nt2 in (("gen1", 0), ("gen2", 1)):
            lib.mmvae_set_tuning(2, nt2)
            res[name] = run()
    finally:
        lib.mmvae_set_tuning(2, 1)
    assert lib.mmvae_set_tuning(1, 1) == -1 and lib.mmvae_set_tuning(5, 1) == -1      # retired kernel generations: keys rejected
    ref, ref_stats = res["gen1"]
    for name in ("gen2",):
        out, stats = res[name]
        assert torch.equal(out, ref), (name, float((out - ref).abs().max()))
        if case in ("store_bf16_stats", "bn_bwd"):
            assert torch.allclose(stats, ref_stats, rtol=1e-6, atol=1e-6 * float(ref_stats.abs().max())), name      # atomics order


@pytest.mark.parametrize("M,N,K", [(16384, 512, 572), (16384, 128, 782), (8192 + 96, 384, 300), (12000, 512, 572), (16384, 100 * 8, 256)])
def test_tn_wide_tiles(M, N, K):
    """The wide-tile dW kernels (gemm_tn_wide.hip: 256 x 288 LDS-DMA form, 128 x 448 register form; BatchNorm-corrected bf16 P x fp32
    Q, M >= 8192 with a slab) against float64 on the same rounded operands, against the 128 x 128 kernel (mmvae_set_tuning key 4),
    with N / K tails, a batch that is not a multiple of the 32-row step, and a row count whose last split is short."""
    prec = PREC_BF16
    g = torch.Generator().manual_seed(5)
    Np = ops.ceil_to(N, 8)
    d = torch.zeros(M, Np, dtype=torch.bfloat16); y = torch.zeros(M, Np, dtype=torch.bfloat16)
    d[:, :N] = torch.randn(M, N, generator=g).bfloat16(); y[:, :N] = (torch.randn(M, N, generator=g) * 2 + 0.3).bfloat16()
    mean, rstd = torch.randn(N, generator=g) * 0.2, torch.rand(N, generator=g) + 0.5
    coef = torch.stack([torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.1, torch.randn(N, generator=g) * 0.1]).contiguous()
    Q = torch.randn(M, K, generator=g)
    xh = (y[:, :N].double() - mean.double()) * rstd.double()
    dy = coef[0].double() * (d[:, :N].double() - coef[1].double() - xh * coef[2].double())
    dyq = _round(dy.float(), prec).double()
    ref, refb = dyq.t() @ _round(Q, prec).double(), dyq.sum(0)
    slab = torch.empty(1 << 25, device=DEV)
    from mmvae import _lib
    lib = _lib.load()
    res = []
    try:
        for on in (1, 0):
            assert lib.mmvae_set_tuning(4, on) == 0
            dw = torch.zeros(N, K, device=DEV); db = torch.zeros(N, device=DEV)
            ops.gemm_tn(prec, d.to(DEV), Q.to(DEV), dw, db, N, K, p_prologue=(y.to(DEV), mean.to(DEV), rstd.to(DEV), coef.to(DEV)), slab=slab)
            res.append((dw.cpu().double(), db.cpu().double()))
    finally:
        lib.mmvae_set_tuning(4, 1)
    p_, dp_ = G.operand_risk(E.bn_bwd_apply(_n(d[:, :N]), _n(y[:, :N]), mean.numpy(), rstd.numpy(), coef.numpy(), np.float64),
                             E.bn_bwd_apply_tol(_n(d[:, :N]), _n(y[:, :N]), mean.numpy(), rstd.numpy(), coef.numpy()), True)
    assert (dp_ > 0).mean() < 0.02
    plan = tn_wide_plan(M, N, K, True, "f32")
    assert plan and plan[3] >= 2 and plan[3] * N * K <= slab.numel()                  # launch_tn_wide takes it: >= 2 splits, all in the slab
    for (dw, db), form in zip(res, ("wide tiles", "128 x 128")):       # both go through the slab
        _dw_within(dw, db, p_, _n(_round(Q, prec)), 0.0, False, f"test_tn_wide_tiles M{M} N{N} K{K} {form}", dp=dp_)
    tol = 3e-3 * np.sqrt(M) * float(ref.abs().max())                 # a bf16 rounding of a corrected P element may flip (see above)
    for dw, db in res:
        assert float((dw - ref).abs().max()) <= tol          # retained
        assert float((db - refb).abs().max()) <= 3e-3 * np.sqrt(M) * float(refb.abs().max()) + 1e-3          # retained
    # wide vs 128 x 128: the same bf16 operands (same correction formula), only the fp32 summation order differs
    assert float((res[0][0] - res[1][0]).abs().max()) <= 2e-5 * np.sqrt(M) * float(ref.abs().max())
    assert float((res[0][1] - res[1][1]).abs().max()) <= 2e-5 * np.sqrt(M) * float(refb.abs().max()) + 1e-4


@pytest.mark.parametrize("M,N,K,with_mask", [(1000, 512, 256, True), (777, 208, 128, True), (4096, 256, 192, False)])
def test_bn_bwd_epilogue_row_coalesced_form(M, N, K, with_mask):
    """BatchNorm+ReLU+Dropout backward epilogue of the dX GEMM (phase 2: store d, sums of d and d*xhat) in the row-coalesced LDS
    form of the second-generation kernel (mmvae_set_tuning key 6) against the accumulator-layout form and against float64:
    same d bits (same arithmetic on the same accumulators), statistics equal to summation order."""
    from mmvae import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(M + N)
    A = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    pl = _prep(W.to(DEV), torch.zeros(N, device=DEV), PREC_BF16)
    Np = ops.ceil_to(N, 8)
    Y = torch.zeros(M, Np, dtype=torch.bfloat16); Y[:, :N] = torch.randn(M, N, generator=g).bfloat16(); Y = Y.to(DEV)
    mask = (torch.rand(M, ops.ceil_to(N, 16), generator=g) > 0.1).to(torch.uint8).to(DEV) if with_mask else None
    f = lambda: (torch.rand(N, generator=g) + 0.5).to(DEV)
    sc, sh, mu, rs = f(), f() - 1.0, f() - 1.0, f()
    res = []
    try:
        for on in (0, 1):
            lib.mmvae_set_tuning(6, on)
            d = torch.full((M, Np), 5.0, dtype=torch.bfloat16, device=DEV)
            st = torch.zeros(2, N, dtype=torch.float64, device=DEV)
            ops.gemm_nt(PREC_BF16, A, pl.wt if False else pl.w, N, K, d, epilogue=ops.EPI_BN_BWD, h=Y, bn=(sc, sh, mu, rs, mask, 1.0 / 0.9), bn_phase=2, stats=st)
            res.append((d, st))
    finally:
        lib.mmvae_set_tuning(6, 1)
    assert torch.equal(res[0][0][:, :N].view(torch.int16), res[1][0][:, :N].view(torch.int16))
    assert float(res[1][0][:, N:].float().abs().max() if Np > N else 0.0) == 0.0                    # pad columns zeroed
    scale = res[0][1].abs().max(dim=1, keepdim=True).values
    assert float(((res[0][1] - res[1][1]).abs() / scale).max()) <= 1e-5
    acc = A.double().cpu() @ _round(W, PREC_BF16).double().t()
    y = Y[:, :N].double().cpu()
    keep = (mask[:, :N].double().cpu() / 0.9) if with_mask else 1.0
    dref = torch.where(y * sc.double().cpu() + sh.double().cpu() > 0, acc * keep, torch.zeros_like(acc))
    xh = (y - mu.double().cpu()) * rs.double().cpu()
    a64, w64 = _n(A), _n(pl.w[:N, :K])
    d_, dt_, share = G.bn_bwd_d(G.nt_ref(a64, w64, None), G.nt_tol(a64, w64, None), _n(y), _n(sc), _n(sh), _n(mask[:, :N]) if with_mask else None, 1.0 / 0.9)
    assert share < 0.02
    for i, form in enumerate(("accumulator layout", "row-coalesced")):
        name = f"test_bn_bwd_epilogue_row_coalesced_form M{M} N{N} K{K} {form}"
        within(_n(res[i][0][:, :N]), d_, G.bf16_out(dt_, d_), name + " d")
        within(_n(res[i][1]), G.bn_bwd_stats(d_, _n(y), _n(mu), _n(rs)), G.bn_bwd_stats_tol(d_, dt_, _n(y), _n(mu), _n(rs)), name + " sums")
    assert float((res[1][0][:, :N].double().cpu() - dref).abs().max()) <= _tol(K, float(dref.abs().max()), out_bf16=True)          # retained
    ref_st = torch.stack([dref.sum(0), (dref * xh).sum(0)])
    assert float((res[1][1].cpu() - ref_st).abs().max()) <= 3e-5 * np.sqrt(M) * float(ref_st.abs().max()) + 1e-3          # retained


@pytest.mark.parametrize("M,N,K", [(1000, 512, 572), (333, 200, 128), (4100, 128, 782)])
def test_relu_mask_epilogue_row_coalesced_form(M, N, K):
    """ReLU-backward dX epilogue in the row-coalesced LDS form (mmvae_set_tuning key 7) against the accumulator-layout form: same
    bits; output and saved activation as column slices of wider buffers (the merged decoder stem hands such slices over)."""
    from mmvae import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(M + K)
    A = torch.randn(M, ops.ceil_to(K, 8), generator=g).bfloat16().to(DEV)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    pl = _prep(W.to(DEV), torch.zeros(N, device=DEV), PREC_BF16)
    Np = ops.ceil_to(N, 8)
    Hbig = torch.randn(M, Np + 64, generator=g).bfloat16().to(DEV)
    H = Hbig[:, 32:32 + Np]
    res = []
    try:
        for on in (0, 1):
            lib.mmvae_set_tuning(7, on)
            Cbig = torch.full((M, Np + 64), 5.0, dtype=torch.bfloat16, device=DEV)
            C = Cbig[:, 16:16 + Np]
            ops.gemm_nt(PREC_BF16, A, pl.w, N, K, C, epilogue=ops.EPI_RELU_MASK, h=H)
            res.append(Cbig)
    finally:
        lib.mmvae_set_tuning(7, 1)
    assert torch.equal(res[0].view(torch.int16), res[1].view(torch.int16))          # incl. the untouched neighbours of the slice
    ref = torch.where(H[:, :N].double().cpu() > 0, A[:, :K].double().cpu() @ _round(W, PREC_BF16).double().t(), torch.zeros(M, N, dtype=torch.float64))
    a64, w64 = _n(A[:, :K]), _n(pl.w[:N, :K])
    r, t = G.relu_mask(G.nt_ref(a64, w64, None), G.nt_tol(a64, w64, None), _n(H[:, :N]))
    within(_n(res[1][:, 16:16 + N]), r, G.bf16_out(t, r), f"test_relu_mask_epilogue_row_coalesced_form M{M} N{N} K{K}")
    assert float((res[1][:, 16:16 + N].double().cpu() - ref).abs().max()) <= _tol(K, float(ref.abs().max()), out_bf16=True)          # retained


@pytest.mark.parametrize("M,N,K", [(8192, 512, 2000), (8192, 256, 12000), (16384, 128, 6000)])
def test_tn_wide_tiles_plain_p_fp32_q(M, N, K):
    """Wide-tile dW kernel with a plain bf16 P and an fp32 Q (first encoder layers at very wide inputs, where the engine applies the
    BatchNorm correction in a pass of its own): LDS-DMA forms of both tile shapes, incl. the linear block map used below 8 batch
    splits (K = 12000 -> 42 tiles, 6 splits), against the 128 x 128 kernel (mmvae_set_tuning key 4) and float64."""
    from mmvae import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(N + K)
    P = torch.randn(M, N, generator=g).bfloat16()
    Q = torch.randn(M, K, generator=g)
    ref, refb = P.double().t() @ _round(Q, PREC_BF16).double(), P.double().sum(0)
    slab = torch.empty(1 << 25, device=DEV)
    Pd, Qd = P.to(DEV), Q.to(DEV)
    res = []
    try:
        for on in (1, 0):
            assert lib.mmvae_set_tuning(4, on) == 0
            dw = torch.zeros(N, K, device=DEV); db = torch.zeros(N, device=DEV)
            ops.gemm_tn(PREC_BF16, Pd, Qd, dw, db, N, K, slab=slab)
            res.append((dw.cpu().double(), db.cpu().double()))
    finally:
        lib.mmvae_set_tuning(4, 1)
    plan = tn_wide_plan(M, N, K, False, "f32")
    assert plan and plan[3] >= 2 and plan[3] * N * K <= slab.numel() and K % 4 == 0   # launch_tn_wide takes it: >= 2 splits, all in the slab
    for (dw, db), form in zip(res, ("wide tiles", "128 x 128")):
        _dw_within(dw, db, _n(P), _n(_round(Q, PREC_BF16)), 0.0, False, f"test_tn_wide_tiles_plain_p_fp32_q M{M} N{N} K{K} {form}")
    for dw, db in res:
        assert float((dw - ref).abs().max()) <= 2e-5 * np.sqrt(M) * float(ref.abs().max())          # retained
        assert float((db - refb).abs().max()) <= 2e-5 * np.sqrt(M) * float(refb.abs().max()) + 1e-4          # retained


def test_tn_wide_tiles_bf16_operands_large_output():
    """bf16 x bf16 dW with a very large output (the decoders' last layers at the scaled omics widths, N K >= 4 M elements) runs the
    wide-tile LDS-DMA kernel (3-stage ring, linear block map): against the 128 x 128 kernel (mmvae_set_tuning key 4) and float64;
    N and K tails."""
    from mmvae import _lib
    lib = _lib.load()
    M, N, K = 8192, 4100, 1100
    g = torch.Generator().manual_seed(77)
    P = torch.zeros(M, ops.ceil_to(N, 8), dtype=torch.bfloat16); P[:, :N] = torch.randn(M, N, generator=g).bfloat16()
    Q = torch.zeros(M, ops.ceil_to(K, 8), dtype=torch.bfloat16); Q[:, :K] = torch.randn(M, K, generator=g).bfloat16()
    ref, refb = P[:, :N].double().t() @ Q[:, :K].double(), P[:, :N].double().sum(0)
    slab = torch.empty(1 << 25, device=DEV)
    Pd, Qd = P.to(DEV), Q.to(DEV)
    res = []
    try:
        for on in (1, 0):
            assert lib.mmvae_set_tuning(4, on) == 0
            dw = torch.zeros(N, K, device=DEV); db = torch.zeros(N, device=DEV)
            ops.gemm_tn(PREC_BF16, Pd, Qd, dw, db, N, K, slab=slab)
            res.append((dw.cpu().double(), db.cpu().double()))
    finally:
        lib.mmvae_set_tuning(4, 1)
    plan = tn_wide_plan(M, N, K, False, "bf16")
    assert plan and plan[3] >= 2 and plan[3] * N * K <= slab.numel()                  # launch_tn_wide takes it: >= 2 splits, all in the slab
    for (dw, db), form in zip(res, ("wide tiles", "128 x 128")):
        _dw_within(dw, db, _n(P[:, :N]), _n(Q[:, :K]), 0.0, False, f"test_tn_wide_tiles_bf16_operands_large_output {form}")
    for dw, db in res:
        assert float((dw - ref).abs().max()) <= 2e-5 * np.sqrt(M) * float(ref.abs().max())          # retained
        assert float((db - refb).abs().max()) <= 2e-5 * np.sqrt(M) * float(refb.abs().max()) + 1e-4          # retained
    assert float((res[0][0] - res[1][0]).abs().max()) <= 2e-5 * np.sqrt(M) * float(ref.abs().max())


def _set_tuning(key, value):
    from mmvae import _lib
    _lib.check(_lib.load().mmvae_set_tuning(key, value), "mmvae_set_tuning")


@pytest.mark.parametrize("M,N,K,lda,stats,act", [
    (4480, 512, 572, 572, True, ops.ACT_NONE),      # EncoderB.L0 shape: 16-byte rows, 128 x 256 tiles, row tiles padded to a multiple of 8
    (2048, 128, 782, 782, True, ops.ACT_NONE),      # EncoderA.L0 shape: 8-byte rows (16-byte loads at 8-byte alignment), K % 4 == 2: rotated tail piece
    (12288, 384, 200, 201, True, ops.ACT_RELU),     # odd leading dimension (4-byte aligned rows); 3 column tiles: a workgroup changes column tile
    (1024, 256, 130, 132, False, ops.ACT_NONE),     # K % 64 != 0 and K % 4 != 0 at 16-byte rows; no statistics
    (640, 128, 97, 97, True, ops.ACT_SIGMOID),      # K % 4 == 1
    (2056, 128, 782, 782, True, ops.ACT_NONE),      # a partial row tile: not taken by the wave-specialised kernel (both runs use the tile kernels)
])
def test_ntp_matches_tile_kernels(M, N, K, lda, stats, act):
    """The wave-specialised NT kernel (gemm_ntp.h: producer / consumer waves, persistent) against the tile kernels it replaces on the
    forward first layers: the same MFMA order over K -> bit-identical bf16 outputs; column statistics to fp32 summation order."""
    g = torch.Generator().manual_seed(M + N + K)
    Af = torch.randn(M, lda, generator=g).to(DEV)
    A = Af[:, :K]
    W = (torch.randn(N, K, generator=g) / np.sqrt(K)).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    pl = _prep(W, b, PREC_BF16)
    res = {}
    try:
        _set_tuning(9, 256)
        for on in (0, 1):
            _set_tuning(8, on)
            out = torch.full((M, ops.ceil_to(N, 8)), 7.0, dtype=torch.bfloat16, device=DEV)
            st = torch.zeros(2, N, dtype=torch.float64, device=DEV) if stats else None
            ops.gemm_nt(PREC_BF16, A, pl.w, N, K, out, bias=pl.bias, act=act, stats=st)
            torch.cuda.synchronize()
            res[on] = (out.clone(), None if st is None else st.clone())
    finally:
        _set_tuning(8, 1); _set_tuning(9, 16384)
    ref = A.to(torch.bfloat16).double() @ W.to(torch.bfloat16).double().t() + b.double()
    if act == ops.ACT_RELU:
        ref = ref.clamp_min(0)
    elif act == ops.ACT_SIGMOID:
        ref = torch.sigmoid(ref)
    got = res[1][0][:, :N].double()
    a64, w64, b64 = _n(A.to(torch.bfloat16)), _n(pl.w[:N, :K]), _n(b)
    within(_n(got), *_act_bound(G.nt_ref(a64, w64, b64), G.nt_tol(a64, w64, b64), act, True), f"test_ntp_matches_tile_kernels M{M} N{N} K{K} lda{lda}")
    assert float((got - ref).abs().max()) <= _tol(K, float(ref.abs().max()), True)          # retained
    assert torch.equal(res[0][0][:, :N], res[1][0][:, :N])
    assert torch.all((res[1][0][:, N:].float() == 7.0) | (res[1][0][:, N:].float() == 0.0))
    if stats:
        np.testing.assert_allclose(res[1][1].cpu(), res[0][1].cpu(), rtol=2e-6, atol=1e-3)
        taken = M % 128 == 0                                      # a partial row tile leaves both runs to the tile kernels
        within(_n(res[1][1]), G.stats_ref(_n(got)), G.stats_tol(_n(got), G.ntp_rows(M, N) if taken else G.ROWS_TILE), f"test_ntp_matches_tile_kernels M{M} N{N} K{K} statistics")
        np.testing.assert_allclose(res[1][1][0].cpu(), got.sum(0).cpu(), rtol=1e-5, atol=1e-2)          # retained
        np.testing.assert_allclose(res[1][1][1].cpu(), (got ** 2).sum(0).cpu(), rtol=1e-5, atol=1e-2)          # retained


@pytest.mark.parametrize("M,N,K,masked,stats", [(1024, 256, 512, True, True),      # EncoderB's second Linear (encoders.py:35) behind BN + ReLU + Dropout
                                                (512, 128, 256, True, False),      # 128 x 128 tiles
                                                (768, 256, 128, False, True)])     # eval mode: no dropout mask
def test_ntp_prologue_matches_tile_kernels(M, N, K, masked, stats):
    """gemm_ntp.h with the producers' BatchNorm + ReLU + Dropout operand prologue (bf16 A) against the register-staged tile kernel with
    the same prologue (SrcBnReluDrop): same per-element arithmetic and MFMA order -> bit-identical bf16 outputs; and against fp64."""
    g = torch.Generator().manual_seed(M + N + K)
    Y = torch.randn(M, K, generator=g).to(DEV).bfloat16()
    scale = (torch.rand(K, generator=g) + 0.5).to(DEV); shift = (torch.randn(K, generator=g) * 0.3).to(DEV)
    mask = (torch.rand(M, K, generator=g) > 0.1).to(torch.uint8).to(DEV) if masked else None
    inv_keep = 1.0 / 0.9 if masked else 1.0
    W = (torch.randn(N, K, generator=g) / np.sqrt(K)).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    pl = _prep(W, b, PREC_BF16)
    res = {}
    try:
        _set_tuning(9, 256)
        for on in (0, 1):
            _set_tuning(8, on)
            out = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
            st = torch.zeros(2, N, dtype=torch.float64, device=DEV) if stats else None
            ops.gemm_nt(PREC_BF16, Y, pl.w, N, K, out, bias=pl.bias, prologue=(scale, shift, mask, inv_keep), stats=st)
            torch.cuda.synchronize()
            res[on] = (out.clone(), None if st is None else st.clone())
    finally:
        _set_tuning(8, 1); _set_tuning(9, 16384)
    h = torch.relu(Y.double() * (scale * inv_keep).double() + (shift * inv_keep).double())
    if masked:
        h = h * mask.double()
    ref = h.to(torch.float32).to(torch.bfloat16).double() @ W.to(torch.bfloat16).double().t() + b.double()
    got = res[1][0].double()
    assert float((got - ref).abs().max()) <= _tol(K, float(ref.abs().max()), True) + 2e-2 * float(ref.abs().max())      # + the prologue's bf16 rounding
    assert torch.equal(res[0][0], res[1][0])
    if stats:
        np.testing.assert_allclose(res[1][1].cpu(), res[0][1].cpu(), rtol=2e-6, atol=1e-3)


@pytest.mark.parametrize("M,N,K,lda,act", [(1024, 512, 256, 256, ops.ACT_RELU),      # DecoderB's hidden Linear + ReLU (decoders.py:29-30)
                                           (512, 128, 200, 208, ops.ACT_NONE)])      # K % 64 != 0, row pitch > K
def test_ntp_plain_bf16_matches_tile_kernels(M, N, K, lda, act):
    """gemm_ntp.h on a plain bf16 A operand (the producers copy 16-byte chunks into the ring) against the LDS-DMA tile kernel: bit-identical."""
    g = torch.Generator().manual_seed(M + N + K)
    Af = torch.zeros(M, lda, dtype=torch.bfloat16, device=DEV)
    Af[:, :K] = torch.randn(M, K, generator=g).to(DEV)
    A = Af[:, :K]
    W = (torch.randn(N, K, generator=g) / np.sqrt(K)).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    pl = _prep(W, b, PREC_BF16)
    res = {}
    try:
        _set_tuning(9, 256)
        for on in (0, 1):
            _set_tuning(8, on)
            out = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
            ops.gemm_nt(PREC_BF16, A, pl.w, N, K, out, bias=pl.bias, act=act)
            torch.cuda.synchronize()
            res[on] = out.clone()
    finally:
        _set_tuning(8, 1); _set_tuning(9, 16384)
    ref = A.double() @ W.to(torch.bfloat16).double().t() + b.double()
    if act == ops.ACT_RELU:
        ref = ref.clamp_min(0)
    a64, w64, b64 = _n(A), _n(pl.w[:N, :K]), _n(b)
    within(_n(res[1]), *_act_bound(G.nt_ref(a64, w64, b64), G.nt_tol(a64, w64, b64), act, True), f"test_ntp_plain_bf16_matches_tile_kernels M{M} N{N} K{K}")
    assert float((res[1].double() - ref).abs().max()) <= _tol(K, float(ref.abs().max()), True)          # retained
    assert torch.equal(res[0], res[1])


def test_ntp_prologue_output_is_the_post_activation():
    """pro_out of mmvae_gemm_nt (wave-specialised kernel only): the operand after BatchNorm-normalise + ReLU + Dropout, bit for bit what
    the dW GEMM's own operand prologue would form; the GEMM result is unchanged; problems the kernel does not take answer ERR_ARG."""
    M, N, K = 16384, 256, 512
    g = torch.Generator().manual_seed(3)
    Y = torch.randn(M, K, generator=g).to(DEV).bfloat16()
    scale = (torch.rand(K, generator=g) + 0.5).to(DEV); shift = (torch.randn(K, generator=g) * 0.3).to(DEV)
    mask = (torch.rand(M, K, generator=g) > 0.1).to(torch.uint8).to(DEV)
    W = (torch.randn(N, K, generator=g) / np.sqrt(K)).to(DEV)
    pl = _prep(W, torch.zeros(N, device=DEV), PREC_BF16)
    pro = (scale, shift, mask, 1.0 / 0.9)
    out0 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV); out1 = torch.empty_like(out0)
    H = torch.full((M, K), 7.0, dtype=torch.bfloat16, device=DEV)
    assert ops.can_keep_pro_out(PREC_BF16, M, N, K, Y, out1)
    ops.gemm_nt(PREC_BF16, Y, pl.w, N, K, out0, bias=pl.bias, prologue=pro)
    ops.gemm_nt(PREC_BF16, Y, pl.w, N, K, out1, bias=pl.bias, prologue=pro, pro_out=H)
    assert torch.equal(out0, out1)
    ik = torch.tensor(1.0 / 0.9, dtype=torch.float32, device=DEV)
    want = (torch.relu((Y.double() * (scale * ik).double() + (shift * ik).double()).float()) * mask.float()).bfloat16()     # one fused multiply-add, as the kernel
    assert torch.equal(H, want)
    # dW from the kept operand == dW through the operand prologue
    P = torch.randn(M, 40, generator=g).to(DEV)
    dw0 = torch.zeros(40, K, device=DEV); db0 = torch.zeros(40, device=DEV); dw1 = torch.zeros_like(dw0); db1 = torch.zeros_like(db0)
    ops.gemm_tn(PREC_BF16, P, Y, dw0, db0, 40, K, q_prologue=pro)
    ops.gemm_tn(PREC_BF16, P, H, dw1, db1, 40, K)
    assert float((dw0 - dw1).abs().max()) <= 1e-5 * float(dw0.abs().max())
    small = Y[:1024]
    with pytest.raises(RuntimeError):                         # below the kernel's minimum M: nobody would write pro_out
        ops.gemm_nt(PREC_BF16, small, pl.w, N, K, out0[:1024], bias=pl.bias, prologue=(scale, shift, mask[:1024], 1.0 / 0.9), pro_out=H[:1024])


# =============================================================================================
# Every kernel form against float64, element by element, inside the derived bounds of tests/gemm_bounds.py.  Inputs with the edges of
# tests/gemm_cases.py (small-magnitude rows, tail-only columns, saturated logits, exact zeros), operands and outputs inside NaN- /
# sentinel-filled buffers (tests/gemm_gpu_util.py), references from the values the device stores.  Every case asserts the dispatch
# conditions of the form it means to run (csrc/gemm_nt.hip launch_nt / dispatch_epi, gemm_ntp.hip ntp_dispatch, gemm_tn.hip launch_tn)
# and a zero return of the entry point.
# =============================================================================================


def _nt_form(form, prec, M, N, K, a_kind, out_bf16=True, ldc=None):
    """Tuning keys that make `form` the kernel of a plain store-epilogue call, after asserting that the problem is one of its."""
    bf = prec == PREC_BF16
    if form == "tile128":                 # register-staged 128 x 128: the LDS-DMA generation off (or an fp32 A, which it never takes)
        return tuning(k2=0, k8=0, k0=1 << 30)
    if form == "tile256":                 # register-staged 128 x 256
        assert bf and N % 256 == 0
        return tuning(k2=0, k8=0, k0=1)
    if form == "nt2":                     # LDS-DMA ring, 128 x 128
        assert bf and a_kind == "bf16" and K > 64
        return tuning(k8=0, k0=1 << 30)
    if form == "nt2wide":                 # LDS-DMA ring, 128 x 256
        assert bf and a_kind == "bf16" and K > 64 and N % 256 == 0
        return tuning(k8=0, k0=1)
    assert form == "ntp" and bf and out_bf16 and K > 64 and M >= 256 and M % 128 == 0 and N % 128 == 0 and ldc % 64 == 0
    return tuning(k8=1, k9=256)


NT_STORE_FORMS = [  # form, prec, a_kind, M, N, K, lda
    ("tile128", PREC_F32, "f32", 31, 130, 20, None), ("tile128", PREC_F32, "f32", 128, 40, 77, None),
    ("tile128", PREC_BF16, "f32", 257, 512, 572, None), ("tile128", PREC_BF16, "bf16", 389, 136, 256, None),
    ("tile128", PREC_BF16, "bf16", 31, 130, 20, 40),
    ("nt2", PREC_BF16, "bf16", 300, 333, 256, None), ("nt2", PREC_BF16, "bf16", 389, 572, 512, 520), ("nt2", PREC_BF16, "bf16", 777, 208, 128, None),
    ("nt2wide", PREC_BF16, "bf16", 389, 256, 512, None), ("nt2wide", PREC_BF16, "bf16", 389, 512, 572, None),
    ("tile256", PREC_BF16, "bf16", 389, 256, 512, None), ("tile256", PREC_BF16, "f32", 389, 512, 572, None),
    ("ntp", PREC_BF16, "f32", 640, 128, 97, None), ("ntp", PREC_BF16, "f32", 1024, 256, 130, 132), ("ntp", PREC_BF16, "f32", 768, 384, 200, 201),
    ("ntp", PREC_BF16, "bf16", 512, 128, 256, 264),
]


@pytest.mark.parametrize("form,prec,a_kind,M,N,K,lda", NT_STORE_FORMS,
                         ids=[f"{c[0]}-{'bf16' if c[1] == PREC_BF16 else 'fp32'}-A{c[2]}-M{c[3]}-N{c[4]}-K{c[5]}" for c in NT_STORE_FORMS])
def test_nt_store_forms_per_element(form, prec, a_kind, M, N, K, lda):
    """C = act(a w^T + bias) and its column statistics on every NT form: identity / ReLU (nt_tol), sigmoid (sigmoid_tol, two columns of
    saturated logits), bf16 and fp32 outputs, C += ... (accumulate_tol; always the register-staged 128 x 128 kernel)."""
    case = NtCase(prec, M, N, K, a_kind, lda)
    tag = f"NT store {form} {case.tag}"
    ntp = form == "ntp"
    rows = G.ntp_rows(M, N) if ntp else G.ROWS_TILE
    sig, sig_tol = G.sigmoid(case.ref), G.sigmoid_tol(case.ref, case.tol)
    assert (np.abs(case.ref) > 17).any()
    runs = [(ops.ACT_NONE, torch.float32), (ops.ACT_RELU, torch.bfloat16 if prec == PREC_BF16 else torch.float32), (ops.ACT_SIGMOID, torch.float32),
            (ops.ACT_SIGMOID, torch.bfloat16)]
    if ntp:
        runs = [(ops.ACT_NONE, torch.bfloat16), (ops.ACT_RELU, torch.bfloat16), (ops.ACT_SIGMOID, torch.bfloat16)]
    for act, out_dt in runs:
        bf_out = out_dt == torch.bfloat16
        if prec == PREC_F32 and bf_out:
            continue
        o = Out(M, N, out_dt, extra=64 - N % 64 if ntp else 8)
        st = torch.zeros(2, N + 3, dtype=torch.float64, device=DEV)
        with _nt_form(form, prec, M, N, K, a_kind, bf_out, o.buf.stride(0)):
            assert not ntp or o.c.data_ptr() % 128 == 0
            assert case.gemm(o.c, act=act, stats=st) == 0
            torch.cuda.synchronize()
        r, t = {ops.ACT_NONE: (case.ref, case.tol), ops.ACT_RELU: (np.maximum(case.ref, 0), case.tol), ops.ACT_SIGMOID: (sig, sig_tol)}[act]
        got = host(o.c)
        what = f"{tag} act{act} {'bf16' if bf_out else 'fp32'} out"
        within(got, r, G.bf16_out(t, r) if bf_out else t, what)
        assert o.guards(), f"{what}: written outside C"
        within(host(st[:, :N]), G.stats_ref(got), G.stats_tol(got, rows), f"{what} statistics")
        assert float(st[:, N:].abs().max()) == 0.0
    if form == "tile128":
        old = GC.rnd(case.rng, M, N)
        o = Out(M, N, torch.float32)
        o.c.copy_(dev(old))
        with _nt_form(form, prec, M, N, K, a_kind):
            assert case.gemm(o.c, accumulate=True) == 0
            torch.cuda.synchronize()
        within(host(o.c), old.astype(np.float64) + case.ref, G.accumulate_tol(case.tol, case.ref, old), f"{tag} C += ...")
        assert o.guards()


class EpiCase(NtCase):
    """A dX problem (no bias) with the operands of the backward epilogues as column slices of wider NaN-filled buffers."""

    def __init__(self, prec, M, N, K, sliced=True, seed=1):
        super().__init__(prec, M, N, K, "bf16" if prec == PREC_BF16 else "f32", bias=False, seed=seed)
        e = GC.epi_case(self.rng, M, N)
        adt = ops.act_dtype(prec)
        self.off = (32, 16) if sliced else (0, 0)
        self.extra = 24 if sliced else 0
        self.h, _ = col_slice(e["h"], adt, self.off[0], self.extra)
        self.y, _ = col_slice(e["y"], adt, self.off[0], self.extra)
        self.h_host, self.y_host = host(self.h), host(self.y)
        assert (self.h_host == 0).mean() > 0.3                                   # h == 0 exactly occurs
        self.e = e
        n16 = ops.ceil_to(N, 16)
        mbuf = torch.full((M, n16 + 16), 3, dtype=torch.uint8, device=DEV)       # pad bytes of the mask: non-zero ("keep") garbage
        mbuf[:, :N] = dev(e["mask"])
        self.mask = mbuf[:, :N]
        self.vec = {k: dev(e[k]) for k in ("scale", "shift", "mean", "rstd")}
        self.coef = dev(e["coef"])

    def out(self, dtype=None):
        return Out(self.M, self.N, dtype or ops.act_dtype(self.prec), off=self.off[1], extra=self.extra, sentinel=5.0)

    def bn(self, masked):
        v = self.vec
        return ops.BnBwdEpilogue(v["scale"], v["shift"], v["mean"], v["rstd"], self.mask if masked else None, 1.0 / 0.9 if masked else 1.0)

    def d(self, masked):
        e = self.e
        return G.bn_bwd_d(self.ref, self.tol, self.y_host, e["scale"], e["shift"], e["mask"] if masked else None, 1.0 / 0.9 if masked else 1.0)


def _stream_ok(case, o, mask=None):
    """The conditions under which dispatch_epi (csrc/gemm_nt.hip) hands a ReLU-mask or BatchNorm-backward phase-2 problem to the
    row-coalesced LDS form at the defaults of keys 2 / 6 / 7; every row block keeps them (block offsets are whole rows)."""
    return (case.prec == PREC_BF16 and case.a_kind == "bf16" and case.h.stride(0) % 4 == 0 and case.h.data_ptr() % 8 == 0
            and o.c.stride(0) % 4 == 0 and o.c.data_ptr() % 8 == 0 and (mask is None or (mask.stride(0) % 4 == 0 and mask.data_ptr() % 4 == 0)))


def _epi_form(form, case, o=None, mask=None):
    """'stream': the row-coalesced LDS forms of the backward epilogues (gemm_nt2.h; keys 6 / 7; 128 x 128 tiles only); 'acc': the
    accumulator-layout forms (gemm_nt_epi.h) on the register-staged 128 x 128 kernel; 'acc256': the same on its 128 x 256 tiles."""
    if form == "acc":
        return tuning(k6=0, k7=0, k0=1 << 30)
    if form == "acc256":
        assert case.prec == PREC_BF16 and case.N % 256 == 0                      # nt_wide_ok at key 0 = 1; launch_nt: Epi::NEED != 0 -> no nt2
        return tuning(k6=0, k7=0, k0=1)
    assert form == "stream" and (o is None or _stream_ok(case, o, mask))
    return tuning(k0=1 << 30)


# M, N, K, mask allowed in bf16 mode, sliced, precision, form: the row-coalesced (stream) forms exist in bf16 mode only, 128 x 256 tiles at N % 256 == 0
EPI_CASES = [(M, N, K, mask_ok, sliced, prec, form)
             for M, N, K, mask_ok, sliced in [(333, 200, 128, False, True), (777, 208, 128, True, True), (389, 512, 256, True, False)]
             for prec, form in [(PREC_F32, "acc"), (PREC_BF16, "acc"), (PREC_BF16, "stream")] + ([(PREC_BF16, "acc256")] if N % 256 == 0 else [])]
EPI_IDS = [f"M{c[0]}-N{c[1]}-K{c[2]}-{'bf16' if c[5] == PREC_BF16 else 'fp32'}-{c[6]}" for c in EPI_CASES]


@pytest.mark.parametrize("M,N,K,mask_ok,sliced,prec,form", EPI_CASES, ids=EPI_IDS)
def test_relu_mask_epilogue_per_element(M, N, K, mask_ok, sliced, prec, form):
    case = EpiCase(prec, M, N, K, sliced)
    bf = prec == PREC_BF16
    ref, tol = G.relu_mask(case.ref, case.tol, case.h_host)
    o = case.out()
    with _epi_form(form, case, o):
        assert case.gemm(o.c, epilogue=ops.EPI_RELU_MASK, h=case.h) == 0
        torch.cuda.synchronize()
    within(host(o.c), ref, G.bf16_out(tol, ref) if bf else tol, f"ReLU mask {form} {case.tag}")
    assert o.guards(), "written outside the C slice"


@pytest.mark.parametrize("M,N,K,mask_ok,sliced,prec,form", EPI_CASES, ids=EPI_IDS)
def test_bn_bwd_epilogue_per_element(M, N, K, mask_ok, sliced, prec, form):
    """Phases 0, 1 and 2 with and without the keep mask (bf16 mode takes a mask only at N % 16 == 0).  The stream form exists for
    phase 2; phases 0 and 1 run the accumulator-layout form either way and are checked once."""
    case = EpiCase(prec, M, N, K, sliced)
    bf = prec == PREC_BF16
    stream = form == "stream"
    e = case.e
    for masked in ((False, True) if (mask_ok or not bf) else (False,)):
        assert not (masked and bf) or (N % 16 == 0 and case.mask.stride(0) % 16 == 0)
        dref, dtol, share = case.d(masked)
        assert share < 0.02                                                   # the at-risk cap: a condition on the inputs
        sref, stol = G.bn_bwd_stats(dref, case.y_host, e["mean"], e["rstd"]), G.bn_bwd_stats_tol(dref, dtol, case.y_host, e["mean"], e["rstd"])
        tag = f"BN backward {form} {case.tag} {'mask' if masked else 'nomask'}"
        for phase in ((2,) if stream else (0, 1, 2)):
            o = case.out() if phase else None
            st = torch.zeros(2, N + 3, dtype=torch.float64, device=DEV) if phase != 1 else None
            with _epi_form(form, case, o, case.mask if masked else None):
                assert case.gemm(None if o is None else o.c, epilogue=ops.EPI_BN_BWD, h=case.y, bn=case.bn(masked), bn_phase=phase, stats=st,
                                 bn_coef=case.coef if phase == 1 else None) == 0
                torch.cuda.synchronize()
            if phase == 2:
                within(host(o.c), dref, G.bf16_out(dtol, dref) if bf else dtol, f"{tag} phase 2 d")
            if phase == 1:
                r = E.bn_bwd_apply(dref, case.y_host, e["mean"], e["rstd"], e["coef"], np.float64)
                t = G.bn_bwd_phase1_tol(dref, dtol, case.y_host, e["mean"], e["rstd"], e["coef"])
                within(host(o.c), r, G.bf16_out(t, r) if bf else t, f"{tag} phase 1")
            if o is not None:
                assert o.guards(), "written outside the C slice"
            if st is not None:
                within(host(st[:, :N]), sref, stol, f"{tag} phase {phase} sums")
                assert float(st[:, N:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------
# the row-block path of mmvae_gemm_nt (for_row_blocks, csrc/common.h): key 3 = 17 -> 128 KiB threshold, 64 KiB blocks
# ---------------------------------------------------------------------------------------------
ROW_BLOCK_KEY = 17


@pytest.mark.parametrize("M", [389, 1000])
@pytest.mark.parametrize("what", ["store_stats", "relu_mask", "bn_bwd_mask", "loss_mse_f32", "loss_mse_bf16", "loss_bce_f32", "loss_bce_bf16", "prologue"])
def test_nt_row_blocks_per_element(what, M):
    """mmvae_gemm_nt re-enters itself per row block with a, c, h, pro_mask and epi_mask advanced: every block's rows are held to the
    same per-element bounds as a single launch (an operand advanced by the wrong element size moves the rows of every block after the
    first), the statistics and the loss sum accumulate across the blocks."""
    K = 256
    prec = PREC_BF16
    blocks = row_blocks(M, K * 2, ROW_BLOCK_KEY)
    with tuning(k3=ROW_BLOCK_KEY):
        if what == "store_stats":
            case = NtCase(prec, M, 136, K, "bf16")
            o, st = Out(M, 136, torch.bfloat16), torch.zeros(2, 136, dtype=torch.float64, device=DEV)
            assert K > 64 and max(r for _, r in blocks) < 16384                  # every block: LDS-DMA 128 x 128 (launch_nt), never gemm_ntp.h
            assert case.gemm(o.c, stats=st) == 0
            torch.cuda.synchronize()
            got = host(o.c)
            within_blocks(got, case.ref, G.bf16_out(case.tol, case.ref), blocks, f"row blocks store {case.tag}")
            within(host(st), G.stats_ref(got), G.stats_tol(got, G.ROWS_TILE), f"row blocks store {case.tag} statistics")
            assert o.guards()
        elif what == "relu_mask":
            case = EpiCase(prec, M, 200, K)
            ref, tol = G.relu_mask(case.ref, case.tol, case.h_host)
            o = case.out()
            assert _stream_ok(case, o)                                           # every block: the row-coalesced form (keys 6 / 7 at their defaults)
            assert case.gemm(o.c, epilogue=ops.EPI_RELU_MASK, h=case.h) == 0
            torch.cuda.synchronize()
            within_blocks(host(o.c), ref, G.bf16_out(tol, ref), blocks, f"row blocks ReLU mask {case.tag}")
            assert o.guards()
        elif what == "bn_bwd_mask":
            case = EpiCase(prec, M, 208, K)
            e = case.e
            dref, dtol, share = case.d(True)
            assert share < 0.02
            o, st = case.out(), torch.zeros(2, 208, dtype=torch.float64, device=DEV)
            assert _stream_ok(case, o, case.mask)                                # every block: the row-coalesced form
            assert case.gemm(o.c, epilogue=ops.EPI_BN_BWD, h=case.y, bn=case.bn(True), bn_phase=2, stats=st) == 0
            torch.cuda.synchronize()
            within_blocks(host(o.c), dref, G.bf16_out(dtol, dref), blocks, f"row blocks BN backward {case.tag} d")
            within(host(st), G.bn_bwd_stats(dref, case.y_host, e["mean"], e["rstd"]), G.bn_bwd_stats_tol(dref, dtol, case.y_host, e["mean"], e["rstd"]),
                   f"row blocks BN backward {case.tag} sums")
            assert o.guards()
        elif what.startswith("loss"):
            bce, kind = "bce" in what, what[-3:] if what.endswith("f32") else "bf16"
            N = 333 if kind == "f32" else 572
            case = NtCase(prec, M, N, K, "bf16", w_scale=(4.0 if bce else 1.0) * K ** -0.5)
            T, t_host = loss_target(GC.loss_case(case.rng, M, N, bce), kind, ld=N if kind == "f32" else N + 3)
            check_loss_epilogue(case, bce, T, t_host, f"row blocks {what} {case.tag}", blocks)
        else:
            # BatchNorm + ReLU + Dropout prologue with its mask (register-staged kernel: the operand is formed on load)
            N = 136
            rng = np.random.default_rng(M)
            y, w, b = GC.nt_case(rng, M, N, K)
            yd, y_host = a_operand(y, prec, "bf16")
            scale, shift = rng.uniform(0.5, 1.5, K).astype(np.float32), GC.rnd(rng, K, scale=0.3)
            mask = (rng.random((M, K)) < 0.9).astype(np.uint8)
            mbuf = torch.full((M, K + 8), 3, dtype=torch.uint8, device=DEV)
            mbuf[:, :K] = dev(mask)
            pl = prep(w, b, prec)
            W_host = host(pl.w[:N, :K])
            h, dh = G.prologue_operand(y_host, scale, shift, 1.0 / 0.9, mask, True)
            assert (dh > 0).mean() < 0.02
            ref = G.nt_ref(h, W_host, b)
            o = Out(M, N, torch.float32)
            pro = ops.Prologue(dev(scale), dev(shift), mbuf[:, :K], 1.0 / 0.9)
            assert max(r for _, r in blocks) < 16384                             # below ntp_min_m: the register-staged kernel forms the operand on load
            assert status(ops.gemm_nt, prec, yd, pl.w, N, K, o.c, bias=pl.bias, prologue=pro) == 0
            torch.cuda.synchronize()
            within_blocks(host(o.c), ref, G.nt_tol(h, W_host, b, dh), blocks, f"row blocks prologue bf16 M{M} N{N} K{K}")
            assert o.guards()


def test_nt_row_blocks_refuse_pro_finalize_and_pro_out_before_the_first_block():
    from test_gemm_folded_gpu import ERR_ARG, ProFinCase, snapshot, unchanged
    M, N, K = 1024, 128, 256
    case = ProFinCase(PREC_BF16, M, N, K, True, True, seed=3)
    t = case.state()
    for k in ("mean", "rstd", "scale", "shift"):
        t[k].fill_(5.0)
    c, st = case.outputs()
    H = torch.full((M, K), 7.0, dtype=torch.bfloat16, device=DEV)
    watched = list(t.values()) + [c, st, H]
    before = [snapshot(x) for x in watched]
    row_blocks(M, K * 2, ROW_BLOCK_KEY)
    with tuning(k3=ROW_BLOCK_KEY, k8=1, k9=256):
        assert case.gemm(t, c, st, fin=case.fin_args(t)) == ERR_ARG
        assert case.gemm(t, c, st, pro_out=H) == ERR_ARG
        torch.cuda.synchronize()
    assert all(unchanged(x, b) for x, b in zip(watched, before)), "a refused call enqueued something"


# ---------------------------------------------------------------------------------------------
# dW / db
# ---------------------------------------------------------------------------------------------
def tn_plan(M, N, K, MT, want, wg_target=512):
    """plan_splits / tn_plan of csrc/common.h and gemm_tn.hip -> (ntiles, nsplit, rows per split)."""
    ntiles = -(-N // 128) * -(-K // 128)
    nsplit = want
    if want <= 0:
        nsplit = wg_target // ntiles
        if nsplit >= 8:
            nsplit &= ~7
        nsplit = max(1, min(nsplit, -(-M // (4 * MT))))
    rps = -(-(-(-M // nsplit)) // MT) * MT
    return ntiles, -(-M // rps), rps


class DwCase:
    def __init__(self, prec, M, N, K, p_kind, q_kind, seed=0):
        rng = np.random.default_rng(seed + M + 3 * N + 7 * K)
        self.prec, self.M, self.N, self.K = prec, M, N, K
        p, q = GC.dw_case(rng, M, N, K)
        pad = lambda n, kind: ops.ceil_to(n, 8) if kind == "bf16" else n + 1
        self.p, self.p_host = a_operand(p, prec, p_kind, pad(N, p_kind))
        self.q, self.q_host = a_operand(q, prec, q_kind, pad(K, q_kind))
        for t, n in ((self.p, N), (self.q, K)):               # the pad columns of bf16 P / Q hold 7.0: they must not leak in
            if t.dtype == torch.bfloat16 and t.stride(0) > n:
                torch.as_strided(t, (M, t.stride(0) - n), t.stride(), t.storage_offset() + n).fill_(7.0)
        self.old_dw, self.old_db = GC.rnd(rng, N, K), GC.rnd(rng, N)
        self.plain_bf16 = prec == PREC_BF16 and p_kind == "bf16" and q_kind == "bf16"
        self.ref = G.dw_ref(self.p_host, self.q_host, self.old_dw, self.old_db)

    def outputs(self):
        a = Arena([(self.N, self.K), (self.N,)])
        a.views[0].copy_(dev(self.old_dw)); a.views[1].copy_(dev(self.old_db))
        return a

    def tol(self, atomics):
        return G.dw_tol(self.p_host, self.q_host, self.old_dw, self.old_db, atomics=atomics)


@pytest.mark.parametrize("prec", [PREC_F32, PREC_BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(130, 24, 64), (333, 128, 782), (1000, 40, 128), (1024, 40, 128)])
def test_tn_per_element(prec, M, N, K):
    """dW += P^T Q, db += column sums of P on the 128 x 128 forms (register-staged; LDS-DMA for plain bf16 x bf16 at M % 64 == 0), split
    0 / 1 / 3 ways, through the slab (dw_tol) and through f32 atomics (dw_tol(atomics=True)), onto non-zero old values."""
    lp = prec == PREC_BF16
    MT = 64 if lp else 32
    for pk, qk in ([("f32", "f32")] + ([("bf16", "f32"), ("bf16", "bf16"), ("f32", "bf16")] if lp else [])):
        case = DwCase(prec, M, N, K, pk, qk)
        dma = case.plain_bf16 and M % MT == 0
        assert M < 8192                                                          # never the wide-tile or the two-wave-group form
        if (M, pk, qk) == (1024, "bf16", "bf16"):
            assert dma                                                           # the case that reaches the LDS-DMA form
        slab = torch.empty(4 * N * K, device=DEV)
        for nsplit in (0, 1, 3):
            ns = tn_plan(M, N, K, MT, nsplit)[1]
            for use_slab in (False, True):
                atomics = not (use_slab and ns > 1 and ns * N * K <= slab.numel())          # tn_use_slab
                a = case.outputs()
                assert status(ops.gemm_tn, prec, case.p, case.q, a.views[0], a.views[1], N, K, nsplit=nsplit, slab=slab if use_slab else None) == 0
                torch.cuda.synchronize()
                tw, tb = case.tol(atomics)
                tag = f"dW {'DMA' if dma else 'register'} {prec_name(prec)} M{M} N{N} K{K} P {pk} Q {qk} nsplit {nsplit} ({ns}) {'atomics' if atomics else 'slab'}"
                within(host(a.views[0]), case.ref[0], tw, tag + " dW")
                within(host(a.views[1]), case.ref[1], tb, tag + " db")
                assert a.guards_unchanged(), "the gradient arena was written outside dw / db"


def test_tn_row_blocks_per_element():
    """mmvae_gemm_tn in row blocks (key 3 = 17) with the BatchNorm-backward correction on P from explicit coefficients: p, q and p_y are
    advanced per block and every block adds onto dW / db: the atomics form of the bound with the M of the whole call."""
    prec, M, N, K = PREC_BF16, 1000, 256, 150
    rng = np.random.default_rng(17)
    d, q = GC.dw_case(rng, M, N, K)
    y = GC.rnd(rng, M, N, scale=2.0) + np.float32(0.3)
    mean, rstd = GC.rnd(rng, N, scale=0.2), rng.uniform(0.5, 1.5, N).astype(np.float32)
    coef = np.stack([rng.uniform(0.5, 1.5, N), rng.standard_normal(N) * 0.1, rng.standard_normal(N) * 0.1]).astype(np.float32)
    dd, d_host = a_operand(d, prec, "bf16")
    yd, y_host = a_operand(y, prec, "bf16")
    qd, q_host = a_operand(q, prec, "f32", K + 2)
    blocks = row_blocks(M, (K + 2) * 4, ROW_BLOCK_KEY)
    p, dp = G.operand_risk(E.bn_bwd_apply(d_host, y_host, mean, rstd, coef, np.float64), E.bn_bwd_apply_tol(d_host, y_host, mean, rstd, coef), True)
    assert (dp > 0).mean() < 0.02
    old_dw, old_db = GC.rnd(rng, N, K), GC.rnd(rng, N)
    a = Arena([(N, K), (N,)])
    a.views[0].copy_(dev(old_dw)); a.views[1].copy_(dev(old_db))
    with tuning(k3=ROW_BLOCK_KEY):
        assert status(ops.gemm_tn, prec, dd, qd, a.views[0], a.views[1], N, K,
                      p_prologue=ops.BnBwdApply(yd, dev(mean), dev(rstd), dev(coef).contiguous())) == 0
        torch.cuda.synchronize()
    rw, rb = G.dw_ref(p, q_host, old_dw, old_db)
    tw, tb = G.dw_tol(p, q_host, old_dw, old_db, dp=dp, atomics=True)
    within(host(a.views[0]), rw, tw, f"row blocks dW ({len(blocks)} blocks) bf16 M{M} N{N} K{K} BN-corrected P")
    within(host(a.views[1]), rb, tb, f"row blocks db ({len(blocks)} blocks) bf16 M{M} N{N} K{K} BN-corrected P")
    assert a.guards_unchanged()


# ---------------------------------------------------------------------------------------------
# the wave-specialised kernel behind the BatchNorm + ReLU + Dropout prologue (gemm_ntp.hip ntp_dispatch: NtpProBn)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
def test_ntp_prologue_per_element(masked):
    """The producers' prologue with an explicit scale and shift against float64 from the stored y: the operand h and its at-risk
    allowance from prologue_operand (an h within the rounding of the fused multiply-add of a bf16 rounding boundary, or of 0, may
    differ by one bf16 ulp, or by its whole value), the product inside nt_tol(..., dh), the bf16 output rounding on top."""
    prec, M, N, K = PREC_BF16, 512, 128, 256
    rng = np.random.default_rng(M + K + masked)
    y, w, b = GC.nt_case(rng, M, N, K)
    yd, y_host = a_operand(y, prec, "bf16", K + 8)
    scale, shift = rng.uniform(0.5, 1.5, K).astype(np.float32), GC.rnd(rng, K, scale=0.3)
    mask = (rng.random((M, K)) < 0.9).astype(np.uint8) if masked else None
    inv_keep = 1.0 / 0.9 if masked else 1.0
    mv = None
    if masked:
        mbuf = torch.full((M, K + 8), 3, dtype=torch.uint8, device=DEV)          # pad bytes: non-zero ("keep") garbage
        mbuf[:, :K] = dev(mask)
        mv = mbuf[:, :K]
    pl = prep(w, b, prec)
    W_host = host(pl.w[:N, :K])
    h, dh = G.prologue_operand(y_host, scale, shift, inv_keep, mask, True)
    assert (dh > 0).mean() < 0.02                                                # the at-risk cap: a condition on the inputs
    ref, tol = G.nt_ref(h, W_host, b), G.nt_tol(h, W_host, b, dh)
    o = Out(M, N, torch.bfloat16, extra=64)
    st = torch.zeros(2, N + 3, dtype=torch.float64, device=DEV)
    # ntp_dispatch / ntp_launch: store epilogue, bf16 A and C, K % 64 == 0 <= 512, M >= key 9, whole tiles, 128-byte aligned output lines
    assert K % 64 == 0 and 64 < K <= 512 and M >= 256 and M % 128 == 0 and N % 128 == 0 and o.buf.stride(0) % 64 == 0 and o.c.data_ptr() % 128 == 0
    assert yd.stride(0) % 8 == 0 and yd.data_ptr() % 16 == 0 and (mv is None or (mv.stride(0) % 8 == 0 and mv.data_ptr() % 8 == 0))
    with tuning(k8=1, k9=256):
        assert status(ops.gemm_nt, prec, yd, pl.w, N, K, o.c, bias=pl.bias, prologue=ops.Prologue(dev(scale), dev(shift), mv, inv_keep), stats=st) == 0
        torch.cuda.synchronize()
    got = host(o.c)
    tag = f"NT ntp prologue bf16 M{M} N{N} K{K} {'mask' if masked else 'nomask'}"
    within(got, ref, G.bf16_out(tol, ref), tag)
    assert o.guards(), "written outside C"
    within(host(st[:, :N]), G.stats_ref(got), G.stats_tol(got, G.ntp_rows(M, N)), tag + " statistics")
    assert float(st[:, N:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------
# the large-batch dW forms: two wave groups (gemm_tn.hip launch_tn) and wide tiles (gemm_tn_wide.hip launch_tn_wide)
# ---------------------------------------------------------------------------------------------
LARGE_DW = [("two wave groups", 8192, 512, 256), ("two wave groups", 8192, 782, 128), ("wide BN-corrected P x fp32 Q", 8192 + 96, 384, 300),
            ("wide plain P x fp32 Q", 8192, 512, 2000), ("wide bf16 x bf16", 8192, 4100, 1100)]


@pytest.mark.parametrize("form,M,N,K", LARGE_DW, ids=[f"{c[0].replace(' ', '_')}-M{c[1]}-N{c[2]}-K{c[3]}" for c in LARGE_DW])
def test_tn_large_batch_forms_per_element(form, M, N, K):
    """The dW forms of batches >= 8192 on inputs with the edges of tests/gemm_cases.py.  The tail-only P and Q columns keep only the
    rows of the last 32-row step of the LAST SPLIT of the form's own plan: the bound of their dW elements counts those rows alone, so
    a dropped last step, or a dropped last row of a short last split, falls outside it at this M too, where the worst-case bound of
    an ordinary element is far above the arithmetic error.  Every form goes through the slab: dw_tol without atomics; db: atomics."""
    prec = PREC_BF16
    rng = np.random.default_rng(M + 3 * N + 7 * K)
    slab = torch.empty(1 << 25, device=DEV)
    pmode = form.startswith("wide BN")
    if form == "two wave groups":
        # launch_tn: plain bf16 x bf16, M % 64 == 0 (LDS-DMA), automatic split planned for 256 workgroups in whole multiples of 8 on >= 224 CUs
        ntiles = -(-N // 128) * -(-K // 128)
        nsplit, rps = tn_plan_rows(M, 64, ntiles, 256)
        assert M % 64 == 0 and nsplit % 8 == 0 and nsplit * ntiles >= 224 and N * K < 4 << 20
        q_kind = "bf16"
    else:
        q_kind = "bf16" if form == "wide bf16 x bf16" else "f32"
        plan = tn_wide_plan(M, N, K, pmode, q_kind)
        assert plan and plan[3] >= 2, "launch_tn_wide does not take it"
        _, _, ntiles, nsplit, rps = plan
    assert nsplit > 1 and nsplit * N * K <= slab.numel()                         # tn_use_slab / launch_tn_wide: the partial tiles go to the slab
    tail = GC.dw_tail(M, rps)
    assert tail.start >= (nsplit - 1) * rps and 0 < M - tail.start <= 32
    p, q = GC.dw_case(rng, M, N, K, tail)
    pd, p_host = a_operand(p, prec, "bf16")
    qd, q_host = a_operand(q, prec, q_kind, ops.ceil_to(K, 8) if q_kind == "bf16" else ops.ceil_to(K, 4))
    if q_kind == "f32":
        assert qd.stride(0) % 4 == 0 and K % 4 == 0 and qd.data_ptr() % 16 == 0   # vec_width 4
    for t, n in ((pd, N), (qd, K)):                                              # the pad columns of bf16 P / Q hold 7.0: they must not leak in
        if t.dtype == torch.bfloat16 and t.stride(0) > n:
            torch.as_strided(t, (M, t.stride(0) - n), t.stride(), t.storage_offset() + n).fill_(7.0)
    dp = pro = None
    if pmode:
        y = GC.rnd(rng, M, N, scale=2.0) + np.float32(0.3)
        mean, rstd = GC.rnd(rng, N, scale=0.2), rng.uniform(0.5, 1.5, N).astype(np.float32)
        coef = np.stack([rng.uniform(0.5, 1.5, N), rng.standard_normal(N) * 0.1, rng.standard_normal(N) * 0.1]).astype(np.float32)
        yd, y_host = a_operand(y, prec, "bf16")
        assert N % 8 == 0 and yd.stride(0) == pd.stride(0)
        p_host, dp = G.operand_risk(E.bn_bwd_apply(p_host, y_host, mean, rstd, coef, np.float64), E.bn_bwd_apply_tol(p_host, y_host, mean, rstd, coef), True)
        assert (dp > 0).mean() < 0.02
        pro = ops.BnBwdApply(yd, dev(mean), dev(rstd), dev(coef).contiguous())
    old_dw, old_db = GC.rnd(rng, N, K), GC.rnd(rng, N)
    a = Arena([(N, K), (N,)])
    a.views[0].copy_(dev(old_dw)); a.views[1].copy_(dev(old_db))
    with tuning(k4=1):
        assert status(ops.gemm_tn, prec, pd, qd, a.views[0], a.views[1], N, K, slab=slab, **({"p_prologue": pro} if pro else {})) == 0
        torch.cuda.synchronize()
    mm = _mm_dev if M * N * K > 5e8 else np.matmul
    rw, rb = G.dw_ref(p_host, q_host, old_dw, old_db, mm=mm)
    tw, tb = G.dw_tol(p_host, q_host, old_dw, old_db, dp=dp, mm=mm)
    tag = f"dW {form} M{M} N{N} K{K} ({nsplit} splits of {rps} rows)"
    got = host(a.views[0])
    tail_cols = np.zeros((N, K), bool)
    if not pmode:                                                                # the correction fills the tail-only columns of P
        tail_cols[[1 % N, N - 1], :] = True
    tail_cols[:, [2 % K, K - 1]] = True
    within(got[tail_cols], rw[tail_cols], tw[tail_cols], tag + " dW, tail-only columns")
    within(got, rw, tw, tag + " dW")
    within(host(a.views[1]), rb, tb, tag + " db")
    assert a.guards_unchanged(), "the gradient arena was written outside dw / db"


SLAB_VIEWS = [("plain P x fp32 Q, slab on an odd float", 8192, 128, 256, 1, False, ("dma", (128, 448), 1, 64, 128)),
              ("BN-corrected P x fp32 Q in 8-byte rows, slab on 8 bytes", 8192 + 96, 128, 258, 2, True, ("reg", (128, 448), 1, 65, 128))]


@pytest.mark.parametrize("what,M,N,K,off,pmode,expect", SLAB_VIEWS, ids=[f"M{c[1]}-N{c[2]}-K{c[3]}-slab{c[4]}" for c in SLAB_VIEWS])
def test_tn_wide_tiles_slab_view(what, M, N, K, off, pmode, expect):
    """The wide-tile dW kernels choose the width of their slab stores from K AND the slab's alignment (tn_store_slab,
    csrc/gemm_tn_tile.h): 16 bytes for K % 4 == 0 on a 16-byte aligned slab, 8 bytes for an even K on an 8-byte aligned one, single
    floats otherwise.  The smallest problems launch_tn_wide takes, with the slab handed over as slab[1:] (4-byte aligned; K = 256) and
    as slab[2:] (8-byte aligned; K = 258, whose fp32 rows of 8 bytes only the 128 x 448 register form takes): dW has the bits of the
    same call on the 16-byte aligned slab (one fixed-order group of <= 128 splits either way), dW and db are inside dw_tol, and the
    tail-only columns keep the rows of the plan's last 32-row step."""
    prec = PREC_BF16
    rng = np.random.default_rng(M + 3 * N + 7 * K)
    ldq = K
    plan = tn_wide_plan(M, N, K, pmode, "f32", ldq)
    assert plan == expect, plan                                                  # the form taken and the split, by launch_tn_wide's own rules
    _, _, ntiles, nsplit, rps = plan
    elems = nsplit * N * K
    assert nsplit <= 128 and (off != 1 or elems == 2097152)                      # one reduce group (TN_RG): a fixed-order sum
    buf = torch.empty(elems + 4, device=DEV)
    aligned, view = buf[:elems], buf[off:]
    assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off and view.numel() >= elems
    tail = GC.dw_tail(M, rps)
    assert tail.start >= (nsplit - 1) * rps and 0 < M - tail.start <= 32
    p, q = GC.dw_case(rng, M, N, K, tail)
    pd, p_host = a_operand(p, prec, "bf16")
    qd, q_host = a_operand(q, prec, "f32", ldq)
    assert qd.stride(0) == ldq and qd.data_ptr() % 16 == 0 and (ldq * 4) % 16 == (0 if off == 1 else 8)
    dp = pro = None
    if pmode:
        y = GC.rnd(rng, M, N, scale=2.0) + np.float32(0.3)
        mean, rstd = GC.rnd(rng, N, scale=0.2), rng.uniform(0.5, 1.5, N).astype(np.float32)
        coef = np.stack([rng.uniform(0.5, 1.5, N), rng.standard_normal(N) * 0.1, rng.standard_normal(N) * 0.1]).astype(np.float32)
        yd, y_host = a_operand(y, prec, "bf16")
        assert N % 8 == 0 and yd.stride(0) == pd.stride(0)
        p_host, dp = G.operand_risk(E.bn_bwd_apply(p_host, y_host, mean, rstd, coef, np.float64), E.bn_bwd_apply_tol(p_host, y_host, mean, rstd, coef), True)
        assert (dp > 0).mean() < 0.02
        pro = ops.BnBwdApply(yd, dev(mean), dev(rstd), dev(coef).contiguous())
    old_dw, old_db = GC.rnd(rng, N, K), GC.rnd(rng, N)
    got = []
    for slab in (aligned, view):
        buf.fill_(NAN)                                                           # an element the kernel does not store reaches dW as NaN
        a = Arena([(N, K), (N,)])
        a.views[0].copy_(dev(old_dw)); a.views[1].copy_(dev(old_db))
        with tuning(k4=1):
            assert status(ops.gemm_tn, prec, pd, qd, a.views[0], a.views[1], N, K, slab=slab, **({"p_prologue": pro} if pro else {})) == 0
            torch.cuda.synchronize()
        assert a.guards_unchanged(), "the gradient arena was written outside dw / db"
        got.append((a.views[0].clone(), host(a.views[1])))
    assert torch.equal(got[0][0], got[1][0]), "dW depends on the slab's alignment"
    rw, rb = G.dw_ref(p_host, q_host, old_dw, old_db)
    tw, tb = G.dw_tol(p_host, q_host, old_dw, old_db, dp=dp)
    tag = f"dW {what} M{M} N{N} K{K} ({nsplit} splits of {rps} rows)"
    for (dw, db), name in zip(got, ("aligned slab", f"slab[{off}:]")):
        within(host(dw), rw, tw, f"{tag} dW, {name}")
        within(db, rb, tb, f"{tag} db, {name}")
