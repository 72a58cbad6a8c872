"""The stand-alone loss kernel (mmvae_vae_loss: vae_loss_kernel in csrc/elementwise.hip) and mmvae_gather_rows, one launch at a time,
every form the launcher can pick.

Nothing here is a tolerance fitted to what the kernels return.  The loss kernel is held, ELEMENT BY ELEMENT, to the bounds DERIVED in
tests/loss_bounds.py against a float64 reference of the same operation (tests/test_loss_bounds_cpu.py shows on the CPU that float32
arithmetic stays inside them and that a dozen deliberate mistakes do not); the inputs are those of tests/loss_cases.py.  Everything
else is EXACT: pad columns (+0 bit patterns), untouched memory (outputs are pre-filled with NaN and every buffer is compared as a
whole), the count of labels outside [0, S), gathered rows (bit for bit), refusals (every output bit-unchanged).  No element is
excluded anywhere.  Each case asserts, from its own pointers, leading dimensions and the launcher's grid as restated in
loss_bounds.py, which form it reaches: the vector widths, the class path, TAIL or not, how often a loop goes round.

No call hands the library a pointer or a size that could take a kernel outside its buffers: every buffer is allocated at its full
padded size, and the refusal tests use only arguments the entry points reject before they launch.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import elementwise_bounds as E  # noqa: E402
import loss_bounds as LB  # noqa: E402
import loss_cases as LC  # noqa: E402
from mmvae import _lib as L  # noqa: E402
from mmvae import ops  # noqa: E402

DEV = "cuda"
F32, F64 = np.float32, np.float64
NAN = float("nan")
ERR_ARG, ERR_DTYPE = -1, -2
LOSS_U = 4                      # csrc/elementwise.hip
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().double().cpu().numpy()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()]).cpu().numpy()


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


def view2d(x, ld, shift=0, dt="f32"):
    """Device copy of the 2-D array x as a [B][W] view, row stride ld, `shift` elements into a NaN-filled buffer of its own
    (bf16: x holds bf16 values, the copy is exact).  -> (view, whole buffer)"""
    B, W = x.shape
    assert ld >= W
    buf = torch.full((shift + B * ld,), NAN, dtype=TORCH_DT[dt], device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf.as_strided((B, W), (ld, 1), shift)
    v.copy_(dev(x))
    return v, buf


def out2d(B, W, ld, dt="f32"):
    """A NaN-filled [B][ld] output buffer and its [B][W] view.  -> (view, whole buffer as [B][ld])"""
    buf = torch.full((B, ld), NAN, dtype=TORCH_DT[dt], device=DEV)
    return buf.as_strided((B, W), (ld, 1)), buf


def new_sums():
    return torch.zeros(5, dtype=torch.float64, device=DEV)


def check_sum(sums, k, terms, tol_terms, n32, what):
    inside(sums[k].item(), float(np.sum(terms, dtype=F64)), LB.sum_tol(terms, tol_terms, n32), f"{what} sums[{k}] (fp32 chains of {n32})")


def check_grad_rows(whole, W, ref, tol, what):
    """Columns < W inside the bound; W ... min(ld, ceil8(W)) +0 bit patterns (the GEMM operand contract); beyond still NaN."""
    ld = whole.shape[1]
    pad_end = min(ld, (W + 7) // 8 * 8)
    inside(host(whole[:, :W]), ref, LB.bf16_out(tol, ref) if whole.dtype == torch.bfloat16 else tol, what)
    assert (bits(whole[:, W:pad_end]) == 0).all(), f"{what}: pad columns"
    assert torch.isnan(whole[:, pad_end:]).all(), f"{what}: columns past the pad were written"


# =============================================================================================
# streaming parts: MSE and BCE
# =============================================================================================
# one side of a launch: width, leading dimension of the prediction, target (type, element shift of its base, leading dimension),
# leading dimension of the gradient rows (None: no gradient output), the vector width the launcher must pick
Side = namedtuple("Side", "W ld_p t_dt t_shift ld_t ld_g V", defaults=(None, "f32", 0, None, None, None))

STREAM_CASES = {   # name: (B, gradient type, MSE side, BCE side).  The nine (VA, VD) pairs; V = 4, 2, 1 with each gradient type (fp32,
    # bf16, none) and each target type on each side; ld_g = W, W + 3, ceil8(W), ceil8(W) + 8 (and 574: bf16 rows with ld % 4 != 0)
    "4x4 dc=0":        (37, "f32", Side(572, ld_g=572, V=4), Side(256, t_dt="bf16", ld_g=264, V=4)),
    "4x2 bf16":        (37, "bf16", Side(572, t_dt="bf16", ld_t=576, ld_g=576, V=4), Side(782, t_dt="bf16", ld_g=784, V=2)),
    "4x1 loss only":   (37, "f32", Side(572, V=4), Side(333, t_dt="bf16", V=1)),
    "2x4 grid cap":    (4099, "f32", Side(782, t_dt="bf16", ld_g=792, V=2), Side(572, V=4)),
    "2x2 alignment":   (37, "bf16", Side(572, t_dt="bf16", t_shift=2, ld_t=572, ld_g=576, V=2), Side(572, ld_g=574, V=2)),
    "2x1 shifted":     (37, "f32", Side(782, V=2), Side(572, t_shift=1, ld_g=575, V=1)),
    "1x4 odd ld":      (37, "bf16", Side(572, ld_p=573, ld_g=572, V=1), Side(572, ld_g=584, V=4)),
    "1x2 one row":     (1, "f32", Side(333, t_dt="bf16", V=1), Side(782, t_dt="bf16", ld_g=782, V=2)),
    "1x1 dr=0":        (3, "f32", Side(2051, ld_g=2054, V=1), Side(333, ld_g=336, V=1)),
    "1x1 bf16":        (37, "bf16", Side(333, ld_g=336, V=1), Side(333, ld_g=333, V=1)),
    "4x2 loss only b": (37, "f32", Side(572, ld_g=576, V=4), Side(782, V=2)),
}


def _assert_stream_coverage():
    """The table above really is what its comment says (checked when the module is collected, GPU or not)."""
    cases = list(STREAM_CASES.values())
    widths = (4, 2, 1)
    assert {(a.V, b.V) for _, _, a, b in cases} == {(u, v) for u in widths for v in widths}
    for side in (2, 3):                                                               # MSE side, BCE side
        assert {(c[side].V, c[1] if c[side].ld_g else None) for c in cases} == {(v, g) for v in widths for g in ("f32", "bf16", None)}, side
        assert {(c[side].V, c[side].t_dt) for c in cases} == {(v, t) for v in widths for t in ("f32", "bf16")}, side
    ceil8 = lambda w: (w + 7) // 8 * 8
    kinds = {"W" if s.ld_g == s.W else "W+3" if s.ld_g == s.W + 3 else "ceil8" if s.ld_g == ceil8(s.W) else "ceil8+8" if s.ld_g == ceil8(s.W) + 8 else "other"
             for c in cases for s in c[2:] if s.ld_g}
    assert kinds >= {"W", "W+3", "ceil8", "ceil8+8"}


_assert_stream_coverage()


def _side(rng, gen, B, s, g_dt):
    x, t = gen(rng, B, s.W, s.t_dt == "bf16")
    pred, pbuf = view2d(x, s.ld_p or s.W)
    tgt, tbuf = view2d(t, s.ld_t or s.W, s.t_shift, s.t_dt)
    g, gbuf = out2d(B, s.W, s.ld_g, g_dt) if s.ld_g else (None, None)
    ld = lambda v: v.stride(0)
    operands = [(pred.data_ptr(), ld(pred), 4), (tgt.data_ptr(), ld(tgt), tgt.element_size()),
                (None, 0, 4) if g is None else (g.data_ptr(), ld(g), g.element_size())]
    V = LB.vec_width(s.W, operands)
    assert V == s.V, (s, operands)
    return dict(x=x, t=t, pred=pred, tgt=tgt, g=g, gbuf=gbuf, keep=[(b, bits(b).copy()) for b in (pbuf, tbuf)])


@pytest.mark.parametrize("wrt_logit", [False, True])
@pytest.mark.parametrize("name", list(STREAM_CASES))
def test_stream_parts(name, wrt_logit):
    B, g_dt, sa, sb = STREAM_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    a, b = _side(rng, LC.mse_case, B, sa, g_dt), _side(rng, LC.bce_case, B, sb, g_dt)
    c = LC.bce_edge_counts(b["x"], b["t"])
    assert c["zero"] == 3 and c["one"] == 3 and c["denormal"] == 9 and c["clamped"] >= 27 and c["unclamped_near"] >= 3, c
    grid, tail = LB.launch(B, A=sa.W, va=sa.V, D=sb.W, vd=sb.V)
    stride = grid * 256
    assert not tail
    # RowWalk geometry the case is there for
    if "dr=0" in name:
        assert sa.W // sa.V > stride                                                  # a pass does not reach the next row
    if "dc=0" in name:
        assert stride % (sb.W // sb.V) == 0                                           # the column never moves
    if "grid cap" in name:
        total = B * (sa.W // sa.V)
        assert grid == 1024 and total % (LOSS_U * stride) != 0
        assert total // (LOSS_U * stride) == 1 and -(-(total % (LOSS_U * stride)) // stride) == 3      # one unrolled pass, three single ones
    sums = new_sums()
    ops.vae_loss(B, recon_a=a["pred"], a=a["tgt"], recon_b=b["pred"], b=b["tgt"], sums=sums, g_a=a["g"], g_b=b["g"], grad_b_wrt_logit=wrt_logit)
    torch.cuda.synchronize()
    for k, (part, ref, tol, s) in enumerate(((a, LB.mse(a["x"], a["t"], F64), LB.mse_tol(a["x"], a["t"]), sa),
                                             (b, LB.bce(b["x"], b["t"], wrt_logit, F64), LB.bce_tol(b["x"], b["t"], wrt_logit), sb))):
        what = f"{name} {'BCE' if k else 'MSE'} V={s.V}"
        check_sum(sums, k, ref[1], tol[1], LB.fp32_chain("stream", grid, False, B, s.W, s.V), what)
        if part["g"] is not None:
            check_grad_rows(part["gbuf"], s.W, ref[0], tol[0], f"{what} gradient {g_dt} ld {s.ld_g}")
        for buf, before in part["keep"]:                                              # inputs and their NaN pads: untouched
            assert np.array_equal(bits(buf), before), what
    assert sums[2:].tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("with_g", [False, True])
@pytest.mark.parametrize("wrt_logit", [False, True])
def test_bce_edges_alone(wrt_logit, with_g):
    """One row that consists of the 45 edge pairs of loss_cases.bce_case and nothing else: sums[1] has no ordinary terms to hide
    behind, so every clamped, denormal and saturated term counts against a bound of the size of its own roundings."""
    W = len(LC.P_EDGES) * len(LC.T_EDGES)
    p, t = LC.bce_case(np.random.default_rng(0), 1, W)
    assert set(p.ravel()) == set(LC.P_EDGES) and LC.bce_edge_counts(p, t)["denormal"] == 9
    pred, tgt = dev(p), dev(t)
    g, gbuf = out2d(1, W, W + 3) if with_g else (None, None)
    assert LB.vec_width(W, [(pred.data_ptr(), W, 4)]) == 1 and LB.launch(1, D=W) == (1, False)
    sums = new_sums()
    ops.vae_loss(1, recon_b=pred, b=tgt, sums=sums, g_b=g, grad_b_wrt_logit=wrt_logit)
    torch.cuda.synchronize()
    ref, tol = LB.bce(p, t, wrt_logit, F64), LB.bce_tol(p, t, wrt_logit)
    check_sum(sums, 1, ref[1], tol[1], LB.fp32_chain("stream", 1, False, 1, W, 1), "BCE edges alone")
    if with_g:
        check_grad_rows(gbuf, W, ref[0], tol[0], f"BCE edges alone gradient wrt {'logit' if wrt_logit else 'p'}")
    assert sums[0].item() == 0.0 and sums[2:].tolist() == [0.0, 0.0, 0.0]


# =============================================================================================
# class term
# =============================================================================================
def _class_cases():
    out = [("thread", S, B, S + 4, S + 4) for S in (4, 24, 32) for B in (1, 2, 3, 515)] + [("thread", 4, 131077, 8, 8)]
    # half wave: S % 4 != 0, and S = 24 demoted once by ld_logits = 25 and once by g_c rows with ld_gc = 26
    for S, ldl, ldg in ((1, 2, 4), (22, 23, 25), (31, 32, 34), (24, 25, 28), (24, 24, 26)):
        out += [("half", S, B, ldl, ldg) for B in (1, 2, 3, 515)]
    out += [("half", 22, 40000, 23, 25), ("scalar", 33, 515, 34, 36), ("scalar", 40, 515, 41, 43), ("scalar", 33, 131077, 34, 36)]
    return out


def _mse8(rng, B):
    x, t = LC.mse_case(rng, B, 8)
    return x, t, dev(x), dev(t)


def _run_class(case, weighted, by_device=False):
    path, S, B, ld_logits, ld_gc = case
    rng = np.random.default_rng(1000 * S + B + weighted)
    gamma, beta = 1.7, 0.3
    x, y, cw = LC.class_case(rng, B, S, weighted)
    logits, _ = view2d(x, ld_logits)
    site, cwd = dev(y), None if cw is None else dev(cw)
    form = "scalar" if path == "scalar" else "softmax"
    term_ref, g_ref, n_bad = LB.ce(x, y, cw, gamma, form, F64)
    tol_t, tol_g = LB.ce_tol(x, y, cw, gamma, form)
    ign = y == -100
    assert n_bad == len(range(2, B, 91)) and ign.sum() == len(range(0, B, 7))
    assert (tol_g[ign] == 0).all() and (tol_t[ign] == 0).all()
    x8, t8, x8d, t8d = _mse8(rng, B)
    hyper = dict(beta=99.0, gamma=-5.0, beta_gamma_dev=dev(np.array([beta, gamma], F32))) if by_device else dict(beta=beta, gamma=gamma)
    for tail in (True, False):
        gc, gcbuf = out2d(B, S, ld_gc)
        assert LB.ce_path(S, ld_logits, logits.data_ptr(), ld_gc, gc.data_ptr()) == path, case
        grid, is_tail = LB.launch(B, A=0 if tail else 8, va=4, S=S, path=path)
        assert is_tail == tail
        if B == 131077:
            assert not tail or grid == 512
            assert B > grid * 256 if tail else True                                   # the TAIL grid of 512 x 256 threads goes round twice
        if B == 40000:
            assert grid == (512 if tail else 1024) and B > grid * 8 * (8 if tail else 4) == 32768      # rows of one unrolled pass
        sums = new_sums()
        recon = {} if tail else dict(recon_a=x8d, a=t8d)
        ops.vae_loss(B, logits=logits, site=site, class_weights=cwd, sums=sums, g_c=gc, **recon, **hyper)
        torch.cuda.synchronize()
        what = f"class {path} S={S} B={B} ld {ld_logits}/{ld_gc} {'weighted' if weighted else 'plain'} {'TAIL' if tail else 'with MSE'}"
        assert sums[4].item() == float(n_bad), what                                  # exact, and -100 is not counted
        check_sum(sums, 2, term_ref, tol_t, LB.fp32_chain("class", grid, tail, B, path=path), what)
        inside(host(gcbuf[:, :S]), g_ref, tol_g, what + " g_c")
        assert (gcbuf[:, :S][dev(ign)] == 0).all() and torch.isnan(gcbuf[:, S:]).all(), what
        assert sums[1].item() == 0.0 and sums[3].item() == 0.0
        if tail:
            assert sums[0].item() == 0.0
        else:
            check_sum(sums, 0, LB.mse(x8, t8, F64)[1], LB.mse_tol(x8, t8)[1], LB.fp32_chain("stream", grid, False, B, 8, 4), what)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case", _class_cases(), ids=lambda c: f"{c[0]}-S{c[1]}-B{c[2]}-ld{c[3]}-{c[4]}")
def test_class_term(case, weighted):
    _run_class(case, weighted)


@pytest.mark.parametrize("case", [("thread", 24, 515, 28, 28), ("half", 22, 515, 23, 25), ("scalar", 40, 515, 41, 43)], ids=lambda c: c[0])
def test_class_term_hyperparameters_from_the_device(case):
    """beta_gamma_dev overrides the by-value fields, which are set to wrong values."""
    _run_class(case, True, by_device=True)


# =============================================================================================
# KL term
# =============================================================================================
KL_U = {True: 10, False: 4}     # csrc/elementwise.hip


def _run_kl(B, Ld, tail, class_S=0, passes=None):
    rng = np.random.default_rng(B + Ld)
    beta = 0.25
    mu, lv = LC.kl_case(rng, B, Ld)
    mud, lvd = dev(mu), dev(lv)
    ref, tol = LB.kl(mu, lv, beta, F64), LB.kl_tol(mu, lv, beta)
    extra, path = {}, None
    if class_S:
        x, y, _ = LC.class_case(rng, B, class_S, False)
        path = "thread"
        extra = dict(logits=dev(x), site=dev(y))
        assert LB.ce_path(class_S, class_S, extra["logits"].data_ptr()) == path
    x8, t8, x8d, t8d = _mse8(rng, B)
    if not tail:
        extra.update(recon_a=x8d, a=t8d)
    grid, is_tail = LB.launch(B, A=0 if tail else 8, va=4, S=class_S, path=path, L=Ld)
    assert is_tail == tail
    total, per_pass = B * Ld, grid * 256 * KL_U[tail]
    assert -(-total // per_pass) == passes, (grid, total, per_pass)
    keep = [bits(mud).copy(), bits(lvd).copy()]
    for want_mu, want_lv, by_device in ((1, 1, 0), (1, 0, 1), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        gm = torch.full((B, Ld), NAN, device=DEV) if want_mu else None
        gl = torch.full((B, Ld), NAN, device=DEV) if want_lv else None
        hyper = dict(beta=99.0, gamma=-5.0, beta_gamma_dev=dev(np.array([beta, 1.0], F32))) if by_device else dict(beta=beta)
        sums = new_sums()
        ops.vae_loss(B, mu=mud, logvar=lvd, sums=sums, g_mu=gm, g_lv=gl, **extra, **hyper)
        torch.cuda.synchronize()
        what = f"kl B={B} L={Ld} {'TAIL' if tail else 'with MSE'} grads {want_mu}{want_lv} {'device' if by_device else 'value'} beta"
        check_sum(sums, 3, ref[0], tol[0], LB.fp32_chain("kl", grid, tail, B, W=Ld), what)
        if gm is not None:
            inside(host(gm), ref[1], tol[1], what + " g_mu")
        if gl is not None:
            inside(host(gl), ref[2], tol[2], what + " g_lv")
        assert np.array_equal(bits(mud), keep[0]) and np.array_equal(bits(lvd), keep[1]) and sums[1].item() == 0.0
        assert (sums[2].item() != 0.0) == bool(class_S) and (sums[0].item() != 0.0) == (not tail)


@pytest.mark.parametrize("tail", [True, False], ids=["TAIL", "with-MSE"])
def test_kl_single_element(tail):
    """Fewer elements than one unroll: every clamped preload reads element total - 1 = 0."""
    _run_kl(1, 1, tail, passes=1)


@pytest.mark.parametrize("tail", [True, False], ids=["TAIL", "with-MSE"])
def test_kl_one_pass_clamped_at_the_tail(tail):
    _run_kl(4099, 20, tail, passes=1)


def test_kl_tail_beside_row_per_thread_class_term():
    """B = 300, L = 24 beside S = 24: two workgroups (a row per thread), stride 512, 5120 elements per pass of KL_U = 10: the loop goes
    round twice, the second pass reloads (the first uses the preloaded operands)."""
    _run_kl(300, 24, True, class_S=24, passes=2)


def test_kl_tail_grid_at_its_cap():
    _run_kl(65537, 24, True, passes=2)


# =============================================================================================
# refusals of mmvae_vae_loss
# =============================================================================================
def test_loss_refusals_leave_every_output_untouched():
    B, A, D, S, Ld = 5, 16, 12, 5, 4
    rng = np.random.default_rng(9)
    xa, ta = LC.mse_case(rng, B, A)
    pb, tb = (rng.uniform(0.1, 0.9, (B, D)).astype(F32) for _ in range(2))
    xc = rng.standard_normal((B, S)).astype(F32)
    mu, lv = LC.kl_case(rng, B, Ld)
    ins = [dev(v) for v in (xa, ta, pb, tb, xc, rng.integers(0, S, B).astype(np.int64), mu, lv)]
    outs = [torch.full(s, NAN, device=DEV) for s in ((B, A), (B, D), (B, S), (B, Ld), (B, Ld))]
    sums = new_sums()
    x = L.LossArgs()
    x.B, x.A, x.D, x.S, x.L = B, A, D, S, Ld
    x.recon_a, x.a, x.recon_b, x.b, x.logits, x.site, x.mu, x.logvar = (t.data_ptr() for t in ins)
    x.ld_ra, x.ld_a, x.ld_rb, x.ld_b, x.ld_logits = A, A, D, D, S
    x.g_a, x.g_b, x.g_c, x.g_mu, x.g_lv = (t.data_ptr() for t in outs)
    x.ld_ga, x.ld_gb, x.ld_gc, x.beta, x.gamma, x.sums = A, D, S, 0.5, 1.0, sums.data_ptr()
    x.g_a_dtype = x.g_b_dtype = x.a_dtype = x.b_dtype = L.F32
    lib = L.load()
    before = [bits(t).copy() for t in outs + [sums]]

    def refused(code, **change):
        y = L.LossArgs.from_buffer_copy(x)
        for k, v in change.items():
            setattr(y, k, v)
        assert lib.mmvae_vae_loss(C.byref(y), stream()) == code, change
        torch.cuda.synchronize()
        assert all(np.array_equal(bits(t), b) for t, b in zip(outs + [sums], before)), change

    assert lib.mmvae_vae_loss(None, stream()) == ERR_ARG
    refused(ERR_ARG, sums=None)
    refused(ERR_ARG, B=0)
    refused(ERR_ARG, a=None)                # recon_a without a
    refused(ERR_ARG, site=None)             # logits without site
    refused(ERR_ARG, logvar=None)           # mu without logvar
    refused(ERR_ARG, A=0)
    refused(ERR_DTYPE, a_dtype=7)
    refused(ERR_DTYPE, g_b_dtype=L.BF16)    # g_a_dtype != g_b_dtype (the buffers have the larger, fp32, size)
    # and the same arguments unchanged are taken: the refusals above were not an accident of the set-up
    assert lib.mmvae_vae_loss(C.byref(x), stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in outs) and sums[:4].abs().min().item() > 0


# =============================================================================================
# mmvae_gather_rows: exact
# =============================================================================================
SENT_F, SENT_I = -123.0, -77


def _gather_fixture(rows, src_rows, idx_np):
    rng = np.random.default_rng(rows)
    pairs, checks = [], []
    # (width, source row stride, element offset of the source base, destination row stride); strides > width: views of wider buffers
    for W, lds, shift, ldd in ((782, 784, 0, 790), (781, 783, 0, 785), (572, 572, 1, 572)):
        data = rng.standard_normal((src_rows, W)).astype(F32)
        src, _ = view2d(data, lds, shift)                                            # pads: NaN, must not arrive
        dbuf = torch.full((rows, ldd), SENT_F, device=DEV)
        pairs.append((src, dbuf.as_strided((rows, W), (ldd, 1))))
        checks.append((data, dbuf, W))
    labels = rng.integers(-5, 50, src_rows).astype(np.int64)
    ldst = torch.full((rows,), SENT_I, dtype=torch.int64, device=DEV)
    pairs.append((dev(labels), ldst))
    checks.append((labels, ldst, None))
    word8 = [all(v % 8 == 0 for v in (ops._gather_row(s)[1], ops._gather_row(s)[0], ops._gather_row(d)[0], s.data_ptr(), d.data_ptr())) for s, d in pairs]
    assert word8 == [True, False, False, True]            # 8-byte words; odd width; alignment of the base alone; the int64 labels
    return pairs, checks


def _check_gather(checks, idx_np, src_rows):
    cl = np.clip(idx_np, 0, src_rows - 1)
    for data, dbuf, W in checks:
        if W is None:
            assert np.array_equal(dbuf.cpu().numpy(), data[cl])
            continue
        want = np.full(tuple(dbuf.shape), SENT_F, F32)
        want[:, :W] = data[cl]
        assert np.array_equal(bits(dbuf), want.view(np.int32)), W                    # the rows bit for bit, the pads still the sentinel


@pytest.mark.parametrize("rows", [1, 5000])
def test_gather_rows_four_items_both_word_paths(rows):
    src_rows = 300
    rng = np.random.default_rng(rows)
    special = np.array([0, src_rows - 1, -1, src_rows, 2 ** 40, -2 ** 62, 17, 17, 17], np.int64)      # ends, out of range, duplicates
    idx_np = rng.integers(0, src_rows, rows).astype(np.int64)
    if rows == 1:
        idx_np[:] = src_rows                                                         # clamps to the last row
    else:
        idx_np[:len(special)] = special
        assert rows * 4 > 4096 * 4                                                   # more waves than the capped grid holds: the loop goes round
    pairs, checks = _gather_fixture(rows, src_rows, idx_np)
    ops.gather_rows(pairs, dev(idx_np), src_rows)
    torch.cuda.synchronize()
    _check_gather(checks, idx_np, src_rows)


@pytest.mark.parametrize("idx", [-1, 2 ** 40, -2 ** 62, 0, 299, 300])
def test_gather_rows_single_row_clamps(idx):
    idx_np = np.array([idx], np.int64)
    pairs, checks = _gather_fixture(1, 300, idx_np)
    ops.gather_rows(pairs, dev(idx_np), 300)
    torch.cuda.synchronize()
    _check_gather(checks, idx_np, 300)


def test_gather_rows_refusals_write_nothing():
    rows, src_rows, W = 6, 9, 10
    src = dev(np.random.default_rng(0).standard_normal((src_rows, W)).astype(F32))
    dst = torch.full((rows, W + 2), SENT_F, device=DEV)
    idx = dev(np.arange(rows, dtype=np.int64))
    before = bits(dst).copy()
    lib = L.load()
    good = dict(src=src.data_ptr(), dst=dst.data_ptr(), src_row_stride=W * 4, dst_row_stride=(W + 2) * 4, row_bytes=W * 4)

    def call(n_struct, n_items, idx_ptr, rows_, src_rows_, **change):
        items = (L.GatherItem * max(n_struct, 1))()
        for k in range(n_struct):
            f = dict(good, **(change if k == n_struct - 1 else {}))
            items[k] = L.GatherItem(f["src"], f["dst"], f["src_row_stride"], f["dst_row_stride"], f["row_bytes"], 0)
        rc = lib.mmvae_gather_rows(C.cast(items, C.c_void_p), n_items, idx_ptr, rows_, src_rows_, stream())
        torch.cuda.synchronize()
        assert np.array_equal(bits(dst), before), (n_items, rows_, src_rows_, change)
        return rc

    ip = idx.data_ptr()
    assert call(5, 5, ip, rows, src_rows) == ERR_ARG                                 # one more than MMVAE_GATHER_MAX
    assert call(1, 0, ip, rows, src_rows) == ERR_ARG
    assert call(1, 1, ip, 0, src_rows) == ERR_ARG
    assert call(1, 1, ip, rows, 0) == ERR_ARG
    assert call(1, 1, None, rows, src_rows) == ERR_ARG
    assert lib.mmvae_gather_rows(None, 1, ip, rows, src_rows, stream()) == ERR_ARG
    for change in (dict(src=None), dict(dst=None), dict(row_bytes=0), dict(row_bytes=6), dict(src_row_stride=6), dict(dst_row_stride=6),
                   dict(dst=dst.data_ptr() + 2)):
        assert call(1, 1, ip, rows, src_rows, **change) == ERR_ARG, change
        assert call(2, 2, ip, rows, src_rows, **change) == ERR_ARG, change           # the second item is the bad one
    items = (L.GatherItem * 1)(L.GatherItem(good["src"], good["dst"], good["src_row_stride"], good["dst_row_stride"], good["row_bytes"], 0))
    assert lib.mmvae_gather_rows(C.cast(items, C.c_void_p), 1, ip, rows, src_rows, stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(dst[:, :W]), bits(src[:rows]))                        # and the unchanged arguments are taken
