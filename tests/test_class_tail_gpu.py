"""mmvae_class_tail (the class decoder's last Linear + the class / KL terms of vae_loss + the Linear's dX in ONE launch) against the
three entry points it replaces -- mmvae_gemm_nt (logits), mmvae_vae_loss with only logits / mu / logvar given, mmvae_gemm_nt with the
ReLU-mask epilogue (dX) -- on the same inputs, and the training step with tuning key 12 on against off.

Bit identity (torch.equal) is asked of everything that is a function of one row: the fp32 class gradient, the class decoder's columns
of D0, the KL gradients, the count of labels out of range.  The fused kernel uses the same MFMA with K ascending, the same fp32
bias add, the per-row arithmetic of loss_terms.h and the same bf16 roundings.  The class and KL SUMS are f64 additions of per-row
(per-element) fp32 terms that both forms compute alike and widen one by one; they differ by the order of those additions only, which
is bounded by (n - 1) 2^-53 sum |t_i| over the n terms, with sum |t_i| from a float64 recomputation of the terms here."""
import numpy as np
import pytest
import torch

from golden_util import load
from model_util import load_state, masks_list, named_grads, scaled_err, CHAOTIC_BIASES
from mmvae import _lib, engine, ops
from mmvae import functional as F_
from mmvae.optim import FusedAdamW
from src.models import MultiModalVAE

import np_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
PREC = ops.PREC_BF16
S, L, HID, NSTEM, OFF = 24, 20, 64, 448, 384       # sites, latent, DecoderC's hidden width, merged stems, DecoderC's first column
KEY = 12
SENT = -3.0


def _set_tuning(key, value):
    _lib.check(_lib.load().mmvae_set_tuning(key, value), "mmvae_set_tuning")


class _Case:
    """One class head: the merged hidden activation H0 (exact zeros in DecoderC's columns: relu of a normal sample), labels with one
    at S - 1, one out of range and one ignored, mu / logvar, the prepared Linear."""

    def __init__(self, B, weights, n_sites=S, seed=0):
        g = torch.Generator().manual_seed(100 * seed + B)
        self.B, self.S = B, n_sites
        self.H0 = torch.relu(torch.randn(B, NSTEM, generator=g)).to(torch.bfloat16).to(DEV)
        self.h0 = self.H0[:, OFF:OFF + HID]
        assert bool((self.h0 == 0).any()) and bool((self.h0 > 0).any())
        site = torch.randint(0, n_sites, (B,), generator=g)
        site[0], site[1], site[B - 1] = n_sites - 1, n_sites + 3, n_sites - 1
        site[2] = -100
        site[3] = -1
        self.site = site.to(DEV)
        self.mu = torch.randn(B, L, generator=g).to(DEV)
        self.logvar = (torch.randn(B, L, generator=g) * 0.7).to(DEV)
        self.cw = (torch.rand(n_sites, generator=g) + 0.5).to(DEV) if weights else None
        w = (torch.randn(n_sites, HID, generator=g) / HID ** 0.5).to(DEV)
        b = (torch.randn(n_sites, generator=g) * 0.1).to(DEV)
        self.head = ops.PreparedLinear([w], [b], PREC, DEV)
        ops.WeightPrep([self.head], DEV).run()
        self.beta, self.gamma = 1e-3, 0.7
        self.hyper = torch.tensor([2e-3, 1.3], dtype=torch.float32, device=DEV)

    def outputs(self):
        B = self.B
        mk = lambda *shape, dt: torch.full(shape, SENT, dtype=dt, device=DEV)          # a sentinel: what must be written, and only that
        sums, out5 = ops.loss_workspace(DEV)
        return dict(gc=mk(B, self.S, dt=torch.float32), D0=mk(B, NSTEM, dt=torch.bfloat16), g_mu=mk(B, L, dt=torch.float32),
                    g_lv=mk(B, L, dt=torch.float32), sums=sums, out5=out5)

    def run(self, fused, dev_hyper=False, prec=PREC):
        B, o = self.B, self.outputs()
        bg = self.hyper if dev_hyper else None
        d0 = o["D0"][:, OFF:OFF + HID]
        if fused:
            ops.class_tail(prec, B, self.h0, self.head, self.site, self.cw, self.mu, self.logvar, self.beta, self.gamma, o["sums"],
                           o["gc"], d0, o["g_mu"], o["g_lv"], beta_gamma_dev=bg)
        else:
            o["logits"] = torch.empty(B, self.S, dtype=torch.float32, device=DEV)
            ops.gemm_nt(PREC, self.h0, self.head.w, self.S, HID, o["logits"], bias=self.head.bias)
            ops.vae_loss(B, logits=o["logits"], site=self.site, class_weights=self.cw, mu=self.mu, logvar=self.logvar, beta=self.beta,
                         gamma=self.gamma, sums=o["sums"], g_c=o["gc"], g_mu=o["g_mu"], g_lv=o["g_lv"], beta_gamma_dev=bg)
            ops.gemm_nt(PREC, o["gc"], self.head.wt, HID, self.S, d0, epilogue=ops.EPI_RELU_MASK, h=self.h0)
        ops.loss_finalize(o["sums"], self.beta, self.gamma, o["out5"], bg)
        torch.cuda.synchronize()
        return o

    def abs_term_sums(self, logits):
        """(sum |t_i| of the class terms, of the KL terms) in float64, from the logits the unfused form wrote."""
        x = logits.double()
        y = self.site.clone()
        ign = y == -100
        y[ign | (y < 0) | (y >= self.S)] = 0
        w = (self.cw.double()[y] if self.cw is not None else torch.ones_like(x[:, 0]))
        w = torch.where(ign, torch.zeros_like(w), w)
        t_cls = w * (torch.logsumexp(x, 1) - x.gather(1, y[:, None])[:, 0])
        mu, lv = self.mu.double(), self.logvar.double()
        t_kl = -0.5 * (1.0 + lv - mu * mu - torch.exp(lv))
        return float(t_cls.abs().sum()), float(t_kl.abs().sum())


def _ulps(a, b):
    """Distance of two fp32 values in units of the last place of the larger."""
    a, b = np.float32(a), np.float32(b)
    if a == b:
        return 0.0
    return float(abs(np.float64(a) - np.float64(b)) / np.spacing(max(abs(a), abs(b))))


def _compare(c, want, got):
    for k in ("gc", "D0", "g_mu", "g_lv"):
        assert torch.equal(want[k], got[k]), (k, int((want[k] != got[k]).sum()), want[k].numel())
    # D0 outside DecoderC's columns: untouched by both forms; inside: every element written
    for o in (want, got):
        assert bool((o["D0"][:, :OFF] == SENT).all()) and bool((o["D0"][:, OFF + HID:] == SENT).all())
    assert not bool((got["gc"] == SENT).any()) and not bool((got["g_mu"] == SENT).any()) and not bool((got["g_lv"] == SENT).any())
    assert bool((got["D0"][:, OFF:OFF + HID][c.h0 == 0] == 0).all())                   # the ReLU mask
    assert bool((got["D0"][:, OFF:OFF + HID] != 0).any())
    sw, sg = want["sums"].cpu().numpy(), got["sums"].cpu().numpy()
    assert sw[0] == sg[0] == 0.0 and sw[1] == sg[1] == 0.0
    assert sw[4] == sg[4] == 2.0, (sw[4], sg[4])                                       # labels S + 3 and -1; -100 is ignored, not counted
    abs_cls, abs_kl = c.abs_term_sums(want["logits"])
    u = 2.0 ** -53
    for i, n, tot, what in ((2, c.B, abs_cls, "class"), (3, c.B * L, abs_kl, "KL")):
        bound = (n - 1) * u * tot
        print(f"\n[class_tail B={c.B}] {what} sum: unfused {sw[i]!r} fused {sg[i]!r} |diff| {abs(sw[i] - sg[i]):.3e} bound {bound:.3e}")
        assert abs(sw[i] - sg[i]) <= bound, (what, sw[i], sg[i], bound)
    lw, lf = want["out5"].cpu().numpy(), got["out5"].cpu().numpy()
    for i in range(5):
        same_sums = sw[2] == sg[2] and sw[3] == sg[3]
        assert _ulps(lw[i], lf[i]) <= (0.0 if same_sums else 1.0), (i, lw[i], lf[i])


@pytest.mark.parametrize("weights", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("B", [16, 77, 4099])
def test_fused_class_head_against_three_launches(B, weights):
    """B = 16: one slab in one wave; 77: a ragged last slab (13 rows); 4099: 257 slabs on 33 workgroups' waves -- at most one slab per
    wave there, so the prefetch loop's second trip is covered by the B = 70 000 case below -- and a last slab of 3 rows."""
    c = _Case(B, weights)
    _compare(c, c.run(False), c.run(True))


def test_several_slabs_per_wave_and_device_hyperparameters():
    """B = 70 003: 4376 slabs on 2048 resident waves -- every wave carries two or three slabs through its loop, with the next slab's
    loads in flight, and the last slab has 3 rows; beta / gamma read from device memory."""
    c = _Case(70003, True, seed=1)
    _compare(c, c.run(False, dev_hyper=True), c.run(True, dev_hyper=True))


def test_s32_fills_both_column_tiles():
    c = _Case(333, True, n_sites=32, seed=2)
    _compare(c, c.run(False), c.run(True))


def _refused(c, call):
    o = c.outputs()
    before = {k: v.clone() for k, v in o.items()}
    with pytest.raises(_lib.MMVAEArgError):
        call(o)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(v, o[k]), k


def test_refusals_enqueue_nothing():
    """S = 33, fp32 mode and the tuning key off: MMVAE_ERR_ARG, every output and the sums untouched."""
    B = 77
    c = _Case(B, True, seed=3)
    lib = _lib.load()

    def call(case, prec=PREC):
        def f(o):
            ops.class_tail(prec, B, case.h0, case.head, case.site, case.cw, case.mu, case.logvar, case.beta, case.gamma, o["sums"], o["gc"],
                           o["D0"][:, OFF:OFF + HID], o["g_mu"], o["g_lv"])
        return f

    c33 = _Case(B, True, n_sites=33, seed=3)
    _refused(c33, call(c33))
    _refused(c, call(c, ops.PREC_F32))
    try:
        _set_tuning(KEY, 0)
        _refused(c, call(c))
        assert not ops.class_tail_fits(PREC, S, HID, L, NSTEM, NSTEM)
    finally:
        _set_tuning(KEY, 1)
    # the raw entry point answers MMVAE_ERR_ARG (-1) for each, and for what the wrapper cannot produce
    import ctypes as C
    stream = torch.cuda.current_stream().cuda_stream

    def raw(mutate):
        o = c.outputs()
        a, _ = ops.class_tail_args(PREC, B, c.h0, c.head, c.site, c.cw, c.mu, c.logvar, c.beta, c.gamma, o["sums"], o["gc"],
                                   o["D0"][:, OFF:OFF + HID], o["g_mu"], o["g_lv"])
        mutate(a)
        rc = lib.mmvae_class_tail(C.byref(a), stream)
        torch.cuda.synchronize()
        assert bool((o["gc"] == SENT).all()) and bool((o["D0"] == SENT).all()) and bool((o["g_mu"] == SENT).all()) and float(o["sums"].abs().sum()) == 0.0
        return rc

    cases = {"S = 33": lambda a: setattr(a, "S", 33), "S % 4": lambda a: setattr(a, "S", 22), "fp32": lambda a: setattr(a, "prec", ops.PREC_F32),
             "hidden": lambda a: setattr(a, "hidden", 128), "L > 24": lambda a: setattr(a, "L", 25), "B = 0": lambda a: setattr(a, "B", 0),
             "ldh0 % 8": lambda a: setattr(a, "ldh0", NSTEM + 4), "ldd0 % 64": lambda a: setattr(a, "ldd0", NSTEM + 8),
             "d0 not 128-byte aligned": lambda a: setattr(a, "d0", a.d0 + 64), "h0 not 16-byte aligned": lambda a: setattr(a, "h0", a.h0 + 8),
             "ld_gc < S": lambda a: setattr(a, "ld_gc", 20), "no site": lambda a: setattr(a, "site", None), "no mu": lambda a: setattr(a, "mu", None)}
    for name, m in cases.items():
        assert raw(m) == -1, name
    assert lib.mmvae_class_tail_fits(PREC, 33, HID, L, NSTEM, NSTEM) == -1 and lib.mmvae_class_tail_fits(ops.PREC_F32, S, HID, L, NSTEM, NSTEM) == -1
    assert lib.mmvae_class_tail_fits(PREC, S, HID, L, NSTEM, NSTEM) == 0
    assert lib.mmvae_set_tuning(11, 1) == -1


# ----------------------------------------------------------------------------------------------------------------------------------
# the whole step through the engine: tuning key 12 off (today's three launches) against on, from the same seeded start
# ----------------------------------------------------------------------------------------------------------------------------------
def _fixture_step(on, unit_grad, probe=False, defer=True):
    """The captured training step's launch sequence (reconstruction losses inside the decoder GEMMs, the class head left to the loss as
    mmvae.graphs asks for it -- defer --, fused loss, backward) issued
    eagerly on tests/golden/mm_default_b77_w's batch, parameters, class weights and injected noise (a capture cannot take injected
    noise) -> (out5 floats, {name: gradient}, launch tags, fixture, the forward's class logits)."""
    fx = load("mm_default_b77_w")
    A, D, S_, L_, E = [int(x) for x in fx["dims"]]
    B, seed = int(fx["B"]), int(fx["seed"])
    t = lambda x: torch.from_numpy(np.asarray(x)).to(DEV)
    P, Bf = O.make_params(seed, A, D, S_, L_, E)
    model = load_state(MultiModalVAE(A, D, S_, L_, embed_dim=E), P, Bf).to(DEV).set_precision("bf16").train()
    a, b, site, cw = t(fx["a"]), t(fx["b"]), t(fx["site"]), t(fx["class_weights"])
    masks, eps = O.make_noise(seed + 100, B, L_)
    _set_tuning(KEY, int(on))
    ops.PROBE = ops.KernelProbe() if probe else None
    try:
        engine.GLOBAL_NOISE.inject(masks_list(masks), torch.from_numpy(eps))
        g = model._graph()
        g.fused_recon, g.defer_class_head = [a, b, None], defer
        try:
            ra, rb, rc, mu, lv = model(a=a, b=b, site=site)
        finally:
            g.fused_recon, g.defer_class_head = None, False
            engine.GLOBAL_NOISE.clear()
        total, out5 = F_.fused_loss({"a": (ra, a), "b": (rb, b), "c": (rc, site), "kl": (mu, lv)}, float(fx["beta"]), float(fx["gamma"]),
                                    class_weights=cw, unit_grad=unit_grad)
        total.backward()
        torch.cuda.synchronize()
        tags = set(ops.PROBE.records) if probe else set()
    finally:
        ops.PROBE = None
        _set_tuning(KEY, 1)
    return out5.cpu().numpy(), named_grads(model), tags, fx, rc.detach()


_STEP = {}
# EncoderC's five gradients come out of the table gradient, which mmvae_fuse_reparam_bwd accumulates with unordered fp32 atomics: the
# unfused step differs from ITSELF there by an ulp from run to run, whatever the class head does (its inputs -- g_mu, g_lv and dL/dz --
# are bit-identical, or the encoders' gradients in front of them in the comparison would differ too).
ATOMIC = ("encoder_c.",)


def _same_gradients(old, old_again, new):
    """Every gradient bit-identical to the unfused step's; the tensors behind unordered fp32 atomics within 4 x what the unfused step
    differs from itself by (measured here, at least one ulp at the tensor's largest magnitude: one pair of runs is one sample)."""
    as_np = lambda x: x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()
    for k in old:
        a, a2, b = as_np(old[k]), as_np(old_again[k]), as_np(new[k])
        if k.startswith(ATOMIC):
            floor = max(float(np.abs(a - a2).max()), float(np.abs(a).max()) * 2.0 ** -23)
            assert float(np.abs(a - b).max()) <= 4.0 * floor, (k, float(np.abs(a - b).max()), floor)
        else:
            assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))


def _step(on, unit_grad=True):
    if (on, unit_grad) not in _STEP:
        _STEP[(on, unit_grad)] = _fixture_step(on, unit_grad, probe=True)
    return _STEP[(on, unit_grad)]


def test_step_takes_the_fused_launch_and_equals_the_unfused_step():
    """B = 77: the step with key 12 on issues class_tail and neither DecoderC.L1.fwd nor DecoderC.L1.dX; with the key off it issues
    today's launches.  The gradients are bit-identical (EncoderC's: within the unfused step's own run-to-run difference, see ATOMIC), the
    loss floats equal or one ulp apart (the order of the f64 additions)."""
    l0, g0, tags0, _, _ = _step(False)
    l1, g1, tags1, _, _ = _step(True)
    assert "class_tail" in tags1 and "DecoderC.L1.fwd" not in tags1 and "DecoderC.L1.dX" not in tags1 and "vae_loss" not in tags1, sorted(tags1)
    assert "class_tail" not in tags0 and {"DecoderC.L1.fwd", "DecoderC.L1.dX", "vae_loss"} <= tags0, sorted(tags0)
    assert len(g0) == 39
    _same_gradients(g0, _fixture_step(False, True)[1], g1)
    for i in range(5):
        assert _ulps(l0[i], l1[i]) <= 1.0, (i, l0[i], l1[i])


def test_step_without_unit_grad_stays_on_the_three_launches():
    """unit_grad off (the loss's gradient is rescaled afterwards): the loss issues the Linear the forward left out and today's loss
    launch, the backward its dX; gradients bit-identical to the step with the key off."""
    l0, g0, _, _, _ = _step(False)
    l2, g2, tags2, _, _ = _step(True, unit_grad=False)
    assert "class_tail" not in tags2 and {"DecoderC.L1.fwd", "DecoderC.L1.dX", "vae_loss"} <= tags2, sorted(tags2)
    _same_gradients(g0, g0, g2)
    for i in range(5):
        assert _ulps(l0[i], l2[i]) <= 1.0, (i, l0[i], l2[i])


def test_forward_that_was_not_asked_to_defer_returns_the_logits():
    """Reconstruction losses inside the decoder GEMMs WITHOUT defer_class_head (a caller of model() that reads the class logits, key 12
    on): the forward runs DecoderC's last Linear and returns logits with storage behind them, bit-identical to those of the step with
    the key off; the loss then issues today's launches and the gradients are those of the unfused step."""
    l0, g0, _, fx, rc0 = _step(False)
    l3, g3, tags3, _, rc3 = _fixture_step(True, True, probe=True, defer=False)
    assert rc3.shape == (int(fx["B"]), int(fx["dims"][2])) and rc3.stride() == (rc3.shape[1], 1)
    assert torch.equal(rc3, rc0) and bool(rc3.abs().max() > 0)
    assert "class_tail" not in tags3 and {"DecoderC.L1.fwd", "DecoderC.L1.dX", "vae_loss"} <= tags3, sorted(tags3)
    _same_gradients(g0, g0, g3)
    for i in range(5):
        assert _ulps(l0[i], l3[i]) <= 1.0, (i, l0[i], l3[i])


def test_step_matches_the_golden_fixture():
    """The fused step against the reference's step 0 of mm_default_b77_w, within the bf16 bounds of the existing full-step tests
    (tests/test_model_gpu.py TOL["bf16"]: losses 3e-3 relative; gradients 0.12 Frobenius-relative, 0.25 scaled max per tensor)."""
    l1, g1, _, fx, _ = _step(True)
    assert l1[4] == 0.0
    np.testing.assert_allclose(l1[:4], fx["s0.loss"], rtol=3e-3)
    g1 = {k: g for k, g in g1.items() if k not in CHAOTIC_BIASES}       # analytically zero (a bias in front of BatchNorm): noise on both sides
    for k, g in g1.items():
        key = "s0.grad." + k
        if key not in fx.files:
            continue                                       # large tensors are stored as samples: covered by the element check below
        ref = fx[key].astype(np.float64)
        fro = float(np.linalg.norm(g - ref) / max(np.linalg.norm(ref), 1e-30))
        print(f"[class_tail step vs golden] {k}: Frobenius-rel {fro:.3e} scaled max {scaled_err(g, ref):.3e}")
        assert fro <= 0.12 and scaled_err(g, ref) <= 0.25, (k, fro, scaled_err(g, ref))
    for k, g in g1.items():
        if ("s0.grad." + k + "@idx") in fx.files:
            idx, val = fx["s0.grad." + k + "@idx"], fx["s0.grad." + k + "@val"].astype(np.float64)
            assert float(np.abs(g.reshape(-1)[idx] - val).max()) <= 0.25 * float(np.abs(val).max()), k


@pytest.mark.parametrize("replay", [True, False], ids=["replayed", "run_eager"])
def test_captured_step_fused_against_unfused(replay):
    """One captured training step at B = 77 (GraphedTrainStep, class weights, Philox noise from the same offset) with key 12 on
    against off: gradients bit-identical (EncoderC's: see ATOMIC), loss floats equal or one ulp apart."""
    from mmvae.graphs import GraphedTrainStep
    B, A_DIM, D_DIM = 77, 782, 572
    g = torch.Generator().manual_seed(5)
    a = torch.randn(B, A_DIM, generator=g).to(DEV)
    b = (torch.rand(B, D_DIM, generator=g) < 0.3).float().to(DEV)
    site = torch.randint(0, S, (B,), generator=g).to(DEV)
    cw = (torch.rand(S, generator=g) + 0.5).to(DEV)
    res = []
    for on in (0, 0, 1):
        _set_tuning(KEY, on)
        try:
            torch.manual_seed(321)
            m = MultiModalVAE(A_DIM, D_DIM, S, L).to(DEV).train()
            engine.GLOBAL_NOISE.offset_tensor(torch.device(DEV, torch.cuda.current_device())).zero_()
            opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
            gs = GraphedTrainStep(m, opt, a, b, site, class_weights=cw, warmup=1, preserve_state=True)
            if replay:
                gs()
                out5 = gs.out4.cpu().numpy()
            else:
                out5 = gs.run_eager().cpu().numpy()
            torch.cuda.synchronize()
            res.append((out5, {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
        finally:
            _set_tuning(KEY, 1)
    (l0, g0), (_, g0b), (l1, g1) = res
    assert len(g0) == 39
    _same_gradients(g0, g0b, g1)
    for i in range(5):
        assert _ulps(l0[i], l1[i]) <= 1.0, (i, l0[i], l1[i])
