"""mmvae_latent_fwd (heads + mean fusion + reparameterisation + decoder stems in ONE launch) against the four entry points it
replaces -- mmvae_gemm_nt (heads of EncoderA / EncoderB, BatchNorm finalisation folded in), mmvae_fuse_reparam_fwd and mmvae_gemm_nt
(merged decoder first layers) -- on the same inputs.  The target is bit identity: the fused kernel applies the same operand prologue
(SrcBnReluDrop), the same MFMA with K ascending, the same fp32 bias / fusion / reparameterisation arithmetic (fuse_math.h) and the
same bf16 roundings, so every comparison below is torch.equal (NaN rows: equal with NaNs in the same places)."""
import itertools

import numpy as np
import pytest
import torch

from mmvae import _lib, engine, ops
from mmvae.optim import FusedAdamW
from src.models import MultiModalVAE

pytestmark = pytest.mark.gpu
DEV = "cuda"
KA, KB, L, S, NSTEM = 128, 256, 20, 24, 448          # the model's shapes: last hidden widths, latent, sites, merged stems
PREC = ops.PREC_BF16
SUBSETS = [s for s in itertools.product((False, True), repeat=3) if any(s)]


def _set_tuning(key, value):
    _lib.check(_lib.load().mmvae_set_tuning(key, value), "mmvae_set_tuning")


class _Enc:
    """One encoder's operands: the last layer's pre-BatchNorm output, its f64 column sums, BatchNorm parameters and state, keep mask."""

    def __init__(self, g, B, K, train):
        self.K, self.train = K, train
        self.y = (torch.randn(B, K, generator=g) * 1.5 + 0.3).to(torch.bfloat16).to(DEV)
        yd = self.y.double()
        self.stats = torch.stack([yd.sum(0), (yd * yd).sum(0)]).contiguous()
        self.gamma = (torch.rand(K, generator=g) + 0.5).to(DEV)
        self.beta = (torch.randn(K, generator=g) * 0.2).to(DEV)
        self.mask = (torch.rand(B, K, generator=g) < 0.9).to(torch.uint8).to(DEV) if train else None
        self.rm0 = (torch.randn(K, generator=g) * 0.1).to(DEV)
        self.rv0 = (torch.rand(K, generator=g) + 0.5).to(DEV)
        w = [torch.randn(L, K, generator=g).to(DEV) / K ** 0.5 for _ in range(2)]
        b = [torch.randn(L, generator=g).to(DEV) * 0.1 for _ in range(2)]
        self.pl = ops.PreparedLinear(w, b, PREC, DEV)

    def fresh(self):
        """BatchNorm state of one run: (BNState, running_mean, running_var, num_batches_tracked, Prologue, BnFinalizeArgs or None)."""
        B = self.y.shape[0]
        st = engine.BNState(self.K, DEV)
        st.buf.fill_(-7.0)
        rm, rv, nbt = self.rm0.clone(), self.rv0.clone(), torch.full((), 3, dtype=torch.int64, device=DEV)
        if self.train:
            fin = ops.bn_finalize_args(B, self.K, self.stats, self.gamma, self.beta, rm, rv, nbt, st.mean, st.rstd, st.scale, st.shift)
            pro = ops.Prologue(st.scale, st.shift, self.mask, 1.0 / 0.9)
        else:
            fin = None
            ops.bn_eval_coeffs(self.gamma, self.beta, rm, rv, st.scale, st.shift, 1e-5, st.mean, st.rstd)
            pro = ops.Prologue(st.scale, st.shift, None, 1.0)
        return st, rm, rv, nbt, pro, fin


class _Case:
    def __init__(self, B, has_a, has_b, has_c, train, seed=0, bad_label=None):
        g = torch.Generator().manual_seed(1000 * seed + B)
        self.B = B
        self.enc = [_Enc(g, B, K, train) if on else None for on, K in ((has_a, KA), (has_b, KB))]
        self.table = (torch.randn(S, 2 * L, generator=g) * 0.5).to(DEV) if has_c else None
        self.site = torch.randint(0, S, (B,), generator=g).to(DEV) if has_c else None
        if bad_label is not None:
            self.site[bad_label[0]] = bad_label[1]
        self.eps = torch.randn(B, L, generator=g).to(DEV)
        ws = [torch.randn(n, L, generator=g).to(DEV) / L ** 0.5 for n in (128, 256, 64)]
        bs = [torch.randn(n, generator=g).to(DEV) * 0.1 for n in (128, 256, 64)]
        self.stem = ops.PreparedLinear(ws, bs, PREC, DEV)
        ops.WeightPrep([e.pl for e in self.enc if e is not None] + [self.stem], DEV).run()

    def outputs(self):
        B = self.B
        mk = lambda *shape, dt: torch.full(shape, -3.0, dtype=dt, device=DEV)          # a sentinel: every element must be written
        return dict(mu=mk(B, L, dt=torch.float32), logvar=mk(B, L, dt=torch.float32), z=mk(B, 24, dt=torch.bfloat16),
                    h0=mk(B, NSTEM, dt=torch.bfloat16))

    def run(self, fused):
        B = self.B
        o = self.outputs()
        states = [e.fresh() if e is not None else None for e in self.enc]
        if fused:
            owed = [ops.LatentEncoder(e.y, s[4], s[5], e.pl) if e is not None else None for e, s in zip(self.enc, states)]
            ops.latent_fwd(PREC, B, L, owed[0], owed[1], self.table, self.site, self.eps, o["mu"], o["logvar"], o["z"], self.stem, o["h0"])
        else:
            heads = [None, None]
            for i, (e, s) in enumerate(zip(self.enc, states)):
                if e is not None:
                    heads[i] = torch.empty(B, 2 * L, dtype=torch.float32, device=DEV)
                    ops.gemm_nt(PREC, e.y, e.pl.w, 2 * L, e.K, heads[i], bias=e.pl.bias, prologue=s[4], pro_finalize=s[5])
            ops.fuse_reparam_fwd(B, L, heads[0], heads[1], self.table, self.site, self.eps, o["mu"], o["logvar"], o["z"])
            ops.gemm_nt(PREC, o["z"], self.stem.w, NSTEM, L, o["h0"], bias=self.stem.bias, act=ops.ACT_RELU)
        torch.cuda.synchronize()
        for i, s in enumerate(states):
            if s is not None:
                o.update({f"bn{i}": s[0].buf, f"rm{i}": s[1], f"rv{i}": s[2], f"nbt{i}": s[3]})
        return o


def _same(a, b):
    """Bit-identical as numbers (torch.equal), NaNs allowed in the same places."""
    if a.dtype.is_floating_point:
        na, nb = torch.isnan(a), torch.isnan(b)
        return bool(torch.equal(na, nb)) and bool(torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b)))
    return bool(torch.equal(a, b))


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "".join(c for c, on in zip("abc", s) if on))
@pytest.mark.parametrize("B", [2, 77, 4096, 65536])
def test_fused_forward_is_bit_identical(B, subset, train):
    """mu, logvar, z (pad columns included), H0, the saved mean / rstd / scale / shift, the running statistics and the batch counter
    of the fused launch == those of today's four launches: torch.equal on every one."""
    c = _Case(B, *subset, train)
    want, got = c.run(False), c.run(True)
    assert set(want) == set(got)
    for k in want:
        assert torch.equal(want[k], got[k]), (k, int((want[k] != got[k]).sum()), want[k].numel())
    assert not bool((got["z"][:, L:] != 0).any())
    if train:
        for i, e in enumerate(c.enc):
            if e is not None:
                assert int(got[f"nbt{i}"]) == 4 and not bool((got[f"bn{i}"] == -7.0).any())


@pytest.mark.parametrize("label", [-1, S, 2 ** 40])
def test_out_of_range_label_poisons_its_own_row_only(label):
    """A label outside [0, S): that row is NaN in mu / logvar / z (as mmvae_fuse_reparam_fwd does it), every other row is what the
    valid labels give, nothing outside the table is read; and the backward scatters nothing for it."""
    B, row = 333, 100
    c = _Case(B, True, True, True, True, seed=2, bad_label=(row, label))
    want, got = c.run(False), c.run(True)
    for k in want:
        assert _same(want[k], got[k]), k
    assert bool(torch.isnan(got["mu"][row]).all()) and bool(torch.isnan(got["logvar"][row]).all()) and bool(torch.isnan(got["z"][row, :L].float()).all())
    others = torch.arange(B, device=DEV) != row
    for k in ("mu", "logvar", "z", "h0"):
        assert not bool(torch.isnan(got[k][others].float()).any()), k
    clean = _Case(B, True, True, True, True, seed=2)
    ref = clean.run(True)
    keep = others & (clean.site == c.site)
    for k in ("mu", "logvar", "z", "h0"):
        assert torch.equal(ref[k][keep], got[k][keep]), k
    # backward: no scatter for the poisoned row
    dz = torch.randn(B, L, device=DEV)
    d_heads = torch.empty(B, 2 * L, device=DEV)
    d_table = torch.zeros(1, S, 2 * L, device=DEV)
    lv = torch.where(torch.isnan(got["logvar"]), torch.zeros_like(got["logvar"]), got["logvar"])
    ops.fuse_reparam_bwd(B, L, 3, None, None, [dz], c.eps, lv, d_heads, d_table, c.site)
    torch.cuda.synchronize()
    exp = torch.zeros(S, 2 * L, dtype=torch.float64, device=DEV)
    exp.index_add_(0, c.site[others], d_heads[others].double())
    np.testing.assert_allclose(d_table[0].cpu().numpy(), exp.cpu().numpy(), rtol=1e-4, atol=1e-4)


def _refused(c, mutate, exc=_lib.MMVAEArgError):
    """The call raises and leaves every output, the BatchNorm vectors and the running statistics untouched."""
    o = c.outputs()
    states = [e.fresh() if e is not None else None for e in c.enc]
    owed = [ops.LatentEncoder(e.y, s[4], s[5], e.pl) if e is not None else None for e, s in zip(c.enc, states)]
    kw = dict(prec=PREC, B=c.B, Ld=L, enc_a=owed[0], enc_b=owed[1], table=c.table, site=c.site, eps=c.eps, mu=o["mu"], logvar=o["logvar"],
              z=o["z"], stem=c.stem, h0=o["h0"])
    mutate(kw)
    before = {k: v.clone() for k, v in o.items()}
    with pytest.raises(exc):
        ops.latent_fwd(**kw)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert _same(v, o[k]), k
    for e, s in zip(c.enc, states):
        if e is not None:
            assert bool((s[0].buf == -7.0).all()) and torch.equal(s[1], e.rm0) and torch.equal(s[2], e.rv0) and int(s[3]) == 3


def test_refusals_leave_everything_untouched():
    """Every documented limit answers MMVAE_ERR_ARG / MMVAE_ERR_DTYPE before anything is enqueued."""
    B = 512
    c = _Case(B, True, True, True, True, seed=3)
    g = torch.Generator().manual_seed(9)

    def wide_latent(kw):            # the scaled config's latent 128
        kw["Ld"] = 128
        kw["eps"] = torch.zeros(B, 128, device=DEV)
        kw["mu"], kw["logvar"] = (torch.full((B, 128), -3.0, device=DEV) for _ in range(2))
        kw["z"] = torch.full((B, 128), -3.0, dtype=torch.bfloat16, device=DEV)

    def fp32(kw):
        kw["prec"] = ops.PREC_F32

    def z_pitch(kw):                # ldz not a multiple of 8
        kw["z"] = torch.full((B, 28), -3.0, dtype=torch.bfloat16, device=DEV)[:, :24]

    def z_wide(kw):                 # ldz > 32
        kw["z"] = torch.full((B, 40), -3.0, dtype=torch.bfloat16, device=DEV)[:, :24]

    def h0_lines(kw):               # H0 rows that are not whole 128-byte lines
        kw["h0"] = torch.full((B, NSTEM + 8), -3.0, dtype=torch.bfloat16, device=DEV)[:, :NSTEM]

    def y_pitch(kw):                # misaligned leading dimension of y
        e = kw["enc_a"]
        y = torch.zeros(B, KA + 4, dtype=torch.bfloat16, device=DEV)[:, :KA]
        kw["enc_a"] = e._replace(y=y)

    def mask_pitch(kw):
        e = kw["enc_b"]
        m = torch.ones(B, KB + 4, dtype=torch.uint8, device=DEV)[:, :KB]
        kw["enc_b"] = e._replace(prologue=e.prologue._replace(mask=m))

    def hidden_wide(kw):            # a hidden width outside the register plan (K = 512)
        e = kw["enc_b"]
        pl = ops.PreparedLinear([torch.randn(L, 512, generator=g).to(DEV)] * 2, [torch.zeros(L, device=DEV)] * 2, PREC, DEV)
        kw["enc_b"] = ops.LatentEncoder(torch.zeros(B, 512, dtype=torch.bfloat16, device=DEV),
                                        ops.Prologue(torch.ones(512, device=DEV), torch.zeros(512, device=DEV), None, 1.0), None, pl)

    def stem_width(kw):             # stem wider than the LDS plan
        n = 512
        kw["stem"] = ops.PreparedLinear([torch.randn(n, L, generator=g).to(DEV)], [torch.zeros(n, device=DEV)], PREC, DEV)
        kw["h0"] = torch.full((B, n), -3.0, dtype=torch.bfloat16, device=DEV)

    def table_big(kw):              # S * 2L floats beyond the table's LDS
        kw["table"] = torch.zeros(32, 2 * L, device=DEV)

    def no_modality(kw):
        kw["enc_a"] = kw["enc_b"] = kw["table"] = kw["site"] = None

    for m in (wide_latent, z_pitch, z_wide, h0_lines, y_pitch, mask_pitch, hidden_wide, stem_width, table_big, no_modality):
        _refused(c, m)
    _refused(c, fp32)
    try:
        _set_tuning(10, 0)          # the tuning key: off -> refused, the engine falls back
        _refused(c, lambda kw: None)
    finally:
        _set_tuning(10, 1)
    lib = _lib.load()
    assert lib.mmvae_set_tuning(1, 1) == -1 and lib.mmvae_set_tuning(5, 1) == -1 and lib.mmvae_set_tuning(11, 1) == -1


def test_refusals_of_the_raw_entry_point():
    """The limits that the tensor-level wrapper cannot produce (it derives these fields from the tensors): a valid LatentFwdArgs with
    ONE field changed, given to mmvae_latent_fwd itself.  Each returns MMVAE_ERR_ARG and leaves every output, the BatchNorm vectors
    and the running statistics untouched.  Not covered here: the 4 GiB limit of the row operands (y, mask, h0) -- it needs a batch
    of more than 4 M rows, i.e. tens of GB of operands."""
    import ctypes as C
    B = 512
    c = _Case(B, True, True, True, True, seed=4)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    def fin_copy(a, enc):            # a private copy of the encoder's BnFinalizeArgs that the case may change
        f = _lib.BnFinalizeArgs.from_buffer_copy(C.cast(getattr(a, enc).finalize, C.POINTER(_lib.BnFinalizeArgs)).contents)
        getattr(a, enc).finalize = C.addressof(f)
        return f

    def set_(path, value):
        def m(a):
            obj = a
            *head, last = path.split(".")
            for h in head:
                obj = getattr(obj, h)
            setattr(obj, last, value(getattr(obj, last)) if callable(value) else value)
        return m

    def fin_field(enc, field, value):
        def m(a):
            f = fin_copy(a, enc)
            setattr(f, field, value)
            return f                 # kept alive by the caller
        return m

    def one_row(a):                  # B < 2 with a finalisation (BatchNorm needs two rows)
        a.B = 1
        fa, fb = fin_copy(a, "enc_a"), fin_copy(a, "enc_b")
        fa.M = fb.M = 1
        return fa, fb

    cases = {
        "K % 32": set_("enc_a.K", 120), "K < 32": set_("enc_b.K", 16), "K > 256": set_("enc_b.K", 288),
        "ldy % 8": set_("enc_a.ldy", KA + 4), "ldy < K": set_("enc_a.ldy", KA - 8),
        "ld_mask % 8": set_("enc_b.ld_mask", KB + 4), "ld_mask < K": set_("enc_b.ld_mask", KB - 8),
        "heads ldw % 64": set_("enc_a.ldw", 160), "heads ldw < K": set_("enc_b.ldw", 128),
        "stem ldw % 64": set_("ldw_stem", 96), "stem ldw < 32": set_("ldw_stem", 0),
        "N_stem % 64": set_("N_stem", 416 + 8), "N_stem < 64": set_("N_stem", 0), "N_stem > 448": set_("N_stem", 512),
        "ldh0 % 64": set_("ldh0", NSTEM + 8), "ldh0 < N_stem": set_("ldh0", 384),
        "ldz % 8": set_("ldz", 28), "ldz < L": set_("ldz", 16), "ldz > 32": set_("ldz", 40),
        "finalize N != K": fin_field("enc_a", "N", KA - 32), "finalize M != B": fin_field("enc_b", "M", B - 1),
        "finalize without sums": fin_field("enc_a", "sum", None), "B < 2 with a finalisation": one_row,
        "y not 16-byte aligned": set_("enc_a.y", lambda p: p + 8), "mask not 8-byte aligned": set_("enc_b.mask", lambda p: p + 4),
        "z not 16-byte aligned": set_("z", lambda p: p + 8), "h0 not 128-byte aligned": set_("h0", lambda p: p + 64),
        "heads w not 16-byte aligned": set_("enc_a.w", lambda p: p + 8), "stem w not 16-byte aligned": set_("w_stem", lambda p: p + 8),
        "n_mod != modalities present": set_("n_mod", 2), "table without site": set_("site", None), "S = 0": set_("S", 0),
        "L = 0": set_("L", 0), "L > 24": set_("L", 25), "B = 0": set_("B", 0),
        "no eps": set_("eps", None), "no mu": set_("mu", None), "no logvar": set_("logvar", None), "no z": set_("z", None),
        "no h0": set_("h0", None), "no stem weights": set_("w_stem", None), "no heads weights": set_("enc_b.w", None),
        "precision": set_("prec", ops.PREC_F32),
    }
    for name, mutate in cases.items():
        o = c.outputs()
        states = [e.fresh() for e in c.enc]
        owed = [ops.LatentEncoder(e.y, s[4], s[5], e.pl) for e, s in zip(c.enc, states)]
        a, _ = ops.latent_fwd_args(PREC, B, L, owed[0], owed[1], c.table, c.site, c.eps, o["mu"], o["logvar"], o["z"], c.stem, o["h0"])
        keep = mutate(a)             # noqa: F841 -- changed copies of host structs live until the call returns
        rc = lib.mmvae_latent_fwd(C.byref(a), stream)
        assert rc == (-2 if name == "precision" else -1), (name, rc)
        torch.cuda.synchronize()
        for k, v in o.items():
            assert bool((v == -3.0).all()), (name, k)
        for e, s in zip(c.enc, states):
            assert bool((s[0].buf == -7.0).all()) and torch.equal(s[1], e.rm0) and torch.equal(s[2], e.rv0) and int(s[3]) == 3, name
    # the unchanged struct is taken
    o = c.outputs()
    states = [e.fresh() for e in c.enc]
    owed = [ops.LatentEncoder(e.y, s[4], s[5], e.pl) for e, s in zip(c.enc, states)]
    a, _ = ops.latent_fwd_args(PREC, B, L, owed[0], owed[1], c.table, c.site, c.eps, o["mu"], o["logvar"], o["z"], c.stem, o["h0"])
    assert lib.mmvae_latent_fwd(C.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert not bool((o["h0"] == -3.0).all())


# ----------------------------------------------------------------------------------------------------------------------------------
# the whole step through the engine: tuning key 10 off (today's launch sequence) against on, from the same seeded start
# ----------------------------------------------------------------------------------------------------------------------------------
A_DIM, D_DIM = 782, 572


def _batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, A_DIM, generator=g).to(DEV)
    b = (torch.rand(B, D_DIM, generator=g) < 0.3).float().to(DEV)
    site = torch.randint(0, S, (B,), generator=g).to(DEV)
    return a, b, site


def _reset_noise():
    engine.GLOBAL_NOISE.offset_tensor(torch.device(DEV, torch.cuda.current_device())).zero_()


def _one_step(B, replay, on, batch):
    from mmvae.graphs import GraphedTrainStep
    _set_tuning(10, int(on))
    try:
        torch.manual_seed(321)
        m = MultiModalVAE(A_DIM, D_DIM, S, L).to(DEV).train()
        _reset_noise()
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
        gs = GraphedTrainStep(m, opt, *batch, warmup=1, preserve_state=True)
        if replay:
            gs()
            losses = gs.losses()
        else:
            from mmvae import functional as F_
            losses = tuple(F_.read_losses(gs.run_eager()))
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        return losses, grads
    finally:
        _set_tuning(10, 1)


@pytest.mark.parametrize("replay", [True, False], ids=["replayed", "run_eager"])
@pytest.mark.parametrize("B", [4096, 65536])
def test_training_step_fused_against_unfused(B, replay):
    """One captured training step (bf16) with the fused latent launch against the same step with tuning key 10 off.  The forward is
    bit-identical, so the four loss values must be EQUAL.  The 39 gradients see the same inputs in both runs and differ only by what
    the old path differs from itself: the order of the float atomics in the dW / db / table accumulations.  That floor is measured
    here (key off, run twice from the same start: per-tensor max |difference|) and printed.  One pair of runs is ONE sample of it: a
    tensor whose accumulation is unordered can show 0 in the sample and one ulp in the next run, so the floor of a tensor is taken as
    at least the smallest difference a reordered fp32 accumulation can show, one ulp at the tensor's largest magnitude
    (2^-23 max |g|).  The fused run is allowed 4 x that floor per tensor: the floor is a sample of the maximum of a noise process whose
    samples spread by a few-fold, and nothing else may differ."""
    batch = _batch(B, 11)
    l0, g0 = _one_step(B, replay, False, batch)
    l1, g1 = _one_step(B, replay, False, batch)
    l2, g2 = _one_step(B, replay, True, batch)
    assert len(g0) == 39
    assert l2 == l0 == l1, (l0, l1, l2)
    worst = (0.0, 0.0, 0.0, None)
    raw_max = (0.0, None)
    for k in g0:
        scale = float(g0[k].abs().max())
        raw = float((g0[k] - g1[k]).abs().max())            # the measured floor: old path against old path
        floor = max(raw, scale * 2.0 ** -23)
        diff = float((g2[k] - g0[k]).abs().max())
        if diff >= worst[0]:
            worst = (diff, raw, floor, k)
        if raw > raw_max[0]:
            raw_max = (raw, k)
        assert diff <= 4.0 * floor, (k, diff, raw, floor, scale)
    print(f"\n[latent fused step B={B} {'replay' if replay else 'eager'}] losses equal; largest measured old-path floor {raw_max[0]:.3e} "
          f"({raw_max[1]}); worst fused-against-old gradient difference {worst[0]:.3e} in {worst[3]} (measured floor of that tensor "
          f"{worst[1]:.3e}, with the one-ulp minimum {worst[2]:.3e}, allowed 4 x that)")


@pytest.mark.parametrize("with_site", [True, False], ids=["site", "nosite"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_model_forward_fused_against_unfused(train, with_site):
    """MultiModalVAE forward (training mode: mu / logvar and the BatchNorm buffers; eval mode with and without site): key off == on."""
    B = 4096
    a, b, site = _batch(B, 12)
    outs = []
    for on in (0, 1):
        _set_tuning(10, on)
        try:
            torch.manual_seed(77)
            m = MultiModalVAE(A_DIM, D_DIM, S, L).to(DEV)
            m.train() if train else m.eval()
            _reset_noise()
            with torch.no_grad():
                res = m(a=a, b=b, site=site if with_site else None)
            torch.cuda.synchronize()
            outs.append(([t.clone() for t in res], {k: v.clone() for k, v in m.state_dict().items()}))
        finally:
            _set_tuning(10, 1)
    for t0, t1 in zip(outs[0][0], outs[1][0]):
        assert torch.equal(t0, t1)
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k
