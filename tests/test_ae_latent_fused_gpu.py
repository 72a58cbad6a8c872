"""mmvae_ae_latent_fwd (the encoder's head + plain mean + the decoder's first layer in ONE launch) against the three entry points it
replaces -- mmvae_gemm_nt (the head, BatchNorm finalisation folded in), mmvae_fuse_mean_fwd and mmvae_gemm_nt (the decoder's layer 0) --
on the same inputs, modelled on tests/test_latent_fused_gpu.py.  The target is bit identity: latent, z with its pads, h0, the BatchNorm
tables and the running statistics are torch.equal (NaN rows: NaNs in the same places).

B in {1, 16, 17, 1000} (1000 = 62 slabs + 8 rows; B = 1 only in eval mode: BatchNorm needs two rows), K in {128, 256}, N_stem in
{128, 256}, L in {7, 20, 24}, with and without table, with and without encoder, training (finalize + mask) and eval (scale / shift).
One case at B = 40 000: 2 500 slabs against 256 x 8 waves, so some waves carry a second slab through the prefetch path.  Refused
calls leave guarded outputs untouched.  No call hands the library a pointer or size that could make the kernel touch memory outside
its buffers: refusals use only arguments the entry point rejects before it launches."""
import ctypes as C

import pytest
import torch

from mmvae import _lib, engine, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 24
PREC = ops.PREC_BF16
KEY = 15


def _set_tuning(key, value):
    _lib.check(_lib.load().mmvae_set_tuning(key, value), "mmvae_set_tuning")


class _Case:
    def __init__(self, B, K, N, L, has_enc, has_table, train, seed=0, bad_label=None):
        g = torch.Generator().manual_seed(1000 * seed + B + K + N + L)
        self.B, self.K, self.N, self.L, self.train, self.has_enc = B, K, N, L, train, has_enc
        if has_enc:
            self.y = (torch.randn(B, K, generator=g) * 1.5 + 0.3).to(torch.bfloat16).to(DEV)
            yd = self.y.double()
            self.stats = torch.stack([yd.sum(0), (yd * yd).sum(0)]).contiguous()
            self.gamma = (torch.rand(K, generator=g) + 0.5).to(DEV)
            self.beta = (torch.randn(K, generator=g) * 0.2).to(DEV)
            self.mask = (torch.rand(B, K, generator=g) < 0.9).to(torch.uint8).to(DEV) if train else None
            self.rm0 = (torch.randn(K, generator=g) * 0.1).to(DEV)
            self.rv0 = (torch.rand(K, generator=g) + 0.5).to(DEV)
            self.pl = ops.PreparedLinear([torch.randn(L, K, generator=g).to(DEV) / K ** 0.5], [torch.randn(L, generator=g).to(DEV) * 0.1], PREC, DEV)
        self.table = (torch.randn(S, L, generator=g) * 0.5).to(DEV) if has_table else None
        self.site = torch.randint(0, S, (B,), generator=g).to(DEV) if has_table else None
        if bad_label is not None:
            self.site[bad_label[0]] = bad_label[1]
        self.first = ops.PreparedLinear([torch.randn(N, L, generator=g).to(DEV) / L ** 0.5], [torch.randn(N, generator=g).to(DEV) * 0.1], PREC, DEV)
        ops.WeightPrep(([self.pl] if has_enc else []) + [self.first], DEV).run()

    def fresh(self):
        """BatchNorm state of one run: (BNState, running_mean, running_var, num_batches_tracked, Prologue, BnFinalizeArgs or None)."""
        st = engine.BNState(self.K, DEV)
        st.buf.fill_(-7.0)
        rm, rv, nbt = self.rm0.clone(), self.rv0.clone(), torch.full((), 3, dtype=torch.int64, device=DEV)
        if self.train:
            fin = ops.bn_finalize_args(self.B, self.K, self.stats, self.gamma, self.beta, rm, rv, nbt, st.mean, st.rstd, st.scale, st.shift)
            pro = ops.Prologue(st.scale, st.shift, self.mask, 1.0 / 0.9)
        else:
            fin = None
            ops.bn_eval_coeffs(self.gamma, self.beta, rm, rv, st.scale, st.shift, 1e-5, st.mean, st.rstd)
            pro = ops.Prologue(st.scale, st.shift, None, 1.0)
        return st, rm, rv, nbt, pro, fin

    def outputs(self):
        mk = lambda *shape, dt: torch.full(shape, -3.0, dtype=dt, device=DEV)          # a sentinel: every element must be written
        return dict(latent=mk(self.B, self.L, dt=torch.float32), z=mk(self.B, ops.ceil_to(self.L, 8), dt=torch.bfloat16),
                    h0=mk(self.B, self.N, dt=torch.bfloat16))

    def run(self, fused):
        B, L = self.B, self.L
        o = self.outputs()
        s = self.fresh() if self.has_enc else None
        if fused:
            owed = ops.LatentEncoder(self.y, s[4], s[5], self.pl) if self.has_enc else None
            ops.ae_latent_fwd(PREC, B, L, owed, self.table, self.site, o["latent"], o["z"], self.first, o["h0"])
        else:
            head = None
            if self.has_enc:
                head = torch.empty(B, L, dtype=torch.float32, device=DEV)
                try:
                    ops.gemm_nt(PREC, self.y, self.pl.w, L, self.K, head, bias=self.pl.bias, prologue=s[4], pro_finalize=s[5])
                except _lib.MMVAEArgError:               # the folded finalisation is not taken for this shape: its own launch, as the engine does
                    ops.bn_finalize_launch(s[5])
                    ops.gemm_nt(PREC, self.y, self.pl.w, L, self.K, head, bias=self.pl.bias, prologue=s[4])
            ops.fuse_mean_fwd(B, L, head, self.table, self.site, o["latent"], o["z"])
            ops.gemm_nt(PREC, o["z"], self.first.w, self.N, L, o["h0"], bias=self.first.bias, act=ops.ACT_RELU)
        torch.cuda.synchronize()
        if s is not None:
            o.update(bn=s[0].buf, rm=s[1], rv=s[2], nbt=s[3])
        return o, s


def _same(a, b):
    if a.dtype.is_floating_point:
        na, nb = torch.isnan(a), torch.isnan(b)
        return bool(torch.equal(na, nb)) and bool(torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b)))
    return bool(torch.equal(a, b))


def _check(c):
    (want, _), (got, _) = c.run(False), c.run(True)
    assert set(want) == set(got)
    for k in want:
        assert torch.equal(want[k], got[k]), (k, int((want[k] != got[k]).sum()), want[k].numel())
    assert not bool((got["z"][:, c.L:] != 0).any())
    if c.train and c.has_enc:
        assert int(got["nbt"]) == 4 and not bool((got["bn"] == -7.0).any())


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("has_enc,has_table", [(True, True), (True, False), (False, True)], ids=["enc+site", "enc", "site"])
@pytest.mark.parametrize("K,N", [(128, 256), (256, 128)])
@pytest.mark.parametrize("L", [7, 20, 24])
def test_fused_forward_is_bit_identical(L, K, N, has_enc, has_table, train):
    for B in (1, 16, 17, 1000):
        if B == 1 and train and has_enc:
            continue                                     # BatchNorm's finalisation needs two rows (refused: see the refusals)
        _check(_Case(B, K, N, L, has_enc, has_table, train))


def test_second_slab_through_the_prefetch_path():
    """B = 40 000: 2 500 slabs against at most 256 workgroups x 8 waves, so some waves fetch a second slab under their first."""
    _check(_Case(40000, 256, 128, 20, True, True, True, seed=5))


@pytest.mark.parametrize("label", [-1, S, 2 ** 40])
def test_out_of_range_label_poisons_its_own_row_only(label):
    B, row, L = 333, 100, 20
    c = _Case(B, 128, 256, L, True, True, True, seed=2, bad_label=(row, label))
    (want, _), (got, _) = c.run(False), c.run(True)
    for k in want:
        assert _same(want[k], got[k]), k
    assert bool(torch.isnan(got["latent"][row]).all()) and bool(torch.isnan(got["z"][row, :L].float()).all())
    others = torch.arange(B, device=DEV) != row
    for k in ("latent", "z", "h0"):
        assert not bool(torch.isnan(got[k][others].float()).any()), k


def test_refusals_leave_everything_untouched():
    """A valid AELatentFwdArgs with ONE field changed, given to mmvae_ae_latent_fwd itself: MMVAE_ERR_ARG (fp32: MMVAE_ERR_DTYPE), and
    every output, the BatchNorm vectors and the running statistics are as they were."""
    B, K, N, L = 512, 256, 128, 20
    c = _Case(B, K, N, L, True, True, True, seed=4)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    def set_(path, value):
        def m(a):
            obj = a
            *head, last = path.split(".")
            for h in head:
                obj = getattr(obj, h)
            setattr(obj, last, value(getattr(obj, last)) if callable(value) else value)
        return m

    def fin_field(field, value):
        def m(a):
            f = _lib.BnFinalizeArgs.from_buffer_copy(C.cast(a.enc.finalize, C.POINTER(_lib.BnFinalizeArgs)).contents)
            a.enc.finalize = C.addressof(f)
            setattr(f, field, value)
            return f
        return m

    def one_row(a):
        a.B = 1
        return fin_field("M", 1)(a)

    cases = {
        "L = 25": set_("L", 25), "L = 0": set_("L", 0), "B = 0": set_("B", 0), "K = 288": set_("enc.K", 288), "K % 32": set_("enc.K", 120),
        "K < 32": set_("enc.K", 16), "N_stem = 100": set_("N_stem", 100), "N_stem > 448": set_("N_stem", 512), "N_stem < 64": set_("N_stem", 0),
        "ldy % 8": set_("enc.ldy", K + 4), "ld_mask % 8": set_("enc.ld_mask", K + 4), "head ldw % 64": set_("enc.ldw", 288),
        "stem ldw % 64": set_("ldw_stem", 96), "ldh0 % 64": set_("ldh0", N + 8), "ldh0 < N_stem": set_("ldh0", 64),
        "ldz % 8": set_("ldz", 28), "ldz < L": set_("ldz", 16), "ldz > 32": set_("ldz", 40),
        "z not 16-byte aligned": set_("z", lambda p: p + 8), "h0 not 128-byte aligned": set_("h0", lambda p: p + 64),
        "y not 16-byte aligned": set_("enc.y", lambda p: p + 8), "n_mod != modalities present": set_("n_mod", 1),
        "table without site": set_("site", None), "S = 0": set_("S", 0), "S * L > 1024": set_("S", 52),
        "finalize N != K": fin_field("N", K - 32), "finalize M != B": fin_field("M", B - 1), "B < 2 with a finalisation": one_row,
        "no latent": set_("latent", None), "no z": set_("z", None), "no h0": set_("h0", None), "no first-layer weights": set_("w_stem", None),
        "no head weights": set_("enc.w", None), "precision": set_("prec", ops.PREC_F32),
    }

    def attempt(name, mutate, want_rc):
        o = c.outputs()
        s = c.fresh()
        a, _ = ops.ae_latent_fwd_args(PREC, B, L, ops.LatentEncoder(c.y, s[4], s[5], c.pl), c.table, c.site, o["latent"], o["z"], c.first, o["h0"])
        keep = mutate(a)             # noqa: F841 -- changed copies of host structs live until the call returns
        rc = lib.mmvae_ae_latent_fwd(C.byref(a), stream)
        assert rc == want_rc, (name, rc)
        torch.cuda.synchronize()
        return o, s

    for name, mutate in cases.items():
        o, s = attempt(name, mutate, -2 if name == "precision" else -1)
        for k, v in o.items():
            assert bool((v == -3.0).all()), (name, k)
        assert bool((s[0].buf == -7.0).all()) and torch.equal(s[1], c.rm0) and torch.equal(s[2], c.rv0) and int(s[3]) == 3, name
    try:
        _set_tuning(KEY, 0)          # the tuning key: off -> refused, the engine issues the three launches
        o, s = attempt("key off", lambda a: None, -1)
        assert all(bool((v == -3.0).all()) for v in o.values()) and bool((s[0].buf == -7.0).all())
    finally:
        _set_tuning(KEY, 1)
    o, s = attempt("unchanged", lambda a: None, 0)       # the unchanged struct is taken
    assert not bool((o["h0"] == -3.0).all()) and int(s[3]) == 4
    assert lib.mmvae_set_tuning(11, 1) == -1 and lib.mmvae_set_tuning(16, 1) == -1


@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_model_forward_fused_against_unfused(kind, train):
    """RNA2DNAAE / DNA2RNAAE forward with key 15 off == on: reconstruction, latent and the BatchNorm buffers, bit for bit."""
    from src.models import RNA2DNAAE, DNA2RNAAE
    B, A, D, L = 1000, 782, 572, 20
    g = torch.Generator().manual_seed(12)
    a, b, site = torch.randn(B, A, generator=g).to(DEV), torch.rand(B, D, generator=g).to(DEV), torch.randint(0, S, (B,), generator=g).to(DEV)
    outs = []
    for on in (0, 1):
        _set_tuning(KEY, on)
        try:
            torch.manual_seed(77)
            m = (RNA2DNAAE if kind == "rna2dna" else DNA2RNAAE)(A, D, S, L).to(DEV)
            m.train() if train else m.eval()
            engine.GLOBAL_NOISE.offset_tensor(torch.device(DEV, torch.cuda.current_device())).zero_()
            with torch.no_grad():
                res = m(rna=a, site=site) if kind == "rna2dna" else m(dna=b, site=site)
            torch.cuda.synchronize()
            outs.append(([t.clone() for t in res], {k: v.clone() for k, v in m.state_dict().items()}))
        finally:
            _set_tuning(KEY, 1)
    for t0, t1 in zip(outs[0][0], outs[1][0]):
        assert torch.equal(t0, t1)
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k
