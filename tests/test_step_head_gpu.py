"""The merged head-of-step launch (mmvae_step_head, csrc/elementwise.hip) against the four stand-alone calls it replaces --
mmvae_embed_table_fwd, the memset, mmvae_prep_weights, mmvae_noise -- from the same starting state, bit for bit (torch.equal on
every destination, guard bytes included): every role runs the device code of its stand-alone kernel, so nothing may differ.

  noise   B = 37, widths (24, 9): 16-byte aligned segments whose total, 1229 bytes, ends inside a 16-byte quad; 37 x 5 = 185
          normals (not a multiple of 4); all MMVAE_CTR_COPIES counter copies advanced by what was consumed; two calls in a row.
  prep    plain 70 x 33 -> bf16 128 x 64, transposed 33 x 70 -> bf16 128 x 128, an fp32 destination, two sources concatenated
          into one destination (the fc_mu | fc_logvar form).
  zero    16 bytes, and 1 MiB + 16 bytes (more than one grid-stride trip), pre-filled with 0xFF between 64 guard bytes.
  table   (S, E, L) = (24, 32, 20) and (5, 7, 3).
  roles   each role empty in turn; all empty, a misaligned range and tuning key 13 off are refused with nothing written.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvae import _lib as L  # noqa: E402

DEV = "cuda"
GUARD = 64
B, WIDTHS, LD = 37, (24, 9), 5
N_MASK = 896 + 37 * 9                 # 37 x 24 = 888 -> the second segment starts at 896; 896 + 333 = 1229
N_EPS = B * LD
CONSUMED = (N_MASK + 15) // 16 * 4 + (N_EPS + 3) // 4
CTR_OLD = 0x1_0000_0F00               # above 2^32: the high counter word is carried along
SEED = 0xDEADBEEF12345678
ZERO_BYTES = (16, (1 << 20) + 16)
ROLES = ("table", "zero", "prep", "noise")
FILL = -777.0                         # what float destinations hold before a launch (not NaN: torch.equal must see equal guards)


def _check(status, what):
    L.check(status, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen).to(DEV)


class State:
    """Operands and guarded destinations of all four roles; two States of the same (seed, S, E, L) start out identical."""

    def __init__(self, S, E, Lt, seed=3):
        gen = torch.Generator().manual_seed(seed)
        # noise: the mask buffer is the engine's (segments at 16-byte multiples), handed over with its exact byte count
        self.mask = torch.full((GUARD + (N_MASK + 15) // 16 * 16 + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.eps = torch.full((16 + N_EPS + 16,), FILL, device=DEV)
        self.ctr = torch.full((L.CTR_COPIES,), CTR_OLD, dtype=torch.int64, device=DEV)
        # prep: sources, destinations pre-filled with a pattern, the item table on the device
        self.w_plain, self.w_tr, self.bias = _rand(gen, 70, 33), _rand(gen, 33, 70), _rand(gen, 1, 40)
        self.w_mu, self.w_lv = _rand(gen, 20, 33), _rand(gen, 20, 33)
        self.d_plain = torch.full((128, 64), 7.0, dtype=torch.bfloat16, device=DEV)
        self.d_tr = torch.full((128, 128), 7.0, dtype=torch.bfloat16, device=DEV)
        self.d_bias = torch.full((1, 40), 7.0, device=DEV)
        self.d_cat = torch.full((128, 64), 7.0, dtype=torch.bfloat16, device=DEV)
        items = [L.PrepItem(self.w_plain.data_ptr(), self.d_plain.data_ptr(), 70, 33, 33, 128, 64, 64, 0, L.BF16),
                 L.PrepItem(self.w_tr.data_ptr(), self.d_tr.data_ptr(), 33, 70, 70, 128, 128, 128, 1, L.BF16),
                 L.PrepItem(self.bias.data_ptr(), self.d_bias.data_ptr(), 1, 40, 40, 1, 40, 40, 0, L.F32),
                 L.PrepItem(self.w_mu.data_ptr(), self.d_cat.data_ptr(), 20, 33, 33, 20, 64, 64, 0, L.BF16),
                 L.PrepItem(self.w_lv.data_ptr(), self.d_cat.data_ptr() + 20 * 64 * 2, 20, 33, 33, 108, 64, 64, 0, L.BF16)]
        self.n_items = len(items)
        self.items = torch.frombuffer(bytearray(bytes((L.PrepItem * len(items))(*items))), dtype=torch.uint8).to(DEV)
        # zero: ranges between guards, everything 0xFF
        self.zbufs = [torch.full((GUARD + n + GUARD,), 0xFF, dtype=torch.uint8, device=DEV) for n in ZERO_BYTES]
        # table
        self.S, self.E, self.Lt = S, E, Lt
        self.emb, self.t_wmu, self.t_bmu = _rand(gen, S, E), _rand(gen, Lt, E), _rand(gen, Lt)
        self.t_wlv, self.t_blv = _rand(gen, Lt, E), _rand(gen, Lt)
        self.table = torch.full((S * 2 * Lt + 16,), FILL, device=DEV)

    def outputs(self):
        return dict(mask=self.mask, eps=self.eps, ctr=self.ctr, d_plain=self.d_plain, d_tr=self.d_tr, d_bias=self.d_bias, d_cat=self.d_cat,
                    zero0=self.zbufs[0], zero1=self.zbufs[1], table=self.table)

    # ---- the stand-alone launches -------------------------------------------------------------------------------
    def alone(self, roles=ROLES):
        lib = L.load()
        if "table" in roles:
            _check(lib.mmvae_embed_table_fwd(self.S, self.E, self.Lt, self.emb.data_ptr(), self.t_wmu.data_ptr(), self.t_bmu.data_ptr(),
                                             self.t_wlv.data_ptr(), self.t_blv.data_ptr(), self.table.data_ptr(), _stream()), "embed_table_fwd")
        if "zero" in roles:
            for z, n in zip(self.zbufs, ZERO_BYTES):
                z[GUARD:GUARD + n].zero_()
        if "prep" in roles:
            _check(lib.mmvae_prep_weights(self.items.data_ptr(), self.n_items, _stream()), "prep_weights")
        if "noise" in roles:
            _check(lib.mmvae_noise(self.mask.data_ptr() + GUARD, N_MASK, 0.9, self.eps.data_ptr() + 64, N_EPS, SEED, 11, self.ctr.data_ptr(), 1,
                                   _stream()), "noise")
        torch.cuda.synchronize()

    # ---- the merged launch --------------------------------------------------------------------------------------
    def head_args(self, roles=ROLES, zero_shift=0):
        a = L.StepHeadArgs()
        if "table" in roles:
            a.S, a.E, a.L = self.S, self.E, self.Lt
            a.emb, a.w_mu, a.b_mu, a.w_lv, a.b_lv, a.table = (t.data_ptr() for t in (self.emb, self.t_wmu, self.t_bmu, self.t_wlv, self.t_blv, self.table))
        if "zero" in roles:
            a.n_zero = len(ZERO_BYTES)
            for k, (z, n) in enumerate(zip(self.zbufs, ZERO_BYTES)):
                a.zero_ptr[k], a.zero_bytes[k] = z.data_ptr() + GUARD + zero_shift, n
        if "prep" in roles:
            a.prep_items, a.n_prep = self.items.data_ptr(), self.n_items
        if "noise" in roles:
            a.mask, a.n_mask, a.eps, a.n_eps = self.mask.data_ptr() + GUARD, N_MASK, self.eps.data_ptr() + 64, N_EPS
            a.keep_prob, a.seed, a.offset, a.offset_dev, a.advance = 0.9, SEED, 11, self.ctr.data_ptr(), 1
        return a

    def head(self, roles=ROLES, **kw):
        status = L.load().mmvae_step_head(C.byref(self.head_args(roles, **kw)), _stream())
        torch.cuda.synchronize()
        return status


def _same(a, b):
    oa, ob = a.outputs(), b.outputs()
    for name in oa:
        assert torch.equal(oa[name], ob[name]), name


def _assert_written(st):
    """The roles did something: what the comparison holds equal is not two untouched buffers."""
    assert (st.ctr == CTR_OLD + CONSUMED).all()
    assert (st.eps[16:16 + N_EPS].abs() < 10).all() and (st.eps[:16] == FILL).all() and (st.eps[16 + N_EPS:] == FILL).all()
    m = st.mask[GUARD:GUARD + N_MASK]
    assert (m <= 1).all() and 0.8 < m.float().mean().item() < 0.97
    assert (st.mask[:GUARD] == 0xA5).all() and (st.mask[GUARD + N_MASK:] == 0xA5).all()          # bytes 1229 .. 1231 of the last quad too
    for z, n in zip(st.zbufs, ZERO_BYTES):
        assert not z[GUARD:GUARD + n].any() and (z[:GUARD] == 0xFF).all() and (z[GUARD + n:] == 0xFF).all()
    assert torch.equal(st.d_plain[:70, :33], st.w_plain.bfloat16()) and not st.d_plain[70:].any() and not st.d_plain[:, 33:].any()
    assert torch.equal(st.d_tr[:70, :33], st.w_tr.t().bfloat16()) and not st.d_tr[70:].any() and not st.d_tr[:, 33:].any()
    assert torch.equal(st.d_bias, st.bias)
    assert torch.equal(st.d_cat[:20, :33], st.w_mu.bfloat16()) and torch.equal(st.d_cat[20:40, :33], st.w_lv.bfloat16()) and not st.d_cat[40:].any()
    n = st.S * 2 * st.Lt
    assert (st.table[:n] != FILL).all() and (st.table[n:] == FILL).all()


@pytest.mark.parametrize("S,E,Lt", [(24, 32, 20), (5, 7, 3)])
def test_head_equals_the_four_launches(S, E, Lt):
    ref, got = State(S, E, Lt), State(S, E, Lt)
    _same(ref, got)
    ref.alone()
    assert got.head() == 0
    _assert_written(ref)
    _same(ref, got)
    # the table against its definition (the comparison above only says both forms agree)
    emb, wcat = ref.emb.double(), torch.cat([ref.t_wmu, ref.t_wlv]).double()
    bcat = torch.cat([ref.t_bmu, ref.t_blv]).double()
    want = emb @ wcat.t() + bcat
    # E products and E additions in fp32, each within 2^-24 relative of its exact value: (E + 1) 2^-23 of the sum of magnitudes
    bound = (E + 1) * 2.0 ** -23 * (emb.abs() @ wcat.abs().t() + bcat.abs())
    err = (ref.table[:S * 2 * Lt].view(S, 2 * Lt).double() - want).abs()
    print(f"table ({S}, {E}, {Lt}): max err / bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


def test_two_calls_in_a_row_follow_the_counter():
    ref, got = State(24, 32, 20), State(24, 32, 20)
    for _ in range(2):
        first = got.mask.clone()
        ref.alone()
        assert got.head() == 0
    _same(ref, got)
    assert (got.ctr == CTR_OLD + 2 * CONSUMED).all()
    assert not torch.equal(first, got.mask)              # the second call drew from the advanced offset


@pytest.mark.parametrize("empty", ROLES)
def test_each_role_may_be_empty(empty):
    roles = tuple(r for r in ROLES if r != empty)
    ref, got, untouched = State(24, 32, 20), State(24, 32, 20), State(24, 32, 20)
    ref.alone(roles)
    assert got.head(roles) == 0
    _same(ref, got)
    mine = {"table": ["table"], "zero": ["zero0", "zero1"], "prep": ["d_plain", "d_tr", "d_bias", "d_cat"], "noise": ["mask", "eps", "ctr"]}
    for name in mine[empty]:
        assert torch.equal(got.outputs()[name], untouched.outputs()[name]), name
    for role in roles:
        for name in mine[role]:
            assert not torch.equal(got.outputs()[name], untouched.outputs()[name]), name


def test_refusals_write_nothing():
    got, untouched = State(24, 32, 20), State(24, 32, 20)
    assert got.head(()) == -1                                            # every role empty
    assert got.head(zero_shift=8) == -1                                  # a range that is not 16-byte aligned
    a = got.head_args()
    a.zero_bytes[1] = ZERO_BYTES[1] - 8                                  # ... or not a whole number of 16-byte vectors
    assert L.load().mmvae_step_head(C.byref(a), _stream()) == -1
    a = got.head_args()
    a.mask = a.mask + 4                                                  # the noise role's own refusal (mmvae_noise: mask 16-byte aligned)
    assert L.load().mmvae_step_head(C.byref(a), _stream()) == -1
    try:
        assert L.load().mmvae_set_tuning(13, 0) == 0
        assert got.head() == -1
    finally:
        assert L.load().mmvae_set_tuning(13, 1) == 0
    torch.cuda.synchronize()
    _same(got, untouched)
    assert got.head() == 0                                               # the key is back on
    _assert_written(got)
