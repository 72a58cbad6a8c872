"""The device noise stream (mmvae_noise, csrc/elementwise.hip) against its numpy restatement (oracle/np_noise.py, pinned by
tests/test_noise_ref_cpu.py): checkpoint / resume, the two-rank stream and bench_expect.json all rest on this stream being what
include/mmvae_hip.h says it is.

  masks     bit for bit, every byte, plus guard bytes behind the buffer.
  normals   every element within eps_tolerance(radius) of the float64 reference: 4 x the float32 noise of the Box-Muller formula
            as measured on the CPU (tests/test_noise_ref_cpu.py).  A wrong counter, tag or eps base is off by O(1).
  counters  every one of the MMVAE_CTR_COPIES copies after a self-advancing launch, for a one-block grid and at the grid cap.
  refusals  MMVAE_ERR_ARG with the outputs untouched; only arguments the entry point rejects before it launches anything.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import np_noise as N  # noqa: E402
from mmvae import _lib as L  # noqa: E402
from mmvae import engine, ops  # noqa: E402
from test_noise_ref_cpu import eps_tolerance  # noqa: E402

DEV = "cuda"
GUARD = 64
SEED_HI = 0xDEADBEEF12345678          # high 32 bits set: the second key word
OFF_CARRY = 2 ** 32 - 2               # the low counter word carries into the second one inside the call
GRID_CAP_QUADS = 2048 * 256           # quads of a launch that just fills the 2048-block grid


def _i64(v):
    """uint64 value -> the int64 with the same bits (torch has no uint64 arithmetic)."""
    v &= 2 ** 64 - 1
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _draw(n_mask, n_eps, keep, seed, offset, offset_dev=None, advance=False, eps_shift=0):
    """One launch into guarded buffers -> (mask uint8[n_mask] or None, eps float64[n_eps] or None), both as numpy."""
    mbuf = torch.full((n_mask + GUARD,), 0xAB, dtype=torch.uint8, device=DEV) if n_mask else None
    ebuf = torch.full((eps_shift + n_eps + GUARD,), float("nan"), device=DEV) if n_eps else None
    mask = mbuf[:n_mask] if n_mask else None
    eps = ebuf[eps_shift:eps_shift + n_eps] if n_eps else None
    used = ops.noise(mask, eps, keep, seed, offset, offset_dev, advance)
    torch.cuda.synchronize()
    assert used == N.consumed(n_mask, n_eps)
    if n_mask:
        assert (mbuf[n_mask:] == 0xAB).all(), "bytes behind the mask were written"
    if n_eps:
        assert torch.isnan(ebuf[:eps_shift]).all() and torch.isnan(ebuf[eps_shift + n_eps:]).all(), "floats outside eps were written"
    return (mask.cpu().numpy() if n_mask else None), (eps.double().cpu().numpy() if n_eps else None)


def _check_eps(got, n, seed, offset):
    ref, rad = N.normals(n, seed, offset, with_radius=True)
    err = np.abs(got - ref)
    tol = eps_tolerance(rad)
    print(f"eps n={n}: max |z - ref| = {err.max():.3e}, max err / tol = {(err[tol > 0] / tol[tol > 0]).max() if (tol > 0).any() else 0:.3f}")
    assert np.isfinite(got).all()
    assert (err <= tol).all(), f"{int((err > tol).sum())} of {n} normals outside the bound; worst {err.max():.3e}"


# ---------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [0.9, 0.5, 0.0, 1.0])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096 + 5])
def test_mask_bits(n, keep):
    got, _ = _draw(n, 0, keep, 1234, 0)
    np.testing.assert_array_equal(got, N.mask_bytes(n, keep, 1234, 0))


def test_mask_bits_large_draw_loops_the_grid():
    n = (16 << 20) + 5                      # 2^20 + 1 quads on 2048 x 256 threads: every thread takes two or three
    got, _ = _draw(n, 0, 0.9, 1234, 0)
    np.testing.assert_array_equal(got, N.mask_bytes(n, 0.9, 1234, 0))


@pytest.mark.parametrize("n", [17, 4096 + 5])
def test_mask_bits_seed_high_word_and_counter_carry(n):
    got, _ = _draw(n, 0, 0.9, SEED_HI, OFF_CARRY)
    np.testing.assert_array_equal(got, N.mask_bytes(n, 0.9, SEED_HI, OFF_CARRY))
    assert not np.array_equal(got, N.mask_bytes(n, 0.9, SEED_HI & 0xFFFFFFFF, OFF_CARRY))      # the high key word matters


def test_offset_by_value_plus_device_offset():
    dev_off = torch.tensor([5_000_000_011], dtype=torch.int64, device=DEV)
    gm, ge = _draw(4096 + 5, 7, 0.5, 99, 1000, offset_dev=dev_off)
    start = 1000 + 5_000_000_011
    np.testing.assert_array_equal(gm, N.mask_bytes(4096 + 5, 0.5, 99, start))
    _check_eps(ge, 7, 99, N.eps_base(start, 4096 + 5))
    assert dev_off.item() == 5_000_000_011          # advance = 0: the counter is read, not written


# ---------------------------------------------------------------------------------------------
# normals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, (1 << 20) + 3])
def test_eps_against_float64(n):
    _, got = _draw(0, n, 1.0, 7, 0)
    _check_eps(got, n, 7, 0)


@pytest.mark.parametrize("n", [1, 5, 4096 + 3])
def test_eps_unaligned_output_takes_the_scalar_path(n):
    _, got = _draw(0, n, 1.0, SEED_HI, OFF_CARRY, eps_shift=1)       # pointer 4 bytes past a 16-byte boundary
    _check_eps(got, n, SEED_HI, OFF_CARRY)


@pytest.mark.parametrize("n_mask,n_eps", [(1, 1), (17, 5), (4096 + 5, 1027), (77 * 896, 77 * 20)])
def test_combined_call_pins_the_eps_base(n_mask, n_eps):
    gm, ge = _draw(n_mask, n_eps, 0.9, SEED_HI, OFF_CARRY)
    np.testing.assert_array_equal(gm, N.mask_bytes(n_mask, 0.9, SEED_HI, OFF_CARRY))
    _check_eps(ge, n_eps, SEED_HI, N.eps_base(OFF_CARRY, n_mask))


# ---------------------------------------------------------------------------------------------
# refusals: nothing may be enqueued
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    mbuf = torch.full((256,), 0xAB, dtype=torch.uint8, device=DEV)
    ebuf = torch.full((64,), 3.0, device=DEV)
    ctr = torch.full((L.CTR_COPIES,), 17, dtype=torch.int64, device=DEV)
    m, e, c = mbuf.data_ptr(), ebuf.data_ptr(), ctr.data_ptr()
    assert m % 16 == 0
    calls = {
        "mask not 16-byte aligned": (m + 1, 64, 0.9, e, 16, 1, 0, None, 0),
        "keep < 0": (m, 64, -0.1, e, 16, 1, 0, None, 0),
        "keep > 1": (m, 64, 1.5, e, 16, 1, 0, c, 1),
        "advance without offset_dev": (m, 64, 0.9, e, 16, 1, 0, None, 1),
        "nothing to draw": (m, 0, 0.9, e, 0, 1, 0, c, 1),
        "negative count": (m, -16, 0.9, e, 16, 1, 0, c, 1),
    }
    for what, args in calls.items():
        assert lib.mmvae_noise(*args, st) == -1, what
    torch.cuda.synchronize()
    assert (mbuf == 0xAB).all() and (ebuf == 3.0).all() and (ctr == 17).all()
    with pytest.raises(L.MMVAEArgError):
        ops.noise(mbuf[1:65], None, 0.9, 1, 0)


# ---------------------------------------------------------------------------------------------
# self-advancing counters
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mask,n_eps", [(16, 4), (GRID_CAP_QUADS * 16 - 64, 16)], ids=["one_block", "grid_cap"])
def test_every_counter_copy_advances(n_mask, n_eps):
    assert (n_mask + 15) // 16 + (n_eps + 3) // 4 in (2, GRID_CAP_QUADS)       # 1 block / exactly 2048 blocks
    c0 = 3 * 2 ** 32 - 9                    # the copies carry past a 32-bit boundary
    ctr = torch.full((L.CTR_COPIES,), c0, dtype=torch.int64, device=DEV)
    gm, ge = _draw(n_mask, n_eps, 0.9, 42, 0, offset_dev=ctr, advance=True)
    want = c0 + N.consumed(n_mask, n_eps)
    got = ctr.cpu().numpy()
    assert (got == want).all(), f"{int((got != want).sum())} of {L.CTR_COPIES} copies differ from {want}: {np.unique(got)[:8]}"
    np.testing.assert_array_equal(gm, N.mask_bytes(n_mask, 0.9, 42, c0))        # every block read the old value
    _check_eps(ge, n_eps, 42, N.eps_base(c0, n_mask))


def test_consecutive_advancing_calls_continue_the_stream():
    c0 = 1_000_003
    ctr = torch.full((L.CTR_COPIES,), c0, dtype=torch.int64, device=DEV)
    n_mask, n_eps = 4096 + 5, 1027
    gm1, ge1 = _draw(n_mask, n_eps, 0.9, 42, 0, offset_dev=ctr, advance=True)
    gm2, ge2 = _draw(n_mask, n_eps, 0.9, 42, 0, offset_dev=ctr, advance=True)
    c1 = c0 + N.consumed(n_mask, n_eps)
    np.testing.assert_array_equal(gm1, N.mask_bytes(n_mask, 0.9, 42, c0))
    np.testing.assert_array_equal(gm2, N.mask_bytes(n_mask, 0.9, 42, c1))
    _check_eps(ge1, n_eps, 42, N.eps_base(c0, n_mask))
    _check_eps(ge2, n_eps, 42, N.eps_base(c1, n_mask))
    assert (ctr == c0 + 2 * N.consumed(n_mask, n_eps)).all()


def test_counter_add_on_a_single_word():
    words = torch.tensor([5, 2 ** 32 - 1, 7], dtype=torch.int64, device=DEV)
    ops.counter_add(words[1:2], 2 ** 33 + 3)
    ops.counter_add(words[1:2], 1)
    assert words.tolist() == [5, 2 ** 32 - 1 + 2 ** 33 + 4, 7]
    wrap = torch.tensor([-1], dtype=torch.int64, device=DEV)          # 2^64 - 1 as uint64
    ops.counter_add(wrap, 2)
    assert wrap.item() == 1
    assert L.load().mmvae_counter_add(None, 1, torch.cuda.current_stream().cuda_stream) == -1


# ---------------------------------------------------------------------------------------------
# the engine's noise source: the stream position a checkpoint stores
# ---------------------------------------------------------------------------------------------
def test_noise_source_draw_follows_the_reference_stream():
    B, widths, Ld = 77, (100, 256, 33), 20          # 7700 and 2541 bytes: the segments need their 16-byte alignment
    torch.manual_seed(0x1234_5678_9ABC_DEF1)
    seed = torch.initial_seed() & (2 ** 64 - 1)
    src = engine.NoiseSource()
    dev = torch.device("cuda", torch.cuda.current_device())
    src.load_state_dict({"offset": 12345}, dev)
    segs, total = N.mask_segments(B, widths)
    assert segs == [0, 7712, 7712 + B * 256] and total == 7712 + B * 256 + 2544      # 7700 -> 7712, 2541 -> 2544
    off = 12345
    for _ in range(2):                              # the second draw starts where the first one ended
        masks, eps = src.draw(B, widths, Ld, dev)
        torch.cuda.synchronize()
        ref, ref_eps, nxt = N.noise_source_draw(seed, off, B, widths, Ld, 1.0 - ops.DROP_P)
        for m, r, w in zip(masks, ref, widths):
            assert tuple(m.shape) == (B, w) and m.dtype == torch.uint8
            np.testing.assert_array_equal(m.cpu().numpy().reshape(-1), r.reshape(-1))
        assert tuple(eps.shape) == (B, Ld)
        _check_eps(eps.double().cpu().numpy().reshape(-1), B * Ld, seed, N.eps_base(off, total))
        assert ref_eps.dtype == np.float32 and np.array_equal(ref_eps.reshape(-1), N.normals(B * Ld, seed, N.eps_base(off, total)).astype(np.float32))
        off += N.consumed(total, B * Ld)
        assert nxt == off
        assert src.state_dict(dev)["offset"] == off
        assert (src.offset_tensor(dev) == off).all()
    masks, eps = src.draw(B, widths, None, dev)     # masks alone (a directional model without eps)
    assert eps is None and src.state_dict(dev)["offset"] == off + N.consumed(total, 0)
