"""The numpy reference of the noise stream (oracle/np_noise.py) pinned on its own, without a GPU: tests/test_noise_gpu.py compares
the device stream with it bit for bit (masks) and element by element (normals), so the reference has to be right by itself.

  * Philox4x32-10 against the three known-answer vectors of the Random123 distribution (kat_vectors: philox4x32 10).
  * the 16-bit keep thresholds.
  * moments of 2^20 reference normals.
  * BOX_MULLER_F32_NOISE: what a float32 evaluation of the Box-Muller formula differs from the float64 one by, measured here with
    numpy over the 2^20 draws of seed 7 in units of 2^-24 * radius.  The GPU comparison allows 4 x that (DEVICE_MARGIN: the device's
    logf / sincosf / sqrtf may be off by a few ulp where glibc's float32 functions are within 1).
"""
import numpy as np

import np_noise as N

BOX_MULLER_F32_NOISE = 3.25          # x 2^-24 x sqrt(-2 ln u1); measured below: 3.246 (largest absolute difference 4.3e-7)
DEVICE_MARGIN = 4.0


def eps_tolerance(rad_ref):
    """|z_device - z_ref| allowed per element; rad_ref = sqrt(-2 ln u1) of that element in float64."""
    return DEVICE_MARGIN * BOX_MULLER_F32_NOISE * 2.0 ** -24 * rad_ref


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    assert _hex(N.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert _hex(N.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(N.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_philox_is_vectorised_consistently():
    c = np.arange(5, dtype=np.uint64) + np.uint64(0xFFFFFFFE)          # crosses 2^32: the second counter word changes
    out = N.philox4x32_10((c & N.M32, c >> np.uint64(32), np.uint64(N.TAG_MASK), np.uint64(0)), (3, 4))
    for i in range(5):
        one = N.philox4x32_10((int(c[i]) & 0xFFFFFFFF, int(c[i]) >> 32, N.TAG_MASK, 0), (3, 4))
        assert [int(o[i]) for o in out] == [int(o) for o in one]


def test_keep_thresholds():
    assert [N.t16_of(k) for k in (0.9, 0.5, 1.0, 0.0)] == [58982, 32768, 65536, 0]


def test_mask_layout_and_edges():
    m = N.mask_bytes(1 << 16, 0.9, 1234, 0)
    assert m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}
    assert abs(m.mean() - 58982 / 65536) < 5e-3
    assert N.mask_bytes(1000, 1.0, 5, 9).all() and not N.mask_bytes(1000, 0.0, 5, 9).any()
    # a prefix of a longer draw is the shorter draw, and quad q of a draw at offset o is quad 0 of a draw at o + 4 q
    assert np.array_equal(N.mask_bytes(37, 0.5, 11, 3), N.mask_bytes(64, 0.5, 11, 3)[:37])
    assert np.array_equal(N.mask_bytes(64, 0.5, 11, 3)[32:48], N.mask_bytes(16, 0.5, 11, 3 + 8))
    # byte 8 k + 2 j + h of a quad: half h of word j of counter offset + k
    r = N.philox4x32_10((7, 0, N.TAG_MASK, 0), (11, 0))
    want = [int((int(r[j]) >> (16 * h)) & 0xFFFF) < 32768 for j in range(4) for h in range(2)]
    assert N.mask_bytes(16, 0.5, 11, 6)[8:].tolist() == want           # k = 1 of quad 0 at offset 6 is counter 7


def test_counter_bookkeeping():
    assert N.consumed(0, 1) == 1 and N.consumed(1, 0) == 4 and N.consumed(16, 4) == 5 and N.consumed(17, 5) == 10
    assert N.eps_base(10, 17) == 18
    assert np.array_equal(N.normals(8, 3, 5)[4:], N.normals(4, 3, 6))   # one counter per four normals
    assert N.eps_base(2 ** 64 - 4, 16) == 0                             # 64-bit wrap


def test_noise_source_draw_layout():
    """The host restatement of one engine draw: 16-byte aligned mask segments inside ONE mask stream, the normals behind it,
    and the offset of the following draw."""
    B, widths, Ld = 7, (5, 16, 3), 3                # 35 -> 48, 112 -> 112, 21 -> 32 bytes
    assert N.mask_segments(B, widths) == ([0, 48, 160], 192)
    masks, eps, nxt = N.noise_source_draw(11, 1000, B, widths, Ld, 0.5)
    stream = N.mask_bytes(192, 0.5, 11, 1000)
    for m, o, w in zip(masks, (0, 48, 160), widths):
        assert m.shape == (B, w) and m.dtype == np.uint8 and np.array_equal(m.reshape(-1), stream[o:o + B * w])
    assert np.array_equal(masks[1].reshape(-1)[:16], N.mask_bytes(16, 0.5, 11, 1000 + 4 * 3))    # segment 1 starts at quad 3
    assert eps.shape == (B, Ld) and eps.dtype == np.float32
    assert np.array_equal(eps.reshape(-1), N.normals(21, 11, 1000 + 4 * 12).astype(np.float32))
    assert nxt == 1000 + 4 * 12 + 6
    m2, e2, n2 = N.noise_source_draw(11, nxt, B, (), Ld)               # no masks: the normals start at the offset itself
    assert m2 == [] and np.array_equal(e2.reshape(-1), N.normals(21, 11, nxt).astype(np.float32)) and n2 == nxt + 6
    m3, e3, n3 = N.noise_source_draw(11, 0, B, (5,), None)             # masks alone
    assert e3 is None and n3 == 4 * 3 and N.noise_source_draw(11, 2 ** 64 - 4, B, (5,), None)[2] == 8      # 64-bit wrap


def test_reference_normals_moments():
    z = N.normals(1 << 20, 7, 0)
    assert z.dtype == np.float64 and np.isfinite(z).all()
    # standard errors at n = 2^20: mean 1e-3, std 7e-4, kurtosis sqrt(24/n) = 4.8e-3; four of each
    assert abs(z.mean()) < 4e-3 and abs(z.std() - 1.0) < 3e-3
    assert abs((z ** 4).mean() / z.var() ** 2 - 3.0) < 2e-2


def test_float32_noise_of_the_box_muller_formula():
    """The float32 restatement stays inside BOX_MULLER_F32_NOISE x 2^-24 x radius on every one of the 2^20 draws of seed 7, so the
    bound the device stream is held to (4 x that) is not tighter than float32 arithmetic itself."""
    z, rad = N.normals(1 << 20, 7, 0, with_radius=True)
    z32 = N.normals(1 << 20, 7, 0, dtype=np.float32)
    assert z32.dtype == np.float32
    d = np.abs(z32.astype(np.float64) - z)
    worst = (d[rad > 0] / rad[rad > 0]).max() * 2.0 ** 24
    print(f"float32 Box-Muller noise: {worst:.3f} x 2^-24 x radius, max abs {d.max():.2e}")
    assert (d[rad == 0] == 0).all()
    assert worst <= BOX_MULLER_F32_NOISE
    assert worst >= 0.5 * BOX_MULLER_F32_NOISE          # the stored figure is the measured one, not a loose ceiling
    assert (d <= eps_tolerance(rad) / DEVICE_MARGIN).all()
