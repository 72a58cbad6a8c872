"""Numpy restatement of the library's noise stream (include/mmvae_hip.h: mmvae_noise), written from the header's and the kernel's
description: Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as 1, 2, 3") keyed by the 64-bit seed, with a
128-bit counter whose low 64 bits are the running offset and whose third word is a stream tag.

  dropout keep-mask   quad q (16 bytes) uses the counters offset + 4q + k, k in {0, 1}, tag "MASK"; every 32-bit output word
                      decides two bytes, low 16-bit half first, by half < t16.  (offset + 4q + 2, + 3 stay unused.)
  standard normals    quad q (4 floats) uses the counter offset + q, tag "NORM"; Box-Muller on (0, 1] x [0, 1).
  one combined call   the normals start at offset + 4 ceil(n_mask / 16); the call consumes consumed(n_mask, n_eps) counters.

Everything is vectorised over uint64 arrays (32-bit values held in 64-bit lanes, so the 32 x 32 products are exact).
"""
import numpy as np

TAG_MASK = 0x4D41534B        # "MASK"
TAG_NORM = 0x4E4F524D        # "NORM"
M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85      # Weyl increments of the two key words
_S32 = np.uint64(32)


def philox4x32_10(ctr4, key2):
    """ctr4: four uint64 arrays (or scalars) holding 32-bit counter words, key2: two 32-bit key words -> four uint64 arrays of
    32-bit outputs.  Ten rounds; the key is bumped by the Weyl constants BETWEEN rounds (nine times)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in ctr4)
    k0, k1 = int(key2[0]) & 0xFFFFFFFF, int(key2[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2                     # < 2^64: exact
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & M32, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & M32
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _stream(seed, counters, tag):
    """Philox outputs [4][n] for the 64-bit counters (uint64 array; arithmetic on it wraps as the device's does)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((counters & M32, counters >> _S32, np.uint64(tag), np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))


def _u64(x):
    return np.uint64(int(x) & 0xFFFFFFFFFFFFFFFF)


def t16_of(keep_prob):
    """16-bit keep threshold: floor(float32(keep) * 2^32) >> 16; keep = 1 (any product that does not fit 32 bits) -> 0x10000, so
    that every 16-bit value passes.  The keep probability is therefore quantised to 1/65536 (0.9 -> 58982 / 65536)."""
    t = int(np.floor(float(np.float32(keep_prob)) * 4294967296.0))
    return 0x10000 if t >= 0xFFFFFFFF else t >> 16


def mask_bytes(n, keep_prob, seed, offset):
    """-> uint8[n] of 0 / 1.  Byte 8k + 2j + h of quad q is decided by half h (0 = low 16 bits) of output word j of counter
    offset + 4q + k."""
    nq = (int(n) + 15) // 16
    q = np.arange(nq, dtype=np.uint64)
    t16 = np.uint64(t16_of(keep_prob))
    out = np.empty((nq, 2, 4, 2), dtype=np.uint8)
    with np.errstate(over="ignore"):
        for k in range(2):
            r = _stream(seed, _u64(offset) + q * np.uint64(4) + np.uint64(k), TAG_MASK)
            for j in range(4):
                out[:, k, j, 0] = (r[j] & np.uint64(0xFFFF)) < t16
                out[:, k, j, 1] = (r[j] >> np.uint64(16)) < t16
    return out.reshape(-1)[:int(n)]


def _uniforms(n, seed, offset):
    nq = (int(n) + 3) // 4
    with np.errstate(over="ignore"):
        r = _stream(seed, _u64(offset) + np.arange(nq, dtype=np.uint64), TAG_NORM)
    # pair k of a quad: u1 from word 2k, u2 from word 2k + 1; 24-bit mantissas, both exactly representable in float32
    u1 = np.stack([(r[0] >> np.uint64(8)).astype(np.float64) + 1.0, (r[2] >> np.uint64(8)).astype(np.float64) + 1.0], 1) * 2.0 ** -24
    u2 = np.stack([(r[1] >> np.uint64(8)).astype(np.float64), (r[3] >> np.uint64(8)).astype(np.float64)], 1) * 2.0 ** -24
    return u1, u2            # [nq][2]: u1 in (0, 1], u2 in [0, 1)


def normals(n, seed, offset, dtype=np.float64, with_radius=False):
    """-> float64[n] standard normals: z[4q + 2k] = rad cos(a), z[4q + 2k + 1] = rad sin(a), rad = sqrt(-2 ln u1) and
    a = float32(2 pi) * u2 ROUNDED TO float32 as the device forms it; everything after that in `dtype` (float64: the reference;
    float32: the restatement tests/test_noise_ref_cpu.py measures the float32 noise of the formula with).
    with_radius: also the float64 radius of every element (the scale of the comparison's tolerance)."""
    u1, u2 = _uniforms(n, seed, offset)
    ang = (np.float32(6.283185307179586) * u2.astype(np.float32)).astype(np.float32)
    rad64 = np.sqrt(-2.0 * np.log(u1))
    if dtype == np.float32:
        rad = np.sqrt(np.float32(-2.0) * np.log(u1.astype(np.float32)))
        a = ang
    else:
        rad, a = rad64, ang.astype(np.float64)
    z = np.stack([rad * np.cos(a), rad * np.sin(a)], 2).reshape(-1)[:int(n)]      # [nq][2][cos, sin]
    if with_radius:
        return z, np.repeat(rad64.reshape(-1), 2)[:int(n)]
    return z


def consumed(n_mask, n_eps):
    """Counter values one call uses: four per 16 mask bytes (two of them drawn), one per four normals."""
    return 4 * ((int(n_mask) + 15) // 16) + (int(n_eps) + 3) // 4


def eps_base(offset, n_mask):
    """First counter of the normals of a combined call."""
    return (int(offset) + 4 * ((int(n_mask) + 15) // 16)) & 0xFFFFFFFFFFFFFFFF


def mask_segments(B, widths):
    """-> ([first byte of every (B, w) keep-mask], bytes in all) of one combined mask buffer: every segment starts on a
    16-byte boundary (a whole quad), so the gaps draw and drop random bytes."""
    segs, total = [], 0
    for w in widths:
        segs.append(total)
        total = (total + int(B) * int(w) + 15) // 16 * 16
    return segs, total


def noise_source_draw(seed, offset, B, widths, Ld, keep_prob=0.9):
    """One draw of the engine's noise source (mmvae.engine.NoiseSource.draw) restated on the host: ONE combined call for all
    keep-masks of a forward, laid out by mask_segments, and the (B, Ld) normals behind them (none if Ld is None).
    -> ([uint8 (B, w) keep-mask for w in widths], eps float32 (B, Ld) or None, offset of the next draw)."""
    segs, total = mask_segments(B, widths)
    ref = mask_bytes(total, keep_prob, seed, offset) if total else None
    masks = [ref[o:o + B * w].reshape(B, w) for o, w in zip(segs, widths)]
    n_eps = 0 if Ld is None else B * Ld
    eps = normals(n_eps, seed, eps_base(offset, total)).astype(np.float32).reshape(B, Ld) if n_eps else None
    return masks, eps, (int(offset) + consumed(total, n_eps)) & 0xFFFFFFFFFFFFFFFF
