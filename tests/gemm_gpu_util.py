"""Helpers of the GPU tests that hold the GEMM kernels to the per-element bounds of tests/gemm_bounds.py (tests/test_gemm_gpu.py and the
loss-epilogue tests of tests/test_loss_gpu.py): operands as the ABI wants them (include/mmvae_hip.h), references from the values the
device actually stores, and `within`, which reports every comparison's worst err / bound before it asserts."""
import numpy as np
import torch

import gemm_bounds as G
import gemm_cases as GC
from mmvae import _lib as L
from mmvae import ops
from mmvae.ops import PREC_BF16, PREC_F32  # noqa: F401
from test_gemm_folded_gpu import DEV, NAN, dev, host, inside, prep, status  # noqa: F401
from test_gemm_folded_gpu import TUNING_DEFAULTS as FOLDED_DEFAULTS, tuning as folded_tuning
from test_model_gpu import report

TUNING_DEFAULTS = {**FOLDED_DEFAULTS, 2: 1, 6: 1, 7: 1}       # with the keys the folded file never changes (csrc/common.h: Tuning)
F32, F64 = np.float32, np.float64


class tuning(folded_tuning):
    """The folded file's `tuning` over this module's table of defaults."""

    def __exit__(self, *exc):
        for k in self.keys:
            L.load().mmvae_set_tuning(k, TUNING_DEFAULTS[k])
        return False


def within(got, ref, tol, what):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    tol = np.broadcast_to(np.asarray(tol, F64), ref.shape)
    err = np.abs(got - ref)
    nz = tol > 0
    ratio = float(np.max(err[nz] / tol[nz])) if nz.any() and got.shape == ref.shape else 0.0
    report(f"gemm bounds | {what} | worst err / bound {ratio:.3f}")
    inside(got, ref, tol, what)


def prec_name(prec):
    return "bf16" if prec == PREC_BF16 else "fp32"


def a_operand(a, prec, kind, ld=None):
    """The A (or P / Q) operand [M][K] as a view of a wider buffer -> (view, the values the kernel multiplies, float64).
    kind 'bf16': pad columns up to 8 elements hold ZEROS (the ABI demands it of a bf16 A), everything beyond NaN;
    kind 'f32': an fp32 operand, rounded to bf16 on load in bf16 mode (exactly, to nearest even); pad columns NaN."""
    M, K = a.shape
    if kind == "bf16":
        k8 = ops.ceil_to(K, 8)
        buf = torch.full((M, ld or k8), NAN, dtype=torch.bfloat16, device=DEV)
        buf[:, :k8] = 0
        buf[:, :K] = dev(a).to(torch.bfloat16)
        v = buf[:, :K]
        return v, host(v)
    buf = torch.full((M, ld or K), NAN, device=DEV)
    buf[:, :K] = dev(a)
    v = buf[:, :K]
    return v, (G.q_bf16(host(v)) if prec == PREC_BF16 else host(v))


def col_slice(x, dtype, off=0, extra=0, fill=NAN):
    """x [M][N] as columns off .. off + N of a buffer [M][off + ceil8(N) + extra] filled with `fill` -> (view [M][N], buffer)."""
    M, N = x.shape
    buf = torch.full((M, off + ops.ceil_to(N, 8) + extra), fill, dtype=dtype, device=DEV)
    buf[:, off:off + N] = dev(np.asarray(x)).to(dtype)
    return buf[:, off:off + N], buf


class Out:
    """An output [M][N] as columns off .. off + N of a sentinel-filled buffer; guards(): everything outside the ceil8(N) columns is
    unchanged and the pad columns N .. ceil8(N) are untouched or zero."""

    def __init__(self, M, N, dtype, off=0, extra=8, ld=None, sentinel=7.0):
        n8 = ops.ceil_to(N, 8)
        self.N, self.n8, self.off, self.s = N, n8, off, sentinel
        self.buf = torch.full((M, ld or off + n8 + extra), sentinel, dtype=dtype, device=DEV)
        self.c = self.buf[:, off:off + N]

    def guards(self):
        b = self.buf.float()
        pad = b[:, self.off + self.N:self.off + self.n8]
        return bool(torch.all(b[:, :self.off] == self.s) and torch.all(b[:, self.off + self.n8:] == self.s) and torch.all((pad == self.s) | (pad == 0)))


class NtCase:
    """One NT problem with the edges of tests/gemm_cases.py; reference and bound of x = a w^T + bias from the stored values."""

    def __init__(self, prec, M, N, K, a_kind, lda=None, w_scale=None, bias=True, seed=0):
        self.rng = rng = np.random.default_rng(seed + M + 3 * N + 7 * K)
        self.prec, self.M, self.N, self.K, self.a_kind = prec, M, N, K, a_kind
        a, w, b = GC.nt_case(rng, M, N, K, w_scale)
        self.a, self.a_host = a_operand(a, prec, a_kind, lda)
        self.pl = prep(w, b, prec)
        self.W_host = host(self.pl.w[:N, :K])
        self.b_host = b.astype(F64) if bias else None
        self.bias = self.pl.bias if bias else None
        self.ref = G.nt_ref(self.a_host, self.W_host, self.b_host)
        self.tol = G.nt_tol(self.a_host, self.W_host, self.b_host)
        self.tag = f"{prec_name(prec)} M{M} N{N} K{K} A {a_kind}"

    def gemm(self, out, **kw):
        return status(ops.gemm_nt, self.prec, self.a, self.pl.w, self.N, self.K, out, bias=self.bias, **kw)


def row_blocks(M, row_bytes, log2_split):
    """The blocks for_row_blocks (csrc/common.h) makes at mmvae_set_tuning(3, log2_split) -> [(r0, rows)]; asserts the path is taken."""
    assert M * row_bytes >= 1 << log2_split, "not a row-block problem"
    rows = (1 << (log2_split - 1)) // row_bytes
    assert rows > 0
    nblk = -(-M // rows)
    even = -(-M // nblk)
    if even >= 256:
        even = (even + 255) & ~255
    if even <= rows:
        rows = even
    elif rows >= 256:
        rows &= ~255
    blocks = [(r0, min(rows, M - r0)) for r0 in range(0, M, rows)]
    assert len(blocks) >= 2
    return blocks


def tn_plan_rows(M, MT, ntiles, wg_target):
    """plan_splits (csrc/common.h) for an automatic split -> (nsplit, rows per split)."""
    nsplit = wg_target // ntiles
    if nsplit >= 8:
        nsplit &= ~7
    nsplit = max(1, min(nsplit, -(-M // (4 * MT))))
    rps = -(-(-(-M // nsplit)) // MT) * MT                  # ceil(M / nsplit), rounded up to whole MT-row steps
    return -(-M // rps), rps


def tn_wide_plan(M, N, K, pmode, q_kind, ldq=None, ldp=None, ldpy=None, q_aligned=True):
    """What launch_tn_wide (csrc/gemm_tn_wide.hip) does with a bf16 P (pmode: BatchNorm-corrected from d and y, row strides ldp and
    ldpy) and a Q of q_kind 'bf16' or 'f32' (row stride ldq, q_aligned: the first row on 16 bytes), given a slab that holds the
    splits -> None (not taken) or (form, tile, ntiles, nsplit, rows per split); form 'dma' = LDS-DMA ring, 'reg' = register-staged,
    tile = (256, 288) or (128, 448)."""
    ldp = ops.ceil_to(N, 8) if ldp is None else ldp
    ldpy = ldp if ldpy is None else ldpy
    if M < 8192 or N < 128 or K < 256 or ldp % 8 or (pmode and (ldpy % 8 or N % 8)):
        return None
    if q_kind == "bf16":
        ldq = ops.ceil_to(K, 8) if ldq is None else ldq
        if ldq % 8 or pmode or M % 32 or N * K < 4 << 20:
            return None
        vec, tile = 8, (256, 288)
    else:
        ldq = K if ldq is None else ldq
        vec = 4 if ldq % 4 == 0 and K % 4 == 0 and q_aligned else 2 if ldq % 2 == 0 and K % 2 == 0 else 1
        if vec == 1 or (not pmode and (vec != 4 or M % 32)):
            return None
        padded = lambda nt, kt: -(-N // nt) * nt * (-(-K // kt) * kt)
        tile = (128, 448) if N <= 128 or padded(128, 448) < padded(256, 288) else (256, 288)       # least padded output
        if pmode and tile == (256, 288) and (vec != 4 or M % 32 or ldp != ldpy):
            return None
    ntiles = -(-K // tile[1]) * -(-N // tile[0])
    if ntiles > (32 if pmode else 4096):
        return None
    nsplit, rps = tn_plan_rows(M, 32, ntiles, 256)
    if pmode and nsplit < 2:
        return None
    return ("reg" if pmode and tile == (128, 448) else "dma"), tile, ntiles, nsplit, rps


def within_blocks(got, ref, tol, blocks, what):
    """Block by block, so that a failure names the row block: an operand advanced by the wrong stride shows from the second block on."""
    for i, (r0, rows) in enumerate(blocks):
        within(got[r0:r0 + rows], ref[r0:r0 + rows], np.broadcast_to(tol, ref.shape)[r0:r0 + rows], f"{what}, row block {i} (rows {r0}..{r0 + rows - 1})")


def loss_target(t, kind, ld=None):
    """Target [M][N] on the device: 'f32' or 'bf16', row stride ld (default N), pad columns NaN -> (view, stored values float64)."""
    M, N = t.shape
    dt = torch.float32 if kind == "f32" else torch.bfloat16
    buf = torch.full((M, ld or N), NAN, dtype=dt, device=DEV)
    buf[:, :N] = dev(t).to(dt)
    v = buf[:, :N]
    return v, host(v)


def check_loss_epilogue(case, bce, T, t_host, what, blocks=None):
    """Runs the loss epilogue of `case` and holds gradient rows, pad columns, guards and the f64 loss sum against float64."""
    M, N, K = case.M, case.N, case.K
    assert case.prec == PREC_BF16 and case.a_kind == "bf16" and K > 64                     # gemm_nt.hip dispatch_epi: nt2 only
    g = Out(M, N, torch.bfloat16, extra=8)
    sums = torch.zeros(3, dtype=torch.float64, device=DEV)
    assert case.gemm(g.c, epilogue=ops.EPI_LOSS_BCE_LOGIT if bce else ops.EPI_LOSS_MSE, h=T, loss_sum=sums[1:2]) == 0
    torch.cuda.synchronize()
    gref, gtol, lref, ltol = (G.bce_epilogue if bce else G.mse_epilogue)(case.ref, case.tol, t_host)
    gtol = G.bf16_out(gtol, gref)
    got = host(g.c)
    if blocks:
        within_blocks(got, gref, gtol, blocks, f"{what} gradient")
    else:
        within(got, gref, gtol, f"{what} gradient")
    n8 = ops.ceil_to(N, 8)
    assert float(g.buf[:, N:n8].float().abs().max() if n8 > N else 0.0) == 0.0, "pad columns of the gradient must be zeroed"
    assert g.guards(), "the gradient buffer was written outside its ceil8(N) columns"
    s = host(sums)
    assert s[0] == 0 and s[2] == 0
    within(s[1:2], [float(lref.sum())], [G.loss_sum_tol(lref, ltol)], f"{what} loss sum")
