"""Input generators shared by tests/test_gemm_gpu.py, the loss-epilogue test of tests/test_loss_gpu.py and tests/test_gemm_bounds_cpu.py
(numpy only).  Every generator builds the edges that make a per-element bound tight where kernels go wrong:

  small-magnitude rows   one block of rows scaled by 1e-3: an error there hides behind the matrix maximum, not behind its own terms;
  tail-only columns      NT: a few W rows are zero except in the last 8-element K chunk (and one except in the last 64-step when
                         K % 64 != 0): their outputs are sums over the tail alone.  dW: a few P and Q columns are zero except in the
                         rows of the last 32-row step: their dW elements are sums over those rows alone, at any M;
  saturated logits       two bias elements of +-20: the sigmoid's argument rounding grows with |x|;
  exact zeros            the saved activation of the ReLU-mask epilogue is relu(normal): about half its elements are exactly 0.
"""
import numpy as np

F32, F64 = np.float32, np.float64
SMALL = F32(1e-3)


def rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(F32)


def small_rows(M):
    """The block of rows scaled by 1e-3: never the first block of a row-block run, and it crosses a 16-row MFMA tile."""
    r0 = M // 3
    return slice(r0, r0 + max(1, min(24, M // 8)))


def nt_tail_rows(N, K):
    """{W row: first k that is non-zero}"""
    rows = {1 % N: K - 8, N - 1: K - 8, N // 2: K - 8} if K > 8 else {}
    if K % 64 and K > 64:
        rows[(N // 2 + 1) % N] = K // 64 * 64
    return rows


def nt_case(rng, M, N, K, w_scale=None):
    """-> a [M][K], w [N][K], bias [N] (float32; the caller rounds to the compute type)."""
    a = rnd(rng, M, K)
    a[small_rows(M)] *= SMALL
    w = rnd(rng, N, K, scale=(K ** -0.5 if w_scale is None else w_scale))
    bias = rnd(rng, N)
    for j, k0 in nt_tail_rows(N, K).items():
        w[j, :k0] = 0
        bias[j] = 0
    bias[3 % N], bias[5 % N] = 20.0, -20.0            # two columns of saturated logits for the sigmoid
    return a, w, bias


def epi_case(rng, M, N):
    """Operands of the backward epilogues: h = relu(normal) (exact zeros), y, BatchNorm vectors, keep mask (90 %), coefficients."""
    h = np.maximum(rnd(rng, M, N), F32(0))
    y = rnd(rng, M, N)
    f = lambda: rng.uniform(0.5, 1.5, N).astype(F32)
    d = dict(h=h, y=y, scale=f(), shift=f() - F32(1), mean=f() - F32(1), rstd=f(), mask=(rng.random((M, N)) < 0.9).astype(np.uint8),
             coef=np.stack([f(), rnd(rng, N, scale=0.1), rnd(rng, N, scale=0.1)]))
    assert (h == 0).mean() > 0.3
    return d


def loss_case(rng, M, N, bce):
    """Targets: MSE normal; BCE hard 0 / 1 in the first half of the rows, fractional in the second."""
    if not bce:
        return rnd(rng, M, N)
    t = rng.random((M, N)).astype(F32)
    t[:M // 2] = (t[:M // 2] > 0.5).astype(F32)
    return t


def dw_tail(M, rps=None):
    """Rows of the last 32-row step of the last split (rps rows per split; None: one split)."""
    last0 = 0 if rps is None else (M - 1) // rps * rps
    n = M - last0
    return slice(last0 + (n - 1) // 32 * 32, M)


def dw_case(rng, M, N, K, tail=None):
    """-> p [M][N], q [M][K] (float32).  tail: the rows that the tail-only columns (P columns 1, N - 1; Q columns 2, K - 1) keep."""
    p, q = rnd(rng, M, N), rnd(rng, M, K)
    p[small_rows(M)] *= SMALL
    tail = dw_tail(M) if tail is None else tail
    keep = np.zeros(M, bool)
    keep[tail] = True
    for c in (1 % N, N - 1):
        p[~keep, c] = 0
    for c in (2 % K, K - 1):
        q[~keep, c] = 0
    return p, q
