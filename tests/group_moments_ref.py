"""mmvae_gemm_nt_group_moments (csrc/group_moments.hip) restated twice in numpy: in float64 (the reference the device is compared
with) and in float32 as the kernel computes it (tests/test_group_moments_bounds_cpu.py holds it to tests/group_moments_bounds.py, in
several summation orders, and shows that a set of deliberate mistakes falls outside)."""
import numpy as np

import gemm_bounds as GB

F32, F64 = np.float32, np.float64
TILE = 128
ACT_NONE, ACT_SIGMOID = 0, 2
K_ORDERS = ("blas", "steps-ascending", "steps-descending")
MISTAKES = ("divisor-G", "mean-divisor-G-1", "variance", "one-pass", "mean-over-tile-rows", "neighbour-row", "idle-rows",
            "sigmoid-after-mean", "std-of-logits")


def logits64(a, w, bias):
    return GB.nt_ref(a, w, bias)


def x64(a, w, bias, act):
    v = logits64(a, w, bias)
    return GB.sigmoid(v) if act == ACT_SIGMOID else v


def moments64(x, G):
    """float64 mean and unbiased std over every G consecutive rows -> (mean [B][N], std [B][N] or None for G == 1)"""
    x = np.asarray(x, F64).reshape(-1, G, x.shape[1])
    return x.mean(1), (x.std(1, ddof=1) if G > 1 else None)


def _logits32(a, w, bias, order):
    """fp32 accumulation of the (exact) bf16 products in one of K_ORDERS, then the bias in fp32"""
    a, w = np.asarray(a, F32), np.asarray(w, F32)
    if order == "blas":
        acc = a @ w.T
    else:
        K = a.shape[1]
        steps = [slice(k, k + 32) for k in range(0, K, 32)]                 # one MFMA step each
        acc = np.zeros((a.shape[0], w.shape[0]), F32)
        for s in (steps if order == "steps-ascending" else steps[::-1]):
            acc = acc + (a[:, s] @ w[:, s].T).astype(F32)
    return acc + np.asarray(bias, F32)


def _sigmoid32(v):
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-v.astype(F32)).astype(F32))).astype(F32)


def emulate(a, w, bias, act, G, order="blas", descending=False, mistake=None):
    """The kernel in float32 -> (mean [B][N], std [B][N] or None).  descending: the group walk from g = G - 1 down.  mistake: one of
    MISTAKES (None: the kernel as it is)."""
    assert mistake is None or mistake in MISTAKES
    v = _logits32(a, w, bias, order)
    sig = act == ACT_SIGMOID
    x = _sigmoid32(v) if (sig and mistake != "sigmoid-after-mean") else v
    M, N = x.shape
    B, gpt = M // G, TILE // G
    mean, std = np.zeros((B, N), F32), (np.zeros((B, N), F32) if G > 1 else None)
    for b in range(B):
        rows = list(range(b * G, (b + 1) * G))
        if mistake == "neighbour-row" and b + 1 < B:
            rows[-1] = (b + 1) * G
        if mistake == "idle-rows" and (b % gpt == gpt - 1 or b == B - 1):    # the tile's last group walks on into the idle rows
            rows += [min(r, M - 1) for r in range((b + 1) * G, (b + 1) * G + TILE - gpt * G)]
        if descending:
            rows = rows[::-1]
        s = np.zeros(N, F32)
        for r in rows:
            s = s + x[r]
        div = F32(TILE if mistake == "mean-over-tile-rows" else (G - 1 if mistake == "mean-divisor-G-1" and G > 1 else G))
        mu = (s / div).astype(F32)
        mean[b] = _sigmoid32(mu) if (sig and mistake == "sigmoid-after-mean") else mu
        if std is None:
            continue
        y = v if mistake == "std-of-logits" else x
        if mistake == "std-of-logits":
            s = np.zeros(N, F32)
            for r in rows:
                s = s + y[r]
            mu = (s / F32(G)).astype(F32)
        ss = np.zeros(N, F32)
        if mistake == "one-pass":
            for r in rows:
                ss = ss + y[r] * y[r]
            ss = ss - s * s / F32(G)
        else:
            for r in rows:
                d = y[r] - mu
                ss = ss + d * d
        var = (ss / F32(G if mistake == "divisor-G" else G - 1)).astype(F32)
        with np.errstate(invalid="ignore"):
            std[b] = var if mistake == "variance" else np.sqrt(var)
    return mean, std
