"""Inputs of the loss-kernel tests: tests/test_loss_kernel_gpu.py runs the device on them, tests/test_loss_bounds_cpu.py shows on the
same arrays that the bounds of tests/loss_bounds.py hold for float32 arithmetic, that deliberate mistakes fall outside them, and that
the edges named here are really present (edge counts).  Everything is float32 (targets optionally rounded to bf16 values)."""
import numpy as np

from gemm_bounds import q_bf16

F32 = np.float32
FLUSH32 = F32(2.0 ** -126)


def _bf16(x):
    return q_bf16(x).astype(F32)


def mse_case(rng, B, W, t_bf16=False):
    """Predictions and targets of mixed magnitude: rows scaled by 1e-3 ... 1e3; every 5th entry of the prediction an exact zero, every
    7th of the target; every 11th entry equal to its target.  -> (x, t)"""
    scale = (10.0 ** rng.uniform(-3, 3, (B, 1)))
    x = (rng.standard_normal((B, W)) * scale).astype(F32)
    t = (rng.standard_normal((B, W)) * scale).astype(F32)
    flat = np.arange(B * W).reshape(B, W)
    x[flat % 5 == 0] = 0.0
    t[flat % 7 == 0] = 0.0
    if t_bf16:
        t = _bf16(t)
    eq = flat % 11 == 0
    x[eq] = t[eq]
    return x, t


P_CLAMP = F32(1e-12)
P_EDGES = np.array([0.0, 1.0, 2.0 ** -149, 1e-40, 1e-38, 1e-13, 0.5, 1.0 - 2.0 ** -24] +
                   [float(P_CLAMP) * (1 + k * 2.0 ** -23) for k in (-3, -2, -1, 0, 1, 2, 3)], dtype=np.float64).astype(F32)
T_EDGES = np.array([0.0, 1.0, 0.3], F32)


def bce_case(rng, B, W, t_bf16=False):
    """p random in (1e-4, 1 - 1e-4) against targets in (0, 1), then every pair of P_EDGES x T_EDGES spread over the matrix: p in
    {0, 1} (both logs reach their clamp), denormal p (2^-149, 1e-40, 1e-38), 1e-13 and a few ulp on either side of p (1 - p) = 1e-12
    (the gradient's clamp), 0.5, the largest p below 1; targets 0, 1 and fractional.  Needs B W >= 45.  -> (p, t)"""
    p = rng.uniform(1e-4, 1 - 1e-4, (B, W)).astype(F32)
    t = rng.uniform(0, 1, (B, W)).astype(F32)
    pe, te = [a.ravel() for a in np.meshgrid(P_EDGES, T_EDGES, indexing="ij")]
    assert B * W >= len(pe)
    pos = np.arange(len(pe)) * (B * W // len(pe))
    p.ravel()[pos], t.ravel()[pos] = pe, te
    return p, (_bf16(t) if t_bf16 else t)


def bce_edge_counts(p, t):
    p64 = p.astype(np.float64)
    pq = (1 - p64) * p64
    return dict(zero=int((p == 0).sum()), one=int((p == 1).sum()), denormal=int(((p > 0) & (p < FLUSH32)).sum()),
                clamped=int((pq < 1e-12).sum()), unclamped_near=int(((pq >= 1e-12) & (pq < 1.000001e-12)).sum()),
                hard_targets=int(((t == 0) | (t == 1)).sum()))


BAD_LABELS = (-1, None, 2 ** 40, -2 ** 62)          # None: S


def class_case(rng, B, S, weighted):
    """Logits: standard normal x 3; row r % 5 == 1 all equal; row r % 5 == 3 spread over [-60, 60] with both ends present (S > 1: the
    exponentials underflow against the maximum) and shifted as a whole by 0, +45 or -45 (a softmax that does not subtract the
    maximum overflows at +105).  Labels: random valid ones; the row's maximum on rows r % 11 == 4, its minimum on r % 11 == 5; -100 on
    every 7th row; -1, S, 2^40, -2^62 in turn on rows 2, 93, 184, ... (never a multiple of 7).  Weights: none, or (0.3, 3) with the
    weight of class S // 2 exactly 0 (S > 1).  -> (x, y int64, class weights or None)"""
    x = (3 * rng.standard_normal((B, S))).astype(F32)
    r = np.arange(B)
    eq = r % 5 == 1
    x[eq] = x[eq, :1]
    wide = np.flatnonzero(r % 5 == 3)
    if len(wide):
        xw = rng.uniform(-60, 60, (len(wide), S))
        if S > 1:
            k = np.arange(len(wide))
            hi = rng.integers(0, S, len(wide))
            lo = (hi + 1 + rng.integers(0, S - 1, len(wide))) % S
            xw[k, hi], xw[k, lo] = 60.0, -60.0
        x[wide] = (xw + np.array([0.0, 45.0, -45.0])[np.arange(len(wide)) % 3][:, None]).astype(F32)
    y = rng.integers(0, S, B).astype(np.int64)
    y[r % 11 == 4] = x[r % 11 == 4].argmax(1)
    y[r % 11 == 5] = x[r % 11 == 5].argmin(1)
    y[::7] = -100
    for k, row in enumerate(range(2, B, 91)):
        v = BAD_LABELS[k % 4]
        y[row] = S if v is None else v
    cw = None
    if weighted:
        cw = rng.uniform(0.3, 3.0, S).astype(F32)
        if S > 1:
            cw[S // 2] = 0.0
    return x, y, cw


def class_edge_counts(x, y, cw):
    B, S = x.shape
    ign = y == -100
    bad = ~ign & ((y < 0) | (y >= S))
    ok = ~ign & ~bad
    xm = x.astype(np.float64) - x.max(1, keepdims=True)
    lab = np.where(ok, y, 0)
    at_max = x[np.arange(B), lab] == x.max(1)
    return dict(ignored=int(ign.sum()), bad=int(bad.sum()), equal_rows=int((x == x[:, :1]).all(1).sum()),
                underflow_rows=int((xm < -104).any(1).sum()), overflow_rows=int((x.max(1) > 89).sum()),
                label_is_max=int((ok & at_max).sum()), label_not_max=int((ok & ~at_max).sum()),
                zero_weight_rows=0 if cw is None else int((ok & (cw[lab] == 0)).sum()))


LV_EDGES = np.array([0.0, -110.0, -20.0, 20.0, 80.0], F32)


def kl_case(rng, B, L):
    """mu N(0, 1) with |mu| = 50 on every 97th element; logvar N(0, 1) with 0, -110 (exp underflows to 0), -20, 20, 80 (below 88, where
    fp32 exp overflows and the reference does not) in turn on every 13th element.  A single element stays a plain draw.  -> (mu, lv)"""
    mu, lv = rng.standard_normal((B, L)).astype(F32), rng.standard_normal((B, L)).astype(F32)
    n = B * L
    if n >= 16:
        pos = np.arange(3, n, 13)
        lv.ravel()[pos] = LV_EDGES[np.arange(len(pos)) % 5]
        pos = np.arange(5, n, 97)
        mu.ravel()[pos] = np.where(np.arange(len(pos)) % 2 == 0, 50.0, -50.0)
    return mu, lv


def kl_edge_counts(mu, lv):
    return dict(big_mu=int((np.abs(mu) == 50).sum()), **{f"lv {v:g}": int((lv == v).sum()) for v in LV_EDGES})
