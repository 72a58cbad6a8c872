"""Inputs of the group-moments tests (numpy only), shared by tests/test_group_moments_bounds_cpu.py and tests/test_group_moments_gpu.py:
the smallest problems at which mmvae_gemm_nt_group_moments (csrc/group_moments.hip) can go wrong.

  G        1 (the mean is the row), 2, 3 (an odd group, 42 per tile, 2 idle rows), 24 (5 per tile, 8 idle rows), 128 (one per tile)
  B        1 (one partial tile) and 2 floor(128 / G) + 1 (two full tiles and one group in a third)
  shapes   (N, K, act): (8, 64, none) one K step, one narrow column tile; (782, 128, none) and (572, 512, sigmoid) the two decoders'
           last layers; (1177, 128, none) an odd width over ten column tiles
  offset   bias 100, products at the 1e-3 level: sum-of-squares minus square-of-sum cancels catastrophically there
  identical   the members of a group are the same row: the exact spread is 0
  slice    `a` is a column slice of a wider buffer (the GPU test builds the buffer; here it is an ordinary case)
The operands come from gemm_cases.nt_case (small-magnitude rows, tail-only columns, saturated logits), rounded to bf16.
"""
from collections import namedtuple

import numpy as np

import gemm_bounds as GB
import gemm_cases as GC

F32, F64 = np.float32, np.float64
TILE = 128
ACT_NONE, ACT_SIGMOID = 0, 2

GS = (1, 2, 3, 24, 128)
SHAPES = ((8, 64, ACT_NONE), (782, 128, ACT_NONE), (572, 512, ACT_SIGMOID), (1177, 128, ACT_NONE))

Case = namedtuple("Case", "name G B N K act kind")


def batch_sizes(G):
    return (1, 2 * (TILE // G) + 1)


def grid_cases():
    return [Case(f"G{G}-B{B}-N{N}-K{K}-{'sigmoid' if act else 'none'}", G, B, N, K, act, "grid")
            for G in GS for B in batch_sizes(G) for (N, K, act) in SHAPES]


def special_cases():
    return [Case("offset", 24, 11, 136, 64, ACT_NONE, "offset"),
            Case("identical", 3, 85, 136, 64, ACT_NONE, "identical"),
            Case("identical-sigmoid", 24, 6, 40, 128, ACT_SIGMOID, "identical"),
            Case("slice", 24, 11, 200, 128, ACT_SIGMOID, "slice")]


def all_cases():
    return grid_cases() + special_cases()


def bf16(x):
    """float32 values that are exactly representable in bf16 (nearest even)"""
    return GB.q_bf16(x).astype(F32)


def make(case, seed=0):
    """-> a [B G][K], w [N][K] (float32 holding bf16 values), bias [N] float32"""
    rng = np.random.default_rng(seed + 1000 * case.G + 7 * case.B + 3 * case.N + case.K)
    M = case.B * case.G
    if case.kind == "offset":
        a = GC.rnd(rng, M, case.K)
        w = GC.rnd(rng, case.N, case.K, scale=1e-3 * case.K ** -0.5)
        bias = np.full(case.N, 100.0, F32)
    else:
        a, w, bias = GC.nt_case(rng, M, case.N, case.K)
    if case.kind == "identical":
        a = np.repeat(a[::case.G], case.G, axis=0)
    return bf16(a), bf16(w), bias.astype(F32)
