"""mmvae_gemm_nt_group_moments (csrc/group_moments.hip) on the device against its float64 restatement, within the derived bounds of
tests/group_moments_bounds.py, on the cases of tests/group_moments_cases.py.  mean / std are views of NaN-filled buffers with a
leading dimension beyond N: the guard columns must stay untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import group_moments_bounds as MB  # noqa: E402
import group_moments_cases as MC  # noqa: E402
from gemm_gpu_util import DEV, NAN, PREC_BF16, PREC_F32, a_operand, dev, host, prep, status, within  # noqa: E402
from mmvae import ops  # noqa: E402

GUARD = 5


def outputs(B, N, with_std):
    """NaN-filled [B][N + GUARD] buffers -> (mean buffer, std buffer or None)"""
    return (torch.full((B, N + GUARD), NAN, device=DEV), torch.full((B, N + GUARD), NAN, device=DEV) if with_std else None)


def untouched(buf, N):
    return bool(torch.isnan(buf[:, N:]).all())


def run(case, lda=None):
    a, w, bias = MC.make(case)
    A, a_host = a_operand(a, PREC_BF16, "bf16", lda)
    pl = prep(w, bias, PREC_BF16)
    mean, std = outputs(case.B, case.N, case.G > 1)
    rc = status(ops.gemm_nt_group_moments, PREC_BF16, A, pl.w, case.N, case.K, case.G, mean[:, :case.N],
                None if std is None else std[:, :case.N], bias=pl.bias, act=case.act)
    assert rc == 0, case.name
    torch.cuda.synchronize()
    m, tm, s, ts = MB.problem_tol(a_host, host(pl.w[:case.N, :case.K]), bias.astype(np.float64), case.act, case.G)
    within(host(mean[:, :case.N]), m, tm, f"group moments {case.name} mean")
    assert untouched(mean, case.N), "mean: columns >= N were written"
    if std is not None:
        within(host(std[:, :case.N]), s, ts, f"group moments {case.name} std")
        assert untouched(std, case.N), "std: columns >= N were written"


@pytest.mark.parametrize("case", MC.grid_cases(), ids=lambda c: c.name)
def test_group_moments_within_bounds(case):
    run(case)


@pytest.mark.parametrize("case", [c for c in MC.special_cases() if c.kind != "slice"], ids=lambda c: c.name)
def test_group_moments_special_cases(case):
    run(case)


def test_group_moments_a_is_a_column_slice():
    case = next(c for c in MC.special_cases() if c.kind == "slice")
    run(case, lda=case.K + 72)                      # rows 16-byte aligned, NaN beyond the K columns


def test_group_moments_mean_only_and_no_bias():
    case = MC.Case("mean-only", 24, 11, 136, 64, MC.ACT_NONE, "grid")
    a, w, bias = MC.make(case)
    A, a_host = a_operand(a, PREC_BF16, "bf16")
    pl = prep(w, bias, PREC_BF16)
    mean, _ = outputs(case.B, case.N, False)
    assert status(ops.gemm_nt_group_moments, PREC_BF16, A, pl.w, case.N, case.K, case.G, mean[:, :case.N]) == 0
    torch.cuda.synchronize()
    m, tm, _, _ = MB.problem_tol(a_host, host(pl.w[:case.N, :case.K]), None, case.act, case.G)
    within(host(mean[:, :case.N]), m, tm, "group moments mean only, no bias")
    assert untouched(mean, case.N)


def test_group_moments_refusals_leave_the_outputs_untouched():
    G, B, N, K = 129, 2, 40, 64
    rng = np.random.default_rng(5)
    w, bias = MC.bf16(MC.GC.rnd(rng, N, K)), MC.GC.rnd(rng, N)
    pl = prep(w, bias, PREC_BF16)

    def call(prec, G, with_std):
        A, _ = a_operand(MC.bf16(MC.GC.rnd(rng, B * G, K)), PREC_BF16, "bf16")
        mean, std = outputs(B, N, True)
        rc = status(ops.gemm_nt_group_moments, prec, A, pl.w, N, K, G, mean[:, :N], std[:, :N] if with_std else None, bias=pl.bias)
        torch.cuda.synchronize()
        assert bool(torch.isnan(mean).all()) and bool(torch.isnan(std).all()), "a refused call wrote its outputs"
        return rc

    assert call(PREC_BF16, 129, True) == -1          # G above the tile
    assert call(PREC_F32, 24, True) == -2            # fp32 compute mode
    assert call(PREC_BF16, 1, True) == -1            # the spread of one member
    # an fp32 operand (the fp32 mode's activations) is refused the same way, before the library is asked
    mean, _ = outputs(B, N, False)
    A32 = dev(MC.GC.rnd(rng, B * 2, K))
    assert status(ops.gemm_nt_group_moments, PREC_F32, A32, pl.w, N, K, 2, mean[:, :N]) == -2
    assert bool(torch.isnan(mean).all())
