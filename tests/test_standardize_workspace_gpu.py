"""The caller-owned workspace of mmvae_standardize_fit on the MI355X, as tests/test_workspace_contract_gpu.py holds the other entries
to it: a workspace of exactly mmvae_standardize_fit_work_bytes between two guards (tests/workspace_util.py), 8 bytes aligned and no more,
filled with 0x00, with 0xFF (NaN partial sums) and with the stale partials of a larger problem, gives bit-identical results within the
derived bounds and leaves the guards intact; its first and last word are written; one byte short is refused with nothing written."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import standardize_bounds as B  # noqa: E402
import standardize_ref as R  # noqa: E402
from mmvae import _lib, ops  # noqa: E402
from test_standardize_gpu import DEV, dev_parts, problem  # noqa: E402
from workspace_util import GUARD_BYTE, guarded  # noqa: E402


def stale_image():
    """the work region a larger problem of the same entry left: plausible partial sums"""
    x = torch.randn(5000, 300, device=DEV, generator=torch.Generator(DEV).manual_seed(5)) * 3 + 1
    g = guarded(ops.standardize_fit_work_bytes(5000, 300, 64), "ones", DEV)
    ops.standardize_fit(x, splits=64, work=g.tensor)
    torch.cuda.synchronize()
    g.check("stale run")
    return g.image().cpu()


@pytest.mark.parametrize("name,splits", [("r1", 0), ("r65", 0), ("r257", 5), ("r1000", 0), ("r4099", 0), ("r4099", 64)])
def test_fit_workspace(name, splits):
    case, arrs, X, ref = problem(name)
    rows, F = X.shape
    parts = dev_parts(case.parts, arrs, rows)
    used = ops.standardize_fit_splits(rows, F, splits)
    need = ops.standardize_fit_work_bytes(rows, F, splits)
    assert need == 16 * F * used == R.work_bytes(rows, F, splits) and need % 8 == 0
    want = ops.standardize_fit(parts, splits=splits)
    for g_, w, t in zip(want, ref, B.fit_tol(X, used)):
        assert np.all(np.abs(g_.cpu().numpy() - w) <= t)
    for fill in ("zero", "ones", "stale"):
        g = guarded(need, stale_image() if fill == "stale" else fill, DEV)
        got = ops.standardize_fit(parts, splits=splits, work=g.tensor)
        torch.cuda.synchronize()
        for u, v in zip(got, want):
            assert torch.equal(u.view(torch.int64), v.view(torch.int64)), (name, f"the result depends on the workspace's contents: fill {fill}")
        g.check(f"{name}, fill {fill}")
    # the planner's last byte is used: from 0xA5 the first and the last word change
    g = guarded(need, bytes([GUARD_BYTE]), DEV)
    before = g.image()
    ops.standardize_fit(parts, splits=splits, work=g.tensor)
    g.check(f"{name}, fill 0xA5")
    assert g.word_changed(0, before) and g.word_changed(need - 4, before)

    # one byte short: MMVAE_ERR_ARG, nothing written
    outs = [torch.full((F,), -7.0, dtype=torch.float64, device=DEV) for _ in range(3)]
    g.fill("ones")
    whole = g.buf.clone()
    a = _lib.StandardizeFitArgs()
    ops._std_fill(a, parts)
    a.mean, a.var, a.scale, a.work, a.work_bytes = outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), g.ptr, need - 1
    a.rows, a.splits = rows, splits
    assert _lib.load().mmvae_standardize_fit(C.byref(a), None) == -1
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs) and torch.equal(g.buf, whole)
    a.work_bytes = need                                                                  # the same arguments with the whole workspace pass
    assert _lib.load().mmvae_standardize_fit(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for o, v in zip(outs, want):
        assert torch.equal(o.view(torch.int64), v.view(torch.int64))
    g.check(f"{name}, raw entry")
