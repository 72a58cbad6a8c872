"""mmvae_recon_metrics on the MI355X through ops.recon_metrics and mmvae.metrics.ImputationMetrics: every output element against the
float64 restatement (tests/metrics_ref.py) within the derived bounds (tests/metrics_bounds.py), NaN positions exactly.  Operands are
views of wider NaN-filled buffers (or padded bf16 rows with NaN pads), so a read outside the logical matrix shows in the sums."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_bounds as MB  # noqa: E402
import metrics_ref as MR  # noqa: E402
from mmvae import _lib, ops, to_bf16_rows  # noqa: E402
from mmvae.metrics import ImputationMetrics, imputation_metrics  # noqa: E402
from rowmat_gpu_util import bf16_rows_nan_pads, in_nan_frame  # noqa: E402

DEV = "cuda"


def make(M, F, seed, specials=True):
    """float32 (y, p): target |N(0, 1)|, prediction = target + 0.3 N(0, 1); with room, a constant target row and a zero prediction row"""
    g = np.random.default_rng(seed)
    y = np.abs(g.standard_normal((M, F))).astype(np.float32)
    p = (y + 0.3 * g.standard_normal((M, F))).astype(np.float32)
    if specials and M > 4:
        y[1] = 0.5
        p[M - 2] = 0.0
    return y, p


def f64(t):
    """the values the kernel reads, exactly, as float64 numpy"""
    return t.detach().double().cpu().numpy()


def launch(pred, target, shift=None, prior=None):
    M, F = target.shape
    col = torch.zeros(4, F, dtype=torch.float64, device=DEV) if prior is None else torch.from_numpy(prior).to(DEV)
    rp = torch.full((M,), 7.0, dtype=torch.float32, device=DEV)
    rc = torch.full((M,), 7.0, dtype=torch.float32, device=DEV)
    ops.recon_metrics(pred, target, shift, col, rp, rc)
    torch.cuda.synchronize()
    return col.cpu().numpy(), rp.double().cpu().numpy(), rc.double().cpu().numpy()


def check(pred, target, shift=None, prior=None, label=""):
    """one launch, all outputs against the reference on the values the kernel read; returns the outputs"""
    y, p = f64(target), f64(pred)
    c = None if shift is None else f64(shift)
    col, rp, rc = launch(pred, target, shift, prior)
    ref_col = MR.col_sums(y, p, c) + (0.0 if prior is None else prior)
    tol_col = MB.col_tol(y, p, c, prior)
    err = np.abs(col - ref_col)
    print(f"{label} col_acc: max err / bound {np.max(err / np.maximum(tol_col, 1e-300)):.3f}")
    assert np.isfinite(col).all() and (err <= tol_col).all(), (label, np.argwhere(~(err <= tol_col))[:5])
    ref_r, tol_r = MR.row_pearson(y, p), MB.pearson_tol(y, p)
    assert np.isfinite(tol_r).all()
    assert np.array_equal(np.isnan(rp), np.isnan(ref_r)), (label, np.flatnonzero(np.isnan(rp) != np.isnan(ref_r))[:5])
    ok = ~np.isnan(ref_r)
    if ok.any():
        print(f"{label} pearson: max err {np.abs(rp - ref_r)[ok].max():.3e}, smallest bound {tol_r[ok].min():.3e}")
    assert (np.abs(rp - ref_r)[ok] <= tol_r[ok]).all(), label
    ref_c, tol_c = MR.row_cosine(y, p), MB.cosine_tol(y, p)
    assert not np.isnan(rc).any() and (np.abs(rc - ref_c) <= tol_c).all(), label
    return col, rp, rc


# ---------------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("left", [7, 8])          # 7: rows aligned to 4 bytes only (scalar loads); 8 with ld 64: 16-byte loads
def test_edge_case_as_views_of_nan_filled_buffers(left):
    y, p = MR.edge_case()
    target = in_nan_frame(y, 1, left, 64 - 45 - left)
    pred = in_nan_frame(p, 2, left, 64 - 45 - left)
    shift = torch.from_numpy(y[0].copy()).to(DEV)
    _, rp, rc = check(pred, target, shift, label=f"edge[{left}]")
    assert sorted(np.flatnonzero(np.isnan(rp))) == [3, 5, 7, 9]
    assert rc[7] == 0 and rc[9] == 0
    check(pred, target, None, label=f"edge[{left}], no shift")


@pytest.mark.parametrize("shape", [(1, 1), (3, 2)])
def test_tiny(shape):
    y, p = make(*shape, seed=11, specials=False)
    check(in_nan_frame(p, 1, 3, 2), in_nan_frame(y, 1, 1, 4), label=f"tiny{shape}")


@pytest.mark.parametrize("pred_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("target_kind", ["fp32", "bf16_rows"])
@pytest.mark.parametrize("shape", [(130, 782), (64, 572)])
def test_real_widths(shape, target_kind, pred_dtype):
    y, p = make(*shape, seed=shape[1])
    target = in_nan_frame(y, 1, 0, 3) if target_kind == "fp32" else bf16_rows_nan_pads(y)
    pred = in_nan_frame(p, 1, 0, 5, dtype=pred_dtype)
    if target_kind == "bf16_rows":
        assert target.stride(0) == (784 if shape[1] == 782 else 576)
    check(pred, target, label=f"{shape} {target_kind} {pred_dtype}")


def test_bf16_rows_prediction_and_target():
    y, p = make(64, 572, seed=3)
    check(bf16_rows_nan_pads(p), bf16_rows_nan_pads(y), label="bf16 rows both")


def test_long_row_with_a_scalar_tail():
    y, p = make(5, 4099, seed=5)
    check(in_nan_frame(p, 1, 4, 1), in_nan_frame(y, 1, 4, 1), label="5x4099 (16-byte loads)")
    check(in_nan_frame(p, 1, 1, 0), in_nan_frame(y, 1, 2, 1), label="5x4099 (scalar loads)")


def test_many_rows_and_several_workgroups_per_column():
    y, p = make(2051, 24, seed=6)
    check(in_nan_frame(p, 1, 0, 0), in_nan_frame(y, 1, 0, 8), label="2051x24")


@pytest.mark.parametrize("shape,rpb", [((9001, 24), 12), ((131203, 5), 128)])
def test_several_rows_per_wave(shape, rpb):
    """The launcher gives a workgroup clamp(roundup4(ceil(M / 1024)), 4, 128) rows: every shape above has 4, one row per wave.  9001
    rows: 12 per workgroup (three per wave, column partials carried over rows, row slots and finalising threads beyond 3) and ONE row in
    the last workgroup; 131 203 rows: the clamp at 128 = the LDS row slots, 32 rows per wave, a ragged last workgroup of 3."""
    M = shape[0]
    assert min(max((-(-M // 1024) + 3) // 4 * 4, 4), 128) == rpb and M % rpb in (1, 3)
    y, p = make(*shape, seed=M)
    y[M - 1] = 0.25                                            # a constant row in the ragged last workgroup
    shift = torch.from_numpy(y[0].copy()).to(DEV)
    _, rp, _ = check(in_nan_frame(p, 1, 0, 3), in_nan_frame(y, 1, 0, 0), shift, label=f"{shape}")
    assert np.isnan(rp[M - 1]) and np.isnan(rp[1]) and np.isnan(rp[M - 2]) and np.isnan(rp).sum() == 3


def test_broadcast_prediction():
    y, _ = make(130, 782, seed=7)
    target = in_nan_frame(y, 1, 0, 2)
    mean = torch.from_numpy(y.mean(axis=0)).to(DEV)
    _, rp, _ = check(mean, target, label="broadcast mean")
    assert np.isnan(rp[1]) and not np.isnan(rp[0])
    _, rp, _ = check(torch.full((782,), 0.25, device=DEV), target, label="broadcast constant")
    assert np.isnan(rp).all()                                  # scipy on the row: a constant prediction row gives NaN
    check(mean.to(torch.bfloat16), bf16_rows_nan_pads(y), label="broadcast bf16")


def test_column_shift_keeps_a_near_constant_column_inside_its_bound():
    g = np.random.default_rng(8)
    y, p = make(300, 40, seed=8)
    y[:, 17] = 1000.0 + 1e-3 * g.standard_normal(300)
    p[:, 17] = y[:, 17] + 1e-4 * g.standard_normal(300)
    shift = torch.from_numpy(y[0].copy()).to(DEV)
    col, _, _ = check(torch.from_numpy(p).to(DEV), torch.from_numpy(y).to(DEV), shift, label="shifted column")
    tol = MB.col_tol(y.astype(np.float64), p.astype(np.float64), y[0].astype(np.float64))
    assert tol[1, 17] < 1e-15                                  # sum t^2 ~ 3e-4: the shifted moment carries 15 digits of the spread
    ss_tot = col[1, 17] - col[0, 17] ** 2 / 300
    want = ((y[:, 17].astype(np.float64) - y[:, 17].astype(np.float64).mean()) ** 2).sum()
    # S1 - S0^2 / rows from sums within their bounds; the square, the division and the subtraction: 4 F64 of the terms
    bound = tol[1, 17] + (2 * abs(col[0, 17]) + tol[0, 17]) * tol[0, 17] / 300 + 4 * MB.F64 * (col[1, 17] + col[0, 17] ** 2 / 300)
    assert bound < 1e-12 * want and abs(ss_tot - want) <= bound + 4 * 300 * MB.F64 * want      # `want` is a float64 sum itself


def test_col_acc_is_accumulated_into():
    y, p = make(67, 45, seed=9)
    prior = np.random.default_rng(9).standard_normal((4, 45)) * 100.0
    col, _, _ = check(torch.from_numpy(p).to(DEV), torch.from_numpy(y).to(DEV), None, prior=prior.copy(), label="prior")
    assert (np.abs(col - prior) > 1e-3).any()


def test_wrapper_refuses_before_launch():
    y, p = make(8, 6, seed=10, specials=False)
    t, q = torch.from_numpy(y).to(DEV), torch.from_numpy(p).to(DEV)
    col = torch.zeros(4, 6, dtype=torch.float64, device=DEV)
    rp, rc = torch.empty(8, device=DEV), torch.empty(8, device=DEV)
    with pytest.raises(ValueError):
        ops.recon_metrics(q[:, :5], t, None, col, rp, rc)
    with pytest.raises(ValueError):
        ops.recon_metrics(q, t, None, col.float(), rp, rc)
    with pytest.raises(ValueError):
        ops.recon_metrics(q, t, None, col, rp[:7], rc)
    with pytest.raises(ValueError):
        ops.recon_metrics(q.t().contiguous().t(), t, None, col, rp, rc)            # inner stride != 1
    with pytest.raises(ValueError):
        ops.recon_metrics(q, t.cpu(), None, col, rp, rc)
    with pytest.raises(TypeError):
        ops.recon_metrics(q.half(), t, None, col, rp, rc)
    a = _lib.MetricsArgs(8, 6, q.data_ptr(), _lib.F32, 5, t.data_ptr(), _lib.F32, 6, None, col.data_ptr(), rp.data_ptr(), rc.data_ptr())
    assert _lib.load().mmvae_recon_metrics(C.byref(a), None) == -1                 # ld_pred < N
    torch.cuda.synchronize()
    assert (col == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# ImputationMetrics
# ---------------------------------------------------------------------------------------------------------------------------
SCALARS = ("MAE", "MSE", "RMSE", "R2", "MeanR2", "CosineSimilarity", "PearsonMean", "PearsonStd")


def check_dict(got, y, p, label):
    want, tol = MR.metrics(y, p), MB.metrics_tol(y, p, y[0])
    assert set(got) == set(MR.KEYS)
    for k in SCALARS:
        print(f"{label} {k}: {got[k]!r} want {want[k]!r} bound {tol[k]:.3e}")
        assert np.isfinite(tol[k]) and abs(got[k] - want[k]) <= tol[k], (label, k, got[k], want[k], tol[k])
    assert got["PearsonValid"] == want["PearsonValid"]
    r = got["_pearson_all"].double().cpu().numpy()
    assert np.array_equal(np.isnan(r), np.isnan(want["_pearson_all"]))


def test_imputation_metrics_on_the_edge_case():
    y, p = MR.edge_case()
    got = imputation_metrics(torch.from_numpy(y).to(DEV), torch.from_numpy(p).to(DEV))
    check_dict(got, y.astype(np.float64), p.astype(np.float64), "one shot")
    assert got["PearsonValid"] == 63


def test_two_updates_equal_one():
    y, p = MR.edge_case()
    ty, tp = torch.from_numpy(y).to(DEV), torch.from_numpy(p).to(DEV)
    m = ImputationMetrics(45, DEV)
    m.update(ty[:40], tp[:40]).update(ty[40:], tp[40:])
    assert m.rows == 67 and [t.shape[0] for t in m._pearson] == [40, 27]
    second = m._pearson[1].double().cpu().numpy()                    # the second call's rows start at ITS row 0
    ref2, tol2 = MR.row_pearson(y[40:], p[40:]), MB.pearson_tol(y[40:], p[40:])
    assert not np.isnan(ref2).any() and (np.abs(second - ref2) <= tol2).all()
    col = m.col_acc.cpu().numpy()
    c = y[0].astype(np.float64)
    assert (np.abs(col - MR.col_sums(y, p, c)) <= MB.col_tol(y, p, c)).all()
    check_dict(m.compute(), y.astype(np.float64), p.astype(np.float64), "40 + 27")


def test_broadcast_and_bf16_through_the_class():
    y, _ = make(130, 572, seed=12)
    ty = to_bf16_rows(torch.from_numpy(y).to(DEV))
    mean = ty.float().mean(dim=0)
    got = imputation_metrics(ty, mean)
    check_dict(got, f64(ty), f64(mean), "bf16 target, broadcast mean")
    assert got["PearsonValid"] == 129


def test_cpu_tensors_raise():
    y, p = make(4, 3, seed=13, specials=False)
    with pytest.raises(RuntimeError):
        imputation_metrics(torch.from_numpy(y), torch.from_numpy(p))
    with pytest.raises(RuntimeError):
        ImputationMetrics(3, "cpu")
    with pytest.raises(RuntimeError):
        ImputationMetrics(3, DEV).update(torch.from_numpy(y).to(DEV), torch.from_numpy(p))
