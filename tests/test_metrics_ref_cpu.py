"""The numpy restatement of the imputation metrics (tests/metrics_ref.py) is what sklearn / scipy compute on float64 input, and the
derived bounds (tests/metrics_bounds.py) separate the kernel's arithmetic from the form it must not use."""
import os
import sys

import numpy as np
import pytest

import metrics_bounds as MB
import metrics_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "imputation_metrics.npz")
SCALARS = ("MAE", "MSE", "RMSE", "R2", "MeanR2", "CosineSimilarity", "PearsonMean", "PearsonStd")
NAN_ROWS = [3, 5]                      # constant target row 3, constant prediction row 5 ...
AGREE = 6e-16                          # the two float64 computations differ by their summation order only


def _check_against(want):
    y, p = MR.edge_case()
    got = MR.metrics(y, p)
    assert set(got) == set(MR.KEYS)
    for k in SCALARS:
        assert abs(got[k] - float(want[k])) <= AGREE * max(1.0, abs(float(want[k]))), (k, got[k], float(want[k]))
    assert got["PearsonValid"] == int(want["PearsonValid"])
    r, wr = got["_pearson_all"], np.asarray(want["_pearson_all"])
    assert np.array_equal(np.isnan(r), np.isnan(wr))
    ok = ~np.isnan(wr)
    assert np.abs(r[ok] - wr[ok]).max() <= AGREE
    assert np.abs(MR.row_cosine(y, p) - np.asarray(want["row_cosine"])).max() <= AGREE


def test_edge_case_has_the_rows_and_columns_it_promises():
    y, p = MR.edge_case()
    assert y.shape == p.shape == (67, 45) and y.dtype == p.dtype == np.float32
    assert (y[3] == 0.5).all() and (p[5] == 0.25).all() and (y[7] == 0).all() and (p[9] == 0).all()
    assert abs(y[20] - 1000).max() < 1e-2 and abs(p[20] - 1000).max() < 1e-2
    keep = np.ones(67, bool); keep[[3, 7, 20]] = False
    assert (y[keep, 11] == 0.75).all() and (y[keep, 13] == 0.125).all()
    r = MR.row_pearson(y, p)
    assert sorted(np.flatnonzero(np.isnan(r))) == [3, 5, 7, 9]           # a zero row is a constant row
    c = MR.row_cosine(y, p)
    assert c[7] == 0 and c[9] == 0 and np.isfinite(c).all()


def test_restatement_equals_the_stored_fixture():
    with np.load(GOLDEN) as z:
        y, p = MR.edge_case()
        assert np.array_equal(z["y"], y) and np.array_equal(z["p"], p)
        _check_against({k: z[k] for k in z.files})


def test_restatement_equals_sklearn_and_scipy_on_float64():
    pytest.importorskip("sklearn")
    pytest.importorskip("scipy")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from make_metrics_fixture import library_metrics
    finally:
        sys.path.pop(0)
    y, p = MR.edge_case()
    _check_against(library_metrics(y, p))


def test_force_finite_r2_rules():
    y = np.array([[1.0, 2.0], [1.0, 3.0], [1.0, 4.0]], np.float32)
    assert MR.metrics(y, y)["MeanR2"] == 1.0                               # column 0: SS_tot == 0 and SS_res == 0 -> 1
    p = y.copy(); p[0, 0] = 2.0
    assert MR.metrics(y, p)["MeanR2"] == 0.5 * (0.0 + 1.0)                 # column 0: SS_tot == 0, SS_res > 0 -> 0
    z = np.full((3, 2), 0.5, np.float32)
    m = MR.metrics(z, z)
    assert m["R2"] == 1.0 and m["PearsonValid"] == 0 and m["PearsonMean"] == 0.0 and m["PearsonStd"] == 0.0


def test_constant_non_dyadic_data_takes_the_force_finite_branch_exactly():
    """All targets 0.1f (its float64 mean over 7 x 3 elements rounds): flat and per-feature SS_tot are exactly 0 in the restatement
    and in mmvae.metrics.finalize_columns, so R2 is 0.0 with SS_res > 0 and 1.0 with SS_res == 0 -- never a huge negative number."""
    from mmvae.metrics import finalize_columns
    y = np.full((7, 3), 0.1, np.float32)
    p = y.copy(); p[2, 1] = 0.3
    for pred, want in ((p, 0.0), (y, 1.0)):
        ref = MR.metrics(y, pred)
        got = finalize_columns(MR.col_sums(y, pred, y[0]), y[0], 7)
        tol = MB.metrics_tol(y, pred, y[0])
        assert ref["R2"] == want and got["R2"] == want and tol["R2"] == 0.0
        assert tol["MeanR2"] < 1e-15 and abs(got["MeanR2"] - ref["MeanR2"]) <= tol["MeanR2"]
        assert abs(ref["MeanR2"] - (2.0 / 3.0 if want == 0.0 else 1.0)) < 1e-15       # columns 0 and 2: 1.0; column 1: 0.0 or 1.0


def test_shifted_form_in_any_order_stays_inside_the_bounds_and_raw_moments_do_not():
    """The kernel's arithmetic -- moments of the row shifted by its first element, float64 sums in an order of its own, an fp32
    store -- against the centred reference: inside the derived bound on every row.  Raw moments of the unshifted row leave it on
    row 20 (1000 +- 1e-3): the bound is not slack enough to hide that form."""
    y, p = MR.edge_case()
    ref = MR.row_pearson(y, p)
    tol = MB.pearson_tol(y, p)
    assert np.isfinite(tol).all()
    nan = np.isnan(ref)
    for seed in range(3):
        perm = np.random.default_rng(seed).permutation(y.shape[1])
        got = MR.row_pearson(y, p, form="shifted", perm=perm).astype(np.float32).astype(np.float64)
        assert np.array_equal(np.isnan(got), nan)
        assert (np.abs(got - ref)[~nan] <= tol[~nan]).all(), np.abs(got - ref)[~nan].max()
        cos = MR.row_cosine(y, p, perm=perm).astype(np.float32).astype(np.float64)
        assert (np.abs(cos - MR.row_cosine(y, p)) <= MB.cosine_tol(y, p)).all()
    raw = MR.row_pearson(y, p, form="raw").astype(np.float32).astype(np.float64)
    err = abs(raw[20] - ref[20])
    print(f"row 20: raw-moment error {err:.3e}, bound {tol[20]:.3e}")
    assert not err <= tol[20]                                              # a NaN from a negative variance counts as outside too
    keep = ~nan; keep[20] = False
    assert (np.abs(raw - ref)[keep] <= tol[keep]).all()                    # ... and only there: elsewhere the form is harmless


def test_column_sums_about_a_shift_reproduce_the_metrics_within_their_bounds():
    """mmvae.metrics.finalize_columns (host float64) on exact column sums, taken in two batches about the first target row, gives
    the reference's MAE / MSE / RMSE / R2 / MeanR2 within metrics_tol -- the constant columns 11 and 13 included (exact zeros)."""
    from mmvae.metrics import finalize_columns
    y, p = MR.edge_case()
    shift = y[0]
    acc = MR.col_sums(y[:40], p[:40], shift) + MR.col_sums(y[40:], p[40:], shift)
    assert (np.abs(acc - MR.col_sums(y, p, shift)) <= MB.col_tol(y, p, shift)).all()
    got, want, tol = finalize_columns(acc, shift, 67), MR.metrics(y, p), MB.metrics_tol(y, p, shift)
    for k in ("MAE", "MSE", "RMSE", "R2", "MeanR2"):
        assert np.isfinite(tol[k]) and tol[k] < 1e-9, (k, tol[k])
        assert abs(got[k] - want[k]) <= tol[k], (k, got[k], want[k], tol[k])


def test_near_constant_column_needs_the_shift():
    """A column of 1000 +- 1e-3 over 4096 rows: about its first element the per-feature SS_tot keeps a bound far below itself; about 0
    the bound says +inf (the sums cancel to 1e-6 of their terms)."""
    g = np.random.default_rng(5)
    y = (1000.0 + 1e-3 * g.standard_normal((4096, 3))).astype(np.float32)
    p = (y + 1e-4 * g.standard_normal(y.shape)).astype(np.float32)
    assert np.isfinite(MB.metrics_tol(y, p, y[0])["MeanR2"]) and MB.metrics_tol(y, p, y[0])["MeanR2"] < 1e-6
    assert not MB.metrics_tol(y, p, np.zeros(3, np.float32))["MeanR2"] < 1e-3
