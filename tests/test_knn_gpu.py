"""mmvae_knn_search / mmvae_knn_mean_rows on the MI355X through ops and mmvae.knn: every returned neighbour set must be valid under
the derived bounds of tests/knn_bounds.py (every decided query equal to the float64 set of tests/knn_ref.py), dist2 and the regression
rows within their bounds, the tie rule and run-to-run results exact.  Operands are views of wider NaN-filled buffers or padded bf16 rows
with NaN pads, the outputs are pre-filled with a sentinel inside wider buffers."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import knn_bounds as KB  # noqa: E402
import knn_ref as KR  # noqa: E402
from mmvae import ops  # noqa: E402
from mmvae.knn import ConditionedKNeighborsRegressor, KNeighborsRegressor, neighborhood_hit  # noqa: E402
from rowmat_gpu_util import in_nan_frame, operand  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_baselines.npz")
SENTINEL_I, SENTINEL_F = -77, -7.0


def f64(t):
    return t.detach().double().cpu().numpy()


def launch(q, t, k, shift=None):
    """one search into sentinel-filled, wider output buffers; returns numpy (idx, dist2) and asserts the frame is untouched"""
    Mq = q.shape[0]
    ibuf = torch.full((Mq + 2, k + 3), SENTINEL_I, dtype=torch.int32, device=DEV)
    dbuf = torch.full((Mq + 2, k + 5), SENTINEL_F, dtype=torch.float32, device=DEV)
    idx, d2 = ops.knn_search(q, t, k, shift, idx_out=ibuf[1:Mq + 1, 2:2 + k], dist2_out=dbuf[1:Mq + 1, 1:1 + k])
    torch.cuda.synchronize()
    iframe, dframe = ibuf.clone(), dbuf.clone()
    iframe[1:Mq + 1, 2:2 + k] = SENTINEL_I
    dframe[1:Mq + 1, 1:1 + k] = SENTINEL_F
    assert (iframe == SENTINEL_I).all() and (dframe == SENTINEL_F).all(), "a write outside idx / dist2"
    return idx.cpu().numpy().astype(np.int64), d2.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    c = KR.make_case(name)
    return c, KB.analyse(c["q"], c["t"], c["k"], c["shift"])


def run_case(name, left=7):
    c, an = case(name)
    q, t = operand(c["q"], c["bf16"], left), operand(c["t"], c["bf16"], left)
    assert np.array_equal(f64(q), c["q"].astype(np.float64)) and np.array_equal(f64(t), c["t"].astype(np.float64))
    shift = None if c["shift"] is None else torch.from_numpy(c["shift"]).to(DEV)
    idx, d2 = launch(q, t, c["k"], shift)
    out = KB.check_search(c["q"], c["t"], c["k"], idx, d2, c["shift"], label=name, an=dict(an))
    print(f"{name} left {left}: {out['undecided']} of {len(idx)} queries undecided, all valid")
    assert out["undecided"] <= 0.05 * len(idx)
    return idx, d2


@pytest.mark.parametrize("left", [7, 8])            # 7: rows aligned to 4 bytes only (scalar loads); 8 with ld % 64 == 0: 16-byte loads
@pytest.mark.parametrize("name", ["p77_f32", "p77_bf16"])
def test_partial_block_partial_tile_odd_width(name, left):
    run_case(name, left)


@pytest.mark.parametrize("name", ["t1000_k1", "t1000_k5", "t1000_k50"])
def test_several_tiles_per_row_block(name):
    run_case(name)


def test_split_and_merge_path():
    c, _ = case("split")
    ns, rps = ops.knn_splits(c["q"].shape[0], c["t"].shape[0])
    assert ns > 1 and rps < c["t"].shape[0], "this shape must split the training rows"
    assert ops.knn_work_bytes(3, 5000, c["k"]) > 4 * 5003 + 8
    run_case("split")


@pytest.mark.parametrize("name", ["nt_eq_k", "nt1", "mq1"])
def test_boundary_sizes(name):
    idx, _ = run_case(name)
    if name == "nt_eq_k":
        assert (np.sort(idx, axis=1) == np.arange(5)).all()
    if name == "nt1":
        assert (idx == 0).all()


@pytest.mark.parametrize("Nt", [333, 5000])         # 5000 rows for 3 queries: rows 5 and 200 are in different splits
def test_duplicates_tie_bit_for_bit_and_the_smaller_index_wins(Nt):
    q, t = KR.duplicates_case(Nt)
    if Nt == 5000:
        ns, rps = ops.knn_splits(3, Nt)
        assert ns > 1 and 5 // rps != 200 // rps
    qd, td = in_nan_frame(q, 1, 7, 2), in_nan_frame(t, 1, 7, 2)
    idx1, _ = launch(qd, td, 1)
    assert idx1[0].tolist() == [5]
    idx2, d2 = launch(qd, td, 2)
    assert idx2[0].tolist() == [5, 200] and d2[0, 0] == d2[0, 1]
    KB.check_search(q, t, 2, idx2, d2, label=f"duplicates {Nt}")


def test_ill_conditioned_with_and_without_shift():
    run_case("ill_shift")
    # without the shift the same inputs only have to satisfy their (much wider) bounds: nothing is asserted to match
    c, an = case("ill_noshift")
    idx, d2 = launch(in_nan_frame(c["q"], 2, 7, 3), in_nan_frame(c["t"], 2, 7, 3), c["k"], None)
    out = KB.check_search(c["q"], c["t"], c["k"], idx, d2, None, label="ill_noshift", an=dict(an))
    print(f"ill_noshift: {out['undecided']} of {len(idx)} queries undecided under the widened bounds")


@pytest.mark.parametrize("name", ["t1000_k50", "split"])
def test_run_to_run_bit_identical(name):
    c, _ = case(name)
    q, t = torch.from_numpy(c["q"]).to(DEV), torch.from_numpy(c["t"]).to(DEV)
    a = ops.knn_search(q, t, c["k"])
    b = ops.knn_search(q, t, c["k"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_nan_rows_never_beat_finite_ones():
    c, _ = case("p77_f32")
    t = c["t"].copy()
    t[[3, 130, 332]] = np.nan
    idx, _ = launch(in_nan_frame(c["q"], 2, 7, 3), in_nan_frame(t, 2, 7, 3), 5)
    assert not np.isin(idx, [3, 130, 332]).any()
    keep = np.setdiff1d(np.arange(333), [3, 130, 332])
    KB.check_search(c["q"], t[keep], 5, np.searchsorted(keep, idx), label="nan rows")


@pytest.mark.parametrize("bf16", [False, True])
def test_mean_rows_against_the_float64_mean_over_the_returned_indices(bf16):
    g = np.random.default_rng(21)
    y = g.standard_normal((333, 45)).astype(np.float32)
    y = KR.to_bf16(y) if bf16 else y
    yd = operand(y, bf16, 7)
    for k in (1, 5, 50):
        idx = g.integers(0, 333, (77, k)).astype(np.int32)
        idx[0, 0], idx[1, 0] = -3, 400                                                  # clamped to rows 0 and 332
        ibuf = torch.full((77, k + 3), SENTINEL_I, dtype=torch.int32, device=DEV)
        ibuf[:, 1:1 + k] = torch.from_numpy(idx).to(DEV)
        obuf = torch.full((79, 50), SENTINEL_F, dtype=torch.float32, device=DEV)
        out = ops.knn_mean_rows(ibuf[:, 1:1 + k], yd, obuf[1:78, 2:47])
        torch.cuda.synchronize()
        clamped = np.clip(idx, 0, 332)
        err = np.abs(out.double().cpu().numpy() - KR.mean_rows(clamped, y))
        assert (err <= KB.mean_rows_tol(clamped, y)).all(), (k, err.max())
        frame = obuf.clone()
        frame[1:78, 2:47] = SENTINEL_F
        assert (frame == SENTINEL_F).all()


def test_operand_checks_and_no_cpu_fallback():
    q, t = torch.zeros(4, 8), torch.zeros(9, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_search(q, t, 2)
    qd, td = q.to(DEV), t.to(DEV)
    for bad in (lambda: ops.knn_search(qd, td, 10), lambda: ops.knn_search(qd, td, 0), lambda: ops.knn_search(qd.double(), td, 2),
                lambda: ops.knn_search(qd, td[:, :7], 2), lambda: ops.knn_search(qd.t().contiguous().t(), td, 2),
                lambda: KNeighborsRegressor(5, weights="distance"), lambda: ConditionedKNeighborsRegressor(5, metric="cosine")):
        with pytest.raises((ValueError, TypeError)):
            bad()


# ---------------------------------------------------------------------------------------------------------------------------
# regressors and neighbourhood hit against knn_ref and the records of the reference's own code
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _pred_tol(X, Y, Xq, k):
    """bound on a regression row given that the kernel's neighbour set is the float64 one (asserted by the caller)"""
    idx = KR.search(Xq, X, k)[0]
    return KB.mean_rows_tol(idx, Y)


def test_kneighbors_regressor_against_the_reference_records():
    f = fixture()
    reg = KNeighborsRegressor(5).fit(_dev(f["X"]), _dev(f["Y"]))
    idx, _ = reg.kneighbors(_dev(f["Xq"]))
    an = KB.check_search(f["Xq"], f["X"], 5, idx.cpu().numpy(), shift=f64(reg.shift).astype(np.float32), label="fixture")
    assert an["decided"].all()
    tol = _pred_tol(f["X"], f["Y"], f["Xq"], 5)
    for bs in (None, 16):
        pred = reg.predict(_dev(f["Xq"]), batch_size=bs).double().cpu().numpy()
        assert (np.abs(pred - KR.knn_regress(f["X"], f["Y"], f["Xq"], 5)) <= tol).all()
        assert (np.abs(pred - f["knn_pred"]) <= tol + 1e-14).all()


def test_conditioned_regressor_against_the_reference_records():
    f = fixture()
    reg = ConditionedKNeighborsRegressor(5).fit(_dev(f["X"]), _dev(f["Y"]), _dev(f["site"]))
    pred = reg.predict(_dev(f["Xq"]), _dev(f["site_q"])).double().cpu().numpy()
    ref = KR.conditioned_regress(f["X"], f["Y"], f["site"], f["Xq"], f["site_q"], 5)
    tol = np.zeros_like(ref)
    for s in np.unique(f["site_q"]):
        m = f["site"] == s
        if m.any():
            tol[f["site_q"] == s] = _pred_tol(f["X"][m], f["Y"][m], f["Xq"][f["site_q"] == s], min(5, int(m.sum())))
    assert (pred[f["site_q"] == 6] == 0).all()                                          # a site without training rows: zero rows
    assert (f["site"] == 4).sum() == 3 and (f["site_q"] == 4).any()                     # a site with fewer than k training rows
    assert (np.abs(pred - ref) <= tol).all() and (np.abs(pred - f["cond_pred"]) <= tol + 1e-14).all()


def test_neighborhood_hit_against_the_reference_records():
    f = fixture()
    an = KB.analyse(f["feats"], f["feats"], 6, f["feats"].astype(np.float64).mean(axis=0).astype(np.float32))
    assert an["decided"].all()                                                          # then the hit is a count of exact sets
    got = neighborhood_hit(_dev(f["feats"]), _dev(f["labels"]), k=5)
    assert got == pytest.approx(KR.neighborhood_hit(f["feats"], f["labels"], 5), abs=1e-12)
    assert got == pytest.approx(float(f["nh_k5"]), abs=1e-12)
    assert neighborhood_hit(_dev(f["feats"][:5]), _dev(f["labels"][:5]), k=5) == 0.0
