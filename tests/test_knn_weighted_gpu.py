"""mmvae_knn_weighted_rows on the MI355X through ops.knn_weighted_rows: against the float64 weighted mean over the (idx, dist) the
kernel was given, within the derived bound of tests/knn_l1_bounds.py; sklearn's zero-distance rule exactly; NaN distances."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import knn_l1_bounds as LB  # noqa: E402
import knn_ref as KR  # noqa: E402
from mmvae import ops  # noqa: E402
from rowmat_gpu_util import operand  # noqa: E402

DEV = "cuda"
SENTINEL_I, SENTINEL_F = -77, -7.0
NY, MQ = 333, 77


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(idx, dist, y, yd, squared):
    """one launch from views of wider sentinel-filled idx / dist buffers into a view of a wider output buffer"""
    Mq, k = idx.shape
    Fy = y.shape[1]
    ibuf = torch.full((Mq, k + 3), SENTINEL_I, dtype=torch.int32, device=DEV)
    dbuf = torch.full((Mq, k + 2), float("nan"), dtype=torch.float32, device=DEV)
    ibuf[:, 1:1 + k], dbuf[:, 2:2 + k] = _dev(idx.astype(np.int32)), _dev(dist)
    obuf = torch.full((Mq + 2, Fy + 5), SENTINEL_F, dtype=torch.float32, device=DEV)
    out = ops.knn_weighted_rows(ibuf[:, 1:1 + k], dbuf[:, 2:2 + k], yd, squared, obuf[1:Mq + 1, 2:2 + Fy])
    torch.cuda.synchronize()
    frame = obuf.clone()
    frame[1:Mq + 1, 2:2 + Fy] = SENTINEL_F
    assert (frame == SENTINEL_F).all(), "a write outside out"
    return out.double().cpu().numpy()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("Fy", [1, 257])            # 257: two workgroups per row, the second with one column
def test_against_the_float64_weighted_mean_over_the_given_neighbours(Fy, squared, bf16):
    g = np.random.default_rng(41)
    y = g.standard_normal((NY, Fy)).astype(np.float32)
    y = KR.to_bf16(y) if bf16 else y
    yd = operand(y, bf16, 7)
    for k in (1, 5, 50):
        idx = g.integers(0, NY, (MQ, k))
        dist = np.sort(g.random((MQ, k)).astype(np.float32) * 4 + 0.01, axis=1)
        idx[0, 0], idx[1, 0] = -3, NY + 70                                               # clamped to rows 0 and NY - 1
        out = run(idx, dist, y, yd, squared)
        clamped = np.clip(idx, 0, NY - 1)
        err = np.abs(out - LB.weighted_rows(clamped, dist, y, squared))
        tol = LB.weighted_rows_tol(clamped, dist, y, squared)
        print(f"Fy {Fy} squared {squared} bf16 {bf16} k {k}: largest error / bound {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), (k, float((err / tol).max()))


@pytest.mark.parametrize("squared", [False, True])
def test_prefix_view_zero_distances_and_duplicates(squared):
    """a query equal to one training row gives exactly that y row, a query equal to two duplicates the mean of the two; the first 5
    columns of a k = 50 search are passed in place.  The distances are those of the manhattan search, whose zeros are exact (the
    euclidean search's GEMM form promises a zero only up to its bound); squared: their squares, read as a dist2."""
    g = np.random.default_rng(42)
    t = g.random((NY, 20), np.float32)
    q = g.random((MQ, 20), np.float32)
    t[200] = t[5]
    q[0], q[1] = t[5], t[17]
    y = g.standard_normal((NY, 9)).astype(np.float32)
    qd, td, yd = _dev(q), _dev(t), _dev(y)
    idx, dist = ops.knn_search_l1(qd, td, 50)
    if squared:
        dist = dist * dist
    assert idx[0, :2].tolist() == [5, 200] and idx[1, 0].item() == 17 and (dist[0, :2] == 0).all() and dist[1, 0] == 0 and dist[1, 1] > 0
    out = ops.knn_weighted_rows(idx[:, :5], dist[:, :5], yd, squared).cpu().numpy()
    assert np.array_equal(out[1], y[17])
    assert np.array_equal(out[0], (y[5] + y[200]) / np.float32(2))
    i5, d5 = idx[:, :5].cpu().numpy(), dist[:, :5].cpu().numpy()
    err = np.abs(out.astype(np.float64) - LB.weighted_rows(i5, d5, y, squared))
    assert (err <= LB.weighted_rows_tol(i5, d5, y, squared)).all()
    assert torch.equal(ops.knn_weighted_rows(idx[:, :5].contiguous(), dist[:, :5].contiguous(), yd, squared), torch.from_numpy(out).to(DEV))


def test_a_nan_or_negative_distance_gives_a_nan_row_and_no_error():
    g = np.random.default_rng(43)
    y = g.standard_normal((NY, 9)).astype(np.float32)
    idx = g.integers(0, NY, (4, 5))
    dist = np.sort(g.random((4, 5)).astype(np.float32) + 0.1, axis=1)
    dist[1, 2] = np.nan
    dist[2, 0] = -1.0
    dist[3, 0] = 0.0
    dist[3, 4] = np.nan                                                                  # a zero distance does not hide the NaN
    for squared in (False, True):
        out = run(idx, dist, y, _dev(y), squared)
        assert np.isfinite(out[0]).all() and np.isnan(out[1:]).all()


def test_operand_checks():
    yd = torch.zeros(9, 4, device=DEV)
    idx, dist = torch.zeros(3, 5, dtype=torch.int32, device=DEV), torch.ones(3, 5, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_weighted_rows(idx, dist, yd.cpu(), False)
    for bad in (lambda: ops.knn_weighted_rows(idx.long(), dist, yd, False), lambda: ops.knn_weighted_rows(idx, dist[:, :4], yd, False),
                lambda: ops.knn_weighted_rows(idx, dist.double(), yd, False), lambda: ops.knn_weighted_rows(idx, None, yd, False),
                lambda: ops.knn_weighted_rows(idx, dist, yd.double(), False)):
        with pytest.raises(ValueError):
            bad()
