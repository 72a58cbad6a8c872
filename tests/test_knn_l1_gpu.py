"""mmvae_knn_search_l1 on the MI355X through ops.knn_search_l1: the returned distances are bit-equal to the sequential float32 chain
the header specifies (tests/knn_l1_bounds.py: emulate), the indices its (key, index) ranking, every answer valid under the derived
bounds, the tie rule, the prefix property the grid search rests on and run-to-run results exact.  Operands are views of wider
NaN-filled buffers or padded bf16 rows with NaN pads, the outputs lie in sentinel-filled wider buffers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import knn_bounds as KB  # noqa: E402
import knn_l1_bounds as LB  # noqa: E402
import knn_ref as KR  # noqa: E402
from mmvae import _lib, ops  # noqa: E402
from rowmat_gpu_util import in_nan_frame, operand  # noqa: E402

DEV = "cuda"
SENTINEL_I, SENTINEL_F = -77, -7.0


def launch(q, t, k):
    Mq = q.shape[0]
    ibuf = torch.full((Mq + 2, k + 3), SENTINEL_I, dtype=torch.int32, device=DEV)
    dbuf = torch.full((Mq + 2, k + 5), SENTINEL_F, dtype=torch.float32, device=DEV)
    idx, d = ops.knn_search_l1(q, t, k, idx_out=ibuf[1:Mq + 1, 2:2 + k], dist_out=dbuf[1:Mq + 1, 1:1 + k])
    torch.cuda.synchronize()
    iframe, dframe = ibuf.clone(), dbuf.clone()
    iframe[1:Mq + 1, 2:2 + k] = SENTINEL_I
    dframe[1:Mq + 1, 1:1 + k] = SENTINEL_F
    assert (iframe == SENTINEL_I).all() and (dframe == SENTINEL_F).all(), "a write outside idx / dist"
    return idx.cpu().numpy().astype(np.int64), d.cpu().numpy()


def _data(seed, Mq, Nt, F, bf16=False):
    g = np.random.default_rng(seed)
    q, t = np.abs(g.standard_normal((Mq, F))).astype(np.float32), np.abs(g.standard_normal((Nt, F))).astype(np.float32)
    return (KR.to_bf16(q), KR.to_bf16(t)) if bf16 else (q, t)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (q, t, bf16): the inputs, shared by the tests that use them"""
    if name in ("p77_f32", "p77_bf16"):
        return (*_data(31, 77, 77, 37, name.endswith("bf16")), name.endswith("bf16"))
    if name == "t1000":
        return (*_data(32, 200, 1000, 45), False)
    if name == "split":
        return (*_data(33, 3, 5000, 20), False)
    if name.startswith("f"):                                 # F = 1, 32, 33: below, equal to and one past the chunk
        return (*_data(34, 70, 300, int(name[1:])), False)
    return {"nt_eq_k": (*_data(35, 10, 5, 7), False), "nt1": (*_data(36, 4, 1, 3), False), "mq1": (*_data(37, 1, 300, 33), False)}[name]


def run_case(name, k, left=7):
    q, t, bf16 = case(name)
    idx, d = launch(operand(q, bf16, left), operand(t, bf16, left), k)
    eidx, ed = LB.emulate(q, t, k)
    assert np.array_equal(d.view(np.uint32), ed.view(np.uint32)), (name, k, "distances differ from the sequential float32 chain")
    assert np.array_equal(idx, eidx), (name, k, "indices differ from the (key, index) ranking")
    an = KB.check_search(q, t, k, idx, None, label=f"{name} k={k}", an=LB.analyse(q, t, k))
    LB.check_dist(an, idx, d, label=name)
    return idx, d


@pytest.mark.parametrize("left", [7, 8])            # 7: rows aligned to one element (scalar loads); 8: 16-byte loads
@pytest.mark.parametrize("name", ["p77_f32", "p77_bf16"])
def test_partial_block_partial_tile_odd_width(name, left):
    run_case(name, 5, left)


@pytest.mark.parametrize("k", [1, 5, 50, 96])
def test_several_tiles_per_row_block(k):
    run_case("t1000", k)


def test_split_and_merge_path():
    ns, rps = ops.knn_splits(3, 5000)
    assert ns > 1 and rps < 5000, "this shape must split the training rows"
    assert ops.knn_l1_work_bytes(3, 5000, 6) == 8 * 3 * ns * 6
    run_case("split", 6)


@pytest.mark.parametrize("name", ["nt_eq_k", "nt1", "mq1", "f1", "f32", "f33"])
def test_boundary_sizes(name):
    idx, _ = run_case(name, {"nt_eq_k": 5, "nt1": 1}.get(name, 5))
    if name == "nt_eq_k":
        assert (np.sort(idx, axis=1) == np.arange(5)).all()


@pytest.mark.parametrize("Nt", [333, 5000])         # 5000 rows for 3 queries: rows 5 and 200 are in different splits
def test_duplicates_tie_bit_for_bit_and_the_smaller_index_wins(Nt):
    q, t = KR.duplicates_case(Nt)
    if Nt == 5000:
        ns, rps = ops.knn_splits(3, Nt)
        assert ns > 1 and 5 // rps != 200 // rps
    qd, td = in_nan_frame(q, 1, 7, 2), in_nan_frame(t, 1, 7, 2)
    assert launch(qd, td, 1)[0][0].tolist() == [5]
    idx2, d = launch(qd, td, 2)
    assert idx2[0].tolist() == [5, 200] and d[0, 0] == d[0, 1] == 0.0
    q[0, 3] += 0.25                                  # no longer equal to them: the two keys must still be the same bits
    idx2, d = launch(in_nan_frame(q, 1, 7, 2), td, 2)
    assert idx2[0].tolist() == [5, 200] and d[0, 0] == d[0, 1] > 0.0


@pytest.mark.parametrize("k", [5, 10, 20])
def test_prefix_of_the_k50_search_is_the_k_search(k):
    q, t, _ = case("t1000")
    qd, td = torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)
    i50, d50 = ops.knn_search_l1(qd, td, 50)
    ik, dk = ops.knn_search_l1(qd, td, k)
    assert torch.equal(i50[:, :k], ik) and torch.equal(d50[:, :k].view(torch.int32), dk.view(torch.int32))


def test_prefix_property_of_the_euclidean_search():
    q, t, _ = case("t1000")
    qd, td = torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)
    shift = td.mean(dim=0)
    i50, d50 = ops.knn_search(qd, td, 50, shift)
    for k in (5, 10, 20):
        ik, dk = ops.knn_search(qd, td, k, shift)
        assert torch.equal(i50[:, :k], ik) and torch.equal(d50[:, :k].view(torch.int32), dk.view(torch.int32))


def test_nan_rows_never_beat_finite_ones():
    q, t, _ = case("t1000")
    t = t.copy()
    t[[3, 130, 999]] = np.nan
    idx, d = launch(in_nan_frame(q, 2, 7, 3), in_nan_frame(t, 2, 7, 3), 5)
    assert not np.isin(idx, [3, 130, 999]).any() and np.isfinite(d).all()
    assert np.array_equal(idx, LB.emulate(q, t, 5)[0])


@pytest.mark.parametrize("name,k", [("t1000", 50), ("split", 6)])
def test_run_to_run_bit_identical(name, k):
    q, t, _ = case(name)
    qd, td = torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)
    a, b = ops.knn_search_l1(qd, td, k), ops.knn_search_l1(qd, td, k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_a_shift_and_a_cpu_tensor_are_refused():
    q, t = torch.zeros(4, 8), torch.zeros(9, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_search_l1(q, t, 2)
    qd, td = q.to(DEV), t.to(DEV)
    idx = torch.full((4, 2), SENTINEL_I, dtype=torch.int32, device=DEV)
    shift = torch.zeros(8, device=DEV)
    a = _lib.KnnArgs(qd.data_ptr(), td.data_ptr(), shift.data_ptr(), idx.data_ptr(), None, None, 8, 8, 2, 0, 0, 4, 9, 8, 2, 0, 0)
    assert _lib.load().mmvae_knn_search_l1(C.byref(a), None) == -1
    torch.cuda.synchronize()
    assert (idx == SENTINEL_I).all()
    for bad in (lambda: ops.knn_search_l1(qd, td, 10), lambda: ops.knn_search_l1(qd, td, 0), lambda: ops.knn_search_l1(qd, td[:, :7], 2)):
        with pytest.raises(ValueError):
            bad()
