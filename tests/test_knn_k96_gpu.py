"""mmvae_knn_search beyond k = 64 (MMVAE_KNN_MAXK = 96: the 92 of t-SNE at perplexity 30) on the MI355X, checked as tests/test_knn_gpu.py
checks k <= 64: every returned neighbour set valid under the derived bounds of tests/knn_bounds.py against the float64 sets of
tests/knn_ref.py, dist2 within its bound, ties to the smaller index, run-to-run results exact."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import knn_bounds as KB  # noqa: E402
import knn_ref as KR  # noqa: E402
from mmvae import _lib, ops  # noqa: E402
from rowmat_gpu_util import operand  # noqa: E402

DEV = "cuda"
SENTINEL_I, SENTINEL_F = -77, -7.0
# name -> (Mq, Nt, F, self-search); the two larger ones walk several training tiles and split them across workgroups
SHAPES = {"1x96": (1, 96, 7, False), "97x97": (97, 97, 13, True), "130x700x50": (130, 700, 50, False), "333x1000x77": (333, 1000, 77, False)}


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
def rows(shape, bf16):
    Mq, Nt, F, same = SHAPES[shape]
    g = np.random.default_rng(Mq + Nt)
    t = np.abs(g.standard_normal((Nt, F))).astype(np.float32)
    q = t if same else np.abs(g.standard_normal((Mq, F))).astype(np.float32)
    if bf16:
        q, t = KR.to_bf16(q), KR.to_bf16(t)
    shift = t.astype(np.float64).mean(axis=0).astype(np.float32)
    return q, t, shift


@functools.lru_cache(maxsize=None)
def analysis(shape, bf16, k):
    q, t, shift = rows(shape, bf16)
    return KB.analyse(q, t, k, shift)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("k", [65, 91, 96])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_search_beyond_64(shape, k, bf16):
    q, t, shift = rows(shape, bf16)
    if shape in ("130x700x50", "333x1000x77"):
        ns, rps = ops.knn_splits(q.shape[0], t.shape[0])
        assert ns > 1 and rps < t.shape[0], "this shape must split the training rows"
    idx, d2 = launch(operand(q, bf16, 7), operand(t, bf16, 7), k, torch.from_numpy(shift).to(DEV))
    out = KB.check_search(q, t, k, idx, d2, shift, label=(shape, k, bf16), an=dict(analysis(shape, bf16, k)))
    print(f"{shape} k {k} bf16 {bf16}: {out['undecided']} of {len(idx)} queries undecided, all valid")
    assert out["undecided"] <= 0.05 * len(idx)
    if SHAPES[shape][3] and not out["undecided"]:
        assert (idx[:, 0] == np.arange(len(idx))).all()                              # a row is its own nearest neighbour


@pytest.mark.parametrize("k", [65, 96])
def test_duplicate_rows_tie_bit_for_bit_and_the_smaller_index_wins(k):
    q, t, shift = rows("130x700x50", False)
    t = t.copy()
    t[200] = t[5]
    t[699] = t[5]                                                                    # rows 5, 200 and 699 lie in different splits
    q = q.copy()
    q[0] = t[5]
    ns, rps = ops.knn_splits(q.shape[0], t.shape[0])
    assert 5 // rps != 200 // rps != 699 // rps
    idx, d2 = launch(operand(q, False, 7), operand(t, False, 7), k, torch.from_numpy(shift).to(DEV))
    assert idx[0, :3].tolist() == [5, 200, 699] and d2[0, 0] == d2[0, 1] == d2[0, 2]
    KB.check_search(q, t, k, idx, d2, shift, label=f"duplicates {k}")


@pytest.mark.parametrize("shape,k", [("97x97", 96), ("333x1000x77", 91), ("130x700x50", 65)])
def test_run_to_run_bit_identical(shape, k):
    q, t, _ = rows(shape, False)
    qd, td = torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)
    a = ops.knn_search(qd, td, k)
    b = ops.knn_search(qd, td, k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_the_limit_is_96():
    q = torch.zeros(4, 8, device=DEV)
    t = torch.zeros(200, 8, device=DEV)
    assert _lib.KNN_MAXK == 96
    assert ops.knn_search(q, t, 96)[0].shape == (4, 96)
    with pytest.raises(ValueError):
        ops.knn_search(q, t, 97)
    idx = torch.zeros(4, 96, dtype=torch.int32, device=DEV)
    assert ops.knn_mean_rows(idx, t).shape == (4, 8)
