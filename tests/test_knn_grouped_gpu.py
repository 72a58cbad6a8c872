"""mmvae_knn_search_grouped on the MI355X through ops.knn_search_grouped: for every query the indices and the distance bits equal the
plain search of the same metric (ops.knn_search / ops.knn_search_l1) over the candidates the predicate admits, mapped back, and the
tail of a list shorter than k is idx -1 / distance +inf.  Operands are views of wider NaN-filled buffers or padded bf16 rows with NaN
pads and the outputs lie in sentinel-filled wider buffers, as in tests/test_knn_l1_gpu.py."""
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
METRICS = ("euclidean", "manhattan")


def dev_codes(c):
    return None if c is None else torch.from_numpy(np.ascontiguousarray(c, np.int32)).to(DEV)


def pair(qc, tc):
    return None if qc is None else (dev_codes(qc), dev_codes(tc))


def launch(q, t, k, metric, same=None, differ=None, shift=None):
    """the grouped search into sentinel frames; same / differ: (q codes, t codes) numpy pairs"""
    Mq = q.shape[0]
    ibuf = torch.full((Mq + 2, k + 3), SENTINEL_I, dtype=torch.int32, device=DEV)
    dbuf = torch.full((Mq + 2, k + 5), SENTINEL_F, dtype=torch.float32, device=DEV)
    idx, d = ops.knn_search_grouped(q, t, k, same=None if same is None else pair(*same), differ=None if differ is None else pair(*differ),
                                    metric=metric, shift=shift, idx_out=ibuf[1:Mq + 1, 2:2 + k], dist_out=dbuf[1:Mq + 1, 1:1 + k])
    torch.cuda.synchronize()
    iframe, dframe = ibuf.clone(), dbuf.clone()
    iframe[1:Mq + 1, 2:2 + k] = SENTINEL_I
    dframe[1:Mq + 1, 1:1 + k] = SENTINEL_F
    assert (iframe == SENTINEL_I).all() and (dframe == SENTINEL_F).all(), "a write outside idx / dist"
    return idx.cpu().numpy().astype(np.int64), d.cpu().numpy()


def admitted(i_codes, same, differ, Nt):
    """mask (Nt,) of the candidates admitted for a query with the codes i_codes = (same code, differ code)"""
    m = np.ones(Nt, bool)
    if same is not None:
        m &= same[1] == i_codes[0]
    if differ is not None:
        m &= differ[1] != i_codes[1]
    return m


def plain_reference(q, t, k, metric, same=None, differ=None, shift=None):
    """(idx int64, dist fp32) (Mq, k): per group of queries that see the same candidates, the plain search of the metric over those
    candidates (gathered, k = min(k, their count)), indices mapped back; -1 / +inf behind a short list"""
    Mq, Nt = q.shape[0], t.shape[0]
    qs = same[0] if same is not None else np.zeros(Mq, np.int32)
    qd = differ[0] if differ is not None else np.zeros(Mq, np.int32)
    idx = np.full((Mq, k), -1, np.int64)
    dist = np.full((Mq, k), np.inf, np.float32)
    qdv, tdv = torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)
    for cs, cd in sorted(set(zip(qs.tolist(), qd.tolist()))):
        rows = np.flatnonzero((qs == cs) & (qd == cd))
        cand = np.flatnonzero(admitted((cs, cd), same, differ, Nt))
        c = min(k, len(cand))
        if c == 0:
            continue
        qq, tt = qdv[torch.from_numpy(rows).to(DEV)].contiguous(), tdv[torch.from_numpy(cand).to(DEV)].contiguous()
        i, d = ops.knn_search(qq, tt, c, shift) if metric == "euclidean" else ops.knn_search_l1(qq, tt, c)
        idx[rows, :c] = cand[i.cpu().numpy().astype(np.int64)]
        dist[rows, :c] = d.cpu().numpy()
    return idx, dist


def assert_equal(got, want, label):
    (gi, gd), (wi, wd) = got, want
    short = wi < 0
    assert np.array_equal(gi, wi), (label, "indices differ from the plain search over the admitted subset", np.flatnonzero((gi != wi).any(axis=1))[:5])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (label, "distance bits differ", np.flatnonzero((gd.view(np.uint32) != wd.view(np.uint32)).any(axis=1))[:5])
    assert (gi[short] == -1).all() and np.isposinf(gd[short]).all(), (label, "the tail of a short list")


def _omics(seed, rows, F, bf16=False):
    x = np.abs(np.random.default_rng(seed).standard_normal((rows, F))).astype(np.float32)
    return KR.to_bf16(x) if bf16 else x


def _shift(t, metric):
    return torch.from_numpy(t.astype(np.float64).mean(axis=0).astype(np.float32)).to(DEV) if metric == "euclidean" else None


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (q, t, fold codes of q, fold codes of t, site codes of q, site codes of t): shared and never written"""
    g = np.random.default_rng({"p77_f32": 41, "p77_bf16": 41, "t1000": 42, "split": 43}[name])
    if name.startswith("p77"):                               # the self-search of a cross-validation: 77 rows, 5 folds in random order, 3 sites
        x = _omics(51, 77, 37, name.endswith("bf16"))
        fold, site = g.permutation(77) % 5, g.integers(0, 3, 77)
        return x, x, fold.astype(np.int32), fold.astype(np.int32), site.astype(np.int32), site.astype(np.int32)
    if name == "t1000":
        q, t = _omics(52, 200, 45), _omics(53, 1000, 45)
        return q, t, g.integers(0, 5, 200).astype(np.int32), g.integers(0, 5, 1000).astype(np.int32), g.integers(0, 3, 200).astype(np.int32), g.integers(0, 3, 1000).astype(np.int32)
    q, t = _omics(54, 3, 20), _omics(55, 5000, 20)           # split
    return q, t, np.array([0, 1, 2], np.int32), g.integers(0, 4, 5000).astype(np.int32), np.array([1, 0, 1], np.int32), g.integers(0, 2, 5000).astype(np.int32)


def run_case(name, k, metric, with_sites, left=7, bf16=False):
    q, t, fq, ft, sq, st = case(name)
    same = (sq, st) if with_sites else None
    shift = _shift(t, metric)
    got = launch(operand(q, bf16, left), operand(t, bf16, left), k, metric, same=same, differ=(fq, ft), shift=shift)
    assert_equal(got, plain_reference(q, t, k, metric, same=same, differ=(fq, ft), shift=shift), (name, k, metric, with_sites))
    return got


@pytest.mark.parametrize("with_sites", [False, True])
@pytest.mark.parametrize("left", [7, 8])
@pytest.mark.parametrize("name", ["p77_f32", "p77_bf16"])
@pytest.mark.parametrize("metric", METRICS)
def test_fold_masked_self_search(metric, name, left, with_sites):
    idx, _ = run_case(name, 5, metric, with_sites, left, name.endswith("bf16"))
    fold = case(name)[2]
    assert (fold[idx[idx >= 0]] != np.repeat(fold, 5).reshape(-1, 5)[idx >= 0]).all(), "a neighbour from the query's own fold"
    assert not (idx == np.arange(77)[:, None]).any(), "a row found itself"


@pytest.mark.parametrize("k", [1, 5, 50, 96])
@pytest.mark.parametrize("metric", METRICS)
def test_several_tiles_per_row_block(metric, k):
    run_case("t1000", k, metric, with_sites=True)


@pytest.mark.parametrize("metric", METRICS)
def test_split_and_merge_path(metric):
    ns, rps = ops.knn_splits(3, 5000)
    assert ns > 1 and rps < 5000, "this shape must split the training rows"
    run_case("split", 6, metric, with_sites=True)


def _decided_blobs(n_groups, per, F, seed):
    """rows of `n_groups` groups whose neighbours are far from tied: every query decided under knn_bounds.analyse (asserted by the caller)"""
    g = np.random.default_rng(seed)
    x = np.abs(g.standard_normal((n_groups * per, F))).astype(np.float32)
    return x, np.repeat(np.arange(n_groups), per).astype(np.int32)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", ["tiles", "splits"])
def test_sorted_codes_that_skip_tiles_equal_the_shuffled_rows(metric, shape):
    """rows sorted by group (whole tiles, and with few queries whole splits, hold no admitted pair and are skipped) against the same rows
    shuffled (no tile can be skipped): the same neighbours after un-permuting.  Every query is decided, so ties cannot differ."""
    k = 5
    if shape == "tiles":
        x, grp = _decided_blobs(3, 256, 24, 65)              # 768 rows: 6 tiles, two per group; 6 query blocks
        q, gq = x, grp
    else:
        x, grp = _decided_blobs(4, 1280, 24, 62)             # 5120 candidate rows, 3 queries: split
        q, gq = x[[5, 1300, 5000]] + np.float32(0.125), grp[[5, 1300, 5000]]
        ns, rps = ops.knn_splits(3, 5120)
        assert ns > 1 and rps < 1280, "a split must lie inside one group"
    shift64 = x.astype(np.float64).mean(axis=0).astype(np.float32)
    for s in np.unique(gq):
        an = KB.analyse(q[gq == s], x[grp == s], k, shift64) if metric == "euclidean" else LB.analyse(q[gq == s], x[grp == s], k)
        assert an["decided"].all()
    shift = torch.from_numpy(shift64).to(DEV) if metric == "euclidean" else None
    si, sd = launch(in_nan_frame(q, 1, 8, 0), in_nan_frame(x, 1, 8, 0), k, metric, same=(gq, grp), shift=shift)
    perm = np.random.default_rng(63).permutation(len(x))
    pi, pd = launch(in_nan_frame(q, 1, 8, 0), in_nan_frame(x[perm], 1, 8, 0), k, metric, same=(gq, grp[perm]), shift=shift)
    assert np.array_equal(perm[pi], si) and np.array_equal(pd.view(np.uint32), sd.view(np.uint32))
    assert (grp[si] == gq[:, None]).all()
    assert_equal((si, sd), plain_reference(q, x, k, metric, same=(gq, grp), shift=shift), (shape, metric))


@pytest.mark.parametrize("metric", METRICS)
def test_short_lists_empty_lists_negative_codes_and_a_block_with_two_codes(metric):
    """two query blocks whose rows carry several codes (INT32_MIN, a negative and a large one); a group of 3 rows at k = 5: lists of 3,
    and of 2 once a differ pair that carries the row number keeps a row from finding itself; a query code that no candidate carries:
    the whole row -1 / +inf"""
    x = _omics(71, 140, 19)
    grp = np.where(np.arange(140) < 70, -5, 2_000_000_000).astype(np.int32)
    grp[[10, 75, 139]] = -2147483648                                 # a group of 3
    qg = grp.copy()
    qg[20] = 7                                                       # matches nothing
    shift = _shift(x, metric)
    got = launch(operand(x, False, 7), operand(x, False, 7), 5, metric, same=(qg, grp), shift=shift)
    assert_equal(got, plain_reference(x, x, 5, metric, same=(qg, grp), shift=shift), "same")
    idx, d = got
    assert (idx[20] == -1).all() and np.isposinf(d[20]).all()
    for r in (10, 75, 139):
        assert sorted(idx[r, :3].tolist()) == [10, 75, 139] and (idx[r, 3:] == -1).all() and np.isposinf(d[r, 3:]).all() and np.isfinite(d[r, :3]).all()
    # same group, other row: the differ pair carries the row number, so a row never finds itself and the group of 3 gives lists of 2
    me = np.arange(140, dtype=np.int32)
    got = launch(operand(x, False, 8), operand(x, False, 8), 5, metric, same=(qg, grp), differ=(me, me), shift=shift)
    assert_equal(got, plain_reference(x, x, 5, metric, same=(qg, grp), differ=(me, me), shift=shift), "same + differ")
    assert sorted(got[0][10, :2].tolist()) == [75, 139] and (got[0][10, 2:] == -1).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("Nt", [333, 5000])
def test_duplicate_rows_in_different_groups(metric, Nt):
    """rows 5 and 200 are identical and query 0 equals them: with both admitted they tie bit for bit and the smaller index comes first;
    with row 5 in the query's own fold only 200 is left"""
    q, t = KR.duplicates_case(Nt)
    qd, td = in_nan_frame(q, 1, 7, 2), in_nan_frame(t, 1, 7, 2)
    fq = np.zeros(3, np.int32)
    ft = np.ones(Nt, np.int32)
    ft[7] = 0
    idx, d = launch(qd, td, 2, metric, differ=(fq, ft))
    assert idx[0].tolist() == [5, 200] and d[0, 0] == d[0, 1] == 0.0
    ft[5] = 0
    idx, d = launch(qd, td, 2, metric, differ=(fq, ft))
    assert idx[0, 0] == 200 and d[0, 0] == 0.0 and idx[0, 1] not in (5, 7, 200)
    assert_equal((idx, d), plain_reference(q, t, 2, metric, differ=(fq, ft)), ("duplicates", Nt))


@pytest.mark.parametrize("metric", METRICS)
def test_nan_rows_never_beat_finite_ones(metric):
    q, t, fq, ft, _, _ = case("t1000")
    t = t.copy()
    t[[3, 130, 999]] = np.nan
    idx, d = launch(in_nan_frame(q, 2, 7, 3), in_nan_frame(t, 2, 7, 3), 5, metric, differ=(fq, ft))
    assert not np.isin(idx, [3, 130, 999]).any() and np.isfinite(d).all()
    assert_equal((idx, d), plain_reference(q, t, 5, metric, differ=(fq, ft)), "nan rows")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name,k", [("t1000", 50), ("split", 6)])
def test_run_to_run_bit_identical(name, k, metric):
    q, t, fq, ft, sq, st = case(name)
    qd, td = torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)
    a = ops.knn_search_grouped(qd, td, k, same=pair(sq, st), differ=pair(fq, ft), metric=metric)
    b = ops.knn_search_grouped(qd, td, k, same=pair(sq, st), differ=pair(fq, ft), metric=metric)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_refusals_write_nothing():
    q, t = torch.zeros(4, 8), torch.zeros(9, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_search_grouped(q, t, 2, differ=(torch.zeros(4, dtype=torch.int32), torch.zeros(9, dtype=torch.int32)))
    qd, td = q.to(DEV), t.to(DEV)
    cq, ct = torch.zeros(4, dtype=torch.int32, device=DEV), torch.ones(9, dtype=torch.int32, device=DEV)
    idx = torch.full((4, 2), SENTINEL_I, dtype=torch.int32, device=DEV)
    work = torch.zeros(64, dtype=torch.int64, device=DEV)
    base = _lib.KnnArgs(qd.data_ptr(), td.data_ptr(), None, idx.data_ptr(), None, work.data_ptr(), 8, 8, 2, 0, 512, 4, 9, 8, 2, 0, 0)
    lib = _lib.load()
    for codes, metric in (((None, None, None, None), 0), ((cq.data_ptr(), None, None, None), 0), ((None, None, None, ct.data_ptr()), 1),
                          ((cq.data_ptr(), ct.data_ptr(), None, None), 2), ((cq.data_ptr() + 2, ct.data_ptr(), None, None), 0)):
        assert lib.mmvae_knn_search_grouped(C.byref(_lib.KnnGroupArgs(base, *codes, metric)), None) == -1, (codes, metric)
    torch.cuda.synchronize()
    assert (idx == SENTINEL_I).all() and (work == 0).all()
    for bad in (lambda: ops.knn_search_grouped(qd, td, 2), lambda: ops.knn_search_grouped(qd, td, 2, differ=(cq, ct), metric="cosine"),
                lambda: ops.knn_search_grouped(qd, td, 2, differ=(cq, ct[:8])), lambda: ops.knn_search_grouped(qd, td, 2, same=(cq.long(), ct)),
                lambda: ops.knn_search_grouped(qd, td, 2, differ=(cq, ct), metric="manhattan", shift=torch.zeros(8, device=DEV)),
                lambda: ops.knn_search_grouped(qd, td, 10, differ=(cq, ct))):
        with pytest.raises(ValueError):
            bad()
