"""tests/knn_l1_bounds.py on the CPU: the float32 emulations of mmvae_knn_search_l1 and mmvae_knn_weighted_rows stay inside the derived
bounds, the emulated key is the sequential chain the header specifies, and each of ten stated mistakes falls outside."""
import numpy as np
import pytest

import knn_bounds as KB
import knn_l1_bounds as LB
import knn_ref as KR


def _data(seed, Mq=40, Nt=333, F=37):
    g = np.random.default_rng(seed)
    return np.abs(g.standard_normal((Mq, F))).astype(np.float32), np.abs(g.standard_normal((Nt, F))).astype(np.float32)


def check(q, t, k, idx, dist):
    an = KB.check_search(q, t, k, idx, None, an=LB.analyse(q, t, k))
    LB.check_dist(an, idx, dist)
    return an


@pytest.mark.parametrize("k", [1, 5, 50])
def test_the_emulated_search_is_inside_the_bounds(k):
    q, t = _data(1)
    an = check(q, t, k, *LB.emulate(q, t, k))
    assert an["undecided"] <= 2
    qb, tb = KR.to_bf16(q), KR.to_bf16(t)
    check(qb, tb, k, *LB.emulate(qb, tb, k))


def test_the_key_is_one_sequential_chain_in_ascending_column_order():
    q, t = _data(2, 3, 4, 37)
    key = LB.keys_f32(q, t)
    differs_from_pairwise = False
    for i in range(3):
        for j in range(4):
            acc = np.float32(0)
            for c in range(37):
                acc = np.float32(acc + np.float32(abs(np.float32(q[i, c] - t[j, c]))))
            assert key[i, j].view(np.uint32) == acc.view(np.uint32)
            differs_from_pairwise |= key[i, j] != np.abs(q[i] - t[j]).sum(dtype=np.float32)
            rev = np.float32(0)
            for c in reversed(range(37)):
                rev = np.float32(rev + np.float32(abs(np.float32(q[i, c] - t[j, c]))))
            differs_from_pairwise |= key[i, j] != rev
    assert differs_from_pairwise, "the inputs do not tell the chain from another order"
    padded = LB.keys_f32(np.hstack([q, np.zeros((3, 27), np.float32)]), np.hstack([t, np.zeros((4, 27), np.float32)]))
    assert np.array_equal(key.view(np.uint32), padded.view(np.uint32))           # zero pad columns add +0


@pytest.mark.parametrize("mistake", ["squares", "drop_last_column", "drop_tail_chunk"])
def test_a_wrong_key_falls_outside(mistake):
    q, t = _data(3)
    with pytest.raises(AssertionError):
        check(q, t, 5, *LB.emulate(q, t, 5, mistake))


def test_the_larger_index_winning_a_tie_is_told_apart():
    q, t = KR.duplicates_case(333)
    assert LB.emulate(q, t, 2)[0][0].tolist() == [5, 200]
    assert LB.emulate(q, t, 2, "tie_larger")[0][0].tolist() == [200, 5]
    assert LB.emulate(q, t, 1, "tie_larger")[0][0].tolist() == [200]


def test_a_prefix_of_an_unsorted_list_falls_outside():
    q, t = _data(4)
    i50, d50 = LB.emulate(q, t, 50)
    i5, d5 = LB.emulate(q, t, 5)
    assert np.array_equal(i50[:, :5], i5) and np.array_equal(d50[:, :5], d5)
    u50, ud50 = LB.emulate(q, t, 50, "unsorted")
    check(q, t, 50, i50, d50)
    with pytest.raises(AssertionError):
        check(q, t, 5, u50[:, :5], ud50[:, :5])


def _weighted_case(zero=False):
    g = np.random.default_rng(5)
    y = g.standard_normal((333, 23)).astype(np.float32)
    idx = g.integers(0, 333, (40, 5))
    dist = np.sort(g.random((40, 5)).astype(np.float32) * 4 + 0.01, axis=1)
    if zero:
        dist[0, :2] = 0                                                           # two duplicates of the query
        dist[1, 0] = 0
    return idx, dist, y


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("zero", [False, True])
def test_the_emulated_weighted_rows_are_inside_the_bound(squared, zero):
    idx, dist, y = _weighted_case(zero)
    err = np.abs(LB.weighted_rows_f32(idx, dist, y, squared) - LB.weighted_rows(idx, dist, y, squared))
    assert (err <= LB.weighted_rows_tol(idx, dist, y, squared)).all()
    if zero:
        out = LB.weighted_rows_f32(idx, dist, y, squared)
        assert np.array_equal(out[1], y[idx[1, 0]]) and np.array_equal(out[0], (y[idx[0, 0]] + y[idx[0, 1]]) / np.float32(2))


@pytest.mark.parametrize("mistake,squared,zero", [("inv_d2", False, False), ("no_sqrt", True, False), ("no_zero_rule", False, True),
                                                  ("zero_rule_first_only", False, True), ("divide_by_k", False, False)])
def test_a_wrong_weight_falls_outside(mistake, squared, zero):
    idx, dist, y = _weighted_case(zero)
    err = np.abs(LB.weighted_rows_f32(idx, dist, y, squared, mistake) - LB.weighted_rows(idx, dist, y, squared))
    assert not (err <= LB.weighted_rows_tol(idx, dist, y, squared)).all()
