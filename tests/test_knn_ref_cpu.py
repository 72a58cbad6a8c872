"""The float64 restatement of the k-NN baselines (tests/knn_ref.py) against the records of the reference's own code
(tests/golden/knn_baselines.npz, tools/make_knn_fixture.py) and, where it imports, against sklearn directly; the tie rule; and the
checker of tests/knn_bounds.py on a float32 emulation of the kernel's arithmetic: valid on every case the GPU tests run, every decided
query matched, at most 5 % of a case's queries undecided, and every seeded mistake caught."""
import functools
import os

import numpy as np
import pytest

import knn_bounds as KB
import knn_ref as KR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_baselines.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def case(name):
    c = KR.make_case(name)
    return c, KB.analyse(c["q"], c["t"], c["k"], c["shift"])


def test_restatement_equals_the_recorded_regressors():
    f = fixture()
    np.testing.assert_allclose(KR.knn_regress(f["X"], f["Y"], f["Xq"], 5), f["knn_pred"], rtol=0, atol=1e-14)
    got = KR.conditioned_regress(f["X"], f["Y"], f["site"], f["Xq"], f["site_q"], 5)
    np.testing.assert_allclose(got, f["cond_pred"], rtol=0, atol=1e-14)
    assert (f["cond_pred"][f["site_q"] == 6] == 0).all() and (f["site"] == 4).sum() == 3 and (f["site_q"] == 4).any()


def test_restatement_equals_the_recorded_neighbourhood_hit():
    f = fixture()
    assert KR.neighborhood_hit(f["feats"], f["labels"], 5) == pytest.approx(float(f["nh_k5"]), abs=1e-15)
    assert KR.neighborhood_hit(f["feats"][:5], f["labels"][:5], 5) == 0.0 == float(f["nh_short"])


def test_restatement_equals_sklearn_where_it_imports():
    nb = pytest.importorskip("sklearn.neighbors")
    g = np.random.default_rng(11)
    X, Y, Xq = g.random((120, 9)), g.random((120, 4)), g.random((50, 9))
    for k in (1, 5, 20):
        ref = nb.KNeighborsRegressor(n_neighbors=k, algorithm="brute").fit(X, Y)
        np.testing.assert_allclose(KR.knn_regress(X, Y, Xq, k), ref.predict(Xq), rtol=0, atol=1e-14)
        d, i = ref.kneighbors(Xq)
        idx, d2 = KR.search(Xq, X, k)
        assert np.array_equal(idx, i)
        np.testing.assert_allclose(np.sqrt(d2), d, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("Nt", [333, 5000])
def test_tie_rule_on_planted_duplicates(Nt):
    q, t = KR.duplicates_case(Nt)
    for fn in (lambda k: KR.search(q, t, k), lambda k: KR.emulate(q, t, k)):
        assert fn(1)[0][0].tolist() == [5]
        idx, d2 = fn(2)
        assert idx[0].tolist() == [5, 200] and d2[0, 0] == d2[0, 1]


@pytest.mark.parametrize("name", KR.MATCH_CASES)
def test_emulation_is_valid_and_few_queries_are_undecided(name):
    c, an = case(name)
    undecided = int((~an["decided"]).sum())
    print(f"{name}: {undecided} of {len(an['decided'])} queries undecided, largest band / D_k {np.max(an['band'] / np.maximum(an['Dk'], 1e-300)):.2e}")
    assert undecided <= 0.05 * len(an["decided"])           # a condition on the case (float64 alone), not a measurement of the kernel
    idx, d2 = KR.emulate(c["q"], c["t"], c["k"], c["shift"])
    KB.check_search(c["q"], c["t"], c["k"], idx, d2, c["shift"], label=name, an=dict(an))


def test_ill_conditioned_inputs_without_shift_only_widen_the_bounds():
    (c, an), (c0, an0) = case("ill_shift"), case("ill_noshift")
    assert np.median(an0["band"]) > 100 * np.median(an["band"])
    idx, d2 = KR.emulate(c0["q"], c0["t"], c0["k"], None)
    KB.check_search(c0["q"], c0["t"], c0["k"], idx, d2, None, label="ill_noshift", an=dict(an0))


MISTAKES = [("drop_train_tail", "p77_f32"), ("drop_train_tail", "t1000_k5"), ("drop_query_tail", "p77_f32"), ("drop_query_tail", "t1000_k5"),
            ("k_minus_1", "p77_f32"), ("k_minus_1", "t1000_k50"), ("read_pads", "p77_f32"), ("read_pads", "p77_bf16"),
            ("shift_one", "ill_shift"), ("bf16_products", "p77_f32"), ("bf16_products", "ill_shift")]


@pytest.mark.parametrize("mistake,name", MISTAKES)
def test_seeded_mistakes_are_caught(mistake, name):
    c, an = case(name)
    pad = np.nan if mistake == "read_pads" else None        # what the GPU tests plant around their operands
    idx, d2 = KR.emulate(c["q"], c["t"], c["k"], c["shift"], mistake=mistake, pad=pad)
    with pytest.raises(AssertionError):
        KB.check_search(c["q"], c["t"], c["k"], idx, d2, c["shift"], label=f"{mistake}/{name}", an=dict(an))


def test_tie_broken_towards_the_larger_index_is_caught():
    """on duplicates the distances tie exactly: the checker's bands cannot see the order, the explicit expectation does"""
    q, t = KR.duplicates_case(333)
    assert KR.emulate(q, t, 1, mistake="tie_larger")[0][0].tolist() == [200]
    assert KR.emulate(q, t, 2, mistake="tie_larger")[0][0].tolist() == [200, 5]
    assert KR.emulate(q, t, 1)[0][0].tolist() == [5]


def test_mean_rows_bound_is_tight_enough_to_see_a_wrong_neighbour():
    f = fixture()
    idx = KR.search(f["Xq"], f["X"], 5)[0]
    ref = KR.mean_rows(idx, f["Y"])
    tol = KB.mean_rows_tol(idx, f["Y"])
    out32 = np.zeros(ref.shape, np.float32)
    for n in range(5):
        out32 += f["Y"][idx[:, n]]
    out32 /= np.float32(5)
    assert (np.abs(out32 - ref) <= tol).all()
    wrong = idx.copy()
    wrong[:, 4] = (wrong[:, 4] + 1) % len(f["Y"])
    assert (np.abs(KR.mean_rows(wrong, f["Y"]) - ref) > tol).any(axis=1).all()
