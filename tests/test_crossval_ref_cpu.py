"""The host half of mmvae/crossval.py and its restatement (tests/crossval_ref.py) against the libraries the reference's
vae_cross_modality_cv.py calls: sklearn's KFold / train_test_split / KNeighborsRegressor, pandas' DataFrame.sample, scipy's ttest_rel."""
import numpy as np
import pytest

import crossval_ref as CR
from mmvae import crossval as CV


@pytest.mark.parametrize("n,folds", [(300, 5), (1000, 10), (7, 3), (10, 10)])
def test_kfold_assignments_are_sklearns_test_sets(n, folds):
    ms = pytest.importorskip("sklearn.model_selection")
    code = CV.kfold_assignments(n, folds)
    assert code.dtype == np.int32 and np.array_equal(code, CR.fold_codes(n, folds))
    for f, (train, test) in enumerate(ms.KFold(n_splits=folds, shuffle=True, random_state=42).split(np.zeros((n, 1)))):
        assert np.array_equal(np.flatnonzero(code == f), test) and np.array_equal(np.flatnonzero(code != f), train)
        assert np.array_equal(CR.fold_sets(n, folds)[f][0], train) and np.array_equal(CR.fold_sets(n, folds)[f][1], test)
    if n >= 300:
        assert not np.array_equal(code, CV.kfold_assignments(n, folds, seed=7))
    for bad in ((5, 1), (5, 6)):
        with pytest.raises(ValueError):
            CV.kfold_assignments(*bad)


@pytest.mark.parametrize("n,frac", [(300, 0.1), (1000, 0.25), (262144, 0.1), (25, 0.1), (15, 0.5)])
def test_subset_rows_are_pandas_sample(n, frac):
    pd = pytest.importorskip("pandas")
    want = pd.DataFrame({"x": np.arange(n)}).sample(frac=frac, random_state=42)["x"].to_numpy()
    assert np.array_equal(CV.subset_rows(n, frac), want) and np.array_equal(CR.subset(n, frac), want)
    if n == 262144:
        assert len(want) == 26214


@pytest.mark.parametrize("n", [270, 240, 11, 2])
def test_inner_split_is_sklearns_train_test_split(n):
    ms = pytest.importorskip("sklearn.model_selection")
    tr, va = ms.train_test_split(np.arange(n), test_size=0.1, random_state=42)
    got = CV.inner_split(n)
    assert np.array_equal(got[0], tr) and np.array_equal(got[1], va)
    assert np.array_equal(CR.inner(n)[0], tr) and np.array_equal(CR.inner(n)[1], va)


def test_inner_split_of_one_row_is_refused():
    with pytest.raises(ValueError):
        CV.inner_split(1)


@pytest.mark.parametrize("n", [3, 5, 10])
def test_paired_ttest_is_scipys(n):
    stats = pytest.importorskip("scipy.stats")
    g = np.random.default_rng(n)
    for trial in range(40):
        a = g.standard_normal(n)
        b = a + g.standard_normal(n) * g.choice([1e-3, 0.1, 1.0, 10.0]) + g.choice([0.0, 0.5, -2.0])
        r = stats.ttest_rel(a, b)
        t, p, df = CV.paired_ttest(a, b)
        assert df == n - 1
        assert abs(t - r.statistic) <= 1e-12 * abs(r.statistic), (t, r.statistic)
        assert abs(p - r.pvalue) <= 1e-12 * abs(r.pvalue), (p, r.pvalue)
    for trial in range(20):                                  # |t| >= 20: p from the far tail
        a = g.standard_normal(n)
        b = a + 3.0 + 1e-2 * g.standard_normal(n)
        r = stats.ttest_rel(a, b)
        t, p, _ = CV.paired_ttest(a, b)
        assert abs(r.statistic) >= 20
        assert abs(t - r.statistic) <= 1e-9 * abs(r.statistic) and abs(p - r.pvalue) <= 1e-9 * abs(r.pvalue), (p, r.pvalue)


def test_paired_ttest_degenerate_cases_are_scipys():
    stats = pytest.importorskip("scipy.stats")
    a = np.array([0.5, 0.25, 0.75, 1.0])
    for b in (a.copy(), a + 0.5, a - 0.25):
        with np.errstate(all="ignore"):
            r = stats.ttest_rel(a, b)
        t, p, df = CV.paired_ttest(a, b)
        assert df == 3
        assert (np.isnan(t) and np.isnan(r.statistic) and np.isnan(p) and np.isnan(r.pvalue)) or (t == r.statistic and p == r.pvalue == 0.0)
    assert np.isnan(CV.paired_ttest(a, a)[0]) and CV.paired_ttest(a, a + 0.5)[:2] == (-np.inf, 0.0) and CV.paired_ttest(a, a - 0.25)[:2] == (np.inf, 0.0)
    with pytest.raises(ValueError):
        CV.paired_ttest([1.0], [2.0])


def _result(direction, model, param, r2, mse):
    fm = {"Mean R2": list(r2), "MSE": list(mse), "Pearson": [x / 2 for x in r2]}
    return CV.aggregate(direction, model, "k" if model.startswith("knn") else "p", param, 0.0, fm)


def hand_built_results():
    a, b = "DNA -> RNA", "RNA -> DNA"
    return [_result(a, "mean", 0, [0.0, -0.01, 0.01, 0.0], [1.0, 1.1, 0.9, 1.0]),
            _result(a, "knn", 5, [0.30, 0.32, 0.28, 0.31], [0.70, 0.69, 0.72, 0.70]),
            _result(a, "knn", 10, [0.35, 0.36, 0.33, 0.36], [0.65, 0.64, 0.67, 0.66]),
            _result(a, "knn_site", 5, [0.40, 0.43, 0.39, 0.45], [0.60, 0.58, 0.61, 0.57]),
            _result(a, "vae", 200, [0.50, 0.52, 0.49, 0.53], [0.50, 0.47, 0.52, 0.46]),
            _result(b, "mean", 0, [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]),
            _result(b, "knn", 5, [0.20, 0.25, 0.15, 0.22], [0.80, 0.74, 0.86, 0.79]),
            _result(b, "vae", 200, [0.21, 0.24, 0.16, 0.21], [0.79, 0.77, 0.84, 0.78]),
            _result("only kNN", "knn", 5, [0.1, 0.2, 0.3, 0.4], [0.9, 0.8, 0.7, 0.6])]


def test_compare_on_hand_built_results():
    pytest.importorskip("scipy.stats")
    results = hand_built_results()
    assert results[1]["std_MSE"] == float(np.std([0.70, 0.69, 0.72, 0.70])) and results[1]["mean_Mean R2"] == float(np.mean([0.30, 0.32, 0.28, 0.31]))
    for metric in ("Mean R2", "MSE", "Pearson"):
        got = CV.compare(results, metric)
        CR.same_comparison(got, CR.compare(results, metric), rel=1e-11)
        assert [e["direction"] for e in got] == ["DNA -> RNA", "RNA -> DNA"]                 # a direction without VAE results is left out
        first, second = got
        assert first["best_knn"] == 10 and first["best_vae"] == 200 and first["best_knn_site"] == 5
        assert first["knn_vs_vae"]["winner"] == "VAE" and first["vae_vs_mean"]["winner"] == "VAE" and first["knn_site_vs_vae"]["winner"] == "VAE"
        assert second["knn_vs_vae"]["winner"] is None and "knn_site_vs_vae" not in second      # p >= 0.05: no winner
        assert first["knn_vs_vae"]["df"] == 3
    # lower is better for MSE: the same data with the kNN's and the VAE's errors swapped makes the kNN win
    swapped = [dict(r, model={"knn": "vae", "vae": "knn"}.get(r["model"], r["model"])) for r in results[:5] if r["param_value"] != 5 or r["model"] != "knn"]
    assert CV.compare(swapped, "MSE")[0]["knn_vs_vae"]["winner"] == "kNN" and CV.compare(swapped, "Mean R2")[0]["knn_vs_vae"]["winner"] == "kNN"


@pytest.mark.parametrize("k", [5, 10])
def test_restated_fold_predictions_are_sklearns(k):
    nb = pytest.importorskip("sklearn.neighbors")
    g = np.random.default_rng(5)
    X, Y = np.abs(g.standard_normal((120, 9))), g.standard_normal((120, 4))
    fold = CV.kfold_assignments(120, 5)
    got = CR.knn_predictions64(X, Y, fold, k)
    for train, test in CR.fold_sets(120, 5):
        want = nb.KNeighborsRegressor(n_neighbors=k).fit(X[train], Y[train]).predict(X[test])
        assert np.allclose(got[test], want, rtol=1e-12, atol=1e-14)
    site = g.integers(0, 3, 120)
    idx = CR.masked_neighbours(X, fold, k, site)
    ok = idx >= 0
    assert (site[idx[ok]] == np.repeat(site, k).reshape(-1, k)[ok]).all() and (fold[idx[ok]] != np.repeat(fold, k).reshape(-1, k)[ok]).all()


def test_metric_dict_has_the_references_keys():
    g = np.random.default_rng(6)
    y = g.standard_normal((30, 7))
    m = CR.metric_dict(y, y + 0.1 * g.standard_normal((30, 7)))
    assert list(m) == ["Mean R2", "Global R2", "MSE", "MAE", "Cosine Sim", "Pearson"] == list(CV.METRIC_KEYS)
    sk = pytest.importorskip("sklearn.metrics")
    p = y + 0.1 * np.random.default_rng(6).standard_normal((30, 7))
    assert abs(CR.metric_dict(y, p)["Mean R2"] - sk.r2_score(y, p)) < 1e-12 and abs(CR.metric_dict(y, p)["Global R2"] - sk.r2_score(y.ravel(), p.ravel())) < 1e-12
