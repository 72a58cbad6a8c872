"""float64 restatement of the cross-validation (mmvae/crossval.py; the reference's vae_cross_modality_cv.py): fold-masked brute-force
neighbours under the (d^2, index) order, the fold / subset / inner-split index sets from numpy's RandomState, the paired t-test
through scipy, the reference's metric dictionary through tests/metrics_ref.py and its statistical comparison."""
import numpy as np

import knn_ref as KR
import metrics_ref as MR

KEYS = {"Mean R2": "MeanR2", "Global R2": "R2", "MSE": "MSE", "MAE": "MAE", "Cosine Sim": "CosineSimilarity", "Pearson": "PearsonMean"}


def fold_sets(n, folds, seed=42):
    """[(train rows, test rows)] as KFold(folds, shuffle=True, random_state=seed).split yields them (both ascending)"""
    idx = np.arange(n)
    np.random.RandomState(seed).shuffle(idx)
    sizes = [n // folds + (1 if f < n % folds else 0) for f in range(folds)]
    out, lo = [], 0
    for s in sizes:
        test = np.sort(idx[lo:lo + s])
        out.append((np.setdiff1d(np.arange(n), test), test))
        lo += s
    return out


def fold_codes(n, folds, seed=42):
    code = np.empty(n, np.int32)
    for f, (_, test) in enumerate(fold_sets(n, folds, seed)):
        code[test] = f
    return code


def subset(n, frac, seed=42):
    return np.random.RandomState(seed).choice(n, round(frac * n), replace=False)


def inner(n, seed=42):
    p = np.random.RandomState(seed).permutation(n)
    n_val = int(np.ceil(0.1 * n))
    return p[n_val:], p[:n_val]


def masked_neighbours(X, fold, k, site=None):
    """(N, k) int64, -1 behind a short list: for every row the k nearest rows (float64 d^2, ties to the smaller index) among the rows of
    other folds (and, with `site`, of the row's own site)"""
    X, fold = np.asarray(X, np.float64), np.asarray(fold)
    N = X.shape[0]
    d = KR.dist2(X, X)
    out = np.full((N, k), -1, np.int64)
    for i in range(N):
        ok = fold != fold[i]
        if site is not None:
            ok &= np.asarray(site) == site[i]
        cand = np.flatnonzero(ok)
        best = cand[np.argsort(d[i, cand], kind="stable")[:k]]
        out[i, :len(best)] = best
    return out


def knn_predictions64(X, Y, fold, k):
    """KNeighborsRegressor(k).fit(train).predict(test) per fold, float64, assembled over all rows"""
    return KR.mean_rows(masked_neighbours(X, fold, k), Y)


def metric_dict(y, p):
    """calculate_metrics of the reference (vae_cross_modality_cv.py:71-108) in float64"""
    m = MR.metrics(y, p)
    return {k: float(m[src]) for k, src in KEYS.items()}


def ttest(a, b):
    from scipy import stats
    r = stats.ttest_rel(np.asarray(a, np.float64), np.asarray(b, np.float64))
    return float(r.statistic), float(r.pvalue), len(a) - 1


def _pair(na, a, nb, b, metric):
    sa, sb = a["fold_metrics"][metric], b["fold_metrics"][metric]
    t, p, df = ttest(sa, sb)
    ma, mb = float(np.mean(sa)), float(np.mean(sb))
    winner = None
    if p < 0.05:
        if any(x in metric for x in ["R2", "Cosine", "Pearson"]):
            winner = na if ma > mb else nb
        else:
            winner = na if ma < mb else nb
    return {"a": na, "b": nb, "t": t, "p": p, "df": df, "mean_a": ma, "mean_b": mb, "winner": winner}


def compare(results, metric):
    """perform_statistical_comparison (vae_cross_modality_cv.py:453-530) as data, through scipy"""
    out = []
    directions = []
    for r in results:
        if r["direction"] not in directions:
            directions.append(r["direction"])
    for direction in directions:
        rows = [r for r in results if r["direction"] == direction]
        knn, vae = [r for r in rows if r["model"] == "knn"], [r for r in rows if r["model"] == "vae"]
        mean, ksite = [r for r in rows if r["model"] == "mean"], [r for r in rows if r["model"] == "knn_site"]
        if not knn or not vae:
            continue
        bk, bv = max(knn, key=lambda x: x["mean_Mean R2"]), max(vae, key=lambda x: x["mean_Mean R2"])
        e = {"direction": direction, "metric": metric, "best_knn": bk["param_value"], "best_vae": bv["param_value"],
             "knn_vs_vae": _pair("kNN", bk, "VAE", bv, metric)}
        if mean:
            e["vae_vs_mean"] = _pair("VAE", bv, "Mean", mean[0], metric)
        if ksite:
            bs = max(ksite, key=lambda x: x["mean_Mean R2"])
            e["best_knn_site"] = bs["param_value"]
            e["knn_site_vs_vae"] = _pair("kNN-site", bs, "VAE", bv, metric)
        out.append(e)
    return out


def same_comparison(got, want, rel=1e-9):
    """the two comparison lists agree: keys, choices and winners exactly, t / p / means within `rel`"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w), (set(g), set(w))
        for key, wv in w.items():
            if not isinstance(wv, dict):
                assert g[key] == wv, key
                continue
            for f, x in wv.items():
                y = g[key][f]
                if isinstance(x, float):
                    assert (np.isnan(x) and np.isnan(y)) or x == y or abs(x - y) <= rel * abs(x), (key, f, y, x)
                else:
                    assert y == x, (key, f, y, x)
