"""Writes tests/golden/knn_baselines.npz: small seeded inputs and what the reference's own code gives on them --
sklearn.neighbors.KNeighborsRegressor(n_neighbors=5), the reference's ConditionedKNeighborsRegressor (src/models/conditioned_knn.py)
and its calculate_neighborhood_hit (src/clustering_evaluation/metrics_utils.py), both loaded from a checkout of the reference by
path (this repository has a `src` package of its own).  tests/test_knn_ref_cpu.py holds the numpy restatement (tests/knn_ref.py) to
these records, tests/test_knn_gpu.py the device path.  Run from the repository root on the CPU:

    python tools/make_knn_fixture.py --reference /path/to/the/reference/checkout

The inputs are continuous random draws and the tool asserts that every query's k-th and (k+1)-th neighbour are clearly apart, so the
records do not depend on sklearn's unspecified order among ties."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GAP = 1e-4            # smallest relative gap between a query's k-th and (k+1)-th squared distance that counts as clear


def clear_gap(q, t, k):
    import knn_ref
    d = np.sort(knn_ref.dist2(q, t), axis=1)
    return float(((d[:, k] - d[:, k - 1]) / d[:, k]).min())


def inputs():
    g = np.random.default_rng(20240611)
    n_tr, n_q, fx, fy = 90, 40, 12, 9
    X = np.abs(g.standard_normal((n_tr, fx))).astype(np.float32)
    Y = g.random((n_tr, fy)).astype(np.float32)
    Xq = np.abs(g.standard_normal((n_q, fx))).astype(np.float32)
    site = g.integers(0, 4, n_tr).astype(np.int64)
    site[:3] = 4                                             # site 4: 3 training rows, fewer than k = 5
    site_q = g.integers(0, 5, n_q).astype(np.int64)
    site_q[:2] = 6                                           # site 6 is not in the training set: zero rows
    for sub in range(100):                                   # the first draw whose 6th and 7th neighbours are clearly apart in every row
        gl = np.random.default_rng([20240611, sub])
        centres = 0.8 * gl.standard_normal((6, 20))
        labels = gl.integers(0, 6, 300).astype(np.int64)
        feats = (centres[labels] + 1.5 * gl.standard_normal((300, 20))).astype(np.float32)
        if clear_gap(feats, feats, 6) > GAP:
            break
    return dict(X=X, Y=Y, Xq=Xq, site=site, site_q=site_q, feats=feats, labels=labels)


def assert_clear_gaps(q, t, k, what):
    assert clear_gap(q, t, k) > GAP, (what, clear_gap(q, t, k))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ref = ap.parse_args().reference
    from sklearn.neighbors import KNeighborsRegressor
    cknn = load_by_path("ref_conditioned_knn", os.path.join(ref, "src", "models", "conditioned_knn.py"))
    mu = load_by_path("ref_metrics_utils", os.path.join(ref, "src", "clustering_evaluation", "metrics_utils.py"))
    d = inputs()
    X, Y, Xq = (d[n].astype(np.float64) for n in ("X", "Y", "Xq"))
    assert_clear_gaps(Xq, X, 5, "plain")
    for s in np.unique(d["site_q"]):
        m = d["site"] == s
        if m.sum() > 5:
            assert_clear_gaps(Xq[d["site_q"] == s], X[m], 5, f"site {s}")
    assert_clear_gaps(d["feats"], d["feats"], 6, "neighbourhood hit")
    out = dict(d)
    out["knn_pred"] = KNeighborsRegressor(n_neighbors=5).fit(X, Y).predict(Xq)
    creg = cknn.ConditionedKNeighborsRegressor(n_neighbors=5).fit(np.hstack([X, d["site"][:, None]]), Y)
    out["cond_pred"] = creg.predict(np.hstack([Xq, d["site_q"][:, None]]))
    out["nh_k5"] = np.float64(mu.calculate_neighborhood_hit(d["feats"].astype(np.float64), d["labels"], k=5))
    out["nh_short"] = np.float64(mu.calculate_neighborhood_hit(d["feats"][:5].astype(np.float64), d["labels"][:5], k=5))
    path = os.path.join(ROOT, "tests", "golden", "knn_baselines.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
