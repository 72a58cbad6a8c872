"""Writes tests/golden/knn_tuned.npz: small seeded inputs and what sklearn's KNeighborsRegressor and the reference's
ConditionedKNeighborsRegressor (src/models/conditioned_knn.py, loaded from a checkout of the reference by path) give on them at every
point of the reference's optimize_knn grid (src/knn_comparison/run_comparison.py:56-94; its loop is restated in tests/knn_tune_ref.py
because that module imports plotting libraries): the 16 predictions and validation MSEs and the winner, for the plain and for the
conditioned regressor.  tests/test_knn_tune_ref_cpu.py holds the numpy restatement to these records, tests/test_knn_tune_gpu.py the
device path.  Run from the repository root on the CPU:

    python tools/make_knn_tune_fixture.py --reference /path/to/the/reference/checkout

Sizes: 300 x 37 training rows, 77 validation rows, 23 outputs, 5 sites of 150 / 100 / 40 / 7 / 3 training rows, float32.  The seed is
the first for which (tests/knn_tune_ref.py: conditions, asserted again by the CPU test) every query is decided under the derived
bounds at every k of the grid for both metrics, plain and per site, and the two smallest MSEs of each grid are further apart than
their bounds."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SITE_ROWS = (150, 100, 40, 7, 3)
SITE_QUERIES = (30, 25, 12, 6, 4)


def inputs(seed):
    g = np.random.default_rng([20250301, seed])
    X = np.abs(g.standard_normal((300, 37))).astype(np.float32)
    Xq = np.abs(g.standard_normal((77, 37))).astype(np.float32)
    W = g.standard_normal((37, 23)) / 6.0
    Y = (X @ W + 0.1 * g.standard_normal((300, 23))).astype(np.float32)
    Yq = (Xq @ W + 0.1 * g.standard_normal((77, 23))).astype(np.float32)
    site = g.permutation(np.repeat(np.arange(5), SITE_ROWS)).astype(np.int64)
    site_q = g.permutation(np.repeat(np.arange(5), SITE_QUERIES)).astype(np.int64)
    return dict(X=X, Y=Y, Xq=Xq, Yq=Yq, site=site, site_q=site_q, seed=np.int64(seed))


if __name__ == "__main__":
    from make_knn_fixture import load_by_path
    import knn_tune_ref as TR
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ref = ap.parse_args().reference
    from sklearn.neighbors import KNeighborsRegressor
    cknn = load_by_path("ref_conditioned_knn", os.path.join(ref, "src", "models", "conditioned_knn.py"))
    for seed in range(200):
        d = inputs(seed)
        ok = TR.conditions(d)
        print("seed", seed, "decided, clear winner:", ok)
        if all(ok):
            break
    else:
        raise SystemExit("no seed satisfies the conditions")
    X, Y, Xq = (d[n].astype(np.float64) for n in ("X", "Y", "Xq"))
    Xs, Xqs = np.hstack([X, d["site"][:, None]]), np.hstack([Xq, d["site_q"][:, None]])
    out = dict(d)
    out["mse"], out["best"], out["pred"] = TR.optimize(lambda **p: KNeighborsRegressor(**p).fit(X, Y).predict(Xq), d["Yq"])
    out["cond_mse"], out["cond_best"], out["cond_pred"] = TR.optimize(lambda **p: cknn.ConditionedKNeighborsRegressor(**p).fit(Xs, Y).predict(Xqs), d["Yq"])
    assert all(TR.conditions(d, out))
    path = os.path.join(ROOT, "tests", "golden", "knn_tuned.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; winners", TR.combinations()[out["best"]], TR.combinations()[out["cond_best"]])
