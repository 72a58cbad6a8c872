"""Writes tests/golden/silhouette.npz: the inputs of the small shared cases (tests/silhouette_ref.py) and what scikit-learn gives on
them in float64 -- sklearn.metrics.silhouette_samples / silhouette_score (euclidean) on the labels of every case, and
StandardScaler().fit_transform on a matrix with a constant column.  tests/test_silhouette_ref_cpu.py holds the numpy restatement to
these records, tests/test_silhouette_gpu.py the device path.  Run from the repository root on the CPU:

    python tools/make_silhouette_fixture.py

The labels are the class codes of the rows, so a case with an empty class records sklearn's answer on the labels that do occur."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scaler_input():
    g = np.random.default_rng(20240702)
    x = (5.0 + 3.0 * g.standard_normal((50, 6))).astype(np.float32)
    x[:, 2] = 0.1                                            # a constant column whose mean is not exact in binary
    x[:, 4] = 7.0
    return x


def main():
    from sklearn.metrics import silhouette_samples, silhouette_score
    from sklearn.preprocessing import StandardScaler
    import silhouette_ref as SR
    out = {}
    for name in SR.SKLEARN_CASES:
        c = SR.make_case(name)
        x = c["x"].astype(np.float64)
        out[f"{name}.x"], out[f"{name}.labels"] = c["x"], c["codes"].astype(np.int64)
        out[f"{name}.samples"] = silhouette_samples(x, c["codes"], metric="euclidean")
        out[f"{name}.score"] = np.float64(silhouette_score(x, c["codes"], metric="euclidean"))
    xs = scaler_input()
    out["scaler.x"], out["scaler.z"] = xs, StandardScaler().fit_transform(xs.astype(np.float64))
    path = os.path.join(ROOT, "tests", "golden", "silhouette.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
