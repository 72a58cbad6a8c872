"""Writes tests/golden/imputation_metrics.npz: the 67 x 45 edge case of tests/metrics_ref.edge_case (float32 inputs) and the values
sklearn.metrics / scipy.stats.pearsonr give on float64 casts of it -- what tests/test_metrics_ref_cpu.py holds the numpy
restatement to on machines without those two packages.  Run from the repository root: python tools/make_metrics_fixture.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def library_metrics(y, p):
    """The ten outputs as the reference's two routines obtain them, on float64 input."""
    from scipy.stats import pearsonr
    from sklearn.metrics import mean_absolute_error, mean_squared_error, r2_score
    from sklearn.metrics.pairwise import cosine_similarity
    import warnings
    y, p = y.astype(np.float64), p.astype(np.float64)
    mse = mean_squared_error(y.flatten(), p.flatten())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # ConstantInputWarning on the constant rows: their r is NaN
        r = np.array([pearsonr(y[i], p[i])[0] for i in range(len(y))])
    v = r[~np.isnan(r)]
    return {"MAE": mean_absolute_error(y.flatten(), p.flatten()), "MSE": mse, "RMSE": np.sqrt(mse),
            "R2": r2_score(y.flatten(), p.flatten()), "MeanR2": r2_score(y, p),
            "CosineSimilarity": float(np.diag(cosine_similarity(y, p)).mean()), "row_cosine": np.diag(cosine_similarity(y, p)).copy(),
            "PearsonMean": v.mean() if v.size else 0.0, "PearsonStd": v.std() if v.size else 0.0, "PearsonValid": int(v.size),
            "_pearson_all": r}


if __name__ == "__main__":
    import metrics_ref
    y, p = metrics_ref.edge_case()
    out = {k: np.asarray(v) for k, v in library_metrics(y, p).items()}
    path = os.path.join(ROOT, "tests", "golden", "imputation_metrics.npz")
    np.savez_compressed(path, y=y, p=p, **out)
    print(path, os.path.getsize(path), "bytes")
