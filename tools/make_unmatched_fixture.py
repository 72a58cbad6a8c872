"""Writes tests/golden/unmatched_clustering.npz: the small seeded inputs of tests/unmatched_ref.py and what the reference's
src/clustering_evaluation/cluster_imputation_methods.py (loaded from a checkout of the reference by path, matplotlib on the Agg
backend) gives on them: apply_mean_imputation, apply_knn_imputation, apply_conditioned_knn_imputation, prepare_features and the PCA half
of perform_dimensionality_reduction, called on pandas frames; then sklearn's StandardScaler, silhouette_score and the reference's
calculate_neighborhood_hit (src/clustering_evaluation/metrics_utils.py) on the original and on the PCA features, as analyze_samples
computes them.  tests/test_unmatched_ref_cpu.py holds the numpy restatement to these records, tests/test_unmatched_gpu.py the device
path.  Run from the repository root on the CPU:

    python tools/make_unmatched_fixture.py --reference /path/to/the/reference/checkout

The seed is the first for which (tests/unmatched_ref.py: conditions, asserted again by the CPU test) every query's neighbour set is
decided under the derived bounds, for the imputation (k = 5) and for the neighbourhood hit (k + 1 = 6), and no feature column falls into
the constant rule's fuzzy zone."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


class Encoder:
    """what the reference uses of sklearn's LabelEncoder"""

    def __init__(self, classes):
        self.classes_ = np.asarray(classes)

    def transform(self, names):
        return np.searchsorted(self.classes_, np.asarray(names))


def frames(d, UR):
    import pandas as pd
    train = pd.DataFrame({"tpm_unstranded": list(d["train_rna"]), "beta_value": list(d["train_dna"]),
                          "primary_site_encoded": d["train_site"], "primary_site": UR.site_names(d["train_site"])})
    rna = pd.DataFrame({"tpm_unstranded": list(d["rna_only"]), "primary_site": UR.site_names(d["rna_only_site"])})
    dna = pd.DataFrame({"beta_value": list(d["dna_only"]), "primary_site": UR.site_names(d["dna_only_site"])})
    return train, rna, dna


if __name__ == "__main__":
    os.environ.setdefault("MPLBACKEND", "Agg")
    from make_knn_fixture import load_by_path
    import unmatched_ref as UR
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ref = ap.parse_args().reference
    from sklearn.metrics import silhouette_score
    from sklearn.preprocessing import StandardScaler
    cim = load_by_path("ref_cluster_imputation_methods", os.path.join(ref, "src", "clustering_evaluation", "cluster_imputation_methods.py"))
    mu = load_by_path("ref_metrics_utils", os.path.join(ref, "src", "clustering_evaluation", "metrics_utils.py"))
    for seed in range(200):
        d = UR.inputs(seed)
        ok = UR.conditions(d)
        print("seed", seed, "imputation decided, neighbourhood hit decided, no fuzzy column:", ok)
        if all(ok):
            break
    else:
        raise SystemExit("no seed satisfies the conditions")
    enc = Encoder(UR.CLASSES)
    train, rna, dna = frames(d, UR)
    imputed = {"mean": cim.apply_mean_imputation(train, rna, dna), "knn": cim.apply_knn_imputation(train, rna, dna, n_neighbors=UR.K),
               "cond_knn": cim.apply_conditioned_knn_imputation(train, rna, dna, enc, n_neighbors=UR.K)}
    out = dict(d)
    for method, pair in imputed.items():
        for st, df in zip(UR.SAMPLE_TYPES, pair):
            df = df[df["primary_site"].isin(enc.classes_)]                       # analyze_samples' filter
            labels = enc.transform(df["primary_site"])
            if st == "RNA-only":
                F = cim.prepare_features(df, use_original_rna=True, use_imputed_dna=True, imputed_dna_col="imputed_beta_value")
            else:
                F = cim.prepare_features(df, use_original_dna=True, use_imputed_rna=True, imputed_rna_col="imputed_tpm_unstranded")
            Y = cim.perform_dimensionality_reduction(F, method="pca", n_components=2)
            Z = StandardScaler().fit_transform(F)
            from sklearn.decomposition import PCA
            key = f"{st}/{method}/"
            out[key + "features"], out[key + "Z"], out[key + "labels"] = F, Z, labels
            out[key + "sil"], out[key + "nh"] = silhouette_score(Z, labels), mu.calculate_neighborhood_hit(Z, labels)
            out[key + "pca_sil"], out[key + "pca_nh"] = silhouette_score(Y, labels), mu.calculate_neighborhood_hit(Y, labels)
            out[key + "explained"] = PCA(n_components=2, random_state=42).fit(Z).explained_variance_ratio_.sum()
    path = os.path.join(ROOT, "tests", "golden", "unmatched_clustering.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, seed", int(d["seed"]))
