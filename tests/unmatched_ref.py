"""The clustering of the unmatched samples restated in float64 numpy (both RNA scalings), the small seeded inputs of
tests/golden/unmatched_clustering.npz and the conditions its seed was chosen by.  tools/make_unmatched_fixture.py records what the
reference's cluster_imputation_methods.py gives on these inputs; cluster_reconstructed.py's feature preparation (its module imports
seaborn) is restated here: [original | reconstructed column], float32, nothing else (cluster_reconstructed.py:100-137).

Inputs: 96 matched rows (sites of 50 / 30 / 13 / 3 rows: the last has fewer than k = 5), A = 13 RNA and D = 11 DNA features, 40 RNA-only
rows with RAW TPM and 40 DNA-only rows, each with one sample of a site the label encoder does not know."""
import numpy as np

import knn_bounds as KB
import knn_ref as KR
import silhouette_ref as SR
import standardize_ref as StdR

A, D, K = 13, 11, 5
CLASSES = np.array(["Breast", "Colon", "Kidney", "Liver"])
UNKNOWN = "Zeta"
TRAIN_ROWS = (50, 30, 13, 3)
UNMATCHED_ROWS = (15, 12, 8, 4)
SAMPLE_TYPES = ("RNA-only", "DNA-only")
IMPUTERS = ("mean", "knn", "cond_knn")


def inputs(seed):
    g = np.random.default_rng([20250907, seed])
    ca, cd = g.standard_normal((4, A)), g.standard_normal((4, D))

    def draw(sites):
        raw = np.exp(0.8 * ca[sites] + 0.5 * g.standard_normal((len(sites), A))).astype(np.float32)         # TPM
        beta = (1.0 / (1.0 + np.exp(-(cd[sites] + 0.5 * g.standard_normal((len(sites), D)))))).astype(np.float32)
        return raw, beta

    ts = g.permutation(np.repeat(np.arange(4), TRAIN_ROWS)).astype(np.int64)
    raw, beta = draw(ts)
    d = dict(seed=np.int64(seed), train_rna=np.log1p(raw), train_dna=beta, train_site=ts)
    for name in ("rna", "dna"):
        s = g.permutation(np.concatenate([np.repeat(np.arange(4), UNMATCHED_ROWS), [-1]])).astype(np.int64)        # -1: the unknown site
        raw, beta = draw(np.where(s < 0, 0, s))
        d[f"{name}_only"], d[f"{name}_only_site"] = (raw if name == "rna" else beta), s
    return d


def site_names(codes):
    return np.where(codes < 0, UNKNOWN, CLASSES[np.maximum(codes, 0)])


def known(d, sample_type):
    """(original rows of the samples whose site the encoder knows, their codes)"""
    name = "rna_only" if sample_type == "RNA-only" else "dna_only"
    keep = d[f"{name}_site"] >= 0
    return d[name][keep], d[f"{name}_site"][keep]


def search_operands(d, sample_type, scaling):
    """(training features, training targets, the query as the imputers see it)"""
    x, _ = known(d, sample_type)
    if sample_type == "RNA-only":
        return d["train_rna"], d["train_dna"], (np.log1p(x) if scaling == "consistent" else x)
    return d["train_dna"], d["train_rna"], x


def impute(d, sample_type, method, scaling, k=K):
    """float64 (rows, cols) imputed block on the imputers' own scale"""
    X, Y, q = search_operands(d, sample_type, scaling)
    _, site = known(d, sample_type)
    if method == "mean":
        return np.broadcast_to(StdR.fit(Y)[0].astype(np.float32).astype(np.float64), (len(q), Y.shape[1]))
    if method == "knn":
        return KR.knn_regress(X, Y, q, k)
    return KR.conditioned_regress(X, Y, d["train_site"], q, site, k)


def features(d, sample_type, method, scaling, block=None, k=K):
    """the float32 feature matrix [original | imputed]; method "vae": block is the reconstructed column"""
    x, _ = known(d, sample_type)
    if method != "vae":
        block = impute(d, sample_type, method, scaling, k).astype(np.float32)
    block = np.asarray(block, np.float32)
    if sample_type == "RNA-only":
        return np.concatenate([np.log1p(x) if scaling == "consistent" else x, block], axis=1)
    if scaling == "reference" and method != "vae":
        block = np.log1p(block)
    return np.concatenate([x, block], axis=1)


def judged(F, labels, k=K):
    """dict of the table's numbers on the original features and on their PCA(2), float64"""
    mean, var, scale = StdR.fit(F)
    Z = StdR.apply64(np.asarray(F, np.float32), mean, scale)
    Zc = Z - Z.mean(axis=0)
    U, S, Vt = np.linalg.svd(Zc, full_matrices=False)
    Y = Zc @ Vt[:2].T
    return dict(Z=Z, sil=SR.silhouette_score(Z, labels), nh=KR.neighborhood_hit(Z, labels, k), pca_sil=SR.silhouette_score(Y, labels),
                pca_nh=KR.neighborhood_hit(Y, labels, k), explained=float((S[:2] ** 2).sum() / (S ** 2).sum()))


def conditions(d, k=K):
    """(every imputation query decided, every neighbourhood-hit query decided, no column in the constant rule's fuzzy zone), under the
    derived bounds of knn_bounds, for scaling="reference" (what the fixture records) and "consistent\""""
    imp = nh = clear = True
    for scaling in ("reference", "consistent"):
        for st in SAMPLE_TYPES:
            X, Y, q = search_operands(d, st, scaling)
            _, site = known(d, st)
            shift = X.astype(np.float64).mean(axis=0).astype(np.float32)
            imp &= bool(KB.analyse(q, X, k, shift)["decided"].all())
            for s in np.unique(site):
                rows = d["train_site"] == s
                Xs = X[rows]
                ks = min(k, len(Xs))
                if ks < len(Xs):
                    imp &= bool(KB.analyse(q[site == s], Xs, ks, Xs.astype(np.float64).mean(axis=0).astype(np.float32))["decided"].all())
            for method in IMPUTERS:
                F = features(d, st, method, scaling)
                mean, var, scale = StdR.fit(F)
                exact = np.ptp(F, axis=0) == 0
                clear &= bool(np.all(exact | (var >= 1e6 * StdR.constant_threshold(len(F), mean, var))))
                Z = StdR.apply(F, mean, scale)
                nh &= bool(KB.analyse(Z, Z, k + 1, Z.astype(np.float64).mean(axis=0).astype(np.float32))["decided"].all())
    return imp, nh, clear
