"""tests/pca_ref.py restates sklearn.decomposition.PCA(svd_solver="full") as the reference uses it
(src/clustering_evaluation/cluster_imputation_methods.py:140-187): components, the three variance vectors and the transform on every
case, and the sign rule on a hand-made case."""
import numpy as np
import pytest

import pca_ref as PR


@pytest.mark.parametrize("name", PR.CASES)
def test_restatement_equals_sklearn(name):
    decomposition = pytest.importorskip("sklearn.decomposition")
    c = PR.make_case(name)
    x = c["x"].astype(np.float64)
    sk = decomposition.PCA(n_components=c["k"], svd_solver="full", random_state=42)
    y = sk.fit_transform(x)
    ref = PR.fit(x, c["k"])
    diffs = {"components": np.abs(ref["components"] - sk.components_).max(),
             "explained_variance": np.abs(ref["explained_variance"] / sk.explained_variance_ - 1).max(),
             "explained_variance_ratio": np.abs(ref["explained_variance_ratio"] / sk.explained_variance_ratio_ - 1).max(),
             "singular_values": np.abs(ref["singular_values"] / sk.singular_values_ - 1).max(),
             "transform": np.abs(PR.transform(x, ref["mean"], ref["components"]) - y).max() / np.abs(y).max()}
    print(name, {k: f"{v:.2e}" for k, v in diffs.items()})
    # two float64 solvers (eigh of the scatter matrix against the SVD of the centred data): components of the k = 50 case move with
    # their eigengap of 1 in 10^4 (condition 1e4 x 1e-16 x the offset's cancellation)
    assert diffs["components"] <= (1e-9 if c["per_component"] else 1e-7)
    assert max(diffs["explained_variance"], diffs["explained_variance_ratio"], diffs["singular_values"]) <= 1e-10
    assert diffs["transform"] <= (1e-9 if c["per_component"] else 1e-7)
    assert np.allclose(ref["mean"], sk.mean_, rtol=0, atol=1e-12)


def test_sign_rule_by_hand():
    # rows along (3, -4) / 5: the one component's entry of largest magnitude is the second, so it is the one made positive
    x = np.array([[3.0, -4.0], [-3.0, 4.0], [6.0, -8.0], [-6.0, 8.0]])
    ref = PR.fit(x, 1)
    assert np.allclose(ref["components"], [[-0.6, 0.8]], atol=1e-15)
    assert np.array_equal(PR.sign_fix([[0.6, -0.8], [-0.1, 0.05], [0.2, 0.9]]), [[-0.6, 0.8], [0.1, -0.05], [0.2, 0.9]])
    assert np.allclose(ref["explained_variance"], [(2 * 25 + 2 * 100) / 3]) and np.allclose(ref["explained_variance_ratio"], [1.0])
    assert np.allclose(ref["singular_values"], [np.sqrt(250.0)])
    assert np.allclose(PR.transform(x, ref["mean"], ref["components"])[:, 0], [-5.0, 5.0, -10.0, 10.0])


def test_planted_spectrum_and_descending_order():
    c = PR.make_case("n300")
    ref = PR.fit(c["x"], 3)
    assert np.allclose(ref["explained_variance"], [40.0, 20.0, 10.0], rtol=1e-4)       # up to the rounding of x to fp32 at offset 100
    assert (np.diff(ref["lam_all"]) <= 0).all() and (ref["lam_all"] >= 0).all()
    n40 = PR.fit(PR.make_case("n40")["x"], 3)
    assert (n40["lam_all"][39:] <= 1e-6).all()                                          # N < F: rank N - 1
    b = PR.make_case("b77")["x"]
    assert np.array_equal(b.view(np.uint32) & 0xFFFF, np.zeros(b.shape, np.uint32))     # exact in bf16


def test_splits_formula():
    assert PR.splits_used(77, 37) == (1, 3) and PR.splits_used(1000, 129) == (4, 8) and PR.splits_used(1000, 129, 3) == (3, 11)
    assert PR.splits_used(52429, 1354) == (7, 235) and PR.splits_used(52429, 782) == (18, 92)
