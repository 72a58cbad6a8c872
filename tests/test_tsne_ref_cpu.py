"""tests/tsne_ref.py (the float64 restatement the device t-SNE is held to) against sklearn's own records in tests/golden/tsne.npz
(tools/make_tsne_fixture.py): the perplexity search and the symmetric P, gradient and KL against _kl_divergence_bh(angle=0), the update
rule against a transcription of _gradient_descent's lines, trustworthiness, and the blobs record the device fit is compared with."""
import functools
import os

import numpy as np
import pytest

import tsne_ref as TR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne.npz")
CASES = ("a", "b", "c")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


def case(name):
    f = fixture()
    return {k[len(name) + 1:]: v for k, v in f.items() if k.startswith(name + "_")}


@pytest.mark.parametrize("name", CASES)
def test_search_reproduces_sklearns_conditional_p(name):
    c = case(name)
    d2, perp = c["d2"].astype(np.float64), float(c["perplexity"])
    p, beta, ok = TR.binary_search(d2, perp)
    assert ok.all()
    H, _ = TR.entropy(d2, beta)
    assert (np.abs(H - np.log(perp)) <= 1e-5).all()
    # sklearn's beta from its own p (log p_0 - log p_last = beta (d_last - d_0)): the restatement walks the same brackets, in the same
    # float64, so it ends on the same precision up to the rounding of the recovery
    sk = c["cond"]
    beta_sk = (np.log(sk[:, 0]) - np.log(sk[:, -1])) / (d2[:, -1] - d2[:, 0])
    assert np.allclose(beta, beta_sk, rtol=1e-9, atol=0)
    assert np.allclose(TR.entropy(d2, beta_sk)[1], sk, rtol=1e-9, atol=1e-300)
    assert np.allclose(p, sk, rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize("name", CASES)
def test_symmetric_csr_is_sklearns_joint_p(name):
    c = case(name)
    row_ptr, col, val = TR.symmetric_csr(c["idx"], c["cond"])
    assert np.array_equal(row_ptr, c["indptr"]) and np.array_equal(col, c["indices"])
    assert np.allclose(val, c["data"], rtol=1e-12, atol=0)
    assert abs(val.sum() - 1.0) <= 1e-12
    # the neighbours and P from the rows alone (sklearn searched on fp32 distances: the sets agree, the values to fp32)
    idx, dist = TR.neighbours(c["X"], c["idx"].shape[1])
    assert np.array_equal(np.sort(idx, axis=1), np.sort(c["idx"], axis=1))
    P = TR.joint_probabilities(c["X"], float(c["perplexity"]))
    assert np.array_equal(P[1], c["indices"]) and np.allclose(P[2], c["data"], rtol=1e-4, atol=1e-12)


@pytest.mark.parametrize("scale", (0, 1, 2))
@pytest.mark.parametrize("name", CASES)
def test_gradient_and_kl_against_the_angle_0_record(name, scale):
    f, c = fixture(), case(name)
    ref = TR.gradient(c[f"Y{scale}"], c["indptr"], c["indices"], c["data"].astype(np.float32))
    err = np.abs(ref["grad"] - c[f"grad{scale}"]).max() / np.abs(ref["grad"]).max()
    kerr = abs(ref["kl"] - float(c[f"kl{scale}"])) / abs(ref["kl"])
    print(f"{name} scale {scale}: gradient {err:.2e} of its largest entry, KL {kerr:.2e} relative")
    assert err <= float(f["grad_rel_tol"]) and kerr <= float(f["kl_rel_tol"])
    assert float(f["grad_rel_seen"]) <= float(f["grad_rel_tol"]) <= 1e-4 and float(f["kl_rel_seen"]) <= float(f["kl_rel_tol"]) <= 1e-4
    # the pieces add up: Z is the sum of z, the gradient is 4 (A - R / Z), exaggeration multiplies A alone
    assert ref["Z"] == pytest.approx(ref["z"].sum(), rel=1e-14)
    ex = TR.gradient(c[f"Y{scale}"], c["indptr"], c["indices"], c["data"], 12.0)
    assert np.allclose(ex["grad"] - 4.0 * 11.0 * ex["A"], 4.0 * (ex["A"] - ex["R"] / ex["Z"]), rtol=1e-12, atol=1e-300)


def test_update_is_sklearns_step_exactly():
    g = np.random.default_rng(3)
    p, upd, gains, grad = g.standard_normal(200), g.standard_normal(200), 0.005 + g.random(200), g.standard_normal(200)
    upd[:20] = 0.0
    # _gradient_descent, scikit-learn 1.7.2, the lines between the objective and the convergence check
    p0, update, gains0, grad0 = p.copy(), upd.copy(), gains.copy(), grad.copy()
    inc = update * grad0 < 0.0
    dec = np.invert(inc)
    gains0[inc] += 0.2
    gains0[dec] *= 0.8
    np.clip(gains0, 0.01, np.inf, out=gains0)
    grad0 *= gains0
    update = 0.8 * update - 200.0 * grad0
    p0 += update
    y1, u1, g1, norm = TR.update(p, upd, gains, grad, 0.8, 200.0)
    assert np.array_equal(y1, p0) and np.array_equal(u1, update) and np.array_equal(g1, gains0)
    assert norm == pytest.approx(np.linalg.norm(grad0), rel=1e-15)
    assert (g1 >= 0.01).all() and (g1 == 0.01).any()


def test_trustworthiness_silhouette_and_kl_of_the_recorded_embedding():
    f = fixture()
    X, labels = TR.blobs()
    Y = f["blobs_Y_pca"]
    assert TR.trustworthiness(X, Y, 5) == pytest.approx(float(f["blobs_trust"][0]), abs=1e-12)
    assert TR.silhouette(Y, labels) == pytest.approx(float(f["blobs_silhouette"][0]), abs=1e-12)
    assert TR.kl_of(TR.joint_probabilities(X, 30.0), Y) == pytest.approx(float(f["blobs_kl"][0]), rel=1e-9)
    # sklearn's own kl_divergence_ (fp32, one step earlier than the embedding it returns) is the same number to four digits
    assert np.allclose(f["blobs_kl"], f["blobs_sklearn_kl"], rtol=1e-3)


def test_blobs_record_is_eight_full_runs():
    f = fixture()
    assert len(f["blobs_kl"]) == len(f["blobs_trust"]) == len(f["blobs_silhouette"]) == 8
    assert (f["blobs_n_iter"] == 999).all()
    assert 0.6 < f["blobs_kl"].min() <= f["blobs_kl"].max() < 0.7 and f["blobs_trust"].min() > 0.98 and f["blobs_silhouette"].min() > 0.85


def test_fit_follows_sklearns_schedule():
    c = case("a")
    P = (c["indptr"], c["indices"], c["data"])
    g = np.random.default_rng(0)
    Y0 = 1e-4 * g.standard_normal((80, 2))
    out = TR.fit(P, Y0, max_iter=300)
    assert out["n_iter"] == 299 and out["learning_rate"] == 50.0
    assert [c[0] for c in out["checks"]] == [50, 100, 150, 200, 250, 300]
    assert [c[3] for c in out["checks"]] == [12.0] * 5 + [1.0]
    assert out["kl"] == out["checks"][-1][1]                # the error of the embedding BEFORE the last step, as sklearn reports it
    short = TR.fit(P, Y0, max_iter=250)
    assert short["n_iter"] == 250 and [c[0] for c in short["checks"]] == [50, 100, 150, 200, 250]
