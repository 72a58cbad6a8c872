"""tests/silhouette_ref.py against scikit-learn computed live and against the stored record (tests/golden/silhouette.npz, written by
tools/make_silhouette_fixture.py); the float32 emulation of the kernel's arithmetic inside the derived bounds of
tests/silhouette_bounds.py on every case, and every mistake a kernel could make outside them on at least one."""
import functools
import os

import numpy as np
import pytest

import silhouette_bounds as SB
import silhouette_ref as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "silhouette.npz")
SPLITS = (1, 3)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def analysed(name, nsplit):
    c = SR.make_case(name)
    return c, SB.analyse(c["x"], c["codes"], c["C"], c["shift"], nsplit)


@pytest.mark.parametrize("name", SR.SKLEARN_CASES)
def test_restatement_equals_sklearn_live_and_recorded(name):
    from sklearn.metrics import silhouette_samples, silhouette_score
    c, f = SR.make_case(name), fixture()
    assert np.array_equal(f[f"{name}.x"], c["x"]) and np.array_equal(f[f"{name}.labels"], c["codes"])
    x = c["x"].astype(np.float64)
    got, score = SR.silhouette_samples(x, c["codes"]), SR.silhouette_score(x, c["codes"])
    live = silhouette_samples(x, c["codes"], metric="euclidean")
    print(f"{name}: max |restatement - sklearn| = {np.abs(got - live).max():.1e}")
    assert np.abs(got - live).max() <= 1e-9 and np.abs(got - f[f"{name}.samples"]).max() <= 1e-9
    assert abs(score - silhouette_score(x, c["codes"], metric="euclidean")) <= 1e-9 and abs(score - float(f[f"{name}.score"])) <= 1e-9
    # class codes with gaps (an empty class) are the same labels
    assert np.array_equal(got, SR.parts(x, c["codes"], c["C"])["s"])


def test_restatement_refuses_what_sklearn_refuses():
    x = np.zeros((4, 2))
    for labels in ([0, 0, 0, 0], [0, 1, 2, 3]):
        with pytest.raises(ValueError, match="Valid values are 2 to n_samples - 1"):
            SR.silhouette_samples(x, labels)


def test_standardize_equals_standard_scaler_with_constant_columns():
    from sklearn.preprocessing import StandardScaler
    f = fixture()
    x = f["scaler.x"].astype(np.float64)
    z = SR.standardize(x)
    assert np.abs(z - StandardScaler().fit_transform(x)).max() <= 1e-9 and np.abs(z - f["scaler.z"]).max() <= 1e-9
    assert np.abs(z[:, [2, 4]]).max() <= 1e-15                      # constant columns: scale 1, not a division by rounding noise
    assert np.abs(z[:, [0, 1, 3, 5]].std(axis=0) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("name", SR.CASES)
def test_emulation_lies_inside_the_bounds(name):
    for ns in SPLITS:
        c, an = analysed(name, ns)
        ra, rb = SB.check(an, *SR.emulate(c["x"], c["codes"], c["C"], c["shift"], ns), label=f"{name} splits {ns}")
        print(f"{name} splits {ns}: errors at most {ra:.2f} (a), {rb:.2f} (b) of their bounds")


@pytest.mark.parametrize("mistake", SR.MISTAKES)
def test_every_mistake_lies_outside_on_some_case(mistake):
    caught = []
    for name in SR.CASES:
        for ns in SPLITS:
            c, an = analysed(name, ns)
            n = SB.outside(an, *SR.emulate(c["x"], c["codes"], c["C"], c["shift"], ns, mistake))
            if n:
                caught.append((name, ns, n))
    print(mistake, caught)
    assert caught, mistake


def test_a_leaking_diagonal_is_caught_where_a_is_one_distance():
    c, an = analysed("pairs_shift", 1)
    n = SB.outside(an, *SR.emulate(c["x"], c["codes"], c["C"], c["shift"], 1, "diag"))
    assert n >= 30, n
    assert (an["da"] / an["a"]).max() <= 2e-5                       # with the shift the bounds are tight
