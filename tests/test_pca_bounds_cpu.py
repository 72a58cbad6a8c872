"""The bounds of tests/pca_bounds.py hold for a float32 emulation of the kernels' arithmetic in several summation orders and split
counts, on every case of tests/pca_ref.py, and each of a list of mistakes lands outside some bound on some case.  The cases' own
conditions (component bounds, span bound) are asserted as well."""
import functools

import numpy as np
import pytest

import pca_bounds as PB
import pca_ref as PR


@functools.lru_cache(maxsize=None)
def case(name):
    return PR.make_case(name)


@functools.lru_cache(maxsize=None)
def analysed(name):
    c = case(name)
    return PB.analyse(c["x"], c["k"])


def violations(name, splits=0, order="ascending", mistake=None):
    """every check of tests/pca_bounds.py on the emulated pipeline of one case"""
    c, an = case(name), analysed(name)
    got = PR.emulate_fit(c["x"], c["k"], splits, order, mistake)
    label = f"{name} splits {splits} {order}"
    bad, ratios = PB.check_fit(an, got, c["per_component"], label)
    b2, ratios["scatter"] = PB.check_scatter(got["S"], c["x"], c["shift"], label)
    y = PR.emulate_project(c["x"], c["shift"], got["components"])
    b3, ratios["projection"] = PB.check_project(y, c["x"], c["shift"], got["components"], label)
    b4 = []
    if c["per_component"]:
        b4, ratios["end to end"] = PB.check_end_to_end(an, y, got["components"], label)
    return bad + b2 + b3 + b4, ratios


@pytest.mark.parametrize("name", PR.CASES)
def test_the_cases_meet_their_own_conditions(name):
    c, an = case(name), analysed(name)
    print(f"{name}: |E|_F {an['EF']:.3g}, centring term {an['centre']:.3g}, component bounds {an['sin'][:3]}, span bound {an['span']:.3g}")
    if c["per_component"]:
        assert c["k"] <= 3 and (an["sin"] <= PB.MAX_COMPONENT_BOUND).all()
    else:
        assert c["k"] == 50 and an["span"] <= PB.MAX_SPAN_BOUND
    assert an["centre"] <= 1e-6 * an["EF"]


@pytest.mark.parametrize("name", PR.CASES)
def test_emulation_stays_inside_every_bound(name):
    N, F = case(name)["x"].shape
    for splits, order in ((1, "ascending"), (0, "ascending"), (1, "descending"), (3, "descending"), (1, "blas"), (2, "blas")):
        bad, ratios = violations(name, splits, order)
        print(f"{name} splits {splits} -> {PR.splits_used(N, F, splits)[0]} {order}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
        assert bad == []


@pytest.mark.parametrize("mistake", PR.SCATTER_MISTAKES + PR.FIT_MISTAKES)
def test_every_mistake_is_caught_on_some_case(mistake):
    caught = []
    for name in PR.CASES:
        bad, _ = violations(name, 3, "ascending", mistake)
        if bad:
            caught.append(name)
    print(f"{mistake}: caught on {caught}")
    assert caught


def test_the_shifted_scatter_lies_far_inside_the_unshifted_bound():
    c = case("n300")
    S = PR.emulate_scatter(c["x"], c["shift"])
    err = np.abs(S.astype(np.float64) - PR.scatter(c["x"], c["shift"]))
    assert (err <= 1e-3 * PB.scatter_bound(c["x"], None)).all()          # what the shift is for: offset 100 squares to 10^4 per term
    bad, _ = PB.check_scatter(PR.emulate_scatter(c["x"], None), c["x"], None, "no shift")
    assert bad == []
