"""tests/group_moments_bounds.py against a float32 numpy restatement of the kernel (tests/group_moments_ref.py): the kernel as it is
must stay inside every bound on every input of tests/group_moments_cases.py, in three summation orders of the K products and both
group walks; each of a set of deliberate mistakes must fall outside on at least one case."""
import numpy as np
import pytest

import group_moments_bounds as MB
import group_moments_cases as MC
import group_moments_ref as MR

CASES = MC.all_cases()
_problems = {}


def problem(case):
    """Operands, float64 reference and bounds of a case, computed once"""
    if case.name not in _problems:
        a, w, bias = MC.make(case)
        _problems[case.name] = (a, w, bias, MB.problem_tol(a, w, bias, case.act, case.G))
    return _problems[case.name]


def worst(got, ref, tol):
    """largest err / bound; inf where a value is not finite or an error exceeds a zero bound"""
    got = np.asarray(got, np.float64)
    if not np.all(np.isfinite(got)):
        return np.inf
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    return float(r.max())


def ratios(case, **kw):
    a, w, bias, (m, tm, s, ts) = problem(case)
    gm, gs = MR.emulate(a, w, bias, case.act, case.G, **kw)
    return worst(gm, m, tm), (worst(gs, s, ts) if s is not None else 0.0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_kernel_restated_in_float32_stays_inside(case):
    for order in MR.K_ORDERS:
        for descending in (False, True):
            rm, rs = ratios(case, order=order, descending=descending)
            assert rm <= 1.0 and rs <= 1.0, (case.name, order, descending, rm, rs)


def test_the_bounds_are_not_vacuous():
    """the mean's bound is a few hundred roundings of the element's own terms at most, not a fraction of the value"""
    for case in CASES:
        a, w, bias, (m, tm, s, ts) = problem(case)
        mag = np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T + np.abs(bias)
        mag = mag.reshape(case.B, case.G, -1).mean(1)
        scale = 1.0 if case.act == MC.ACT_SIGMOID else mag             # a sigmoid's slope is at most 1/4: its bound is below the logit's
        assert np.all(tm <= 2 * (case.K + case.G + 8) * MB.U * np.maximum(scale, mag)), case.name


@pytest.mark.parametrize("mistake", MR.MISTAKES)
def test_a_mistake_falls_outside(mistake):
    hit = []
    for case in CASES:
        if case.G == 1 or (mistake in ("sigmoid-after-mean", "std-of-logits") and case.act != MC.ACT_SIGMOID):
            continue
        if mistake == "one-pass" and case.kind != "offset":              # the case the one-pass form is shown on
            continue
        rm, rs = ratios(case, mistake=mistake)
        if rm > 1.0 or rs > 1.0:
            hit.append(case.name)
            break
    assert hit, f"{mistake}: inside the bounds on every case"
