"""tests/downstream_bounds.py on the CPU: its float64 formulas state what tests/downstream_ref.py states, a float32 emulation of every
kernel stays inside the derived bounds (no bound is tighter than float32 arithmetic), and every plausible mistake of the list leaves
them (no bound is so wide that it would let one pass)."""
import numpy as np
import pytest

import downstream_bounds as DB
import downstream_ref as R

F32, F64 = np.float32, np.float64
SHAPES = [(1, 128), (33, 256), (5, 72), (300, 128)]


def f32(a):
    return np.asarray(a, np.float32)


def inside(got, ref, tol):
    return bool((np.abs(np.asarray(got, F64) - np.asarray(ref, F64)) <= tol).all())


def ln_case(M, N, seed=0):
    g = np.random.default_rng(1000 * M + N + seed)
    z = f32(1.5 + 2 * g.standard_normal((M, N)))
    gamma, beta = f32(1 + 0.3 * g.standard_normal(N)), f32(0.3 * g.standard_normal(N))
    keep = (g.random((M, N)) >= 0.3).astype(np.uint8)
    dy = f32(g.standard_normal((M, N)))
    return z, gamma, beta, keep, 0.3, dy


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("layer_norm", [True, False])
def test_layer_norm_emulation_stays_inside(M, N, masked, layer_norm):
    z, gamma, beta, keep, p, dy = ln_case(M, N)
    if not masked:
        keep = None
    if not layer_norm:
        gamma = beta = None
    y64, mean64, rstd64 = DB.ln_fwd(z, gamma, beta, keep, p, 1e-5, F64)
    ry = R.ln_act_fwd(z, gamma, beta, keep, p)
    assert np.allclose(y64, ry[0], rtol=1e-13, atol=1e-13)
    y32, mean32, rstd32 = DB.ln_fwd(z, gamma, beta, keep, p, 1e-5, F32)
    ty, tm, tr = DB.ln_fwd_tol(z, gamma, beta, keep, p, 1e-5)
    assert inside(y32, y64, ty)
    if layer_norm:
        assert inside(mean32, mean64, tm) and inside(rstd32, rstd64, tr)
        assert np.allclose(mean64, ry[1], rtol=1e-13) and np.allclose(rstd64, ry[2], rtol=1e-13)
        assert (ty[y64 > 0] < 1e-4 * (1 + np.abs(y64[y64 > 0]))).all()             # a bound, not a licence
    # backward from the fp32 mean and rstd
    mean_in, rstd_in = (f32(mean64), f32(rstd64)) if layer_norm else (None, None)
    dz64, dg64, db64 = DB.ln_bwd(dy, z, mean_in, rstd_in, gamma, beta, keep, p, F64)
    dz32, dg32, db32 = DB.ln_bwd(dy, z, mean_in, rstd_in, gamma, beta, keep, p, F32)
    tz, tg, tb = DB.ln_bwd_tol(dy, z, mean_in, rstd_in, gamma, beta, keep, p)
    assert inside(dz32, dz64, tz)
    rz = R.ln_act_bwd(dy, z, gamma, beta, keep, p)
    assert np.abs(dz64 - rz[0]).max() <= 1e-5 * max(np.abs(rz[0]).max(), 1e-30)          # the reference's own mean / rstd differ by an fp32 rounding
    if layer_norm:
        assert inside(dg32, dg64, tg) and inside(db32, db64, tb)
        assert tz.max() < 1e-4 * np.abs(dz64).max()


def outside(got, ref, tol):
    return bool((np.abs(np.asarray(got, F64) - np.asarray(ref, F64)) > tol).any())


@pytest.mark.parametrize("wrong", ["unbiased", "eps_outside", "scale_twice"])
def test_forward_mistakes_leave_the_bound(wrong):
    z, gamma, beta, keep, p, _ = ln_case(33, 256)
    if wrong == "eps_outside":
        z = f32(z * 1e-3)                                          # a row whose variance is comparable to eps
    y64, _, _ = DB.ln_fwd(z, gamma, beta, keep, p, 1e-5, F64)
    ty, _, _ = DB.ln_fwd_tol(z, gamma, beta, keep, p, 1e-5)
    assert inside(DB.ln_fwd(z, gamma, beta, keep, p, 1e-5, F32)[0], y64, ty)
    assert outside(DB.ln_fwd(z, gamma, beta, keep, p, 1e-5, F32, wrong)[0], y64, ty)


@pytest.mark.parametrize("wrong", ["no_scale_bwd", "scale_twice", "gate_xhat", "drop_term"])
def test_backward_mistakes_leave_the_bound(wrong):
    z, gamma, beta, keep, p, dy = ln_case(33, 256)
    _, mean, rstd = DB.ln_fwd(z, gamma, beta, keep, p, 1e-5, F64)
    mean, rstd = f32(mean), f32(rstd)
    ref = DB.ln_bwd(dy, z, mean, rstd, gamma, beta, keep, p, F64)
    tol = DB.ln_bwd_tol(dy, z, mean, rstd, gamma, beta, keep, p)
    good = DB.ln_bwd(dy, z, mean, rstd, gamma, beta, keep, p, F32)
    bad = DB.ln_bwd(dy, z, mean, rstd, gamma, beta, keep, p, F32, wrong)
    assert all(inside(a, b, t) for a, b, t in zip(good, ref, tol))
    assert outside(bad[0], ref[0], tol[0])
    if wrong != "drop_term":                                       # dgamma and dbeta do not contain that term
        assert outside(bad[1], ref[1], tol[1]) and outside(bad[2], ref[2], tol[2])


def wce_case(M, C, seed=0):
    g = np.random.default_rng(100 * M + C + seed)
    x = f32(3 * g.standard_normal((M, C)))
    y = g.integers(0, C, M)
    y[0] = C - 1
    x[0, :] = x[0, 0]                                              # all tied: first maximum 0, last maximum C - 1
    w = f32(0.2 + 2 * g.random(C))
    return x, y, w


@pytest.mark.parametrize("C", [2, 7, 24, 64])
@pytest.mark.parametrize("M", [1, 33, 300])
@pytest.mark.parametrize("weighted", [True, False])
def test_cross_entropy_emulation_stays_inside(M, C, weighted):
    x, y, w = wce_case(M, C)
    w = w if weighted else None
    r64, r32, ref = DB.wce(x, y, w, F64), DB.wce(x, y, w, F32), R.wce_mean(x, y, w)
    assert np.allclose(r64["g"], ref["g"], rtol=1e-12, atol=1e-15) and np.allclose(r64["sum_wnll"], ref["sum_wnll"], rtol=1e-13)
    assert np.array_equal(r64["pred"], ref["pred"]) and np.array_equal(r64["confusion"], ref["confusion"])
    t_nll, t_sum, t_g = DB.wce_tol(x, y, w)
    assert inside(r32["nll"], r64["nll"], t_nll) and inside(r32["g"], r64["g"], t_g)
    assert abs(r32["sum_wnll"] - r64["sum_wnll"]) <= t_sum and r32["sum_w"] == r64["sum_w"]
    assert np.array_equal(r32["pred"], r64["pred"]) and np.array_equal(r32["confusion"], r64["confusion"])
    assert t_g.max() < 1e-5 * np.abs(r64["g"]).max() + 1e-12


@pytest.mark.parametrize("wrong", ["div_M", "no_weight_grad", "last_max", "transposed"])
def test_cross_entropy_mistakes_leave_the_bound(wrong):
    x, y, w = wce_case(33, 7)
    ref, bad = DB.wce(x, y, w, F64), DB.wce(x, y, w, F32, wrong)
    _, _, t_g = DB.wce_tol(x, y, w)
    if wrong in ("div_M", "no_weight_grad"):
        assert outside(bad["g"], ref["g"], t_g)
    elif wrong == "last_max":
        assert bad["pred"][0] == 6 and ref["pred"][0] == 0 and not np.array_equal(bad["pred"], ref["pred"])
    else:
        assert not np.array_equal(bad["confusion"], ref["confusion"]) and np.array_equal(bad["confusion"].T, ref["confusion"])


def adam_case(n, t, seed=0):
    g = np.random.default_rng(n + t + seed)
    p = f32(g.standard_normal(n))
    grad = f32(g.standard_normal(n) * 10.0 ** g.integers(-9, 1, n))
    m = f32(0.1 * g.standard_normal(n)) if t > 1 else np.zeros(n, F32)
    v = f32(0.01 * g.random(n)) if t > 1 else np.zeros(n, F32)
    return p, grad, m, v


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("device_bc", [True, False])
def test_adam_emulation_stays_inside(t, wd, device_bc):
    p, grad, m, v = adam_case(257, t)
    ref = DB.adam(p, grad, m, v, t, 1e-3, 0.9, 0.999, 1e-8, wd, F64)
    want = R.adam_step(p.astype(F64), grad.astype(F64), m.astype(F64), v.astype(F64), t, float(F32(1e-3)), float(F32(wd)), float(F32(0.9)),
                       float(F32(0.999)), float(F32(1e-8)))
    assert all(np.allclose(a, b, rtol=1e-12, atol=1e-300) for a, b in zip(ref, want))
    got = DB.adam(p, grad, m, v, t, 1e-3, 0.9, 0.999, 1e-8, wd, F32, device_bc)
    tol = DB.adam_tol(p, grad, m, v, t, 1e-3, 0.9, 0.999, 1e-8, wd, device_bc)
    assert all(inside(a, b, c) for a, b, c in zip(got, ref, tol))
    assert tol[0].max() < 2e-6                                     # an update is at most about lr


@pytest.mark.parametrize("wrong", ["decoupled", "bc2_inside"])
def test_adam_mistakes_leave_the_bound(wrong):
    p, grad, m, v = adam_case(257, 1)
    wd = 1e-2 if wrong == "decoupled" else 1e-4
    ref = DB.adam(p, grad, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, wd, F64)
    tol = DB.adam_tol(p, grad, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, wd)
    assert inside(DB.adam(p, grad, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, wd, F32)[0], ref[0], tol[0])
    assert outside(DB.adam(p, grad, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, wd, F32, True, wrong)[0], ref[0], tol[0])
