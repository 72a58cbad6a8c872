"""The site classifier's kernels on the MI355X against the float64 restatement (tests/downstream_ref.py, through the formulas of
tests/downstream_bounds.py) within the derived per-element bounds of tests/downstream_bounds.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import downstream_bounds as DB
import downstream_ref as R
from mmvae import _lib, ops

pytestmark = pytest.mark.gpu
F64 = np.float64
DEV = "cuda"


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def padded(a, ld):
    """a device copy of the (M, N) array as a view of an (M, ld) buffer filled with NaN (uint8: 255): nothing outside the view may be read"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((a.shape[0], ld), 255 if t.dtype == torch.uint8 else float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :a.shape[1]] = t.to(DEV)
    return buf[:, :a.shape[1]]


def inside(got, ref, tol, what):
    err = np.abs(got.detach().cpu().numpy().astype(F64) - ref)
    assert (err <= tol).all(), (what, float((err / np.maximum(tol, 1e-300)).max()))


def ln_case(M, N):
    g = np.random.default_rng(1000 * M + N)
    z = (1.5 + 2 * g.standard_normal((M, N))).astype(np.float32)
    gamma, beta = (1 + 0.3 * g.standard_normal(N)).astype(np.float32), (0.3 * g.standard_normal(N)).astype(np.float32)
    keep = (g.random((M, N)) >= 0.3).astype(np.uint8)
    dy = g.standard_normal((M, N)).astype(np.float32)
    return z, gamma, beta, keep, 0.3, dy


@pytest.mark.parametrize("M,N", [(1, 128), (33, 256), (5, 72), (300, 128), (7, 1024), (6, 520), (3, 384)])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("pad", [0, 12])
@pytest.mark.parametrize("layer_norm", [True, False])
def test_ln_act_forward_and_backward(M, N, masked, pad, layer_norm):
    z, gamma, beta, keep, p, dy = ln_case(M, N)
    keep = keep if masked else None
    if not layer_norm:
        gamma = beta = None
    place = (lambda a: padded(a, N + pad)) if pad else dev
    zt, dyt = place(z), place(dy)
    kt = place(keep) if masked else None
    gt, bt = (dev(gamma), dev(beta)) if layer_norm else (None, None)
    y_out = place(np.zeros((M, N), np.float32))
    y, mean, rstd = ops.ln_act_fwd(zt, gt, bt, kt, p, y_out=y_out)
    y64, mean64, rstd64 = DB.ln_fwd(z, gamma, beta, keep, p, 1e-5, F64)
    assert np.allclose(y64, R.ln_act_fwd(z, gamma, beta, keep, p)[0], rtol=1e-13, atol=1e-13)
    ty, tm, tr = DB.ln_fwd_tol(z, gamma, beta, keep, p, 1e-5)
    inside(y, y64, ty, "y")
    if layer_norm:
        inside(mean, mean64, tm, "mean"); inside(rstd, rstd64, tr, "rstd")
    else:
        assert mean is None and rstd is None
    if pad:                                                        # nothing is written outside the view
        assert torch.isnan(y_out._base[:, N:]).all()
    # backward from the device's own mean and rstd, which are inputs of the formula
    mean_in, rstd_in = (mean.cpu().numpy(), rstd.cpu().numpy()) if layer_norm else (None, None)
    dz_out = place(np.zeros((M, N), np.float32))
    dz, dg, db = ops.ln_act_bwd(dyt, zt, mean, rstd, gt, bt, kt, p, dz_out=dz_out)
    dz64, dg64, db64 = DB.ln_bwd(dy, z, mean_in, rstd_in, gamma, beta, keep, p, F64)
    tz, tg, tb = DB.ln_bwd_tol(dy, z, mean_in, rstd_in, gamma, beta, keep, p)
    inside(dz, dz64, tz, "dz")
    if layer_norm:
        inside(dg, dg64, tg, "dgamma"); inside(db, db64, tb, "dbeta")
        # written, not accumulated, and bit-identical from run to run (several workgroups at M = 300: the fixed-order reduction)
        dg2, db2 = torch.full_like(dg, 7.0), torch.full_like(db, -3.0)
        dz2, _, _ = ops.ln_act_bwd(dyt, zt, mean, rstd, gt, bt, kt, p, dgamma_out=dg2, dbeta_out=db2)
        assert torch.equal(dg, dg2) and torch.equal(db, db2) and torch.equal(dz, dz2)
    else:
        assert dg is None and db is None
    if pad:
        assert torch.isnan(dz_out._base[:, N:]).all()


def wce_case(M, C):
    g = np.random.default_rng(100 * M + C)
    x = (3 * g.standard_normal((M, C))).astype(np.float32)
    y = g.integers(0, C, M)
    y[0] = C - 1
    x[0, :] = x[0, 0]                                              # a row of ties: the first maximum is class 0
    if M > 2:
        x[2, C - 1] = x[2, 0] = np.abs(x[2]).max() + 1             # a tie of two
    w = (0.2 + 2 * g.random(C)).astype(np.float32)
    return x, y, w


@pytest.mark.parametrize("C", [2, 7, 24, 64])
@pytest.mark.parametrize("M", [1, 33, 300])
@pytest.mark.parametrize("weighted", [True, False])
def test_wce_mean(M, C, weighted):
    x, y, w = wce_case(M, C)
    w = w if weighted else None
    ref = DB.wce(x, y, w, F64)
    t_nll, t_sum, t_g = DB.wce_tol(x, y, w)
    xt, yt, wt = padded(x, C + 3), dev(y), dev(w) if weighted else None
    sums = torch.zeros(3, dtype=torch.float64, device=DEV)
    conf = torch.zeros(C, C, dtype=torch.int32, device=DEV)
    g, pred, nll = ops.wce_mean(xt, yt, wt, sums=sums, grad=True, pred=True, nll=True, confusion=conf)
    inside(g, ref["g"], t_g, "g"); inside(nll, ref["nll"], t_nll, "nll")
    s = sums.cpu().numpy()
    assert abs(s[0] - ref["sum_wnll"]) <= t_sum + 1e-12 * abs(ref["sum_wnll"]) and abs(s[1] - ref["sum_w"]) <= 1e-12 * ref["sum_w"] and s[2] == 0
    assert np.array_equal(pred.cpu().numpy(), ref["pred"]) and pred[0] == 0 and (M < 3 or pred[2] == 0)
    assert np.array_equal(conf.cpu().numpy(), ref["confusion"])                   # integer atomics: exact
    # sums and the confusion matrix are added to; the NULL groups: an evaluation pass without g, a gradient pass without predictions
    g2, pred2, nll2 = ops.wce_mean(xt, yt, wt, sums=sums, pred=True, confusion=conf)
    assert g2 is None and nll2 is None and torch.equal(pred2, pred)
    assert np.array_equal(conf.cpu().numpy(), 2 * ref["confusion"]) and abs(sums[1].item() - 2 * ref["sum_w"]) <= 1e-12 * ref["sum_w"]
    g3, pred3, _ = ops.wce_mean(xt, yt, wt, grad=True)
    assert pred3 is None and torch.equal(g3, g)


def test_wce_counts_labels_out_of_range_and_ignores_minus_100():
    x, y, w = wce_case(33, 7)
    y2 = y.copy()
    y2[4], y2[9], y2[11] = 7, -1, -100
    sums = torch.zeros(3, dtype=torch.float64, device=DEV)
    conf = torch.zeros(7, 7, dtype=torch.int32, device=DEV)
    g, pred, _ = ops.wce_mean(dev(x), dev(y2), dev(w), sums=sums, grad=True, pred=True, confusion=conf)
    assert sums[2].item() == 2 and conf.sum().item() == 30
    # computed as class 0 with class 0's weight; the ignored row has weight 0
    y3 = y2.copy()
    y3[[4, 9, 11]] = 0
    ref = DB.wce(x, y3, w, F64)
    wy = w.astype(F64)[y3]
    wy[11] = 0.0
    total = wy.sum()
    assert abs(sums[1].item() - total) <= 1e-12 * total
    assert (g[11] == 0).all()
    want4 = ref["g"][4] * ref["sum_w"] / total
    assert np.abs(g[4].cpu().numpy() - want4).max() <= 1e-5 * np.abs(want4).max()


def test_wce_divisor_is_the_same_in_every_workgroup():
    """Rows repeated in other workgroups of one launch get bit-identical gradients: every workgroup forms the same divisor."""
    C, M = 7, 300
    x, y, w = wce_case(M, C)
    for src, dst in ((1, 299), (5, 70), (40, 200), (3, 130)):                 # workgroups own 64 rows
        x[dst], y[dst] = x[src], y[src]
    g, _, _ = ops.wce_mean(dev(x), dev(y), dev(w), grad=True)
    for src, dst in ((1, 299), (5, 70), (40, 200), (3, 130)):
        assert torch.equal(g[src], g[dst])
    # and the divisor is the launch's own: the same 33 rows alone have another sum of weights
    g33, _, _ = ops.wce_mean(dev(x[:33]), dev(y[:33]), dev(w), grad=True)
    ratio = (g33[1] / g[1]).cpu().numpy().astype(F64)
    want = w.astype(F64)[y].sum() / w.astype(F64)[y[:33]].sum()
    assert np.abs(ratio - want).max() <= 4 * 2.0 ** -23 * want
    again, _, _ = ops.wce_mean(dev(x), dev(y), dev(w), grad=True)
    assert torch.equal(again, g)


def _adam_ref_and_tol(p, grad, m, v, t, wd, device_bc):
    ref = DB.adam(p, grad, m, v, t, 1e-3, 0.9, 0.999, 1e-8, wd, F64)
    return ref, DB.adam_tol(p, grad, m, v, t, 1e-3, 0.9, 0.999, 1e-8, wd, device_bc)


@pytest.mark.parametrize("form", ["host", "device", "advance"])
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_adam_step(form, t, wd):
    sizes = (1, 255, 257, 70001)
    g = np.random.default_rng(t)
    host = []
    for n in sizes:
        p = g.standard_normal(n).astype(np.float32)
        grad = (g.standard_normal(n) * 10.0 ** g.integers(-9, 1, n)).astype(np.float32)
        m = (0.1 * g.standard_normal(n)).astype(np.float32) if t > 1 else np.zeros(n, np.float32)
        v = (0.01 * g.random(n)).astype(np.float32) if t > 1 else np.zeros(n, np.float32)
        host.append((p, grad, m, v))
    devs = [[dev(a) for a in tensors] for tensors in host]
    items = (_lib.AdamWItem * len(sizes))(*[_lib.AdamWItem(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[0].numel())
                                            for d in devs])
    lr_dev = torch.tensor([1e-3], dtype=torch.float32, device=DEV)
    if form == "host":                                            # the corrections of the betas the kernel gets: rounded to fp32
        ops.adam_step(items, 1e-3, 0.9, 0.999, 1e-8, wd, 1 - float(np.float32(0.9)) ** t, 1 - float(np.float32(0.999)) ** t)
    elif form == "advance":
        step = torch.full((_lib.CTR_COPIES,), t - 1, dtype=torch.int64, device=DEV)
        ops.adam_step(items, 123.0, 0.9, 0.999, 1e-8, wd, 1.0, 1.0, step_dev=step, lr_dev=lr_dev)        # lr_dev wins over the value
        assert (step == t).all()
    else:                                                          # one counter, advanced by the caller
        step = torch.tensor([t - 1], dtype=torch.int64, device=DEV)
        _lib.check(_lib.load().mmvae_adam_step(C.cast(items, C.c_void_p), len(sizes), 1e-3, 0.9, 0.999, 1e-8, wd, 1.0, 1.0, 0, step.data_ptr(), 0,
                                               None, torch.cuda.current_stream().cuda_stream), "mmvae_adam_step")
        assert step.item() == t - 1
    for (p, grad, m, v), d in zip(host, devs):
        ref, tol = _adam_ref_and_tol(p, grad, m, v, t, wd, form != "host")
        for got, r, tl, name in zip((d[0], d[2], d[3]), ref, tol, "pmv"):
            inside(got, r, tl, (name, p.size))
        assert torch.equal(d[1], dev(grad))                        # the gradient is only read


def test_adam_differs_from_adamw_only_by_the_decay():
    g = np.random.default_rng(0)
    n = 1000
    p, grad = g.standard_normal(n).astype(np.float32), g.standard_normal(n).astype(np.float32)

    def run(fn, wd):
        d = [dev(p), dev(grad), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
        items = (_lib.AdamWItem * 1)(_lib.AdamWItem(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n))
        fn(items, 1e-3, 0.9, 0.999, 1e-8, wd, 0.1, 0.001)
        return d[0]
    assert torch.equal(run(ops.adam_step, 0.0), run(ops.adamw_step, 0.0))
    assert not torch.equal(run(ops.adam_step, 0.1), run(ops.adamw_step, 0.1))
