"""mmvae_tsne_affinities / mmvae_tsne_gradient / mmvae_tsne_update on the MI355X through ops: every output within the derived bounds of
tests/tsne_bounds.py of the float64 values of tests/tsne_ref.py, for every split count, and bit-identical from run to run."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tsne_bounds as TB  # noqa: E402
import tsne_ref as TR  # noqa: E402
from mmvae import ops  # noqa: E402

DEV = "cuda"
SENTINEL = -7.0


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits(t):
    return t.view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# affinities
# ---------------------------------------------------------------------------------------------------------------------------
def distances(N, k, scale, seed):
    """(d2 fp32 (N, k) ascending, rows the float64 search cannot converge on): row 0 has equal distances, row 1 (when there is one and
    k > 1) one neighbour a thousand times closer than the rest"""
    g = np.random.default_rng(seed)
    d = np.sort(scale * (0.5 + g.random((N, k)) * 4.0), axis=1)
    d[0] = d[0, 0]
    if N > 1 and k > 1:
        d[1, 0] = d[1, 1] * 1e-3
    return d.astype(np.float32)


@pytest.mark.parametrize("scale", [1.0, 1e-6, 1e6])
@pytest.mark.parametrize("N,k,perplexity", [(2, 1, 0.5), (2, 5, 2.5), (63, 5, 2.5), (63, 91, 45.5), (63, 91, 30.0), (130, 1, 0.5), (130, 5, 2.5),
                                            (130, 91, 45.5), (130, 91, 30.0)])
def test_affinities_within_bounds_at_the_returned_beta(N, k, perplexity, scale):
    d2 = distances(N, k, scale, 100 * N + k)
    _, _, ok64 = TR.binary_search(d2, perplexity)
    assert ok64[1:].all() or k == 1, "the inputs are chosen so that only the equal-distance row does not converge in float64"
    assert not ok64[0]
    dbuf = torch.full((N + 2, k + 3), float("nan"), device=DEV)
    dbuf[1:N + 1, 2:2 + k] = dev(d2)
    pbuf = torch.full((N + 2, k + 5), SENTINEL, device=DEV)
    bbuf = torch.full((N + 2,), SENTINEL, device=DEV)
    p, beta = ops.tsne_affinities(dbuf[1:N + 1, 2:2 + k], perplexity, p_out=pbuf[1:N + 1, 1:1 + k], beta_out=bbuf[1:N + 1])
    torch.cuda.synchronize()
    frame = pbuf.clone()
    frame[1:N + 1, 1:1 + k] = SENTINEL
    assert (frame == SENTINEL).all() and bbuf[0] == SENTINEL and bbuf[-1] == SENTINEL, "a write outside p / beta"
    beta_np, p_np = beta.cpu().numpy(), p.double().cpu().numpy()
    assert np.isfinite(beta_np).all() and (beta_np > 0).all()
    b = TB.affinity_bounds(d2, beta_np, perplexity)
    err = np.abs(p_np - b["p"])
    assert (err <= b["d_p"]).all(), (np.argwhere(~(err <= b["d_p"]))[:5], float((err / b["d_p"]).max()))
    gap = np.abs(b["H"] - np.log(perplexity))
    print(f"N {N} k {k} perplexity {perplexity} scale {scale}: p at {float((err / b['d_p']).max()):.3f} of its bound, "
          f"|H - log perplexity| at most {gap[ok64].max() if ok64.any() else 0.0:.2e} (bound {b['h_tol'].max():.2e})")
    assert (gap[ok64] <= b["h_tol"][ok64]).all(), (np.flatnonzero(ok64 & ~(gap <= b["h_tol"]))[:5], gap.max())
    assert np.allclose(p_np[0], 1.0 / k, rtol=1e-6)                                  # equal distances: the uniform row
    p2, beta2 = ops.tsne_affinities(dev(d2), perplexity)
    assert torch.equal(bits(p2), bits(p.contiguous())) and torch.equal(bits(beta2), bits(beta.contiguous()))


def test_affinities_end_on_rows_with_inf_and_nan():
    d2 = distances(9, 7, 1.0, 5)
    d2[2, 3], d2[4, 6], d2[5, :] = np.nan, np.inf, np.inf
    p, beta = ops.tsne_affinities(dev(d2), 3.0)
    torch.cuda.synchronize()
    clean = [0, 1, 3, 6, 7, 8]
    b = TB.affinity_bounds(d2[clean], beta.cpu().numpy()[clean], 3.0)
    assert (np.abs(p.double().cpu().numpy()[clean] - b["p"]) <= b["d_p"]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# gradient
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def joint_p(N):
    """CSR P (row_ptr int64, col int64, val fp32) of N random rows at perplexity min(10, (N - 1) / 4)"""
    g = np.random.default_rng(N)
    X = g.standard_normal((N, 4)) + 2.0 * g.standard_normal((3, 4))[np.arange(N) % 3]
    r, c, v = TR.joint_probabilities(X, min(10.0, (N - 1) / 4.0))
    return r, c, v.astype(np.float32)


def star_p(N):
    """row 0 holds every other row, every other row holds row 0 alone"""
    row_ptr = np.concatenate([[0], N - 1 + np.arange(N)]).astype(np.int64)
    col = np.concatenate([np.arange(1, N), np.zeros(N - 1, np.int64)])
    return row_ptr, col, np.full(2 * (N - 1), 1.0 / (2 * (N - 1)), np.float32)


def run_gradient(Y, P, exaggeration, splits):
    row_ptr, col, val = (dev(P[0].astype(np.int32)), dev(P[1].astype(np.int32)), dev(P[2]))
    out = ops.tsne_gradient(dev(Y), row_ptr, col, val, exaggeration, error=True, z_row=True, splits=splits)
    again = ops.tsne_gradient(dev(Y), row_ptr, col, val, exaggeration, error=True, z_row=True, splits=splits)
    torch.cuda.synchronize()
    for a, b in zip(out, again):
        assert torch.equal(bits(a), bits(b)), "two runs at one split count differ"
    grad, Z, err, zr = out
    return grad.double().cpu().numpy(), float(Z), float(err.double().sum()), zr.double().cpu().numpy()


def check_all_splits(Y, P, label):
    N = Y.shape[0]
    for exaggeration in (1.0, 12.0):
        for splits in (1, 2, 5, 0):
            used = ops.tsne_gradient_splits(N, splits)
            b = TB.gradient_bounds(Y, *P, exaggeration, used)
            got = run_gradient(Y, P, exaggeration, splits)
            worst = TB.check_gradient(b, *got, label=(label, exaggeration, splits, used))
            assert np.isfinite(got[0]).all()
            print(f"{label} x{exaggeration} splits {splits} -> {used}: errors over bounds {worst}")
    without = ops.tsne_gradient(dev(Y), dev(P[0].astype(np.int32)), dev(P[1].astype(np.int32)), dev(P[2]), 12.0)
    assert without[2] is None and without[3] is None
    assert np.array_equal(without[0].double().cpu().numpy(), got[0])                 # the error is an extra output, not another gradient


@pytest.mark.parametrize("scale", [1e-4, 1.0, 50.0])
@pytest.mark.parametrize("N", [2, 127, 129, 513, 777])
def test_gradient_within_bounds_for_every_split_count(N, scale):
    Y = (scale * np.random.default_rng(7 * N).standard_normal((N, 2))).astype(np.float32)
    check_all_splits(Y, joint_p(N), f"N {N} scale {scale}")


def test_gradient_with_duplicate_embedding_points():
    N = 513
    Y = np.random.default_rng(1).standard_normal((N, 2)).astype(np.float32)
    Y[9] = Y[100] = Y[512] = Y[5]
    Y[300:310] = Y[300]
    check_all_splits(Y, joint_p(N), "duplicates")


def test_gradient_with_a_hub_row_of_more_than_300_entries():
    N = 513
    P = star_p(N)
    assert P[0][1] - P[0][0] == 512 > 300
    Y = (3.0 * np.random.default_rng(2).standard_normal((N, 2))).astype(np.float32)
    check_all_splits(Y, P, "star")


def test_gradient_in_the_first_iterations_state_all_points_equal():
    """every w is exactly 1: Z = N (N - 1), R = A = 0, the gradient vanishes and KL = sum p log(p N (N - 1))"""
    N = 129
    P = joint_p(N)
    got = run_gradient(np.zeros((N, 2), np.float32), P, 12.0, 0)
    assert (got[0] == 0).all() and got[1] == N * (N - 1) and (got[3] == N - 1).all()


# ---------------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,momentum,lr", [(1, 0.5, 50.0), (777, 0.5, 1092.27), (777, 0.8, 200.0), (128, 0.8, 50.0)])
def test_update_step_within_bounds(N, momentum, lr):
    g = np.random.default_rng(N)
    y = g.standard_normal((N, 2)).astype(np.float32)
    upd = (1e-2 * g.standard_normal((N, 2))).astype(np.float32)
    gains = (0.01 + 3.0 * g.random((N, 2)) ** 3).astype(np.float32)
    grad = (1e-4 * g.standard_normal((N, 2))).astype(np.float32)
    upd[g.random((N, 2)) < 0.2] = 0.0                                                # a product of exactly zero: `dec`, no exemption needed
    if N > 100:
        upd[3, 0], grad[3, 0] = 1e-25, -1e-25                                        # a product below 2^-126: the branch may go either way
        upd[4, 1], grad[4, 1] = -1e-30, 1e-10
    mf, lf = float(np.float32(momentum)), float(np.float32(lr))                     # the values the kernel receives
    b = TB.update_bounds(y, upd, gains, grad, mf, lf)
    assert b["exempt"].mean() <= 0.01 and b["exempt"].sum() == (2 if N > 100 else 0)
    yd, ud, gd, grd = dev(y), dev(upd), dev(gains), dev(grad)
    norm = ops.tsne_update(yd, ud, gd, grd, momentum, lr, grad_norm=True)
    torch.cuda.synchronize()
    bad = TB.update_outside(b, yd.cpu().numpy(), ud.cpu().numpy(), gd.cpu().numpy())
    assert not bad, bad
    assert (gd >= 0.01).all() and torch.equal(bits(grd), bits(dev(grad)))
    clean = TB.update_bounds(y, np.where(b["exempt"], 0.0, upd), gains, grad, mf, lf)                   # the norm: without the exempt elements' doubt
    lo = min(clean["norm"], b["norm"]) * (1.0 - b["rel_norm"])
    hi = max(clean["norm"], b["norm"]) * (1.0 + b["rel_norm"])
    assert lo <= float(norm) <= hi, (float(norm), b["norm"], b["rel_norm"])
    y2, u2, g2 = dev(y), dev(upd), dev(gains)
    assert ops.tsne_update(y2, u2, g2, grd, momentum, lr) is None
    assert torch.equal(bits(y2), bits(yd)) and torch.equal(bits(u2), bits(ud)) and torch.equal(bits(g2), bits(gd))


def test_operand_checks():
    y = torch.zeros(8, 2, device=DEV)
    rp, col, val = torch.zeros(9, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, device=DEV)
    grad, Z, _, _ = ops.tsne_gradient(y, rp, col, val)                                # an empty P: the repulsion alone
    assert Z.item() == 56.0 and (grad == 0).all()
    for bad in (lambda: ops.tsne_gradient(y[:, :1], rp, col, val), lambda: ops.tsne_gradient(y.double(), rp, col, val),
                lambda: ops.tsne_gradient(y, rp[:-1], col, val), lambda: ops.tsne_gradient(y, rp.long(), col, val),
                lambda: ops.tsne_gradient(y, rp, col, val, splits=65), lambda: ops.tsne_gradient(y[:1], rp[:2], col, val),
                lambda: ops.tsne_affinities(torch.zeros(4, 3, device=DEV), 3.0), lambda: ops.tsne_affinities(torch.zeros(4, 3, device=DEV), 0.0),
                lambda: ops.tsne_update(y, y.clone(), y.clone(), torch.zeros(7, 2, device=DEV), 0.5, 1.0)):
        with pytest.raises((ValueError, TypeError)):
            bad()
