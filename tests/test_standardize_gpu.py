"""mmvae_standardize_fit / mmvae_standardize_apply and mmvae.clustering.StandardScaler on the MI355X against tests/standardize_ref.py and
the derived bounds of tests/standardize_bounds.py, on the cases of tests/standardize_cases.py: the fit within the bounds, the apply
with the yardstick's mean / scale BIT-EQUAL to numpy's expression, the apply after the device fit within the z bound, guard columns and
rows of z untouched, two runs identical, every accepted split count on the 4099-row case; more rows than one grid of row blocks holds;
a tie problem on which a reciprocal-multiply shows; StandardScaler beside clustering.standardize, on other rows, and what it refuses."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import standardize_bounds as B  # noqa: E402
import standardize_cases as SC  # noqa: E402
import standardize_ref as R  # noqa: E402
from mmvae import clustering, ops  # noqa: E402

DEV = "cuda"
GUARD = -12345.0
CASE_IDS = [c.name for c in SC.CASES]


def dev_parts(parts, arrs, rows):
    """device tensors of the parts: a matrix part is a view of a (rows, ld) buffer whose pad columns hold NaN"""
    out = []
    for a, p in zip(arrs, parts):
        dt = torch.bfloat16 if p.dtype == "bf16" else torch.float32
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
        if not p.one_row:
            buf = torch.full((rows, p.ld or p.cols), float("nan"), dtype=dt, device=DEV)
            buf[:, :p.cols] = t
            t = buf[:, :p.cols]
        out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def problem(name):
    case = SC.BY_NAME[name]
    arrs = SC.arrays(case)
    X = SC.full(case, arrs)
    mean, var, scale = R.fit(X)
    for a in (X, mean, var, scale):
        a.setflags(write=False)
    return case, arrs, X, (mean, var, scale)


def framed(rows, F):
    """z as a view: one guard row before and after, ldz = F + 3"""
    buf = torch.full((rows + 2, F + 3), GUARD, dtype=torch.float32, device=DEV)
    return buf, buf[1:rows + 1, :F]


def guards_intact(buf, rows, F):
    b = buf.clone()
    b[1:rows + 1, :F] = GUARD
    return bool((b == GUARD).all())


def f64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def check_fit(got, want, tols, label):
    for g, w, t, what in zip(got, want, tols, ("mean", "var", "scale")):
        err = np.abs(g.cpu().numpy() - w)
        print(f"{label} {what}: max err {err.max():.3e}, max err / tol {np.max(err / np.where(t > 0, t, np.inf)):.3f}, zero-tol columns off: {int((err[t == 0] > 0).sum())}")
        assert np.all(err <= t), (label, what, float(err.max()))


@pytest.mark.parametrize("name", CASE_IDS)
def test_fit_and_apply(name):
    case, arrs, X, ref = problem(name)
    rows, F = X.shape
    parts = dev_parts(case.parts, arrs, rows)
    used = ops.standardize_fit_splits(rows, F)
    tols = B.fit_tol(X, used)
    got = ops.standardize_fit(parts)
    check_fit(got, ref, tols, name)
    again = ops.standardize_fit(parts)
    for g, h in zip(got, again):
        assert np.array_equal(bits(g.cpu().numpy()), bits(h.cpu().numpy()))
    mean, var, scale = ref
    exact = np.ptp(X, axis=0) == 0
    assert np.all(got[1].cpu().numpy()[exact] == 0) and np.all(got[2].cpu().numpy()[exact] == 1.0)

    # transform with the yardstick's mean / scale: the bits of numpy's expression, nothing written outside z
    buf, z = framed(rows, F)
    assert ops.standardize_apply(parts, f64(mean), f64(scale), out=z) is z
    want = R.apply(X, mean, scale)
    assert np.array_equal(bits(z.cpu().numpy()), bits(want))
    assert guards_intact(buf, rows, F)
    z2 = ops.standardize_apply(parts, f64(mean), f64(scale))
    assert z2.is_contiguous() and torch.equal(z2.view(torch.int32), z.contiguous().view(torch.int32))

    # transform after the device fit
    buf, z = framed(rows, F)
    ops.standardize_apply(parts, got[0], got[2], out=z)
    z64 = R.apply64(X, mean, scale)
    err = np.abs(z.cpu().numpy().astype(np.float64) - z64)
    tol = B.z_tol(z64, scale, tols[0], tols[2])
    print(f"{name} z: max err {err.max():.3e}, max err / tol {np.max(err / tol):.3f}")
    assert np.all(err <= tol)
    assert guards_intact(buf, rows, F)
    if name == "r1":
        assert np.all(z.cpu().numpy() == 0)


def test_every_split_count():
    """4099 rows (prime): the planner's split and every forced count 1 .. 64, of which every one above 1 leaves the last split short"""
    case, arrs, X, ref = problem(SC.SPLIT_CASE)
    rows, F = X.shape
    parts = dev_parts(case.parts, arrs, rows)
    seen = set()
    for splits in range(0, 65):
        used, rps = R.splits_used(rows, F, splits)
        assert ops.standardize_fit_splits(rows, F, splits) == used and (used == 1 or rows % rps)
        seen.add(used)
        got = ops.standardize_fit(parts, splits=splits)
        again = ops.standardize_fit(parts, splits=splits)
        for g, h in zip(got, again):
            assert np.array_equal(bits(g.cpu().numpy()), bits(h.cpu().numpy())), splits
        tols = B.fit_tol(X, used)
        for g, w, t in zip(got, ref, tols):
            assert np.all(np.abs(g.cpu().numpy() - w) <= t), splits
    assert {1, 2, 3, 64} <= seen


def test_more_row_blocks_than_one_grid_holds():
    """the apply walks blocks of 16 rows with blockIdx.y, at most 65 535 of them at once: 65 535 * 16 + 37 rows take the second round.
    Three columns keep it small (12 MB); the fit runs 64 splits of 16 385 rows."""
    rows = 65535 * 16 + 37
    rng = np.random.default_rng(77)
    a = (2.0 + rng.normal(size=(rows, 2))).astype(np.float32)
    one = np.array([0.75], dtype=np.float32)
    X = np.concatenate([a, np.broadcast_to(one, (rows, 1))], axis=1)
    parts = [torch.from_numpy(a).to(DEV), torch.from_numpy(one).to(DEV)]
    mean, var, scale = R.fit(X)
    used = ops.standardize_fit_splits(rows, 3)
    assert used == 64
    got = ops.standardize_fit(parts)
    check_fit(got, (mean, var, scale), B.fit_tol(X, used), "rows 1048597")
    buf, z = framed(rows, 3)
    ops.standardize_apply(parts, f64(mean), f64(scale), out=z)
    assert np.array_equal(bits(z.cpu().numpy()), bits(R.apply(X, mean, scale)))
    assert guards_intact(buf, rows, 3)


def test_apply_divides_and_does_not_multiply_by_a_reciprocal():
    X, mean, scale = SC.tie_problem()
    z = ops.standardize_apply(torch.from_numpy(X).to(DEV), f64(mean), f64(scale))
    assert np.array_equal(bits(z.cpu().numpy()), bits(R.apply(X, mean, scale)))
    assert not np.array_equal(z.cpu().numpy(), ((X.astype(np.float64) - mean) * (1.0 / scale)).astype(np.float32))


def test_standard_scaler_against_clustering_standardize():
    """one fp32 matrix, the product width: StandardScaler and clustering.standardize are EACH within the z bound of the yardstick's
    unrounded z (the stronger statement: they are then within twice the bound of each other).  The bound counts the kernel's
    n + 3 + splits additions; it holds for any summation whose longest path is no longer, which covers a float64 tree reduction --
    that clustering.standardize meets it is asserted here, not assumed."""
    case, arrs, X, (mean, var, scale) = problem("r1000")
    rows, F = X.shape
    Xd = torch.from_numpy(X.copy()).to(DEV)
    sc = clustering.StandardScaler()
    Z = sc.fit_transform(Xd)
    assert Z.dtype == torch.float32 and Z.shape == (rows, F) and Z.is_contiguous() and sc.n_samples_seen_ == rows
    for t in (sc.mean_, sc.var_, sc.scale_):
        assert t.dtype == torch.float64 and t.shape == (F,) and t.is_cuda
    tols = B.fit_tol(X, ops.standardize_fit_splits(rows, F))
    z64 = R.apply64(X, mean, scale)
    tol = B.z_tol(z64, scale, tols[0], tols[2])
    old = clustering.standardize(Xd)
    assert np.all(np.abs(Z.cpu().numpy().astype(np.float64) - z64) <= tol)
    assert np.all(np.abs(old.cpu().numpy().astype(np.float64) - z64) <= tol)
    # the same matrix as two column blocks gives the same bits: a column's result does not depend on the part it lies in
    Z2 = clustering.StandardScaler().fit_transform([Xd[:, :782], Xd[:, 782:]])
    assert torch.equal(Z2.view(torch.int32), Z.view(torch.int32))


def test_transform_of_other_rows():
    case, arrs, X, (mean, var, scale) = problem("r4099")
    sc = clustering.StandardScaler().fit(dev_parts(case.parts, arrs, case.rows))
    other = SC.other_rows(case, 37)
    Z = sc.transform(dev_parts(case.parts, other, 37))
    assert Z.shape == (37, X.shape[1])
    Xo = np.concatenate([np.broadcast_to(a, (37, a.shape[-1])) for a in other], axis=1).astype(np.float32)
    want = R.apply(Xo, sc.mean_.cpu().numpy(), sc.scale_.cpu().numpy())          # the device's own mean / scale: bit-equal
    assert np.array_equal(bits(Z.cpu().numpy()), bits(want))


def test_python_refusals():
    x = torch.zeros(6, 3, device=DEV)
    v = torch.zeros(3, dtype=torch.float64, device=DEV)
    sc = clustering.StandardScaler().fit(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.transform(x.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clustering.StandardScaler().fit([x, torch.zeros(6, 2)])
    with pytest.raises(ValueError):
        clustering.StandardScaler().fit([x] * 5)
    with pytest.raises(ValueError):
        clustering.StandardScaler().fit([x, torch.zeros(7, 3, device=DEV)])                   # mismatched row counts
    with pytest.raises(ValueError):
        clustering.StandardScaler().fit([torch.zeros(3, device=DEV)])                         # no matrix part
    with pytest.raises(ValueError):
        clustering.StandardScaler().fit(x.double())
    store = torch.zeros(6, 8, device=DEV)
    with pytest.raises(ValueError, match="shares its storage"):
        ops.standardize_apply([store[:, :3]], v, v, out=store[:, 4:7])
    with pytest.raises(ValueError):
        ops.standardize_apply([x], v[:2], v[:2])
    with pytest.raises(ValueError):
        ops.standardize_apply([torch.zeros(3, device=DEV)], v, v)                             # rows unknown
    assert ops.standardize_apply([torch.zeros(3, device=DEV)], v, v + 1, rows=4).shape == (4, 3)
