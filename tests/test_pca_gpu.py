"""mmvae_pca_scatter, mmvae_pca_project and mmvae.pca.PCA on the MI355X: every element of S and of y within the derived bounds of
tests/pca_bounds.py around the float64 restatement of tests/pca_ref.py, S bitwise symmetric, every decomposition (one split, the
library's choice, a forced count) and run-to-run results exact, eigenvalues, components and span within their perturbation bounds.
Operands are views of wider NaN-filled buffers or padded bf16 rows with NaN pads, the outputs are views of sentinel-filled buffers."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pca_bounds as PB  # noqa: E402
import pca_ref as PR  # noqa: E402
from mmvae import _lib, ops  # noqa: E402
from mmvae.pca import PCA  # noqa: E402
from rowmat_gpu_util import in_nan_frame, operand  # noqa: E402

DEV = "cuda"
SENTINEL = -7.0


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def framed(rows, cols):
    """a (rows, cols) view inside a sentinel-filled buffer and the check that nothing but the view was written"""
    buf = torch.full((rows + 3, cols + 5), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[1:1 + rows, 2:2 + cols]

    def untouched():
        torch.cuda.synchronize()
        frame = buf.clone()
        frame[1:1 + rows, 2:2 + cols] = SENTINEL
        assert (frame == SENTINEL).all(), "a write outside the output"
    return view, untouched


def scatter(x, shift, splits=0):
    F = x.shape[1]
    out, untouched = framed(F, F)
    s = ops.pca_scatter(x, shift, splits, out=out)
    untouched()
    assert s.data_ptr() == out.data_ptr()
    return s.cpu().numpy()


def project(x, shift, v):
    out, untouched = framed(x.shape[0], v.shape[0])
    y = ops.pca_project(x, shift, v, out=out)
    untouched()
    return y.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    return PR.make_case(name)


@functools.lru_cache(maxsize=None)
def analysed(name):
    c = case(name)
    return PB.analyse(c["x"], c["k"])


def run_scatter(name, left=7, splits=0, shifted=True):
    c = case(name)
    x = operand(c["x"], c["bf16"], left)
    assert np.array_equal(x.detach().double().cpu().numpy(), c["x"].astype(np.float64))
    shift = c["shift"] if shifted else None
    N, F = c["x"].shape
    used = ops.pca_scatter_splits(N, F, splits)
    S = scatter(x, _dev(shift), splits)
    bad, ratio = PB.check_scatter(S, c["x"], shift, f"{name} left {left} splits {splits} -> {used}")
    print(f"{name} left {left} splits {splits} -> {used} {'shifted' if shifted else 'unshifted'}: scatter error at most {ratio:.3f} of its bound")
    assert bad == []
    return S


@pytest.mark.parametrize("left", [7, 8])            # 7: rows aligned to one element only (scalar loads); 8: 16-byte loads
@pytest.mark.parametrize("name", ["s77", "b77"])
def test_scatter_one_partial_tile_partial_chunk_odd_width(name, left):
    assert case(name)["x"].shape == (77, 37)
    one = run_scatter(name, left, splits=1)
    run_scatter(name, left, splits=0)
    three = run_scatter(name, left, splits=3)                # three chunks, one per split
    assert ops.pca_scatter_splits(77, 37, 3) == 3 and one.shape == three.shape == (37, 37)


def test_scatter_off_diagonal_tile_its_mirror_and_a_partial_second_column():
    assert case("k50")["x"].shape == (300, 200)
    for left in (7, 8):
        run_scatter("k50", left, splits=1)
    run_scatter("k50", 8, splits=4)


def test_scatter_tile_plus_one_column_and_every_split_path():
    assert case("s1000")["x"].shape == (1000, 129)
    assert ops.pca_scatter_splits(1000, 129, 1) == 1 and ops.pca_scatter_splits(1000, 129, 0) == 4 and ops.pca_scatter_splits(1000, 129, 3) == 3
    for splits in (1, 0, 3):
        first = run_scatter("s1000", splits=splits)
        again = run_scatter("s1000", splits=splits)
        assert np.array_equal(first.view(np.int32), again.view(np.int32)), f"splits {splits}: two runs differ"


def test_scatter_with_and_without_shift():
    c = case("n300")
    assert c["offset"] == 100.0
    shifted = run_scatter("n300")
    run_scatter("n300", shifted=False)
    # what the shift is for: its errors are far inside the bound that holds without it
    err = np.abs(shifted.astype(np.float64) - PR.scatter(c["x"], c["shift"]))
    assert (err <= 1e-3 * PB.scatter_bound(c["x"], None)).all()


@pytest.mark.parametrize("name", ["s77", "k50"])    # F = 37 and 200
def test_projection_within_its_bound(name):
    c = case(name)
    N, F = c["x"].shape
    g = np.random.default_rng(21)
    for k, left in ((1, 7), (2, 8), (50, 7), (64, 8)):
        v = np.linalg.qr(g.standard_normal((F, min(k, F))))[0].T
        if len(v) < k:                                       # F = 37: more rows than an orthonormal set has
            v = np.vstack([v, g.standard_normal((k - len(v), F)) / np.sqrt(F)])
        v = v.astype(np.float32)
        vd = in_nan_frame(v, 1, left, 5 if left == 7 else 64 - (left + F) % 64)
        y = project(operand(c["x"], c["bf16"], left), _dev(c["shift"]), vd)
        bad, ratio = PB.check_project(y, c["x"], c["shift"], v, f"{name} k {k}")
        print(f"{name} k {k} left {left}: projection error at most {ratio:.3f} of its bound")
        assert bad == [] and y.shape == (N, k)
    y0 = project(_dev(c["x"]), None, _dev(v))                # no shift
    assert PB.check_project(y0, c["x"], None, v, "no shift")[0] == []


def test_projection_row_bits_do_not_depend_on_position_n_or_ld():
    c = case("k50")
    x, shift = c["x"], _dev(c["shift"])
    v = _dev(np.linalg.qr(np.random.default_rng(22).standard_normal((200, 50)))[0].T.astype(np.float32))
    whole = project(_dev(x), shift, v)
    perm = np.random.default_rng(23).permutation(300)
    moved = project(in_nan_frame(x[perm], 2, 7, 3), shift, v)                   # other positions, another alignment and stride
    assert np.array_equal(moved.view(np.int32), whole[perm].view(np.int32))
    few = project(in_nan_frame(x[130:135], 1, 8, 0), shift, v)                  # N = 5: a row that sat in the second row block
    assert np.array_equal(few.view(np.int32), whole[130:135].view(np.int32))


def fit_case(name, left=8):
    c, an = case(name), analysed(name)
    x = operand(c["x"], c["bf16"], left)
    p = PCA(c["k"], random_state=42)
    y = p.fit_transform(x)
    torch.cuda.synchronize()
    got = dict(components=p.components_.cpu().numpy(), explained_variance=p.explained_variance_.cpu().numpy(),
               explained_variance_ratio=p.explained_variance_ratio_.cpu().numpy(), singular_values=p.singular_values_.cpu().numpy())
    assert p.components_.dtype == torch.float32 and p.components_.shape == (c["k"], c["x"].shape[1]) and y.dtype == torch.float32
    assert (p.n_samples_, p.n_features_in_, p.n_components_) == (*c["x"].shape, c["k"])
    # the float64 column mean rounded to fp32 (torch's float64 sum may end one rounding away from numpy's)
    assert (np.abs(p.mean_.cpu().numpy() - c["shift"]) <= np.spacing(np.abs(c["shift"]))).all()
    bad, ratios = PB.check_fit(an, got, c["per_component"], name)
    b2, ratios["projection"] = PB.check_project(y.cpu().numpy(), c["x"], c["shift"], got["components"], name)
    if c["per_component"]:
        b3, ratios["end to end"] = PB.check_end_to_end(an, y.cpu().numpy(), got["components"], name)
        bad += b3
    print(f"{name}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + " of their bounds")
    assert bad + b2 == []
    # fit then transform: the same bits
    y2 = PCA(c["k"]).fit(x).transform(x)
    assert torch.equal(y, y2)
    return p, y


@pytest.mark.parametrize("name", ["n300", "s1000"])
def test_pca_components_variances_and_transform(name):
    assert (analysed(name)["sin"] <= PB.MAX_COMPONENT_BOUND).all()
    fit_case(name)


def test_pca_fewer_rows_than_features():
    c = case("n40")
    assert c["x"].shape[0] < c["x"].shape[1] and (analysed("n40")["sin"] <= PB.MAX_COMPONENT_BOUND).all()
    fit_case("n40", left=7)
    with pytest.raises(ValueError, match=r"n_components=41 must be between 0 and min\(n_samples, n_features\)=40 with svd_solver='full'"):
        PCA(41).fit(_dev(c["x"]))
    with pytest.raises(ValueError):
        PCA(1).fit(_dev(c["x"][:1]))


def test_pca_fifty_components_by_eigenvalues_span_and_orthonormality():
    assert analysed("k50")["span"] <= PB.MAX_SPAN_BOUND and case("k50")["k"] == 50
    fit_case("k50")


def test_pca_bf16_storage_gives_the_bits_of_the_same_values_as_fp32():
    c = case("b77")
    p16, y16 = fit_case("b77", left=8)                       # padded bf16 rows, NaN pads
    p32 = PCA(c["k"])
    y32 = p32.fit_transform(_dev(c["x"]))
    assert torch.equal(y16, y32) and torch.equal(p16.components_, p32.components_)
    assert torch.equal(p16.explained_variance_ratio_, p32.explained_variance_ratio_)
    y16b = PCA(c["k"]).fit_transform(in_nan_frame(c["x"], 2, 7, 3, torch.bfloat16))            # bf16 rows aligned to one element
    assert torch.equal(y16b, y32)


def test_operand_checks():
    x = torch.zeros(6, 3, device=DEV)
    c, v = torch.zeros(3, device=DEV), torch.zeros(2, 3, device=DEV)
    for bad in (lambda: ops.pca_scatter(x.double(), c), lambda: ops.pca_scatter(x, c[:2]), lambda: ops.pca_scatter(x, c.double()),
                lambda: ops.pca_scatter(x, c, splits=65), lambda: ops.pca_scatter(x, c, out=torch.zeros(3, 4, device=DEV)),
                lambda: ops.pca_project(x, c, v[:, :2]), lambda: ops.pca_project(x, c, v.bfloat16()),
                lambda: ops.pca_project(x, c, torch.zeros(_lib.PCA_MAXK + 1, 3, device=DEV)),
                lambda: ops.pca_project(x, c, v, out=torch.zeros(6, 3, device=DEV)), lambda: PCA(2).fit(x).transform(x[:, :2])):
        with pytest.raises((ValueError, TypeError)):
            bad()
