"""mmvae_silhouette_samples on the MI355X through ops and mmvae.clustering: a, b and s of every row within the derived bounds of
tests/silhouette_bounds.py around the float64 restatement of tests/silhouette_ref.py, for every decomposition (one split, the library's
choice, a forced count), run-to-run results exact.  Operands are views of wider NaN-filled buffers or padded bf16 rows with NaN pads,
the outputs are pre-filled with a sentinel inside wider buffers."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import silhouette_bounds as SB  # noqa: E402
import silhouette_ref as SR  # noqa: E402
from mmvae import _lib, clustering, ops  # noqa: E402
from rowmat_gpu_util import operand  # noqa: E402

DEV = "cuda"
SENTINEL = -7.0


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def launch(x, order, class_start, shift, splits=0):
    """one launch into sentinel-filled wider buffers; returns numpy (a, b, s) float32 and asserts that the frame is untouched"""
    N = x.shape[0]
    buf = torch.full((3, N + 5), SENTINEL, dtype=torch.float32, device=DEV)
    s, a, b = ops.silhouette_samples(x, order, class_start, shift, splits=splits, s_out=buf[0, 2:2 + N], intra_out=buf[1, 3:3 + N],
                                     inter_out=buf[2, 1:1 + N])
    torch.cuda.synchronize()
    frame = buf.clone()
    frame[0, 2:2 + N] = frame[1, 3:3 + N] = frame[2, 1:1 + N] = SENTINEL
    assert (frame == SENTINEL).all(), "a write outside s / intra / inter"
    return a.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    return SR.make_case(name)


@functools.lru_cache(maxsize=None)
def analysed(name, nsplit):
    c = case(name)
    return SB.analyse(c["x"], c["codes"], c["C"], c["shift"], nsplit)


def run_case(name, left=7, splits=1):
    c = case(name)
    x = operand(c["x"], c["bf16"], left)
    assert np.array_equal(x.detach().double().cpu().numpy(), c["x"].astype(np.float64))
    order, start = SR.grouping(c["codes"], c["C"])
    used = ops.silhouette_splits(len(c["x"]), c["C"], splits)
    a, b, s = launch(x, None if c["grouped"] else _dev(order), _dev(start), _dev(c["shift"]), splits)
    ra, rb = SB.check(analysed(name, used), a, b, s, label=f"{name} left {left} splits {splits} -> {used}")
    print(f"{name} left {left} splits {splits} -> {used}: errors at most {ra:.3f} (a), {rb:.3f} (b) of their bounds")
    return a, b, s


@pytest.mark.parametrize("left", [7, 8])            # 7: rows aligned to one element only (scalar loads); 8: 16-byte loads
@pytest.mark.parametrize("name", ["p77_f32", "p77_bf16"])
def test_partial_block_partial_tiles_odd_width_real_permutation(name, left):
    c = case(name)
    assert not np.array_equal(SR.grouping(c["codes"], c["C"])[0], np.arange(77))
    run_case(name, left)
    run_case(name, left, splits=0)


def test_singleton_exact_tile_tile_plus_one_and_every_split_path():
    c = case("c1000")
    assert sorted(np.bincount(c["codes"]).tolist()) == [1, 128, 129, 300, 442]
    assert ops.silhouette_splits(1000, 5, 0) > 1 and ops.silhouette_splits(1000, 5, 1) == 1 and ops.silhouette_splits(1000, 5, 3) == 3
    single = np.flatnonzero(np.bincount(c["codes"])[c["codes"]] == 1)
    for splits in (1, 0, 3):
        first = run_case("c1000", splits=splits)
        again = run_case("c1000", splits=splits)
        assert all(np.array_equal(u.view(np.int32), v.view(np.int32)) for u, v in zip(first, again)), f"splits {splits}: two runs differ"
        assert first[2][single] == 0 and first[0][single] == 0


def test_pairs_with_and_without_shift():
    a, b, s = run_case("pairs_shift")
    an_shift, an_none = analysed("pairs_shift", 1), analysed("pairs_noshift", 1)
    assert (an_shift["da"] / an_shift["a"]).max() <= 2e-5                # tight enough to see half a distance leak in from the diagonal
    run_case("pairs_noshift")
    # what the shift is for: its errors are far inside the bounds that hold without it
    assert (np.abs(a - an_shift["a"]) < 1e-2 * an_none["da"]).all() and (np.abs(b - an_shift["b"]) < 1e-2 * an_none["db"]).all()


def test_grouped_rows_without_order_equal_the_shuffled_rows_with_order():
    c = case("grouped")
    assert c["grouped"] and (np.diff(c["codes"]) >= 0).all()
    grouped = run_case("grouped")
    g = np.random.default_rng(9)
    perm = g.permutation(77)
    x = c["x"][perm]
    order, start = np.argsort(perm).astype(np.int32), SR.grouping(c["codes"], c["C"])[1]
    assert np.array_equal(x[order], c["x"])                                # the same rows at the same positions
    shuffled = launch(_dev(x), _dev(order), _dev(start), _dev(c["shift"]), 1)
    for u, v in zip(grouped, shuffled):
        assert np.array_equal(u[perm].view(np.int32), v.view(np.int32))


@pytest.mark.parametrize("splits", [1, 0])
def test_empty_class_in_the_middle_is_skipped(splits):
    c = case("empty_class")
    assert SR.grouping(c["codes"], c["C"])[1].tolist() == [0, 30, 30, 70, 90]
    a, b, s = run_case("empty_class", splits=splits)
    assert (b > 0).all()


def test_identical_rows():
    a, b, s = run_case("identical")
    an = analysed("identical", 1)
    assert (an["D"] == 0).all() and (an["a"] == 0).all() and (an["b"] == 0).all()
    assert np.isfinite(s).all() and (np.abs(s) <= 1).all()


def test_near_duplicates_without_shift_stay_finite():
    run_case("near_dup")
    run_case("near_dup", splits=0)


@pytest.mark.parametrize("splits", [1, 0])
def test_the_largest_class_count(splits):
    assert case("cmax")["C"] == _lib.SIL_MAXC
    run_case("cmax", splits=splits)


def test_smallest_sizes():
    run_case("n3")
    c = case("n3")
    s = clustering.silhouette_samples(_dev(c["x"]), c["codes"])
    assert s.shape == (3,) and s.dtype == torch.float32 and s[0].item() == 0.0
    with pytest.raises(ValueError, match="Number of labels is 2. Valid values are 2 to n_samples - 1"):
        clustering.silhouette_samples(_dev(c["x"][:2]), [0, 1])


def test_score_and_label_values():
    c = case("c1000")
    x = _dev(c["x"])
    an = SB.analyse(c["x"], c["codes"], c["C"], SR.column_means(c["x"]), ops.silhouette_splits(1000, 5, 0))
    score = clustering.silhouette_score(x, _dev(c["codes"]))
    assert isinstance(score, float)
    width = np.maximum(an["s_hi"] - an["s"], an["s"] - an["s_lo"]).mean()
    assert abs(score - SR.silhouette_score(c["x"], c["codes"])) <= width, (score, width)
    # any integer labels, as a tensor or an array: the values (3, 17, 40, ..) stand for their codes
    values = np.array([17, 3, 40, 5, 1000])
    s_codes = clustering.silhouette_samples(x, c["codes"])
    s_values = clustering.silhouette_samples(x, values[c["codes"]].astype(np.int32))
    ranks = np.argsort(np.argsort(values))                                   # the code of every value: only the class numbering changes
    assert np.array_equal(np.unique(values[c["codes"]], return_inverse=True)[1], ranks[c["codes"]])
    an2 = SB.analyse(c["x"], ranks[c["codes"]], c["C"], SR.column_means(c["x"]), ops.silhouette_splits(1000, 5, 0))
    lo, hi = np.minimum(an["s_lo"], an2["s_lo"]), np.maximum(an["s_hi"], an2["s_hi"])
    for s in (s_codes, s_values):
        s = s.double().cpu().numpy()
        assert ((s >= lo) & (s <= hi)).all()
    # labels in class order keep their codes: bit-identical
    s_sorted = clustering.silhouette_samples(x, (10 * c["codes"] + 3).astype(np.int64))
    assert torch.equal(s_codes, s_sorted)
    z = clustering.standardize(x)
    assert z.dtype == torch.float32 and z.is_contiguous() and np.abs(z.double().cpu().numpy() - SR.standardize(c["x"])).max() <= 1e-6


def test_operand_checks():
    x = torch.zeros(6, 3, device=DEV)
    start = torch.tensor([0, 3, 6], dtype=torch.int32, device=DEV)
    order = torch.arange(6, dtype=torch.int32, device=DEV)
    for bad in (lambda: ops.silhouette_samples(x.double(), order, start), lambda: ops.silhouette_samples(x, order.long(), start),
                lambda: ops.silhouette_samples(x, order[:5], start), lambda: ops.silhouette_samples(x, order, start.long()),
                lambda: ops.silhouette_samples(x, order, start, splits=65), lambda: ops.silhouette_samples(x, order, start[:1]),
                lambda: ops.silhouette_samples(x, order, start, torch.zeros(4, device=DEV)),
                lambda: ops.silhouette_samples(x, order, start, s_out=torch.zeros(5, device=DEV)),
                lambda: ops.silhouette_samples(x[:1], None, start)):
        with pytest.raises((ValueError, TypeError)):
            bad()
