"""The caller-owned workspace of include/mmvae_hip.h on the MI355X: every entry point that takes `work` / `work_bytes` or `slab` /
`slab_elems` needs no more than its planner says, assumes nothing about the contents and writes nothing outside.

Per entry and case: (a) `need` from the planner; (b) one run through the ordinary wrapper, held against the float64 restatement and the
derived bounds the entry's own test file uses; (c) runs on a guarded workspace (tests/workspace_util.py) of exactly `need` bytes, 8 bytes
aligned and no more, under three fills -- 0x00 (adversarial for the k-NN lists: distance 0, index 0 wins every selection; benign for fp32
partial sums), 0xFF (NaN for the sums; the lists' own empty sentinel) and the stale work region of a larger problem of the same entry
(plausible partials); (d) every output bit-identical to (b); (e) both guards intact; (f) the outputs lie in wider NaN / sentinel
filled buffers whose padding stays as it was.  Then, from a work region of 0xA5: the first and the last 4-byte word the header's formula
assigns to data have changed (the planner's last byte is used, so a write one word further would reach the guard), and the raw entry
with work_bytes = need - 8 answers MMVAE_ERR_ARG and leaves outputs, work region and guards as they were."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import downstream_bounds as DB  # noqa: E402
import knn_bounds as KB  # noqa: E402
import knn_l1_bounds as LB  # noqa: E402
import knn_ref as KR  # noqa: E402
import pca_bounds as PB  # noqa: E402
import pca_ref as PR  # noqa: E402
import silhouette_bounds as SB  # noqa: E402
import silhouette_ref as SR  # noqa: E402
import tsne_bounds as TB  # noqa: E402
import tsne_ref as TR  # noqa: E402
from mmvae import _lib, ops  # noqa: E402
from rowmat_gpu_util import operand  # noqa: E402
from workspace_util import GUARD_BYTE, guarded  # noqa: E402

DEV = "cuda"
SENTINEL_I = -77
A5 = bytes([GUARD_BYTE])


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def up8(n):
    return (n + 7) // 8 * 8


class Frame:
    """a (rows, cols) output view inside a wider buffer filled with NaN (int32: a sentinel)"""

    def __init__(self, rows, cols, dtype=torch.float32, top=1, left=2, right=3, bottom=1):
        self.fill = SENTINEL_I if dtype == torch.int32 else float("nan")
        self.buf = torch.full((top + rows + bottom, left + cols + right), self.fill, dtype=dtype, device=DEV)
        self.where = (slice(top, top + rows), slice(left, left + cols))
        self.view = self.buf[self.where]

    def _is_fill(self, t):
        return bool((t.contiguous().view(torch.int32) == torch.full((1,), self.fill, dtype=t.dtype, device=DEV).view(torch.int32)).all())

    def untouched(self):
        """nothing but the view was written"""
        b = self.buf.clone()
        b[self.where] = self.fill
        assert self._is_fill(b), "a write outside the output view"

    def reset(self):
        self.buf.fill_(self.fill)

    def all_fill(self):
        return self._is_fill(self.buf)


def vec_frame(n, dtype=torch.float32):
    """a unit-stride (n,) view inside a filled buffer"""
    f = Frame(1, n, dtype, top=0, left=4, right=3, bottom=0)
    return f, f.view[0]


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


class Recorder:
    """the library with every call recorded: (symbol, arguments)"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


def run_contract(label, symbol, call, need, check_ref, stale, data_words, monkeypatch):
    """call(work) -> (outputs, frames, operands written in place): one run of the wrapper into fresh output frames.
    check_ref(outputs): the float64 restatement and its bounds.  stale(): the work region a larger problem left.  data_words: byte
    offsets of the first and the last 4-byte word of the workspace that the header's formula assigns to data."""
    want, frames, _ = call(None)                                                       # (b)
    torch.cuda.synchronize()
    for f in frames:
        f.untouched()
    check_ref(want)
    if need == 0:
        # the zero-workspace form: work may be NULL (above); a workspace that is given all the same is not touched
        g = guarded(8, "ones", DEV)
        got, frames, _ = call(g.tensor)
        torch.cuda.synchronize()
        assert all(torch.equal(bits(u), bits(v)) for u, v in zip(got, want)), (label, "a workspace that is not needed changed the result")
        assert bool((g.work == 0xFF).all()), (label, "a workspace that is not needed was written")
        g.check(label)
        return
    for fill in ("zero", "ones", "stale"):                                             # (c)
        g = guarded(need, stale() if fill == "stale" else fill, DEV)
        got, frames, _ = call(g.tensor)
        torch.cuda.synchronize()
        for i, (u, v) in enumerate(zip(got, want)):                                    # (d)
            assert torch.equal(bits(u), bits(v)), (label, f"output {i} depends on the workspace's contents: fill {fill}")
        g.check(f"{label}, fill {fill}")                                               # (e)
        for f in frames:                                                               # (f)
            f.untouched()
    # the checker sees writes: from 0xA5 the first and the last data word change
    g = guarded(need, A5, DEV)
    before = g.image()
    rec = Recorder(_lib.load())
    with monkeypatch.context() as m:
        m.setattr(ops.L, "load", lambda: rec)
        got, frames, inplace = call(g.tensor)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(u), bits(v)) for u, v in zip(got, want)), (label, "fill 0xA5")
    g.check(f"{label}, fill 0xA5")
    first, last = data_words
    assert 0 <= first <= last <= need - 4
    assert g.word_changed(first, before), (label, f"the first data word (byte {first}) was not written")
    assert g.word_changed(last, before), (label, f"the last data word (byte {last} of {need}) was not written")
    # a refused call writes nothing: the same arguments with work_bytes = need - 8 on the raw entry
    mine = [(name, args) for name, args in rec.calls if name == symbol]
    assert len(mine) == 1, (label, [name for name, _ in rec.calls])
    good = mine[0][1][0]._obj
    a = type(good).from_buffer_copy(good)
    inner = a.base if hasattr(a, "base") else a
    assert inner.work == g.ptr and inner.work_bytes == need
    inner.work_bytes = need - 8
    for f in frames:
        f.reset()
    kept = [t.clone() for t in inplace]
    g.fill("ones")
    whole = g.buf.clone()
    assert getattr(_lib.load(), symbol)(C.byref(a), None) == -1, (label, "a workspace 8 bytes short was accepted")   # MMVAE_ERR_ARG
    torch.cuda.synchronize()
    assert all(f.all_fill() for f in frames), (label, "the refused call wrote an output")
    assert all(torch.equal(bits(u), bits(v)) for u, v in zip(inplace, kept)), (label, "the refused call wrote an operand")
    assert torch.equal(g.buf, whole), (label, "the refused call wrote the workspace or a guard")


def stale_image(run, larger, *key):
    """the work region after `run(*larger)` on a guarded workspace that started as 0xFF, as host bytes"""
    return _stale_image(run, larger, key)


@functools.lru_cache(maxsize=None)
def _stale_image(run, larger, key):
    g = run(*larger)
    torch.cuda.synchronize()
    g.check(f"stale run {larger}")
    return g.image().cpu()


# ---------------------------------------------------------------------------------------------------------------------------
# k nearest neighbours: euclidean, manhattan, grouped
# ---------------------------------------------------------------------------------------------------------------------------
KNN_F = 16
KNN_SIZES = [(5, 100), (3, 5000), (130, 700)]          # by workspace size; the stale fill of the last comes from (260, 700)


def knn_larger(Mq, Nt):
    i = KNN_SIZES.index((Mq, Nt))
    return KNN_SIZES[i + 1] if i + 1 < len(KNN_SIZES) else (2 * Mq, Nt)


@functools.lru_cache(maxsize=None)
def knn_data(seed, Mq, Nt, bf16):
    g = np.random.default_rng(1000 * seed + Mq + Nt)
    q = (1.0 + g.standard_normal((Mq, KNN_F))).astype(np.float32)
    t = (1.0 + g.standard_normal((Nt, KNN_F))).astype(np.float32)
    return q, (KR.to_bf16(t) if bf16 else t)


def knn_need(Mq, Nt, k, l1):
    """the header's formula: 4 (Mq + Nt) rounded up to 8 for the norms (euclidean) + 8 Mq k splits when split"""
    ns = ops.knn_splits(Mq, Nt)[0]
    return (0 if l1 else up8(4 * (Mq + Nt))) + (8 * Mq * k * ns if ns > 1 else 0), ns


def knn_words(Mq, Nt, k, l1, tail=0):
    need, ns = knn_need(Mq, Nt, k, l1)
    if tail:
        return 0, need + tail - 4
    return 0, (need - 4 if ns > 1 else 4 * (Mq + Nt) - 4)


def knn_run(l1, Mq, Nt, k, bf16, seed, work):
    q, t = knn_data(seed, Mq, Nt, bf16)
    qd, td = operand(q, False, 7), operand(t, bf16, 8 if bf16 else 7)
    fi, fd = Frame(Mq, k, torch.int32), Frame(Mq, k)
    if l1:
        idx, d = ops.knn_search_l1(qd, td, k, idx_out=fi.view, dist_out=fd.view, work=work)
    else:
        shift = dev(t.astype(np.float64).mean(axis=0).astype(np.float32))
        idx, d = ops.knn_search(qd, td, k, shift, idx_out=fi.view, dist2_out=fd.view, work=work)
    return [idx, d], [fi, fd], []


def knn_stale_run(l1, Mq, Nt, k, bf16):
    g = guarded((ops.knn_l1_work_bytes if l1 else ops.knn_work_bytes)(Mq, Nt, k), "ones", DEV)
    knn_run(l1, Mq, Nt, k, bf16, 2, g.tensor)
    return g


@functools.lru_cache(maxsize=None)
def knn_analysis(l1, Mq, Nt, k, bf16):
    q, t = knn_data(1, Mq, Nt, bf16)
    return LB.analyse(q, t, k) if l1 else KB.analyse(q, t, k, t.astype(np.float64).mean(axis=0).astype(np.float32))


def knn_cases(ks):
    return [(Mq, Nt, k) for Mq, Nt in KNN_SIZES for k in ks if k <= Nt]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("Mq,Nt,k", knn_cases((1, 5, 17, 96)))
def test_knn_search(Mq, Nt, k, bf16, monkeypatch):
    need, ns = knn_need(Mq, Nt, k, False)
    assert ops.knn_work_bytes(Mq, Nt, k) == need
    assert (ns > 1) == ((Mq, Nt) != (5, 100))                                          # (3, 5000): 40 tiles; (130, 700): two query blocks of six tiles
    if (Mq, Nt) == (3, 5000):
        assert -(-Nt // 128) == 40 and Nt % 128 == 8 and ns > 1
    if ns == 1:
        assert need == up8(4 * (Mq + Nt))                                              # the norms alone
    q, t = knn_data(1, Mq, Nt, bf16)
    shift = t.astype(np.float64).mean(axis=0).astype(np.float32)

    def check_ref(out):
        KB.check_search(q, t, k, out[0].cpu().numpy(), out[1].cpu().numpy(), shift, label=f"knn {Mq} {Nt} {k}", an=dict(knn_analysis(False, Mq, Nt, k, bf16)))
    run_contract(f"knn_search Mq{Mq} Nt{Nt} k{k} {'bf16' if bf16 else 'f32'}", "mmvae_knn_search",
                 lambda work: knn_run(False, Mq, Nt, k, bf16, 1, work), need, check_ref,
                 lambda: stale_image(knn_stale_run, (False, *knn_larger(Mq, Nt), k, bf16)), knn_words(Mq, Nt, k, False), monkeypatch)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("Mq,Nt,k", knn_cases((5, 17)))
def test_knn_search_l1(Mq, Nt, k, bf16, monkeypatch):
    need, ns = knn_need(Mq, Nt, k, True)
    assert ops.knn_l1_work_bytes(Mq, Nt, k) == need and (need == 0) == (ns == 1) == ((Mq, Nt) == (5, 100))
    q, t = knn_data(1, Mq, Nt, bf16)

    def check_ref(out):
        idx, d = out[0].cpu().numpy().astype(np.int64), out[1].cpu().numpy()
        eidx, ed = LB.emulate(q, t, k)
        assert np.array_equal(d.view(np.uint32), ed.view(np.uint32)) and np.array_equal(idx, eidx)
        an = KB.check_search(q, t, k, idx, None, label=f"knn_l1 {Mq} {Nt} {k}", an=dict(knn_analysis(True, Mq, Nt, k, bf16)))
        LB.check_dist(an, idx, d, label="knn_l1")
    run_contract(f"knn_search_l1 Mq{Mq} Nt{Nt} k{k} {'bf16' if bf16 else 'f32'}", "mmvae_knn_search_l1",
                 lambda work: knn_run(True, Mq, Nt, k, bf16, 1, work), need, check_ref,
                 lambda: stale_image(knn_stale_run, (True, *knn_larger(Mq, Nt), k, bf16)), knn_words(Mq, Nt, k, True) if need else None, monkeypatch)


INT_MIN = -2147483648


@functools.lru_cache(maxsize=None)
def group_codes(Mq, Nt):
    """(q_same, t_same, q_differ, t_differ) int32, after tests/test_knn_grouped_gpu.py: candidates sorted by their `same` code so that
    whole tiles (with 3 queries whole splits) hold no admitted pair and are skipped, a group of three candidates (lists of 3 at k = 5
    and 17), a query code no candidate carries (an empty list), INT32_MIN and a negative code; `differ` codes that are constant over a
    tile and over a query block, so that the differ rule skips tiles too."""
    ts = np.full(Nt, 2_000_000_000, np.int32)
    ts[:Nt * 3 // 7] = -5
    ts[-3:] = INT_MIN
    td = (np.arange(Nt) // 128).astype(np.int32)
    if Mq == 3:
        qs, qd = np.array([-5, INT_MIN, 7], np.int32), np.array([1, 1, 1], np.int32)
        td = np.where(np.arange(Nt) < 1280, 1, 2 + np.arange(Nt) % 3).astype(np.int32)      # tiles 0 .. 9 carry the block's one code
    else:
        qs = np.full(Mq, -5, np.int32)
        qs[128:] = [INT_MIN, 7][:Mq - 128]                                                # the second block: a short and an empty list
        qd = np.where(np.arange(Mq) < 128, 0, Nt // 128).astype(np.int32)                 # block 0 skips tile 0, block 1 the last tile
    return qs, ts, qd, td


def group_run(metric, mode, Mq, Nt, k, seed, work, codes=None):
    q, t = knn_data(seed, Mq, Nt, False)
    qs, ts, qd, td = codes or group_codes(Mq, Nt)
    same = (dev(qs), dev(ts)) if mode in ("same", "both") else None
    differ = (dev(qd), dev(td)) if mode in ("differ", "both") else None
    shift = dev(t.astype(np.float64).mean(axis=0).astype(np.float32)) if metric == "euclidean" else None
    fi, fd = Frame(Mq, k, torch.int32), Frame(Mq, k)
    idx, d = ops.knn_search_grouped(operand(q, False, 7), operand(t, False, 7), k, same=same, differ=differ, metric=metric, shift=shift,
                                    idx_out=fi.view, dist_out=fd.view, work=work)
    return [idx, d], [fi, fd], []


def group_stale_run(metric, mode, Mq, Nt, k):
    g = guarded(ops.knn_group_work_bytes(Mq, Nt, k, metric), "ones", DEV)
    r = np.random.default_rng(Mq + Nt)                                                # other data and other codes: every tile is walked
    codes = (r.integers(0, 3, Mq).astype(np.int32), r.integers(0, 3, Nt).astype(np.int32), r.integers(0, 4, Mq).astype(np.int32),
             r.integers(0, 4, Nt).astype(np.int32))
    group_run(metric, mode, Mq, Nt, k, 2, g.tensor, codes)
    return g


def group_check(metric, mode, Mq, Nt, k, idx, d):
    """every group of queries that see the same candidates: the float64 analysis of the plain search over those candidates (knn_bounds /
    knn_l1_bounds; manhattan: the bits of the sequential chain too), indices mapped back, -1 / +inf behind a short list"""
    q, t = knn_data(1, Mq, Nt, False)
    qs, ts, qd, td = group_codes(Mq, Nt)
    use_s, use_d = mode in ("same", "both"), mode in ("differ", "both")
    shift = t.astype(np.float64).mean(axis=0).astype(np.float32) if metric == "euclidean" else None
    short = skipped = 0
    for cs, cd in sorted(set(zip(qs.tolist() if use_s else [0] * Mq, qd.tolist() if use_d else [0] * Mq))):
        rows = np.flatnonzero((qs == cs if use_s else True) & (qd == cd if use_d else np.ones(Mq, bool)))
        adm = (ts == cs if use_s else np.ones(Nt, bool)) & (td != cd if use_d else np.ones(Nt, bool))
        cand = np.flatnonzero(adm)
        c = min(k, len(cand))
        short += c < k
        skipped += sum(not adm[s:s + 128].any() for s in range(0, Nt, 128))
        gi, gd = idx[rows], d[rows]
        assert (gi[:, c:] == -1).all() and np.isposinf(gd[:, c:]).all(), (metric, mode, cs, cd, "the tail of a short list")
        if c == 0:
            continue
        assert np.isin(gi[:, :c], cand).all(), (metric, mode, cs, cd, "a candidate the predicate does not admit")
        local = np.searchsorted(cand, gi[:, :c])
        if metric == "euclidean":
            KB.check_search(q[rows], t[cand], c, local, gd[:, :c], shift, label=f"grouped {mode} {cs} {cd}")
        else:
            eidx, ed = LB.emulate(q[rows], t[cand], c)
            assert np.array_equal(local, eidx) and np.array_equal(gd[:, :c].view(np.uint32), ed.view(np.uint32)), (mode, cs, cd)
            LB.check_dist(KB.check_search(q[rows], t[cand], c, local, None, label=f"grouped l1 {mode}", an=LB.analyse(q[rows], t[cand], c)), local, gd[:, :c])
    assert skipped > 0, "the codes must let whole tiles be skipped"
    assert mode == "differ" or short >= 2, "the codes must give a short and an empty list"


@pytest.mark.parametrize("mode", ["same", "differ", "both"])
@pytest.mark.parametrize("metric", ["euclidean", "manhattan"])
@pytest.mark.parametrize("Mq,Nt,k", [(Mq, Nt, k) for Mq, Nt in KNN_SIZES[1:] for k in (5, 17)])
def test_knn_search_grouped(Mq, Nt, k, metric, mode, monkeypatch):
    l1 = metric == "manhattan"
    base, ns = knn_need(Mq, Nt, k, l1)
    codes = 16 * -(-Nt // 128)
    need = ops.knn_group_work_bytes(Mq, Nt, k, metric)
    assert ns > 1 and need == base + codes == (ops.knn_l1_work_bytes if l1 else ops.knn_work_bytes)(Mq, Nt, k) + codes

    def check_ref(out):
        group_check(metric, mode, Mq, Nt, k, out[0].cpu().numpy().astype(np.int64), out[1].cpu().numpy())
    larger = knn_larger(Mq, Nt)
    run_contract(f"knn_search_grouped {metric} {mode} Mq{Mq} Nt{Nt} k{k}", "mmvae_knn_search_grouped",
                 lambda work: group_run(metric, mode, Mq, Nt, k, 1, work), need, check_ref,
                 lambda: stale_image(group_stale_run, (metric, mode, *larger, k)), knn_words(Mq, Nt, k, l1, tail=codes), monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------
# silhouette
# ---------------------------------------------------------------------------------------------------------------------------
SIL_F = 10


def sil_sizes(N, C):
    """unequal classes, one of a single member and one larger than 128"""
    sizes = {2: [1], 3: [1, 150], 7: [1, 5, 17, 33, 40, 64]}[C]
    return sizes + [N - sum(sizes)]


@functools.lru_cache(maxsize=None)
def sil_data(seed, N, C):
    g = np.random.default_rng(100 * seed + N + C)
    codes = g.permutation(np.repeat(np.arange(C), sil_sizes(N, C)))
    x = (g.standard_normal((N, SIL_F)) + 1.5 * g.standard_normal((C, SIL_F))[codes]).astype(np.float32)
    return x, codes, SR.column_means(x)


@functools.lru_cache(maxsize=None)
def sil_analysis(N, C, used):
    x, codes, shift = sil_data(1, N, C)
    return SB.analyse(x, codes, C, shift, used)


def sil_run(N, C, splits, seed, work):
    x, codes, shift = sil_data(seed, N, C)
    order, start = SR.grouping(codes, C)
    fs, fa, fb = vec_frame(N), vec_frame(N), vec_frame(N)
    s, a, b = ops.silhouette_samples(operand(x, False, 7), dev(order), dev(start), dev(shift), splits=splits, s_out=fs[1], intra_out=fa[1],
                                     inter_out=fb[1], work=work)
    return [s, a, b], [fs[0], fa[0], fb[0]], []


def sil_stale_run(N, C, splits):
    g = guarded(ops.silhouette_work_bytes(N, C, splits), "ones", DEV)
    sil_run(N, C, splits, 2, g.tensor)
    return g


@pytest.mark.parametrize("splits", [0, 1, 2, 5])
@pytest.mark.parametrize("C", [2, 3, 7])
@pytest.mark.parametrize("N", [300, 1000])
def test_silhouette_samples(N, C, splits, monkeypatch):
    sizes = sil_sizes(N, C)
    assert min(sizes) == 1 and max(sizes) > 128 and len(set(sizes)) == C
    used = ops.silhouette_splits(N, C, splits)
    bound = min(N, (N + 127 * C) // 128)                                               # the header's bound of the number of column tiles
    assert used == min(splits if splits else 64, bound) and (used > 1) == (splits != 1)      # 0: below 1024 row blocks the tiles are split
    need = ops.silhouette_work_bytes(N, C, splits)
    assert need == up8(4 * N) + (4 * N * C * used if used > 1 else 0)

    def check_ref(out):
        s, a, b = (v.cpu().numpy() for v in out)
        SB.check(sil_analysis(N, C, used), a, b, s, label=f"silhouette N{N} C{C} splits {splits} -> {used}")
    run_contract(f"silhouette_samples N{N} C{C} splits {splits} -> {used}", "mmvae_silhouette_samples",
                 lambda work: sil_run(N, C, splits, 1, work), need, check_ref,
                 lambda: stale_image(sil_stale_run, (1000, C, splits) if N == 300 else (2000, C, splits)),
                 (0, need - 4 if used > 1 else 4 * N - 4), monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------
# PCA: the scatter matrix
# ---------------------------------------------------------------------------------------------------------------------------
PCA_CASES = [(257, 40), (257, 130), (257, 300), (1000, 40), (1000, 130), (1000, 300)]      # by workspace size


@functools.lru_cache(maxsize=None)
def pca_data(seed, N, F):
    g = np.random.default_rng(10 * seed + N + F)
    x = (g.standard_normal((N, F)) * (0.5 + g.random(F)) + 3.0 * g.standard_normal(F)).astype(np.float32)
    return x, PR.column_means(x)


def pca_run(N, F, splits, seed, work):
    x, shift = pca_data(seed, N, F)
    f = Frame(F, F)
    s = ops.pca_scatter(operand(x, False, 7), dev(shift), splits, out=f.view, work=work)
    return [s], [f], []


def pca_stale_run(N, F, splits):
    g = guarded(ops.pca_scatter_work_bytes(N, F, splits), "ones", DEV)
    pca_run(N, F, splits, 2, g.tensor)
    return g


@pytest.mark.parametrize("splits", [0, 1, 3])
@pytest.mark.parametrize("N,F", PCA_CASES)
def test_pca_scatter(N, F, splits, monkeypatch):
    T = -(-F // 128)
    pairs = T * (T + 1) // 2
    assert pairs == {40: 1, 130: 3, 300: 6}[F]
    used = ops.pca_scatter_splits(N, F, splits)
    assert used == PR.splits_used(N, F, splits)[0] == {(1000, 0): 4, (257, 0): 1}.get((N, splits), splits)
    need = ops.pca_scatter_work_bytes(N, F, splits)
    assert need == (65536 * pairs * used if used > 1 else 0)
    x, shift = pca_data(1, N, F)

    def check_ref(out):
        S = out[0].cpu().numpy()
        assert np.array_equal(S, S.T), "the two triangles differ"
        bad, _ = PB.check_scatter(S, x, shift, f"pca_scatter N{N} F{F} splits {splits} -> {used}")
        assert bad == []
    i = PCA_CASES.index((N, F))
    larger = PCA_CASES[i + 1] if i + 1 < len(PCA_CASES) else (2 * N, F)
    run_contract(f"pca_scatter N{N} F{F} splits {splits} -> {used}", "mmvae_pca_scatter", lambda work: pca_run(N, F, splits, 1, work), need,
                 check_ref, lambda: stale_image(pca_stale_run, (*larger, max(splits, 2))), (0, need - 4) if need else None, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------
# t-SNE: gradient and update
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tsne_data(seed, N):
    """(Y fp32 (N, 2), the symmetric CSR P of a k = 5 neighbour graph with uniform conditional probabilities)"""
    g = np.random.default_rng(seed + N)
    X = g.standard_normal((N, 4)) + 2.0 * g.standard_normal((3, 4))[np.arange(N) % 3]
    idx, _ = TR.neighbours(X, 5)
    row_ptr, col, val = TR.symmetric_csr(idx, np.full((N, 5), 0.2))
    return (2.0 * g.standard_normal((N, 2))).astype(np.float32), row_ptr, col, val.astype(np.float32)


@functools.lru_cache(maxsize=None)
def tsne_bounds(N, used):
    Y, row_ptr, col, val = tsne_data(1, N)
    return TB.gradient_bounds(Y, row_ptr, col, val, 12.0, used)


def tsne_grad_run(N, splits, seed, work):
    Y, row_ptr, col, val = tsne_data(seed, N)
    f = Frame(N, 2, left=0, right=0)
    grad, Z, err, zr = ops.tsne_gradient(dev(Y), dev(row_ptr.astype(np.int32)), dev(col.astype(np.int32)), dev(val), 12.0, error=True, z_row=True,
                                         splits=splits, grad_out=f.view, work=work)
    return [grad, Z, err, zr], [f], []


def tsne_grad_stale_run(N, splits):
    g = guarded(ops.tsne_gradient_work_bytes(N, splits), "ones", DEV)
    tsne_grad_run(N, splits, 2, g.tensor)
    return g


@pytest.mark.parametrize("splits", [0, 1, 3])
@pytest.mark.parametrize("N", [700, 1500])
def test_tsne_gradient(N, splits, monkeypatch):
    blocks = -(-N // 512)
    assert blocks == {700: 2, 1500: 3}[N] and N % 512                                 # row blocks of 512, the last one ragged
    used = ops.tsne_gradient_splits(N, splits)
    assert used == (TB.splits_used(N, splits) if splits else TB.splits_used(N, -(-2048 // blocks))) and (used > 1) == (splits != 1)
    need = ops.tsne_gradient_work_bytes(N, splits)
    assert need == up8(12 * N * used) + up8(4 * used * blocks)

    def check_ref(out):
        grad, Z, err, zr = out
        TB.check_gradient(tsne_bounds(N, used), grad.double().cpu().numpy(), float(Z), float(err.double().sum()), zr.double().cpu().numpy(),
                          label=f"tsne_gradient N{N} splits {splits} -> {used}")
    run_contract(f"tsne_gradient N{N} splits {splits} -> {used}", "mmvae_tsne_gradient", lambda work: tsne_grad_run(N, splits, 1, work), need,
                 check_ref, lambda: stale_image(tsne_grad_stale_run, (1500 if N == 700 else 3000, splits)),
                 (0, up8(12 * N * used) + 4 * used * blocks - 4), monkeypatch)


@functools.lru_cache(maxsize=None)
def update_data(seed, N):
    g = np.random.default_rng(seed + N)
    y = g.standard_normal((N, 2)).astype(np.float32)
    upd = (1e-2 * g.standard_normal((N, 2))).astype(np.float32)
    gains = (0.01 + 3.0 * g.random((N, 2)) ** 3).astype(np.float32)
    grad = (1e-4 * g.standard_normal((N, 2))).astype(np.float32)
    return y, upd, gains, grad


def update_run(N, seed, work, grad_norm=True):
    y, upd, gains, grad = (dev(v) for v in update_data(seed, N))
    norm = ops.tsne_update(y, upd, gains, grad, 0.8, 200.0, grad_norm=grad_norm, work=work)
    return [y, upd, gains] + ([norm] if grad_norm else []), [], [y, upd, gains]


def update_stale_run(N):
    g = guarded(ops.tsne_update_work_bytes(N), "ones", DEV)
    update_run(N, 2, g.tensor)
    return g


@pytest.mark.parametrize("N", [2, 700])
def test_tsne_update(N, monkeypatch):
    blocks = -(-2 * N // 256)
    assert blocks == {2: 1, 700: 6}[N]                                                # 700: more than one workgroup adds to the norm
    need = ops.tsne_update_work_bytes(N)
    assert need == up8(4 * blocks)
    y, upd, gains, grad = update_data(1, N)
    b = TB.update_bounds(y, upd, gains, grad, float(np.float32(0.8)), 200.0)
    assert not b["exempt"].any()

    def check_ref(out):
        bad = TB.update_outside(b, *(v.cpu().numpy() for v in out[:3]), float(out[3]))
        assert not bad, bad
    run_contract(f"tsne_update N{N}", "mmvae_tsne_update", lambda work: update_run(N, 1, work), need, check_ref,
                 lambda: stale_image(update_stale_run, (700 if N == 2 else 1400,)), (0, 4 * blocks - 4), monkeypatch)
    # without grad_norm no workspace is needed: one that is given all the same stays as it was
    want, _, _ = update_run(N, 1, None, grad_norm=False)
    g = guarded(need, "ones", DEV)
    got, _, _ = update_run(N, 1, g.tensor, grad_norm=False)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(u), bits(v)) for u, v in zip(got, want))
    assert bool((g.work == 0xFF).all()), "tsne_update without grad_norm wrote its workspace"
    g.check("tsne_update without grad_norm")


# ---------------------------------------------------------------------------------------------------------------------------
# the site classifier: LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------------
LN_CASES = [(32, 128), (33, 72), (65, 1024), (300, 520)]                               # by workspace size


@functools.lru_cache(maxsize=None)
def ln_data(seed, M, N):
    g = np.random.default_rng(1000 * M + N + seed)
    z = (1.5 + 2 * g.standard_normal((M, N))).astype(np.float32)
    gamma, beta = (1 + 0.3 * g.standard_normal(N)).astype(np.float32), (0.3 * g.standard_normal(N)).astype(np.float32)
    keep = (g.random((M, N)) >= 0.3).astype(np.uint8)
    dy = g.standard_normal((M, N)).astype(np.float32)
    zt, gt, bt, kt = dev(z), dev(gamma), dev(beta), dev(keep)
    _, mean, rstd = ops.ln_act_fwd(zt, gt, bt, kt, 0.3)
    torch.cuda.synchronize()
    return (z, gamma, beta, keep, dy, mean.cpu().numpy(), rstd.cpu().numpy()), (dev(dy), zt, mean, rstd, gt, bt, kt)


def ln_run(M, N, seed, work):
    _, (dyt, zt, mean, rstd, gt, bt, kt) = ln_data(seed, M, N)
    fz = Frame(M, N, top=0, left=0, right=12, bottom=1)                                # rows of 16-byte chunks: the view starts the buffer
    fg, fb = vec_frame(N), vec_frame(N)
    dz, dg, db = ops.ln_act_bwd(dyt, zt, mean, rstd, gt, bt, kt, 0.3, dz_out=fz.view, dgamma_out=fg[1], dbeta_out=fb[1], work=work)
    return [dz, dg, db], [fz, fg[0], fb[0]], []


def ln_stale_run(M, N):
    g = guarded(ops.ln_act_bwd_work_bytes(M, N, True), "ones", DEV)
    ln_run(M, N, 2, g.tensor)
    return g


@pytest.mark.parametrize("M,N", LN_CASES)
def test_ln_act_bwd(M, N, monkeypatch):
    groups = -(-M // 32)
    need = ops.ln_act_bwd_work_bytes(M, N, True)
    assert need == (8 * N * groups if M > 32 else 0) and (need > 0) == (groups > 1) == ((M, N) != (32, 128))
    (z, gamma, beta, keep, dy, mean, rstd), _ = ln_data(1, M, N)
    dz64, dg64, db64 = DB.ln_bwd(dy, z, mean, rstd, gamma, beta, keep, 0.3, np.float64)
    tz, tg, tb = DB.ln_bwd_tol(dy, z, mean, rstd, gamma, beta, keep, 0.3)

    def check_ref(out):
        for got, ref, tol, what in zip(out, (dz64, dg64, db64), (tz, tg, tb), ("dz", "dgamma", "dbeta")):
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            assert (err <= tol).all(), (what, float((err / np.maximum(tol, 1e-300)).max()))
    i = LN_CASES.index((M, N))
    larger = LN_CASES[i + 1] if i + 1 < len(LN_CASES) else (2 * M, N)
    run_contract(f"ln_act_bwd M{M} N{N}", "mmvae_ln_act_bwd", lambda work: ln_run(M, N, 1, work), need, check_ref,
                 lambda: stale_image(ln_stale_run, larger), (0, need - 4) if need else None, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------
# the dW GEMMs: slab / slab_elems of mmvae_gemm_tn, mmvae_gemm_tn_group and mmvae_gemm_tn_group_riders
# ---------------------------------------------------------------------------------------------------------------------------
import elementwise_bounds as E  # noqa: E402
import gemm_bounds as G  # noqa: E402
import gemm_cases as GC  # noqa: E402
import test_gemm_folded_gpu as FG  # noqa: E402  (Arena, GroupProblem, group_call: imported as modules, so that no test is collected twice)
import test_gemm_gpu as TG  # noqa: E402  (DwCase, tn_plan)
import test_step_tail_gpu as ST  # noqa: E402  (Tail)
from gemm_gpu_util import a_operand, host, status, tn_wide_plan, tuning, within  # noqa: E402
from mmvae.ops import PREC_BF16  # noqa: E402


class FourWaveCase:
    """the 128 x 128 four-wave kernel, register-staged (fp32 P and Q in bf16 mode), the batch split three ways"""

    def __init__(self, M, seed=0):
        self.N, self.K, self.nsplit = 40, 128, 3
        self.case = TG.DwCase(PREC_BF16, M, self.N, self.K, "f32", "f32", seed)
        self.ns = TG.tn_plan(M, self.N, self.K, 64, self.nsplit)[1]                  # read back as tests/test_gemm_gpu.py does
        self.elems = self.ns * self.N * self.K
        self.ref = self.case.ref
        self.fallback_ns = None

    def tol(self, atomics):
        return self.case.tol(atomics)

    def run(self, slab):
        a = self.case.outputs()
        assert status(ops.gemm_tn, PREC_BF16, self.case.p, self.case.q, a.views[0], a.views[1], self.N, self.K, nsplit=self.nsplit, slab=slab) == 0
        torch.cuda.synchronize()
        assert a.guards_unchanged(), "the gradient arena was written outside dw / db"
        return a


class WideCase:
    """the wide-tile kernels on the smallest problems launch_tn_wide takes, built as tests/test_gemm_gpu.py: SLAB_VIEWS builds them"""

    def __init__(self, M, N, K, pmode, seed=0):
        prec = PREC_BF16
        rng = np.random.default_rng(seed + M + 3 * N + 7 * K)
        self.N, self.K = N, K
        self.plan = tn_wide_plan(M, N, K, pmode, "f32", K)
        tail = GC.dw_tail(M, self.plan[4] if self.plan else None)
        p, q = GC.dw_case(rng, M, N, K, tail)
        self.pd, p_host = a_operand(p, prec, "bf16")
        self.qd, self.q_host = a_operand(q, prec, "f32", K)
        self.dp, self.pro = None, {}
        if pmode:
            y = GC.rnd(rng, M, N, scale=2.0) + np.float32(0.3)
            mean, rstd = GC.rnd(rng, N, scale=0.2), rng.uniform(0.5, 1.5, N).astype(np.float32)
            coef = np.stack([rng.uniform(0.5, 1.5, N), rng.standard_normal(N) * 0.1, rng.standard_normal(N) * 0.1]).astype(np.float32)
            yd, y_host = a_operand(y, prec, "bf16")
            p_host, self.dp = G.operand_risk(E.bn_bwd_apply(p_host, y_host, mean, rstd, coef, np.float64), E.bn_bwd_apply_tol(p_host, y_host, mean, rstd, coef), True)
            self.pro = {"p_prologue": ops.BnBwdApply(yd, dev(mean), dev(rstd), dev(coef).contiguous())}
        self.p_host = p_host
        self.old_dw, self.old_db = GC.rnd(rng, N, K), GC.rnd(rng, N)
        if self.plan:
            self.ns = self.plan[3]
            self.elems = self.ns * N * K
            self.fallback_ns = TG.tn_plan(M, N, K, 64, 0)[1]                         # the four-wave form's own split, when the wide one is refused

    @functools.cached_property
    def ref(self):
        return G.dw_ref(self.p_host, self.q_host, self.old_dw, self.old_db)

    @functools.lru_cache(maxsize=None)
    def tol(self, atomics):
        return G.dw_tol(self.p_host, self.q_host, self.old_dw, self.old_db, dp=self.dp, atomics=atomics)

    def run(self, slab):
        a = FG.Arena([(self.N, self.K), (self.N,)])
        a.views[0].copy_(dev(self.old_dw)); a.views[1].copy_(dev(self.old_db))
        with tuning(k4=1):
            assert status(ops.gemm_tn, PREC_BF16, self.pd, self.qd, a.views[0], a.views[1], self.N, self.K, slab=slab, **self.pro) == 0
            torch.cuda.synchronize()
        assert a.guards_unchanged(), "the gradient arena was written outside dw / db"
        return a


def slab_case(form, M, seed=0):
    if form == "four-wave":
        return FourWaveCase(M, seed)
    return WideCase(M, 128, 256 if form == "wide LDS-DMA" else 258, form == "wide register", seed)


def held(c, a, atomics, tag):
    (rw, rb), (tw, tb) = c.ref, c.tol(atomics)
    within(host(a.views[0]), rw, tw, tag + " dW")
    within(host(a.views[1]), rb, tb, tag + " db")


@pytest.mark.parametrize("form,M,phase,expect", [("four-wave", 1000, 4, None), ("wide LDS-DMA", 8192, 4, ("dma", (128, 448), 1, 64, 128)),
                                                 ("wide register", 8192 + 96, 8, ("reg", (128, 448), 1, 65, 128))],
                         ids=["four-wave", "wide-lds-dma", "wide-register"])
def test_gemm_tn_slab(form, M, phase, expect):
    """slab_elems == nsplit * N * K exactly: the slab path, dW inside dw_tol() without atomics and bit-identical under the three fills (db
    is added to by atomics and only held to its bound).  One element fewer: the form's slab path is not taken.  The four-wave form then
    adds with atomics (dw_tol(atomics=True)) and leaves the slab byte for byte as it was.  A wide form is refused by launch_tn_wide
    and the problem goes to the four-wave form, whose own, smaller split still fits the slab (the header: the slab is used when it
    holds nsplit * N * K floats, nsplit being the library's choice): that is asserted through the plan, and the atomics path is then
    reached one element below THAT size.  The slab starts on an odd float (phase 4) or on 8 bytes: tn_store_slab picks its store width."""
    c = slab_case(form, M)
    N, K = c.N, c.K
    if expect:
        assert c.plan == expect
        assert c.qd.stride(0) == K and c.qd.data_ptr() % 16 == 0 and (K * 4) % 16 == (0 if K == 256 else 8)
    assert c.ns > 1
    want = c.run(torch.empty(c.elems, device=DEV))
    held(c, want, False, f"{form} ordinary slab")

    @functools.lru_cache(maxsize=None)
    def stale():
        big = torch.full((max(4 * c.elems, 1 << 20),), float("nan"), device=DEV)     # the partial tiles of twice the rows, other values
        slab_case(form, 2 * M, seed=1).run(big)
        return big[:c.elems].clone()
    for fill in ("zero", "ones", "stale"):
        g = guarded(4 * c.elems, stale() if fill == "stale" else fill, DEV, phase)
        assert g.f32.numel() == c.elems and g.f32.data_ptr() % 16 == phase
        a = c.run(g.f32)
        assert torch.equal(bits(a.views[0]), bits(want.views[0])), (form, f"dW depends on the slab's contents: fill {fill}")
        held(c, a, False, f"{form} guarded slab, fill {fill}")
        g.check(f"{form}, fill {fill}")
    sizes = [c.elems - 1]
    if c.fallback_ns:
        assert 1 < c.fallback_ns and c.fallback_ns * N * K <= c.elems - 1            # the four-wave form's split fits: its slab path
        g = guarded(4 * (c.elems - 1), "ones", DEV, phase)
        held(c, c.run(g.f32), False, f"{form} one element fewer: the four-wave form through the slab")
        g.check(f"{form}, one element fewer")
        sizes = [c.fallback_ns * N * K - 1]
    for elems in sizes:                                                               # no slab path is left: atomics, the slab is not touched
        g = guarded(4 * elems, "ones", DEV, phase)
        before = g.image()
        held(c, c.run(g.f32), True, f"{form} slab of {elems} floats: atomics")
        assert torch.equal(g.work, before), (form, "the atomics path wrote the slab")
        g.check(f"{form}, atomics")


def group_stale(problems, seed):
    """the slabs left by the same shapes at twice the rows on other values, through the same entry"""
    other = [FG.GroupProblem(pr.prec, pr.combo, 2 * pr.M, pr.N, pr.K, masked=pr.pro is not None and pr.pro[2] is not None, seed=seed) for pr in problems]
    arenas = [pr.outputs() for pr in other]
    assert FG.group_call(other, arenas) == 0
    torch.cuda.synchronize()
    return [pr.slab for pr in other]


def group_slabs(problems, fill, stale):
    return [guarded(4 * ops.TN_GROUP_SPLITS * pr.N * pr.K, stale[i] if fill == "stale" else fill, DEV, 4 if i % 2 else 8)
            for i, pr in enumerate(problems)]


def test_gemm_tn_group_slabs():
    """per-problem slabs of exactly MMVAE_TN_GROUP_SPLITS * N * K floats, each between guards: dW bit-identical under the three fills"""
    problems = FG._group(PREC_BF16, 3)                                               # the smallest group of several problems
    want = [pr.outputs() for pr in problems]
    assert FG.group_call(problems, want) == 0
    torch.cuda.synchronize()
    for i, (pr, a) in enumerate(zip(problems, want)):
        pr.check(a, f"group #{i} own slab")
    stale = group_stale(problems, 11)
    for fill in ("zero", "ones", "stale"):
        gs = group_slabs(problems, fill, stale)
        arenas = [pr.outputs() for pr in problems]
        assert FG.group_call([pr.args(a, slab=g.f32) for pr, a, g in zip(problems, arenas, gs)], arenas) == 0
        torch.cuda.synchronize()
        for i, (pr, a, b, g) in enumerate(zip(problems, arenas, want, gs)):
            assert torch.equal(bits(a.views[0]), bits(b.views[0])), f"group #{i}: dW depends on the slab's contents: fill {fill}"
            pr.check(a, f"group #{i} guarded slab, fill {fill}")
            g.check(f"group #{i}, fill {fill}")


def test_gemm_tn_group_riders_slabs():
    """the same under the riders: the problems of tests/test_step_tail_gpu.py with the library's own split, every destination of the
    riders held to its float64 bound"""
    t = ST.Tail(PREC_BF16, 24, 32, 20)
    problems = ST._problems(PREC_BF16)

    def run(slabs):
        o = t.fresh()
        gs = [pr.args(a) if slabs is None else pr.args(a, slab=g.f32) for pr, a, g in zip(problems, o["arenas"], slabs or problems)]
        arr = (_lib.GemmTnArgs * len(gs))(*gs)
        r = ops.tn_riders(t.embed_args(o), t.loss_args(o, False))
        assert _lib.load().mmvae_gemm_tn_group_riders(C.cast(arr, C.c_void_p), len(gs), C.byref(r), ST.stream()) == 0
        torch.cuda.synchronize()
        ST._written(t, o, "riders")
        return o
    want = run(None)
    stale = group_stale(problems, 12)
    for fill in ("zero", "ones", "stale"):
        gs = group_slabs(problems, fill, stale)
        o = run(gs)
        for i, (a, b, g) in enumerate(zip(o["arenas"], want["arenas"], gs)):
            assert torch.equal(bits(a.views[0]), bits(b.views[0])), f"riders, problem {i}: dW depends on the slab's contents: fill {fill}"
            g.check(f"riders, problem {i}, fill {fill}")
