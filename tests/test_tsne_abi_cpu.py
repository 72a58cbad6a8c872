"""Layout of the three t-SNE argument structs as gcc lays include/mmvae_hip.h out == the ctypes mirror (the pattern of
tests/test_knn_abi_cpu.py), the entries in the binding, and what they and the Python wrappers refuse or answer without a device."""
import ctypes as C

import pytest
import torch

from abi_util import header_facts
from mmvae import _lib, clustering, ops, tsne

STRUCTS = {"mmvae_tsne_affinities_args": _lib.TsneAffinitiesArgs, "mmvae_tsne_gradient_args": _lib.TsneGradientArgs,
           "mmvae_tsne_update_args": _lib.TsneUpdateArgs}
ENTRIES = ("mmvae_tsne_affinities", "mmvae_tsne_gradient", "mmvae_tsne_gradient_splits", "mmvae_tsne_gradient_work_bytes", "mmvae_tsne_update",
           "mmvae_tsne_update_work_bytes")


def test_tsne_structs_match_c_layout(tmp_path):
    got = header_facts(tmp_path, structs=STRUCTS, values={"MAXK": "MMVAE_KNN_MAXK"})
    for cname, cls in STRUCTS.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert int(got["MAXK"]) == _lib.KNN_MAXK == 96                # 91 neighbours of perplexity 30 and the row itself


def test_tsne_entries_are_bound_and_the_abi_version_stays():
    for name in ENTRIES:
        assert name in _lib.EXPORTED
        assert hasattr(_lib.load(), name)
    assert _lib.load().mmvae_abi_version() == 20 == _lib.ABI_VERSION


def test_knn_accepts_k_up_to_96_without_a_device():
    lib = _lib.load()
    n = C.c_int64(-1)
    assert ops.knn_work_bytes(200, 5000, 92) >= 4 * 5200
    assert lib.mmvae_knn_work_bytes(200, 5000, 96, C.byref(n)) == 0 and lib.mmvae_knn_work_bytes(200, 5000, 97, C.byref(n)) == -1
    # the list of a split is k entries whatever MMVAE_KNN_MAXK is: the workspace of k <= 64 is what it was
    ns, _ = ops.knn_splits(3, 5000)
    assert ops.knn_work_bytes(3, 5000, 64) == (4 * 5003 + 7) // 8 * 8 + 8 * 3 * ns * 64


def _aff(N=10, k=5, perplexity=2.0, ld=None):
    """pointers that are never dereferenced: every call below is refused before a launch"""
    return _lib.TsneAffinitiesArgs(0x1000, 0x2000, 0x3000, k if ld is None else ld, k, N, k, perplexity, 0)


def test_affinities_refuses_without_a_launch():
    lib = _lib.load()
    assert lib.mmvae_tsne_affinities(None, None) == -1
    assert lib.mmvae_tsne_affinities(C.byref(_lib.TsneAffinitiesArgs()), None) == -1
    for kw in (dict(N=0), dict(k=0), dict(perplexity=0.0), dict(perplexity=-1.0), dict(perplexity=5.0), dict(perplexity=5.5),
               dict(perplexity=float("nan")), dict(ld=4), dict(k=1, perplexity=1.0)):
        assert lib.mmvae_tsne_affinities(C.byref(_aff(**kw)), None) == -1, kw
    for field, value in (("dist2", 0), ("p", 0), ("beta", 0), ("dist2", 0x1002), ("p", 0x2001), ("beta", 0x3002), ("ld_p", 4)):
        a = _aff()
        setattr(a, field, value)
        assert lib.mmvae_tsne_affinities(C.byref(a), None) == -1, (field, value)


def _grad(N=300, nnz=1000, splits=0, work_bytes=None):
    ok = N >= 2 and 0 <= splits <= 64
    need = ops.tsne_gradient_work_bytes(N, splits) if ok else 1 << 30
    return _lib.TsneGradientArgs(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000, nnz,
                                 need if work_bytes is None else work_bytes, N, splits, 1.0, 0)


def test_gradient_refuses_without_a_launch():
    lib = _lib.load()
    assert lib.mmvae_tsne_gradient(None, None) == -1
    assert lib.mmvae_tsne_gradient(C.byref(_lib.TsneGradientArgs()), None) == -1
    for kw in (dict(N=1), dict(N=0), dict(nnz=-1), dict(nnz=1 << 31), dict(splits=-1), dict(splits=65)):
        assert lib.mmvae_tsne_gradient(C.byref(_grad(**kw)), None) == -1, kw
    need = ops.tsne_gradient_work_bytes(300, 0)
    assert lib.mmvae_tsne_gradient(C.byref(_grad(work_bytes=need - 1)), None) == -1
    for field, value in (("y", 0), ("row_ptr", 0), ("col", 0), ("val", 0), ("grad", 0), ("z", 0), ("work", 0), ("y", 0x1004), ("row_ptr", 0x2002),
                         ("col", 0x3001), ("val", 0x4002), ("grad", 0x5002), ("z", 0x6001), ("err", 0x7002), ("z_row", 0x8002), ("work", 0x9004)):
        a = _grad()
        setattr(a, field, value)
        assert lib.mmvae_tsne_gradient(C.byref(a), None) == -1, (field, value)


def test_gradient_planners_need_no_device():
    lib = _lib.load()
    n, ns = C.c_int64(-1), C.c_int32(-1)
    for bad in ((1, 0), (0, 0), (10, -1), (10, 65)):
        assert lib.mmvae_tsne_gradient_work_bytes(*bad, C.byref(n)) == -1, bad
        assert lib.mmvae_tsne_gradient_splits(*bad, C.byref(ns)) == -1, bad
    assert lib.mmvae_tsne_gradient_work_bytes(10, 0, None) == -1 and lib.mmvae_tsne_gradient_splits(10, 0, None) == -1
    # the evaluation's shape: 103 row blocks of 512, ceil(2048 / 103) = 20 wanted, 820 chunks of 64 columns in runs of 41
    assert ops.tsne_gradient_splits(52429) == 20
    assert ops.tsne_gradient_work_bytes(52429) == (12 * 52429 * 20 + 7) // 8 * 8 + 4 * 20 * 103
    # a forced count is kept up to the number of 64-column chunks, and consecutive runs leave no split empty
    assert [ops.tsne_gradient_splits(n, 5) for n in (2, 127, 129, 513, 777)] == [1, 2, 3, 5, 5]
    assert ops.tsne_gradient_splits(777, 64) == 13 and ops.tsne_gradient_splits(777, 12) == 7           # 13 chunks in runs of 2
    assert ops.tsne_gradient_splits(1 << 21) == 1                                                       # 4096 row blocks
    assert ops.tsne_gradient_work_bytes(777, 2) == 12 * 777 * 2 + 4 * 2 * 2
    assert ops.tsne_gradient_work_bytes(3, 1) == 40 + 8


def test_update_refuses_without_a_launch_and_its_planner():
    lib = _lib.load()
    n = C.c_int64(-1)
    assert lib.mmvae_tsne_update_work_bytes(0, C.byref(n)) == -1 and lib.mmvae_tsne_update_work_bytes(5, None) == -1
    assert ops.tsne_update_work_bytes(128) == 8 and ops.tsne_update_work_bytes(129) == 8 and ops.tsne_update_work_bytes(52429) == 4 * 410
    assert lib.mmvae_tsne_update(None, None) == -1
    assert lib.mmvae_tsne_update(C.byref(_lib.TsneUpdateArgs()), None) == -1

    def args(**kw):
        a = _lib.TsneUpdateArgs(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 8, 128, 0.5, 100.0, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for kw in (dict(N=0), dict(y=0), dict(update=0), dict(gains=0), dict(grad=0), dict(y=0x1002), dict(update=0x2001), dict(gains=0x3002),
               dict(grad=0x4002), dict(grad_norm=0x5002), dict(work=0x6004), dict(work=0), dict(work_bytes=4)):
        assert lib.mmvae_tsne_update(C.byref(args(**kw)), None) == -1, kw


def test_python_layer_refuses_on_the_host():
    x = torch.zeros(40, 6)
    assert clustering.TSNE is tsne.TSNE
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsne.TSNE(perplexity=5).fit_transform(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tsne_affinities(torch.zeros(4, 3), 2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tsne_gradient(torch.zeros(4, 2), None, None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tsne_update(torch.zeros(4, 2), None, None, None, 0.5, 1.0)
    for kw in (dict(n_components=3), dict(metric="cosine"), dict(perplexity=0), dict(early_exaggeration=0.5), dict(learning_rate=0.0),
               dict(max_iter=249), dict(init="spectral")):
        with pytest.raises(ValueError):
            tsne.TSNE(**kw)
    t = tsne.TSNE()
    assert (t.n_components, t.perplexity, t.early_exaggeration, t.learning_rate, t.max_iter, t.n_iter_without_progress, t.min_grad_norm, t.init,
            t.random_state) == (2, 30.0, 12.0, "auto", 1000, 300, 1e-7, "pca", None)


def test_joint_probabilities_on_the_host_equal_the_float64_restatement():
    import numpy as np
    import tsne_ref as TR
    g = np.random.default_rng(4)
    N, k = 57, 9
    idx = np.stack([g.permutation(np.delete(np.arange(N), i))[:k] for i in range(N)]).astype(np.int32)
    p = g.random((N, k)).astype(np.float32)
    row_ptr, col, val = tsne.joint_probabilities(torch.from_numpy(idx), torch.from_numpy(p))
    r, c, v = TR.symmetric_csr(idx, p)
    assert row_ptr.dtype == col.dtype == torch.int32 and val.dtype == torch.float32
    assert np.array_equal(row_ptr.numpy(), r) and np.array_equal(col.numpy(), c)
    # a slot: one fp32 addition of two fp32 values, the division by the float64 total, the rounding to fp32
    assert (np.abs(val.double().numpy() - v) <= 3 * 2.0 ** -24 * v).all()
    assert abs(float(val.double().sum()) - 1.0) <= 1e-6
