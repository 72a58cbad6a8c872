"""Layouts of mmvae_pca_scatter_args / mmvae_pca_project_args as gcc lays include/mmvae_hip.h out == the ctypes mirrors (the pattern of
tests/test_silhouette_abi_cpu.py), the PCA entries in the binding, and what they, the Python wrappers and mmvae.pca.PCA refuse or
answer without a device."""
import ctypes as C

import pytest
import torch

import pca_ref as PR
from abi_util import header_facts
from mmvae import _lib, clustering, ops, pca

STRUCTS = (("mmvae_pca_scatter_args", _lib.PcaScatterArgs), ("mmvae_pca_project_args", _lib.PcaProjectArgs))


def test_pca_structs_match_c_layout(tmp_path):
    got = header_facts(tmp_path, structs=dict(STRUCTS), values={"MAXK": "MMVAE_PCA_MAXK"})
    for cname, cls in STRUCTS:
        assert int(got[cname]) == C.sizeof(cls)
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert int(got["MAXK"]) == _lib.PCA_MAXK == 64


def test_pca_entries_are_bound_and_the_abi_version_stays():
    for name in ("mmvae_pca_scatter", "mmvae_pca_scatter_splits", "mmvae_pca_scatter_work_bytes", "mmvae_pca_project"):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.load(), name)
    assert _lib.load().mmvae_abi_version() == 20 == _lib.ABI_VERSION


def _scatter(N=1000, F=129, splits=0, work_bytes=None, dtype=0):
    """pointers that are never dereferenced: every call below is refused before a launch"""
    ok = N >= 1 and F >= 1 and 0 <= splits <= 64
    need = ops.pca_scatter_work_bytes(N, F, splits) if ok else 1 << 30
    return _lib.PcaScatterArgs(0x1000, 0x2000, 0x3000, 0x4000, F, F, need if work_bytes is None else work_bytes, N, F, splits, dtype)


def test_pca_scatter_refuses_without_a_launch():
    lib = _lib.load()
    assert lib.mmvae_pca_scatter(None, None) == -1
    assert lib.mmvae_pca_scatter(C.byref(_lib.PcaScatterArgs()), None) == -1
    for kw in (dict(N=0), dict(N=-1), dict(F=0), dict(splits=-1), dict(splits=65)):
        assert lib.mmvae_pca_scatter(C.byref(_scatter(**kw)), None) == -1, kw
    need = ops.pca_scatter_work_bytes(1000, 129, 0)
    assert need > 0
    assert lib.mmvae_pca_scatter(C.byref(_scatter(work_bytes=need - 1)), None) == -1               # short workspace
    assert lib.mmvae_pca_scatter(C.byref(_scatter(dtype=2)), None) == -2                           # neither fp32 nor bf16
    for field, value in (("ld_x", 128), ("ld_s", 128), ("x", 0), ("s", 0), ("work", 0), ("x", 0x1002), ("shift", 0x2002), ("s", 0x3002),
                         ("work", 0x4004)):
        a = _scatter()
        setattr(a, field, value)
        assert lib.mmvae_pca_scatter(C.byref(a), None) == -1, (field, value)
    a = _scatter(dtype=1)                                                                          # bf16 rows are aligned to 2 bytes
    a.x = 0x1001
    assert lib.mmvae_pca_scatter(C.byref(a), None) == -1


def _project(N=300, F=77, k=3, dtype=0):
    return _lib.PcaProjectArgs(0x1000, 0x2000, 0x3000, 0x4000, F, F, k, N, F, k, dtype)


def test_pca_project_refuses_without_a_launch():
    lib = _lib.load()
    assert lib.mmvae_pca_project(None, None) == -1
    assert lib.mmvae_pca_project(C.byref(_lib.PcaProjectArgs()), None) == -1
    for kw in (dict(N=0), dict(F=0), dict(k=0), dict(k=_lib.PCA_MAXK + 1)):
        assert lib.mmvae_pca_project(C.byref(_project(**kw)), None) == -1, kw
    assert lib.mmvae_pca_project(C.byref(_project(dtype=2)), None) == -2
    for field, value in (("ld_x", 76), ("ld_v", 76), ("ld_y", 2), ("x", 0), ("v", 0), ("y", 0), ("x", 0x1002), ("shift", 0x2002), ("v", 0x3002),
                         ("y", 0x4001)):
        a = _project()
        setattr(a, field, value)
        assert lib.mmvae_pca_project(C.byref(a), None) == -1, (field, value)
    a = _project(dtype=1)
    a.x = 0x1001
    assert lib.mmvae_pca_project(C.byref(a), None) == -1


def test_splits_and_work_bytes_need_no_device():
    lib = _lib.load()
    n, ns = C.c_int64(-1), C.c_int32(-1)
    for bad in ((0, 2, 0), (10, 0, 0), (10, 2, -1), (10, 2, 65), (10, (1 << 22) + 1, 0)):
        assert lib.mmvae_pca_scatter_work_bytes(*bad, C.byref(n)) == -1, bad
        assert lib.mmvae_pca_scatter_splits(*bad, C.byref(ns)) == -1, bad
    assert lib.mmvae_pca_scatter_work_bytes(10, 2, 0, None) == -1 and lib.mmvae_pca_scatter_splits(10, 2, 0, None) == -1
    # the header's formula, restated in tests/pca_ref.py
    for N, F in ((1, 1), (77, 37), (300, 200), (1000, 129), (52429, 1354), (52429, 782), (40, 77), (1 << 20, 65536 + 1)):
        for splits in (0, 1, 3, 64):
            used = PR.splits_used(N, F, splits)[0]
            T = (F + 127) // 128
            assert ops.pca_scatter_splits(N, F, splits) == used, (N, F, splits)
            assert ops.pca_scatter_work_bytes(N, F, splits) == (65536 * (T * (T + 1) // 2) * used if used > 1 else 0), (N, F, splits)
    # the evaluation's shape: 11 x 12 / 2 = 66 tile pairs, 7 splits of 235 chunks give 462 workgroups, one resident round
    assert ops.pca_scatter_splits(52429, 1354) == 7 and ops.pca_scatter_work_bytes(52429, 1354) == 7 * 66 * 65536
    assert ops.pca_scatter_splits(77, 37) == 1 and ops.pca_scatter_work_bytes(77, 37) == 0            # one split: no workspace
    assert ops.pca_scatter_splits(77, 37, 64) == 3 and ops.pca_scatter_splits(1000, 129) == 4 and ops.pca_scatter_splits(1000, 129, 3) == 3
    assert ops.pca_scatter_splits(1 << 20, 128 * 32) == 1                                             # 528 tile pairs alone fill the device


def test_python_wrappers_refuse_on_the_host():
    x, c, v = torch.zeros(6, 3), torch.zeros(3), torch.zeros(2, 3)
    for call in (lambda: ops.pca_scatter(x, c), lambda: ops.pca_project(x, c, v), lambda: pca.PCA(2).fit(x),
                 lambda: pca.PCA(2).fit_transform(x), lambda: clustering.PCA(1).fit(x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert clustering.PCA is pca.PCA and "PCA" in clustering.__all__


def test_pca_argument_errors():
    for bad in (dict(n_components=0), dict(n_components=_lib.PCA_MAXK + 1), dict(n_components=2.0), dict(n_components=None),
                dict(n_components=True), dict(n_components=2, svd_solver="randomized"), dict(n_components=2, svd_solver="arpack"),
                dict(n_components=2, whiten=True)):
        with pytest.raises(ValueError):
            pca.PCA(**bad)
    for solver in ("auto", "full", "covariance_eigh"):
        p = pca.PCA(2, svd_solver=solver, random_state=42)
        assert p.n_components == 2 and p.random_state == 42
    with pytest.raises(RuntimeError, match="before fit"):
        pca.PCA(2).transform(torch.zeros(4, 3))
