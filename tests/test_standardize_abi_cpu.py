"""Layouts of mmvae_std_part / mmvae_standardize_fit_args / mmvae_standardize_apply_args as gcc lays include/mmvae_hip.h out == the
ctypes mirrors (the pattern of tests/test_pca_abi_cpu.py), the StandardScaler entries in the binding, the planner against the header's
formula, and what the entries and the Python wrappers refuse without a device.  The pointers below are never dereferenced: every call
is refused before a launch."""
import ctypes as C

import pytest
import torch

import standardize_ref as R
from abi_util import header_facts
from mmvae import _lib, clustering, ops

STRUCTS = (("mmvae_std_part", _lib.StdPart), ("mmvae_standardize_fit_args", _lib.StandardizeFitArgs),
           ("mmvae_standardize_apply_args", _lib.StandardizeApplyArgs))
ENTRIES = ("mmvae_standardize_fit", "mmvae_standardize_fit_splits", "mmvae_standardize_fit_work_bytes", "mmvae_standardize_apply")
ARG, DTYPE = -1, -2


def test_structs_match_c_layout(tmp_path):
    got = header_facts(tmp_path, structs=dict(STRUCTS), values={"MAXP": "MMVAE_STD_MAX_PARTS"})
    for cname, cls in STRUCTS:
        assert int(got[cname]) == C.sizeof(cls)
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert int(got["MAXP"]) == _lib.STD_MAX_PARTS == 4


def test_entries_are_bound_and_the_abi_version_stays():
    for name in ENTRIES:
        assert name in _lib.EXPORTED
        assert hasattr(_lib.load(), name)
    assert _lib.load().mmvae_abi_version() == 20 == _lib.ABI_VERSION


def _parts(a, specs):
    for i, (cols, dtype, ld, one_row) in enumerate(specs):
        a.part[i] = _lib.StdPart(0x10000 * (i + 1), ld, cols, dtype, one_row, 0)
    a.n_parts = len(specs)


SPECS = ((33, 0, 40, 0), (3, 1, 8, 0), (2, 1, 0, 1))           # F = 38


def _fit(rows=500, specs=SPECS, splits=0, work_bytes=None):
    a = _lib.StandardizeFitArgs()
    _parts(a, specs)
    a.mean, a.var, a.scale, a.work = 0x100000, 0x200000, 0x300000, 0x400000
    F = sum(s[0] for s in specs)
    ok = rows >= 1 and F >= 1 and 0 <= splits <= 64
    a.work_bytes = (ops.standardize_fit_work_bytes(rows, F, splits) if ok else 1 << 30) if work_bytes is None else work_bytes
    a.rows, a.splits = rows, splits
    return a


def _apply(rows=500, specs=SPECS, ldz=None):
    a = _lib.StandardizeApplyArgs()
    _parts(a, specs)
    a.mean, a.scale, a.z = 0x100000, 0x200000, 0x300000
    a.ldz = sum(s[0] for s in specs) if ldz is None else ldz
    a.rows = rows
    return a


BAD_PARTS = (
    ((0, 0, 40, 0),), ((-1, 0, 40, 0),),                         # cols < 1
    ((33, 0, 32, 0),),                                           # ld < cols on a matrix part
    ((33, 0, 40, 0), (3, 1, 2, 0)),
)


def test_fit_refuses_without_a_launch():
    fit = _lib.load().mmvae_standardize_fit
    assert fit(None, None) == ARG
    assert fit(C.byref(_lib.StandardizeFitArgs()), None) == ARG
    for kw in (dict(rows=0), dict(rows=-5), dict(splits=-1), dict(splits=65)):
        assert fit(C.byref(_fit(**kw)), None) == ARG, kw
    for specs in BAD_PARTS:
        assert fit(C.byref(_fit(specs=specs)), None) == ARG, specs
    assert fit(C.byref(_fit(specs=((5, 0, 0, 1), (2, 1, 0, 1)))), None) == ARG                   # every part is one row
    for n_parts in (0, -1, 5):
        a = _fit()
        a.n_parts = n_parts
        assert fit(C.byref(a), None) == ARG, n_parts
    for dtype in (2, -1, 7):
        assert fit(C.byref(_fit(specs=((33, 0, 40, 0), (3, dtype, 8, 0)))), None) == DTYPE, dtype
    need = ops.standardize_fit_work_bytes(500, 38, 0)
    assert need > 0
    assert fit(C.byref(_fit(work_bytes=need - 1)), None) == ARG and fit(C.byref(_fit(work_bytes=0)), None) == ARG
    for field, value in (("mean", 0), ("var", 0), ("scale", 0), ("work", 0), ("mean", 0x100004), ("var", 0x200004), ("scale", 0x300001),
                         ("work", 0x400004)):
        a = _fit()
        setattr(a, field, value)
        assert fit(C.byref(a), None) == ARG, (field, value)
    for i, ptr in ((0, 0), (1, 0), (2, 0), (0, 0x10002), (1, 0x20001), (2, 0x30001)):           # null / not aligned to the element
        a = _fit()
        a.part[i].x = ptr
        assert fit(C.byref(a), None) == ARG, (i, ptr)


def test_apply_refuses_without_a_launch():
    apply = _lib.load().mmvae_standardize_apply
    assert apply(None, None) == ARG
    assert apply(C.byref(_lib.StandardizeApplyArgs()), None) == ARG
    for kw in (dict(rows=0), dict(rows=-1), dict(ldz=37), dict(ldz=0)):
        assert apply(C.byref(_apply(**kw)), None) == ARG, kw
    for specs in BAD_PARTS:
        assert apply(C.byref(_apply(specs=specs)), None) == ARG, specs
    for n_parts in (0, 5):
        a = _apply()
        a.n_parts = n_parts
        assert apply(C.byref(a), None) == ARG, n_parts
    assert apply(C.byref(_apply(specs=((33, 2, 40, 0),))), None) == DTYPE
    for field, value in (("mean", 0), ("scale", 0), ("z", 0), ("mean", 0x100004), ("scale", 0x200004), ("z", 0x300002)):
        a = _apply()
        setattr(a, field, value)
        assert apply(C.byref(a), None) == ARG, (field, value)
    a = _apply()
    a.part[1].x = 0
    assert apply(C.byref(a), None) == ARG


def test_splits_and_work_bytes_need_no_device():
    lib = _lib.load()
    n, ns = C.c_int64(-1), C.c_int32(-1)
    for bad in ((0, 2, 0), (10, 0, 0), (10, 2, -1), (10, 2, 65)):
        assert lib.mmvae_standardize_fit_work_bytes(*bad, C.byref(n)) == ARG, bad
        assert lib.mmvae_standardize_fit_splits(*bad, C.byref(ns)) == ARG, bad
    assert lib.mmvae_standardize_fit_work_bytes(10, 2, 0, None) == ARG and lib.mmvae_standardize_fit_splits(10, 2, 0, None) == ARG
    for rows, F in ((1, 5), (2, 1), (65, 12), (257, 24), (1000, 1354), (4099, 39), (52429, 1354), (52429, 782), (1 << 20, 3), (100, 1 << 33)):
        for splits in (0, 1, 2, 3, 7, 63, 64):
            used = R.splits_used(rows, F, splits)[0]
            assert ops.standardize_fit_splits(rows, F, splits) == used, (rows, F, splits)
            assert ops.standardize_fit_work_bytes(rows, F, splits) == 16 * F * used == R.work_bytes(rows, F, splits), (rows, F, splits)
    assert ops.standardize_fit_splits(52429, 1354) == 64 and ops.standardize_fit_splits(1, 5) == 1 and ops.standardize_fit_splits(1000, 1354) == 31
    assert ops.standardize_fit_splits(4099, 39, 64) == 64 and R.splits_used(4099, 39, 64)[1] * 63 < 4099 < R.splits_used(4099, 39, 64)[1] * 64


def test_python_refuses_on_the_host():
    x, v = torch.zeros(6, 3), torch.zeros(3, dtype=torch.float64)
    for call in (lambda: ops.standardize_fit(x), lambda: ops.standardize_fit([x, x]), lambda: ops.standardize_apply(x, v, v),
                 lambda: clustering.StandardScaler().fit(x), lambda: clustering.StandardScaler().fit_transform([x, torch.zeros(2)])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="before fit"):
        clustering.StandardScaler().transform(x)
    assert "StandardScaler" in clustering.__all__
