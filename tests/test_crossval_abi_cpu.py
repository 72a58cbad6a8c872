"""mmvae_knn_search_grouped / mmvae_knn_group_work_bytes without a device: the entries are bound and the ABI version stays, KnnGroupArgs
mirrors the header's struct, the workspace formula, and every refusal returns MMVAE_ERR_ARG before anything is enqueued (the pointers
below are never dereferenced)."""
import ctypes as C

import pytest

from abi_util import header_facts
from mmvae import _lib, ops


def test_the_entries_are_bound_and_the_abi_version_stays():
    lib = _lib.load()
    for name in ("mmvae_knn_search_grouped", "mmvae_knn_group_work_bytes"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.mmvae_abi_version() == _lib.ABI_VERSION == 20
    assert C.sizeof(_lib.KnnArgs) == 112, "mmvae_knn_args keeps its layout"


def test_group_args_match_the_c_layout(tmp_path):
    pairs = {"mmvae_knn_group_args": _lib.KnnGroupArgs, "mmvae_knn_args": _lib.KnnArgs}
    got = header_facts(tmp_path, structs=pairs)
    for cname, cls in pairs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert _lib.KnnGroupArgs.base.offset == 0 and _lib.KnnGroupArgs.q_same.offset == 112


@pytest.mark.parametrize("Mq,Nt,k", [(3, 5000, 6), (300, 300, 10), (1 << 18, 100000, 50), (7, 129, 1), (7, 128, 96)])
def test_group_work_bytes_is_the_ungrouped_size_plus_four_codes_per_tile(Mq, Nt, k):
    tiles = (Nt + 127) // 128
    assert ops.knn_work_bytes(Mq, Nt, k) % 8 == 0 and ops.knn_l1_work_bytes(Mq, Nt, k) % 8 == 0      # the codes start 8-byte aligned
    assert ops.knn_group_work_bytes(Mq, Nt, k, "euclidean") == ops.knn_work_bytes(Mq, Nt, k) + 16 * tiles
    assert ops.knn_group_work_bytes(Mq, Nt, k, "manhattan") == ops.knn_l1_work_bytes(Mq, Nt, k) + 16 * tiles


def test_group_work_bytes_refusals():
    lib = _lib.load()
    n = C.c_int64(-1)
    for bad in ((0, 10, 1, 0), (10, 0, 1, 0), (10, 10, 0, 1), (10, 4, 5, 0), (10, 1000, _lib.KNN_MAXK + 1, 1), (10, 10, 5, 2), (10, 10, 5, -1)):
        assert lib.mmvae_knn_group_work_bytes(*bad, C.byref(n)) == -1, bad
    assert lib.mmvae_knn_group_work_bytes(10, 10, 5, 0, None) == -1 and n.value == -1
    with pytest.raises(ValueError):
        ops.knn_group_work_bytes(10, 10, 5, "cosine")


SAME, DIFFER = (0x7000, 0x8000, None, None), (None, None, 0x9000, 0xA000)


def _args(codes=DIFFER, metric=0, Mq=3, Nt=5000, F=16, k=5, work=0x5000, work_bytes=None, dtype=0, shift=None):
    need = ops.knn_group_work_bytes(Mq, Nt, min(max(k, 1), min(Nt, _lib.KNN_MAXK)), "manhattan" if metric == 1 else "euclidean")
    base = _lib.KnnArgs(0x1000, 0x2000, shift, 0x3000, 0x4000, work, F, F, k, k, need if work_bytes is None else work_bytes, Mq, Nt, F, k, dtype, dtype)
    return _lib.KnnGroupArgs(base, *codes, metric)


def _call(**kw):
    return _lib.load().mmvae_knn_search_grouped(C.byref(_args(**kw)), None)


@pytest.mark.parametrize("metric", [0, 1])
def test_search_grouped_refuses_without_a_launch(metric):
    lib = _lib.load()
    assert lib.mmvae_knn_search_grouped(None, None) == -1                                   # a null struct
    assert lib.mmvae_knn_search_grouped(C.byref(_lib.KnnGroupArgs()), None) == -1
    assert _call(metric=metric, codes=(None, None, None, None)) == -1                       # both pairs NULL: the plain entry's job
    for half in ((0x7000, None, None, None), (None, 0x8000, None, None), (None, None, 0x9000, None), (None, None, None, 0xA000),
                 (0x7000, 0x8000, 0x9000, None), (0x7000, None, 0x9000, 0xA000)):
        assert _call(metric=metric, codes=half) == -1, half                                 # half a pair
    for i in range(4):                                                                      # a code pointer not 4-byte aligned
        codes = [0x7000, 0x8000, 0x9000, 0xA000]
        codes[i] += 2
        assert _call(metric=metric, codes=tuple(codes)) == -1, i
    assert _call(metric=2) == -1 and _call(metric=-1) == -1                                 # metric outside {0, 1}
    need = ops.knn_group_work_bytes(3, 5000, 5, "manhattan" if metric else "euclidean")
    for codes in (SAME, DIFFER):
        assert _call(metric=metric, codes=codes, work_bytes=need - 1) == -1                 # below mmvae_knn_group_work_bytes,
        ungrouped = ops.knn_l1_work_bytes(3, 5000, 5) if metric else ops.knn_work_bytes(3, 5000, 5)
        assert _call(metric=metric, codes=codes, work_bytes=ungrouped) == -1                # the ungrouped size included
        assert _call(metric=metric, codes=codes, work=None) == -1
    assert _call(metric=metric, Mq=300, Nt=300, work=None, work_bytes=0) == -1              # unsplit manhattan too needs the tile codes
    # everything the ungrouped entry refuses
    assert _call(metric=metric, Nt=4, k=5) == -1 and _call(metric=metric, k=_lib.KNN_MAXK + 1) == -1 and _call(metric=metric, k=0) == -1
    assert _call(metric=metric, dtype=2) == -2
    assert _call(metric=1, shift=0x6000) == -1                                              # manhattan takes no shift
    for field, value in (("ld_q", 15), ("ld_t", 15), ("ld_idx", 4), ("ld_dist2", 4), ("q", 0x1002), ("idx", 0x3002), ("work", 0x5004),
                         ("Mq", 0), ("F", 0), ("t", None), ("idx", None), ("q", None), ("dist2", 0x4002)):
        a = _args(metric=metric)
        setattr(a.base, field, value)
        assert lib.mmvae_knn_search_grouped(C.byref(a), None) == -1, field
    assert _call(metric=0, shift=0x6002) == -1
