"""Layout of mmvae_knn_args as gcc lays include/mmvae_hip.h out == the ctypes mirror (the pattern of tests/test_class_tail_abi_cpu.py),
the k-NN entries in the binding, and what they refuse or answer without a device."""
import ctypes as C

from abi_util import header_facts
from mmvae import _lib, ops


def test_knn_struct_matches_c_layout(tmp_path):
    cname, cls = "mmvae_knn_args", _lib.KnnArgs
    got = header_facts(tmp_path, structs={cname: cls}, values={"MAXK": "MMVAE_KNN_MAXK"})
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    assert int(got["MAXK"]) == _lib.KNN_MAXK >= 50


def test_knn_entries_are_bound_and_the_abi_version_stays():
    for name in ("mmvae_knn_search", "mmvae_knn_work_bytes", "mmvae_knn_splits", "mmvae_knn_mean_rows"):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.load(), name)
    assert _lib.load().mmvae_abi_version() == 20


def _args(Mq=8, Nt=100, F=16, k=5, work_bytes=None, dtype=0):
    """pointers that are never dereferenced: every call below is refused before a launch"""
    need = ops.knn_work_bytes(Mq, Nt, min(max(k, 1), min(Nt, _lib.KNN_MAXK)))
    return _lib.KnnArgs(0x1000, 0x2000, None, 0x3000, 0x4000, 0x5000, F, F, k, k, need if work_bytes is None else work_bytes,
                        Mq, Nt, F, k, dtype, dtype)


def test_knn_search_refuses_without_a_launch():
    lib = _lib.load()
    assert lib.mmvae_knn_search(None, None) == -1
    assert lib.mmvae_knn_search(C.byref(_lib.KnnArgs()), None) == -1
    assert lib.mmvae_knn_search(C.byref(_args(Nt=4, k=5)), None) == -1                     # k > Nt
    assert lib.mmvae_knn_search(C.byref(_args(k=_lib.KNN_MAXK + 1)), None) == -1           # k > MMVAE_KNN_MAXK
    assert lib.mmvae_knn_search(C.byref(_args(k=0)), None) == -1
    need = ops.knn_work_bytes(8, 100, 5)
    assert lib.mmvae_knn_search(C.byref(_args(work_bytes=need - 1)), None) == -1           # short workspace
    assert lib.mmvae_knn_search(C.byref(_args(dtype=2)), None) == -2                       # neither fp32 nor bf16
    for field, value in (("ld_q", 15), ("ld_t", 15), ("ld_idx", 4), ("ld_dist2", 4), ("q", 0x1002), ("work", 0x5004), ("Mq", 0), ("F", 0)):
        a = _args()
        setattr(a, field, value)
        assert lib.mmvae_knn_search(C.byref(a), None) == -1, field
    assert lib.mmvae_knn_mean_rows(None, 5, 0x1000, 0, 8, 0x2000, 8, 4, 5, 10, 8, None) == -1
    assert lib.mmvae_knn_mean_rows(0x1000, 5, 0x2000, 2, 8, 0x3000, 8, 4, 5, 10, 8, None) == -2
    assert lib.mmvae_knn_mean_rows(0x1000, 4, 0x2000, 0, 8, 0x3000, 8, 4, 5, 10, 8, None) == -1       # ld_idx < k


def test_knn_work_bytes_and_splits_need_no_device():
    lib = _lib.load()
    n = C.c_int64(-1)
    for bad in ((0, 10, 1), (10, 0, 1), (10, 10, 0), (10, 4, 5), (10, 1000, _lib.KNN_MAXK + 1)):
        assert lib.mmvae_knn_work_bytes(*bad, C.byref(n)) == -1, bad
    assert lib.mmvae_knn_work_bytes(10, 10, 5, None) == -1
    # enough query blocks: one split, the workspace holds the rows' norms only
    assert ops.knn_splits(1 << 18, 100000)[0] == 1
    assert ops.knn_work_bytes(1 << 18, 100000, 5) == 4 * ((1 << 18) + 100000)
    # few queries: the training rows are split in whole tiles and every split's list has its place
    ns, rps = ops.knn_splits(3, 5000)
    assert ns > 1 and rps % 128 == 0 and (ns - 1) * rps < 5000 <= ns * rps
    assert ops.knn_work_bytes(3, 5000, 6) == (4 * 5003 + 7) // 8 * 8 + 8 * 3 * ns * 6
    assert ops.knn_splits(3, 100) == (1, 128)
