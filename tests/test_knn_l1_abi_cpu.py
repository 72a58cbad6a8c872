"""mmvae_knn_search_l1 / mmvae_knn_l1_work_bytes / mmvae_knn_weighted_rows without a device: mmvae_knn_args keeps its layout, the
workspace formula, and every refusal returns MMVAE_ERR_ARG / MMVAE_ERR_DTYPE before anything is enqueued (the pointers below are
never dereferenced)."""
import ctypes as C

from mmvae import _lib, ops

KNN_ARGS_LAYOUT = [("q", 0), ("t", 8), ("shift", 16), ("idx", 24), ("dist2", 32), ("work", 40), ("ld_q", 48), ("ld_t", 56), ("ld_idx", 64),
                   ("ld_dist2", 72), ("work_bytes", 80), ("Mq", 88), ("Nt", 92), ("F", 96), ("k", 100), ("q_dtype", 104), ("t_dtype", 108)]


def test_the_struct_layout_is_unchanged_and_the_entries_are_bound():
    assert [(n, getattr(_lib.KnnArgs, n).offset) for n, _ in _lib.KnnArgs._fields_] == KNN_ARGS_LAYOUT and C.sizeof(_lib.KnnArgs) == 112
    lib = _lib.load()
    for name in ("mmvae_knn_search_l1", "mmvae_knn_l1_work_bytes", "mmvae_knn_weighted_rows"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.mmvae_abi_version() == _lib.ABI_VERSION == 20


def test_l1_work_bytes_holds_only_the_split_lists():
    lib = _lib.load()
    n = C.c_int64(-1)
    for bad in ((0, 10, 1), (10, 0, 1), (10, 10, 0), (10, 4, 5), (10, 1000, _lib.KNN_MAXK + 1)):
        assert lib.mmvae_knn_l1_work_bytes(*bad, C.byref(n)) == -1, bad
    assert lib.mmvae_knn_l1_work_bytes(10, 10, 5, None) == -1
    assert ops.knn_splits(1 << 18, 100000)[0] == 1 and ops.knn_l1_work_bytes(1 << 18, 100000, 50) == 0
    ns, _ = ops.knn_splits(3, 5000)
    assert ns > 1 and ops.knn_l1_work_bytes(3, 5000, 6) == 8 * 3 * ns * 6
    assert ops.knn_l1_work_bytes(3, 5000, 6) % 8 == 0 and ops.knn_l1_work_bytes(3, 100, 5) == 0
    assert ops.knn_work_bytes(3, 5000, 6) - ops.knn_l1_work_bytes(3, 5000, 6) == (4 * 5003 + 7) // 8 * 8        # the norms it does not need


def _args(Mq=3, Nt=5000, F=16, k=5, work=0x5000, work_bytes=None, dtype=0, shift=None):
    need = ops.knn_l1_work_bytes(Mq, Nt, min(max(k, 1), min(Nt, _lib.KNN_MAXK)))
    return _lib.KnnArgs(0x1000, 0x2000, shift, 0x3000, 0x4000, work, F, F, k, k, need if work_bytes is None else work_bytes, Mq, Nt, F, k, dtype, dtype)


def test_search_l1_refuses_without_a_launch():
    lib = _lib.load()
    assert lib.mmvae_knn_search_l1(None, None) == -1
    assert lib.mmvae_knn_search_l1(C.byref(_lib.KnnArgs()), None) == -1
    assert lib.mmvae_knn_search_l1(C.byref(_args(shift=0x6000)), None) == -1                # a shift
    assert lib.mmvae_knn_search_l1(C.byref(_args(Nt=4, k=5)), None) == -1                   # k > Nt
    assert lib.mmvae_knn_search_l1(C.byref(_args(k=_lib.KNN_MAXK + 1)), None) == -1
    assert lib.mmvae_knn_search_l1(C.byref(_args(k=0)), None) == -1
    assert lib.mmvae_knn_search_l1(C.byref(_args(work=None)), None) == -1                   # split, but no workspace
    assert lib.mmvae_knn_search_l1(C.byref(_args(work_bytes=ops.knn_l1_work_bytes(3, 5000, 5) - 1)), None) == -1
    assert lib.mmvae_knn_search_l1(C.byref(_args(dtype=2)), None) == -2
    for field, value in (("ld_q", 15), ("ld_t", 15), ("ld_idx", 4), ("ld_dist2", 4), ("q", 0x1002), ("idx", 0x3002), ("work", 0x5004),
                         ("Mq", 0), ("F", 0), ("t", None), ("idx", None)):
        a = _args()
        setattr(a, field, value)
        assert lib.mmvae_knn_search_l1(C.byref(a), None) == -1, field


def _weighted(**kw):
    a = dict(idx=0x1000, ld_idx=5, dist=0x2000, ld_dist=5, squared=0, y=0x3000, y_dtype=0, ld_y=8, out=0x4000, ld_out=8, Mq=4, k=5, Ny=10, Fy=8)
    a.update(kw)
    return _lib.load().mmvae_knn_weighted_rows(a["idx"], a["ld_idx"], a["dist"], a["ld_dist"], a["squared"], a["y"], a["y_dtype"], a["ld_y"],
                                               a["out"], a["ld_out"], a["Mq"], a["k"], a["Ny"], a["Fy"], None)


def test_weighted_rows_refuses_without_a_launch():
    for kw in (dict(idx=None), dict(dist=None), dict(y=None), dict(out=None), dict(ld_idx=4), dict(ld_dist=4), dict(ld_y=7), dict(ld_out=7),
               dict(squared=2), dict(squared=-1), dict(Mq=0), dict(k=0), dict(k=_lib.KNN_MAXK + 1, ld_idx=200, ld_dist=200), dict(Ny=0), dict(Fy=0),
               dict(idx=0x1002), dict(dist=0x2002), dict(out=0x4002), dict(y=0x3002), dict(Fy=65535 * 256 + 1, ld_y=1 << 25, ld_out=1 << 25)):
        assert _weighted(**kw) == -1, kw
    assert _weighted(y_dtype=2) == -2
