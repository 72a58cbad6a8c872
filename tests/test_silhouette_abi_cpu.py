"""Layout of mmvae_silhouette_args as gcc lays include/mmvae_hip.h out == the ctypes mirror (the pattern of tests/test_knn_abi_cpu.py),
the silhouette entries in the binding, and what they and the Python wrappers refuse or answer without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_util import header_facts
from mmvae import _lib, clustering, ops


def test_silhouette_struct_matches_c_layout(tmp_path):
    cname, cls = "mmvae_silhouette_args", _lib.SilhouetteArgs
    got = header_facts(tmp_path, structs={cname: cls}, values={"MAXC": "MMVAE_SIL_MAXC"})
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    assert int(got["MAXC"]) == _lib.SIL_MAXC == 64


def test_silhouette_entries_are_bound_and_the_abi_version_stays():
    for name in ("mmvae_silhouette_samples", "mmvae_silhouette_work_bytes", "mmvae_silhouette_splits"):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.load(), name)
    assert _lib.load().mmvae_abi_version() == 20


def _args(N=300, F=16, n_classes=4, splits=0, work_bytes=None, dtype=0):
    """pointers that are never dereferenced: every call below is refused before a launch"""
    ok = N >= 2 and 1 <= n_classes <= _lib.SIL_MAXC and 0 <= splits <= 64
    need = ops.silhouette_work_bytes(N, n_classes, splits) if ok else 1 << 30
    return _lib.SilhouetteArgs(0x1000, None, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, F, need if work_bytes is None else work_bytes,
                               N, F, n_classes, splits, dtype, 0)


def test_silhouette_samples_refuses_without_a_launch():
    lib = _lib.load()
    assert lib.mmvae_silhouette_samples(None, None) == -1
    assert lib.mmvae_silhouette_samples(C.byref(_lib.SilhouetteArgs()), None) == -1
    for kw in (dict(N=1), dict(N=0), dict(F=0), dict(n_classes=0), dict(n_classes=_lib.SIL_MAXC + 1), dict(splits=-1), dict(splits=65)):
        assert lib.mmvae_silhouette_samples(C.byref(_args(**kw)), None) == -1, kw
    need = ops.silhouette_work_bytes(300, 4, 0)
    assert lib.mmvae_silhouette_samples(C.byref(_args(work_bytes=need - 1)), None) == -1            # short workspace
    assert lib.mmvae_silhouette_samples(C.byref(_args(dtype=2)), None) == -2                        # neither fp32 nor bf16
    for field, value in (("ld_x", 15), ("x", 0), ("class_start", 0), ("s", 0), ("work", 0), ("x", 0x1002), ("shift", 0x1002), ("order", 0x2002),
                         ("class_start", 0x3001), ("s", 0x4002), ("intra", 0x5002), ("inter", 0x6001), ("work", 0x7004)):
        a = _args()
        setattr(a, field, value)
        assert lib.mmvae_silhouette_samples(C.byref(a), None) == -1, (field, value)
    a = _args(dtype=1)                                                                              # bf16 rows are aligned to 2 bytes
    a.x = 0x1001
    assert lib.mmvae_silhouette_samples(C.byref(a), None) == -1


def test_silhouette_work_bytes_and_splits_need_no_device():
    lib = _lib.load()
    n, ns = C.c_int64(-1), C.c_int32(-1)
    for bad in ((1, 2, 0), (10, 0, 0), (10, _lib.SIL_MAXC + 1, 0), (10, 2, -1), (10, 2, 65)):
        assert lib.mmvae_silhouette_work_bytes(*bad, C.byref(n)) == -1, bad
        assert lib.mmvae_silhouette_splits(*bad, C.byref(ns)) == -1, bad
    assert lib.mmvae_silhouette_work_bytes(10, 2, 0, None) == -1 and lib.mmvae_silhouette_splits(10, 2, 0, None) == -1
    # enough row blocks: one split, the workspace holds the rows' norms only
    assert ops.silhouette_splits(1 << 18, 24) == 1
    assert ops.silhouette_work_bytes(1 << 18, 24) == 4 * (1 << 18)
    assert ops.silhouette_work_bytes(1001, 3, 1) == 4 * 1002
    # the evaluation's shape: 410 row blocks are below 4 x 256, three splits reach it
    assert ops.silhouette_splits(52429, 24) == 3
    assert ops.silhouette_work_bytes(52429, 24) == (4 * 52429 + 7) // 8 * 8 + 4 * 52429 * 3 * 24
    # a forced count is kept up to the bound of the number of column tiles that needs no device: min(N, (N + 127 C) / 128)
    assert ops.silhouette_splits(52429, 24, 7) == 7 and ops.silhouette_splits(52429, 24, 64) == 64
    assert ops.silhouette_splits(1000, 5) == ops.silhouette_splits(1000, 5, 64) == (1000 + 127 * 5) // 128 == 12
    assert ops.silhouette_splits(3, 2, 64) == 2 and ops.silhouette_splits(300, 1) == 3
    assert ops.silhouette_work_bytes(1000, 5, 3) == 4000 + 4 * 1000 * 3 * 5


def test_python_wrappers_refuse_on_the_host():
    x = torch.zeros(6, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clustering.silhouette_samples(x, [0, 0, 1, 1, 2, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clustering.silhouette_score(x, [0, 0, 1, 1, 2, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.silhouette_samples(x, None, torch.tensor([0, 3, 6], dtype=torch.int32))
    for labels, n in (([0] * 6, 1), (list(range(6)), 6)):
        with pytest.raises(ValueError, match=f"Number of labels is {n}. Valid values are 2 to n_samples - 1"):
            clustering._encode(labels, 6, "cpu")
    with pytest.raises(ValueError, match="at most 64"):
        clustering._encode(np.arange(200) % 65, 200, "cpu")
    with pytest.raises(ValueError, match="integer"):
        clustering._encode(np.zeros(6), 6, "cpu")
    with pytest.raises(ValueError):
        clustering._encode([0, 1, 0], 6, "cpu")
    with pytest.raises(ValueError, match="euclidean"):
        clustering.silhouette_samples(x, [0, 0, 1, 1, 2, 2], metric="cosine")


def test_label_encoding_and_standardize_on_the_host():
    order, start = clustering._encode(np.array([40, 3, 17, 3, 40, 40]), 6, "cpu")
    assert order.dtype == start.dtype == torch.int32
    assert order.tolist() == [1, 3, 2, 0, 4, 5] and start.tolist() == [0, 2, 3, 6]
    assert clustering.neighborhood_hit is __import__("mmvae.knn", fromlist=["x"]).neighborhood_hit
    import silhouette_ref as SR
    g = np.random.default_rng(5)
    x = (5.0 + 3.0 * g.standard_normal((50, 6))).astype(np.float32)
    x[:, 2], x[:, 4] = 0.1, 7.0
    z = clustering.standardize(torch.from_numpy(x))
    assert z.dtype == torch.float32 and z.is_contiguous()
    ref = SR.standardize(x)
    assert np.abs(z.double().numpy() - ref).max() <= 2.0 ** -24 * np.abs(ref).max() + 1e-12
