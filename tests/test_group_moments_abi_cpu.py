"""The group-moments entry points without a device: exported and bound at ABI 20, the argument struct as gcc lays
include/mmvae_hip.h out == the ctypes mirror, every refusal of the header's list of limits (issued with HOST pointers, which a
refused call never reads), and mmvae_gemm_nt_group_moments_fits giving the entry point's answers."""
import ctypes as C

import pytest

from abi_util import header_facts
from mmvae import _lib, ops

BF16, F32 = ops.PREC_BF16, ops.PREC_F32
NONE, RELU, SIGMOID = ops.ACT_NONE, ops.ACT_RELU, ops.ACT_SIGMOID


def test_symbols_are_exported_and_bound_at_abi_20():
    assert _lib.ABI_VERSION == 20 and _lib.load().mmvae_abi_version() == 20
    for name in ("mmvae_gemm_nt_group_moments", "mmvae_gemm_nt_group_moments_fits"):
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name)


def test_struct_matches_c_layout(tmp_path):
    cname, cls = "mmvae_group_moments_args", _lib.GroupMomentsArgs
    got = header_facts(tmp_path, structs={cname: cls})
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname


class Host:
    """Host buffers that stand in for the operands: aligned as asked, never read by a refused call"""

    def __init__(self):
        self.raw = (C.c_char * 4096)()
        self.base = (C.addressof(self.raw) + 127) & ~127

    def args(self, **kw):
        a = _lib.GroupMomentsArgs()
        a.prec, a.B, a.G, a.N, a.K, a.act = BF16, 4, 24, 40, 128, NONE
        a.a, a.lda, a.w, a.ldw, a.bias = self.base, 128, self.base + 1024, 128, self.base + 2048
        a.mean, a.ld_mean, a.std, a.ld_std = self.base + 2560, 40, self.base + 3072, 48
        for k, v in kw.items():
            setattr(a, k, v)
        return a


def fits_of(a):
    return _lib.load().mmvae_gemm_nt_group_moments_fits(a.prec, a.B, a.G, a.N, a.K, a.act, int(bool(a.std)), a.lda, a.ldw)


# what the shape answer covers: (field overrides, status)
SHAPE_REFUSALS = [
    (dict(prec=F32), -2), (dict(prec=7), -1),
    (dict(B=0), -1), (dict(G=0), -1), (dict(G=129), -1), (dict(G=1), -1),                 # G = 1 with std given
    (dict(K=0), -1), (dict(K=32), -1), (dict(K=96, lda=96), -1), (dict(K=576, lda=576, ldw=576), -1),
    (dict(N=0), -1), (dict(act=RELU), -1), (dict(act=3), -1),
    (dict(lda=132), -1), (dict(lda=64), -1), (dict(ldw=160), -1), (dict(ldw=64), -1),
    (dict(B=1 << 20, G=128, lda=512, K=512, ldw=512), -1),                                # B G lda 2 bytes >= 2^32
    (dict(N=(1 << 23), ldw=128), -1),                                                      # (N + 256) ldw 4 >= 2^32
]
# what only the entry point sees: pointers and output strides
OPERAND_REFUSALS = [dict(a=0), dict(w=0), dict(mean=0), dict(ld_mean=39), dict(ld_std=39)]


@pytest.mark.parametrize("over,want", SHAPE_REFUSALS, ids=lambda x: str(x))
def test_shape_refusals_and_fits_agree(over, want):
    a = Host().args(**over)
    assert _lib.load().mmvae_gemm_nt_group_moments(C.byref(a), None) == want
    assert fits_of(a) == want


def test_operand_refusals():
    h, lib = Host(), _lib.load()
    assert lib.mmvae_gemm_nt_group_moments(None, None) == -1
    for over in OPERAND_REFUSALS:
        assert lib.mmvae_gemm_nt_group_moments(C.byref(h.args(**over)), None) == -1, over
    for field, off in (("a", 8), ("w", 8), ("mean", 2), ("std", 2)):
        a = h.args()
        setattr(a, field, getattr(a, field) + off)
        assert lib.mmvae_gemm_nt_group_moments(C.byref(a), None) == -1, field
        assert fits_of(a) == 0                                  # the shape is fine: the refusal is the pointer's


def test_fits_accepts_the_limits_edges():
    f = ops.group_moments_fits
    assert f(BF16, 4096, 24, 782, 128) and f(BF16, 4096, 32, 572, 512, SIGMOID, True)
    assert f(BF16, 1, 1, 1, 64) and f(BF16, 1, 128, 1, 512, NONE, True) and f(BF16, 1, 2, 8, 64, NONE, True)
    assert not f(BF16, 1, 1, 8, 64, NONE, True) and not f(F32, 4096, 24, 782, 128) and not f(BF16, 1, 129, 8, 64)
    assert _lib.load().mmvae_set_tuning(16, 0) == -1           # no tuning key came with the kernel
