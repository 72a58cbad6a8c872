"""Layout of the fused class-head launch's argument struct: sizeof / offsetof as gcc lays include/mmvae_hip.h out == the ctypes
mirror (the pattern of tests/test_latent_abi_cpu.py), and the limits mmvae_class_tail_fits answers without a device."""
import ctypes as C

from abi_util import header_facts
from mmvae import _lib, ops


def test_class_tail_struct_matches_c_layout(tmp_path):
    cname, cls = "mmvae_class_tail_args", _lib.ClassTailArgs
    got = header_facts(tmp_path, structs={cname: cls})
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname


def test_class_tail_entry_points_are_bound_and_refuse_without_a_launch():
    assert "mmvae_class_tail" in _lib.EXPORTED and "mmvae_class_tail_fits" in _lib.EXPORTED
    lib = _lib.load()
    assert lib.mmvae_class_tail(None, None) == -1
    a = _lib.ClassTailArgs()                                  # all zero: refused on its shapes before any pointer is looked at
    assert lib.mmvae_class_tail(C.byref(a), None) == -1


def test_class_tail_fits_states_the_limits():
    bf16, f32 = ops.PREC_BF16, ops.PREC_F32
    assert ops.class_tail_fits(bf16, 24, 64, 20, 448, 448) and ops.class_tail_fits(bf16, 32, 64, 24, 64, 64) and ops.class_tail_fits(bf16, 4, 64, 1, 72, 128)
    for bad in ((f32, 24, 64, 20, 448, 448), (bf16, 33, 64, 20, 448, 448), (bf16, 36, 64, 20, 448, 448), (bf16, 22, 64, 20, 448, 448),
                (bf16, 0, 64, 20, 448, 448), (bf16, 24, 128, 20, 448, 448), (bf16, 24, 32, 20, 448, 448), (bf16, 24, 64, 25, 448, 448),
                (bf16, 24, 64, 0, 448, 448), (bf16, 24, 64, 20, 452, 448), (bf16, 24, 64, 20, 56, 448), (bf16, 24, 64, 20, 448, 456),
                (bf16, 24, 64, 20, 448, 32)):
        assert not ops.class_tail_fits(*bad), bad
    lib = _lib.load()
    try:
        assert lib.mmvae_set_tuning(12, 0) == 0
        assert not ops.class_tail_fits(bf16, 24, 64, 20, 448, 448)
    finally:
        assert lib.mmvae_set_tuning(12, 1) == 0
    assert ops.class_tail_fits(bf16, 24, 64, 20, 448, 448)
