"""Layout of the fused class-head launch's argument struct: sizeof / offsetof as gcc lays include/mmvae_hip.h out == the ctypes
mirror (the pattern of tests/test_latent_abi_cpu.py), and the limits mmvae_class_tail_fits answers without a device."""
import ctypes as C
import os
import subprocess

from mmvae import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_class_tail_struct_matches_c_layout(tmp_path):
    cname, cls = "mmvae_class_tail_args", _lib.ClassTailArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mmvae_hip.h"', "int main(void) {",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
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
