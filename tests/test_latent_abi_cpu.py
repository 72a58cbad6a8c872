"""Layout of the fused latent launch's argument structs: sizeof / offsetof as gcc lays include/mmvae_hip.h out == the ctypes mirrors
(the pattern of test_host_cpu.test_ctypes_structs_match_c_layout, for the structs added with mmvae_latent_fwd)."""
import ctypes as C
import os
import subprocess

from mmvae import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_latent_structs_match_c_layout(tmp_path):
    pairs = {"mmvae_latent_enc": _lib.LatentEnc, "mmvae_latent_fwd_args": _lib.LatentFwdArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mmvae_hip.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)


def test_latent_entry_point_is_bound_and_abi_is_unchanged():
    assert "mmvae_latent_fwd" in _lib.EXPORTED and _lib.ABI_VERSION == 20
    lib = _lib.load()
    assert lib.mmvae_abi_version() == 20
    assert lib.mmvae_latent_fwd(None, None) == -1            # a null argument struct is refused, nothing is launched
