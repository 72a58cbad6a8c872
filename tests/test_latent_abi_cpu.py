"""Layout of the fused latent launch's argument structs: sizeof / offsetof as gcc lays include/mmvae_hip.h out == the ctypes mirrors
(the pattern of test_host_cpu.test_ctypes_structs_match_c_layout, for the structs added with mmvae_latent_fwd)."""
import ctypes as C

from abi_util import header_facts
from mmvae import _lib


def test_latent_structs_match_c_layout(tmp_path):
    pairs = {"mmvae_latent_enc": _lib.LatentEnc, "mmvae_latent_fwd_args": _lib.LatentFwdArgs}
    got = header_facts(tmp_path, structs=pairs)
    for cname, cls in pairs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)


def test_latent_entry_point_is_bound_and_abi_is_unchanged():
    assert "mmvae_latent_fwd" in _lib.EXPORTED and _lib.ABI_VERSION == 20
    lib = _lib.load()
    assert lib.mmvae_abi_version() == 20
    assert lib.mmvae_latent_fwd(None, None) == -1            # a null argument struct is refused, nothing is launched
