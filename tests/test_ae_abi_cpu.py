"""The autoencoders' latent-path entry points (mmvae_embed_proj_fwd / _bwd, mmvae_fuse_mean_fwd / _bwd, mmvae_ae_latent_fwd) as the binding sees them,
without a device: the symbols exported and bound at the unchanged ABI version, the ctypes mirrors of the two argument structs laid out
as gcc lays include/mmvae_hip.h out, and the refusals that need no launch -- the LDS capacity of mmvae_embed_proj_bwd, an n_mod that
is not the number of modalities present, missing operands, and for the fused latent launch L = 25, K = 288, N_stem = 100, fp32, a
misaligned z / h0 and tuning key 15.  The pointers handed over are host addresses that a refused call never
reads."""
import ctypes as C

from abi_util import header_facts
from mmvae import _lib

SYMBOLS = ("mmvae_embed_proj_fwd", "mmvae_embed_proj_bwd", "mmvae_fuse_mean_fwd", "mmvae_fuse_mean_bwd", "mmvae_ae_latent_fwd")


def test_symbols_are_exported_and_bound_at_abi_20():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED and name in _lib._SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name]
    assert _lib.ABI_VERSION == 20 and lib.mmvae_abi_version() == 20


def test_structs_match_c_layout(tmp_path):
    structs = {"mmvae_fuse_mean_fwd_args": _lib.FuseMeanFwdArgs, "mmvae_fuse_mean_bwd_args": _lib.FuseMeanBwdArgs,
               "mmvae_ae_latent_fwd_args": _lib.AELatentFwdArgs}
    got = header_facts(tmp_path, structs=structs, values={"copies": "MMVAE_TABLE_COPIES"})
    assert int(got["copies"]) == _lib.TABLE_COPIES
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)


def test_embed_proj_refusals_need_no_device():
    lib = _lib.load()
    buf = (C.c_float * 4)()
    p = C.addressof(buf)                                                            # never read: every call below is refused first
    assert lib.mmvae_embed_proj_fwd(0, 32, 20, p, p, p, p, None) == -1
    assert lib.mmvae_embed_proj_fwd(24, 32, 20, p, p, None, p, None) == -1
    assert lib.mmvae_embed_proj_bwd(24, 32, 20, p, p, None, 8, p, p, p, None) == -1
    assert lib.mmvae_embed_proj_bwd(24, 32, 20, p, p, p, 8, p, None, p, None) == -1
    # the LDS capacity, for one head: (S L + S E + L E) * 4 bytes beyond 160 KiB (77 sites x latent 256 x embed 64 = 160.25 KiB; one site
    # fewer is a launch, which this file must not make: the buffer is four host floats)
    S, E, L = 77, 64, 256
    assert (S * L + S * E + L * E) * 4 > 160 * 1024 >= ((S - 1) * L + (S - 1) * E + L * E) * 4
    assert lib.mmvae_embed_proj_bwd(S, E, L, p, p, p, 8, p, p, p, None) == -1


def test_fuse_mean_refusals_need_no_device():
    lib = _lib.load()
    buf = (C.c_float * 4)()
    p = C.addressof(buf)
    assert lib.mmvae_fuse_mean_fwd(None, None) == -1 and lib.mmvae_fuse_mean_bwd(None, None) == -1

    def fwd(n_mod, head=p, table=None, site=None, S=0, L=4, ldz=8, zdt=_lib.F32, latent=p, z=p):
        return lib.mmvae_fuse_mean_fwd(C.byref(_lib.FuseMeanFwdArgs(16, L, n_mod, head, L, table, site, S, latent, z, zdt, ldz)), None)
    assert fwd(2) == -1 and fwd(0) == -1 and fwd(0, head=None) == -1                # n_mod is not the number of modalities present
    assert fwd(1, table=p, site=p, S=3) == -1 and fwd(3, table=p, site=p, S=3) == -1
    assert fwd(2, table=p, site=None, S=3) == -1 and fwd(2, table=p, site=p, S=0) == -1
    assert fwd(1, ldz=3) == -1 and fwd(1, latent=None) == -1 and fwd(1, z=None) == -1
    assert fwd(1, zdt=5) == -2

    def bwd(n_mod=1, dz=p, d_head=p, table=None, site=None, S=0, ld_lp=0, lp=None):
        return lib.mmvae_fuse_mean_bwd(C.byref(_lib.FuseMeanBwdArgs(16, 4, n_mod, dz, 4, None, d_head, 4, lp, ld_lp, table, site, S, 8)), None)
    assert bwd(n_mod=0) == -1 and bwd(n_mod=3) == -1 and bwd(dz=None) == -1 and bwd(d_head=None) == -1
    assert bwd(table=p, site=None, S=3) == -1 and bwd(table=p, site=p, S=0) == -1
    assert bwd(lp=p, ld_lp=2) == -1


def _fused_args(buf):
    """an AELatentFwdArgs the entry point would take (RNA2DNAAE's shapes) if its addresses were device memory: 128-byte aligned host
    addresses that a refused call never reads"""
    p = (C.addressof(buf) + 127) & ~127
    a = _lib.AELatentFwdArgs()
    a.prec, a.B, a.L, a.n_mod = _lib.PREC_BF16, 64, 20, 2
    a.enc.y, a.enc.ldy, a.enc.K, a.enc.scale, a.enc.shift = p, 128, 128, p, p
    a.enc.w, a.enc.ldw, a.enc.bias = p, 128, p
    a.table, a.site, a.S = p, p, 24
    a.latent, a.z, a.ldz = p, p, 24
    a.w_stem, a.ldw_stem, a.bias_stem, a.N_stem = p, 64, p, 256
    a.h0, a.ldh0 = p, 256
    return a


def test_fused_latent_launch_refusals_need_no_device():
    lib = _lib.load()
    buf = (C.c_char * 512)()
    assert lib.mmvae_ae_latent_fwd(None, None) == -1

    def call(**changes):
        a = _fused_args(buf)
        for path, v in changes.items():
            obj, *rest = a, *path.split("__")
            for h in rest[:-1]:
                obj = getattr(obj, h)
            setattr(obj, rest[-1], v)
        return lib.mmvae_ae_latent_fwd(C.byref(a), None)
    p = _fused_args(buf).z
    assert call(L=25) == -1 and call(enc__K=288) == -1 and call(N_stem=100) == -1
    assert call(prec=_lib.PREC_F32) == -2                                           # fp32: MMVAE_ERR_DTYPE
    assert call(z=p + 8) == -1 and call(h0=p + 64) == -1 and call(ldz=28) == -1 and call(ldh0=264) == -1      # misaligned z / h0
    assert call(n_mod=1) == -1 and call(n_mod=3) == -1 and call(site=None) == -1 and call(S=52) == -1
    assert call(latent=None) == -1 and call(w_stem=None) == -1 and call(enc__w=None) == -1
    try:
        assert lib.mmvae_set_tuning(15, 0) == 0
        assert call() == -1                                                         # the key off: refused whatever the arguments
    finally:
        assert lib.mmvae_set_tuning(15, 1) == 0
    assert lib.mmvae_set_tuning(16, 1) == -1
