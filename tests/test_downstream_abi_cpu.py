"""Layout of the site classifier's argument structs as gcc lays include/mmvae_hip.h out == the ctypes mirror (the pattern of
tests/test_tsne_abi_cpu.py), the entries in the binding, and what they and the Python layer refuse or answer without a device."""
import ctypes as C

import pytest
import torch

from abi_util import header_facts
from mmvae import _lib, downstream, ops

STRUCTS = {"mmvae_ln_act_fwd_args": _lib.LnActFwdArgs, "mmvae_ln_act_bwd_args": _lib.LnActBwdArgs, "mmvae_wce_args": _lib.WceArgs,
           "mmvae_adamw_item": _lib.AdamWItem}
ENTRIES = ("mmvae_ln_act_fwd", "mmvae_ln_act_bwd", "mmvae_ln_act_bwd_work_bytes", "mmvae_wce_mean", "mmvae_adam_step", "mmvae_adamw_step")


def test_structs_match_c_layout(tmp_path):
    got = header_facts(tmp_path, structs=STRUCTS, values={"MAXN": "MMVAE_LN_MAXN", "MAXC": "MMVAE_WCE_MAXC"})
    for cname, cls in STRUCTS.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert int(got["MAXN"]) == _lib.LN_MAXN == 1024 and int(got["MAXC"]) == _lib.WCE_MAXC == 64


def test_entries_are_bound_and_the_abi_version_stays():
    for name in ENTRIES:
        assert name in _lib.EXPORTED
        assert hasattr(_lib.load(), name)
    assert _lib.load().mmvae_abi_version() == 20 == _lib.ABI_VERSION
    assert _lib._SIGNATURES["mmvae_adam_step"] == _lib._SIGNATURES["mmvae_adamw_step"]


def _fwd(**kw):
    """pointers that are never dereferenced: every call below is refused before a launch"""
    a = _lib.LnActFwdArgs(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 128, 128, 128, 33, 128, 1, 1e-5, 1.25, 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_ln_act_fwd_refuses_without_a_launch():
    lib = _lib.load()
    assert lib.mmvae_ln_act_fwd(None, None) == -1
    assert lib.mmvae_ln_act_fwd(C.byref(_lib.LnActFwdArgs()), None) == -1
    for kw in (dict(M=0), dict(N=0), dict(N=126, ldz=126, ldy=126, ld_mask=126), dict(N=1028, ldz=1028, ldy=1028, ld_mask=1028), dict(N=2048),
               dict(ldz=124), dict(ldy=124), dict(ld_mask=124), dict(ldz=130), dict(ldy=130), dict(ld_mask=130),
               dict(z=0), dict(y=0), dict(gamma=0), dict(beta=0), dict(mean=0), dict(rstd=0),
               dict(z=0x1004), dict(y=0x5008), dict(gamma=0x2004), dict(beta=0x3008), dict(mean=0x6002), dict(rstd=0x7001), dict(mask=0x4002),
               dict(eps=0.0), dict(eps=-1.0), dict(inv_keep=0.5), dict(inv_keep=float("nan"))):
        assert lib.mmvae_ln_act_fwd(C.byref(_fwd(**kw)), None) == -1, kw
    # the form without LayerNorm does not look at gamma, beta, mean, rstd or eps -- and still checks the rest
    for kw in (dict(z=0), dict(y=0x5004), dict(N=6, ldz=8, ldy=8, ld_mask=8), dict(mask=0x4001)):
        assert lib.mmvae_ln_act_fwd(C.byref(_fwd(layer_norm=0, gamma=0, beta=0, mean=0, rstd=0, eps=0.0, **kw)), None) == -1, kw


def _bwd(**kw):
    M = 300
    need = ops.ln_act_bwd_work_bytes(M, 128)
    a = _lib.LnActBwdArgs(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000, 0xa000, 0xb000, 128, 128, 128, 128, need, M, 128, 1,
                          1.25)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_ln_act_bwd_refuses_without_a_launch_and_its_planner():
    lib = _lib.load()
    n = C.c_int64(-1)
    for bad in ((0, 128, 1), (5, 0, 1), (5, 126, 1), (5, 1028, 1), (5, 1028, 0)):
        assert lib.mmvae_ln_act_bwd_work_bytes(*bad, C.byref(n)) == -1, bad
    assert lib.mmvae_ln_act_bwd_work_bytes(5, 128, 1, None) == -1
    # a workgroup owns 32 rows; one workgroup writes dgamma / dbeta itself; the form without LayerNorm has no sums
    assert [ops.ln_act_bwd_work_bytes(M, 128) for M in (1, 32, 33, 300)] == [0, 0, 2 * 8 * 128, 10 * 8 * 128]
    assert ops.ln_act_bwd_work_bytes(300, 72) == 10 * 8 * 72 and ops.ln_act_bwd_work_bytes(300, 128, False) == 0
    assert lib.mmvae_ln_act_bwd(None, None) == -1
    assert lib.mmvae_ln_act_bwd(C.byref(_lib.LnActBwdArgs()), None) == -1
    for kw in (dict(M=0), dict(N=0), dict(N=126), dict(N=1028), dict(lddy=124), dict(ldz=130), dict(lddz=124), dict(ld_mask=126),
               dict(dy=0), dict(z=0), dict(dz=0), dict(mean=0), dict(rstd=0), dict(gamma=0), dict(beta=0), dict(dgamma=0), dict(dbeta=0), dict(work=0),
               dict(dy=0x1004), dict(z=0x2008), dict(dz=0x8004), dict(mean=0x3002), dict(rstd=0x4001), dict(gamma=0x5004), dict(beta=0x6008),
               dict(dgamma=0x9002), dict(dbeta=0xa001), dict(mask=0x7002), dict(work=0xb004), dict(inv_keep=0.0),
               dict(work_bytes=ops.ln_act_bwd_work_bytes(300, 128) - 1)):
        assert lib.mmvae_ln_act_bwd(C.byref(_bwd(**kw)), None) == -1, kw


def _wce(**kw):
    a = _lib.WceArgs(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 8, 8, 33, 7)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_wce_mean_refuses_without_a_launch():
    lib = _lib.load()
    assert lib.mmvae_wce_mean(None, None) == -1
    assert lib.mmvae_wce_mean(C.byref(_lib.WceArgs()), None) == -1
    for kw in (dict(M=0), dict(C=1), dict(C=0), dict(C=65, ld=65, ldg=65), dict(ld=6), dict(ldg=6), dict(logits=0), dict(labels=0),
               dict(logits=0x1002), dict(labels=0x2004), dict(class_weights=0x3002), dict(sums=0x4004), dict(g=0x5002), dict(pred=0x6002),
               dict(nll=0x7001), dict(confusion=0x8002), dict(sums=0, g=0, pred=0, nll=0, confusion=0)):
        assert lib.mmvae_wce_mean(C.byref(_wce(**kw)), None) == -1, kw


def test_adam_step_refuses_without_a_launch():
    lib = _lib.load()
    item = lambda **kw: _lib.AdamWItem(**{**dict(p=0x1000, g=0x2000, m=0x3000, v=0x4000, n=10), **kw})
    one = (_lib.AdamWItem * 1)(item())
    args = lambda items, n, bc=(0.1, 0.001), step=None, advance=0: (C.cast(items, C.c_void_p), n, 1e-3, 0.9, 0.999, 1e-8, 1e-4, bc[0], bc[1], 0, step,
                                                                    advance, None, None)
    assert lib.mmvae_adam_step(*args(None, 1)) == -1 and lib.mmvae_adam_step(*args(one, 0)) == -1
    assert lib.mmvae_adam_step(*args(one, 1, bc=(0.0, 0.001))) == -1 and lib.mmvae_adam_step(*args(one, 1, bc=(0.1, 0.0))) == -1
    assert lib.mmvae_adam_step(*args(one, 1, advance=1)) == -1                   # a self-advancing counter needs the counter
    for kw in (dict(p=0), dict(g=0), dict(m=0), dict(v=0), dict(n=0)):
        assert lib.mmvae_adam_step(*args((_lib.AdamWItem * 2)(item(), item(**kw)), 2)) == -1, kw
    many = (_lib.AdamWItem * 65)(*[item() for _ in range(65)])
    assert lib.mmvae_adam_step(*args(many, 65, step=0x9000, advance=1)) == -1


def test_python_layer_refuses_on_the_host_and_bad_arguments():
    z = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ln_act_fwd(z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ln_act_bwd(z, z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.wce_mean(z, torch.zeros(4, dtype=torch.int64), sums=None, pred=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        downstream.cross_validate(torch.zeros(20, 4), torch.zeros(20, dtype=torch.int64), ["a", "b"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        downstream.SiteClassifier(10, 3, device="cpu")
    for kw in (dict(input_dim=0), dict(n_classes=1), dict(n_classes=65), dict(hidden=()), dict(hidden=(256,)), dict(hidden=(250, 128)),
               dict(hidden=(2048, 128)), dict(dropout=(0.3, 1.0)), dict(dropout=(-0.1, 0.2)), dict(batch_size=0), dict(lr=0.0), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            downstream.SiteClassifier(**{**dict(input_dim=10, n_classes=3, device="cuda"), **kw})
    assert downstream.BATCH_SIZE == 32
