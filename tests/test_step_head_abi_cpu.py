"""The merged head-of-step launch (mmvae_step_head) and the riders of the grouped dW launch (mmvae_gemm_tn_group_riders) as the
binding sees them, without a device: both symbols exported at the unchanged ABI version, the ctypes mirrors of their two argument
structs laid out as gcc lays include/mmvae_hip.h out (the pattern of tests/test_class_tail_abi_cpu.py), refusals that need no launch,
and the tuning keys 13 / 14 that switch them off."""
import ctypes as C

from abi_util import header_facts
from mmvae import _lib


def test_both_symbols_are_exported_at_abi_20():
    assert "mmvae_step_head" in _lib.EXPORTED and "mmvae_gemm_tn_group_riders" in _lib.EXPORTED
    lib = _lib.load()
    assert hasattr(lib, "mmvae_step_head") and hasattr(lib, "mmvae_gemm_tn_group_riders")
    assert _lib.ABI_VERSION == 20 and lib.mmvae_abi_version() == 20


def test_structs_match_c_layout(tmp_path):
    structs = {"mmvae_step_head_args": _lib.StepHeadArgs, "mmvae_tn_riders": _lib.TnRiders}
    got = header_facts(tmp_path, structs=structs, values={"zero_max": "MMVAE_HEAD_ZERO_MAX"})
    assert int(got["zero_max"]) == _lib.HEAD_ZERO_MAX
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)


def _one_problem():
    """A problem record the grouped entry point gets as far as classifying (it never launches: the riders are refused first, or the
    record's NULL operands are)."""
    arr = (_lib.GemmTnArgs * 1)()
    arr[0].prec, arr[0].M, arr[0].N, arr[0].K = _lib.PREC_BF16, 256, 24, 64
    return arr


def test_null_and_empty_arguments_are_refused():
    lib = _lib.load()
    assert lib.mmvae_step_head(None, None) == -1
    assert lib.mmvae_step_head(C.byref(_lib.StepHeadArgs()), None) == -1           # every role empty
    a = _lib.StepHeadArgs()
    a.n_zero, a.zero_bytes[0] = 1, 16                                               # a range without an address
    assert lib.mmvae_step_head(C.byref(a), None) == -1
    a = _lib.StepHeadArgs()
    a.n_zero = _lib.HEAD_ZERO_MAX + 1
    assert lib.mmvae_step_head(C.byref(a), None) == -1
    a = _lib.StepHeadArgs()
    a.S, a.E, a.L = 24, 32, 20                                                      # a table without operands
    assert lib.mmvae_step_head(C.byref(a), None) == -1
    a = _lib.StepHeadArgs()
    a.n_prep = 3                                                                    # items without a table of them
    assert lib.mmvae_step_head(C.byref(a), None) == -1
    a = _lib.StepHeadArgs()
    a.n_eps, a.keep_prob = 8, 0.9                                                   # noise without a destination
    assert lib.mmvae_step_head(C.byref(a), None) == -1

    arr = _one_problem()
    assert lib.mmvae_gemm_tn_group_riders(C.cast(arr, C.c_void_p), 1, None, None) == -1
    assert lib.mmvae_gemm_tn_group_riders(C.cast(arr, C.c_void_p), 1, C.byref(_lib.TnRiders()), None) == -1      # no rider named
    r = _lib.TnRiders()
    r.S, r.E, r.L = 24, 32, 20                                                      # EncoderC rider without operands
    assert lib.mmvae_gemm_tn_group_riders(C.cast(arr, C.c_void_p), 1, C.byref(r), None) == -1
    buf = (C.c_double * 5)()
    r = _lib.TnRiders()
    r.sums = C.addressof(buf)                                                       # loss rider without its output
    assert lib.mmvae_gemm_tn_group_riders(C.cast(arr, C.c_void_p), 1, C.byref(r), None) == -1
    r.out5 = C.addressof(buf)
    assert lib.mmvae_gemm_tn_group_riders(None, 1, C.byref(r), None) == -1
    assert lib.mmvae_gemm_tn_group_riders(C.cast(arr, C.c_void_p), 1, C.byref(r), None) == -1      # the problem has no operands


def test_keys_13_and_14_toggle_and_key_11_stays_invalid():
    lib = _lib.load()
    assert lib.mmvae_set_tuning(11, 1) == -1
    buf = (C.c_double * 5)()
    for key in (13, 14):
        try:
            assert lib.mmvae_set_tuning(key, 0) == 0
            # off: refused whatever the arguments are (these would otherwise get past the first checks)
            a = _lib.StepHeadArgs()
            a.n_zero, a.zero_ptr[0], a.zero_bytes[0] = 1, 16, 0
            assert lib.mmvae_step_head(C.byref(a), None) == -1
            r = _lib.TnRiders()
            r.sums = r.out5 = C.addressof(buf)
            assert lib.mmvae_gemm_tn_group_riders(C.cast(_one_problem(), C.c_void_p), 1, C.byref(r), None) == -1
        finally:
            assert lib.mmvae_set_tuning(key, 1) == 0
