"""mmvae_recon_metrics: the argument struct as gcc lays include/mmvae_hip.h out == the ctypes mirror (the pattern of
test_latent_abi_cpu.py), the symbol is exported under the unchanged ABI version, and every refusal the header lists returns
MMVAE_ERR_ARG before anything is launched (so these run without a GPU: no pointer is ever dereferenced)."""
import ctypes as C

import pytest

from abi_util import header_facts
from mmvae import _lib


def test_metrics_struct_matches_c_layout(tmp_path):
    cname, cls = "mmvae_metrics_args", _lib.MetricsArgs
    got = header_facts(tmp_path, structs={cname: cls})
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname


def test_metrics_entry_point_is_bound_and_abi_is_unchanged():
    assert "mmvae_recon_metrics" in _lib.EXPORTED and _lib.ABI_VERSION == 20
    lib = _lib.load()
    assert lib.mmvae_abi_version() == 20
    assert lib.mmvae_recon_metrics(None, None) == -1


def _good():
    """Arguments that pass every check: fake, suitably aligned addresses (nothing reads them before the checks)."""
    return dict(M=8, N=6, pred=0x10000, pred_dtype=_lib.F32, ld_pred=6, target=0x20000, target_dtype=_lib.F32, ld_target=6,
                col_shift=None, col_acc=0x30000, row_pearson=0x40000, row_cosine=0x50000)


REFUSALS = {
    "null pred": dict(pred=None),
    "null target": dict(target=None),
    "null col_acc": dict(col_acc=None),
    "null row_pearson": dict(row_pearson=None),
    "null row_cosine": dict(row_cosine=None),
    "M = 0": dict(M=0),
    "M < 0": dict(M=-3),
    "N = 0": dict(N=0),
    "ld_target < N": dict(ld_target=5),
    "ld_target = 0 (no broadcast target)": dict(ld_target=0),
    "0 < ld_pred < N": dict(ld_pred=5),
    "ld_pred < 0": dict(ld_pred=-6),
    "pred dtype": dict(pred_dtype=2),
    "target dtype": dict(target_dtype=-1),
    "bf16 pred at an odd address": dict(pred_dtype=_lib.BF16, pred=0x10001),
    "bf16 target at an odd address": dict(target_dtype=_lib.BF16, target=0x20001, ld_target=8),
    "fp32 target off its element size": dict(target=0x20002),
    "col_acc off 8 bytes": dict(col_acc=0x30004),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_metrics_refusals_return_err_arg_before_any_launch(case):
    lib = _lib.load()
    a = _lib.MetricsArgs(**{**_good(), **REFUSALS[case]})
    assert lib.mmvae_recon_metrics(C.byref(a), None) == -1, case
