"""bf16 input storage, host side: the ABI fields it adds and the no-CPU-fallback rule of its entry points."""
import pytest
import torch

from mmvae import _lib


def test_new_abi_fields_are_last_and_default_to_fp32():
    """h_dtype / a_dtype / b_dtype close their structs (older field offsets unchanged); zero-initialised means MMVAE_F32."""
    assert _lib.ABI_VERSION == 20
    assert _lib.GemmNtArgs._fields_[-1][0] == "h_dtype" and _lib.GemmNtArgs().h_dtype == _lib.F32
    assert [f for f, _ in _lib.LossArgs._fields_[-2:]] == ["a_dtype", "b_dtype"]
    la = _lib.LossArgs()
    assert la.a_dtype == la.b_dtype == _lib.F32
    assert "mmvae_rows_to_bf16" in _lib.EXPORTED


def test_to_bf16_rows_refuses_cpu_tensors():
    from mmvae import to_bf16_rows
    for dt in (torch.float32, torch.bfloat16):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            to_bf16_rows(torch.zeros(4, 782, dtype=dt))


def test_model_refuses_cpu_bf16_inputs():
    from src.models import MultiModalVAE
    m = MultiModalVAE(782, 572, 24, 20)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(a=torch.zeros(4, 782, dtype=torch.bfloat16), b=torch.zeros(4, 572, dtype=torch.bfloat16), site=torch.zeros(4, dtype=torch.int64))
