"""Pins the bf16-AWARE mode of oracle/np_oracle.py (`q=BF16`) -- the yardstick the GPU tests hold the bf16 kernels to at
1e-2 -- against the golden vectors of the imported reference (tests/golden/*.npz, oracle/make_fixtures.py).  CPU only.

Two statements:
  1. With the rounding hook replaced by the identity the q code path IS the fp64 oracle (the path differs in form: it
     back-propagates DecoderB through the logit gradient p - t instead of dL/dp followed by the sigmoid derivative): every
     output, loss term and gradient equal to 1e-9.  A rounding point cannot hide a different algorithm.
  2. With q=BF16 the oracle stays within bf16 storage error of the REFERENCE's numbers: outputs <= 1e-2 of the tensor's
     scale (measured 2.9e-3 .. 4.6e-3), loss terms <= 3e-3 relative (measured <= 2e-4), every gradient <= 0.12
     Frobenius-relative -- the bound tests/test_model_gpu.py holds the bf16 KERNELS to against the fp64 oracle -- with the median
     over the 36 tensors <= 4e-2 (measured: worst 0.071 .. 0.102, always encoder_b.fc.1.bias, then encoder_b.fc.0.weight
     0.069 .. 0.091; median 0.011 .. 0.035 at B = 16 .. 77: gradients summed over a batch whose ReLU gates flip when the stored
     pre-BN output is rounded; the same 0.09-0.10 on that tensor is what the GPU shows against the fp64 oracle at
     B = 1000 .. 65 536).  These are the "fp64-vs-q" figures the GPU parity report quotes."""
import numpy as np
import pytest

import np_oracle as O
from golden_util import load

F64 = np.float64
CHAOTIC_BIASES = ("encoder_a.fc.0.bias", "encoder_b.fc.0.bias", "encoder_b.fc.4.bias")     # analytically zero gradients


def _first_step(fx, q):
    A, D, S, L, E = [int(x) for x in fx["dims"]]
    B, seed = int(fx["B"]), int(fx["seed"])
    cw = fx["class_weights"].astype(F64) if "class_weights" in fx.files else None
    P, Bf = O.make_params(seed, A, D, S, L, E)
    P, Bf = O.cast_tree(P, F64), O.cast_tree(Bf, F64)
    a, b, site = O.make_batch(seed + 1, B, A, D, S)
    state, step = O.adamw_init(P)
    masks, eps = O.make_noise(seed + 100, B, L)
    return O.train_step(P, Bf, state, step, a.astype(F64), b.astype(F64), site, masks, eps.astype(F64), float(fx["beta"]),
                        float(fx["gamma"]), cw, lr=float(fx["lr"]), wd=float(fx["wd"]), q=q)


def _fixture_entry(fx, key, arr):
    """(got, expected) restricted to what the fixture stores (all of it, or a sample of indices)."""
    arr = np.asarray(arr, F64)
    if key in fx.files:
        return arr.reshape(-1), fx[key].astype(F64).reshape(-1)
    return arr.reshape(-1)[fx[key + "@idx"]], fx[key + "@val"].astype(F64)


@pytest.mark.parametrize("name", ["mm_tiny_b16", "mm_default_b32", "mm_default_b77_w"])
def test_identity_hook_is_the_fp64_oracle(name):
    fx = load(name)
    r0, ri = _first_step(fx, None), _first_step(fx, O._id)
    for k in ("out_a", "out_b", "out_c", "mu", "logvar"):
        np.testing.assert_allclose(ri[k], r0[k], rtol=1e-12, atol=0)
    for k in ("total", "recon", "cls", "kld"):
        assert ri[k] == r0[k]
    for k, g in r0["grads"].items():
        if k in CHAOTIC_BIASES:
            assert np.abs(ri["grads"][k]).max() <= 1e-9 * max(1.0, np.abs(r0["grads"]["encoder_b.fc.0.weight"]).max())
            continue
        assert np.linalg.norm(ri["grads"][k] - g) <= 1e-9 * np.linalg.norm(g), k


@pytest.mark.parametrize("name", ["mm_tiny_b16", "mm_default_b32", "mm_default_b77_w"])
def test_bf16_aware_oracle_vs_golden(name):
    fx = load(name)
    rq = _first_step(fx, O.BF16)
    for k in ("out_a", "out_b", "out_c", "mu", "logvar"):
        got, ref = _fixture_entry(fx, "s0." + k, rq[k])
        assert np.abs(got - ref).max() <= 1e-2 * np.abs(ref).max(), k
    np.testing.assert_allclose([rq["total"], rq["recon"], rq["cls"], rq["kld"]], fx["s0.loss"], rtol=3e-3)
    fros = {}
    for k, g in rq["grads"].items():
        if k in CHAOTIC_BIASES:
            continue
        got, ref = _fixture_entry(fx, "s0.grad." + k, g)
        fros[k] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        assert fros[k] <= 0.12, (k, fros[k])
    assert len(fros) == 36 and float(np.median(list(fros.values()))) <= 4e-2
    worst = max(fros, key=fros.get)
    print(f"{name}: worst gradient Frobenius {fros[worst]:.3e} ({worst}), median {np.median(list(fros.values())):.3e}")


def _first_directional_step(fx, kind, q):
    A, D, S, L, E = [int(x) for x in fx["dims"]]
    B, seed = int(fx["B"]), int(fx["seed"])
    P, Bf = O.make_params(seed, A, D, S, L, E)
    P, Bf = O.cast_tree(P, F64), O.cast_tree(Bf, F64)
    a, b, site = O.make_batch(seed + 1, B, A, D, S)
    x, tgt = (a, b) if kind == "rna2dna" else (b, a)
    state, step = O.adamw_init(P)
    masks, eps = O.make_noise(seed + 100, B, L)
    return O.directional_train_step(kind, P, Bf, state, step, x.astype(F64), tgt.astype(F64), site, masks, eps.astype(F64),
                                    float(fx["beta"]), q=q)


@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
def test_identity_hook_is_the_fp64_oracle_directional(kind):
    """The q path of the directional models (for rna2dna: DecoderB back-propagated from the logit gradient) with the identity
    hook against the reference form, to 1e-9 (measured <= 5e-15)."""
    fx = load(kind + "_b32")
    r0, ri = _first_directional_step(fx, kind, None), _first_directional_step(fx, kind, O._id)
    for k in ("out", "mu", "logvar"):
        np.testing.assert_allclose(ri[k], r0[k], rtol=1e-9, atol=0)
    for k in ("total", "recon", "kld"):
        assert abs(ri[k] - r0[k]) <= 1e-9 * abs(r0[k])
    assert set(ri["grads"]) == set(r0["grads"])
    wscale = np.abs(r0["grads"]["encoder_a.fc.0.weight" if kind == "rna2dna" else "encoder_b.fc.0.weight"]).max()
    for k, g in r0["grads"].items():
        if k in CHAOTIC_BIASES:
            assert np.abs(ri["grads"][k]).max() <= 1e-9 * max(1.0, wscale)
            continue
        assert np.linalg.norm(ri["grads"][k] - g) <= 1e-9 * np.linalg.norm(g), k


@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
def test_bf16_aware_oracle_vs_golden_directional(kind):
    """q=BF16 on the directional models stays within this file's bounds of the reference's vectors (measured worst Frobenius:
    0.061 rna2dna, encoder_a.fc.0.weight; 0.087 dna2rna, encoder_b.fc.1.bias)."""
    fx = load(kind + "_b32")
    A, D, S, L, E = [int(x) for x in fx["dims"]]
    ren = O.directional_param_names(kind, A, D, S, L, E)
    rq = _first_directional_step(fx, kind, O.BF16)
    for k in ("out", "mu", "logvar"):
        got, ref = _fixture_entry(fx, "s0." + k, rq[k])
        assert np.abs(got - ref).max() <= 1e-2 * np.abs(ref).max(), k
    np.testing.assert_allclose([rq["total"], rq["recon"], rq["kld"]], fx["s0.loss"], rtol=3e-3)
    fros = {}
    for k, g in rq["grads"].items():
        if k in CHAOTIC_BIASES:
            continue
        top, rest = k.split(".", 1)
        got, ref = _fixture_entry(fx, f"s0.grad.{ren[top]}.{rest}", g)
        fros[k] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        assert fros[k] <= 0.12, (k, fros[k])
    assert len(fros) == len(rq["grads"]) - (1 if kind == "rna2dna" else 2)
    worst = max(fros, key=fros.get)
    print(f"{kind}: worst gradient Frobenius {fros[worst]:.3e} ({worst}), median {np.median(list(fros.values())):.3e}")


def test_bf16_round_is_round_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.005859375, 1.01171875, -3.1415927, 0.0, 65504.0], dtype=np.float32)
    # 1 + 2^-8 is a tie between 1.0 and 1 + 2^-7: to even (1.0); 1 + 3*2^-9 rounds up; 1 + 3*2^-8 is a tie: to even (1 + 2^-6)
    want = np.array([1.0, 1.0, 1.0078125, 1.015625, -3.140625, 0.0, 65536.0], dtype=np.float32)
    np.testing.assert_array_equal(O.bf16_round(x), want)
    import torch
    t = torch.randn(4096, generator=torch.Generator().manual_seed(0))
    np.testing.assert_array_equal(O.bf16_round(t.numpy()), t.bfloat16().float().numpy())
