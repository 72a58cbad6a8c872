"""Shared helpers for the GPU parity tests (model construction from oracle parameters, error
metrics).  Test infrastructure only."""
import numpy as np
import torch

import np_oracle as O

CHAOTIC_BIASES = ("encoder_a.fc.0.bias", "encoder_b.fc.0.bias", "encoder_b.fc.4.bias")


def load_state(model, P, Bf, rename=None):
    """Load oracle-named parameters/buffers into a drop-in module (optionally through the
    directional models' sub-module renaming)."""
    sd = {}
    for k, v in list(P.items()) + list(Bf.items()):
        kk = k
        if rename is not None:
            top, rest = k.split(".", 1)
            if top not in rename:
                continue
            kk = rename[top] + "." + rest
        sd[kk] = torch.from_numpy(np.array(v, dtype=np.int64 if np.asarray(v).dtype == np.int64 else np.float32))
    model.load_state_dict(sd, strict=True)
    return model


def masks_list(masks, which=("encoder_a.fc.3", "encoder_b.fc.3", "encoder_b.fc.7")):
    return [torch.from_numpy(masks[k]) for k in which]


def scaled_err(got, ref):
    """max |got - ref| / max |ref|  (error relative to the tensor's scale)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    s = float(np.max(np.abs(ref))) if ref.size else 1.0
    return float(np.max(np.abs(got - ref))) / (s if s > 0 else 1.0)


def named_grads(model, rename=None):
    inv = {v: k for k, v in rename.items()} if rename else None
    out = {}
    for k, p in model.named_parameters():
        if inv is not None:
            top, rest = k.split(".", 1)
            k = inv[top] + "." + rest
        out[k] = None if p.grad is None else p.grad.detach().float().cpu().numpy()
    return out


ADAM_SHARE = {"fp32": 2e-3, "bf16": 2e-2}


def check_params_after_adamw(model, P1, lr, prec, rename=None):
    """Parameters after ONE AdamW step against the oracle's update of ITS gradients (P1, oracle names), in the form of
    tests/test_fullsize_gpu.py::test_full_step_at_batch_65536: a first Adam step moves every element by ~lr, and an element
    whose gradient is rounding noise may take the other sign -- the share of elements off by more than 1e-6 stays <= 2e-3
    (fp32) / 2e-2 (bf16) per tensor and none is further off than 2.1 lr.  The analytically zero biases are skipped.
    -> (worst share, worst distance)."""
    inv = {v: k for k, v in rename.items()} if rename else None
    worst_share = worst_d = 0.0
    for k, p in model.named_parameters():
        if inv is not None:
            top, rest = k.split(".", 1)
            k = inv[top] + "." + rest
        if k in CHAOTIC_BIASES:
            continue
        d = np.abs(p.detach().cpu().numpy() - P1[k])
        share = float(np.mean(d > 1e-6))
        worst_share, worst_d = max(worst_share, share), max(worst_d, float(d.max()))
        assert share <= ADAM_SHARE[prec] and d.max() <= 2.1 * lr, (k, float(d.max()), share)
    return worst_share, worst_d


def f64(d):
    return O.cast_tree(d, np.float64)
