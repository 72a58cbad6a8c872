"""MultiModalVAE TRAINING steps on a subset of the modalities and of the loss terms against the numpy oracle, default widths,
B = 1000, both precisions.  The four cases and the engine path each one is chosen for are listed in tests/partial_cases.py; the
oracle side of them is pinned to float64 autograd on the CPU (tests/test_oracle_vs_golden.py).

Every case is run twice on the device -- the loss through the fused loss kernel (F_.fused_loss on the case's terms, or the
public vae_loss where the case has all four), and through stock torch loss functions on the returned outputs with a
grad_output of 2, the general autograd path -- and BOTH runs are compared with the oracle, not with each other.  (The factor 2
is exact in every number format involved, so the second run's reference is the first one's with the gradients doubled.)

  fp32   against the fp64 oracle at TOL["fp32"].
  bf16   against the bf16-aware oracle (q=O.BF16) at tol_q(1000); the deviation from the fp64 oracle is reported and bounded per
         tensor by the bf16-aware oracle's own deviation from the fp64 oracle on the same inputs + tol_q(1000).
Asserted besides: exactly the parameters absent from the oracle's G have .grad None (compare_step); the running statistics of an
encoder that did not run are unchanged bit for bit and num_batches_tracked advanced only for the encoders that ran.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import np_oracle as O  # noqa: E402
from model_util import load_state, masks_list, f64  # noqa: E402
from partial_cases import CASES, ENCODER_OF, mask_names, oracle_partial_step  # noqa: E402
from test_model_gpu import compare_step, oracle_deviation, TOL, tol_q, report, t  # noqa: E402
from mmvae import engine  # noqa: E402
from mmvae import functional as F_  # noqa: E402
from src.models import MultiModalVAE  # noqa: E402
from src.utils import vae_loss  # noqa: E402

DEV = "cuda"
A, D, S, L, E, B = 782, 572, 24, 20, 32, 1000
SEED, BETA, GAMMA = 300, 1e-3, 0.7


@pytest.fixture(scope="module")
def data():
    P, Bf = O.make_params(SEED, A, D, S, L, E)
    a, b, site = O.make_batch(SEED + 1, B, A, D, S)
    masks, eps = O.make_noise(SEED + 2, B, L)
    cw = np.random.default_rng(5).uniform(0.5, 2.0, S).astype(np.float32)
    return dict(P=P, Bf=Bf, P64=f64(P), Bf64=f64(Bf), a=a, b=b, site=site, masks=masks, eps=eps, cw=cw, ref={})


def oracle(data, case, q):
    key = (case, "q" if q is not None else "f")
    if key not in data["ref"]:
        data["ref"][key] = oracle_partial_step(data["P64"], data["Bf64"], data["a"], data["b"], data["site"], data["masks"], data["eps"],
                                               case, BETA, GAMMA, data["cw"], q)
    return data["ref"][key]


def doubled(ref):
    return dict(ref, G={k: 2.0 * v for k, v in ref["G"].items()})


@pytest.mark.parametrize("mode", ["fused", "torch"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["a", "b_site", "a_b", "site"])
def test_partial_step_vs_oracle(data, case, prec, mode):
    c = CASES[case]
    inputs, terms = c["inputs"], c["terms"]
    model = load_state(MultiModalVAE(A, D, S, L, embed_dim=E), data["P"], data["Bf"]).to(DEV).set_precision(prec).train()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    a, b, site, cw = t(data["a"]), t(data["b"]), t(data["site"]), t(data["cw"])
    engine.GLOBAL_NOISE.inject(masks_list(data["masks"], mask_names(case)), torch.from_numpy(data["eps"]))
    try:
        ra, rb, rc, mu, lv = model(a=a if "a" in inputs else None, b=b if "b" in inputs else None, site=site if "site" in inputs else None)
    finally:
        engine.GLOBAL_NOISE.clear()
    if mode == "fused":
        if len(terms) == 4:
            loss, rec_, cls_, kld_ = vae_loss(ra, a, rb, b, rc, site, mu, lv, beta=BETA, gamma=GAMMA, class_weights=cw)
            losses = (loss.item(), rec_, cls_, kld_)
        else:
            full = {"a": (ra, a), "b": (rb, b), "c": (rc, site), "kl": (mu, lv)}
            loss, out5 = F_.fused_loss({k: full[k] for k in terms}, BETA, GAMMA, cw)
            losses = tuple(F_.read_losses(out5))
        loss.backward()
    else:
        zero = torch.zeros((), device=DEV)
        mse = F.mse_loss(ra, a, reduction="sum") if "a" in terms else zero
        bce = F.binary_cross_entropy(rb, b, reduction="sum") if "b" in terms else zero
        cls = F.cross_entropy(rc, site, weight=cw, reduction="sum") if "c" in terms else zero
        kld = -0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp()) if "kl" in terms else zero
        loss = mse + bce + GAMMA * cls + BETA * kld
        (2.0 * loss).backward()                   # grad_output != 1: the gradients arrive through autograd, scaled
        losses = (loss.item(), (mse + bce).item(), cls.item(), kld.item())
    outs = (ra, rb, rc, mu, lv)
    scale = (lambda r: r) if mode == "fused" else doubled
    tag = f"partial inputs={'+'.join(inputs)} terms={'+'.join(terms)} prec={prec} loss={mode} B={B}"

    def line(what, e):
        report(f"{tag} {what}: out {e['out']:.3e}; loss rel {e['loss']:.3e}; grad max scaled {e['grad']:.3e} ({e['grad_worst']}); "
               f"grad max Frobenius-rel {e['fro']:.3e} ({e['fro_worst']}); running statistics {e['bn']:.3e}")
    ref64 = oracle(data, case, None)
    for got, want in zip(losses, ref64["losses"]):
        assert want is not None or got == 0.0, (losses, ref64["losses"])          # a term the step does not have counts nothing
    if prec == "fp32":
        line("vs fp64 reference arithmetic", compare_step(model, outs, losses, scale(ref64), TOL["fp32"]))
    else:
        refq = oracle(data, case, O.BF16)
        line("vs bf16-aware oracle", compare_step(model, outs, losses, scale(refq), tol_q(B)))
        line("vs fp64 reference arithmetic (bound: q-oracle's own deviation + tol_q)",
             compare_step(model, outs, losses, scale(ref64), tol_q(B), base=oracle_deviation(refq, ref64)))
    # the encoders that did not run: statistics untouched, bit for bit; the ones that ran: one more batch tracked
    after = model.state_dict()
    ran = {ENCODER_OF[m] for m in inputs}
    n_bn = 0
    for k, v in before.items():
        top = k.split(".", 1)[0]
        if not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked")):
            assert torch.equal(after[k], v), k                                   # no optimiser step was taken
            continue
        n_bn += 1
        if top not in ran:
            assert torch.equal(after[k], v), k
        elif k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(v) + 1, k
        else:
            assert not torch.equal(after[k], v), k
    assert n_bn == 9
