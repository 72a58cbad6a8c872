"""RNA2DNAVAE / DNA2RNAVAE training steps against the numpy oracle at the default widths (782 / 572 / 24 / 20 / 32), in both
precisions and in the form the captured step runs them.

A one-decoder graph has no merged decoder stem (VAEGraph.dec_stem is None), so none of the fused latent launch, the merged first
decoder layer or the merged stem dX that the multimodal oracle tests pin is on its path.  It runs the decoder's own first-layer
GEMM on z (K = 20 padded to 24), its own layer-0 dX GEMM into an fp32 dz, mmvae_fuse_reparam_bwd with n_mod = 2 and a zero pack
with one MLP encoder missing.

  fp32, B = 1000              against the fp64 oracle at TOL["fp32"]: outputs, mu, logvar, the three loss floats, every gradient
                              (Frobenius and scaled max), running statistics.  1000 = 7 x 128 + 104 and 1000 % 32 = 8: row tails
                              in the NT and in the dW kernels.
  bf16, B = 1000 and 4096     against the bf16-aware oracle (q=O.BF16) at tol_q(B), the bound the multimodal step is held to.  The
                              deviation from the fp64 oracle is reported and bounded PER TENSOR by the bf16-aware oracle's own
                              deviation from the fp64 oracle on the same inputs (computed here) + tol_q(B): the fixed 0.12 / 0.25
                              would leave a margin nobody measured (the q-oracle alone sits at 0.10 Frobenius on
                              encoder_b.fc.1.bias for dna2rna).
  bf16, B = 16384             the smallest batch at which these graphs reach the wave-specialised NT kernel (minimum M 16384, with
                              pro_out) and the wide-tile dW kernels with the folded BatchNorm-backward finalize (M >= 8192).
  the captured step's form    eager, bf16, B = 1000 and 16384: g.fused_recon = [target], F_.fused_loss on the single
                              reconstruction term + KL with unit_grad=True (what GraphedTrainStep(kind=...) issues): the loss
                              floats and every gradient against the bf16-aware oracle at tol_q(B), NOT against the un-fused device
                              run; once more with input and target in bf16 storage (padded bf16 rows), pre-rounded on both sides.
  AdamW on top                once per kind and precision: parameters after opt.step() against O.adamw_step of the oracle's
                              gradients (model_util.check_params_after_adamw).
The measured figures go to the parity report (test_model_gpu.report).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import np_oracle as O  # noqa: E402
from model_util import load_state, masks_list, f64, check_params_after_adamw  # noqa: E402
from test_model_gpu import compare_step, oracle_deviation, TOL, tol_q, report, t  # noqa: E402
from mmvae import engine, to_bf16_rows  # noqa: E402
from mmvae import functional as F_  # noqa: E402
from mmvae.optim import FusedAdamW  # noqa: E402
from src.models import RNA2DNAVAE, DNA2RNAVAE  # noqa: E402
from src.utils.directional_losses import rna2dna_loss, dna2rna_loss  # noqa: E402

DEV = "cuda"
A, D, S, L, E = 782, 572, 24, 20, 32
BETA, LR, WD = 1e-3, 5e-4, 1e-5
MASKS = {"rna2dna": ("encoder_a.fc.3",), "dna2rna": ("encoder_b.fc.3", "encoder_b.fc.7")}
OUTS = ("out", "mu", "logvar")
_cases = {}


def case(kind, B, dims=(A, D, S, L, E), settle=False):
    """Seeded inputs of one (kind, batch, widths), built once and left unchanged; the oracle results are kept with them.
    settle: no kept ReLU gate of the encoder within fp32 rounding of zero (width_cases.settle_gates)."""
    key = (kind, B, tuple(dims), settle)
    if key not in _cases:
        seed = 100 + B
        A_, D_, S_, L_, E_ = dims
        P, Bf = O.make_params(seed, A_, D_, S_, L_, E_)
        a, b, site = O.make_batch(seed + 1, B, A_, D_, S_)
        masks, eps = O.make_noise(seed + 2, B, L_)
        x, tgt = (a, b) if kind == "rna2dna" else (b, a)
        if settle:
            import width_cases as W
            masks, _ = W.settle_gates(masks, W.directional_gates(kind, f64(P), f64(Bf), x.astype(np.float64), site, eps.astype(np.float64)))
        _cases[key] = dict(kind=kind, B=B, dims=tuple(dims), P=P, Bf=Bf, P64=f64(P), Bf64=f64(Bf), x=x, tgt=tgt, site=site, masks=masks, eps=eps,
                           ren=O.directional_param_names(kind, A_, D_, S_, L_, E_), ref={})
    return _cases[key]


def oracle(c, q, rounded=False):
    """One oracle step (forward, loss, backward, AdamW at LR / WD) -> the dict compare_step takes, + P1: the parameters after the
    update.  rounded: input and target pre-rounded to bf16 (bf16 storage)."""
    key = ("q" if q is not None else "f", rounded)
    if key not in c["ref"]:
        f = np.float64
        x, tgt = (O.bf16_round(c["x"]), O.bf16_round(c["tgt"])) if rounded else (c["x"], c["tgt"])
        P1, Bf1 = {k: v.copy() for k, v in c["P64"].items()}, dict(c["Bf64"])
        st, step = O.adamw_init(P1)
        r = O.directional_train_step(c["kind"], P1, Bf1, st, step, x.astype(f), tgt.astype(f), c["site"], c["masks"], c["eps"].astype(f),
                                     BETA, LR, WD, q)
        c["ref"][key] = dict(out=r["out"], mu=r["mu"], logvar=r["logvar"], losses=(r["total"], r["recon"], r["kld"]), G=r["grads"],
                             Bf=Bf1, P1=P1)
    return c["ref"][key]


def build(c, prec):
    cls = RNA2DNAVAE if c["kind"] == "rna2dna" else DNA2RNAVAE
    A_, D_, S_, L_, E_ = c["dims"]
    model = load_state(cls(A_, D_, S_, L_, embed_dim=E_), c["P"], c["Bf"], c["ren"]).to(DEV).set_precision(prec).train()
    return model, FusedAdamW(model.parameters(), lr=LR, weight_decay=WD)


def forward(model, c, x, site, fused_target=None):
    """One training forward with the case's noise injected; fused_target: the captured step's form (the reconstruction loss
    inside the decoder's last GEMM)."""
    engine.GLOBAL_NOISE.inject(masks_list(c["masks"], MASKS[c["kind"]]), torch.from_numpy(c["eps"]))
    g = model._graph()
    g.fused_recon = None if fused_target is None else [fused_target]
    try:
        return model(rna=x, site=site) if c["kind"] == "rna2dna" else model(dna=x, site=site)
    finally:
        g.fused_recon = None
        engine.GLOBAL_NOISE.clear()


def line(tag, e):
    report(f"{tag}: out {e['out']:.3e}; loss rel {e['loss']:.3e}; grad max scaled {e['grad']:.3e} ({e['grad_worst']}); "
           f"grad max Frobenius-rel {e['fro']:.3e} ({e['fro_worst']}); running statistics {e['bn']:.3e}")


@pytest.mark.parametrize("prec,B", [("fp32", 1000), ("bf16", 1000), ("bf16", 4096), ("bf16", 16384)])
@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
def test_directional_step_vs_oracle(kind, prec, B):
    c = case(kind, B)
    model, opt = build(c, prec)
    x, tgt, site = t(c["x"]), t(c["tgt"]), t(c["site"])
    rec, mu, lv = forward(model, c, x, site)
    loss, r_, k_ = (rna2dna_loss if kind == "rna2dna" else dna2rna_loss)(rec, tgt, mu, lv, beta=BETA)
    opt.zero_grad()
    loss.backward()
    outs, losses = (rec, mu, lv), (loss.item(), r_, k_)
    tag = f"directional {kind} prec={prec} B={B}"
    if prec == "fp32":
        ref = oracle(c, None)
        line(tag + " vs fp64 reference arithmetic", compare_step(model, outs, losses, ref, TOL["fp32"], rename=c["ren"], out_names=OUTS))
    else:
        ref = oracle(c, O.BF16)
        line(tag + " vs bf16-aware oracle", compare_step(model, outs, losses, ref, tol_q(B), rename=c["ren"], out_names=OUTS))
        if B <= 4096:
            ref64 = oracle(c, None)
            dev = oracle_deviation(ref, ref64)
            line(tag + " vs fp64 reference arithmetic (bound: q-oracle's own deviation + tol_q)",
                 compare_step(model, outs, losses, ref64, tol_q(B), rename=c["ren"], out_names=OUTS, base=dev))
    if B == 1000:
        opt.step()
        share, dist = check_params_after_adamw(model, ref["P1"], LR, prec, c["ren"])
        report(f"{tag} parameters after AdamW vs O.adamw_step of the oracle's gradients: worst share off by > 1e-6 {share:.2e}, "
               f"worst distance {dist:.2e} (lr {LR})")


def _captured_form(c, x, tgt, site, ref, tag):
    B, kind = c["B"], c["kind"]
    model, opt = build(c, "bf16")
    rec, mu, lv = forward(model, c, x, site, fused_target=tgt)
    assert rec.stride(0) == 0, "the captured step's form must not materialise the reconstruction"
    total, out5 = F_.fused_loss({("b" if kind == "rna2dna" else "a"): (rec, tgt), "kl": (mu, lv)}, BETA, 1.0, unit_grad=True)
    opt.zero_grad()
    total.backward()
    vals = F_.read_losses(out5)
    assert vals[2] == 0.0                                # no class term
    line(tag, compare_step(model, (mu, lv), (vals[0], vals[1], vals[3]), ref, tol_q(B), rename=c["ren"], out_names=("mu", "logvar")))
    return model, opt


@pytest.mark.parametrize("B", [1000, 16384])
@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
def test_captured_form_vs_oracle(kind, B):
    """What GraphedTrainStep(kind=...) issues, eagerly: the single-term loss epilogue in the decoder's last GEMM (its loss sum
    and its gradient w.r.t. the pre-activation output) + KL, no class tail, unit gradient."""
    c = case(kind, B)
    ref = oracle(c, O.BF16)
    model, opt = _captured_form(c, t(c["x"]), t(c["tgt"]), t(c["site"]), ref,
                                f"directional {kind} prec=bf16 B={B} captured form (loss in the decoder GEMM) vs bf16-aware oracle")
    if B == 1000:
        opt.step()
        check_params_after_adamw(model, ref["P1"], LR, "bf16", c["ren"])


def test_captured_form_with_bf16_storage_vs_oracle():
    """Input and target in bf16 storage (padded bf16 rows: 782 -> 784 columns): the forward GEMM's A operand, the dW GEMM's Q
    operand and the loss epilogue's target are read as stored.  Both sides start from the same bf16-rounded values."""
    c = case("dna2rna", 1000)
    x, tgt = to_bf16_rows(t(O.bf16_round(c["x"]))), to_bf16_rows(t(O.bf16_round(c["tgt"])))
    assert x.dtype == torch.bfloat16 and tgt.stride(0) == 784
    _captured_form(c, x, tgt, t(c["site"]), oracle(c, O.BF16, rounded=True),
                   "directional dna2rna prec=bf16 B=1000 captured form, bf16-storage input and target, vs bf16-aware oracle")
