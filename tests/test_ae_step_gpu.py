"""RNA2DNAAE / DNA2RNAAE training steps against the float64 oracle (tests/ae_oracle.py) at the default widths
(782 / 572 / 24 / 20 / 32), mirroring tests/test_directional_gpu.py, with the project's own tolerances (TOL["fp32"], tol_q(B),
compare_step, check_params_after_adamw).

  fp32, B = 1000              against the fp64 oracle at TOL["fp32"]: reconstruction, latent, the loss, every gradient, running statistics
  bf16, B = 1000 and 4096     against the bf16-aware oracle (q = O.BF16) at tol_q(B); the deviation from the fp64 oracle is bounded per
                              tensor by the q-oracle's own deviation + tol_q(B); once with the fused latent launch and once with its
                              tuning key (15) off
  the captured step's form    bf16, B = 1000: g.fused_recon = [target], fused_loss on the single reconstruction term with unit_grad
                              (what GraphedTrainStep(kind="..._ae") issues): rec.stride(0) == 0; the loss floats and every gradient
  AdamW on top                parameters after opt.step() against O.adamw_step of the oracle's gradients
  noise                       the Philox offset after a training forward is np_noise.consumed(mask bytes, 0): masks only, no eps;
                              after an eval forward it has not moved
  the reference's state       tests/golden/ae_b32.npz loads through load_state_dict; the eval forwards (both inputs, site=None, site
                              only) match the recorded outputs at TOL["fp32"]["out"] in fp32
The oracle's names are mapped onto np_oracle's for compare_step (encoder_rna.0 -> encoder_a.fc.0, encoder_dna.4 -> encoder_b.fc.4): the
biases in front of a BatchNorm are then the analytically zero ones it already knows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ae_oracle as AO  # noqa: E402
import golden_util as G  # noqa: E402
import np_noise as N  # noqa: E402
import np_oracle as O  # noqa: E402
from model_util import scaled_err, check_params_after_adamw  # noqa: E402
from test_model_gpu import compare_step, oracle_deviation, TOL, tol_q, report, t  # noqa: E402
from mmvae import _lib, engine  # noqa: E402
from mmvae import functional as F_  # noqa: E402
from mmvae.optim import FusedAdamW  # noqa: E402
from src.models import RNA2DNAAE, DNA2RNAAE  # noqa: E402
from src.utils.ae_losses import rna2dna_ae_loss, dna2rna_ae_loss  # noqa: E402

DEV = "cuda"
A, D, S, L, E = 782, 572, 24, 20, 32
LR, WD = 5e-4, 1e-5
MODELS = {"rna2dna": RNA2DNAAE, "dna2rna": DNA2RNAAE}
# np_oracle's name of every top-level module of the model (compare_step's `rename`: oracle top -> model top)
REN = {"rna2dna": {"encoder_a.fc": "encoder_rna", "site_embedding": "site_embedding", "site_projection": "site_projection", "decoder_dna": "decoder_dna"},
       "dna2rna": {"encoder_b.fc": "encoder_dna", "site_embedding": "site_embedding", "site_projection": "site_projection", "decoder_rna": "decoder_rna"}}
OUTS = ("out", "latent")
_cases = {}


def oname(kind, key):
    top, rest = key.split(".", 1)
    return {v: k for k, v in REN[kind].items()}[top] + "." + rest


def load_ae(model, P, Bf):
    sd = {k: torch.from_numpy(np.array(v, dtype=np.int64 if k.endswith("num_batches_tracked") else np.float32)) for k, v in list(P.items()) + list(Bf.items())}
    model.load_state_dict(sd, strict=True)
    return model


def case(kind, B, dims=(A, D, S, L, E), settle=False):
    """settle: no kept ReLU gate of the encoder within fp32 rounding of zero (width_cases.settle_gates)."""
    key = (kind, B, tuple(dims), settle)
    if key not in _cases:
        seed = 700 + B
        A_, D_, S_, L_, E_ = dims
        P, Bf = AO.make_params(seed, kind, A_, D_, S_, L_, E_)
        a, b, site = O.make_batch(seed + 1, B, A_, D_, S_)
        rng = np.random.default_rng(seed + 2)
        masks = {n: (rng.random((B, w)) >= O.DROP_P).astype(np.uint8) for n, w in zip(AO.mask_names(kind), AO.HIDDEN[kind])}
        x, tgt = (a, b) if kind == "rna2dna" else (b, a)
        if settle:
            import width_cases as W
            masks, _ = W.settle_gates(masks, W.ae_gates(kind, P, Bf, x.astype(np.float64), site))
        _cases[key] = dict(kind=kind, B=B, dims=tuple(dims), P=P, Bf=Bf, x=x, tgt=tgt, site=site, masks=masks, ref={})
    return _cases[key]


def oracle(c, q):
    """One oracle step (forward, loss, backward, AdamW) -> the dict compare_step takes (np_oracle-style names) + P1, Bf1 (model names)."""
    key = "q" if q is not None else "f"
    if key not in c["ref"]:
        f, kind = np.float64, c["kind"]
        P1, Bf1 = {k: v.copy() for k, v in c["P"].items()}, dict(c["Bf"])
        st, step = O.adamw_init(P1)
        r = AO.train_step(kind, P1, Bf1, st, step, c["x"].astype(f), c["tgt"].astype(f), c["site"], c["masks"], LR, WD, q)
        c["ref"][key] = dict(out=r["out"], latent=r["latent"], losses=(r["total"],), G={oname(kind, k): v for k, v in r["grads"].items()}, Bf={},
                             P1={oname(kind, k): v for k, v in P1.items()}, Bf1=Bf1)
    return c["ref"][key]


def build(c, prec):
    A_, D_, S_, L_, E_ = c["dims"]
    model = load_ae(MODELS[c["kind"]](A_, D_, S_, L_, embed_dim=E_), c["P"], c["Bf"]).to(DEV).set_precision(prec).train()
    return model, FusedAdamW(model.parameters(), lr=LR, weight_decay=WD)


def forward(model, c, x, site, fused_target=None):
    engine.GLOBAL_NOISE.inject([torch.from_numpy(c["masks"][n]) for n in AO.mask_names(c["kind"])], None)
    g = model._graph()
    g.fused_recon = None if fused_target is None else [fused_target]
    try:
        return model(rna=x, site=site) if c["kind"] == "rna2dna" else model(dna=x, site=site)
    finally:
        g.fused_recon = None
        engine.GLOBAL_NOISE.clear()


def running_stats(model, ref, tol, base=None):
    """the BatchNorm buffers after the step against the oracle's, at the `out` tolerance"""
    sd, worst = model.state_dict(), 0.0
    for k, v in ref["Bf1"].items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v) == 1, k
            continue
        e = scaled_err(sd[k].cpu().numpy(), v)
        worst = max(worst, e)
        assert e <= tol["out"] + (base or 0.0), (k, e)
    return worst


def line(tag, e, bn):
    report(f"{tag}: out {e['out']:.3e}; loss rel {e['loss']:.3e}; grad max scaled {e['grad']:.3e} ({e['grad_worst']}); "
           f"grad max Frobenius-rel {e['fro']:.3e} ({e['fro_worst']}); running statistics {bn:.3e}")


def _fused_key(on):
    _lib.check(_lib.load().mmvae_set_tuning(15, int(on)), "mmvae_set_tuning")


@pytest.mark.parametrize("prec,B,fused", [("fp32", 1000, True), ("bf16", 1000, True), ("bf16", 1000, False), ("bf16", 4096, True), ("bf16", 4096, False)])
@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
def test_ae_step_vs_oracle(kind, prec, B, fused):
    """fused: the bf16 cases run once with the fused latent launch (mmvae_ae_latent_fwd, tuning key 15) and once with the key off, i.e.
    on the three launches it replaces; fp32 never takes it."""
    _fused_key(fused)
    try:
        _ae_step_vs_oracle(kind, prec, B, fused)
    finally:
        _fused_key(True)


def _ae_step_vs_oracle(kind, prec, B, fused):
    c = case(kind, B)
    model, opt = build(c, prec)
    x, tgt, site = t(c["x"]), t(c["tgt"]), t(c["site"])
    rec, latent = forward(model, c, x, site)
    loss, val = (rna2dna_ae_loss if kind == "rna2dna" else dna2rna_ae_loss)(rec, tgt)
    assert isinstance(val, float) and val == loss.item()
    opt.zero_grad()
    loss.backward()
    outs, losses = (rec, latent), (loss.item(),)
    tag = f"autoencoder {kind} prec={prec} B={B}" + ("" if prec == "fp32" else f" fused latent launch {'on' if fused else 'off'}")
    if prec == "fp32":
        ref = oracle(c, None)
        e = compare_step(model, outs, losses, ref, TOL["fp32"], rename=REN[kind], out_names=OUTS)
        line(tag + " vs fp64 reference arithmetic", e, running_stats(model, ref, TOL["fp32"]))
    else:
        ref = oracle(c, O.BF16)
        e = compare_step(model, outs, losses, ref, tol_q(B), rename=REN[kind], out_names=OUTS)
        line(tag + " vs bf16-aware oracle", e, running_stats(model, ref, tol_q(B)))
        ref64 = oracle(c, None)
        dev = oracle_deviation(ref, ref64)
        e = compare_step(model, outs, losses, ref64, tol_q(B), rename=REN[kind], out_names=OUTS, base=dev)
        bn_dev = max(scaled_err(ref["Bf1"][k], v) for k, v in ref64["Bf1"].items() if not k.endswith("num_batches_tracked"))
        line(tag + " vs fp64 reference arithmetic (bound: q-oracle's own deviation + tol_q)", e, running_stats(model, ref64, tol_q(B), bn_dev))
    if B == 1000:
        opt.step()
        share, dist = check_params_after_adamw(model, ref["P1"], LR, prec, REN[kind])
        report(f"{tag} parameters after AdamW vs O.adamw_step of the oracle's gradients: worst share off by > 1e-6 {share:.2e}, "
               f"worst distance {dist:.2e} (lr {LR})")


@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
def test_ae_captured_form_vs_oracle(kind):
    """What GraphedTrainStep(kind=kind + "_ae") issues, eagerly: the single-term loss epilogue in the decoder's last GEMM, unit gradient."""
    B = 1000
    c = case(kind, B)
    ref = oracle(c, O.BF16)
    model, opt = build(c, "bf16")
    tgt = t(c["tgt"])
    rec, latent = forward(model, c, t(c["x"]), t(c["site"]), fused_target=tgt)
    assert rec.stride(0) == 0, "the captured step's form must not materialise the reconstruction"
    total, out5 = F_.fused_loss({("b" if kind == "rna2dna" else "a"): (rec, tgt)}, 0.0, 1.0, unit_grad=True)
    opt.zero_grad()
    total.backward()
    vals = F_.read_losses(out5)
    assert vals[2] == 0.0 and vals[3] == 0.0 and vals[0] == vals[1]                 # no class term, no KL term
    e = compare_step(model, (latent,), (vals[0],), ref, tol_q(B), rename=REN[kind], out_names=("latent",))
    line(f"autoencoder {kind} prec=bf16 B={B} captured form (loss in the decoder GEMM) vs bf16-aware oracle", e, running_stats(model, ref, tol_q(B)))
    opt.step()
    check_params_after_adamw(model, ref["P1"], LR, "bf16", REN[kind])


@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
def test_ae_noise_is_masks_only(kind):
    B = 1000
    c = case(kind, B)
    dev = torch.device(DEV, torch.cuda.current_device())
    model, _ = build(c, "bf16")
    x, site = t(c["x"]), t(c["site"])
    kw = "rna" if kind == "rna2dna" else "dna"
    engine.GLOBAL_NOISE.offset_tensor(dev).zero_()
    model(**{kw: x, "site": site})
    want = N.consumed(N.mask_segments(B, AO.HIDDEN[kind])[1], 0)
    assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == want
    model.eval()
    with torch.no_grad():
        model(**{kw: x, "site": site})
        model(**{kw: x})
        model(site=site)
    assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == want, "an eval-mode forward drew noise"
    model.train()
    model(site=site)                                     # no encoder, no masks: nothing is drawn in training mode either
    assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == want
    assert model() == (None, None)


@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
def test_ae_reference_state_loads_and_eval_matches(kind):
    fx = G.load("ae_b32")
    k = kind + "."
    Af, Df, Sf, Lf, Ef = (int(v) for v in fx["dims"])
    model = MODELS[kind](Af, Df, Sf, Lf, embed_dim=Ef)
    sd = model.state_dict()
    assert list(sd) == [str(n) for n in fx[k + "names"]]
    assert [",".join(str(n) for n in v.shape) for v in sd.values()] == [str(s) for s in fx[k + "shapes"]]
    P, Bf = AO.decode({n[len(k) + 5:]: fx[n] for n in fx.files if n.startswith(k + "code.")},
                      {n[len(k) + 6:]: fx[n] for n in fx.files if n.startswith(k + "scale.")})
    load_ae(model, P, Bf).to(DEV).set_precision("fp32").eval()
    x, site = t(fx[k + ("rna" if kind == "rna2dna" else "dna")].astype(np.float32)), t(fx[k + "site"])
    kw = "rna" if kind == "rna2dna" else "dna"
    with torch.no_grad():
        for tag, args in (("both", {kw: x, "site": site}), ("nosite", {kw: x}), ("siteonly", {"site": site})):
            rec, latent = model(**args)
            for nm, got in (("out", rec), ("latent", latent)):
                want = fx[k + f"eval.{tag}.{nm}"]
                err = scaled_err(got.cpu().numpy(), want)
                report(f"autoencoder {kind} fixture eval.{tag}.{nm} fp32: {err:.3e}")
                assert tuple(got.shape) == want.shape and err <= TOL["fp32"]["out"], (tag, nm, err)
