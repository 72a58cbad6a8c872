"""Whole training steps against the numpy oracle across the model's width space: the rows of tests/width_cases.py (odd input
widths, odd and large latents, 5 to 33 sites, embed 8 to 64), B = 1000, with the tolerances the default widths are held to
(test_model_gpu: TOL["fp32"], tol_q(B), oracle_deviation; model_util.check_params_after_adamw).  The oracle itself is pinned at
these widths on the CPU (tests/test_width_oracle_cpu.py).

  a  MultiModalVAE, every row, both precisions: injected noise, vae_loss with class weights; all five outputs, the four loss floats,
     all 39 gradients, the BatchNorm buffers; one FusedAdamW step; eval-mode forwards with and without the site.  fp32 against the
     fp64 oracle, bf16 against the bf16-aware oracle and (bounded by that oracle's own deviation + tol_q) against the fp64 one.
     bf16 once more in the form the captured step issues (losses in the decoder GEMMs, the class head left to the loss, the tail
     riders), which is where the fused class head is taken or refused.
  b  RNA2DNAVAE / DNA2RNAVAE / RNA2DNAAE / DNA2RNAAE on three rows, both precisions (tests/test_directional_gpu.py's and
     tests/test_ae_step_gpu.py's cases, bounds and AdamW check at these widths).
  c  GraphedTrainStep, two replays with the oracle following the device's Philox stream (tests/test_graphed_oracle_gpu.py).
  d  input subsets (tests/partial_cases.py) with an odd latent; both inputs in bf16 storage at 1177 / 1211 (rows of 1184 / 1216).
  e  `big_batch`: B = 16384, odd widths, bf16.
Every case also asserts WHICH launches it issued -- the tags of an ops.KernelProbe installed for the step -- against what its row
says: a row that silently takes another path fails.  That covers the launches that have a tag of their own: the fused latent
launch, the fused class head, the grouped dW flush and its riders, the merged stem and the per-decoder layer-0 launches, the input
conversion.  It does NOT cover which GEMM kernel form a tagged launch ran (one-float operand loads, persistent or multi-split tiles,
the wide-tile dW form that `big_batch` must stay out of): the library has neither a planner nor a tag for those, so for them the
tests assert only the operand facts the dispatch keys on (row pitches, widths, batch) and the numbers.
The measured errors go to the parity report (test_model_gpu.report).

Two things about the inputs and bounds, both stated in tests/width_cases.py and measured in DESIGN.md section 2:
  * the injected keep-masks drop the few units whose ReLU gate the fp64 oracle has within 1e-5 of zero (settle_gates): one such gate
    decided the other way by an fp32 sum is 1 / sqrt(B) of a dW row, twice TOL["fp32"] at B = 1000, and no error of either side.
    No case therefore exercises a gate at zero, and the replayed graphs, whose noise the device draws, cannot be conditioned;
  * six bf16 gradient tensors in five cases exceed tol_q(B) against the bf16-aware oracle in one norm, by 3 .. 8 % (Frobenius 1.03e-2 ..
    1.08e-2 against 1e-2) and, at B = 16384, in the max norm (4.9e-2 against 3.1e-2), identically with every fused form and newer
    GEMM generation switched off and not at B = 4096.  STORAGE_BOUND names each tensor and norm; only that entry is taken out of the
    comparison with the bf16-aware oracle and held by the fp64 comparison (the bf16-aware oracle's own deviation + tol_q(B))
    instead.  Every other tensor and norm of those cases stays at tol_q(B)."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ae_oracle as AO  # noqa: E402
import np_noise as N  # noqa: E402
import np_oracle as O  # noqa: E402
import test_ae_step_gpu as AE  # noqa: E402
import test_bf16_inputs_gpu as S16  # noqa: E402
import test_directional_gpu as DIR  # noqa: E402
import width_cases as W  # noqa: E402
from model_util import load_state, masks_list, scaled_err, f64, check_params_after_adamw  # noqa: E402
from partial_cases import CASES, mask_names, oracle_partial_step  # noqa: E402
from test_graphed_oracle_gpu import TRAJ, _adam_steps, _loss_dev  # noqa: E402
from test_model_gpu import oracle_step, compare_step, oracle_deviation, tol_q, TOL, TOL_Q, OUT_NAMES, report, t  # noqa: E402
from mmvae import engine, ops, to_bf16_rows  # noqa: E402
from mmvae import functional as F_  # noqa: E402
from mmvae.graphs import GraphedTrainStep  # noqa: E402
from mmvae.optim import FusedAdamW  # noqa: E402
from src.models import MultiModalVAE, RNA2DNAVAE  # noqa: E402
from src.utils import vae_loss  # noqa: E402
from src.utils.ae_losses import rna2dna_ae_loss, dna2rna_ae_loss  # noqa: E402
from src.utils.directional_losses import rna2dna_loss, dna2rna_loss  # noqa: E402

DEV = "cuda"
BETA, GAMMA, LR, WD = 1e-3, 1.0, 5e-4, 1e-5
MM_ROWS = [r.id for r in W.ROWS if r.B == 1000]
UNFUSED_LATENT = {"EncoderA.heads.fwd", "EncoderB.heads.fwd", "fuse_reparam_fwd", "Decoders.L0.fwd"}
UNFUSED_CLASS = {"DecoderC.L1.fwd", "vae_loss", "DecoderC.L1.dX"}
_cases = {}


@contextlib.contextmanager
def probed():
    """An ops.KernelProbe for the launches issued inside -> {tag: [meta of every launch]} (filled on exit)."""
    out = {}
    ops.PROBE = ops.KernelProbe()
    try:
        yield out
        torch.cuda.synchronize()
        out.update({k: [m for _, _, m in v] for k, v in ops.PROBE.records.items()})
    finally:
        ops.PROBE = None


def mm_case(rid):
    """Seeded parameters, batch, noise and class weights of one row, built once and left unchanged; oracle results are kept with them."""
    if rid not in _cases:
        row = W.BY_ID[rid]
        A, D, S, L, E = row.dims
        seed = 2000 + 10 * [r.id for r in W.ROWS].index(rid)
        P, Bf = O.make_params(seed, A, D, S, L, E)
        a, b, site = O.make_batch(seed + 1, row.B, A, D, S)
        masks, eps = O.make_noise(seed + 2, row.B, L)
        cw = np.random.default_rng(seed + 3).uniform(0.5, 2.0, S).astype(np.float32)
        P64, Bf64 = f64(P), f64(Bf)
        f = np.float64
        masks, dropped = W.settle_gates(masks, W.mm_gates(P64, Bf64, a.astype(f), b.astype(f), site, eps.astype(f)))
        report(f"width_space {rid}: {dropped} kept unit(s) with a gate within {W.GATE_MARGIN:.0e} of zero dropped from the keep-masks")
        _cases[rid] = dict(row=row, P=P, Bf=Bf, P64=P64, Bf64=Bf64, a=a, b=b, site=site, masks=masks, eps=eps, cw=cw, ref={})
    return _cases[rid]


def q_exempt(kind, rid, ref):
    """compare_step's base= for the comparison with the bf16-aware oracle `ref`: None, or -- for a case in width_cases.STORAGE_BOUND --
    allowances that are zero for every tensor and norm except the (tensor, norm) pairs named there, which are unbounded in THIS
    comparison (the fp64 comparison holds them).  -> (base, a note for the report line)."""
    pairs = W.STORAGE_BOUND.get((kind, rid))
    if not pairs:
        return None, ""
    base = oracle_deviation(ref, ref)                    # the right keys, all zero
    assert all(v == 0.0 for part in base.values() for v in part.values())
    for tensor, norm in pairs:
        part = base[{"fro": "gfro", "grad": "gerr"}[norm]]
        assert tensor in part, tensor
        part[tensor] = float("inf")
    return base, " (storage-bound, held by the fp64 comparison: " + ", ".join(f"{t_} {n}" for t_, n in pairs) + ")"


def mm_oracle(c, q):
    """oracle_step's dict + P1 (the parameters after O.adamw_step of its gradients) + the eval-mode forwards on its buffers."""
    key = "q" if q is not None else "f"
    if key not in c["ref"]:
        r = oracle_step(c["P64"], c["Bf64"], c["a"], c["b"], c["site"], c["masks"], c["eps"], BETA, GAMMA, c["cw"], q)
        P1 = {k: v.copy() for k, v in c["P64"].items()}
        st, step = O.adamw_init(P1)
        O.adamw_step(P1, r["G"], st, step, LR, WD)
        f = np.float64
        ev = {tag: O.vae_forward(c["P64"], dict(r["Bf"]), c["a"].astype(f), c["b"].astype(f), s, None, c["eps"].astype(f), False, q=q)[:5]
              for tag, s in (("site", c["site"]), ("nosite", None))}
        c["ref"][key] = dict(r, P1=P1, eval=ev)
    return c["ref"][key]


def mm_build(c, prec):
    A, D, S, L, E = c["row"].dims
    model = load_state(MultiModalVAE(A, D, S, L, embed_dim=E), c["P"], c["Bf"]).to(DEV).set_precision(prec).train()
    return model, FusedAdamW(model.parameters(), lr=LR, weight_decay=WD)


def line(tag, e):
    report(f"width_space {tag}: out {e['out']:.3e}; loss rel {e['loss']:.3e}; grad max scaled {e['grad']:.3e} ({e['grad_worst']}); "
           f"grad max Frobenius-rel {e['fro']:.3e} ({e['fro_worst']}); running statistics {e['bn']:.3e}")


def check_tn_group(tags, prec, dims, riders):
    """The grouped dW launch that ends the backward: grouped or one launch per problem, with or without its riders, as
    width_cases.tn_group_expect derives it from the library's conditions (None: not stated for these widths)."""
    A, D, S, L, E = dims
    meta = tags["tiny_dW.heads"][0]
    want = W.tn_group_expect(prec, S, L)
    if want is not None:
        assert meta["grouped"] == want, (meta, prec, dims)
    if riders:
        fits = W.embed_bwd_lds(S, L, E) <= W.EMBED_RIDER_LDS
        assert meta["riders"] == (meta["grouped"] and fits), (meta, dims)
    else:
        assert not meta["riders"]
    return meta


def mm_step(rid, prec):
    c = mm_case(rid)
    row = c["row"]
    A, D, S, L, E = row.dims
    B = row.B
    model, opt = mm_build(c, prec)
    a, b, site, cw = t(c["a"]), t(c["b"]), t(c["site"]), t(c["cw"])
    assert a.stride(0) == A and b.stride(0) == D                       # fp32 rows as they are: one-float rows at the odd widths
    with probed() as tags:
        engine.GLOBAL_NOISE.inject(masks_list(c["masks"]), torch.from_numpy(c["eps"]))
        try:
            ra, rb, rc, mu, lv = model(a=a, b=b, site=site)
        finally:
            engine.GLOBAL_NOISE.clear()
        loss, r_, c_, k_ = vae_loss(ra, a, rb, b, rc, site, mu, lv, beta=BETA, gamma=GAMMA, class_weights=cw)
        opt.zero_grad()
        loss.backward()
    # the forms this row says it takes
    fused = prec == "bf16" and row.latent_fused
    assert ("latent.fwd" in tags) == fused, sorted(tags)
    assert fused or UNFUSED_LATENT <= set(tags), sorted(tags)
    assert not fused or not (UNFUSED_LATENT & set(tags)), sorted(tags)
    assert "class_tail" not in tags and {"DecoderC.L1.fwd", "vae_loss"} <= set(tags)      # the class head is fused in the captured form only
    meta = check_tn_group(tags, prec, row.dims, riders=False)
    outs, losses = (ra, rb, rc, mu, lv), (loss.item(), r_, c_, k_)
    tag = f"{rid} {row.dims} B={B} prec={prec} (latent {'fused' if fused else 'unfused'}, heads dW {'grouped' if meta['grouped'] else 'ungrouped'})"
    ref64 = mm_oracle(c, None)
    if prec == "fp32":
        ref = ref64
        line(tag + " vs fp64 reference arithmetic", compare_step(model, outs, losses, ref, TOL["fp32"]))
    else:
        ref = mm_oracle(c, O.BF16)
        exempt, note = q_exempt("multimodal", rid, ref)
        line(tag + " vs bf16-aware oracle" + note, compare_step(model, outs, losses, ref, tol_q(B), base=exempt))
        line(tag + " vs fp64 reference arithmetic (bound: q-oracle's own deviation + tol_q)",
             compare_step(model, outs, losses, ref64, tol_q(B), base=oracle_deviation(ref, ref64)))
    opt.step()
    share, dist = check_params_after_adamw(model, ref["P1"], LR, prec)
    report(f"width_space {tag} parameters after AdamW: worst share off by > 1e-6 {share:.2e}, worst distance {dist:.2e} (lr {LR})")
    # eval mode, with and without the site, from the step's start parameters and the oracle's buffers after it
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in c["P"].items():
            sd[k].copy_(t(v))
        for k, v in ref["Bf"].items():
            if k.endswith("running_mean") or k.endswith("running_var"):
                sd[k].copy_(t(np.asarray(v, np.float32)))
        model.eval()
        worst = 0.0
        for etag, s in (("site", site), ("nosite", None)):
            engine.GLOBAL_NOISE.inject([], torch.from_numpy(c["eps"]))
            try:
                got = model(a=a, b=b, site=s)
            finally:
                engine.GLOBAL_NOISE.clear()
            for nm, g_, w_ in zip(OUT_NAMES, got, ref["eval"][etag]):
                err = scaled_err(g_.cpu().numpy(), w_)
                worst = max(worst, err)
                assert tuple(g_.shape) == w_.shape and err <= (TOL["fp32"]["out"] if prec == "fp32" else TOL_Q["out"]), (etag, nm, err)
    report(f"width_space {tag} eval-mode forwards (site, site=None): worst output {worst:.3e}")


# ----------------------------------------------------------------------------------------------------------------------------------
# a. MultiModalVAE on every row
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("rid", MM_ROWS)
def test_multimodal_step_vs_oracle(rid, prec):
    mm_step(rid, prec)


def captured_form(rid):
    """What GraphedTrainStep issues, eagerly and with injected noise (a capture cannot take it): the reconstruction losses inside the
    decoders' last GEMMs, the class head left to the loss, the loss finalisation and EncoderC's backward as riders of the last
    grouped dW launch.  mu, logvar, the loss floats and every gradient against the bf16-aware oracle at tol_q(B)."""
    c = mm_case(rid)
    row = c["row"]
    A, D, S, L, E = row.dims
    model, opt = mm_build(c, "bf16")
    a, b, site, cw = t(c["a"]), t(c["b"]), t(c["site"]), t(c["cw"])
    g = model._graph()
    with probed() as tags:
        engine.GLOBAL_NOISE.inject(masks_list(c["masks"]), torch.from_numpy(c["eps"]))
        g.fused_recon, g.defer_class_head, g.tail_riders = [a, b, None], True, True
        try:
            ra, rb, rc, mu, lv = model(a=a, b=b, site=site)
        finally:
            g.fused_recon, g.defer_class_head, g.tail_riders = None, False, False
            engine.GLOBAL_NOISE.clear()
        total, out5 = F_.fused_loss({"a": (ra, a), "b": (rb, b), "c": (rc, site), "kl": (mu, lv)}, BETA, GAMMA, cw, unit_grad=True)
        opt.zero_grad()
        total.backward()
    vals = F_.read_losses(out5)
    assert ra.stride(0) == 0 and rb.stride(0) == 0, "the captured step's form must not materialise the reconstructions"
    n_stem = O.DEC_A_H + O.DEC_B_H1 + O.DEC_C_H                        # the merged first layers: H0's and D0's row pitch
    assert row.class_tail == ops.class_tail_fits(ops.PREC_BF16, S, O.DEC_C_H, L, n_stem, n_stem)      # the library's own answer
    assert ("class_tail" in tags) == row.class_tail, sorted(tags)
    assert row.class_tail or UNFUSED_CLASS <= set(tags), sorted(tags)
    assert not row.class_tail or not (UNFUSED_CLASS & set(tags)), sorted(tags)
    assert ("latent.fwd" in tags) == row.latent_fused, sorted(tags)
    meta = check_tn_group(tags, "bf16", row.dims, riders=True)
    tag = (f"{rid} {row.dims} B={row.B} prec=bf16 captured form (class head {'fused' if row.class_tail else 'unfused'}, riders "
           f"{'rode' if meta['riders'] else 'stand-alone'}) vs bf16-aware oracle")
    ref = mm_oracle(c, O.BF16)
    exempt, note = q_exempt("multimodal", rid, ref)
    line(tag + note, compare_step(model, (mu, lv), tuple(vals), ref, tol_q(row.B), out_names=("mu", "logvar"), base=exempt))
    if exempt is not None:
        ref64 = mm_oracle(c, None)
        compare_step(model, (mu, lv), tuple(vals), ref64, tol_q(row.B), out_names=("mu", "logvar"), base=oracle_deviation(ref, ref64))
    opt.step()
    check_params_after_adamw(model, ref["P1"], LR, "bf16")


@pytest.mark.parametrize("rid", MM_ROWS)
def test_multimodal_captured_form_vs_oracle(rid):
    captured_form(rid)


# ----------------------------------------------------------------------------------------------------------------------------------
# b. the directional models
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
@pytest.mark.parametrize("rid", W.DIRECTIONAL_ROWS)
def test_directional_vae_step_vs_oracle(rid, kind, prec):
    """tests/test_directional_gpu.py::test_directional_step_vs_oracle at the row's widths, B = 1000."""
    row = W.BY_ID[rid]
    B = row.B
    c = DIR.case(kind, B, row.dims, settle=True)
    model, opt = DIR.build(c, prec)
    x, tgt, site = t(c["x"]), t(c["tgt"]), t(c["site"])
    with probed() as tags:
        rec, mu, lv = DIR.forward(model, c, x, site)
        loss, r_, k_ = (rna2dna_loss if kind == "rna2dna" else dna2rna_loss)(rec, tgt, mu, lv, beta=DIR.BETA)
        opt.zero_grad()
        loss.backward()
    assert "latent.fwd" not in tags and "fuse_reparam_fwd" in tags, sorted(tags)       # one decoder: no merged stem, no fused latent stage
    outs, losses = (rec, mu, lv), (loss.item(), r_, k_)
    tag = f"{rid} {row.dims} directional {kind} prec={prec} B={B}"
    if prec == "fp32":
        ref = DIR.oracle(c, None)
        line(tag + " vs fp64 reference arithmetic", compare_step(model, outs, losses, ref, TOL["fp32"], rename=c["ren"], out_names=DIR.OUTS))
    else:
        ref, ref64 = DIR.oracle(c, O.BF16), DIR.oracle(c, None)
        line(tag + " vs bf16-aware oracle", compare_step(model, outs, losses, ref, tol_q(B), rename=c["ren"], out_names=DIR.OUTS))
        line(tag + " vs fp64 reference arithmetic (bound: q-oracle's own deviation + tol_q)",
             compare_step(model, outs, losses, ref64, tol_q(B), rename=c["ren"], out_names=DIR.OUTS, base=oracle_deviation(ref, ref64)))
    opt.step()
    check_params_after_adamw(model, ref["P1"], DIR.LR, prec, c["ren"])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
@pytest.mark.parametrize("rid", W.DIRECTIONAL_ROWS)
def test_autoencoder_step_vs_oracle(rid, kind, prec):
    """tests/test_ae_step_gpu.py::test_ae_step_vs_oracle at the row's widths, B = 1000; the fused latent launch where the row fits it."""
    row = W.BY_ID[rid]
    A, D, S, L, E = row.dims
    B = row.B
    c = AE.case(kind, B, row.dims, settle=True)
    model, opt = AE.build(c, prec)
    x, tgt, site = t(c["x"]), t(c["tgt"]), t(c["site"])
    with probed() as tags:
        rec, latent = AE.forward(model, c, x, site)
        loss, val = (rna2dna_ae_loss if kind == "rna2dna" else dna2rna_ae_loss)(rec, tgt)
        opt.zero_grad()
        loss.backward()
    fused = prec == "bf16" and W.latent_fits(S, L, heads=1)
    assert ("ae_latent.fwd" in tags) == fused and ("fuse_mean_fwd" in tags) == (not fused), sorted(tags)
    outs, losses = (rec, latent), (loss.item(),)
    ren = AE.REN[kind]
    tag = f"{rid} {row.dims} autoencoder {kind} prec={prec} B={B} (latent {'fused' if fused else 'unfused'})"
    if prec == "fp32":
        ref = AE.oracle(c, None)
        e = compare_step(model, outs, losses, ref, TOL["fp32"], rename=ren, out_names=AE.OUTS)
        AE.line("width_space " + tag + " vs fp64 reference arithmetic", e, AE.running_stats(model, ref, TOL["fp32"]))
    else:
        ref, ref64 = AE.oracle(c, O.BF16), AE.oracle(c, None)
        exempt, note = q_exempt(kind + "_ae", rid, ref)
        e = compare_step(model, outs, losses, ref, tol_q(B), rename=ren, out_names=AE.OUTS, base=exempt)
        AE.line("width_space " + tag + " vs bf16-aware oracle" + note, e,
                AE.running_stats(model, ref, tol_q(B)))
        e = compare_step(model, outs, losses, ref64, tol_q(B), rename=ren, out_names=AE.OUTS, base=oracle_deviation(ref, ref64))
        bn_dev = max(scaled_err(ref["Bf1"][k], v) for k, v in ref64["Bf1"].items() if not k.endswith("num_batches_tracked"))
        AE.line("width_space " + tag + " vs fp64 reference arithmetic (bound: q-oracle's own deviation + tol_q)", e,
                AE.running_stats(model, ref64, tol_q(B), bn_dev))
    opt.step()
    check_params_after_adamw(model, ref["P1"], AE.LR, prec, ren)


# ----------------------------------------------------------------------------------------------------------------------------------
# c. the captured and replayed step
# ----------------------------------------------------------------------------------------------------------------------------------
G_LR = 5e-3                                              # tests/test_graphed_oracle_gpu.py: the parameters really move
G_MASKS = {"multimodal": ("encoder_a.fc.3", "encoder_b.fc.3", "encoder_b.fc.7"), "rna2dna": ("encoder_a.fc.3",)}
G_WIDTHS = {"encoder_a.fc.3": O.HID_A, "encoder_b.fc.3": O.HID_B1, "encoder_b.fc.7": O.HID_B2}


@pytest.mark.parametrize("rid,kind,prec", [("odd_latent", "multimodal", "fp32"), ("odd_latent", "multimodal", "bf16"),
                                           ("past_latent", "multimodal", "bf16"), ("corner", "rna2dna", "bf16")])
def test_replayed_graph_vs_oracle(rid, kind, prec):
    """Two replays; the oracle draws the device's noise from the seed and the running offset (np_noise.noise_source_draw).  Per replay
    the loss floats; after the first the parameters after the replayed AdamW and the running statistics; the Philox offset and Adam's
    step count after each."""
    row = W.BY_ID[rid]
    A, D, S, L, E = row.dims
    B = row.B
    seed = 3000 + 10 * W.ROWS.index(row) + (prec == "bf16")
    torch.manual_seed(seed)
    dev = torch.device(DEV, torch.cuda.current_device())
    P, Bf = O.make_params(seed, A, D, S, L, E)
    ren = None if kind == "multimodal" else O.directional_param_names(kind, A, D, S, L, E)
    cls = MultiModalVAE if kind == "multimodal" else RNA2DNAVAE
    model = load_state(cls(A, D, S, L, embed_dim=E), P, Bf, ren).to(DEV).set_precision(prec).train()
    engine.GLOBAL_NOISE.offset_tensor(dev).zero_()
    opt = FusedAdamW(model.parameters(), lr=G_LR, weight_decay=WD)
    a, b, site = O.make_batch(seed + 1, B, A, D, S)
    gs = GraphedTrainStep(model, opt, t(a), t(b), t(site), beta=BETA, gamma=GAMMA, kind=kind, warmup=1, preserve_state=True)
    assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == 0 and _adam_steps(opt, model)[0] <= {0}      # the warm-up step was undone
    q = None if prec == "fp32" else O.BF16
    hP, hBf = f64(P), f64(Bf)
    state, step, offset, pseed = *O.adamw_init(hP), 0, torch.initial_seed() & (2 ** 64 - 1)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    names = G_MASKS[kind]
    tag = f"width_space {rid} {row.dims} replayed graph kind={kind} prec={prec} B={B}"
    devs = []
    for s in range(2):
        masks, eps, offset = N.noise_source_draw(pseed, offset, B, [G_WIDTHS[n] for n in names], L)
        masks, eps = dict(zip(names, masks)), eps.astype(np.float64)
        if kind == "multimodal":
            r = O.train_step(hP, hBf, state, step, a64, b64, site, masks, eps, BETA, GAMMA, None, G_LR, WD, q=q)
            want = (r["total"], r["recon"], r["cls"], r["kld"])
        else:
            r = O.directional_train_step(kind, hP, hBf, state, step, a64, b64, site, masks, eps, BETA, G_LR, WD, q=q)
            want = (r["total"], r["recon"], None, r["kld"])
        step = r["step"]
        gs()
        ldev = _loss_dev(gs.losses(), want)
        devs.append(max(ldev))
        assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == offset
        assert (engine.GLOBAL_NOISE.offset_tensor(dev) == offset).all()
        assert _adam_steps(opt, model) == ({s + 1}, {s + 1})
        if s == 0:
            assert devs[0] <= (TOL["fp32"]["loss"] if prec == "fp32" else TOL_Q["loss"]), (gs.losses(), want)
            inv = {v: k for k, v in ren.items()} if ren else None
            bn = {}
            for k, v in model.state_dict().items():
                top, rest = k.split(".", 1)
                ko = k if inv is None else inv[top] + "." + rest
                if k.endswith("num_batches_tracked"):
                    assert int(v) == 1 == int(hBf[ko]), k
                elif k.endswith("running_mean") or k.endswith("running_var"):
                    bn[ko] = scaled_err(v.cpu().numpy(), hBf[ko])
            assert max(bn.values()) <= (TOL["fp32"]["out"] if prec == "fp32" else TOL_Q["out"]), bn
            share, dist = check_params_after_adamw(model, hP, G_LR, prec, ren)
            report(f"{tag} step 0: loss floats rel {devs[0]:.3e}; running statistics {max(bn.values()):.3e}; parameters after the replayed "
                   f"AdamW step: worst share off by > 1e-6 {share:.2e}, worst distance {dist:.2e} (lr {G_LR})")
    report(f"{tag} loss floats vs same-q oracle, replays 0..1: " + ", ".join(f"{d:.3e}" for d in devs) + f" (bound {TRAJ[prec]:.0e})")
    assert max(devs) <= TRAJ[prec], devs


def test_replayed_ae_graph_vs_oracle():
    """GraphedTrainStep(kind="rna2dna_ae") at the corner's widths, as tests/test_ae_graphed_gpu.py at the default ones."""
    rid, kind = "corner", "rna2dna"
    row = W.BY_ID[rid]
    A, D, S, L, E = row.dims
    B = row.B
    seed = 3900
    torch.manual_seed(seed)
    dev = torch.device(DEV, torch.cuda.current_device())
    P, Bf = AO.make_params(seed, kind, A, D, S, L, E)
    model = AE.load_ae(AE.MODELS[kind](A, D, S, L, embed_dim=E), P, Bf).to(DEV).set_precision("bf16").train()
    engine.GLOBAL_NOISE.offset_tensor(dev).zero_()
    opt = FusedAdamW(model.parameters(), lr=G_LR, weight_decay=WD)
    a, b, site = O.make_batch(seed + 1, B, A, D, S)
    gs = GraphedTrainStep(model, opt, t(a), t(b), t(site), kind=kind + "_ae", warmup=1, preserve_state=True)
    assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == 0 and _adam_steps(opt, model)[0] <= {0}
    hP, hBf = {k: v.copy() for k, v in P.items()}, dict(Bf)
    state, step, offset, pseed = *O.adamw_init(hP), 0, torch.initial_seed() & (2 ** 64 - 1)
    x, tgt = a.astype(np.float64), b.astype(np.float64)
    devs = []
    for s in range(2):
        masks, eps, offset = N.noise_source_draw(pseed, offset, B, AO.HIDDEN[kind], None)
        assert eps is None
        r = AO.train_step(kind, hP, hBf, state, step, x, tgt, site, dict(zip(AO.mask_names(kind), masks)), G_LR, WD, q=O.BF16)
        step = r["step"]
        gs()
        total, recon, cls, kld = gs.losses()
        assert cls == 0.0 and kld == 0.0 and total == recon
        devs.append(abs(total - r["total"]) / abs(r["total"]))
        assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == offset
        assert _adam_steps(opt, model) == ({s + 1}, {s + 1})
        if s == 0:
            assert devs[0] <= TOL_Q["loss"], (total, r["total"])
            sd = model.state_dict()
            bn = {k: scaled_err(sd[k].cpu().numpy(), v) for k, v in hBf.items() if not k.endswith("num_batches_tracked")}
            assert max(bn.values()) <= TOL_Q["out"], bn
            check_params_after_adamw(model, {AE.oname(kind, k): v for k, v in hP.items()}, G_LR, "bf16", AE.REN[kind])
    report(f"width_space {rid} {row.dims} replayed graph kind={kind}_ae prec=bf16 B={B} loss vs bf16-aware oracle, replays 0..1: "
           + ", ".join(f"{d:.3e}" for d in devs) + f" (bound {TRAJ['bf16']:.0e})")
    assert max(devs) <= TRAJ["bf16"], devs


# ----------------------------------------------------------------------------------------------------------------------------------
# d. subsets of the inputs, bf16 storage
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["a", "b_site"])
def test_partial_step_with_an_odd_latent(case, prec):
    """tests/test_partial_modalities_gpu.py's fused-loss form on `past_latent` (L = 25): inputs `a` alone (the backward goes without
    the merged stem: dz of 100-byte rows summed in the fusion backward) and `b, site`."""
    c = mm_case("past_latent")
    row = c["row"]
    B = row.B
    inputs, terms = CASES[case]["inputs"], CASES[case]["terms"]
    model, _ = mm_build(c, prec)
    a, b, site, cw = t(c["a"]), t(c["b"]), t(c["site"]), t(c["cw"])
    with probed() as tags:
        engine.GLOBAL_NOISE.inject(masks_list(c["masks"], mask_names(case)), torch.from_numpy(c["eps"]))
        try:
            ra, rb, rc, mu, lv = model(a=a if "a" in inputs else None, b=b if "b" in inputs else None, site=site if "site" in inputs else None)
        finally:
            engine.GLOBAL_NOISE.clear()
        if len(terms) == 4:
            loss, rec_, cls_, kld_ = vae_loss(ra, a, rb, b, rc, site, mu, lv, beta=BETA, gamma=GAMMA, class_weights=cw)
            losses = (loss.item(), rec_, cls_, kld_)
        else:
            full = {"a": (ra, a), "b": (rb, b), "c": (rc, site), "kl": (mu, lv)}
            loss, out5 = F_.fused_loss({k: full[k] for k in terms}, BETA, GAMMA, cw)
            losses = tuple(F_.read_losses(out5))
        loss.backward()
    # L = 25: no fused latent launch in either precision; only the encoder that was fed runs its heads; the merged stem ran in the
    # forward, and the backward goes through it only where every decoder has a gradient (`a`: decoder_c has none -> per-decoder dX)
    ran, idle = ("EncoderA", "EncoderB") if case == "a" else ("EncoderB", "EncoderA")
    assert "latent.fwd" not in tags and {"fuse_reparam_fwd", "Decoders.L0.fwd", ran + ".heads.fwd"} <= set(tags), sorted(tags)
    assert not any(k.startswith(idle + ".") for k in tags), sorted(tags)
    own_dx = {"DecoderA.L0.dX", "DecoderB.L0.dX"}
    if case == "a":
        assert own_dx <= set(tags) and "Decoders.L0.dX" not in tags and "DecoderC.L1.dX" not in tags, sorted(tags)
    else:
        assert "Decoders.L0.dX" in tags and not (own_dx & set(tags)), sorted(tags)
    assert tags["tiny_dW.heads"][0]["grouped"] is False and not tags["tiny_dW.heads"][0]["riders"]      # odd latent, no tail riders asked for
    outs = (ra, rb, rc, mu, lv)

    def oracle(q):
        key = (case, "q" if q is not None else "f")
        if key not in c["ref"]:
            c["ref"][key] = oracle_partial_step(c["P64"], c["Bf64"], c["a"], c["b"], c["site"], c["masks"], c["eps"], case, BETA, GAMMA, c["cw"], q)
        return c["ref"][key]
    ref64 = oracle(None)
    for got, want in zip(losses, ref64["losses"]):
        assert want is not None or got == 0.0, (losses, ref64["losses"])
    tag = f"past_latent {row.dims} partial inputs={'+'.join(inputs)} terms={'+'.join(terms)} prec={prec} B={B}"
    if prec == "fp32":
        line(tag + " vs fp64 reference arithmetic", compare_step(model, outs, losses, ref64, TOL["fp32"]))
    else:
        refq = oracle(O.BF16)
        line(tag + " vs bf16-aware oracle", compare_step(model, outs, losses, refq, tol_q(B)))
        line(tag + " vs fp64 reference arithmetic (bound: q-oracle's own deviation + tol_q)",
             compare_step(model, outs, losses, ref64, tol_q(B), base=oracle_deviation(refq, ref64)))


@pytest.mark.parametrize("fuse", [False, True])
def test_bf16_storage_at_the_config_widths(fuse):
    """tests/test_bf16_inputs_gpu.py::test_multimodal_step_bf16_storage_equals_fp32_storage at 1177 / 1211: padded bf16 rows (1184 / 1216
    columns) against fp32 storage of the same bf16-rounded values -- one-float fp32 rows on one side, 16-byte bf16 rows on the other."""
    A, D, S, L, E = W.BY_ID["config"].dims
    B = 1000
    g = torch.Generator().manual_seed(77)
    a = torch.randn(B, A, generator=g).abs().to(torch.bfloat16).float().to(DEV)
    b = torch.rand(B, D, generator=g).to(torch.bfloat16).float().to(DEV)
    site = torch.randint(0, S, (B,), generator=g).to(DEV)
    a16, b16 = to_bf16_rows(a), to_bf16_rows(b)
    assert a16.stride(0) == 1184 and b16.stride(0) == 1216 and a.stride(0) == 1177
    m0, m1 = S16._pair(MultiModalVAE, (A, D, S, L), "bf16")
    with probed() as tags0:
        r0 = S16._run(m0, S16._mm_fwd(a, b, site), S16._mm_loss(a, b, site), fused=[a, b, None] if fuse else None)
    with probed() as tags1:
        r1 = S16._run(m1, S16._mm_fwd(a16, b16, site), S16._mm_loss(a16, b16, site), fused=[a16, b16, None] if fuse else None)
    # the padded rows are used as they are (no conversion launch), both storages take the same launches, and those are `config`'s
    assert "rows_to_bf16" not in tags0 and "rows_to_bf16" not in tags1, (sorted(tags0), sorted(tags1))
    assert set(tags0) == set(tags1), sorted(set(tags0) ^ set(tags1))
    assert "latent.fwd" in tags1 and "class_tail" not in tags1 and {"EncoderA.L0.fwd", "EncoderB.L0.fwd", "DecoderA.L1.fwd", "DecoderB.L2.fwd"} <= set(tags1), sorted(tags1)
    assert tags1["tiny_dW.heads"][0]["grouped"] is True
    S16._compare(r0, r1, [2, 3, 4] if fuse else [0, 1, 2, 3, 4])


# ----------------------------------------------------------------------------------------------------------------------------------
# e. odd widths at the batch where the persistent and multi-split forms start
# ----------------------------------------------------------------------------------------------------------------------------------
def test_big_batch_step_vs_oracle():
    """The persistent / multi-split NT forms and the wide-tile dW form that this row is about have no tag and no planner: what is
    asserted of them is that the operands are the ones their dispatch keys on (B past ntp_min_m and the dW forms' M floor, first-layer
    K >= 256, fp32 input rows of an odd pitch, which the wide-tile form declines) -- and the numbers.  The tagged launches (fused
    latent, fused class head, the dW flush) are asserted as on every row."""
    row = W.BY_ID["big_batch"]
    assert row.B >= 16384 and row.dims[0] % 2 and row.dims[1] % 2 and row.dims[0] >= 256      # past ntp_min_m and the wide dW form's M, N, K floors
    mm_step("big_batch", "bf16")


def test_big_batch_captured_form_vs_oracle():
    captured_form("big_batch")
