"""The width tuples (A, D, S, L, E) = (RNA width, DNA width, sites, latent, embed) at which whole training steps are held to the oracle,
shared by tests/test_width_oracle_cpu.py (the oracle itself at these widths, on the CPU) and tests/test_width_space_gpu.py (the
device).  The model lives in a larger space than the default tuple 782 / 572 / 24 / 20 / 32: src/config.py carries the odd widths
1177 / 1211, the reference's hyperparameter search draws the latent from [10, 100] and the embed width from {16, 32, 64}
(optimize_hyperparameters.py:71-76), the trainers take the widths from the command line and the site count from the data.

Every row states why it is there and which launch forms it must reach or leave.  The limits restated here are the library's
(include/mmvae_hip.h); the tests check the statements against what the step really issued (the launch tags of an ops.KernelProbe,
ops.class_tail_fits) and against the parameter layout, so a row that silently takes another path than it says fails.

  fused latent launch    mmvae_latent_fwd, bf16 only: L <= 24 and, with a site table, S * 2L <= 1024 floats
  fused AE latent launch mmvae_ae_latent_fwd, bf16 only: L <= 24 and S * L <= 1024
  fused class head       mmvae_class_tail, bf16 and the captured step's form only: 4 <= S <= 32, S % 4 == 0, L <= 24
  grouped heads dW       mmvae_gemm_tn_group takes an fp32 P operand (d_heads, rows of 2L floats) only with 16-byte rows: L even
                         (the autoencoders' one head: L % 4 == 0); else every problem of that flush is a launch of its own
                         (tn_group_expect below; the probe record of the flush says which it was)
  EncoderC rider         its LDS image (S*2L + S*E + 2L*E floats) within 64 KiB; else mmvae_embed_table_bwd alone (up to 160 KiB)
  gradient arena         engine.carve_arena tiles it by numel, in VAEGraph.param_list() order: behind a tensor with an odd element
                         count the views start on 4 bytes only, until the next odd one (`arena_odd_from`: the first such tensor,
                         None: all even).  The two head biases of an encoder are adjacent, so an odd latent alone misaligns only
                         the second bias (and EncoderC's logvar weight); an odd output width (decoder_a's or decoder_c's last
                         bias) misaligns the large dW targets behind it (`misaligned_dw`: the first of them)
"""
from typing import NamedTuple, Optional

import np_oracle as O


class Row(NamedTuple):
    id: str
    dims: tuple                     # (A, D, S, L, E)
    B: int
    precs: tuple
    why: str
    latent_fused: bool              # bf16: the step issues latent.fwd (else the heads GEMMs + fuse_reparam_fwd + the stem GEMM)
    class_tail: bool                # bf16, captured form: the loss issues class_tail (else DecoderC.L1.fwd + vae_loss + DecoderC.L1.dX)
    arena_odd_from: Optional[str]   # the first MultiModalVAE parameter with an odd element count, in arena order
    misaligned_dw: Optional[str]    # the first weight of >= 16384 elements whose gradient view starts on 4 bytes only


BOTH = ("fp32", "bf16")
ROWS = [
    Row("config", (1177, 1211, 24, 20, 32), 1000, BOTH,
        "Config's own widths: one-float input, target and output rows; decoder_b's gradient views misaligned behind decoder_a's last bias",
        True, True, "decoder_a.fc.2.bias", "decoder_b.fc.2.weight"),
    Row("odd_latent", (1177, 1211, 24, 13, 16), 1000, BOTH,
        "odd latent inside every fused form's limits: 26 head columns, 52-byte mu / eps / dz rows, ldz = 16, the second head bias of "
        "every encoder on 4 bytes only; embed 16",
        True, True, "encoder_a.fc_mu.bias", "decoder_b.fc.2.weight"),
    Row("at_limits", (783, 571, 32, 16, 64), 1000, BOTH,
        "S * 2L = 1024 and S = 32: the last size every fused form takes; embed 64",
        True, True, "decoder_a.fc.2.bias", "decoder_b.fc.2.weight"),
    Row("past_table", (782, 572, 28, 20, 32), 1000, BOTH,
        "S * 2L = 1120: the fused latent launch refuses on the table alone while the class tail is still taken",
        False, True, None, None),
    Row("past_latent", (782, 572, 24, 25, 32), 1000, BOTH,
        "first latent past 24, and odd: fused latent and class tail refuse by shape; ldz = 32",
        False, False, "encoder_a.fc_mu.bias", None),
    Row("odd_sites", (781, 573, 7, 37, 64), 1000, BOTH,
        "S % 4 != 0: class tail refused, the class term's narrow paths; a prime latent",
        False, False, "encoder_a.fc_mu.bias", "decoder_a.fc.2.weight"),
    Row("many_sites", (782, 572, 33, 24, 32), 1000, BOTH,
        "S > 32 with the latent still at the fused limit: the table (1584 floats) and the class tail refuse",
        False, False, "decoder_c.fc.2.bias", "decoder_a.fc.2.weight"),
    Row("corner", (782, 572, 24, 100, 64), 1000, BOTH,
        "the search space's corner: heads of 200 columns (two column tiles), K = 100 stems; EncoderC's backward at 74.75 KiB of LDS",
        False, False, None, None),
    Row("low", (100, 96, 24, 10, 16), 1000, BOTH,
        "the lower corner: inputs below one 128-wide tile",
        True, True, None, None),
    Row("tiny_odd", (65, 63, 5, 11, 8), 1000, BOTH,
        "everything odd and below a tile, K just past 64",
        True, False, "encoder_a.fc_mu.bias", None),
    Row("big_batch", (269, 301, 24, 13, 16), 16384, ("bf16",),
        "odd widths where the persistent and multi-split forms start (ntp_min_m, M >= 8192): the first-layer dW must not take the "
        "wide-tile form, its Q rows are one-float (no tag or planner exists for GEMM forms: asserted on the operand facts and the numbers only)",
        True, True, "encoder_a.fc_mu.bias", "decoder_b.fc.2.weight"),
]
BY_ID = {r.id: r for r in ROWS}
DIRECTIONAL_ROWS = ("odd_latent", "past_latent", "corner")        # the directional VAEs and autoencoders run at these
CPU_B = 16                                                         # the batch of the oracle-against-autograd checks

# bf16 gradient tensors that exceed tol_q(B) against the bf16-aware oracle while the fp32 twin of the case holds TOL["fp32"]:
# (model kind, row) -> [(tensor, in np_oracle's names; norm)], norm `fro` = Frobenius-relative (bound 1e-2) or `grad` = scaled max
# (bound 4 / sqrt(B)).  Six tensors in five cases, each the same in the eager step and in the captured step's form.  Every case was
# rerun on these inputs with every fused form (tuning keys 10, 12, 13, 14, 15) and then every newer GEMM generation (2, 4, 6, 7, 8)
# switched off -- the same digits each time -- and at B = 4096, where the worst Frobenius figure of the case falls to the value noted:
# the excess is the weight of ReLU gates that flip where an fp32 sum and the oracle's fp64 sum round a stored pre-BatchNorm value to
# neighbouring bf16 numbers, 1 / sqrt(B) each, and more of them behind a sum of 1211 terms than behind one of 572.  A property of bf16
# storage at that width and batch, not of a launch form.  ONLY the tensor named here, in the norm named here, is taken out of the
# comparison with the bf16-aware oracle; it is held instead by the comparison with the fp64 oracle, bounded by the bf16-aware oracle's
# own deviation on the same inputs + tol_q(B) (compare_step's base=).  Every other tensor of the case, and the named tensor's other
# norm, stay at tol_q(B).
STORAGE_BOUND = {
    ("multimodal", "odd_latent"): [("encoder_b.fc.0.weight", "fro")],        # 1.036e-2 (K = 1211); case worst 3.0e-3 at B = 4096
    ("multimodal", "odd_sites"): [("encoder_b.fc.0.weight", "fro")],         # 1.033e-2; 5.0e-3 at B = 4096
    ("multimodal", "corner"): [("decoder_b.fc.0.weight", "fro")],            # 1.036e-2 (K = 100); 8.3e-3 at B = 4096
    ("dna2rna_ae", "past_latent"): [("encoder_b.fc.0.weight", "fro"),        # encoder_dna.0.weight 1.076e-2 and
                                    ("encoder_b.fc.4.weight", "fro")],       # encoder_dna.4.weight 1.041e-2; 7.4e-3 at B = 4096
    ("multimodal", "big_batch"): [("encoder_b.fc.4.weight", "grad")],        # 4.87e-2 against 4 / sqrt(16384) = 3.1e-2 (already 16 384 rows)
}

LAT_MAX_L, LAT_MAX_TABLE = 24, 1024                               # mmvae_latent_fwd / mmvae_ae_latent_fwd
EMBED_RIDER_LDS, EMBED_BWD_LDS = 64 * 1024, 160 * 1024             # mmvae_gemm_tn_group_riders / mmvae_embed_table_bwd


def latent_fits(S, L, heads=2):
    """Whether the fused latent launch takes the shape with a site table (heads = 2: mu | logvar; 1: the autoencoders)."""
    return L <= LAT_MAX_L and S * heads * L <= LAT_MAX_TABLE


def class_tail_fits(S, L):
    return 4 <= S <= 32 and S % 4 == 0 and L <= LAT_MAX_L


def heads_dw_grouped(L, heads=2):
    """d_heads is fp32 [B][heads * L] without padding: the grouped dW launch wants its rows 16-byte aligned."""
    return (heads * L) % 4 == 0


def tn_group_expect(prec, S, L):
    """Whether the MultiModalVAE backward's last flush of small-output dW GEMMs runs as ONE grouped launch (True) or one launch per
    problem (False); None where these widths do not decide it.  mmvae_gemm_tn_group classifies every problem and refuses the whole
    group if one does not fit (gemm_tn.hip, tn_group_combo):
      * the encoders' heads: P = d_heads, fp32 rows of 2L floats, N = 2L -- needs ldp % 4 == 0: refused at an odd latent;
      * the decoders' first layers: Q = z with K = L -- in fp32 mode an fp32 operand needs K % 4 == 0;
      * DecoderC's last layer: P = the class-logit gradient with N = S -- S % 4 == 0 takes every form of it; else not stated."""
    if L % 2 or (prec == "fp32" and L % 4):
        return False
    return True if S % 4 == 0 else None


def embed_bwd_lds(S, L, E, heads=2):
    return (S * heads * L + S * E + heads * L * E) * 4


# A ReLU gate that the fp64 oracle sees within fp32 rounding of zero may fall on the other side on the device, and ONE flipped gate
# moves one row of a first-layer dW by one sample's whole contribution: ~1 / sqrt(B) of the row's scale, 1e-2 at B = 1000 against the
# 5e-3 the fp32 step is held to.  (Measured on the device before the cases were conditioned: `at_limits` fp32, encoder_b.fc.0.weight
# off by 1.1e-2 scaled, all of it in row 494 and along sample 72's input, whose gate the oracle has at 6.1e-8; the dna2rna autoencoder
# at `odd_latent`, 5.05e-3, row 152 / sample 848, gate at 4.1e-7.)  An fp32 GEMM over K <= 1211 terms carries a rounding error of about
# sqrt(K) * 2^-24 ~ 2e-6 of a unit-scale pre-activation, so the cases leave no kept gate of an encoder within GATE_MARGIN = 1e-5 of
# zero: such a unit is dropped for that sample (its keep-mask entry set to 0, a handful out of ~10^6), decided from the oracle's
# forward alone.  Behind a dropped unit neither side has a gradient whatever the sign, and the tolerances stay what they are.
GATE_MARGIN = 1e-5


def settle_gates(masks, gates_of, margin=GATE_MARGIN, rounds=8):
    """masks: {name: uint8 (B, width) keep-mask}; gates_of(masks) -> {name: the fp64 oracle's post-BatchNorm pre-ReLU values under
    those masks}.  -> (a copy of the masks in which every kept unit whose gate lies within `margin` of zero is dropped, how many).
    Dropping a unit in one layer moves the next layer's gates a little, so the forward is repeated until none is left."""
    masks = {k: v.copy() for k, v in masks.items()}
    dropped = 0
    for _ in range(rounds):
        gates = gates_of(masks)
        risky = {k: (abs(gates[k]) < margin) & (masks[k] != 0) for k in gates}
        n = sum(int(r.sum()) for r in risky.values())
        if n == 0:
            return masks, dropped
        for k, r in risky.items():
            masks[k][r] = 0
        dropped += n
    raise RuntimeError("settle_gates: gates still within the margin")


def _layer_gates(prefix, layers):
    return {f"{prefix}.{c['bi'] + 2}": c["yh"] for c in layers}                     # the Dropout sits two places behind the BatchNorm


def mm_gates(P64, Bf64, a, b, site, eps):
    """gates_of for np_oracle.vae_forward on (a, b, site), float64 inputs"""
    def gates_of(masks):
        cache = O.vae_forward(P64, dict(Bf64), a, b, site, masks, eps, True)[5]
        return {**_layer_gates("encoder_a.fc", cache["enc_a"]["layers"]), **_layer_gates("encoder_b.fc", cache["enc_b"]["layers"])}
    return gates_of


def directional_gates(kind, P64, Bf64, x, site, eps):
    """gates_of for np_oracle.directional_forward"""
    def gates_of(masks):
        cache = O.directional_forward(kind, P64, dict(Bf64), x, site, masks, eps, True)[3]
        return _layer_gates(cache["enc_x"]["pre"] + ".fc", cache["enc_x"]["layers"])
    return gates_of


def ae_gates(kind, P, Bf, x, site):
    """gates_of for tests/ae_oracle.py's forward"""
    import ae_oracle as AO

    def gates_of(masks):
        cache = AO.forward(kind, P, dict(Bf), x, site, masks, True)[2]
        return _layer_gates(AO.KINDS[kind][0], cache["enc"]["layers"])
    return gates_of


def first_odd(named_numels):
    """[(name, numel)] in arena order -> the first name with an odd numel, or None."""
    return next((k for k, n in named_numels if n % 2), None)
