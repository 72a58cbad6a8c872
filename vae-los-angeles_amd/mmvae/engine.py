"""Launch orchestration of the MultiModalVAE training path on one MI355X.

The compute blocks mirror the reference modules (file:line in each docstring) but each is a
short sequence of launches into libmmvae_hip.so; no torch arithmetic is used on the data path.
Activations between GEMMs are stored in the *activation type* of the precision mode (bf16 or
f32); BatchNorm statistics, loss sums, gradients of parameters and the optimiser are fp32.

What is saved for backward per BN layer (a `LayerSave`) is only the PRE-BatchNorm GEMM output, the
per-column (mean, rstd, scale, shift) and the dropout keep-mask: post-activation tensors are
recomputed inside the consumer GEMM's operand prologue (an `ops.Prologue`).

What travels from the forward through the loss to the backward is one `StepState`: the layer saves
of each encoder, the decoders' activations, eps / logvar, the step's zeroed buffers (`StepZeros`:
ONE allocation, laid out by `VAEGraph.zero_pack`), and what the loss adds on the way -- the
reconstruction losses computed inside the decoder GEMMs (`FusedRecon`) and the gradients the loss
kernel left for the backward (`LossGrads`).
"""
import os
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch

from . import ops
from . import _lib as L_
from .ops import (PREC_BF16, PREC_F32, ACT_NONE, ACT_RELU, ACT_SIGMOID, EPI_RELU_MASK, EPI_BN_BWD, DROP_P,
                  ceil_to, act_dtype, Prologue, BnBwdEpilogue, BnBwdFinalize, BnBwdApply)

_PRECISIONS = {"bf16": PREC_BF16, "fp32": PREC_F32, "f32": PREC_F32}
_default_precision = _PRECISIONS[os.environ.get("MMVAE_PRECISION", "bf16").lower()]
_TINY_DW_MAX = 16384                                                       # N*K at or below which a dW GEMM counts as small-output


def set_default_precision(name):
    """'bf16' (bf16 MFMA operands/activations, f32 accumulate) or 'fp32' (f32 MFMA)."""
    global _default_precision
    _default_precision = _PRECISIONS[name.lower()]


def default_precision():
    return _default_precision


# --------------------------------------------------------------------------------------------
# noise
# --------------------------------------------------------------------------------------------
class NoiseSource:
    """Dropout keep-masks and eps.  Default: ONE Philox launch per forward (all masks of the pass in one uint8
    buffer + eps), keyed by (torch.initial_seed() [+ rank], a DEVICE-resident running offset) -- the offset lives on
    the device so that a captured hipGraph draws fresh noise on every replay.  `inject` replays explicit arrays in the
    order the reference consumes its RNG (EncoderA mask, EncoderB masks, eps): parity tests."""

    def __init__(self):
        self._injected = None
        self._offsets = {}            # device -> int64[1] tensor (bit pattern of the uint64 Philox offset)
        self.stream_rank = None       # None: torch.distributed's rank; an int: draw THAT rank's stream (single-process restatement of N ranks)

    def inject(self, masks, eps):
        self._injected = (list(masks), eps)

    def clear(self):
        self._injected = None

    def _seed(self):
        seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
        rank = self.stream_rank
        if rank is None and torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()
        if rank is not None:
            seed = (seed + 0x9E3779B97F4A7C15 * (int(rank) + 1)) & 0xFFFFFFFFFFFFFFFF
        return seed

    def offset_tensor(self, device):
        t = self._offsets.get(device)
        if t is None:
            t = self._offsets[device] = torch.zeros(L_.CTR_COPIES, dtype=torch.int64, device=device)    # identical copies, see mmvae_noise
        return t

    def state_dict(self, device):
        """Position of the Philox stream on `device` (one host read): part of a resumable checkpoint."""
        t = self._offsets.get(torch.device(device) if not isinstance(device, torch.device) else device)
        return {"offset": 0 if t is None else int(t[0].item())}

    def load_state_dict(self, state, device):
        device = torch.device(device) if not isinstance(device, torch.device) else device
        self.offset_tensor(device).fill_(int(state["offset"]))

    def draw(self, B, widths, Ld, device):
        """-> ([uint8 (B,w) keep-mask for w in widths], eps fp32 (B,Ld) or None if Ld is None)."""
        masks, eps, launch = self.plan(B, widths, Ld, device)
        if launch is not None:
            ops.noise(*launch)                           # the launch advances the device offset itself
        return masks, eps

    def plan(self, B, widths, Ld, device):
        """draw() without its launch -> (masks, eps, ops.noise()'s arguments): the caller issues the launch, alone or as a role of
        ops.step_head.  Injected arrays need none: the third result is then None."""
        if self._injected is not None:
            masks = []
            for w in widths:
                m = self._injected[0].pop(0)
                if tuple(m.shape) != (B, w):
                    raise ValueError(f"injected mask shape {tuple(m.shape)} != {(B, w)}")
                masks.append(m.to(device=device, dtype=torch.uint8).contiguous())
            eps = None
            if Ld is not None:
                eps = self._injected[1]
                if tuple(eps.shape) != (B, Ld):
                    raise ValueError(f"injected eps shape {tuple(eps.shape)} != {(B, Ld)}")
                eps = eps.to(device=device, dtype=torch.float32).contiguous()
            return masks, eps, None
        segs, total = [], 0
        for w in widths:
            segs.append(total)
            total = ceil_to(total + B * w, 16)
        buf = torch.empty(total, dtype=torch.uint8, device=device) if total else None
        eps = torch.empty(B, Ld, dtype=torch.float32, device=device) if Ld is not None else None
        off = self.offset_tensor(device)
        return [buf[o:o + B * w].view(B, w) for o, w in zip(segs, widths)], eps, (buf, eps, 1.0 - DROP_P, self._seed(), 0, off, True)


GLOBAL_NOISE = NoiseSource()


# --------------------------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------------------------
def _check_input(x, name, cols, prec):
    """The operand of a first-layer GEMM.  bf16 inputs ("bf16 storage"): in bf16 mode a matrix in the padded-row
    layout (ops.is_bf16_rows; what mmvae.to_bf16_rows returns) is used as it is -- the forward GEMM's A, the dW GEMM's Q, the
    reconstruction loss's target, no copy; any other bf16 matrix is converted into that layout once per call (the slow path: one
    mmvae_rows_to_bf16 launch and a copy of the input).  In fp32 mode a bf16 input is widened to fp32 (exact)."""
    if x.dim() != 2 or x.shape[1] != cols:
        raise RuntimeError(f"{name}: expected shape (B, {cols}), got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError(f"{name}: the MI355X path needs CUDA/HIP tensors (got {x.device}); there is no CPU fallback")
    if x.dtype == torch.bfloat16:
        if prec != PREC_BF16:
            return x.float()
        return x if ops.is_bf16_rows(x) else ops.to_bf16_rows(x)
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(1) != 1:
        x = x.contiguous()
    return x


def zeros_pack(device, specs, fill=True):
    """[(numel, dtype)] -> zero-filled tensors carved out of ONE allocation (one memset launch instead of one per tensor).
    fill=False: allocated only -> (tensors, the allocation): the caller zeroes it (a role of ops.step_head)."""
    offs, total = [], 0
    for n, dt in specs:
        offs.append(total)
        total += ceil_to(n * _ITEMSIZE[dt], 16)
    buf = (torch.zeros if fill else torch.empty)(max(total, 16), dtype=torch.uint8, device=device)
    out = [buf[o:o + n * _ITEMSIZE[dt]].view(dt) for o, (n, dt) in zip(offs, specs)]
    return out if fill else (out, buf)


_ITEMSIZE = {torch.float32: 4, torch.float64: 8, torch.uint8: 1, torch.int64: 8}


def carve_arena(flat, params):
    """{param: view of its shape} tiling the flat fp32 gradient arena in the order of `params`."""
    views, off = {}, 0
    for p in params:
        views[p] = flat[off:off + p.numel()].view(p.shape)
        off += p.numel()
    return views


class PrepCache:
    """The prepared (MFMA operand) weights of a module tree: rebuilt when the precision, the device or the storage of a parameter
    changes, and refreshed from the fp32 masters by ONE launch on every call.  It holds no reference to its owner (an owner that
    kept bound methods of itself here would be freed only by the cyclic GC, with its gradients and prepared weights in HBM)."""

    def __init__(self):
        self.key = self.prep = None

    def ensure(self, prec, device, params, build, run=True):
        """params: the parameters; build(prec, device) -> their PreparedLinears.  run=False: no launch -> the ops.WeightPrep (or
        None) for the caller to run, alone or as a role of ops.step_head -- on every call all the same: the masters may have
        been rewritten in place since the last one."""
        key = (prec, str(device)) + tuple(p.data_ptr() for p in params)
        if key != self.key:
            pls = build(prec, device)
            self.prep = ops.WeightPrep(pls, device) if pls else None
            self.key = key
        if run and self.prep is not None:
            self.prep.run()
        return self.prep


class BNState:
    """Per-layer BatchNorm vectors: rows of one [4][N] fp32 buffer (mean, rstd, scale, shift)."""

    def __init__(self, N, device):
        self.buf = torch.empty(4, N, dtype=torch.float32, device=device)
        self.mean, self.rstd, self.scale, self.shift = self.buf[0], self.buf[1], self.buf[2], self.buf[3]


class LayerSave(NamedTuple):
    """What the backward needs of one [Linear -> BatchNorm -> ReLU -> Dropout] layer."""
    q: torch.Tensor                     # the dW GEMM's Q operand: the layer's input as stored, or its kept post-activation form
    q_prologue: Optional[Prologue]      # what turns the stored input into the layer's input on load (None: first layer, or kept)
    y: torch.Tensor                     # the Linear's output, before BatchNorm
    bn: BNState
    y_prologue: Prologue                # what the consumer of y applies: this layer's BatchNorm + ReLU + Dropout


class FusedRecon(NamedTuple):
    """Reconstruction losses computed inside the decoders' last GEMMs (VAEGraph.fused_recon)."""
    sums: torch.Tensor                  # float64[5] loss accumulators those GEMMs added to
    out5: torch.Tensor                  # float32[5] that mmvae_loss_finalize fills from them
    g: dict                             # decoder index -> gradient w.r.t. its pre-activation output
    targets: dict                       # decoder index -> the target the forward was given


@dataclass(slots=True, eq=False)
class LossGrads:
    """Gradients the fused loss left for the backward of the forward that produced its inputs (functional, "fused hand-off")."""
    g_outs: list                        # per decoder: activation-typed gradient (w.r.t. the logits behind a Sigmoid) or None
    g_mu: torch.Tensor
    g_lv: torch.Tensor
    unit_grad: bool                     # the caller promised loss.backward() with the default gradient of 1
    scale: Optional[torch.Tensor] = None        # the gradient that arrived at the loss (device scalar), unless unit_grad
    armed: bool = False                 # the loss's own backward ran


@dataclass(slots=True, eq=False)
class ClassTail:
    """The class decoder's last Linear, left out of the forward for the fused class-head launch (ops.class_tail): the loss runs it
    with the class / KL terms and the Linear's dX in one launch, or -- where the library refuses -- issues the Linear itself."""
    index: int                          # which decoder
    head: object                        # its last layer's PreparedLinear
    h0: torch.Tensor                    # (B, 64) its hidden activation: a column slice of the merged stems' output
    d0: torch.Tensor                    # (B, stem.N) gradient w.r.t. the merged stems' output, allocated with the step state
    d0_slice: torch.Tensor              # this decoder's columns of d0
    name: str                           # the decoder's name, for the launch tags
    done: bool = False                  # the fused launch ran: d0_slice holds the gradient, the backward skips the Linear's dX

    def logits(self, prec):
        """The launch the forward left out -> fp32 (B, S)."""
        out = torch.empty(self.h0.shape[0], self.head.N, dtype=torch.float32, device=self.h0.device)
        ops.gemm_nt(prec, self.h0, self.head.w, self.head.N, self.head.K, out, bias=self.head.bias, act=ACT_NONE, tag=f"{self.name}.L1.fwd")
        return out


@dataclass(slots=True, eq=False)
class StepZeros:
    """Everything one step needs zeroed, in the order of its regions inside ONE allocation (VAEGraph.zero_pack).  The forward half
    is the first two fields (loss_ws only when a backward follows), the backward half the last three."""
    fwd_stats: list                     # per BN layer: float64 (2, width) sums of the forward BatchNorm
    loss_ws: Optional[tuple]            # (sums float64[5], out5 float32[5]) as ops.loss_workspace; None once the loss took it
    arena: Optional[torch.Tensor]       # flat fp32 gradient arena (param_list() order)
    bwd_stats: list                     # per BN layer: float64 (2, width) sums of the BatchNorm backward
    d_table: Optional[torch.Tensor]     # (copies, sites, table_width * latent): the EmbedEncoder's table gradient, summed over the copies in its backward
    unfilled: Optional[torch.Tensor] = None     # zero_pack(fill=False): the whole allocation, still to be zeroed by the caller


@dataclass(slots=True, eq=False)
class StepState:
    """One forward's state for the loss and the backward.  Parts that are absent (an encoder that did not run, no fused
    reconstruction loss, no fused loss yet) are None."""
    prec: int
    B: int
    train: bool
    eps: Optional[torch.Tensor] = None
    logvar: Optional[torch.Tensor] = None
    n_mod: int = 0
    enc_a: Optional[list] = None        # [LayerSave]
    enc_b: Optional[list] = None
    site: Optional[torch.Tensor] = None
    dec: Optional[list] = None          # per decoder: (activations, output)
    zeros: Optional[StepZeros] = None   # the forward's memset when a backward follows; dropped where the backward starts
    fused: Optional[FusedRecon] = None
    loss_grads: Optional[LossGrads] = None
    class_tail: Optional[ClassTail] = None
    tail_riders: bool = False           # VAEGraph.tail_riders at the forward: the loss leaves its finalisation to the backward
    loss_tail: Optional[tuple] = None   # ops.loss_finalize's arguments, left by that loss for the backward's last launch
    consumed: bool = False              # the backward ran: buffers are not retained


# --------------------------------------------------------------------------------------------
# blocks
# --------------------------------------------------------------------------------------------
class EncoderMLP:
    """EncoderA / EncoderB (reference src/models/encoders.py:8-23, 26-46):
    [Linear -> BatchNorm1d -> ReLU -> Dropout(0.1)] x n, then the fc_mu | fc_logvar heads
    computed as ONE GEMM with N = 2*latent.
    fc_logvar=None: the single-head form of the autoencoders (directional_ae.py:20-26, 81-91) -- the stack ends in ONE
    Linear(hidden, latent) (`fc_mu` here): the head GEMM has N = latent, the arena one weight and one bias."""

    def __init__(self, linears, bns, fc_mu, fc_logvar=None, name="enc"):
        self.linears, self.bns, self.fc_mu, self.fc_logvar = list(linears), list(bns), fc_mu, fc_logvar
        self.in_dim = self.linears[0].in_features
        self.latent = fc_mu.out_features
        self.head_width = self.latent * (1 if fc_logvar is None else 2)
        self.name = name

    def prepare(self, prec, device):
        self.pl = [ops.PreparedLinear([l.weight], [l.bias], prec, device) for l in self.linears]
        heads = [self.fc_mu] if self.fc_logvar is None else [self.fc_mu, self.fc_logvar]
        self.pl_heads = ops.PreparedLinear([h.weight for h in heads], [h.bias for h in heads], prec, device)
        return self.pl + [self.pl_heads]

    def params(self):
        """Order of the gradient arena (heads adjacent so that one TN GEMM writes both)."""
        out = []
        for l, bn in zip(self.linears, self.bns):
            out += [l.weight, l.bias, bn.weight, bn.bias]
        if self.fc_logvar is None:
            return out + [self.fc_mu.weight, self.fc_mu.bias]
        out += [self.fc_mu.weight, self.fc_logvar.weight, self.fc_mu.bias, self.fc_logvar.bias]
        return out

    def widths(self):
        return [l.out_features for l in self.linears]

    def _consume(self, prec, h, pro, fin, N, K, out, bias, w, tag, stats=None, pro_out=None):
        """GEMM on (h, pro) that also finalises h's BatchNorm statistics (`fin`, owed by the layer that produced h) when the library
        can fold that in; else the launch of its own.  Returns pro_out if the launch wrote it, else None."""
        if fin is not None:
            try:
                ops.gemm_nt(prec, h, w, N, K, out, bias=bias, prologue=pro, stats=stats, tag=tag, pro_out=pro_out, pro_finalize=fin)
                return pro_out
            except L_.MMVAEArgError:
                pass                                   # refused before anything was enqueued (argument check)
            ops.bn_finalize_launch(fin)
        try:
            ops.gemm_nt(prec, h, w, N, K, out, bias=bias, prologue=pro, stats=stats, tag=tag, pro_out=pro_out)
            return pro_out
        except L_.MMVAEArgError:
            if pro_out is None:
                raise
            # the library did not take the problem on the kernel that writes pro_out: the ordinary call, and the backward redoes
            # the prologue on its operand load
            ops.gemm_nt(prec, h, w, N, K, out, bias=bias, prologue=pro, stats=stats, tag=tag)
            return None

    def forward(self, prec, x, train, masks, stats_bufs=None, want_bwd=False, heads=True):
        """masks: one uint8 (B, width) keep-mask per BN layer (training) or None (eval).
        stats_bufs: optional pre-zeroed float64 (2, N) accumulators, one per BN layer.
        heads=False: stop before the heads -- returns (ops.LatentEncoder, layers): the last layer's output with its prologue and the
        finalisation still owed, for VAEGraph's fused latent launch (or run_heads() when the library does not take it)."""
        B, dev = x.shape[0], x.device
        adt = act_dtype(prec)
        layers = []
        h, pro = x, None
        fin = None            # the BatchNorm finalisation of the layer that produced h, still owed: it rides in the GEMM that consumes h
        for lin, bn, pl in zip(self.linears, self.bns, self.pl):
            N, K = pl.N, pl.K
            y = torch.empty(B, ceil_to(N, 8), dtype=adt, device=dev)
            st = BNState(N, dev)
            # a hidden BN layer on the wave-specialised kernel: its producers also write the operand AFTER the prologue (the previous
            # layer's post-activation, 2 bytes per element), which lets this layer's dW GEMM run the plain LDS-DMA kernel instead of
            # redoing the prologue on its Q operand (EncoderB's second Linear: 52 -> 39 us for the dW GEMM)
            h_act = None
            if want_bwd and pro is not None and ops.can_keep_pro_out(prec, B, N, K, h, y) and pro.mask is not None \
                    and pro.mask.stride(0) % 8 == 0 and pro.mask.data_ptr() % 8 == 0:
                h_act = torch.empty(B, K, dtype=torch.bfloat16, device=dev)
            if train:
                stats = stats_bufs[len(layers)] if stats_bufs is not None else torch.zeros(2, N, dtype=torch.float64, device=dev)
                h_act = self._consume(prec, h, pro, fin, N, K, y, pl.bias, pl.w, f"{self.name}.L{len(layers)}.fwd", stats=stats, pro_out=h_act)
                # the finalisation of THIS layer's statistics is owed to whoever reads y next (the next layer or the heads)
                fin = ops.bn_finalize_args(B, N, stats, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                           bn.num_batches_tracked, st.mean, st.rstd, st.scale, st.shift, bn.eps,
                                           bn.momentum if bn.momentum is not None else 0.1)
                new_pro = Prologue(st.scale, st.shift, masks[len(layers)], 1.0 / (1.0 - DROP_P))
            else:
                ops.gemm_nt(prec, h, pl.w, N, K, y, bias=pl.bias, prologue=pro, tag=f"{self.name}.L{len(layers)}.fwd")
                ops.bn_eval_coeffs(bn.weight, bn.bias, bn.running_mean, bn.running_var, st.scale, st.shift, bn.eps, st.mean, st.rstd)
                new_pro = Prologue(st.scale, st.shift, None, 1.0)
            layers.append(LayerSave(h, pro, y, st, new_pro) if h_act is None else LayerSave(h_act, None, y, st, new_pro))      # backward's Q operand: plain when kept
            h, pro = y, new_pro
        owed = ops.LatentEncoder(h, pro, fin, self.pl_heads)
        return (self.run_heads(prec, owed) if heads else owed), layers

    def run_heads(self, prec, owed):
        """The fc_mu | fc_logvar heads as a GEMM of their own -> fp32 (B, 2 * latent); (B, latent) in the single-head form."""
        heads = torch.empty(owed.y.shape[0], self.head_width, dtype=torch.float32, device=owed.y.device)
        self._consume(prec, owed.y, owed.prologue, owed.fin, self.head_width, self.pl_heads.K, heads, self.pl_heads.bias, self.pl_heads.w,
                      f"{self.name}.heads.fwd")
        return heads

    def backward(self, prec, layers, d_heads, grads, tn=ops.gemm_tn, stats_bufs=None, train=True, d_heads_lp=None):
        """d_heads: [B][2L] fp32 ([B][L] in the single-head form).  grads: dict param -> fp32 view (pre-zeroed, accumulated).
        train=False: the forward ran in eval mode (running statistics, no dropout) -- torch's
        batch_norm(training=False) backward: dy = gamma * rstd * d, no batch-statistics correction."""
        B, dev = d_heads.shape[0], d_heads.device
        adt = act_dtype(prec)
        L2 = self.head_width
        Kl = self.pl_heads.K
        gw = grads[self.fc_mu.weight]            # fc_logvar.weight follows immediately in the arena
        gb = grads[self.fc_mu.bias]
        tn(prec, d_heads, layers[-1].y, _span(gw, L2 * Kl).view(L2, Kl), _span(gb, L2), L2, Kl, q_prologue=layers[-1].y_prologue, tag=f"{self.name}.heads.dW")
        # gradient entering the last hidden layer: dX GEMM of the heads (A = d_heads, W = heads^T)
        src, src_wt, src_n, src_k = (d_heads_lp if d_heads_lp is not None else d_heads), self.pl_heads.wt, Kl, L2
        for i in reversed(range(len(self.linears))):
            lin, bn, pl = self.linears[i], self.bns[i], self.pl[i]
            sv = layers[i]
            y = sv.y
            st = sv.bn
            N, K = pl.N, pl.K
            bnargs = BnBwdEpilogue(st.scale, st.shift, st.mean, st.rstd, sv.y_prologue.mask, sv.y_prologue.inv_keep)
            # BatchNorm/ReLU/Dropout backward of layer i: ONE contraction that stores d = dX * keep * relu' and accumulates
            # (sum d, sum d*xhat); then the BN correction in place (mmvae_bn_bwd_apply) or on the dW GEMM's operand load.
            stats = stats_bufs[i] if stats_bufs is not None else torch.zeros(2, N, dtype=torch.float64, device=dev)
            coef = torch.empty(3, N, dtype=torch.float32, device=dev)
            d = torch.empty(B, ceil_to(N, 8), dtype=adt, device=dev)                  # d := dL/dy_i
            ops.gemm_nt(prec, src, src_wt, src_n, src_k, d, epilogue=EPI_BN_BWD, h=y, bn=bnargs, bn_phase=2, stats=stats, tag=f"{self.name}.L{i}.dX")
            # The finalisation of the backward sums (dgamma, dbeta, the three constants per column) rides in the launch that consumes
            # them -- the first layer's dW GEMM or the in-place correction pass -- instead of a 5 us launch of its own (round 3); the
            # library answers ERR_ARG where its kernels cannot do that (small batches, unusual widths): then the separate launch.
            fin = BnBwdFinalize(stats, bn.weight, grads[bn.weight], grads[bn.bias], not train)
            # (not for very wide inputs -- the scaled omics widths: the dW GEMM then has hundreds of K tiles and every one of them
            # would redo the correction of its P rows; one pass over d is cheaper)
            if i == 0 and K <= 4096:
                # first layer: only the dW GEMM consumes dL/dy -> the correction rides on its operand load, no pass over d
                if prec == PREC_BF16 and B >= 8192 and N >= 128 and K >= 256:
                    try:
                        tn(prec, d, sv.q, grads[lin.weight], grads[lin.bias], N, K, q_prologue=sv.q_prologue,
                           p_prologue=BnBwdApply(y, st.mean, st.rstd, fin=fin), tag=f"{self.name}.L{i}.dW")
                        continue
                    except L_.MMVAEArgError:
                        pass                                   # refused before anything was enqueued
                ops.bn_bwd_finalize(B, N, stats, bn.weight, st.rstd, grads[bn.weight], grads[bn.bias], coef, eval_mode=not train)
                tn(prec, d, sv.q, grads[lin.weight], grads[lin.bias], N, K, q_prologue=sv.q_prologue,
                   p_prologue=BnBwdApply(y, st.mean, st.rstd, coef), tag=f"{self.name}.L{i}.dW")
                continue
            try:
                ops.bn_bwd_finalize_apply(d, y, B, N, st.mean, st.rstd, *fin)
            except L_.MMVAEArgError:
                ops.bn_bwd_finalize(B, N, stats, bn.weight, st.rstd, grads[bn.weight], grads[bn.bias], coef, eval_mode=not train)
                ops.bn_bwd_apply(d, y, N, st.mean, st.rstd, coef)
            tn(prec, d, sv.q, grads[lin.weight], grads[lin.bias], N, K, q_prologue=sv.q_prologue, tag=f"{self.name}.L{i}.dW")
            src, src_wt, src_n, src_k = d, pl.wt, K, N


def _span(t, n):
    """View of n contiguous fp32 elements starting at tensor t (inside the gradient arena)."""
    return torch.as_strided(t, (n,), (1,))


class EmbedEncoder:
    """EncoderC (encoders.py:49-61): Embedding(S,E) + two heads == a [S][2L] table + gather.
    fc_logvar=None: the autoencoders' site path (directional_ae.py:29-30, 52-56) -- Embedding(S,E) -> ONE Linear(E, latent) (`fc_mu`
    here) == a [S][L] table + gather, through the one-head launches ops.embed_proj_fwd / embed_proj_bwd."""

    def __init__(self, embedding, fc_mu, fc_logvar=None):
        self.embedding, self.fc_mu, self.fc_logvar = embedding, fc_mu, fc_logvar
        self.latent = fc_mu.out_features
        self.table_width = 1 if fc_logvar is None else 2       # table columns per latent dimension
        # the two-head table has a role in the step's shared launches: ops.step_head may make it, and its backward may run as rider
        # workgroups of the grouped dW launch (ops.tn_riders).  The one-head table and its backward are always launches of their own.
        self.rides = fc_logvar is not None
        self._heads = [fc_mu] if fc_logvar is None else [fc_mu, fc_logvar]

    def prepare(self, prec, device):
        return []

    def params(self):
        """Order of the gradient arena: the embedding, then weight and bias head by head."""
        return [self.embedding.weight] + [p for h in self._heads for p in (h.weight, h.bias)]

    def table_args(self):
        """ops.embed_table_fwd's arguments (ops.embed_proj_fwd's in the one-head form), the table (the last of them) freshly allocated."""
        emb = self.embedding.weight
        t = torch.empty(emb.shape[0], self.table_width * self.latent, dtype=torch.float32, device=emb.device)
        return (emb, *(p for h in self._heads for p in (h.weight, h.bias)), t)

    def table(self, args=None):
        """The table by a launch of its own (args: table_args() made earlier)."""
        args = self.table_args() if args is None else args
        (ops.embed_table_fwd if self.rides else ops.embed_proj_fwd)(*args)
        return args[-1]

    def backward_args(self, d_table, grads):
        """ops.embed_table_bwd's arguments (ops.embed_proj_bwd's in the one-head form)."""
        return (self.embedding.weight, *(h.weight for h in self._heads), d_table, grads[self.embedding.weight],
                *(grads[p] for h in self._heads for p in (h.weight, h.bias)))

    def launch_backward(self, *args):
        (ops.embed_table_bwd if self.rides else ops.embed_proj_bwd)(*args)

    def backward(self, d_table, grads):
        self.launch_backward(*self.backward_args(d_table, grads))


class DecoderMLP:
    """DecoderA/B/C (src/models/decoders.py:8-50): Linear(+ReLU) chain, optional final Sigmoid.
    Hidden activations are stored in the activation type, the output in fp32 (it is returned
    to the caller)."""

    def __init__(self, linears, final_sigmoid, name="dec"):
        self.linears, self.final_sigmoid = list(linears), final_sigmoid
        self.out_dim = self.linears[-1].out_features
        self.name = name

    def prepare(self, prec, device):
        self.pl = [ops.PreparedLinear([l.weight], [l.bias], prec, device) for l in self.linears]
        return self.pl

    def params(self):
        out = []
        for l in self.linears:
            out += [l.weight, l.bias]
        return out

    def can_fuse_loss(self, prec):
        """The reconstruction loss can run inside the last layer's GEMM (EPI_LOSS_*): bf16 mode, a hidden layer in front of it
        (bf16 A operand) and more than one K step."""
        return prec == ops.PREC_BF16 and len(self.pl) >= 2 and self.pl[-1].K > 64

    def forward(self, prec, z, fused_loss=None, first=None):
        """fused_loss = (target fp32 or bf16 [B][N], one-element float64 accumulator): the last layer does not store its output; its GEMM
        epilogue adds the reconstruction loss (sum-MSE, or sum-BCE behind the final Sigmoid: losses.py:31,34) to the accumulator and
        writes the bf16 gradient w.r.t. the pre-activation output.  Returns (gradient, acts) then instead of (output, acts).
        first: output of layer 0 computed elsewhere (VAEGraph's merged first layers of all decoders), a [B][N0] column slice."""
        B, dev = z.shape[0], z.device
        adt = act_dtype(prec)
        acts = [z]
        h = z
        if first is not None:
            acts.append(first)
            h = first
        for j, pl in enumerate(self.pl):
            if j == 0 and first is not None:
                continue
            last = j == len(self.pl) - 1
            if last and fused_loss is not None:
                target, acc = fused_loss
                # fp32, or bf16 storage (padded bf16 rows read in the widest pieces; any bf16 rows are accepted by the kernel)
                if tuple(target.shape) != (B, pl.N) or target.dtype not in (torch.float32, torch.bfloat16) or target.stride(1) != 1 \
                        or not target.is_cuda:
                    raise ValueError(f"fused reconstruction loss: target must be fp32 or bf16 [{B}, {pl.N}] with unit inner stride, "
                                     f"got {tuple(target.shape)} {target.dtype}")
                out = torch.empty(B, ceil_to(pl.N, 8), dtype=adt, device=dev)
                ops.gemm_nt(prec, h, pl.w, pl.N, pl.K, out, bias=pl.bias, epilogue=ops.EPI_LOSS_BCE_LOGIT if self.final_sigmoid else ops.EPI_LOSS_MSE,
                            h=target, loss_sum=acc, tag=f"{self.name}.L{j}.fwd")
            elif last:
                out = torch.empty(B, pl.N, dtype=torch.float32, device=dev)
                ops.gemm_nt(prec, h, pl.w, pl.N, pl.K, out, bias=pl.bias, act=ACT_SIGMOID if self.final_sigmoid else ACT_NONE, tag=f"{self.name}.L{j}.fwd")
            else:
                out = torch.empty(B, ceil_to(pl.N, 8), dtype=adt, device=dev)
                ops.gemm_nt(prec, h, pl.w, pl.N, pl.K, out, bias=pl.bias, act=ACT_RELU, tag=f"{self.name}.L{j}.fwd")
                acts.append(out)
            h = out
        return h, acts

    def backward(self, prec, acts, out, g_out, g_is_logit_grad, dz, grads, tn=ops.gemm_tn, d0_out=None, dx_done=None):
        """g_out: gradient w.r.t. the decoder output ([B][>=N], fp32 or activation type).  For a
        sigmoid decoder it is w.r.t. the pre-sigmoid logits iff g_is_logit_grad.
        d0_out: where the gradient w.r.t. layer 0's output goes (a column slice of the buffer VAEGraph multiplies with the merged
        first-layer weights of all decoders); layer 0's own dX GEMM is then skipped and dz is not touched.
        dx_done: the gradient w.r.t. the LAST layer's input, already computed (the fused class-head launch): its dX GEMM is skipped."""
        B, dev = g_out.shape[0], g_out.device
        adt = act_dtype(prec)
        d = g_out
        if self.final_sigmoid and not g_is_logit_grad:
            dl = torch.empty(B, ceil_to(self.out_dim, 8), dtype=adt, device=dev)
            ops.sigmoid_bwd(g_out, out, dl)
            d = dl
        for j in reversed(range(len(self.pl))):
            pl, lin = self.pl[j], self.linears[j]
            tn(prec, d, acts[j], grads[lin.weight], grads[lin.bias], pl.N, pl.K, tag=f"{self.name}.L{j}.dW")
            if j > 0 and j == len(self.pl) - 1 and dx_done is not None:
                d = dx_done
            elif j > 0:
                d_prev = d0_out if (j == 1 and d0_out is not None) else torch.empty(B, ceil_to(pl.K, 8), dtype=adt, device=dev)
                ops.gemm_nt(prec, d, pl.wt, pl.K, pl.N, d_prev, epilogue=EPI_RELU_MASK, h=acts[j], tag=f"{self.name}.L{j}.dX")
                d = d_prev
            elif d0_out is None:
                ops.gemm_nt(prec, d, pl.wt, pl.K, pl.N, dz, tag=f"{self.name}.L{j}.dX")


# --------------------------------------------------------------------------------------------
# a VAE graph: encoders -> mean-fusion -> reparameterise -> decoders
# --------------------------------------------------------------------------------------------
class VAEGraph:
    """Compute graph shared by MultiModalVAE (vae.py:18-79), RNA2DNAVAE and DNA2RNAVAE
    (directional_vae.py:12-111): any subset of {MLP encoder a, MLP encoder b, embedding
    encoder}, mean fusion, reparameterisation, and a list of decoders."""

    def __init__(self, enc_a=None, enc_b=None, enc_c=None, decoders=()):
        self.enc_a, self.enc_b, self.enc_c = enc_a, enc_b, enc_c
        self.decoders = list(decoders)
        self.blocks = [b for b in (enc_a, enc_b, enc_c) if b is not None] + self.decoders
        self.latent = (enc_a or enc_b or enc_c).latent
        self._prep = PrepCache()
        self.dec_stem = None
        self.noise = GLOBAL_NOISE
        self.grad_sync = None          # mmvae.parallel.GradAllReduce (early/final hooks) under data parallelism
        # (Independent chains on side HIP streams -- EncoderA beside EncoderB, the small decoders beside DecoderB, the dW GEMMs beside
        # the dX chain, the noise launch beside the first GEMMs -- were measured slower every time the kernels got faster: overlapped
        # bandwidth-bound kernels only take turns and the fork / join edges cost more than they buy.  One stream.)
        # Training-step fusion (mmvae.graphs): [target or None per decoder].  The next forward then computes those decoders'
        # reconstruction losses inside their last GEMM instead of returning the reconstruction (see DecoderMLP.forward).
        self.fused_recon = None
        # Training-step fusion (mmvae.graphs): the caller hands the class logits straight to fused_loss and never reads them, so the
        # next forward may leave the class decoder's last Linear to the loss (ClassTail).  Off, the forward returns real logits.
        self.defer_class_head = False
        # Training-step fusion (mmvae.graphs): the caller reads the loss values only after the backward, so the loss may leave its
        # finalisation to the backward, whose last grouped dW launch carries it and EncoderC's backward as riders
        # (ops.gemm_tn_group).  Off, the loss finalises itself and EncoderC's backward is a launch of its own.
        self.tail_riders = False

    def _late_decoder_params(self):
        """Decoder tensors whose dW GEMM is small-output (latent / class widths: the decoders' first layers, DecoderC): they are
        computed by the grouped launch at the END of backward, so under data parallelism they travel with the encoder half of the
        gradient arena instead of forcing an early flush of that launch."""
        out = []
        for d in self.decoders:
            for l in d.linears:
                if l.weight.numel() <= _TINY_DW_MAX:
                    out += [l.weight, l.bias]
        return out

    def param_list(self):
        """Order of the flat gradient arena: encoders, the decoders' small-output tensors, then the large decoder tensors -- the tail
        (from early_cut() on) is final when the decoders' backward is done and is all-reduced under the encoder backward."""
        out = []
        for b in self.blocks:
            if b not in self.decoders:
                out += b.params()
        late = self._late_decoder_params()
        out += late
        ids = {id(p) for p in late}
        for d in self.decoders:
            out += [p for p in d.params() if id(p) not in ids]
        return out

    def early_cut(self):
        """Index into the arena where the early all-reduce bucket starts."""
        return sum(p.numel() for b in self.blocks if b not in self.decoders for p in b.params()) + sum(p.numel() for p in self._late_decoder_params())

    def _prepare(self, prec, device):
        """The PreparedLinears of every block (+ the merged first layers of the decoders): what the preparation cache refreshes."""
        pls = []
        for b in self.blocks:
            pls += b.prepare(prec, device)
        # The first layers of all decoders read the same z (K = latent: one K step): ONE GEMM with their weights concatenated
        # along N instead of one latency-bound launch per decoder, and ONE dX GEMM (K = sum of their widths) for dL/dz in
        # backward.  Each decoder continues from / writes into its column slice (widths must keep the slices 16-byte aligned).
        self.dec_stem = None
        decs = self.decoders
        if (len(decs) >= 2 and all(isinstance(d, DecoderMLP) and len(d.linears) >= 2 for d in decs)
                and all(d.linears[0].in_features == decs[0].linears[0].in_features and d.linears[0].out_features % 8 == 0 for d in decs)):
            self.dec_stem = ops.PreparedLinear([d.linears[0].weight for d in decs], [d.linears[0].bias for d in decs], prec, device)
            pls.append(self.dec_stem)
        return pls

    def zero_pack(self, device, has_a, has_b, has_site, fwd, bwd, fill=True):
        """ONE memset for what a step with these modalities needs zeroed -> StepZeros.  fwd: the forward BatchNorm sums (training);
        bwd: the flat gradient arena, the backward's BatchNorm sums and the embedding-table gradient; both: the loss accumulators
        too (three fills before).  The half that was not asked for is empty / None.  fill=False: allocated only; the caller
        zeroes StepZeros.unfilled (the head-of-step launch does)."""
        widths = (self.enc_a.widths() if has_a else []) + (self.enc_b.widths() if has_b else [])
        n_sums = 2 * sum(widths)                       # every layer's (2, width) float64 sums are a multiple of 16 bytes: no gaps
        n_sites = self.enc_c.embedding.weight.shape[0] if has_site else 0
        tab_w = self.enc_c.table_width * self.latent if has_site else 0
        n_tab = n_sites * tab_w * L_.TABLE_COPIES
        both = fwd and bwd
        packed = zeros_pack(device, [
            (n_sums if fwd else 0, torch.float64),
            (5 if both else 0, torch.float64),
            (5 if both else 0, torch.float32),
            (sum(p.numel() for p in self.param_list()) if bwd else 0, torch.float32),
            (n_sums if bwd else 0, torch.float64),
            (max(n_tab, 1) if bwd else 0, torch.float32)], fill)
        (fwd_sums, loss_sums, loss_out5, arena, bwd_sums, d_table), unfilled = packed if not fill else (packed, None)

        def per_layer(sums):
            return [t.view(2, -1) for t in sums.split([2 * w for w in widths])]
        return StepZeros(fwd_stats=per_layer(fwd_sums) if fwd else [],
                         loss_ws=(loss_sums, loss_out5) if both else None,
                         arena=arena if bwd else None,
                         bwd_stats=per_layer(bwd_sums) if bwd else [],
                         d_table=d_table[:n_tab].view(-1, n_sites, tab_w) if bwd and has_site else None,
                         unfilled=unfilled)

    def forward(self, prec, xa, xb, site, train, want_bwd=False):
        """Returns (outs(list, fp32), mu, logvar, state); an AEGraph (outs, latent, state).  want_bwd: a backward will follow (training only) -- decided by the caller
        (functional.run_graph) BEFORE it enters the autograd.Function, inside which grad mode is always off."""
        ref = xa if xa is not None else (xb if xb is not None else site)
        if not ref.is_cuda or any(p.device != ref.device for p in self.param_list()):
            raise RuntimeError(f"the MI355X path needs inputs and parameters on one CUDA/HIP device (input on {ref.device}); "
                               "there is no CPU fallback")
        with ops.pinned_stream():
            return self._forward(prec, xa, xb, site, train, train and want_bwd)

    def _head_of_step(self, prec, dev, B, has_a, has_b, has_site, train, want_bwd, eps_width, table_args):
        """What a forward begins with -> (masks, eps, zeros, n_a, whether the head launch ran -- it then made the table of table_args).
        eps_width: the latent width eps is drawn for; None: masks only (AEGraph)."""
        widths_a = self.enc_a.widths() if (train and has_a) else []
        widths_b = self.enc_b.widths() if (train and has_b) else []
        # A training forward begins with four launches that depend on nothing of the step -- the weight preparation, the Philox
        # noise, the step's one memset and EncoderC's table -- of which only the noise has real work: ONE launch
        # (ops.step_head), its arguments collected here.  The weights are prepared at the HEAD of every step, from the masters as
        # they are then: a caller may rewrite parameters in place between two replays of a captured step (a checkpoint restore).
        prep = self._prep.ensure(prec, dev, self.param_list(), self._prepare, run=False)
        masks, eps, noise_launch = self.noise.plan(B, widths_a + widths_b, eps_width, dev)       # eps is sampled in eval mode too (vae.py:73)
        # (Only an AEGraph gets here with neither masks nor eps -- eval mode, or no encoder: nothing is drawn.  A VAEGraph always draws
        # eps, eps_width is its latent width, so this branch changes no launch of it.)
        if eps_width is None and noise_launch is not None and noise_launch[0] is None:
            noise_launch = None
        head = train and noise_launch is not None      # eval mode, injected noise: the launches as they were
        # ONE fill for everything this step needs zeroed: forward BatchNorm sums, the loss accumulators, and -- when a backward will
        # follow -- the flat gradient arena with the backward's BatchNorm sums and embedding-table gradient (three fills before)
        zeros = self.zero_pack(dev, has_a, has_b, has_site, fwd=True, bwd=want_bwd, fill=not head) if train else None
        if head:
            try:
                ops.step_head(noise_launch, prep, [zeros.unfilled], table_args)
            except L_.MMVAEArgError:                   # refused before anything was enqueued: the four launches, as before
                head = False
        if not head:
            if prep is not None:
                prep.run()
            if noise_launch is not None:
                ops.noise(*noise_launch)
            if zeros is not None and zeros.unfilled is not None:
                zeros.unfilled.zero_()
        if zeros is not None:
            zeros.unfilled = None
        return masks, eps, zeros, len(widths_a), head

    draws_eps = True                   # the head of the step draws eps of the latent width (an AEGraph: dropout masks only)
    flatten_a = False                  # input a is taken as given; b is always flattened (encoders.py:44 view)

    def _forward(self, prec, xa, xb, site, train, want_bwd):
        """The step up to the latent stage, that stage (_latent_forward, the one part a subclass replaces), the decoders.
        Returns (outs, *latent tensors, state)."""
        for x, enc in ((xa, self.enc_a), (xb, self.enc_b)):
            if x is not None and enc is None:
                raise RuntimeError(f"{type(self).__name__}: this graph has no encoder for that input")
        ref = xa if xa is not None else (xb if xb is not None else site)
        dev, B = ref.device, ref.shape[0]
        state = StepState(prec, B, train, tail_riders=self.tail_riders and want_bwd)
        enc_out = [None, None]                         # per MLP encoder: its heads, or the ops.LatentEncoder it stopped at
        table = None
        # a two-head table is handed to the head launch; a one-head table is a launch of its own behind the encoders
        table_args = self.enc_c.table_args() if (site is not None and self.enc_c.rides) else None
        masks, eps, zeros, n_a, head = self._head_of_step(prec, dev, B, xa is not None, xb is not None, site is not None, train, want_bwd,
                                                          self.latent if self.draws_eps else None, table_args)
        if head and table_args is not None:
            table = table_args[-1]
        if want_bwd:
            state.zeros = zeros
        # Where the latent stage is ONE launch the encoders stop before their heads; where the library does not take it, the launches it
        # replaces run inside the stage.  The refusal is only known once both encoders have run, so that fallback issues
        # [A layers, B layers, A heads, B heads, fusion, stems] where graphs without a fused stage issue [A layers, A heads, B layers,
        # B heads, ...]: the same launches on the same operands with the same results, EncoderA's last pre-BatchNorm output is simply read later.
        fuse_latent = self._fuses_latent(prec)
        if xa is not None:
            xa = _check_input(xa.reshape(xa.shape[0], -1) if self.flatten_a else xa, "a", self.enc_a.in_dim, prec)
            enc_out[0], state.enc_a = self.enc_a.forward(prec, xa, train, masks[:n_a] if train else None,
                                                         zeros.fwd_stats[:n_a] if train else None, want_bwd=want_bwd, heads=not fuse_latent)
        if xb is not None:
            xb = _check_input(xb.reshape(xb.shape[0], -1), "b", self.enc_b.in_dim, prec)     # encoders.py:44 view
            enc_out[1], state.enc_b = self.enc_b.forward(prec, xb, train, masks[n_a:] if train else None,
                                                         zeros.fwd_stats[n_a:] if train else None, want_bwd=want_bwd, heads=not fuse_latent)
        if site is not None:
            if site.dtype != torch.int64:
                site = site.long()
            site = state.site = site.contiguous()
            if table is None:                          # not made by the head launch
                table = self.enc_c.table(table_args)
        state.eps = eps
        state.n_mod = (xa is not None) + (xb is not None) + (table is not None)
        latents, z, H0, stem_done, first0 = self._latent_forward(prec, B, dev, enc_out, table, site, eps, fuse_latent, state)
        return (self._decode(prec, B, dev, z, H0, stem_done, state, zeros, want_bwd, site, first0=first0), *latents, state)

    def _fuses_latent(self, prec):
        """Whether the latent stage is tried as one launch (the encoders then stop before their heads)."""
        return self.dec_stem is not None and prec == PREC_BF16

    def _latent_forward(self, prec, B, dev, enc_out, table, site, eps, fused, state):
        """Heads, mean fusion, reparameterisation and the decoders' stems -> ((mu, logvar), z, and _decode's H0, stem_done, first0).
        enc_out: per MLP encoder its heads, or (fused) the LatentEncoder it stopped at: ONE launch (mmvae_latent_fwd) with merged decoder
        first layers in bf16 mode."""
        Ld, stem = self.latent, self.dec_stem
        heads_a, heads_b = enc_out
        mu = torch.empty(B, Ld, dtype=torch.float32, device=dev)
        logvar = torch.empty(B, Ld, dtype=torch.float32, device=dev)
        z = torch.empty(B, ceil_to(Ld, 8), dtype=act_dtype(prec), device=dev)
        H0 = torch.empty(B, stem.N, dtype=act_dtype(prec), device=dev) if stem is not None else None
        if fused:
            try:
                ops.latent_fwd(prec, B, Ld, heads_a, heads_b, table, site, eps, mu, logvar, z, stem, H0)
            except L_.MMVAEArgError:                   # refused before anything was enqueued
                fused = False
                heads_a = self.enc_a.run_heads(prec, heads_a) if heads_a is not None else None
                heads_b = self.enc_b.run_heads(prec, heads_b) if heads_b is not None else None
        if not fused:
            ops.fuse_reparam_fwd(B, Ld, heads_a, heads_b, table, site, eps, mu, logvar, z)
        # .detach(): an alias of the RETURNED tensor, so the saved state holds no reference to objects that own the
        # autograd node (tensor -> grad_fn -> ctx -> state -> tensor would be a cycle only the cyclic GC frees,
        # i.e. every step's activations would pile up in HBM until it runs)
        state.logvar = logvar.detach()
        return (mu, logvar), z, H0, fused, None

    def _decode(self, prec, B, dev, z, H0, stem_done, state, zeros, want_bwd, site, first0=None):
        """The decoders on z -> their outputs; fills state.dec / fused / class_tail.  H0: the merged first layers' output buffer (None
        without a stem), already computed when stem_done.  first0: the first decoder's layer-0 output, computed elsewhere (AEGraph)."""
        stem = self.dec_stem
        outs, state.dec = [None] * len(self.decoders), [None] * len(self.decoders)
        order = sorted(range(len(self.decoders)), key=lambda i: -sum(l.weight.numel() for l in self.decoders[i].linears))
        firsts = [None] * len(self.decoders)
        firsts[0] = first0
        if stem is not None:
            if not stem_done:
                ops.gemm_nt(prec, z, stem.w, stem.N, stem.K, H0, bias=stem.bias, act=ACT_RELU, tag="Decoders.L0.fwd")
            off = 0
            for i, d in enumerate(self.decoders):
                firsts[i] = H0[:, off:off + d.linears[0].out_features]
                off += d.linears[0].out_features
        fused = None
        want = self.fused_recon
        if want is not None and any(t is not None and self.decoders[i].can_fuse_loss(prec) for i, t in enumerate(want)):
            fused = state.fused = FusedRecon(*(zeros.loss_ws if want_bwd else ops.loss_workspace(dev)), {}, {})
        tail_i = self._class_tail_index(prec, H0, want, site) if (self.defer_class_head and fused is not None and want_bwd) else None
        for i in order:                                 # largest decoder first
            dec = self.decoders[i]
            tgt = want[i] if (fused is not None and want[i] is not None and dec.can_fuse_loss(prec)) else None
            if i == tail_i:
                # the class head: its last Linear runs inside the loss (mmvae_class_tail), which also leaves the gradient w.r.t. this
                # decoder's hidden activation in D0 -- allocated here, with the step state, because the loss writes it
                D0 = torch.empty(B, stem.N, dtype=act_dtype(prec), device=dev)
                off = sum(d.linears[0].out_features for d in self.decoders[:i])
                state.class_tail = ClassTail(i, dec.pl[1], firsts[i], D0, D0[:, off:off + dec.linears[0].out_features], dec.name)
                o = torch.empty(1, dtype=torch.float32, device=dev).expand(B, dec.out_dim)     # placeholder: no storage behind it
                acts = [z, firsts[i]]
            elif tgt is not None:
                k = 1 if dec.final_sigmoid else 0                     # sums[0] = MSE, sums[1] = BCE (mmvae_vae_loss)
                g, acts = dec.forward(prec, z, fused_loss=(tgt, fused.sums[k:k + 1]), first=firsts[i])
                fused.g[i], fused.targets[i] = g, tgt
                o = torch.empty(1, dtype=torch.float32, device=dev).expand(B, dec.out_dim)     # placeholder: no storage behind it
            else:
                o, acts = dec.forward(prec, z, first=firsts[i])
            outs[i] = o
            state.dec[i] = (acts, o.detach())
        return outs

    def _class_tail_index(self, prec, H0, want, site):
        """The decoder whose last Linear the fused class-head launch can take over, or None: the training step asked for it
        (defer_class_head) and computes its reconstruction losses inside the decoder GEMMs (the caller checked both), labels are given, the stems are merged, and one decoder
        without a reconstruction target is Linear -> ReLU -> Linear within the library's limits (asked, not duplicated here)."""
        if self.dec_stem is None or site is None or H0 is None:
            return None
        for i, dec in enumerate(self.decoders):
            if want[i] is None and isinstance(dec, DecoderMLP) and len(dec.pl) == 2 and not dec.final_sigmoid \
                    and ops.class_tail_fits(prec, dec.pl[1].N, dec.pl[1].K, self.latent, H0.stride(0), H0.stride(0)):
                return i
        return None

    def backward(self, state, g_outs, g_logit_flags, g_mu, g_lv):
        with ops.pinned_stream():
            return self._backward(state, g_outs, g_logit_flags, g_mu, g_lv)

    def _backward(self, state, g_outs, g_logit_flags, g_mu, g_lv):
        """g_outs[i]: gradient w.r.t. decoder i's output or None; g_mu/g_lv fp32 [B][L] or None.
        Returns (flat_arena, {param: grad view})."""
        prec, B = state.prec, state.B
        site = state.site
        dev = state.dec[0][1].device
        Ld = self.latent
        zeros, state.zeros = state.zeros, None         # zeroed by the forward's one memset; else (eval-mode forward, no want_bwd) here
        if zeros is None:
            zeros = self.zero_pack(dev, state.enc_a is not None, state.enc_b is not None, site is not None, fwd=False, bwd=True)
        flat = zeros.arena
        grads = carve_arena(flat, self.param_list())
        n_a = len(state.enc_a) if state.enc_a is not None else 0
        dzs = []                                       # one dL/dz per decoder; summed in mmvae_fuse_reparam_bwd
        # slab workspace for the split-batch dW GEMMs (<= 64 splits of the largest weight matrix); launches that use it
        # run one after another on one stream, so a single buffer serves them all
        big = max(p.numel() for p in self.param_list())
        slab = torch.empty(min(64 * big, 1 << 25), dtype=torch.float32, device=dev)     # <= 128 MiB; too small -> that GEMM uses atomics

        # Small-output dW GEMMs (latent / class widths: encoder heads, decoder first layers, DecoderC) are latency chains when
        # launched alone (~25 us each for a few MB + a reduce launch): they are DEFERRED and run as one grouped launch + one
        # reduce per flush -- after the decoders (their gradients are then final for the early all-reduce bucket) and at the end.
        tiny = []

        def tn(prec_, p, q, dw, db, N, K, q_prologue=None, p_prologue=None, tag=None):
            if p_prologue is None and N * K <= _TINY_DW_MAX:
                tiny.append(dict(p=p, q=q, dw=dw, db=db, N=N, K=K, q_prologue=q_prologue))
                return
            ops.gemm_tn(prec_, p, q, dw, db, N, K, q_prologue=q_prologue, p_prologue=p_prologue, slab=slab, tag=tag)

        def flush_tiny(tag, riders=None):
            """-> whether `riders` rode in the grouped launch."""
            rode = False
            if tiny:
                need = ops.TN_GROUP_SPLITS * sum(t_["N"] * t_["K"] for t_ in tiny)
                rode = ops.gemm_tn_group(prec, tiny, torch.empty(need, dtype=torch.float32, device=dev), tag=tag, riders=riders)
                tiny.clear()
            return rode
        stem = self.dec_stem if all(g is not None for g in g_outs) else None      # every decoder must fill its slice
        D0, off = None, 0
        tail = state.class_tail
        if stem is not None:
            D0 = tail.d0 if tail is not None else torch.empty(B, stem.N, dtype=act_dtype(prec), device=dev)
        for i, (dec, (acts, out), g, is_logit) in enumerate(zip(self.decoders, state.dec, g_outs, g_logit_flags)):
            n0 = dec.linears[0].out_features if stem is not None else 0
            if g is None:
                off += n0
                continue
            # the fused class-head launch has already left this decoder's hidden-activation gradient in its columns of D0
            dx_done = tail.d0_slice if (tail is not None and tail.index == i and tail.done) else None
            if stem is not None:
                dec.backward(prec, acts, out, g, is_logit, None, grads, tn, d0_out=D0[:, off:off + n0], dx_done=dx_done)
                off += n0
                continue
            dz = torch.empty(B, Ld, dtype=torch.float32, device=dev)
            dec.backward(prec, acts, out, g, is_logit, dz, grads, tn, dx_done=dx_done)
            dzs.append(dz)
        if stem is not None:
            dz = torch.empty(B, Ld, dtype=torch.float32, device=dev)
            ops.gemm_nt(prec, D0, stem.wt, stem.K, stem.N, dz, tag="Decoders.L0.dX")
            dzs.append(dz)
        if not dzs:
            dzs.append(torch.zeros(B, Ld, dtype=torch.float32, device=dev))
        if self.grad_sync is not None:
            # the large decoder gradients (tail of the arena) are final: start reducing them under the encoder backward.  The decoders'
            # small-output tensors sit in front of the cut: their grouped dW launch stays ONE launch at the end of backward, as on one GPU
            # (round 3; before, data parallelism flushed that launch here: an extra grouped GEMM + reduce per step).
            self.grad_sync.early(flat, self.early_cut())
        d_heads, d_heads_lp = self._fusion_backward(state, zeros, dzs, g_mu, g_lv, dev)
        if state.enc_a is not None:
            self.enc_a.backward(prec, state.enc_a, d_heads, grads, tn, zeros.bwd_stats[:n_a], train=state.train, d_heads_lp=d_heads_lp)
        if state.enc_b is not None:
            self.enc_b.backward(prec, state.enc_b, d_heads, grads, tn, zeros.bwd_stats[n_a:], train=state.train, d_heads_lp=d_heads_lp)
        # EncoderC's backward (it reads the table gradient the fusion backward scattered, and writes EncoderC's gradients only) and
        # the loss finalisation the loss left behind have nothing to do with the grouped dW launch that ends the backward: with
        # tail_riders they run as extra workgroups of it.  Without, where there is no such launch, or where the library refuses
        # (nothing enqueued), they are the launches of their own they were.
        # (A one-head EmbedEncoder's backward does not ride: the rider role is EncoderC's two-head table; it is always its own launch.)
        embed_bwd = self.enc_c.backward_args(zeros.d_table, grads) if site is not None else None
        ride_embed = embed_bwd if (embed_bwd is not None and self.enc_c.rides) else None
        loss_tail, state.loss_tail = state.loss_tail, None
        riders = ops.tn_riders(ride_embed, loss_tail) if (state.tail_riders and (ride_embed is not None or loss_tail is not None)) else None
        if embed_bwd is not None and (riders is None or ride_embed is None):
            self.enc_c.launch_backward(*embed_bwd)
        rode = flush_tiny("tiny_dW.heads", riders)
        if riders is not None and not rode:
            if ride_embed is not None:
                self.enc_c.launch_backward(*ride_embed)
            if loss_tail is not None:
                ops.loss_finalize(*loss_tail)
        elif riders is None and loss_tail is not None:
            ops.loss_finalize(*loss_tail)
        if self.grad_sync is not None:
            self.grad_sync.final(flat)
        return flat, grads

    def _fusion_backward(self, state, zeros, dzs, g_mu, g_lv, dev):
        """Backward of the mean fusion + reparameterisation -> (d_heads fp32 (B, 2L), its bf16 copy or None); scatters into zeros.d_table."""
        prec, B, Ld = state.prec, state.B, self.latent
        d_heads = torch.empty(B, 2 * Ld, dtype=torch.float32, device=dev)
        # bf16 mode: a bf16 copy of d_heads for the heads' dX GEMMs (they round it on load anyway; plain bf16 A -> LDS-DMA kernel)
        d_heads_lp = torch.empty(B, ceil_to(2 * Ld, 8), dtype=torch.bfloat16, device=dev) if prec == PREC_BF16 else None
        ops.fuse_reparam_bwd(B, Ld, state.n_mod, g_mu, g_lv, dzs, state.eps, state.logvar, d_heads, zeros.d_table, state.site, d_heads_lp=d_heads_lp)
        return d_heads, d_heads_lp


# --------------------------------------------------------------------------------------------
# an autoencoder graph: one single-head encoder and / or the projected site embedding -> plain mean -> one decoder
# --------------------------------------------------------------------------------------------
class AEGraph(VAEGraph):
    """Compute graph of RNA2DNAAE / DNA2RNAAE (reference src/models/directional_ae.py:10-134): a single-head MLP encoder (in slot a for
    RNA, slot b for DNA), the site through a one-head EmbedEncoder, the plain mean of the latents present, one decoder.  No eps is drawn,
    no logvar exists, nothing of a KL term: forward returns (outs, latent, state).  Everything else -- the head of the step, the one
    memset, the decoders, fused_recon, tail_riders, the gradient arena, grad_sync -- is VAEGraph's."""

    def __init__(self, enc_a=None, enc_b=None, site=None, decoder=None):
        if (enc_a is None) == (enc_b is None) or site is None or decoder is None:
            raise ValueError("AEGraph: exactly one MLP encoder, the projected site embedding and one decoder")
        if (enc_a or enc_b).fc_logvar is not None or site.fc_logvar is not None:
            raise ValueError("AEGraph: the encoder and the site embedding must be in their single-head form")
        super().__init__(enc_a=enc_a, enc_b=enc_b, enc_c=site, decoders=[decoder])

    # masks only: the Philox offset advances by exactly the mask draw, and not at all in eval mode
    draws_eps = False
    flatten_a = True                   # directional_ae.py flattens whichever input it encodes

    def _fuses_latent(self, prec):
        dec = self.decoders[0]
        return prec == PREC_BF16 and isinstance(dec, DecoderMLP) and len(dec.linears) >= 2

    def _latent_forward(self, prec, B, dev, enc_out, table, site, eps, fused, state):
        """Head, plain mean with the site's table row and the decoder's first layer -> ((latent,), z, and _decode's H0, stem_done,
        first0).  In bf16 mode ONE launch (mmvae_ae_latent_fwd) on the LatentEncoder the encoder stopped at; where the library does not
        take it, the three launches it replaces."""
        Ld, dec = self.latent, self.decoders[0]
        enc, head = (self.enc_a, enc_out[0]) if enc_out[0] is not None else (self.enc_b, enc_out[1])
        latent = torch.empty(B, Ld, dtype=torch.float32, device=dev)
        z = torch.empty(B, ceil_to(Ld, 8), dtype=act_dtype(prec), device=dev)
        first = None
        if fused:
            pl0 = dec.pl[0]
            first = torch.empty(B, ceil_to(pl0.N, 8), dtype=act_dtype(prec), device=dev)
            try:
                ops.ae_latent_fwd(prec, B, Ld, head, table, site, latent, z, pl0, first)
            except L_.MMVAEArgError:                   # refused before anything was enqueued
                fused, first = False, None
                head = enc.run_heads(prec, head) if head is not None else None
        if not fused:
            ops.fuse_mean_fwd(B, Ld, head, table, site, latent, z)
        return (latent,), z, None, False, first

    def _backward(self, state, g_outs, g_logit_flags, g_latent, g_lv=None):
        return super()._backward(state, g_outs, g_logit_flags, g_latent, None)

    def _fusion_backward(self, state, zeros, dzs, g_latent, g_lv, dev):
        """Backward of the plain mean -> (d_head fp32 (B, L), its bf16 copy or None); scatters into zeros.d_table (copies, S, L)."""
        prec, B, Ld = state.prec, state.B, self.latent
        d_head = torch.empty(B, Ld, dtype=torch.float32, device=dev)
        d_head_lp = torch.empty(B, ceil_to(Ld, 8), dtype=torch.bfloat16, device=dev) if prec == PREC_BF16 else None
        ops.fuse_mean_bwd(B, Ld, state.n_mod, dzs[0], g_latent, d_head, zeros.d_table, state.site, d_head_lp=d_head_lp)
        return d_head, d_head_lp
