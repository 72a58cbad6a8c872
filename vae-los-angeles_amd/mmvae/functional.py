"""torch.autograd bridges: the reference's callers drive training through
`loss.backward()` and `optimizer.step()` (optimize_hyperparameters.py:111-113), so the HIP
launch sequences of `engine.VAEGraph` sit behind `torch.autograd.Function`s.

Two gradient hand-offs exist between the loss and the model:
  * general: any loss may be applied to the model outputs; fp32 gradients arrive through
    autograd and are consumed directly by the backward GEMMs (converted on the fly).
  * fused (what `src.utils.losses.vae_loss` uses when it is given the outputs of one forward
    of our own model): the loss kernel already writes activation-typed gradients
    (w.r.t. the pre-sigmoid logits for DecoderB) into buffers owned by that forward's
    `engine.StepState` (its `loss_grads`, an `engine.LossGrads`); autograd then only carries
    `None`s plus the scalar grad_output, and no fp32 gradient of the size of the
    reconstructions is ever materialised.

The loss finds the forward through the `OutTag` that `run_graph` leaves on every tensor it returns.
"""
from typing import NamedTuple

import torch
from torch.autograd.function import once_differentiable

from . import engine, ops
from .ops import ceil_to, act_dtype


class VAEGraphFn(torch.autograd.Function):
    """One forward of an engine.VAEGraph or AEGraph.  Whatever graph.forward returns between the decoders' outputs and the state are
    the latent outputs -- (mu, logvar), or an AEGraph's (latent,) -- and as many gradients go to the graph's backward."""

    @staticmethod
    def forward(ctx, graph, prec, train, want_bwd, xa, xb, site, *params):
        ctx.set_materialize_grads(False)
        outs, *latents, state = graph.forward(prec, xa, xb, site, train, want_bwd)
        ctx.graph, ctx.saved, ctx.n_out = graph, state, len(outs)
        graph._last_saved = state
        return (*outs, *latents)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        graph, state, n_out = ctx.graph, ctx.saved, ctx.n_out
        if state.consumed:
            raise RuntimeError("backward through this forward was already run (buffers are not retained)")
        g_outs = [None if g is None else _as_rows(g) for g in gs[:n_out]]
        g_lat = [None if g is None else g.contiguous().float() for g in gs[n_out:]] + [None]      # g_lv: None behind an AEGraph's one latent
        return (None, None, None, None, None, None, None, *_graph_backward(graph, state, g_outs, g_lat[0], g_lat[1]))


def _graph_backward(graph, state, g_outs, g_mu, g_lv):
    """The backward of one forward of a VAEGraph / AEGraph (g_mu: the gradient at mu, or at the AEGraph's latent; g_lv None there),
    with the gradients the fused loss stashed -> the parameters' gradients in param_list() order (None: did not take part)."""
    flags = [False] * len(g_outs)
    lg = state.loss_grads
    if lg is not None and lg.armed:                              # the loss handle's backward ran: its gradients are the ones to use
        if lg.scale is not None:                                 # None: unit_grad promised by the caller (fused_loss)
            ops.scale_many(list(lg.g_outs) + [lg.g_mu, lg.g_lv], lg.scale)       # one launch, not five
        for i, sg in enumerate(lg.g_outs):
            if sg is None:
                continue
            if g_outs[i] is not None:            # rare: another loss term also touched this output
                sg[:, :g_outs[i].shape[1]] += _to_stash_space(g_outs[i], state.dec[i][1], graph.decoders[i], sg.dtype)
            g_outs[i], flags[i] = sg, graph.decoders[i].final_sigmoid
        if lg.g_mu is not None:                  # None: an AEGraph's forward -- the loss has no term on the latent
            for sg, cur in ((lg.g_mu, g_mu), (lg.g_lv, g_lv)):
                if cur is not None:
                    sg += cur
            g_mu, g_lv = lg.g_mu, lg.g_lv
    flat, grads = graph.backward(state, g_outs, flags, g_mu, g_lv)
    state.consumed = True
    used = _participating(graph, state, g_outs)
    out = [grads[p] if id(p) in used else None for p in graph.param_list()]
    del grads                                     # keep the views unique so autograd can adopt them
    return out


def _as_rows(g):
    if g.dtype not in (torch.float32, torch.bfloat16):
        g = g.float()
    if g.dim() != 2 or g.stride(1) != 1 or (g.shape[0] > 1 and g.stride(0) < g.shape[1]):
        g = g.contiguous()
    return g


def _to_stash_space(g, out, dec, dtype):
    if dec.final_sigmoid:
        g = g * out * (1.0 - out)
    return g.to(dtype)


def _participating(graph, state, g_outs):
    """ids of the parameters of the blocks that took part: the encoders that ran and the decoders a gradient arrived for."""
    blocks = [b for b, ran in ((graph.enc_a, state.enc_a), (graph.enc_b, state.enc_b), (graph.enc_c, state.site)) if ran is not None]
    blocks += [dec for dec, g in zip(graph.decoders, g_outs) if g is not None]
    return {id(p) for b in blocks for p in b.params()}


class OutTag(NamedTuple):
    """Marks a tensor that run_graph returned (`t._mmvae`): the forward that made it and which of its outputs it is."""
    state: engine.StepState
    kind: str                       # "out" (a decoder's output) | "mu" | "logvar" | "latent" (an AEGraph's)
    index: int                      # the decoder, for "out"


def _run(graph, prec, train, xa, xb, site, kinds):
    """Forward of a graph with autograd wiring -> (outs, *latent outputs); kinds: the OutTag kind of each latent output."""
    params = graph.param_list()
    # a backward will follow: the forward's ONE memset then also zeroes the gradient arena, the backward's BatchNorm sums, the table
    # gradient and the loss accumulators (3 fill launches per step -> 1)
    want_bwd = train and torch.is_grad_enabled() and any(p.requires_grad for p in params)
    res = VAEGraphFn.apply(graph, prec, train, want_bwd, xa, xb, site, *params)
    n = len(graph.decoders)
    outs, latents = list(res[:n]), res[n:]
    state = graph._last_saved
    graph._last_saved = None
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        for i, o in enumerate(outs):
            o._mmvae = OutTag(state, "out", i)
        for t, kind in zip(latents, kinds):
            t._mmvae = OutTag(state, kind, 0)
    return (outs, *latents)


def run_graph(graph, prec, train, xa, xb, site):
    """Forward of a VAEGraph with autograd wiring.  Returns (outs, mu, logvar)."""
    return _run(graph, prec, train, xa, xb, site, ("mu", "logvar"))


def run_ae_graph(graph, prec, train, x_a, x_b, site):
    """Forward of an engine.AEGraph with autograd wiring (x_a: RNA for a graph with an RNA encoder, x_b: DNA for one with a DNA
    encoder; either and the site may be None).  Returns (outs, latent)."""
    return _run(graph, prec, train, x_a, x_b, site, ("latent",))


# --------------------------------------------------------------------------------------------
# loss
# --------------------------------------------------------------------------------------------
class _LossHandleFn(torch.autograd.Function):
    """Connects the fused loss value to the model's autograd node; gradients travel through the
    forward's LossGrads (see module docstring), autograd only delivers grad_output."""

    @staticmethod
    def forward(ctx, total, loss_grads, *model_outputs):
        ctx.loss_grads = loss_grads
        ctx.n_outputs = len(model_outputs)
        return total.view(())            # a view of the kernel's output buffer (not of an input that requires grad): no copy launch

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.loss_grads.unit_grad:
            ctx.loss_grads.scale = g.reshape(1).float().contiguous()
        ctx.loss_grads.armed = True
        return (None,) * (2 + ctx.n_outputs)


class _LossGeneralFn(torch.autograd.Function):
    """Fused loss for arbitrary inputs: fp32 gradients are produced by the same kernel pass and
    handed to autograd."""

    @staticmethod
    def forward(ctx, spec, *tensors):
        ctx.set_materialize_grads(False)
        total, grads = spec(tensors)
        ctx.grads = grads
        return total

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        scale = g.reshape(1).float().contiguous()
        out = []
        for t in ctx.grads:
            if t is not None:
                ops.scale_if_needed(t, scale)
            out.append(t)
        return (None, *out)


def _tag_of(t):
    return getattr(t, "_mmvae", None) if t is not None else None


def fused_loss(terms, beta, gamma, class_weights=None, unit_grad=False, beta_gamma_dev=None):
    """unit_grad=True: the caller promises to call `total.backward()` with the default gradient of 1 (a captured training step
    does): the stashed gradients are then used as they are, without the launch that multiplies them by the incoming gradient.
    beta_gamma_dev: device float32[2] overriding (beta, gamma): a captured step follows the beta warm-up without re-capture."""
    if not next(v[0] for v in terms.values() if v is not None).is_cuda:
        raise RuntimeError("the MI355X loss kernel needs CUDA/HIP tensors; there is no CPU fallback")
    with ops.pinned_stream():
        return _fused_loss(terms, beta, gamma, class_weights, unit_grad, beta_gamma_dev)


def _validate_loss_args(dev, B, ra, a, rb, b, lg, site, mu, lv, class_weights):
    """The kernel takes raw pointers: everything torch's own losses would reject (F.mse_loss / binary_cross_entropy /
    cross_entropy on mismatched devices or shapes, losses.py:31,34,39) is rejected here, before any launch."""
    for nm, pred, tgt in (("a", ra, a), ("b", rb, b), ("logvar", mu, lv)):
        if pred is None:
            continue
        if tgt.device != pred.device or pred.device != dev:
            raise RuntimeError(f"vae_loss: '{nm}' tensors are on different devices ({pred.device} vs {tgt.device}); "
                               "the MI355X loss kernel needs all of them on one CUDA/HIP device")
        if pred.dim() != 2 or tuple(tgt.shape) != tuple(pred.shape) or pred.shape[0] != B:
            raise RuntimeError(f"vae_loss: shape mismatch for '{nm}': prediction {tuple(pred.shape)} vs target {tuple(tgt.shape)} (batch {B})")
    if lg is not None:
        if site.device != dev or lg.device != dev:
            raise RuntimeError(f"vae_loss: site labels / logits are on another device ({site.device}, {lg.device}) than {dev}")
        if lg.dim() != 2 or lg.shape[0] != B or site.dim() != 1 or site.shape[0] != B:
            raise RuntimeError(f"vae_loss: site must have shape ({B},) for logits {tuple(lg.shape)}, got {tuple(site.shape)}")
        if site.dtype in (torch.float16, torch.float32, torch.float64, torch.bfloat16, torch.bool):
            raise RuntimeError(f"vae_loss: site labels must be integer class indices, got {site.dtype}")
        if class_weights is not None and class_weights.numel() != lg.shape[1]:
            raise RuntimeError(f"vae_loss: class_weights has {class_weights.numel()} entries for {lg.shape[1]} classes")


def _fused_loss(terms, beta, gamma, class_weights=None, unit_grad=False, beta_gamma_dev=None):
    """terms: dict with optional entries
         'a': (recon_a, a)  sum-MSE           'b': (recon_b, b)  sum-BCE (clamped logs)
         'c': (logits, site) weighted sum-CE  'kl': (mu, logvar)
    Returns (total (0-dim tensor, differentiable), out5 (device fp32 [total, recon, class, kld, labels out of range]))."""
    any_t = next(v[0] for v in terms.values() if v is not None)
    dev, B = any_t.device, any_t.shape[0]
    ra, a = terms.get("a") or (None, None)
    rb, b = terms.get("b") or (None, None)
    lg, site = terms.get("c") or (None, None)
    mu, lv = terms.get("kl") or (None, None)
    _validate_loss_args(dev, B, ra, a, rb, b, lg, site, mu, lv, class_weights)
    if site is not None and site.dtype != torch.int64:
        site = site.long()
    if site is not None:
        site = site.contiguous()
    cw = None if class_weights is None else class_weights.to(device=dev, dtype=torch.float32).contiguous()
    need_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (ra, rb, lg, mu, lv))

    # reconstruction terms whose loss already ran inside the decoder's last GEMM (engine.VAEGraph.fused_recon): the "reconstruction"
    # is a placeholder, its loss sum sits in the forward's accumulators and its gradient in the forward's saved state
    fused, fused_idx = None, {}
    placeholders = []                                  # the tensors that stand in for those reconstructions
    for key, (r, t) in (("a", (ra, a)), ("b", (rb, b))):
        tg = _tag_of(r)
        fr = tg.state.fused if tg is not None else None
        if fr is not None and tg.kind == "out" and tg.index in fr.g:
            if fr.targets[tg.index].data_ptr() != t.data_ptr() or tuple(fr.targets[tg.index].shape) != tuple(t.shape):
                raise RuntimeError("fused reconstruction loss: the target passed to the loss is not the tensor the forward was given")
            fused, fused_idx[key] = fr, tg.index
            placeholders.append(r)
    if fused is not None and not (torch.is_grad_enabled()):
        raise RuntimeError("fused reconstruction loss needs the training step (gradients enabled)")
    if "a" in fused_idx:
        ra = None
    if "b" in fused_idx:
        rb = None
    # the class head whose last Linear the forward left to this loss (engine.ClassTail): `lg` is a placeholder of the logits' shape
    tg = _tag_of(lg)
    tail = tg.state.class_tail if (tg is not None and tg.kind == "out") else None
    if tail is not None and (tail.index != tg.index or tail.done):
        tail = None
    lg_real = lg
    if tail is not None:
        lg = None                                      # nothing to read behind the placeholder: the logits are made below

    def prep(x):
        return None if x is None else (x if (x.dtype == torch.float32 and x.stride(-1) == 1) else x.float().contiguous())

    def prep_target(x):         # bf16 targets (bf16 storage) are read as they are: the kernel widens them on load
        return x if (x is not None and x.dtype == torch.bfloat16 and x.stride(-1) == 1) else prep(x)
    ra_, a_, rb_, b_, lg_, mu_, lv_ = (prep(ra), prep_target(a), prep(rb), prep_target(b), prep(lg), prep(mu), prep(lv))
    if mu_ is not None:
        mu_, lv_ = mu_.contiguous(), lv_.contiguous()
    if fused is not None:
        sums, out4 = fused.sums, fused.out5               # the decoders' GEMMs have already added their terms
    else:
        sums = out4 = None                                 # out4: [total, recon, class, kld, labels out of range]

    # ---- fused hand-off: all differentiable inputs are outputs of ONE forward of our model --------------------
    # (the placeholders count: an autoencoder's step has no other differentiable input once its one reconstruction term is fused)
    tags = [_tag_of(t) for t in (ra, rb, lg_real, mu, lv) if t is not None and t.requires_grad] + [_tag_of(t) for t in placeholders]
    state = tags[0].state if tags and all(t is not None and t.state is tags[0].state for t in tags) else None
    if need_grad and state is not None and not state.consumed and state.loss_grads is None:
        if sums is None:
            zeros = state.zeros
            if zeros is not None and zeros.loss_ws is not None:                    # zeroed by the forward's one memset; taken once
                (sums, out4), zeros.loss_ws = zeros.loss_ws, None
            else:
                sums, out4 = ops.loss_workspace(dev)
        adt = act_dtype(state.prec)
        g_outs = [None] * len(state.dec)
        for key, i in fused_idx.items():
            g_outs[i] = fused.g[i]
        ga = gb = gc = None
        if ra is not None and ra.requires_grad:
            ga = torch.empty(B, ceil_to(ra.shape[1], 8), dtype=adt, device=dev)
            g_outs[_tag_of(ra).index] = ga
        if rb is not None and rb.requires_grad:
            gb = torch.empty(B, ceil_to(rb.shape[1], 8), dtype=adt, device=dev)
            g_outs[_tag_of(rb).index] = gb
        if lg_real is not None and lg_real.requires_grad:
            gc = torch.empty(B, lg_real.shape[1], dtype=torch.float32, device=dev)
            g_outs[_tag_of(lg_real).index] = gc
        g_mu = torch.empty(B, mu.shape[1], dtype=torch.float32, device=dev) if mu is not None else None
        g_lv = torch.empty_like(g_mu) if mu is not None else None
        if tail is not None:
            # ONE launch for the class head: its Linear, the class + KL terms and the Linear's dX (mmvae_class_tail).  It takes the
            # captured step's form only (unit gradient: nothing rescales its dX afterwards; reconstruction terms inside the decoder
            # GEMMs); otherwise, or where the library refuses (nothing enqueued), the Linear runs here and the step goes on as before
            if unit_grad and ra_ is None and rb_ is None and mu_ is not None and gc is not None:
                try:
                    ops.class_tail(state.prec, B, tail.h0, tail.head, site, cw, mu_, lv_, beta, gamma, sums, gc, tail.d0_slice, g_mu, g_lv,
                                   beta_gamma_dev=beta_gamma_dev)
                    tail.done = True
                except ops.L.MMVAEArgError:
                    pass
            if not tail.done:
                lg_ = tail.logits(state.prec)
        if tail is None or not tail.done:
            ops.vae_loss(B, recon_a=ra_, a=a_, recon_b=rb_, b=b_, logits=lg_, site=site, class_weights=cw, mu=mu_, logvar=lv_,
                         beta=beta, gamma=gamma, sums=sums, g_a=ga, g_b=gb, grad_b_wrt_logit=True, g_c=gc, g_mu=g_mu, g_lv=g_lv,
                         beta_gamma_dev=beta_gamma_dev)
        if state.tail_riders and unit_grad:
            # the captured step reads out4 only after its backward: the finalisation rides in the backward's last launch
            # (engine.VAEGraph._backward), or is launched there; until then out4 holds nothing
            state.loss_tail = (sums, beta, gamma, out4, beta_gamma_dev)
        else:
            ops.loss_finalize(sums, beta, gamma, out4, beta_gamma_dev)
        if g_mu is None and state.logvar is not None:      # KL term absent: nothing flows into mu/logvar from this loss (an AEGraph has neither)
            g_mu = torch.zeros(B, state.logvar.shape[1], dtype=torch.float32, device=dev)
            g_lv = torch.zeros_like(g_mu)
        state.loss_grads = engine.LossGrads(g_outs=g_outs, g_mu=g_mu, g_lv=g_lv, unit_grad=bool(unit_grad))
        pads = [t for t in (ra, rb, lg_real, mu, lv) if t is not None] + placeholders
        total = _LossHandleFn.apply(out4[0], state.loss_grads, *pads)
        return total, out4

    if fused is not None:
        raise RuntimeError("fused reconstruction loss: the loss terms are not all outputs of the one forward that computed it")
    if tail is not None:
        raise RuntimeError("fused class head: the loss terms are not all outputs of the one forward that left its logits to the loss")

    # ---- general path --------------------------------------------------------------------------------------------
    if sums is None:
        sums, out4 = ops.loss_workspace(dev)

    def spec(tensors):
        ga = torch.empty_like(ra_) if (need_grad and ra is not None and ra.requires_grad) else None
        gb = torch.empty_like(rb_) if (need_grad and rb is not None and rb.requires_grad) else None
        gc = torch.empty_like(lg_) if (need_grad and lg is not None and lg.requires_grad) else None
        gm = torch.empty_like(mu_) if (need_grad and mu is not None and mu.requires_grad) else None
        gl = torch.empty_like(lv_) if (need_grad and lv is not None and lv.requires_grad) else None
        ops.vae_loss(B, recon_a=ra_, a=a_, recon_b=rb_, b=b_, logits=lg_, site=site, class_weights=cw, mu=mu_, logvar=lv_,
                     beta=beta, gamma=gamma, sums=sums, g_a=ga, g_b=gb, grad_b_wrt_logit=False, g_c=gc, g_mu=gm, g_lv=gl,
                     beta_gamma_dev=beta_gamma_dev)
        ops.loss_finalize(sums, beta, gamma, out4, beta_gamma_dev)
        grads = []
        for t, g in ((ra, ga), (rb, gb), (lg, gc), (mu, gm), (lv, gl)):
            if t is not None:
                grads.append(g)
        return out4[0].clone(), grads

    inputs = [t for t in (ra, rb, lg, mu, lv) if t is not None]
    total = _LossGeneralFn.apply(spec, *inputs)
    return total, out4


def read_losses(out5):
    """The ONE host read of the loss (the reference's three `.item()` calls, losses.py:46): [total, recon, class, kld] as
    floats.  Raises if the kernel met a class index outside [0, n_sites) (torch's cross_entropy device-asserts there)."""
    vals = out5.tolist()
    if vals[4] != 0.0:
        raise RuntimeError(f"vae_loss: {int(vals[4])} class index(es) in `site` outside [0, n_classes)")
    return vals[:4]


class ReparamFn(torch.autograd.Function):
    """Stand-alone reparameterize(mu, logvar) (reference src/models/vae.py:11-15) on the HIP kernels: the fused
    mean-fusion + reparameterisation launch with ONE modality; backward d_mu = g, d_logvar = g * eps * exp(logvar / 2) / 2."""

    @staticmethod
    def forward(ctx, mu, logvar):
        if not (mu.is_cuda and logvar.is_cuda):
            raise RuntimeError(f"reparameterize: the MI355X path needs CUDA/HIP tensors (got {mu.device}); there is no CPU fallback")
        if mu.dim() != 2 or mu.shape != logvar.shape:
            raise RuntimeError(f"reparameterize: expected two (B, L) tensors, got {tuple(mu.shape)} and {tuple(logvar.shape)}")
        B, Ld = mu.shape
        heads = torch.cat([mu.detach().float(), logvar.detach().float()], dim=1).contiguous()
        eps = engine.GLOBAL_NOISE.draw(B, [], Ld, mu.device)[1]
        mu_o, lv_o = torch.empty_like(heads[:, :Ld]).contiguous(), torch.empty_like(heads[:, :Ld]).contiguous()
        z = torch.empty(B, Ld, dtype=torch.float32, device=mu.device)
        with ops.pinned_stream():
            ops.fuse_reparam_fwd(B, Ld, heads, None, None, None, eps, mu_o, lv_o, z)
        ctx.save_for_backward(eps, lv_o)
        return z

    @staticmethod
    def backward(ctx, g):
        eps, lv = ctx.saved_tensors
        B, Ld = lv.shape
        d_heads = torch.empty(B, 2 * Ld, dtype=torch.float32, device=g.device)
        with ops.pinned_stream():
            ops.fuse_reparam_bwd(B, Ld, 1, None, None, [g.contiguous().float()], eps, lv, d_heads, None, None)
        return d_heads[:, :Ld], d_heads[:, Ld:]


# --------------------------------------------------------------------------------------------
# stand-alone blocks (EncoderA/B/C and DecoderA/B/C used on their own)
# --------------------------------------------------------------------------------------------
class BlockRuntime(engine.PrepCache):
    """Weight preparation cache for one block used outside a VAEGraph."""

    def __init__(self, block):
        super().__init__()
        self.block = block

    def ensure(self, prec, device):
        super().ensure(prec, device, self.block.params(), self.block.prepare)


def _zero_grads(block, device):
    """{param: zeroed fp32 gradient view}: the block's own flat arena (one fill launch)."""
    params = block.params()
    return engine.carve_arena(torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=device), params)


class EncoderMLPFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rt, prec, train, noise, x, *params):
        ctx.set_materialize_grads(False)
        x = engine._check_input(x.reshape(x.shape[0], -1), "x", rt.block.in_dim, prec)
        rt.ensure(prec, x.device)
        masks = noise.draw(x.shape[0], rt.block.widths(), None, x.device)[0] if train else None
        heads, layers = rt.block.forward(prec, x, train, masks)
        ctx.rt, ctx.prec, ctx.layers, ctx.train = rt, prec, layers, train
        Ld = rt.block.latent
        return heads[:, :Ld], heads[:, Ld:]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_mu, g_lv):
        blk = ctx.rt.block
        Ld = blk.latent
        y = ctx.layers[-1].y
        d_heads = torch.zeros(y.shape[0], 2 * Ld, dtype=torch.float32, device=y.device)
        if g_mu is not None:
            d_heads[:, :Ld].copy_(g_mu)
        if g_lv is not None:
            d_heads[:, Ld:].copy_(g_lv)
        grads = _zero_grads(blk, y.device)
        blk.backward(ctx.prec, ctx.layers, d_heads, grads, train=ctx.train)
        out = [grads[p] for p in blk.params()]
        del grads
        return (None, None, None, None, None, *out)


class EmbedEncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, block, site, *params):
        ctx.set_materialize_grads(False)
        if not site.is_cuda:
            raise RuntimeError("the MI355X path needs CUDA/HIP tensors; there is no CPU fallback")
        site = site.long().contiguous()
        B, Ld, dev = site.shape[0], block.latent, site.device
        table = block.table()
        mu = torch.empty(B, Ld, dtype=torch.float32, device=dev)
        lv = torch.empty(B, Ld, dtype=torch.float32, device=dev)
        z = torch.empty(B, ceil_to(Ld, 8), dtype=torch.float32, device=dev)
        zeros = torch.zeros(B, Ld, dtype=torch.float32, device=dev)
        ops.fuse_reparam_fwd(B, Ld, None, None, table, site, zeros, mu, lv, z)     # gather only (eps = 0)
        ctx.block, ctx.site = block, site
        return mu, lv

    @staticmethod
    @once_differentiable
    def backward(ctx, g_mu, g_lv):
        blk, site = ctx.block, ctx.site
        B, Ld, dev = site.shape[0], blk.latent, site.device
        zeros = torch.zeros(B, Ld, dtype=torch.float32, device=dev)
        g_mu = zeros if g_mu is None else g_mu.contiguous().float()
        g_lv = zeros if g_lv is None else g_lv.contiguous().float()
        d_heads = torch.empty(B, 2 * Ld, dtype=torch.float32, device=dev)
        d_table = torch.zeros(blk.embedding.weight.shape[0], 2 * Ld, dtype=torch.float32, device=dev)
        # dz = 0 and eps = 0: the kernel reduces to the scatter-add of (g_mu | g_lv) by class
        ops.fuse_reparam_bwd(B, Ld, 1, g_mu, g_lv, [zeros], zeros, zeros, d_heads, d_table, site)
        grads = _zero_grads(blk, dev)
        blk.backward(d_table, grads)
        out = [grads[p] for p in blk.params()]
        del grads
        return (None, None, *out)


class DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rt, prec, z, *params):
        ctx.set_materialize_grads(False)
        if not z.is_cuda:
            raise RuntimeError("the MI355X path needs CUDA/HIP tensors; there is no CPU fallback")
        blk = rt.block
        rt.ensure(prec, z.device)
        B, Ld = z.shape
        za = torch.zeros(B, ceil_to(Ld, 8), dtype=act_dtype(prec), device=z.device)
        za[:, :Ld].copy_(z)
        out, acts = blk.forward(prec, za)
        ctx.rt, ctx.prec, ctx.acts, ctx.out, ctx.Ld = rt, prec, acts, out.detach(), Ld      # detach: no ctx <-> output cycle
        ctx.z_needs = z.requires_grad
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        blk = ctx.rt.block
        if g is None:
            return (None,) * (3 + len(blk.params()))
        g = _as_rows(g)
        dz = torch.zeros(g.shape[0], ctx.Ld, dtype=torch.float32, device=g.device)
        grads = _zero_grads(blk, g.device)
        blk.backward(ctx.prec, ctx.acts, ctx.out, g, False, dz, grads)
        out = [grads[p] for p in blk.params()]
        del grads
        return (None, None, dz if ctx.z_needs else None, *out)
