"""float64 numpy oracle of the non-variational baselines RNA2DNAAE / DNA2RNAAE (reference src/models/directional_ae.py:10-134,
src/utils/ae_losses.py:8-39): forward, loss, backward and one AdamW step, built from np_oracle's layer primitives.

Parameters are keyed by the models' own state_dict names (encoder_rna.0.weight, site_projection.bias, decoder_dna.fc.4.weight, ...).
`q` is the hook directional_forward has: with q = bf16_round the GEMM operands are rounded where the device's bf16 mode rounds them
(inputs, prepared weights, stored activations and gradients), and z is rounded before the decoder; the head and the projected
table stay fp32 there, as on the device."""
import numpy as np

import np_oracle as O

# kind -> (encoder prefix, [(Linear, BatchNorm, Dropout) positions], head Linear position, decoder prefix, its Linear positions, Sigmoid)
KINDS = {"rna2dna": ("encoder_rna", [(0, 1, 3)], 4, "decoder_dna", [0, 2, 4], True),
         "dna2rna": ("encoder_dna", [(0, 1, 3), (4, 5, 7)], 8, "decoder_rna", [0, 2], False)}
HIDDEN = {"rna2dna": [128], "dna2rna": [512, 256]}


def param_shapes(kind, A, D, S, L, E=32):
    """[(state_dict key, shape)] in the order of the reference's state_dict"""
    pre, bn_idx, head, dec, dec_idx, _ = KINDS[kind]
    out, fan = [], (A if kind == "rna2dna" else D)
    for (li, bi, _), w in zip(bn_idx, HIDDEN[kind]):
        out += [(f"{pre}.{li}.weight", (w, fan)), (f"{pre}.{li}.bias", (w,)), (f"{pre}.{bi}.weight", (w,)), (f"{pre}.{bi}.bias", (w,)),
                (f"{pre}.{bi}.running_mean", (w,)), (f"{pre}.{bi}.running_var", (w,)), (f"{pre}.{bi}.num_batches_tracked", ())]
        fan = w
    out += [(f"{pre}.{head}.weight", (L, fan)), (f"{pre}.{head}.bias", (L,)),
            ("site_embedding.weight", (S, E)), ("site_projection.weight", (L, E)), ("site_projection.bias", (L,))]
    widths = ([256, 512, D] if kind == "rna2dna" else [128, A])
    fan = L
    for li, w in zip(dec_idx, widths):
        out += [(f"{dec}.fc.{li}.weight", (w, fan)), (f"{dec}.fc.{li}.bias", (w,))]
        fan = w
    return out


def is_buffer(key):
    return key.endswith(("running_mean", "running_var", "num_batches_tracked"))


def mask_names(kind):
    pre, bn_idx = KINDS[kind][:2]
    return [f"{pre}.{di}" for (_, _, di) in bn_idx]


def forward(kind, P, Bf, x=None, site=None, masks=None, train=True, update_running=True, q=None):
    """RNA2DNAAE.forward / DNA2RNAAE.forward -> (reconstruction, latent, cache); three Nones without inputs.  masks: {mask_names(): (B, width)}."""
    q = q or O._id
    pre, bn_idx, head, dec, dec_idx, sig = KINDS[kind]
    lat, cache = [], {"kind": kind}
    if x is not None:
        layers, h = [], q(x.reshape(x.shape[0], -1))
        for (li, bi, di) in bn_idx:
            W, b = q(P[f"{pre}.{li}.weight"]), P[f"{pre}.{li}.bias"]
            y = q(O._linear(h, W, b))                     # BatchNorm sees the stored (rounded) pre-activation
            base = f"{pre}.{bi}"
            hn, c = O._bn_relu_drop_fwd(y, P[base + ".weight"], P[base + ".bias"], masks.get(f"{pre}.{di}") if masks else None, train,
                                        Bf[base + ".running_mean"], Bf[base + ".running_var"])
            if train and update_running:
                O._bn_running_update(Bf, base, c["mean"], c["var"], x.shape[0])
            c.update(x=h, W=W, li=li, bi=bi)
            layers.append(c)
            h = q(hn)
        Wh = q(P[f"{pre}.{head}.weight"])
        lat.append(O._linear(h, Wh, P[f"{pre}.{head}.bias"]))
        cache["enc"] = dict(layers=layers, h=h, Wh=Wh)
    if site is not None:
        e = P["site_embedding.weight"][site]
        lat.append(O._linear(e, P["site_projection.weight"], P["site_projection.bias"]))
        cache["site"] = dict(e=e, site=site)
    if not lat:
        return None, None, None
    latent = lat[0] if len(lat) == 1 else (lat[0] + lat[1]) * 0.5          # torch.stack(latent_list).mean(0)
    out, cache["dec"] = O.decoder_fwd(P, dec, dec_idx, latent, sig, q)
    cache["n"] = len(lat)
    return out, latent, cache


def loss(kind, recon, target, q=None):
    """rna2dna_ae_loss (sum-BCE) / dna2rna_ae_loss (sum-MSE) -> (loss, the gradient the device's backward starts from, whether that
    gradient is w.r.t. the decoder's pre-sigmoid logits).  Without q the gradient is w.r.t. the reconstruction, as autograd has it."""
    if kind == "rna2dna":
        with np.errstate(divide="ignore"):
            val = O._bce_sum(recon, target)
        if q is None:
            return val, O._bce_grad(recon, target), False
        return val, q(O._bce_logit_grad(recon, target)), True
    return np.sum((recon - target) ** 2), (q or O._id)(2.0 * (recon - target)), False


def backward(kind, P, cache, d_out, q=None, out_is_logit_grad=False, d_latent=None):
    """-> {state_dict key: gradient}.  d_latent: a gradient that arrived at the returned latent (added to the decoder's)."""
    pre, _, head, _, _, _ = KINDS[kind]
    qq = q or O._id
    G = {}
    dz = O.decoder_bwd(P, cache["dec"], d_out, G, q, out_is_logit_grad)
    if d_latent is not None:
        dz = dz + d_latent
    d = dz / cache["n"]
    if "enc" in cache:
        enc = cache["enc"]
        dh, G[f"{pre}.{head}.weight"], G[f"{pre}.{head}.bias"] = O._linear_bwd(qq(d), enc["h"], enc["Wh"])     # d_head is an MFMA operand
        for c in reversed(enc["layers"]):
            dy, dg, db = O._bn_relu_drop_bwd(dh, c, q)
            G[f"{pre}.{c['bi']}.weight"], G[f"{pre}.{c['bi']}.bias"] = dg, db
            dh, G[f"{pre}.{c['li']}.weight"], G[f"{pre}.{c['li']}.bias"] = O._linear_bwd(dy, c["x"], c["W"])
    if "site" in cache:
        s = cache["site"]
        de, G["site_projection.weight"], G["site_projection.bias"] = O._linear_bwd(d, s["e"], P["site_projection.weight"])
        dE = np.zeros_like(P["site_embedding.weight"])
        np.add.at(dE, s["site"], de)
        G["site_embedding.weight"] = dE
    return G


def train_step(kind, P, Bf, state, step, x, target, site, masks, lr=5e-4, wd=1e-5, q=None):
    """forward -> AE loss -> backward -> AdamW (vae_cross_modality_cv.py:225-237).  Mutates P, Bf, state; returns a dict."""
    out, latent, cache = forward(kind, P, Bf, x, site, masks, True, q=q)
    val, g, is_logit = loss(kind, out, target, q)
    G = backward(kind, P, cache, g, q, is_logit)
    step = O.adamw_step(P, G, state, step, lr, wd)
    return dict(out=out, latent=latent, total=val, grads=G, step=step)


def make_params(seed, kind, A, D, S, L, E=32):
    """(P, Bf) float64 with values on a coarse grid (small integer codes times a power of two: the fixture stores the codes)."""
    codes, scales = make_codes(seed, kind, A, D, S, L, E)
    return decode(codes, scales)


def make_codes(seed, kind, A, D, S, L, E=32):
    rng = np.random.default_rng(seed)
    shapes = param_shapes(kind, A, D, S, L, E)
    bn = {k.rsplit(".", 1)[0] for k, _ in shapes if k.endswith("running_var")}
    codes, scales = {}, {}
    for key, shape in shapes:
        base, leaf = key.rsplit(".", 1)
        if leaf == "num_batches_tracked":
            continue
        if leaf == "running_var" or (base in bn and leaf == "weight"):
            codes[key] = rng.integers(16, 32, shape).astype(np.int8)              # positive: variances and BatchNorm gains, in [1, 2)
            scales[key] = 2.0 ** -4
        elif key == "site_embedding.weight":
            codes[key] = rng.integers(-31, 32, shape).astype(np.int8)             # N(0, 1)-sized, as nn.Embedding initialises
            scales[key] = 2.0 ** -4
        else:
            fan = shape[-1] if len(shape) == 2 else 16                            # about U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
            codes[key] = rng.integers(-31, 32, shape).astype(np.int8)             # six bits: the file compresses them
            scales[key] = 2.0 ** -(5 + int(np.ceil(0.5 * np.log2(fan))))
    return codes, scales


def decode(codes, scales):
    """{key: int8 codes}, {key: scale} -> (P, Bf) float64"""
    P, Bf = {}, {}
    for key, c in codes.items():
        (Bf if is_buffer(key) else P)[key] = c.astype(np.float64) * float(scales[key])
    for key in list(Bf):
        if key.endswith("running_mean"):
            Bf[key.replace("running_mean", "num_batches_tracked")] = np.int64(0)
    return P, Bf
