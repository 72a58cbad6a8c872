"""MultiModalVAE training steps on a SUBSET of the modalities and of the loss terms: the cases and their oracle step, shared by the
CPU check of the oracle (tests/test_oracle_vs_golden.py) and the GPU comparison (tests/test_partial_modalities_gpu.py).

  inputs      loss terms           what the engine does differently from the full step
  a           MSE a + BCE b + KL   n_mod = 1; decoder_c gets no gradient: the stem ran in the forward, the backward goes without it
                                   (dW and ReLU-mask dX on column slices of H0, dz summed in the fusion backward); encoder_b,
                                   encoder_c and decoder_c end with .grad None
  b, site     all four             n_mod = 2, encoder_a absent (mask slicing with n_a = 0), stem backward
  a, b        MSE a + KL           two decoders without gradient, no embedding-table gradient
  site        all four             no MLP encoder: no masks, no BatchNorm sums
"""
import numpy as np

import np_oracle as O

CASES = {
    "a": dict(inputs=("a",), terms=("a", "b", "kl")),
    "b_site": dict(inputs=("b", "site"), terms=("a", "b", "c", "kl")),
    "a_b": dict(inputs=("a", "b"), terms=("a", "kl")),
    "site": dict(inputs=("site",), terms=("a", "b", "c", "kl")),
}
ENCODER_OF = {"a": "encoder_a", "b": "encoder_b", "site": "encoder_c"}
MASKS_OF = {"a": ("encoder_a.fc.3",), "b": ("encoder_b.fc.3", "encoder_b.fc.7"), "site": ()}


def mask_names(case):
    """The keep-masks a forward with this case's inputs consumes, in the order it consumes them."""
    return tuple(n for m in ("a", "b", "site") if m in CASES[case]["inputs"] for n in MASKS_OF[m])


def oracle_partial_step(P64, Bf64, a, b, site, masks, eps, case, beta, gamma, cw, q):
    """One forward on the case's inputs + the loss on its terms + backward of the numpy oracle, float64 (q=None: reference
    arithmetic; q=O.BF16: bf16-aware, DecoderB from the logit gradient).  a / b / site are the full batch: the TARGETS of the loss
    terms; only the case's inputs are fed to the model.  -> the dict tests/test_model_gpu.py::compare_step takes; a decoder
    without a gradient and an encoder that did not run are absent from G."""
    f = np.float64
    c = CASES[case]
    a, b = a.astype(f), b.astype(f)
    Bf_run = dict(Bf64)
    kw = dict(a=a if "a" in c["inputs"] else None, b=b if "b" in c["inputs"] else None, site=site if "site" in c["inputs"] else None)
    oa, ob, oc, mu, lv, cache = O.vae_forward(P64, Bf_run, masks=masks, eps=eps.astype(f), train=True, q=q, **kw)
    tot, rec, cls, kld, g = O.partial_loss(c["terms"], oa, a, ob, b, oc, site, mu, lv, beta, gamma, None if cw is None else cw.astype(f), q=q)
    if q is None:
        G = O.vae_backward(P64, cache, g["recon_a"], g["recon_b"], g["recon_c"], g["mu"], g["logvar"])
    else:
        G = O.vae_backward(P64, cache, g["recon_a"], g["recon_b_logit"], g["recon_c"], g["mu"], g["logvar"], q, True)
    t = c["terms"]
    losses = (tot, rec if ("a" in t or "b" in t) else None, cls if "c" in t else None, kld if "kl" in t else None)      # None: no such term
    return dict(out_a=oa, out_b=ob, out_c=oc, mu=mu, logvar=lv, losses=losses, G=G, Bf=Bf_run)
