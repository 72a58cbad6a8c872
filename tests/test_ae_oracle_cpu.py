"""tests/ae_oracle.py (float64 numpy) against tests/golden/ae_b32.npz, the reference's RNA2DNAAE / DNA2RNAAE run in float64 on the CPU
(tools/make_ae_fixture.py): every recorded array -- the training step's reconstruction, latent, loss, every gradient and the running
statistics afterwards, the eval-mode forwards with both inputs, with site=None and with the site alone -- to 1e-9 relative; and the
recorded state_dict keys and shapes against the drop-in modules' own."""
import numpy as np
import pytest

import ae_oracle as AO
import golden_util as G

RTOL, ATOL = 1e-9, 1e-12
KINDS = ("rna2dna", "dna2rna")


@pytest.fixture(scope="module")
def fx():
    return G.load("ae_b32")


def _state(fx, kind):
    k = kind + "."
    return AO.decode({n[len(k) + 5:]: fx[n] for n in fx.files if n.startswith(k + "code.")},
                     {n[len(k) + 6:]: fx[n] for n in fx.files if n.startswith(k + "scale.")})


def _batch(fx, kind):
    k = kind + "."
    x, tgt = (fx[k + "rna"], fx[k + "dna"]) if kind == "rna2dna" else (fx[k + "dna"], fx[k + "rna"])
    return x, tgt, fx[k + "site"], {n: fx[k + "mask." + n] for n in AO.mask_names(kind)}


@pytest.mark.parametrize("kind", KINDS)
def test_training_step_matches_the_reference(fx, kind):
    k = kind + "."
    P, Bf = _state(fx, kind)
    x, tgt, site, masks = _batch(fx, kind)
    assert x.dtype == np.float64 and all(v.dtype == np.float64 for v in P.values())
    out, latent, cache = AO.forward(kind, P, Bf, x, site, masks, True)
    G.expect(fx, k + "s0.out", out, RTOL, ATOL)
    G.expect(fx, k + "s0.latent", latent, RTOL, ATOL)
    val, g, is_logit = AO.loss(kind, out, tgt)
    assert abs(val - float(fx[k + "s0.loss"])) <= RTOL * abs(val)
    grads = AO.backward(kind, P, cache, g, None, is_logit)
    recorded = {n[len(k) + 8:].split("@")[0] for n in fx.files if n.startswith(k + "s0.grad.")}
    assert recorded == set(grads) == set(P)
    for key, gv in grads.items():
        G.expect(fx, k + "s0.grad." + key, gv, RTOL, ATOL, scale_atol=1e-12)
    after = {n[len(k) + 9:] for n in fx.files if n.startswith(k + "s0.after.")}
    assert after == set(Bf)
    for key in after:
        G.expect(fx, k + "s0.after." + key, np.asarray(Bf[key], np.float64), RTOL, ATOL)


@pytest.mark.parametrize("kind", KINDS)
def test_eval_forwards_match_the_reference(fx, kind):
    k = kind + "."
    P, Bf = _state(fx, kind)
    x, _, site, _ = _batch(fx, kind)
    for tag, args in (("both", (x, site)), ("nosite", (x, None)), ("siteonly", (None, site))):
        out, latent, _ = AO.forward(kind, P, dict(Bf), args[0], args[1], None, False)
        G.expect(fx, k + f"eval.{tag}.out", out, RTOL, ATOL)
        G.expect(fx, k + f"eval.{tag}.latent", latent, RTOL, ATOL)
    assert AO.forward(kind, P, Bf) == (None, None, None)


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_keys_and_shapes_are_the_reference_s(fx, kind):
    from src.models import RNA2DNAAE, DNA2RNAAE
    A, D, S, L, E = (int(v) for v in fx["dims"])
    model = (RNA2DNAAE if kind == "rna2dna" else DNA2RNAAE)(A, D, S, L, embed_dim=E)
    sd = model.state_dict()
    names, shapes = [str(n) for n in fx[kind + ".names"]], [str(s) for s in fx[kind + ".shapes"]]
    assert list(sd) == names
    assert [",".join(str(n) for n in v.shape) for v in sd.values()] == shapes
    assert [(n, ",".join(str(d) for d in s)) for n, s in AO.param_shapes(kind, A, D, S, L, E)] == list(zip(names, shapes))
    enc = "encoder_rna" if kind == "rna2dna" else "encoder_dna"
    digits = sorted({int(n.split(".")[1]) for n in names if n.startswith(enc + ".")})
    assert digits == ([0, 1, 4] if kind == "rna2dna" else [0, 1, 4, 5, 8])
    assert model() == (None, None)
