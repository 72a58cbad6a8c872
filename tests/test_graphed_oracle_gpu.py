"""The captured and REPLAYED training step (mmvae.graphs.GraphedTrainStep: what bench.py and the three trainers run) against the
numpy oracle, for the multimodal step and both directional kinds, in both precisions, default widths, B = 1000.

The replayed graph draws its own noise on the device (Philox, keyed by torch.initial_seed() and a device-resident offset that
the launch advances).  oracle/np_noise.py restates that stream on the host (pinned by tests/test_noise_gpu.py), so the oracle
can follow the replay: np_noise.noise_source_draw gives the keep-masks and eps of steps 0..3 from the seed and offset 0, and
O.train_step / O.directional_train_step run on them with q=None (fp32) or q=O.BF16 (bf16).

  after ONE replay   the loss floats of step 0 (TOL["fp32"]["loss"] / TOL_Q["loss"]); the parameters after that AdamW step
                     (model_util.check_params_after_adamw, lr 5e-3); the running statistics at the `out` tolerance; the device's
                     Philox offset = the host helper's next offset; Adam's step count = 1 on the host and on the device.
  three more         the per-step total loss within the project's trajectory tolerance (tests/test_train_gpu.py: 2e-4 fp32,
                     4e-3 bf16, set for 8 such steps at this lr) of the same-q oracle; the offset after four draws.
  dataset=           one directional kind in bf16, two steps whose minibatches the captured gather takes from a device-resident
                     dataset through set_indices: the oracle gathers the same rows.

The device's eps is the float32 evaluation of the normals whose float64 values the host casts to float32.  tests/test_noise_gpu.py
holds every element to 13 x 2^-24 x radius (eps_tolerance), and the radius of a Box-Muller draw from a 24-bit uniform is at most
sqrt(2 ln 2^24) = 5.77: |d eps| <= 4.5e-6, 1e-7 typically, against |eps| ~ 1.  z = mu + eps exp(logvar / 2) moves by the same
relative amount, and everything behind z is Lipschitz in it with constants of order one, so the step-0 quantities move by
<= 4.5e-6 of their scale at the very worst: a factor >= 4 below the tightest tolerance relied on here (2e-5 on the fp32 loss
floats, which as sums over 1000 x 782 terms of random sign in d eps move ~ 1e-3 of that worst case), >= 11 below the fp32 `out`
tolerance 5e-5 and >= 20 below every bf16 tolerance (1e-4).
The measured deviations go to the parity report (test_model_gpu.report).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import np_noise as N  # noqa: E402
import np_oracle as O  # noqa: E402
from model_util import load_state, scaled_err, f64, check_params_after_adamw  # noqa: E402
from test_model_gpu import TOL, TOL_Q, report, t  # noqa: E402
from mmvae import engine  # noqa: E402
from mmvae.graphs import GraphedTrainStep  # noqa: E402
from mmvae.optim import FusedAdamW  # noqa: E402
from src.models import MultiModalVAE, RNA2DNAVAE, DNA2RNAVAE  # noqa: E402

DEV = "cuda"
A, D, S, L, E, B = 782, 572, 24, 20, 32, 1000
BETA, GAMMA, LR, WD = 1e-3, 1.0, 5e-3, 1e-5
TRAJ = {"fp32": 2e-4, "bf16": 4e-3}                      # tests/test_train_gpu.py::test_loss_trajectory_vs_oracle
MASKS = {"multimodal": ("encoder_a.fc.3", "encoder_b.fc.3", "encoder_b.fc.7"), "rna2dna": ("encoder_a.fc.3",),
         "dna2rna": ("encoder_b.fc.3", "encoder_b.fc.7")}
WIDTHS = {"encoder_a.fc.3": O.HID_A, "encoder_b.fc.3": O.HID_B1, "encoder_b.fc.7": O.HID_B2}
MODELS = {"multimodal": MultiModalVAE, "rna2dna": RNA2DNAVAE, "dna2rna": DNA2RNAVAE}


class Host:
    """The oracle's side of a training run that follows the device's noise stream."""

    def __init__(self, kind, prec, P, Bf, seed):
        self.kind, self.q, self.seed, self.offset = kind, (None if prec == "fp32" else O.BF16), seed, 0
        self.P, self.Bf = f64(P), f64(Bf)
        self.state, self.step = O.adamw_init(self.P)

    def train_step(self, a, b, site):
        """One step on the batch (a, b, site) with the noise of the stream's next draw -> (total, recon, class or None, kld)."""
        names = MASKS[self.kind]
        masks, eps, self.offset = N.noise_source_draw(self.seed, self.offset, len(site), [WIDTHS[n] for n in names], L)
        masks, eps = dict(zip(names, masks)), eps.astype(np.float64)
        a, b = a.astype(np.float64), b.astype(np.float64)
        if self.kind == "multimodal":
            r = O.train_step(self.P, self.Bf, self.state, self.step, a, b, site, masks, eps, BETA, GAMMA, None, LR, WD, q=self.q)
            out = (r["total"], r["recon"], r["cls"], r["kld"])
        else:
            x, tgt = (a, b) if self.kind == "rna2dna" else (b, a)
            r = O.directional_train_step(self.kind, self.P, self.Bf, self.state, self.step, x, tgt, site, masks, eps, BETA, LR, WD, q=self.q)
            out = (r["total"], r["recon"], None, r["kld"])
        self.step = r["step"]
        return out


def _setup(kind, prec, seed):
    torch.manual_seed(seed)
    dev = torch.device(DEV, torch.cuda.current_device())
    P, Bf = O.make_params(seed, A, D, S, L, E)
    ren = None if kind == "multimodal" else O.directional_param_names(kind, A, D, S, L, E)
    model = load_state(MODELS[kind](A, D, S, L, embed_dim=E), P, Bf, ren).to(DEV).set_precision(prec).train()
    engine.GLOBAL_NOISE.offset_tensor(dev).zero_()
    opt = FusedAdamW(model.parameters(), lr=LR, weight_decay=WD)
    return dev, model, opt, ren, Host(kind, prec, P, Bf, torch.initial_seed() & (2 ** 64 - 1))


def _loss_dev(got, want):
    """Relative deviation per loss float; a term the step does not have (None) must read exactly 0."""
    out = []
    for g_, w_ in zip(got, want):
        if w_ is None:
            assert g_ == 0.0, got
        else:
            out.append(abs(g_ - w_) / abs(w_))
    return out


def _adam_steps(opt, model):
    host = {int(opt.state[p]["step"].item()) for p in model.parameters()}
    devc = {int(v) for fast in opt._fast.values() for v in fast["step_dev"].tolist()}       # the counter the captured launch advances
    return host, devc


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["multimodal", "dna2rna", "rna2dna"])
def test_replayed_graph_vs_oracle(kind, prec):
    seed = 500 + 10 * GraphedTrainStep.KINDS.index(kind) + (prec == "bf16")
    dev, model, opt, ren, host = _setup(kind, prec, seed)
    a, b, site = O.make_batch(seed + 1, B, A, D, S)
    gs = GraphedTrainStep(model, opt, t(a), t(b), t(site), beta=BETA, gamma=GAMMA, kind=kind, warmup=1, preserve_state=True)
    assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == 0 and _adam_steps(opt, model)[0] <= {0}      # the warm-up step was undone
    tag = f"replayed graph kind={kind} prec={prec} B={B}"

    # ---- one replay -------------------------------------------------------------------------------------------------
    want = host.train_step(a, b, site)
    gs()
    got = gs.losses()
    ldev = _loss_dev(got, want)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    inv = {v: k for k, v in ren.items()} if ren else None
    bn = {}
    for k, v in sd.items():
        top, rest = k.split(".", 1)
        ko = k if inv is None else inv[top] + "." + rest
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1 == int(host.Bf[ko]), k
        elif k.endswith("running_mean") or k.endswith("running_var"):
            bn[ko] = scaled_err(v, host.Bf[ko])
    report(f"{tag} step 0 vs same-q oracle: loss floats rel {max(ldev):.3e}; running statistics {max(bn.values()):.3e}")
    assert max(ldev) <= (TOL["fp32"]["loss"] if prec == "fp32" else TOL_Q["loss"]), (got, want)
    assert max(bn.values()) <= (TOL["fp32"]["out"] if prec == "fp32" else TOL_Q["out"]), bn
    share, dist = check_params_after_adamw(model, host.P, LR, prec, ren)
    report(f"{tag} parameters after the replayed AdamW step: worst share off by > 1e-6 {share:.2e}, worst distance {dist:.2e} (lr {LR})")
    assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == host.offset
    assert (engine.GLOBAL_NOISE.offset_tensor(dev) == host.offset).all()
    assert _adam_steps(opt, model) == ({1}, {1})

    # ---- three more -------------------------------------------------------------------------------------------------
    devs = [ldev[0]]
    for s in range(1, 4):
        want = host.train_step(a, b, site)
        gs()
        got = gs.losses()
        devs.append(abs(got[0] - want[0]) / abs(want[0]))
    report(f"{tag} per-step total loss vs same-q oracle, steps 0..3: " + ", ".join(f"{d:.3e}" for d in devs) + f" (bound {TRAJ[prec]:.0e})")
    assert max(devs) <= TRAJ[prec], devs
    assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == host.offset
    assert _adam_steps(opt, model) == ({4}, {4})


def test_replayed_graph_with_dataset_vs_oracle():
    """dataset= with set_indices: the step begins with the captured gather.  rna2dna, bf16, two steps on different rows."""
    kind, prec, seed, n_rows = "rna2dna", "bf16", 540, 2500
    dev, model, opt, ren, host = _setup(kind, prec, seed)
    dA, dB, dS = O.make_batch(seed + 1, n_rows, A, D, S)
    order = np.random.default_rng(seed + 2).permutation(n_rows)
    gs = GraphedTrainStep(model, opt, beta=BETA, gamma=GAMMA, kind=kind, warmup=1, preserve_state=True,
                          dataset=(t(dA), t(dB), t(dS)), batch_size=B)
    devs = []
    for s in range(2):
        idx = order[s * B:(s + 1) * B]
        want = host.train_step(dA[idx], dB[idx], dS[idx])
        gs.set_indices(t(idx))
        gs()
        got = gs.losses()
        devs.append(max(_loss_dev(got, want)))
        if s == 0:
            assert devs[0] <= TOL_Q["loss"], (got, want)
            check_params_after_adamw(model, host.P, LR, prec, ren)
    report(f"replayed graph kind={kind} prec={prec} B={B} dataset= + set_indices, loss floats vs same-q oracle, steps 0..1: "
           + ", ".join(f"{d:.3e}" for d in devs) + f" (bound {TRAJ[prec]:.0e})")
    assert max(devs) <= TRAJ[prec], devs
    assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == host.offset
    assert _adam_steps(opt, model) == ({2}, {2})
