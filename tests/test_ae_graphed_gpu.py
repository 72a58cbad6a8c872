"""The captured and REPLAYED autoencoder step -- GraphedTrainStep(kind="rna2dna_ae" / "dna2rna_ae") -- against the numpy oracle
(tests/ae_oracle.py), bf16, default widths, B = 1000, two replays, as tests/test_graphed_oracle_gpu.py does for the VAE kinds.

The replayed graph draws its own keep-masks on the device; the oracle follows the stream through
np_noise.noise_source_draw(..., Ld=None): masks only, no eps.  After every replay: the loss floats (TOL_Q["loss"] after the first,
the trajectory tolerance of tests/test_train_gpu.py after the second), after the first also the parameters
(check_params_after_adamw) and the running statistics; the device's Philox offset and Adam's step count after each."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ae_oracle as AO  # noqa: E402
import np_noise as N  # noqa: E402
import np_oracle as O  # noqa: E402
from model_util import scaled_err, check_params_after_adamw  # noqa: E402
from test_model_gpu import TOL_Q, report, t  # noqa: E402
from test_graphed_oracle_gpu import TRAJ, _adam_steps  # noqa: E402
from test_ae_step_gpu import MODELS, REN, oname, load_ae  # noqa: E402
from mmvae import engine  # noqa: E402
from mmvae.graphs import GraphedTrainStep  # noqa: E402
from mmvae.optim import FusedAdamW  # noqa: E402

DEV = "cuda"
A, D, S, L, E, B = 782, 572, 24, 20, 32, 1000
LR, WD = 5e-3, 1e-5


@pytest.mark.parametrize("kind", ["rna2dna", "dna2rna"])
def test_replayed_ae_graph_vs_oracle(kind):
    step_kind = kind + "_ae"
    seed = 900 + 10 * GraphedTrainStep.KINDS.index(step_kind)
    torch.manual_seed(seed)
    dev = torch.device(DEV, torch.cuda.current_device())
    P, Bf = AO.make_params(seed, kind, A, D, S, L, E)
    model = load_ae(MODELS[kind](A, D, S, L, embed_dim=E), P, Bf).to(DEV).set_precision("bf16").train()
    engine.GLOBAL_NOISE.offset_tensor(dev).zero_()
    opt = FusedAdamW(model.parameters(), lr=LR, weight_decay=WD)
    a, b, site = O.make_batch(seed + 1, B, A, D, S)
    gs = GraphedTrainStep(model, opt, t(a), t(b), t(site), kind=step_kind, warmup=1, preserve_state=True)
    assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == 0 and _adam_steps(opt, model)[0] <= {0}      # the warm-up step was undone
    hP, hBf = {k: v.copy() for k, v in P.items()}, dict(Bf)
    state, step, offset, pseed = *O.adamw_init(hP), 0, torch.initial_seed() & (2 ** 64 - 1)
    x, tgt = ((a, b) if kind == "rna2dna" else (b, a))
    x, tgt = x.astype(np.float64), tgt.astype(np.float64)
    tag = f"replayed graph kind={step_kind} prec=bf16 B={B}"
    devs = []
    for s in range(2):
        masks, eps, offset = N.noise_source_draw(pseed, offset, B, AO.HIDDEN[kind], None)
        assert eps is None
        r = AO.train_step(kind, hP, hBf, state, step, x, tgt, site, dict(zip(AO.mask_names(kind), masks)), LR, WD, q=O.BF16)
        step = r["step"]
        gs()
        total, recon, cls, kld = gs.losses()
        assert cls == 0.0 and kld == 0.0 and total == recon
        devs.append(abs(total - r["total"]) / abs(r["total"]))
        assert engine.GLOBAL_NOISE.state_dict(dev)["offset"] == offset
        assert (engine.GLOBAL_NOISE.offset_tensor(dev) == offset).all()
        assert _adam_steps(opt, model) == ({s + 1}, {s + 1})
        if s == 0:
            assert devs[0] <= TOL_Q["loss"], (total, r["total"])
            sd = model.state_dict()
            bn = {k: scaled_err(sd[k].cpu().numpy(), v) for k, v in hBf.items() if not k.endswith("num_batches_tracked")}
            assert all(int(sd[k]) == 1 for k in hBf if k.endswith("num_batches_tracked"))
            assert max(bn.values()) <= TOL_Q["out"], bn
            share, dist = check_params_after_adamw(model, {oname(kind, k): v for k, v in hP.items()}, LR, "bf16", REN[kind])
            report(f"{tag} step 0: loss rel {devs[0]:.3e}; running statistics {max(bn.values()):.3e}; parameters after the replayed AdamW step: "
                   f"worst share off by > 1e-6 {share:.2e}, worst distance {dist:.2e} (lr {LR})")
    report(f"{tag} per-step loss vs bf16-aware oracle, steps 0..1: " + ", ".join(f"{d:.3e}" for d in devs) + f" (bound {TRAJ['bf16']:.0e})")
    assert max(devs) <= TRAJ["bf16"], devs
