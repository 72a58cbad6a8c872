#!/usr/bin/env python3
"""Device time of the autoencoder baselines RNA2DNAAE / DNA2RNAAE (src/models/directional_ae.py on mmvae.engine.AEGraph).

At the default widths (RNA 782, DNA 572, 24 sites, latent 20), bf16:
  (a) one training step per kind -- forward, loss in the decoder's last GEMM, backward, AdamW -- issued from Python
      (GraphedTrainStep.run_eager) and as a replay of the captured graph, at the cross-validation's batch (64) and at 65 536; the AE
      kinds twice, captured with the fused latent launch (tuning key 15) on and off; beside them the directional VAE's step
  (b) the latent path alone at both batches: mmvae_ae_latent_fwd against the three launches it replaces (the encoder's head GEMM +
      mmvae_fuse_mean_fwd + the decoder's first-layer GEMM) on the same operands
  Every comparison is INTERLEAVED in one process on one device: all sides are built and warmed up first (--warmup calls each), then
  every round times each side once, the side that goes first rotating with the round.
  (c) a whole fit_ae fold at the shape of tests/test_crossval_ae_gpu.py (RNA 40, DNA 24, 5 sites, latent 8, 200 rows, 2 epochs, batch
      32), captured and eager, wall clock, beside fit_vae
Device events around synchronised work, a warm-up call and --rounds timed ones: median / min / max.  ONE JSON object is printed and
written to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-los-angeles_amd")]

import torch  # noqa: E402


def interleaved(sides, rounds, warmup, inner):
    """sides: {name: fn} -> {name: median / min / max ms per call}: every side warmed up, then per round one timed interval of
    `inner` calls per side, the order rotating with the round"""
    names = list(sides)
    for n in names:
        for _ in range(warmup):
            sides[n]()
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    for r in range(rounds):
        for n in names[r % len(names):] + names[:r % len(names)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                sides[n]()
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1) / inner)
    return {n: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for n, v in ms.items()}


def wall(fn, rounds):
    fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 65536])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="steps per timed interval")
    ap.add_argument("--warmup", type=int, default=30, help="untimed calls of every side before the first timed round")
    ap.add_argument("--skip", nargs="*", default=[], choices=["a", "b", "c"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ae.py needs an MI355X: the product path has no CPU fallback")
    import trainer
    from mmvae import _lib, crossval, ops
    from mmvae.graphs import GraphedTrainStep
    from mmvae.optim import FusedAdamW
    from src.config import Config
    from src.models import DNA2RNAAE, RNA2DNAAE, DNA2RNAVAE, RNA2DNAVAE

    def key(on):
        _lib.check(_lib.load().mmvae_set_tuning(15, int(bool(on))), "mmvae_set_tuning")

    dev = torch.device("cuda", 0)
    A, D, S, L = 782, 572, 24, Config.LATENT_DIM
    models = {"rna2dna_ae": RNA2DNAAE, "dna2rna_ae": DNA2RNAAE, "rna2dna": RNA2DNAVAE, "dna2rna": DNA2RNAVAE}
    result = dict(dims=[A, D, S, L], precision="bf16", rounds=args.rounds, a=[], b=[])
    for B in args.batches:
        tpm, beta_v, site = trainer.synthetic_dataset(B, A, D, S, Config.RANDOM_SEED)
        a, b, s = tpm.to(dev), beta_v.to(dev), site.to(dev)
        if "a" not in args.skip:
            steps = {}
            for kind, cls in models.items():
                for fused in ((True, False) if kind.endswith("_ae") else (True,)):
                    key(fused)                           # the capture records the launches the engine issues under this key
                    torch.manual_seed(0)
                    model = cls(A, D, S, L).to(dev).set_precision("bf16")
                    opt = FusedAdamW(model.parameters(), lr=Config.LEARNING_RATE, weight_decay=Config.WEIGHT_DECAY)
                    steps[kind + ("" if fused else "/three_launches")] = GraphedTrainStep(model, opt, a, b, s, beta=1e-3, kind=kind, warmup=2)
            key(True)
            replay = interleaved(dict(steps), args.rounds, args.warmup, args.inner)

            def eager_of(name, gs):
                def fn():
                    key("/" not in name)
                    gs.run_eager()
                return fn
            eager = interleaved({n: eager_of(n, gs) for n, gs in steps.items()}, args.rounds, max(3, args.warmup // 5), args.inner)
            key(True)
            for name in steps:
                row = dict(kind=name, batch=B, graph_replay=replay[name], eager=eager[name], samples_per_s_replay=B / (replay[name]["median_ms"] * 1e-3))
                result["a"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
            del steps
        if "b" not in args.skip:
            for kind in ("rna2dna_ae", "dna2rna_ae"):
                model = models[kind](A, D, S, L).to(dev).set_precision("bf16").eval()
                g = model._graph()
                enc, dec = (g.enc_a or g.enc_b), g.decoders[0]
                g._prep.ensure(ops.PREC_BF16, dev, g.param_list(), g._prepare)
                K = enc.pl_heads.K
                y = torch.randn(B, K, device=dev).to(torch.bfloat16)
                scale, shift = torch.rand(K, device=dev) + 0.5, torch.randn(K, device=dev)
                mask = (torch.rand(B, K, device=dev) >= 0.1).to(torch.uint8)
                owed = ops.LatentEncoder(y, ops.Prologue(scale, shift, mask, 1.0 / 0.9), None, enc.pl_heads)
                table = g.enc_c.table()
                latent = torch.empty(B, L, dtype=torch.float32, device=dev)
                z = torch.empty(B, ops.ceil_to(L, 8), dtype=torch.bfloat16, device=dev)
                pl0 = dec.pl[0]
                h0 = torch.empty(B, ops.ceil_to(pl0.N, 8), dtype=torch.bfloat16, device=dev)

                def three():
                    with ops.pinned_stream():
                        head = enc.run_heads(ops.PREC_BF16, owed)
                        ops.fuse_mean_fwd(B, L, head, table, s, latent, z)
                        ops.gemm_nt(ops.PREC_BF16, z, pl0.w, pl0.N, pl0.K, h0, bias=pl0.bias, act=ops.ACT_RELU)

                def fused():
                    with ops.pinned_stream():
                        ops.ae_latent_fwd(ops.PREC_BF16, B, L, owed, table, s, latent, z, pl0, h0)
                row = dict(kind=kind, batch=B, head_K=K, stem_N=pl0.N,
                           **interleaved(dict(fused_launch=fused, three_launches=three), args.rounds, args.warmup, args.inner))
                row["fused_over_three"] = row["fused_launch"]["median_ms"] / row["three_launches"]["median_ms"]
                result["b"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    if "c" not in args.skip:
        A2, D2, S2, L2, N2 = 40, 24, 5, 8, 200
        tpm, beta_v, site = trainer.synthetic_dataset(N2, A2, D2, S2, Config.RANDOM_SEED)
        a, b, s = tpm.to(dev), beta_v.to(dev), site.to(dev)
        result["c"] = dict(dims=[A2, D2, S2, L2], rows=N2, epochs=2, batch=32)
        for name, fit in (("fit_ae", crossval.fit_ae), ("fit_vae", crossval.fit_vae)):
            for eager in (False, True):
                result["c"][f"{name}_{'eager' if eager else 'captured'}"] = wall(
                    lambda: fit("dna2rna", a, b, s, (A2, D2, S2, L2), epochs=2, batch_size=32, eager=eager), max(2, args.rounds // 2))
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
