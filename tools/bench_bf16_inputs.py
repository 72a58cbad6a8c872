#!/usr/bin/env python3
"""Captured training step with the RNA / DNA inputs in fp32 storage against bf16 storage (padded bf16 rows, mmvae.to_bf16_rows).

The bench.py workload: B = 65 536, bench.synth_batch, seed-0 weights, MultiModalVAE in bf16 mode, GraphedTrainStep.  Both sides
get the SAME values -- the batch rounded to bf16 once, kept as fp32 on one side and as padded bf16 rows on the other -- so the two
steps compute the same thing and differ only in what the first-layer GEMMs, their dW GEMMs and the reconstruction-loss epilogues
read.  The two steps are timed interleaved in one process, `--rounds` rounds of `--steps` replays each (the order alternates per
round), and ONE JSON object is printed: ms/step and samples/s of each side (median over rounds) with the spread (min / max).

`--probe`: afterwards one eager step of each side with events around the launches that change (bench.py's KernelProbe): the two
first-layer forward GEMMs (the GEMMs SURVEY.md section 8(d) names, floors 17.8 / 14.9 us in bf16), their dW GEMMs and the two
loss-epilogue GEMMs; the times are added to the JSON.

Per-kernel times from the profiler, in a run of their own (kernel names are templated: read the table sorted by total time;
`--only` keeps one side in the process):
    rocprofv3 --kernel-trace --stats -d prof_bf16 -o run -- python tools/bench_bf16_inputs.py --only bf16 --rounds 1 --steps 50
    rocprofv3 --kernel-trace --stats -d prof_fp32 -o run -- python tools/bench_bf16_inputs.py --only fp32 --rounds 1 --steps 50
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-los-angeles_amd")]

import torch  # noqa: E402

TAGS = ("EncoderA.L0.fwd", "EncoderB.L0.fwd", "EncoderA.L0.dW", "EncoderB.L0.dW", "DecoderA.L1.fwd", "DecoderB.L2.fwd")
FLOORS_US = {"EncoderA.L0.fwd": 17.8, "EncoderB.L0.fwd": 14.9}      # SURVEY.md section 8(d), bf16 storage


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50, help="replays per side and round")
    ap.add_argument("--warmup", type=int, default=10, help="untimed replays per side before the first round")
    ap.add_argument("--only", choices=["fp32", "bf16"], default=None, help="build and time one side only (profiler runs)")
    ap.add_argument("--probe", action="store_true", help="also time the changed launches of one eager step per side with events")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bf16_inputs.py needs an MI355X: the product path has no CPU fallback")
    from bench import synth_batch, A, D, S, L
    from mmvae import ops, to_bf16_rows
    from mmvae.graphs import GraphedTrainStep
    from mmvae.optim import FusedAdamW
    from src.models import MultiModalVAE

    dev = torch.device("cuda", 0)
    B = args.batch
    a, b, site = synth_batch(B, 0, dev)
    a32, b32 = a.bfloat16().float(), b.bfloat16().float()          # the same values on both sides
    a16, b16 = to_bf16_rows(a), to_bf16_rows(b)
    del a, b
    torch.manual_seed(0)
    init = {k: v.clone() for k, v in MultiModalVAE(A, D, S, L).to(dev).state_dict().items()}

    sides = {}
    for name, xa, xb in (("fp32", a32, b32), ("bf16", a16, b16)):
        if args.only is not None and name != args.only:
            continue
        model = MultiModalVAE(A, D, S, L).to(dev).set_precision("bf16")
        model.load_state_dict(init)
        opt = FusedAdamW(model.parameters(), lr=5e-4, weight_decay=1e-5)
        step = GraphedTrainStep(model, opt, xa, xb, site, beta=1e-3, gamma=1.0, warmup=2)
        for _ in range(args.warmup):
            step()
        sides[name] = step
    torch.cuda.synchronize()

    times = {n: [] for n in sides}
    names = list(sides)
    for r in range(args.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                sides[n]()
            t1.record()
            torch.cuda.synchronize()
            times[n].append(t0.elapsed_time(t1) / args.steps)
    out = dict(tool="bench_bf16_inputs", batch=B, rounds=args.rounds, steps_per_round=args.steps, precision="bf16")
    for n in names:
        ms = times[n]
        med = statistics.median(ms)
        out[f"{n}_storage"] = dict(ms_per_step=med, ms_min=min(ms), ms_max=max(ms), spread_ms=max(ms) - min(ms),
                                   samples_per_s=B / med * 1e3, rounds_ms=ms, losses=list(sides[n].losses()))
    if len(names) == 2:
        f, h = out["fp32_storage"], out["bf16_storage"]
        out["saved_ms_per_step"] = f["ms_per_step"] - h["ms_per_step"]
        out["speedup"] = f["ms_per_step"] / h["ms_per_step"]
        # faster beyond the noise: the slowest bf16 round beats the fastest fp32 round
        out["faster_beyond_spread"] = h["ms_max"] < f["ms_min"]
    if args.probe:
        out["kernels_us"] = {}
        for n in names:
            ops.PROBE = ops.KernelProbe(only=set(TAGS))
            sides[n].run_eager()
            torch.cuda.synchronize()
            summ = ops.PROBE.summary()
            ops.PROBE = None
            out["kernels_us"][n] = {t: round(summ[t]["mean_ms"] * 1e3, 2) for t in TAGS if t in summ}
        out["floors_us_bf16"] = FLOORS_US
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
