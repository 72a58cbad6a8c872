#!/usr/bin/env python3
"""Device time of the decoder's last Linear with the on-chip group reduce (ops.gemm_nt_group_moments) beside what it replaces --
mmvae_gemm_nt with an fp32 C of B G rows, then torch's mean and unbiased std over its view (B, G, N) -- in the same process, on the
same operands, in alternating windows:
  (a) B = 4096, G = 24, N = 782, K = 128, no activation    all sites, DNA -> RNA
  (b) B = 4096, G = 32, N = 572, K = 512, sigmoid          32 draws, RNA -> DNA
and of a whole Reconstructor.reconstruct call at both shapes (default-width models, 4096 samples), as it runs and with the fused
launch refused (the fallback the library's refusal leads to).

Times are device events around `--reps` back-to-back calls, divided by the count; median / min / max over `--rounds` windows after a
warm-up window, the two forms alternating round by round.  "fused_wins" is the criterion the kernel is kept by: the fused form's
SLOWEST window is faster than the unfused pair's FASTEST.  Bytes are the algorithm's: the operand, the weights and the two (B, N)
results for the fused form; for the pair also the (B G, N) fp32 matrix written once and read by each reduction.  Before anything is
timed the two forms' results are compared and the largest differences recorded.  ONE JSON object is printed, and written to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-los-angeles_amd")]

import torch  # noqa: E402

SHAPES = (dict(name="a: all sites, DNA->RNA", B=4096, G=24, N=782, K=128, sigmoid=False),
          dict(name="b: 32 draws, RNA->DNA", B=4096, G=32, N=572, K=512, sigmoid=True))


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternating(fns, rounds, reps):
    """{name: fn} -> {name: dict(median_ms, min_ms, max_ms)}; one warm-up window each, then the forms take turns round by round"""
    for fn in fns.values():
        window(fn, reps)
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(window(fn, reps))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), calls_per_window=reps) for k, v in ms.items()}


def verdict(t):
    return dict(fused_over_unfused=t["fused"]["median_ms"] / t["unfused"]["median_ms"], fused_wins=t["fused"]["max_ms"] < t["unfused"]["min_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_group_moments.py needs an MI355X: the product path has no CPU fallback")
    from mmvae import _lib as L, ops
    from mmvae.reconstruct import Reconstructor
    from src.models import DNA2RNAVAE, RNA2DNAVAE

    dev = torch.device("cuda", 0)
    result = dict(rounds=args.rounds, reps=args.reps, kernel=[], reconstruct=[])
    for sh in SHAPES:
        B, G, N, K = sh["B"], sh["G"], sh["N"], sh["K"]
        act = ops.ACT_SIGMOID if sh["sigmoid"] else ops.ACT_NONE
        gen = torch.Generator().manual_seed(1)
        a = torch.relu(torch.randn(B * G, K, generator=gen)).to(dev).to(torch.bfloat16)             # a hidden activation: behind a ReLU
        w = (torch.randn(N, K, generator=gen) * K ** -0.5).to(dev)
        bias = torch.randn(N, generator=gen).to(dev)
        pl = ops.PreparedLinear([w], [bias], ops.PREC_BF16, dev)
        ops.WeightPrep([pl], dev).run()
        mean, std = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)
        mean_u, std_u = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)
        full = torch.empty(B * G, N, device=dev)

        def fused():
            ops.gemm_nt_group_moments(ops.PREC_BF16, a, pl.w, N, K, G, mean, std, bias=pl.bias, act=act)

        def unfused():
            ops.gemm_nt(ops.PREC_BF16, a, pl.w, N, K, full, bias=pl.bias, act=act)
            v = full.view(B, G, N)
            torch.mean(v, dim=1, out=mean_u)
            torch.std(v, dim=1, out=std_u)

        with ops.pinned_stream():
            fused(); unfused()
            torch.cuda.synchronize()
            case = dict(sh, max_abs_diff_mean=float((mean - mean_u).abs().max()), max_abs_diff_std=float((std - std_u).abs().max()),
                        max_abs_mean=float(mean_u.abs().max()), max_abs_std=float(std_u.abs().max()))
            t = alternating(dict(fused=fused, unfused=unfused), args.rounds, args.reps)
        by_fused = B * G * K * 2 + N * K * 2 + 2 * B * N * 4
        by_unfused = by_fused + 3 * B * G * N * 4
        t["fused"]["GBps"] = by_fused / (t["fused"]["median_ms"] * 1e-3) / 1e9
        t["unfused"]["GBps"] = by_unfused / (t["unfused"]["median_ms"] * 1e-3) / 1e9
        t["fused"]["TFLOPs"] = 2.0 * B * G * N * K / (t["fused"]["median_ms"] * 1e-3) / 1e12
        result["kernel"].append(dict(case, bytes_fused=by_fused, bytes_unfused=by_unfused, **t, **verdict(t)))
        del a, full

    real = ops.gemm_nt_group_moments

    def refused(*a_, **k_):
        raise L.MMVAEArgError("mmvae_gemm_nt_group_moments failed: invalid argument")

    for name, cls, in_dim, kw in (("a: DNA2RNAVAE, sites='all'", DNA2RNAVAE, 572, dict(sites="all", draws=1)),
                                  ("b: RNA2DNAVAE, draws=32", RNA2DNAVAE, 782, dict(sites="given", draws=32))):
        torch.manual_seed(2)
        model = cls(782, 572, 24, 20).to(dev).set_precision("bf16").eval()
        rec = Reconstructor(model)
        x = torch.rand(4096, in_dim, device=dev)
        site = torch.randint(0, 24, (4096,), device=dev) if kw["sites"] == "given" else None

        def call():
            return rec.reconstruct(x, site, return_std=True, **kw)

        def call_unfused():
            ops.gemm_nt_group_moments = refused
            try:
                return rec.reconstruct(x, site, return_std=True, **kw)
            finally:
                ops.gemm_nt_group_moments = real
        call()
        assert rec.last_fused
        call_unfused()
        assert rec.last_fused is False
        t = alternating(dict(fused=call, unfused=call_unfused), args.rounds, max(1, args.reps // 5))
        result["reconstruct"].append(dict(name=name, B=4096, G=rec.group_size(kw["draws"], kw["sites"]), **t, **verdict(t)))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
