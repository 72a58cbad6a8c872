#!/usr/bin/env python3
"""Device time and extra device memory of the StandardScaler on column blocks (ops.standardize_fit / standardize_apply,
clustering.StandardScaler.fit_transform) at the evaluation shape -- the validation rows of evaluate.py's default split (52 429), the
feature matrix [RNA 782 | DNA 572] as two fp32 parts -- beside, from the same run on the same data, the path it stands next to:
  the assembly of the (rows, 1354) matrix from its parts in batches with copy_ (evaluate.py's clustering_table), and
  clustering.standardize of the assembled matrix (a float64 torch chain).

Times are device events around `--reps` back-to-back calls, divided by the count; median / min / max over `--rounds` such windows after
a warm-up one.  The achieved bytes/s of fit and apply are against their ALGORITHMIC bytes (fit: the parts read once + three float64
vectors; apply: the parts read once + mean and scale + z written once).  Peak extra device memory is the rise of
torch.cuda.max_memory_allocated over the allocation held before the call (inputs resident, outputs and temporaries counted).  Before
anything is timed the two results are compared element by element.  "cold_cache": the same calls one at a time, each after a 1 GiB
buffer has been overwritten, as the scaler runs in the workflow (once, on fresh data); the windows above re-read a warm Infinity Cache.  ONE JSON object is printed, and written to --out if given."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-los-angeles_amd")]

import torch  # noqa: E402


def timed(fn, rounds, reps=1, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), calls_per_window=reps)


def timed_cold(fn, flush, calls=20):
    """single calls, each after `flush` has been overwritten (1 GiB: four times the 256 MiB Infinity Cache), so that neither the inputs
    nor a previous call's output are cache-resident; events around the one call"""
    ms = []
    for _ in range(calls + 1):
        flush.add_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[1:]
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), calls=calls)


def peak_extra_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - held
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=52429)
    ap.add_argument("--batch", type=int, default=4096, help="rows per copy_ of the assembly comparator")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1000, help="calls per timed window (a call takes 0.1 - 0.3 ms: windows of 0.1 - 0.3 s)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_standardize.py needs an MI355X: the product path has no CPU fallback")
    from mmvae import clustering, ops
    from src.config import Config
    from trainer import synthetic_dataset

    dev = torch.device("cuda", 0)
    N, A, D = args.rows, 782, 572
    F = A + D
    tpm, beta_v, _ = synthetic_dataset(N, A, D, 24, Config.RANDOM_SEED)
    parts = [tpm.to(dev).contiguous(), beta_v.to(dev).contiguous()]
    in_bytes = sum(p.numel() * p.element_size() for p in parts)
    result = dict(rows=N, parts=[A, D], width=F, rounds=args.rounds, fit_splits=ops.standardize_fit_splits(N, F),
                  fit_work_bytes=ops.standardize_fit_work_bytes(N, F))

    def assemble(out=None):
        feats = torch.empty(N, F, dtype=torch.float32, device=dev) if out is None else out
        for i in range(0, N, args.batch):
            feats[i:i + args.batch, :A].copy_(parts[0][i:i + args.batch])
            feats[i:i + args.batch, A:].copy_(parts[1][i:i + args.batch])
        return feats

    # the two paths agree
    feats = assemble()
    z_old = clustering.standardize(feats)
    z_new = clustering.StandardScaler().fit_transform(parts)
    diff = (z_new.double() - z_old.double()).abs()
    result["max_abs_diff_to_clustering_standardize"] = float(diff.max())
    result["elements_differing"] = int((diff > 0).sum())
    result["max_abs_z"] = float(z_old.abs().max())
    del z_old, diff

    mean, var, scale = ops.standardize_fit(parts)
    work = ops._workspace(result["fit_work_bytes"], dev)
    fit_bytes = in_bytes + 24 * F
    apply_bytes = in_bytes + 16 * F + 4 * N * F
    t = timed(lambda: ops.standardize_fit(parts, mean_out=mean, var_out=var, scale_out=scale, work=work), args.rounds, args.reps)
    result["fit"] = dict(t, algorithmic_bytes=fit_bytes, GBps=fit_bytes / (t["median_ms"] * 1e-3) / 1e9)
    t = timed(lambda: ops.standardize_apply(parts, mean, scale, out=z_new), args.rounds, args.reps)
    result["apply"] = dict(t, algorithmic_bytes=apply_bytes, GBps=apply_bytes / (t["median_ms"] * 1e-3) / 1e9)
    del z_new
    result["fit_transform"] = timed(lambda: clustering.StandardScaler().fit_transform(parts), args.rounds, args.reps)
    result["parent_assemble_copy"] = timed(lambda: assemble(feats), args.rounds, args.reps)
    result["parent_clustering_standardize"] = timed(lambda: clustering.standardize(feats), args.rounds, max(1, args.reps // 5))
    result["parent_total_median_ms"] = result["parent_assemble_copy"]["median_ms"] + result["parent_clustering_standardize"]["median_ms"]
    result["speedup_over_parent_path"] = result["parent_total_median_ms"] / result["fit_transform"]["median_ms"]
    # the same calls on a cold cache: how the scaler runs in the workflow, once on fresh data
    flush = torch.zeros(1 << 28, dtype=torch.int32, device=dev)
    z_cold = torch.empty(N, F, dtype=torch.float32, device=dev)
    cold = dict(fit=timed_cold(lambda: ops.standardize_fit(parts, mean_out=mean, var_out=var, scale_out=scale, work=work), flush),
                apply=timed_cold(lambda: ops.standardize_apply(parts, mean, scale, out=z_cold), flush),
                fit_transform=timed_cold(lambda: clustering.StandardScaler().fit_transform(parts), flush),
                parent_assemble_copy=timed_cold(lambda: assemble(feats), flush),
                parent_clustering_standardize=timed_cold(lambda: clustering.standardize(feats), flush))
    cold["fit"]["GBps"] = fit_bytes / (cold["fit"]["median_ms"] * 1e-3) / 1e9
    cold["apply"]["GBps"] = apply_bytes / (cold["apply"]["median_ms"] * 1e-3) / 1e9
    cold["speedup_over_parent_path"] = (cold["parent_assemble_copy"]["median_ms"] + cold["parent_clustering_standardize"]["median_ms"]) \
        / cold["fit_transform"]["median_ms"]
    result["cold_cache"] = cold
    del feats, work, flush, z_cold
    result["peak_extra_bytes"] = dict(
        fit_transform=peak_extra_bytes(lambda: clustering.StandardScaler().fit_transform(parts)),
        parent_assemble_and_standardize=peak_extra_bytes(lambda: clustering.standardize(assemble())),
        z_bytes=4 * N * F)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
