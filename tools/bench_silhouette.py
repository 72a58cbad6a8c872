#!/usr/bin/env python3
"""Device time of mmvae_silhouette_samples at the evaluation shape -- the validation rows of evaluate.py's default split (52 429),
standardised features of width 1 354 (RNA | DNA, fp32) and 782 (RNA, fp32 and padded bf16 rows), the 24 uniform sites of
trainer.synthetic_dataset as labels -- beside, from the same run on the same matrix:
  (a) ops.knn_search(x, x, 1, shift, dist2=False): the same distance GEMM with the top-k epilogue the k-NN search has,
  (b) what a user would write today with stock torch: torch.cdist over chunks of rows followed by @ one_hot(labels), in fp32,
  (c) sklearn.metrics.silhouette_samples on the host for the first 2 048 rows only (its cost grows with the square of the rows).

Times are device events around ONE call (norms + main [+ finish] launches; a call takes tenths of a second, far above the enqueue
cost), median / min / max over `--rounds` calls after a warm-up one.  Reported per case: the time, TFLOP/s taking 2 N^2 F flops, the
share of the 155 TFLOP/s that v_mfma_f32_16x16x4_f32 measures on this card (MI355X_MICROARCH.md), and the ratios to (a) and (b).
Before anything is timed the kernel's samples are compared with the torch formulation's (float32, so the last digits differ; above
1e-3 the run ends).  ONE JSON object is printed, and written to --out if given."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-los-angeles_amd")]

import torch  # noqa: E402

MFMA_F32_PEAK = 155e12


def torch_silhouette(x, labels, n_classes, chunk):
    """silhouette samples with stock ops in fp32: per chunk of rows one cdist and one matmul with the one-hot labels"""
    onehot = torch.nn.functional.one_hot(labels, n_classes).float()
    counts = onehot.sum(0)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    for lo in range(0, x.shape[0], chunk):
        S = torch.cdist(x[lo:lo + chunk], x) @ onehot
        own = onehot[lo:lo + chunk].bool()
        n_own = counts[labels[lo:lo + chunk]]
        a = S[own] / (n_own - 1).clamp(min=1)
        b = (S / counts).masked_fill(own | (counts == 0), float("inf")).min(1)[0]
        out[lo:lo + chunk] = torch.where(n_own > 1, torch.nan_to_num((b - a) / torch.maximum(a, b)), torch.zeros_like(a))
    return out


def timed(fn, rounds, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=52429)
    ap.add_argument("--sites", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=2048, help="rows per cdist of the torch formulation")
    ap.add_argument("--host-rows", type=int, default=2048, help="rows of the sklearn comparator (0 = skip)")
    ap.add_argument("--no-comparators", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_silhouette.py needs an MI355X: the product path has no CPU fallback")
    from mmvae import clustering, ops, to_bf16_rows
    from src.config import Config
    from trainer import synthetic_dataset

    dev = torch.device("cuda", 0)
    N, C = args.rows, args.sites
    tpm, beta_v, site = synthetic_dataset(N, 782, 572, C, Config.RANDOM_SEED)
    site = site.to(dev)
    order, class_start = clustering._encode(site, N, dev)
    C = class_start.numel() - 1
    result = dict(rows=N, classes=C, rounds=args.rounds, mfma_f32_peak_TFLOPs=MFMA_F32_PEAK / 1e12, splits=ops.silhouette_splits(N, C, 0),
                  knn_splits=ops.knn_splits(N, N)[0], cases=[])
    for F, feats in ((782 + 572, torch.cat([tpm, beta_v], 1)), (782, tpm)):
        x32 = clustering.standardize(feats.to(dev))
        shift = x32.double().mean(0).float()
        flops = 2.0 * N * N * F
        ref = None if args.no_comparators else torch_silhouette(x32, site, C, args.chunk)
        for storage, x in (("fp32", x32),) + ((("bf16_rows", to_bf16_rows(x32)),) if F == 782 else ()):
            case = dict(width=F, storage=storage)
            run = lambda: ops.silhouette_samples(x, order, class_start, shift)  # noqa: E731
            s = run()[0]
            case["score"] = float(s.double().mean())
            if ref is not None and storage == "fp32":
                case["max_abs_diff_to_torch"] = float((s - ref).abs().max())
                if not case["max_abs_diff_to_torch"] <= 1e-3:
                    raise SystemExit(f"bench_silhouette: samples differ from the torch formulation's by {case['max_abs_diff_to_torch']:.3e} at width {F}")
            tm = timed(run, args.rounds)
            rate = flops / (tm["median_ms"] * 1e-3)
            case["kernel"] = dict(tm, TFLOPs=rate / 1e12, share_of_mfma_f32=rate / MFMA_F32_PEAK)
            if not args.no_comparators:
                tk = timed(lambda: ops.knn_search(x, x, 1, shift, dist2=False), args.rounds)
                case["knn_search_k1"] = dict(tk, kernel_over_this=tm["median_ms"] / tk["median_ms"])
                if storage == "fp32":
                    tt = timed(lambda: torch_silhouette(x, site, C, args.chunk), args.rounds)
                    case["torch_cdist_onehot"] = dict(tt, chunk=args.chunk, times_kernel=tt["median_ms"] / tm["median_ms"])
            result["cases"].append(case)
        if not args.no_comparators and args.host_rows > 0:
            from sklearn.metrics import silhouette_samples
            R = min(args.host_rows, N)
            xh, lh = x32[:R].cpu().numpy(), site[:R].cpu().numpy()
            t0 = time.perf_counter()
            sk = silhouette_samples(xh, lh)
            host_ms = (time.perf_counter() - t0) * 1e3
            sub_order, sub_start = clustering._encode(site[:R], R, dev)
            got = ops.silhouette_samples(x32[:R], sub_order, sub_start, shift)[0].cpu().numpy()
            result["cases"][-1 if F != 782 else -2]["sklearn_host"] = dict(rows=R, ms=host_ms, max_abs_diff=float(abs(got - sk).max()),
                                                                           ms_scaled_to_all_rows=host_ms * (N / R) ** 2)
        del x32
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
