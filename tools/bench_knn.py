#!/usr/bin/env python3
"""Device time of mmvae_knn_search at the evaluation shape -- the validation rows of evaluate.py's default split (52 429) against its
training rows (209 715), widths 782 (RNA) and 572 (DNA), k 5 and 50, fp32 and padded-bf16-rows storage -- beside what a user would
write today with stock torch on the same card: matmul + topk over chunks of training rows that fit memory, merged by a second topk.

Times are device events around ONE search (norms + search [+ merge] launches; a search takes tenths of a second, far above the
enqueue cost), median / min / max over `--rounds` searches after a warm-up one.  Reported per case: the time, the share of the
155 TFLOP/s that v_mfma_f32_16x16x4_f32 measures on this card (MI355X_MICROARCH.md) taking 2 Mq Nt F flops, and for the cost of
the selection the same distances at k = 1 (fp32 rows).  Before anything is timed the kernel's neighbour sets of the first
`--check-rows` queries are compared with the torch formulation's (float32 GEMM form, so sets may differ at near ties; below 99 %
identical sets the run ends).  ONE JSON object is printed, and written to --out if given."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-los-angeles_amd")]

import torch  # noqa: E402

MFMA_F32_PEAK = 155e12


def torch_knn(q, t, k, chunk):
    """the k nearest by |t|^2 - 2 q.t with stock ops: per chunk of training rows one matmul and one topk, the running best merged"""
    best_v = best_i = None
    for lo in range(0, t.shape[0], chunk):
        tc = t[lo:lo + chunk].float()
        key = (tc * tc).sum(1)[None, :] - 2.0 * (q.float() @ tc.t())
        v, i = torch.topk(key, min(k, tc.shape[0]), dim=1, largest=False)
        i = i + lo
        if best_v is not None:
            v, i = torch.cat([best_v, v], 1), torch.cat([best_i, i], 1)
            v, sel = torch.topk(v, k, dim=1, largest=False)
            i = torch.gather(i, 1, sel)
        best_v, best_i = v, i
    return best_i, best_v


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
    ap.add_argument("--queries", type=int, default=52429)
    ap.add_argument("--train", type=int, default=209715)
    ap.add_argument("--widths", type=int, nargs="+", default=[782, 572])
    ap.add_argument("--ks", type=int, nargs="+", default=[5, 50])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=8192, help="training rows per matmul of the torch formulation")
    ap.add_argument("--check-rows", type=int, default=512)
    ap.add_argument("--no-comparators", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py needs an MI355X: the product path has no CPU fallback")
    from mmvae import ops, to_bf16_rows

    dev = torch.device("cuda", 0)
    Mq, Nt = args.queries, args.train
    result = dict(queries=Mq, train=Nt, rounds=args.rounds, mfma_f32_peak_TFLOPs=MFMA_F32_PEAK / 1e12, splits=ops.knn_splits(Mq, Nt)[0], cases=[])
    for F in args.widths:
        g = torch.Generator(device=dev).manual_seed(F)
        t32 = torch.randn(Nt, F, device=dev, generator=g).abs()
        q32 = torch.randn(Mq, F, device=dev, generator=g).abs()
        shift = t32.double().mean(0).float()
        flops = 2.0 * Mq * Nt * F
        R = min(args.check_rows, Mq)
        ref_i, _ = torch_knn(q32[:R] - shift, t32 - shift, max(args.ks), args.chunk)
        for storage, q, t in (("fp32", q32, t32), ("bf16_rows", to_bf16_rows(q32), to_bf16_rows(t32))):
            for k in args.ks + ([1] if storage == "fp32" else []):
                case = dict(width=F, storage=storage, k=k)
                if storage == "fp32":
                    got = ops.knn_search(q[:R], t, k, shift, dist2=False)[0].long()
                    same = (got.sort(1)[0] == ref_i[:, :k].sort(1)[0]).all(1).double().mean().item()
                    case["sets_identical_to_torch"] = same
                    if same < 0.99:
                        raise SystemExit(f"bench_knn: only {same:.4f} of the neighbour sets equal the torch formulation's at width {F}, k {k}")
                tm = timed(lambda: ops.knn_search(q, t, k, shift), args.rounds)
                rate = flops / (tm["median_ms"] * 1e-3)
                case["kernel"] = dict(tm, TFLOPs=rate / 1e12, share_of_mfma_f32=rate / MFMA_F32_PEAK)
                if not args.no_comparators and storage == "fp32" and k != 1:
                    tt = timed(lambda: torch_knn(q, t, k, args.chunk), args.rounds)
                    case["torch_matmul_topk"] = dict(tt, chunk=args.chunk, times_kernel=tt["median_ms"] / tm["median_ms"])
                result["cases"].append(case)
        del t32, q32
    by = {(c["width"], c["storage"], c["k"]): c["kernel"]["median_ms"] for c in result["cases"]}
    result["selection_cost"] = [dict(width=F, k1_ms=by[(F, "fp32", 1)], **{f"k{k}_over_k1": by[(F, "fp32", k)] / by[(F, "fp32", 1)] for k in args.ks})
                                for F in args.widths]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
