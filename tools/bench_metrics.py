#!/usr/bin/env python3
"""Device time of mmvae_recon_metrics at the training batch (65 536 rows) and the two model widths (782 RNA, 572 DNA), fp32 and
padded-bf16-rows targets against an fp32 prediction, beside its comparators (this code has no earlier version to compare with):

  torch   the same metrics written with stock torch ops on the device (float64 casts, centred Pearson, row norms, column sums)
  host    the reference's route: copy both matrices to the host, sklearn.metrics + the diagonal of cosine_similarity + a loop of
          scipy.stats.pearsonr -- on `--host-rows` rows only (default 2048): cosine_similarity builds a rows x rows matrix, 34 GB of
          float64 at 65 536 rows.  Skipped where sklearn / scipy do not import.

Times are device events around `--launches` back-to-back launches (the kernel takes several times the host's enqueue cost, so the
queue stays full; 500 launches = 50-80 ms per round), median / min / max over `--rounds` rounds after a warm-up.  Consecutive
launches read DIFFERENT copies of the operands, enough copies for 1 GiB in rotation, so that no launch finds its input in the
256 MB Infinity Cache from the launch before.  Bytes are the algorithmic ones from the shapes (both operands read once, the two
row vectors written, col_acc read and written); the share is of the 6.3 TB/s achievable HBM rate (MI355X_MICROARCH.md).
Before anything is timed the kernel's outputs AT THE TIMED SIZE are compared with the torch formulation (float64): the column
sums within (rows + 3) 2^-52 of the sum of their terms' magnitudes, r and the cosine within 2^-22 (their fp32 store and the
float64 reference's own rounding); a mismatch ends the run.  ONE JSON object is printed, and written to --out if given.

Kernel time from the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats -d prof_metrics -o run -- python tools/bench_metrics.py --rounds 1 --no-comparators
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-los-angeles_amd")]

import torch  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def torch_metrics(y, p, shift=None):
    """the metrics with stock torch ops, float64 like the kernel's sums"""
    y, p = y.double(), p.double()
    d = p - y
    t = y if shift is None else y - shift.double()
    out = [d.abs().sum(0), (d * d).sum(0), t.sum(0), (t * t).sum(0)]
    yc, pc = y - y.mean(1, keepdim=True), p - p.mean(1, keepdim=True)
    out.append((yc * pc).sum(1) / ((yc * yc).sum(1).sqrt() * (pc * pc).sum(1).sqrt()))
    out.append((y * p).sum(1) / (y.norm(dim=1).clamp_min(1e-300) * p.norm(dim=1).clamp_min(1e-300)))
    return out


def host_metrics(y, p):
    from scipy.stats import pearsonr
    from sklearn.metrics import mean_absolute_error, mean_squared_error, r2_score
    from sklearn.metrics.pairwise import cosine_similarity
    y, p = y.cpu().float().numpy(), p.cpu().float().numpy()                   # the copies are part of the route
    yf, pf = y.flatten(), p.flatten()
    out = [mean_absolute_error(yf, pf), mean_squared_error(yf, pf), r2_score(yf, pf), cosine_similarity(y, p).diagonal().mean()]
    out.append([pearsonr(y[i], p[i])[0] for i in range(len(y))])
    return out


def check_outputs(ops, target, pred, shift):
    """the kernel at the timed size against the torch formulation; raises on a mismatch, returns the largest deviations"""
    M, F = target.shape
    col = torch.zeros(4, F, dtype=torch.float64, device=target.device)
    rp, rc = torch.empty(M, device=target.device), torch.empty(M, device=target.device)
    ops.recon_metrics(pred, target, shift, col, rp, rc)
    s_abs, s_res, s0, s1, r, cos = torch_metrics(target, pred, shift)
    y, p = target.double(), pred.double()
    mags = torch.stack([(y - shift.double()).abs().sum(0), s1, s_res, s_abs])
    err = (col - torch.stack([s0, s1, s_res, s_abs])).abs()
    rel = float((err / mags.clamp_min(1e-300)).max())
    e_r, e_c = float((rp.double() - r).abs().max()), float((rc.double() - cos).abs().max())
    if not (rel <= (M + 3) * 2.0 ** -52 and e_r <= 2.0 ** -22 and e_c <= 2.0 ** -22):
        raise SystemExit(f"bench_metrics: kernel output differs from the torch formulation at {M} x {F}: columns {rel:.3e} of their "
                         f"terms, r {e_r:.3e}, cosine {e_c:.3e}")
    return dict(col_rel=rel, pearson_abs=e_r, cosine_abs=e_c)


def timed(fn, launches, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / launches)
    return dict(median_us=1e3 * statistics.median(ms), min_us=1e3 * min(ms), max_us=1e3 * max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--widths", type=int, nargs="+", default=[782, 572])
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-rows", type=int, default=2048)
    ap.add_argument("--no-comparators", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py needs an MI355X: the product path has no CPU fallback")
    from mmvae import ops, to_bf16_rows

    dev = torch.device("cuda", 0)
    M = args.rows
    result = dict(rows=M, launches=args.launches, rounds=args.rounds, hbm_achievable_TBps=HBM_ACHIEVABLE / 1e12, cases=[])
    for F in args.widths:
        g = torch.Generator(device=dev).manual_seed(F)
        y32 = torch.randn(M, F, device=dev, generator=g).abs()
        p32 = y32 + 0.3 * torch.randn(M, F, device=dev, generator=g)
        shift = y32[0].clone()
        col = torch.zeros(4, F, dtype=torch.float64, device=dev)
        rp, rc = torch.empty(M, device=dev), torch.empty(M, device=dev)
        for name, target in (("fp32", y32), ("bf16_rows", to_bf16_rows(y32))):
            nbytes = M * F * (target.element_size() + 4) + 8 * M + 64 * F + 4 * F
            case = dict(width=F, target=name, prediction="fp32", bytes=nbytes)
            case["output_check"] = check_outputs(ops, target, p32, shift)
            copies = max(2, -(-(1 << 30) // nbytes))                              # operands in rotation: 1 GiB before one repeats
            dup = to_bf16_rows if name == "bf16_rows" else torch.clone             # a copy in the same layout (padded rows stay padded)
            sets = [(p32, target)] + [(p32.clone(), dup(target)) for _ in range(copies - 1)]
            case["operand_copies"] = copies
            turn = [0]

            def launch():
                pp, tt_ = sets[turn[0] % copies]
                turn[0] += 1
                ops.recon_metrics(pp, tt_, shift, col, rp, rc)
            with ops.pinned_stream():
                t = timed(launch, args.launches, args.rounds, args.warmup)
            rate = nbytes / (t["median_us"] * 1e-6)
            case["kernel"] = dict(t, GBps=rate / 1e9, share_of_hbm=rate / HBM_ACHIEVABLE)
            del sets
            if not args.no_comparators:
                tt = timed(lambda: torch_metrics(target, p32), 10, 5, 2)
                case["torch_ops"] = dict(tt, times_kernel=tt["median_us"] / t["median_us"])
            result["cases"].append(case)
        if not args.no_comparators:
            try:
                import scipy  # noqa: F401
                import sklearn  # noqa: F401
            except ImportError:
                result.setdefault("host", "sklearn / scipy not importable: not measured")
                continue
            R = min(args.host_rows, M)
            host_metrics(y32[:64], p32[:64])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_metrics(y32[:R], p32[:R])
            dt = time.perf_counter() - t0
            result.setdefault("host", []).append(dict(width=F, rows=R, seconds=dt, us_per_row=1e6 * dt / R,
                                                      note="rows x rows cosine matrix: not runnable at the full row count"))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
