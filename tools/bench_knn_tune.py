#!/usr/bin/env python3
"""Device time of the tuned k-NN baseline (mmvae.knn.optimize_knn) at the evaluation shape -- the validation rows of evaluate.py's
default split (52 429) against its training rows (209 715), RNA (782) -> DNA (572), fp32 rows:

  searches   mmvae_knn_search_l1 at k = 50 beside mmvae_knn_search at k = 50, and a chunked torch.cdist(p=1) + topk on the same card;
  regression mmvae_knn_weighted_rows (k = 50, 572 outputs) beside the y[idx]-based torch formulation;
  grid       the whole 16-point grid through optimize_knn (two searches) beside 16 independent fit / predict pairs;
  sklearn    KNeighborsRegressor(50, weights='distance', metric='manhattan') on the CPU at a REDUCED shape (--sk-queries x --sk-train,
             stated in the output), and the device on that same reduced shape.

The L1 search is VALU work: 2 Mq Nt F lane operations (a subtract and an add with |.| per pair and column).  Its rate is reported
against the fp32 vector peak of MI355X_MICROARCH.md (157.3 TFLOP/s, which counts an FMA as two: a subtract and an add cannot fuse, so
78.65 T lane operations / s is the most this instruction mix can reach).  No target is fixed; the numbers are recorded.
--parent-lib PATH: a libmmvae_hip.so built from the parent commit (with the entry points it lacks stubbed).  The euclidean search is
then timed in fresh child processes, parent and branch alternating --alternations times on the same card, and both series are recorded
(is the euclidean search as fast as it was?).  Times are device events around one call, median / min / max over --rounds after a
warm-up.  ONE JSON object is printed, and written to --out if given."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-los-angeles_amd")]

FP32_VECTOR_PEAK = 157.3e12       # MI355X_MICROARCH.md: FLOP/s with an FMA counted as two


def timed(fn, rounds, warmup=1):
    import torch
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


def data(Mq, Nt, F, Fy, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(F)
    t = torch.randn(Nt, F, device=dev, generator=g).abs()
    q = torch.randn(Mq, F, device=dev, generator=g).abs()
    w = torch.randn(F, Fy, device=dev, generator=g) / F ** 0.5
    return q, t, (q @ w + 0.1 * torch.randn(Mq, Fy, device=dev, generator=g)), (t @ w + 0.1 * torch.randn(Nt, Fy, device=dev, generator=g))


def torch_l1(q, t, k, chunk):
    """the k nearest under L1 with stock ops: per chunk of training rows one cdist(p=1) and one topk, the running best merged"""
    import torch
    best_v = best_i = None
    for lo in range(0, t.shape[0], chunk):
        v, i = torch.topk(torch.cdist(q, t[lo:lo + chunk], p=1.0), min(k, t.shape[0] - lo), dim=1, largest=False)
        i = i + lo
        if best_v is not None:
            v, i = torch.cat([best_v, v], 1), torch.cat([best_i, i], 1)
            v, sel = torch.topk(v, k, dim=1, largest=False)
            i = torch.gather(i, 1, sel)
        best_v, best_i = v, i
    return best_i, best_v


def torch_weighted(idx, dist, y):
    """sklearn's weights='distance' with stock ops: materialises the (Mq, k, Fy) gather"""
    import torch
    zero = dist == 0
    w = torch.where(zero.any(1, keepdim=True), zero.float(), 1.0 / dist)
    return (y[idx.long()] * w[:, :, None]).sum(1) / w.sum(1, keepdim=True)


def euclid_only(args):
    """child process: the euclidean search alone with whatever library MMVAE_LIB_PATH names"""
    import torch
    from mmvae import ops
    dev = torch.device("cuda", 0)
    q, t, _, _ = data(args.queries, args.train, args.width, 1, dev)
    shift = t.double().mean(0).float()
    out = {f"k{k}": timed(lambda: ops.knn_search(q, t, k, shift), args.rounds) for k in (5, 50)}
    print("EUCLID " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=52429)
    ap.add_argument("--train", type=int, default=209715)
    ap.add_argument("--width", type=int, default=782)
    ap.add_argument("--outputs", type=int, default=572)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=8192, help="training rows per cdist of the torch formulation")
    ap.add_argument("--sk-queries", type=int, default=1024)
    ap.add_argument("--sk-train", type=int, default=8192)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--no-comparators", action="store_true")
    ap.add_argument("--euclid-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.euclid_only:
        return euclid_only(args)

    Mq, Nt, F, Fy = args.queries, args.train, args.width, args.outputs
    result = dict(queries=Mq, train=Nt, width=F, outputs=Fy, rounds=args.rounds, fp32_vector_peak_TFLOPs=FP32_VECTOR_PEAK / 1e12,
                  lane_op_ceiling_T_per_s=FP32_VECTOR_PEAK / 2e12)
    if args.parent_lib:
        # before this process opens the device: fresh children, parent and branch alternating on the same card
        series = {"parent": [], "branch": []}
        for _ in range(args.alternations):
            for who in ("parent", "branch"):
                env = dict(os.environ)
                env.pop("MMVAE_LIB_PATH", None)
                if who == "parent":
                    env["MMVAE_LIB_PATH"] = os.path.abspath(args.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--euclid-only", "--queries", str(Mq), "--train", str(Nt), "--width", str(F),
                       "--rounds", str(args.rounds)]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    raise SystemExit(f"bench_knn_tune: the {who} child failed ({p.returncode}): {p.stderr[-2000:]}")
                series[who].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("EUCLID ")][-1][7:]))
        result["euclidean_search_parent_vs_branch"] = {
            who: {k: dict(run_medians_ms=[r[k]["median_ms"] for r in runs], median_ms=statistics.median(r[k]["median_ms"] for r in runs),
                          spread_ms=max(r[k]["median_ms"] for r in runs) - min(r[k]["median_ms"] for r in runs)) for k in ("k5", "k50")}
            for who, runs in series.items()}

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn_tune.py needs an MI355X: the product path has no CPU fallback")
    from mmvae import ops
    from mmvae.knn import GRID, KNeighborsRegressor, optimize_knn
    dev = torch.device("cuda", 0)
    q, t, yq, yt = data(Mq, Nt, F, Fy, dev)
    shift = t.double().mean(0).float()
    lane_ops = 2.0 * Mq * Nt * F

    # searches
    R = min(256, Mq)
    got = ops.knn_search_l1(q[:R], t, 50)
    if not args.no_comparators:
        ref_i, ref_v = torch_l1(q[:R], t, 50, args.chunk)
        same = (got[0].long().sort(1)[0] == ref_i.sort(1)[0]).all(1).double().mean().item()
        result["l1_sets_identical_to_torch_cdist"] = same
        if same < 0.99:
            raise SystemExit(f"bench_knn_tune: only {same:.4f} of the L1 neighbour sets equal torch.cdist's")
    l1 = timed(lambda: ops.knn_search_l1(q, t, 50), args.rounds)
    l1_k5 = timed(lambda: ops.knn_search_l1(q, t, 5), args.rounds)
    l2 = timed(lambda: ops.knn_search(q, t, 50, shift), args.rounds)
    rate = lane_ops / (l1["median_ms"] * 1e-3)
    result["search_k50"] = dict(
        l1=dict(l1, lane_ops_T_per_s=rate / 1e12, share_of_fp32_vector_peak=rate / FP32_VECTOR_PEAK, share_of_lane_op_ceiling=2 * rate / FP32_VECTOR_PEAK),
        l1_k5=l1_k5, euclidean=dict(l2, l1_over_euclidean=l1["median_ms"] / l2["median_ms"]), splits=ops.knn_splits(Mq, Nt)[0])
    if not args.no_comparators:
        tc = timed(lambda: torch_l1(q, t, 50, args.chunk), 1, warmup=0)
        result["search_k50"]["torch_cdist_topk"] = dict(tc, chunk=args.chunk, rounds=1, times_kernel=tc["median_ms"] / l1["median_ms"])

    # regression
    idx, dist = ops.knn_search_l1(q, t, 50)
    out = torch.empty(Mq, Fy, device=dev)
    wr = timed(lambda: ops.knn_weighted_rows(idx, dist, yt, False, out), args.rounds)
    mr = timed(lambda: ops.knn_mean_rows(idx, yt, out), args.rounds)
    nbytes = Mq * 50 * (8 + 4 * Fy) + 4 * Mq * Fy
    result["weighted_rows_k50"] = dict(kernel=dict(wr, GBps=nbytes / (wr["median_ms"] * 1e-3) / 1e9), mean_rows=mr)
    if not args.no_comparators:
        tw = timed(lambda: torch_weighted(idx, dist, yt), args.rounds)
        err = (torch_weighted(idx[:R], dist[:R], yt) - ops.knn_weighted_rows(idx[:R], dist[:R], yt, False)).abs().max().item()
        result["weighted_rows_k50"]["torch_gather"] = dict(tw, times_kernel=tw["median_ms"] / wr["median_ms"], max_abs_difference=err)

    # the grid
    def independent():
        for k in GRID["n_neighbors"]:
            for w in GRID["weights"]:
                for m in GRID["metric"]:
                    KNeighborsRegressor.from_params(k, w, m).fit(t, yt).predict(q)
    tg = timed(lambda: optimize_knn(t, yt, q, yq), args.rounds)
    ti = timed(independent, 1, warmup=0)
    _, params, grid = optimize_knn(t, yt, q, yq)
    result["grid_16_points"] = dict(optimize_knn=tg, independent_fits=dict(ti, rounds=1, times_optimize_knn=ti["median_ms"] / tg["median_ms"]),
                                    winner=params, mse=[m for _, m in grid])

    # sklearn on the CPU, reduced shape
    if not args.no_comparators:
        try:
            from sklearn.neighbors import KNeighborsRegressor as SK
        except ImportError:
            result["sklearn_cpu_reduced"] = "sklearn is not installed: not measured"
        else:
            sq, st_ = q[:args.sk_queries], t[:args.sk_train]
            Xs, Ys, Xqs = st_.cpu().numpy(), yt[:args.sk_train].cpu().numpy(), sq.cpu().numpy()
            t0 = time.perf_counter()
            want = SK(50, weights="distance", metric="manhattan").fit(Xs, Ys).predict(Xqs)
            cpu_s = time.perf_counter() - t0
            reg = KNeighborsRegressor.from_params(50, "distance", "manhattan").fit(st_, yt[:args.sk_train])
            td = timed(lambda: reg.predict(sq), args.rounds)
            diff = (torch.from_numpy(want).to(dev) - reg.predict(sq)).abs()      # fp32 near-ties at the 50th neighbour swap a row here and there
            result["sklearn_cpu_reduced"] = dict(queries=args.sk_queries, train=args.sk_train, width=F, cpu_threads=os.environ.get("OMP_NUM_THREADS"),
                                                 sklearn_fit_predict_s=cpu_s, device_predict=td, max_abs_difference=float(diff.max()),
                                                 median_abs_difference=float(diff.median()),
                                                 times_device=cpu_s * 1e3 / td["median_ms"])
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
