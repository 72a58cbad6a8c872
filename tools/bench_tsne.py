#!/usr/bin/env python3
"""Device time of the t-SNE kernels at the evaluation shape -- the validation rows of evaluate.py's default split (52 429), a 50-column
input as PCA(50) leaves it, 24 sites -- beside, from the same run:
  (a) what a user would write today with stock torch: the dense gradient over chunks of rows (broadcast differences, 1 / (1 + d^2), two
      reductions) and the attraction by gathers over the same CSR P,
  (b) sklearn.manifold.TSNE (Barnes-Hut, angle 0.5) on the host for the first 4 096 rows only.

Times are device events, median / min / max over `--rounds` windows after a warm-up one; a window is `--iters` iterations of the timed
call for the per-iteration kernels (they take about a millisecond) and ONE call for the neighbour search, the affinities and the whole
fit.  Reported: milliseconds per iteration of mmvae_tsne_gradient (both launches), of the same call over an empty P (the repulsion launch
and the second launch's sum of the partials: the difference is the walk over P's entries) and of mmvae_tsne_update; the repulsion's
pairs per second beside the issue-rate estimate (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz / 13 issue cycles per pair: 9 fp32 operations
and a quarter-rate reciprocal); the search (k = 92), the affinities and the symmetrisation once; fit_transform.  Before anything is
timed the kernel's gradient is compared with the torch formulation's (above 1e-4 of its largest entry the run ends).
--parent-tree DIR: also run tools/bench_knn.py (--no-comparators, k 5 and 50) of this tree and of the built tree at DIR, each in a child
process, and record both: the k <= 64 search must not have become slower when MMVAE_KNN_MAXK grew.
ONE JSON object is printed, and written to --out if given."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-los-angeles_amd")]

import torch  # noqa: E402

LANES_PER_SECOND = 256 * 4 * 16 * 2.4e9
CYCLES_PER_PAIR = 13.0


def torch_gradient(Y, row_ptr, col, val, exaggeration, chunk):
    """the same gradient with stock ops in fp32, `chunk` rows at a time"""
    N = Y.shape[0]
    R = torch.empty_like(Y)
    Z = torch.zeros((), dtype=torch.float64, device=Y.device)
    for lo in range(0, N, chunk):
        diff = Y[lo:lo + chunk, None, :] - Y[None, :, :]
        w = 1.0 / (1.0 + (diff * diff).sum(2))
        idx = torch.arange(lo, min(lo + chunk, N), device=Y.device)
        w[idx - lo, idx] = 0.0
        Z += w.sum(dtype=torch.float64)
        R[lo:lo + chunk] = ((w * w)[:, :, None] * diff).sum(1)
    rows = torch.repeat_interleave(torch.arange(N, device=Y.device), (row_ptr[1:] - row_ptr[:-1]).long())
    d = Y[rows] - Y[col.long()]
    pw = val / (1.0 + (d * d).sum(1))
    A = torch.zeros_like(Y).index_add_(0, rows, pw[:, None] * d)
    return 4.0 * (exaggeration * A - R / Z.float())


def timed(fn, rounds, iters=1, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def knn_bench(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "tools", "bench_knn.py"), "--no-comparators", "--ks", "5", "50"], check=True,
                         capture_output=True, text=True, cwd=tree).stdout
    cases = json.loads(out.strip().splitlines()[-1])["cases"]
    return [dict(width=c["width"], storage=c["storage"], k=c["k"], **{k: c["kernel"][k] for k in ("median_ms", "min_ms", "max_ms")}) for c in cases]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=52429)
    ap.add_argument("--width", type=int, default=50)
    ap.add_argument("--sites", type=int, default=24)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20, help="iterations per window of the per-iteration kernels")
    ap.add_argument("--chunk", type=int, default=1024, help="rows per block of the torch formulation")
    ap.add_argument("--host-rows", type=int, default=4096, help="rows of the sklearn comparator (0 = skip)")
    ap.add_argument("--no-comparators", action="store_true")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsne.py needs an MI355X: the product path has no CPU fallback")
    from mmvae import ops, tsne

    dev = torch.device("cuda", 0)
    N, F = args.rows, args.width
    g = torch.Generator(device=dev).manual_seed(0)
    centres = 4.0 * torch.randn(args.sites, F, device=dev, generator=g)
    X = (centres[torch.arange(N, device=dev) % args.sites] + torch.randn(N, F, device=dev, generator=g)).contiguous()
    k = min(N - 1, int(3.0 * args.perplexity + 1))
    result = dict(rows=N, width=F, sites=args.sites, perplexity=args.perplexity, neighbours=k, rounds=args.rounds, iters=args.iters,
                  splits=ops.tsne_gradient_splits(N), pairs=N * (N - 1.0), estimate_pairs_per_s=LANES_PER_SECOND / CYCLES_PER_PAIR)

    result["neighbour_search"] = timed(lambda: tsne.conditional_neighbours(X, k), args.rounds)
    idx, d2 = tsne.conditional_neighbours(X, k)
    result["affinities"] = timed(lambda: ops.tsne_affinities(d2, args.perplexity), args.rounds)
    p_cond, _ = ops.tsne_affinities(d2, args.perplexity)
    result["symmetrisation_torch"] = timed(lambda: tsne.joint_probabilities(idx, p_cond), args.rounds)
    P = tsne.joint_probabilities(idx, p_cond)
    result["nnz"] = int(P[1].numel())
    empty = (torch.zeros(N + 1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, device=dev))

    Y = (3.0 * torch.randn(N, 2, device=dev, generator=g)).contiguous()
    grad = ops.tsne_gradient(Y, *P, 1.0)[0]
    if not args.no_comparators:
        ref = torch_gradient(Y, *P, 1.0, args.chunk)
        result["max_diff_to_torch_over_largest"] = float((grad - ref).abs().max() / ref.abs().max())
        if not result["max_diff_to_torch_over_largest"] <= 1e-4:
            raise SystemExit(f"bench_tsne: the gradient differs from the torch formulation's by {result['max_diff_to_torch_over_largest']:.3e}")
    work = ops._workspace(ops.tsne_gradient_work_bytes(N), dev)
    out = torch.empty_like(Y)
    tg = timed(lambda: ops.tsne_gradient(Y, *P, 1.0, grad_out=out, work=work), args.rounds, args.iters)
    te = timed(lambda: ops.tsne_gradient(Y, *empty, 1.0, grad_out=out, work=work), args.rounds, args.iters)
    tk = timed(lambda: ops.tsne_gradient(Y, *P, 1.0, error=True, grad_out=out, work=work), args.rounds, args.iters)
    rate = result["pairs"] / (te["median_ms"] * 1e-3)
    result["gradient"] = tg
    result["gradient_with_error"] = tk
    result["gradient_empty_P"] = dict(te, pairs_per_s=rate, share_of_estimate=rate / result["estimate_pairs_per_s"])
    upd, gains, Yu = torch.zeros_like(Y), torch.ones_like(Y), Y.clone()
    uwork = ops._workspace(ops.tsne_update_work_bytes(N), dev)
    result["update"] = timed(lambda: ops.tsne_update(Yu, upd, gains, grad, 0.8, 1.0, work=uwork), args.rounds, args.iters)
    result["update_with_norm"] = timed(lambda: ops.tsne_update(Yu, upd, gains, grad, 0.8, 1.0, grad_norm=True, work=uwork), args.rounds, args.iters)
    if not args.no_comparators:
        tt = timed(lambda: torch_gradient(Y, *P, 1.0, args.chunk), args.rounds)
        result["torch_dense_gradient"] = dict(tt, chunk=args.chunk, times_kernel=tt["median_ms"] / tg["median_ms"])
    if not args.no_fit:
        model = tsne.TSNE(perplexity=args.perplexity, random_state=42)
        tf = timed(lambda: model.fit_transform(X), args.rounds)
        result["fit_transform"] = dict(tf, n_iter=model.n_iter_, kl_divergence=model.kl_divergence_, learning_rate=model.learning_rate_)
        if "torch_dense_gradient" in result:
            result["fit_transform"]["torch_gradients_alone_ms"] = result["torch_dense_gradient"]["median_ms"] * (model.n_iter_ + 1)
    if not args.no_comparators and args.host_rows > 0:
        from sklearn.manifold import TSNE
        R = min(args.host_rows, N)
        xh = X[:R].cpu().numpy()
        t0 = time.perf_counter()
        sk = TSNE(2, perplexity=args.perplexity, random_state=42).fit(xh)
        host_ms = (time.perf_counter() - t0) * 1e3
        sub = tsne.TSNE(perplexity=args.perplexity, random_state=42)
        ts = timed(lambda: sub.fit_transform(X[:R]), 1)
        result["sklearn_host"] = dict(rows=R, ms=host_ms, kl_divergence=float(sk.kl_divergence_), device_ms_same_rows=ts["median_ms"],
                                      device_kl_divergence=sub.kl_divergence_)
    if args.parent_tree:
        result["knn_search_this_commit"] = knn_bench(ROOT)
        result["knn_search_parent"] = knn_bench(os.path.abspath(args.parent_tree))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
