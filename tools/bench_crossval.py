#!/usr/bin/env python3
"""Device time of the fold-masked k-NN search behind mmvae.crossval, beside the loops of plain searches it replaces.

At the rows of `cross_validate.py --subset 0.1` of the trainers' synthetic default (26 214) and at 2 048, widths 782 (RNA) and 572
(DNA), k = 10, 10 folds of kfold_assignments, 24 sites:
  (a) the fold-masked search (ops.knn_search_grouped, differ = fold) | the loop it replaces: one plain ops.knn_search per fold on the
      gathered training rows, gathers included | a plain N x N search of the same shape: the price of the predicate
  (b) same site + other fold (same = site, differ = fold) with the rows sorted by site (tiles of other sites are skipped) | with the
      rows as they come | as the loop of plain searches per (site, fold), gathers included
  (c) a whole cross_validate(models = mean, knn) of one direction (wall clock, synchronised) | sklearn on the CPU at --sklearn-rows
      rows when sklearn is importable
  (d) with --parent-tree DIR (a checkout of the parent commit with its library built): tools/bench_knn.py of this tree and of that
      one, alternating, each in a fresh process; per case the two medians and both spreads
Device events around synchronised work, a warm-up call and --rounds timed ones: median / min / max.  At the timed size the grouped
answer and the loop's are compared on --check-rows sampled rows: indices equal, distance bits equal.  ONE JSON object is printed and
written to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-los-angeles_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


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


def loop_search(ops, X, groups, k, shift):
    """the loop the grouped search replaces: per (query rows, candidate rows) group one plain search on gathered copies; (idx, dist2) in
    the caller's row numbers, -1 / +inf behind a list of fewer than k"""
    N = X.shape[0]
    idx = torch.full((N, k), -1, dtype=torch.int32, device=X.device)
    d2 = torch.full((N, k), float("inf"), dtype=torch.float32, device=X.device)
    for q_rows, c_rows in groups:
        kk = min(k, c_rows.numel())
        if kk == 0 or q_rows.numel() == 0:
            continue
        i, d = ops.knn_search(X[q_rows], X[c_rows], kk, shift)
        idx[q_rows, :kk] = c_rows[i.long()].int()
        d2[q_rows, :kk] = d
    return idx, d2


def same_answer(a, b, rows):
    return bool(torch.equal(a[0][rows], b[0][rows]) and torch.equal(a[1][rows].view(torch.int32), b[1][rows].view(torch.int32)))


def run_ab(parent_tree, rounds):
    """(d): bench_knn.py of the parent's tree and of this one, alternating, each run a fresh process"""
    runs = {"parent": [], "this": []}
    for r in range(rounds):
        for name in (("parent", "this") if r % 2 == 0 else ("this", "parent")):      # who goes first alternates too
            tree = os.path.abspath(parent_tree) if name == "parent" else ROOT
            env = {k: v for k, v in os.environ.items() if k != "MMVAE_LIB_PATH"}
            done = subprocess.run([sys.executable, os.path.join(tree, "tools", "bench_knn.py"), "--no-comparators", "--rounds", "3"], env=env,
                                  capture_output=True, text=True, timeout=600)
            if done.returncode:
                raise SystemExit(f"bench_knn.py of {tree} ended with {done.returncode}:\n{done.stderr[-2000:]}")
            runs[name].append(json.loads(done.stdout.strip().splitlines()[-1]))
    cases = []
    for i, c in enumerate(runs["this"][0]["cases"]):
        row = dict(width=c["width"], storage=c["storage"], k=c["k"])
        for name in ("parent", "this"):
            med = [r["cases"][i]["kernel"]["median_ms"] for r in runs[name]]
            lo = min(r["cases"][i]["kernel"]["min_ms"] for r in runs[name])
            hi = max(r["cases"][i]["kernel"]["max_ms"] for r in runs[name])
            row[name] = dict(median_ms=statistics.median(med), medians_ms=med, min_ms=lo, max_ms=hi)
        row["this_over_parent"] = row["this"]["median_ms"] / row["parent"]["median_ms"]
        row["parent_spread"] = (row["parent"]["max_ms"] - row["parent"]["min_ms"]) / row["parent"]["median_ms"]
        row["within_parent_spread"] = row["parent"]["min_ms"] <= row["this"]["median_ms"] <= row["parent"]["max_ms"] or row["this_over_parent"] <= 1.0
        cases.append(row)
    return dict(queries=runs["this"][0]["queries"], train=runs["this"][0]["train"], processes_per_side=rounds, cases=cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[26214, 2048])
    ap.add_argument("--widths", type=int, nargs="+", default=[782, 572])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--folds", type=int, default=10)
    ap.add_argument("--sites", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check-rows", type=int, default=512)
    ap.add_argument("--sklearn-rows", type=int, default=2048, help="rows of the sklearn comparison of (c); 0 = skip")
    ap.add_argument("--sklearn-jobs", type=int, default=16, help="n_jobs of the sklearn comparison")
    ap.add_argument("--parent-tree", default=None, help="(d): a checkout of the parent commit with its library built")
    ap.add_argument("--ab-rounds", type=int, default=2)
    ap.add_argument("--skip", nargs="*", default=[], choices=["a", "b", "c"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crossval.py needs an MI355X: the product path has no CPU fallback")
    import trainer
    from mmvae import crossval, ops
    from src.config import Config

    dev = torch.device("cuda", 0)
    k, R = args.k, args.rounds
    result = dict(k=k, folds=args.folds, sites=args.sites, rounds=R, shapes=[])
    for N in args.rows:
        tpm, beta_v, site = trainer.synthetic_dataset(N, max(args.widths), min(args.widths), args.sites, Config.RANDOM_SEED)
        fold_h = crossval.kfold_assignments(N, args.folds)
        fold = torch.from_numpy(fold_h).to(dev)
        site32 = site.to(dev).int()
        sample = torch.from_numpy(np.random.default_rng(0).choice(N, min(args.check_rows, N), replace=False)).to(dev)
        for F in args.widths:
            X = (tpm if F == tpm.shape[1] else beta_v)[:, :F].to(dev).contiguous()
            Y = (beta_v if F == tpm.shape[1] else tpm).to(dev).contiguous()
            shift = ops._column_means(X)
            shape = dict(rows=N, width=F, splits=ops.knn_splits(N, N)[0])
            if "a" not in args.skip:
                groups = [(torch.nonzero(fold == f).squeeze(1), torch.nonzero(fold != f).squeeze(1)) for f in range(args.folds)]
                grouped = ops.knn_search_grouped(X, X, k, differ=(fold, fold), shift=shift)
                shape["a"] = dict(
                    identical_on_sample=same_answer(grouped, loop_search(ops, X, groups, k, shift), sample),
                    fold_masked=timed(lambda: ops.knn_search_grouped(X, X, k, differ=(fold, fold), shift=shift), R),
                    loop_of_plain_searches=timed(lambda: loop_search(ops, X, groups, k, shift), R),
                    plain_search_same_shape=timed(lambda: ops.knn_search(X, X, k, shift), R),
                    gathered_copy_bytes_of_the_loop=int(sum(c.numel() for _, c in groups) // args.folds * F * 4))
                a = shape["a"]
                a["loop_over_fold_masked"] = a["loop_of_plain_searches"]["median_ms"] / a["fold_masked"]["median_ms"]
                a["fold_masked_over_plain"] = a["fold_masked"]["median_ms"] / a["plain_search_same_shape"]["median_ms"]
            if "b" not in args.skip:
                order = torch.argsort(site32, stable=True)
                Xs, fs, ss = X[order].contiguous(), fold[order].contiguous(), site32[order].contiguous()
                groups = [(torch.nonzero((site32 == s) & (fold == f)).squeeze(1), torch.nonzero((site32 == s) & (fold != f)).squeeze(1))
                          for s in range(args.sites) for f in range(args.folds)]
                srt = ops.knn_search_grouped(Xs, Xs, k, same=(ss, ss), differ=(fs, fs), shift=shift)
                back = torch.empty_like(srt[0])
                back[order] = torch.where(srt[0] >= 0, order[srt[0].clamp(min=0).long()].int(), srt[0])
                dback = torch.empty_like(srt[1])
                dback[order] = srt[1]
                shape["b"] = dict(
                    identical_on_sample=same_answer((back, dback), loop_search(ops, X, groups, k, shift), sample),
                    site_sorted=timed(lambda: ops.knn_search_grouped(Xs, Xs, k, same=(ss, ss), differ=(fs, fs), shift=shift), R),
                    rows_as_they_come=timed(lambda: ops.knn_search_grouped(X, X, k, same=(site32, site32), differ=(fold, fold), shift=shift), R),
                    loop_per_site_and_fold=timed(lambda: loop_search(ops, X, groups, k, shift), max(2, R // 2)))
                b = shape["b"]
                b["loop_over_site_sorted"] = b["loop_per_site_and_fold"]["median_ms"] / b["site_sorted"]["median_ms"]
                b["as_they_come_over_site_sorted"] = b["rows_as_they_come"]["median_ms"] / b["site_sorted"]["median_ms"]
            if "c" not in args.skip:
                def whole():
                    crossval.cross_validate(X, Y, site, fold_h, "DNA -> RNA", ("mean", "knn"), (5, k))
                    torch.cuda.synchronize()
                whole()
                wall = []
                for _ in range(max(2, R // 2)):
                    t0 = time.perf_counter()
                    whole()
                    wall.append((time.perf_counter() - t0) * 1e3)
                shape["c"] = dict(cross_validate_mean_knn=dict(median_ms=statistics.median(wall), min_ms=min(wall), max_ms=max(wall)))
                if args.sklearn_rows and N <= args.sklearn_rows:
                    try:
                        from sklearn.neighbors import KNeighborsRegressor
                    except ImportError:
                        KNeighborsRegressor = None
                    if KNeighborsRegressor is not None:
                        Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
                        t0 = time.perf_counter()
                        for kk in (5, k):
                            for f in range(args.folds):
                                tr, te = fold_h != f, fold_h == f
                                KNeighborsRegressor(n_neighbors=kk, n_jobs=args.sklearn_jobs).fit(Xh[tr], Yh[tr]).predict(Xh[te])
                        shape["c"]["sklearn_knn_fits_only_ms"] = (time.perf_counter() - t0) * 1e3
                        shape["c"]["sklearn_jobs"] = args.sklearn_jobs
            result["shapes"].append(shape)
            print(json.dumps(shape), file=sys.stderr, flush=True)
    if args.parent_tree:
        result["d"] = run_ab(args.parent_tree, args.ab_rounds)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
