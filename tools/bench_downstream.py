#!/usr/bin/env python3
"""Device time of the downstream task's site classifier at the evaluation shape -- the reference's widths (RNA 782 + DNA 572 = 1354
features for the widest scenario, 24 sites, batches of 32, hidden 256 / 128) and a validation split of `--rows` rows -- from one run:
  kernels   mmvae_ln_act_fwd, mmvae_ln_act_bwd, mmvae_wce_mean (with gradient) and mmvae_adam_step at the training batch (32 rows) and,
            for the two that evaluation launches, at one fold's validation rows; microseconds per call.  At 32 rows these are
            launch-latency numbers: 32 x 256 x 4 bytes is nothing to move.
  step      one training step of SiteClassifier, eager (about 20 launches issued from Python) and as a hipGraph replay, on the same batch
  scenario  cross_validate (5 folds, `--epochs` epochs) on a synthetic set of the evaluation shape, beside the same architecture and
            protocol in stock torch on the same GPU (nn.Sequential, nn.CrossEntropyLoss(weight), torch.optim.Adam, the same folds, the
            same number of epochs, early stopping switched off on both sides so that both run the same number of steps)
Times are device events (kernels, step: median / min / max over `--rounds` windows of `--iters` calls after a warm-up window) or a host
clock around work that ends in a synchronise (scenario).  ONE JSON object is printed, and written to --out if given."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-los-angeles_amd")]

import torch  # noqa: E402


def timed(fn, rounds, iters, warmup=1):
    for _ in range(warmup * iters):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / iters)
    return dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us))


def torch_scenario(z, labels, n_classes, folds, epochs, seed):
    """the same protocol in stock torch on the same device, patience switched off; -> mean accuracy"""
    import numpy as np
    import torch.nn as nn
    from mmvae import downstream
    from trainer import balanced_class_weights
    accs = []
    for fold, (tr, te) in enumerate(folds):
        tr, te = torch.from_numpy(tr).to(z.device), torch.from_numpy(te).to(z.device)
        torch.manual_seed(seed + fold)
        model = nn.Sequential(nn.Linear(z.shape[1], 256), nn.LayerNorm(256), nn.ReLU(), nn.Dropout(0.3), nn.Linear(256, 128), nn.LayerNorm(128),
                              nn.ReLU(), nn.Dropout(0.2), nn.Linear(128, n_classes)).to(z.device)
        crit = nn.CrossEntropyLoss(weight=balanced_class_weights(labels[tr].cpu(), n_classes).to(z.device))
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=5)
        Xtr, ytr, Xva, yva = z[tr], labels[tr], z[te], labels[te]
        for _ in range(epochs):
            model.train()
            perm = torch.randperm(Xtr.shape[0], device=z.device)
            for i in range(0, Xtr.shape[0], 32):
                idx = perm[i:i + 32]
                opt.zero_grad()
                crit(model(Xtr[idx]), ytr[idx]).backward()
                opt.step()
            model.eval()
            with torch.no_grad():
                out = model(Xva)
                losses = [crit(out[i:i + 32], yva[i:i + 32]) for i in range(0, Xva.shape[0], 32)]
                stats = torch.stack([torch.stack(losses).mean(), (out.argmax(1) == yva).sum()]).tolist()      # one read-back per epoch here too
            sched.step(stats[0])
        accs.append(stats[1] / Xva.shape[0])
    return float(np.mean(accs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048, help="rows of the scenario's set (one fold validates on a fifth)")
    ap.add_argument("--features", type=int, default=1354)
    ap.add_argument("--sites", type=int, default=24)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_downstream.py needs an MI355X: nothing here is measured on a CPU")
    from mmvae import _lib, downstream, ops
    from mmvae.clustering import standardize
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    res = dict(device=torch.cuda.get_device_name(0), rows=args.rows, features=args.features, sites=args.sites, batch=32, rounds=args.rounds,
               iters=args.iters, kernels={})

    # ---- the kernels --------------------------------------------------------------------------------------------
    n_val = args.rows // 5
    for M in (32, n_val):
        for N, p in ((256, 0.3), (128, 0.2)):
            z = torch.randn(M, N, generator=g).to(dev)
            gamma, beta = torch.rand(N, generator=g).to(dev) + 0.5, torch.randn(N, generator=g).to(dev)
            mask = (torch.rand(M, N, generator=g) >= p).to(torch.uint8).to(dev)
            y, mean, rstd = ops.ln_act_fwd(z, gamma, beta, mask, p)
            res["kernels"][f"ln_act_fwd M={M} N={N}"] = timed(lambda: ops.ln_act_fwd(z, gamma, beta, mask, p, y_out=y, mean_out=mean, rstd_out=rstd),
                                                              args.rounds, args.iters)
            if M == 32:
                dz, dg, db = ops.ln_act_bwd(y, z, mean, rstd, gamma, beta, mask, p)
                res["kernels"][f"ln_act_bwd M={M} N={N}"] = timed(
                    lambda: ops.ln_act_bwd(y, z, mean, rstd, gamma, beta, mask, p, dz_out=dz, dgamma_out=dg, dbeta_out=db), args.rounds, args.iters)
        logits = torch.randn(M, args.sites, generator=g).to(dev)
        labels = torch.randint(0, args.sites, (M,), generator=g).to(dev)
        w = (torch.rand(args.sites, generator=g) + 0.5).to(dev)
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        if M == 32:
            grad = torch.empty(M, args.sites, device=dev)
            res["kernels"][f"wce_mean(gradient) M={M} C={args.sites}"] = timed(lambda: ops.wce_mean(logits, labels, w, sums=sums, grad_out=grad),
                                                                               args.rounds, args.iters)
        else:
            conf = torch.zeros(args.sites, args.sites, dtype=torch.int32, device=dev)
            pred = torch.empty(M, dtype=torch.int32, device=dev)
            res["kernels"][f"wce_mean(pred, nll, confusion) M={M} C={args.sites}"] = timed(
                lambda: ops.wce_mean(logits, labels, w, sums=sums, pred_out=pred, nll=True, confusion=conf), args.rounds, args.iters)
    net = downstream.SiteClassifier(args.features, args.sites, device=dev, seed=1)
    n_param = net._flat["p"].numel()
    step = torch.zeros(_lib.CTR_COPIES, dtype=torch.int64, device=dev)
    res["kernels"][f"adam_step n={n_param}"] = timed(lambda: ops.adam_step(net._adam_items, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1.0, 1.0, step_dev=step,
                                                                          lr_dev=net._lr), args.rounds, args.iters)
    res["kernels"][f"adam_step n={n_param}"]["bytes"] = 28 * n_param

    # ---- one training step: eager and as graph replay --------------------------------------------------------------
    X = torch.randn(args.rows, args.features, generator=g).to(dev)
    y = torch.randint(0, args.sites, (args.rows,), generator=g).to(dev)
    net.set_data(X, y, None, graph=True)
    buf = net._train_buffers(32)
    buf.idx.copy_(torch.randperm(args.rows, generator=g)[:32].to(dev))
    res["step_eager"] = timed(lambda: net._batch_launches(buf, args.rows), args.rounds, args.iters)
    graph = net._capture(buf, args.rows)
    res["step_graph_replay"] = timed(graph.replay, args.rounds, args.iters)
    res["step_launches_note"] = "gather, 2 noise, 3 x gemm_nt, 2 x ln_act_fwd, wce_mean, memset, 2 x gemm_nt (dX), 3 x gemm_tn, 2 x ln_act_bwd, adam, prep"

    # ---- one whole scenario -----------------------------------------------------------------------------------------
    centres = 0.25 * torch.randn(args.sites, args.features, generator=g)
    ys = torch.randint(0, args.sites, (args.rows,), generator=g)
    Xs = (centres[ys] + torch.randn(args.rows, args.features, generator=g)).to(dev)
    ys = ys.to(dev)
    names = [str(c) for c in range(args.sites)]
    scen = {}
    for label, graph_on in (("graph", True), ("eager", False)):
        times = []
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            # patience = epochs: early stopping cannot end a fold, both sides run the same number of steps
            zs = standardize(Xs)
            reports = []
            for fold, (tr, te) in enumerate(downstream.stratified_kfold(ys, 5, 42)):
                tr, te = torch.from_numpy(tr).to(dev), torch.from_numpy(te).to(dev)
                from trainer import balanced_class_weights
                c = downstream.SiteClassifier(args.features, args.sites, device=dev, seed=42 + fold)
                out = c.fit(zs[tr], ys[tr], zs[te], ys[te], balanced_class_weights(ys[tr].cpu(), args.sites), epochs=args.epochs,
                            patience=args.epochs + 1, graph=graph_on, generator=torch.Generator().manual_seed(fold))
                reports.append(downstream.classification_report(out["confusion"], names))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        scen[f"mmvae_{label}"] = dict(seconds=times, accuracy=downstream.aggregate_reports(reports, names)["accuracy"])
    times = []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        zs = standardize(Xs)
        acc = torch_scenario(zs, ys, args.sites, downstream.stratified_kfold(ys, 5, 42), args.epochs, 42)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    scen["stock_torch"] = dict(seconds=times, accuracy=acc)
    scen["steps_per_scenario"] = 5 * args.epochs * -(-(args.rows * 4 // 5) // 32)
    res["scenario"] = scen
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
