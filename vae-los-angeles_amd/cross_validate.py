#!/usr/bin/env python3
"""K-fold cross-validation of the imputers (reference vae_cross_modality_cv.py): mean baseline, kNN and the directional VAE over the
same shuffled folds, both directions, compared with paired t-tests on Mean R2, MSE and Pearson.

    python cross_validate.py --folds 10 --subset 0.1 --neighbors 5 10 --epochs 200 --batch-size 32 --out cv.json
    python cross_validate.py --models mean knn --knn-by-site            # baselines only, with the site-conditioned kNN
    python cross_validate.py --autoencoder                              # adds the non-variational AE rows and their two t-tests

The folds are sklearn's KFold(folds, shuffle=True, random_state=42) and the subset is DataFrame.sample(frac, random_state=42), so a
run on the reference's processed_data.pkl sees the reference's rows and folds.  All folds and all k of the kNN come from one
fold-masked search on the device (mmvae/crossval.py).  No plots are made."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402

import hostlib  # noqa: E402
from mmvae import crossval  # noqa: E402
from mmvae.data import load_matched  # noqa: E402
from src.config import Config  # noqa: E402

NO_AE = "the AE rows of the reference are not produced, because the project has no AE models"
COMPARED = ("Mean R2", "MSE", "Pearson")


def build_parser():
    ap = argparse.ArgumentParser(description="Cross-validate the DNA <-> RNA imputers on the MI355X")
    ap.add_argument("--folds", type=int, default=10, help="number of cross-validation folds")
    ap.add_argument("--subset", type=float, default=0.1, help="fraction of the rows to use (1.0: all)")
    ap.add_argument("--neighbors", type=int, nargs="+", default=[5, 10], help="k values of the kNN")
    ap.add_argument("--epochs", type=int, default=200, help="most VAE epochs per fold (early stopping may end sooner)")
    ap.add_argument("--batch-size", type=int, default=32)
    hostlib.add_dataset_args(ap)
    hostlib.add_model_args(ap, n_sites=True)
    hostlib.add_precision_args(ap)
    ap.add_argument("--seed", type=int, default=Config.RANDOM_SEED, help="folds, subset, VAE initialisation, noise and batch order")
    ap.add_argument("--models", nargs="+", default=["mean", "knn", "vae"], help="any of: mean knn vae")
    ap.add_argument("--knn-by-site", action="store_true", help="with knn: add the site-conditioned kNN under the same folds")
    ap.add_argument("--autoencoder", action="store_true", help="add the non-variational baselines RNA2DNAAE / DNA2RNAAE (the reference's "
                    "'ae' rows) under the same folds, trained with --epochs, --batch-size, --precision, --eager and --seed")
    ap.add_argument("--eager", action="store_true", help="train the VAEs with launches issued from Python instead of the captured step")
    ap.add_argument("--out", default=None, help="write the results and the comparisons as JSON here")
    return ap


def print_summary(results):
    print("\n" + "=" * 120)
    print("FINAL RESULTS SUMMARY (Mean R2 & MSE)")
    print("=" * 120)
    print(f"{'Direction':<12} | {'Model':<8} | {'Param':<10} | {'Mean R2':<10} | {'Std':<8} | {'MSE':<10} | {'Std':<8} | {'Time (s)':<8}")
    print("-" * 120)
    for r in results:
        param = f"{r['param_name']}={r['param_value']}"
        print(f"{r['direction']:<12} | {r['model']:<8} | {param:<10} | {r['mean_Mean R2']:<10.4f} | {r['std_Mean R2']:<8.4f} | "
              f"{r['mean_MSE']:<10.4f} | {r['std_MSE']:<8.4f} | {r['time']:<8.2f}")
    print("=" * 120)


def print_comparison(metric, entries):
    print("\n" + "=" * 80)
    print(f"STATISTICAL COMPARISON (Paired t-test) on {metric}")
    print("=" * 80)
    for e in entries:
        print(f"\nDirection: {e['direction']}")
        print(f"  Best kNN: k={e['best_knn']}   Best VAE: epochs={e['best_vae']}")
        if "best_ae" in e:
            print(f"  Best AE: epochs={e['best_ae']}")
        for key in ("ae_vs_vae", "ae_vs_knn", "vae_vs_mean", "knn_site_vs_vae", "knn_vs_vae"):
            if key in e:
                c = e[key]
                print(f"  {c['a']} vs {c['b']}: t={c['t']:.4f}, p={c['p']:.4e}  ({metric}: {c['mean_a']:.4f} vs {c['mean_b']:.4f})")
        w = e["knn_vs_vae"]["winner"]
        print(f"  -> Significant difference! {w} performs better." if w else "  -> No significant difference detected (p >= 0.05).")


def run(argv=None):
    args = build_parser().parse_args(argv)
    if "ae" in args.models:
        raise SystemExit(f"--models ae: {NO_AE}")
    bad = [m for m in args.models if m not in ("mean", "knn", "vae")]
    if bad:
        raise SystemExit(f"--models {' '.join(bad)}: any of mean knn vae")
    if args.knn_by_site and "knn" not in args.models:
        raise SystemExit("--knn-by-site needs knn among --models")
    if args.folds < 2 or not 0.0 < args.subset <= 1.0 or min(args.neighbors) < 1 or args.epochs < 1 or args.batch_size < 1:
        raise SystemExit("--folds must be at least 2, --subset in (0, 1], --neighbors, --epochs and --batch-size at least 1")
    hostlib.require_device("cross_validate.py")
    dev = torch.device("cuda", 0)
    tpm, beta_v, site, (args.input_dim_a, args.input_dim_b, args.n_sites) = load_matched(
        args.data, args.samples, args.input_dim_a, args.input_dim_b, args.n_sites, Config.RANDOM_SEED)
    if args.subset < 1.0:
        rows = torch.from_numpy(crossval.subset_rows(tpm.shape[0], args.subset, args.seed))
        tpm, beta_v, site = tpm[rows], beta_v[rows], site[rows]
    n = tpm.shape[0]
    if n < args.folds or max(args.neighbors) > n - (n + args.folds - 1) // args.folds:
        raise SystemExit(f"{n} rows are too few for {args.folds} folds and k = {max(args.neighbors)}")
    print(f"{n} rows, RNA {tpm.shape[1]} / DNA {beta_v.shape[1]} / {args.n_sites} sites; {args.folds} folds shared by all models")
    rna, dna, site = tpm.to(dev).contiguous(), beta_v.to(dev).contiguous(), site.to(dev)
    if args.input_dtype == "bf16":
        from mmvae import to_bf16_rows
        rna, dna = to_bf16_rows(rna), to_bf16_rows(dna)
    fold = crossval.kfold_assignments(n, args.folds, args.seed)
    models = [m for m in ("mean", "knn") if m in args.models] + (["knn_site"] if args.knn_by_site else []) \
        + (["vae"] if "vae" in args.models else []) + ([crossval.AE_MODEL] if args.autoencoder else [])

    def say(r):
        label = "Mean baseline" if r["model"] == "mean" else f"{r['model']} {r['param_name']}={r['param_value']}"
        print(f"  {label}: Mean R2 = {r['mean_Mean R2']:.4f} (+/- {r['std_Mean R2']:.4f})  MSE = {r['mean_MSE']:.4f} (+/- {r['std_MSE']:.4f})")

    results = []
    for direction, X, Y in (("DNA -> RNA", dna, rna), ("RNA -> DNA", rna, dna)):
        print(f"\n--- Processing {direction} ---")
        results += crossval.cross_validate(X, Y, site, fold, direction, models, args.neighbors, epochs=args.epochs, batch_size=args.batch_size,
                                           seed=args.seed, precision=args.precision, eager=args.eager, latent_dim=args.latent_dim,
                                           n_sites=args.n_sites, log=say)
    print_summary(results)
    comparisons = {metric: crossval.compare(results, metric) for metric in COMPARED}
    for metric in COMPARED:
        print_comparison(metric, comparisons[metric])
    out = {"rows": n, "folds": args.folds, "neighbors": list(args.neighbors), "results": results, "comparisons": comparisons}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    run()
