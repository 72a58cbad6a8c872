#!/usr/bin/env python3
"""Device time of mmvae.pca.PCA's parts at the evaluation shape -- the validation rows of evaluate.py's default split (52 429),
standardised features of width 1 354 (RNA | DNA, fp32) and 782 (RNA, fp32 and padded bf16 rows) -- each given separately:
  the scatter matrix (ops.pca_scatter: main + reduce launches, with the split count), the float64 eigen-solve of the F x F matrix
  (torch.linalg.eigh, a library call), the projection (ops.pca_project, k = 2 and 50) and PCA(2).fit_transform as a whole;
beside them, from the same run on the same matrix, what a user would write with stock torch on the device
  zc = z - z.mean(0); zc.T @ zc  (fp32, the centred copy included), torch.linalg.eigh in float64, zc @ V.T,
and sklearn.decomposition.PCA(2) on the host for the whole matrix.

Times are device events around `--reps` back-to-back calls (a kernel takes milliseconds), divided by the count; median / min / max over
`--rounds` such windows after a warm-up one.  The scatter's rate counts N F^2 flops (the triangle with the diagonal, 2 flops per
multiply-add) against the 155 TFLOP/s that v_mfma_f32_16x16x4_f32 measures on this card (MI355X_MICROARCH.md).  Before anything is
timed the projection is compared with the torch formulation's after sign alignment and the largest difference recorded beside the
first three eigenvalues (both are float32 passes: the difference scales with the rounding of the scatter matrix over the eigengap).
ONE JSON object is printed, and written to --out if given."""
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


def torch_pca(z, k):
    zc = z - z.mean(0)
    lam, vec = torch.linalg.eigh((zc.T @ zc).double())
    V = vec.flip(1)[:, :k].T.float().contiguous()
    return zc @ V.T, V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=52429)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="kernel calls per timed window")
    ap.add_argument("--no-comparators", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip sklearn on the host")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pca.py needs an MI355X: the product path has no CPU fallback")
    from mmvae import clustering, ops, to_bf16_rows
    from mmvae.pca import PCA
    from src.config import Config
    from trainer import synthetic_dataset

    dev = torch.device("cuda", 0)
    N = args.rows
    tpm, beta_v, _ = synthetic_dataset(N, 782, 572, 24, Config.RANDOM_SEED)
    result = dict(rows=N, rounds=args.rounds, mfma_f32_peak_TFLOPs=MFMA_F32_PEAK / 1e12, cases=[])
    for F, feats in ((782 + 572, torch.cat([tpm, beta_v], 1)), (782, tpm)):
        z32 = clustering.standardize(feats.to(dev))
        for storage, z in (("fp32", z32),) + ((("bf16_rows", to_bf16_rows(z32)),) if F == 782 else ()):
            case = dict(width=F, storage=storage, scatter_splits=ops.pca_scatter_splits(N, F, 0),
                        scatter_work_bytes=ops.pca_scatter_work_bytes(N, F, 0))
            pca = PCA(50).fit(z)
            mean, comps = pca.mean_, pca.components_
            case["explained_2"] = float(pca.explained_variance_ratio_[:2].sum())
            case["explained_variance_top3"] = pca.explained_variance_[:3].tolist()
            if not args.no_comparators and storage == "fp32":
                y_t, V_t = torch_pca(z, 2)
                y = ops.pca_project(z, mean, comps[:2].contiguous())
                sign = torch.sign((V_t * comps[:2]).sum(1))
                diff = float((y - y_t * sign).abs().max())
                case["max_abs_diff_to_torch_projection"] = diff
                case["max_abs_projection"] = float(y.abs().max())
                del y_t, y
            S = ops.pca_scatter(z, mean)
            flops = 1.0 * N * F * F
            ts = timed(lambda: ops.pca_scatter(z, mean, out=S), args.rounds, args.reps)
            rate = flops / (ts["median_ms"] * 1e-3)
            case["scatter"] = dict(ts, TFLOPs=rate / 1e12, share_of_mfma_f32=rate / MFMA_F32_PEAK)
            Sd = S.double()
            case["eigh_float64"] = timed(lambda: torch.linalg.eigh(Sd), args.rounds, 1)
            for k in (2, 50):
                v = comps[:k].contiguous()
                out = torch.empty(N, k, device=dev)
                tp = timed(lambda: ops.pca_project(z, mean, v, out=out), args.rounds, args.reps)
                nbytes = N * F * z.element_size() + 4 * N * k
                case[f"project_k{k}"] = dict(tp, GBps=nbytes / (tp["median_ms"] * 1e-3) / 1e9)
            case["fit_transform_k2"] = timed(lambda: PCA(2).fit_transform(z), args.rounds, 1)
            if not args.no_comparators and storage == "fp32":
                def centred_gram():
                    zc = z - z.mean(0)
                    return zc.T @ zc
                tg = timed(centred_gram, args.rounds, args.reps)
                case["torch_centred_gram_fp32"] = dict(tg, TFLOPs_counting_N_F2=flops / (tg["median_ms"] * 1e-3) / 1e12,
                                                       scatter_over_this=ts["median_ms"] / tg["median_ms"])
                zc = z - z.mean(0)
                for k in (2, 50):
                    Vt = comps[:k].T.contiguous()
                    case[f"torch_project_k{k}"] = timed(lambda: zc @ Vt, args.rounds, args.reps)
                del zc
                case["torch_pca_k2"] = timed(lambda: torch_pca(z, 2), args.rounds, 1)
            result["cases"].append(case)
        if not args.no_comparators and not args.no_host and F == 782 + 572:
            from sklearn.decomposition import PCA as SkPCA
            zh = z32.cpu().numpy()
            t0 = time.perf_counter()
            sk = SkPCA(n_components=2, random_state=42)
            yh = sk.fit_transform(zh)
            host_ms = (time.perf_counter() - t0) * 1e3
            y = PCA(2).fit_transform(z32).cpu().numpy()
            # PCA(2) as a user writes it: above 1 000 features sklearn's "auto" is the randomized solver, in the input's float32, so on a
            # matrix whose leading eigenvalues nearly tie it returns other vectors; the difference is given as it is and after aligning
            # each column's sign
            sign = [1.0 if (y[:, j] * yh[:, j]).sum() >= 0 else -1.0 for j in range(2)]
            result["cases"][0]["sklearn_host_pca2"] = dict(ms=host_ms, max_abs_diff=float(abs(y - yh).max()),
                                                           max_abs_diff_sign_aligned=float(abs(y - yh * sign).max()), signs=sign,
                                                           host_threads=torch.get_num_threads())
        del z32
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
