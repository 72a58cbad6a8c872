#!/usr/bin/env python3
"""Imputation quality of a trained model on the trainers' validation split: the last stage of the reference's pipeline
(prepare -> train.py -> evaluate.py; its README and run_pipeline.sh name the script, the snapshot does not contain it).

    python evaluate.py --kind rna2dna                         # checkpoint of the latest train_rna2dna.py run
    python evaluate.py --kind multimodal --checkpoint checkpoints/best_multivae_<run id>.pt --out results.json

One table row per (route, target modality) with the columns of compute_metrics (compare_directional_imputation.py:167-210), and
beside every target modality the mean-imputation baseline (training-set column means, compare_directional_imputation.py:213-232).
--knn K adds the reference's second baseline, KNeighborsRegressor(n_neighbors=K) from the other modality fitted on the training rows
(compare_directional_imputation.py:235-254), --knn-by-site its per-site form (src/models/conditioned_knn.py); both search on the
device (mmvae.knn).
--knn-tune adds the reference's tuned baseline (src/knn_comparison/run_comparison.py:56-94, optimize_knn): per target modality the
16-point grid n_neighbors {5, 10, 20, 50} x weights {uniform, distance} x metric {euclidean, manhattan} is fitted on the training rows
and scored on the validation rows, the winner becomes the row kNN-tuned(k=..,w=..,m=..) (with --knn-by-site also kNN-site-tuned(..), the
conditioned regressor's own grid) -- two searches per route serve all 16 points (mmvae.knn.optimize_knn).  --knn-tune-out FILE holds
per route the grid, the winner and the per-sample MSE summary (min, quartiles, max, mean: the reference's box plots) of the winner
beside the model's.
--clustering adds the reference's clustering table (src/clustering_evaluation/cluster_imputation_methods.py:478-504): silhouette score
and neighbourhood hit (k = 5) of the standardised features [a | b] against the validation sites -- for the true features and, per
single-target imputation route, with the target part replaced by the model's, the mean's and (with --knn) the k-NN imputations; both
numbers are computed on the device (mmvae.clustering), one feature matrix at a time.
--clustering-pca K adds the table's second half (its "PCA Silh | NH" columns, cluster_imputation_methods.py:140-187, 473-504): the
same two numbers on the projection of the same standardised matrix onto its first K principal components (the reference's K is 2), and
the share of the variance those components explain; the PCA runs on the device too (mmvae.pca).
--clustering-tsne adds its last part (its "t-SNE Silh | NH" columns, same lines): the same two numbers on TSNE(2, perplexity=min(30, n - 1),
random_state=seed) of the standardised matrix, through a PCA(50) first when it has more than 50 columns, as the reference does; the
t-SNE runs on the device as well (mmvae.tsne: exact repulsion, no tree).  --tsne-perplexity and --tsne-iters change its 30 and 1000.
--downstream adds the reference's downstream task (downstream_task.py, downstream_task_directional.py): does a site classifier learn
as well from the model's estimated modality as from the measured one?  On the validation rows whose site has at least two of them, the
estimated modalities are drawn batch by batch, every scenario's features are standardised, split into --downstream-folds stratified
folds, and a small MLP is trained per fold on the device (mmvae.downstream); one row per scenario with accuracy and weighted precision /
recall / F1, each +- its std over the folds; --downstream-out FILE holds the per-class rows too.  MultiModalVAE: the eight scenarios of
downstream_task.py:436-445; a directional model: the five its one route can fill.
Routes: the directional models' one route; MultiModalVAE: a -> b, b -> a and the full (a, b, site) reconstruction.  The metrics
are computed on the device (mmvae.metrics: one streaming launch per batch and route), nothing but 32 bytes per feature and the
per-row vectors' aggregates reaches the host.  Evaluation runs in eval mode under no_grad; eps is still sampled (vae.py:73), so
--seed selects the Philox stream.  Single process; the accumulators are additive, a multi-rank form is one all-reduce away."""
import argparse
import json
import os
import sys
from collections import namedtuple
from functools import partial

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402

import hostlib  # noqa: E402
from mmvae import clustering, to_bf16_rows  # noqa: E402
from mmvae._lib import PCA_MAXK, SIL_MAXC, WCE_MAXC  # noqa: E402
from mmvae.clustering import CLUSTERING_COLUMNS, NH_K, PCA_COLUMNS, TSNE_COLUMNS, TSNE_PCA_K, tsne_embedding  # noqa: E402,F401  (re-exported)
from mmvae.data import load_matched, split_indices  # noqa: E402
from mmvae.knn import GRID as TUNE_GRID  # noqa: E402  (the reference's 16-point grid, run_comparison.py:63-67)
from mmvae.metrics import ImputationMetrics  # noqa: E402
from src.config import Config  # noqa: E402
from src.models import KINDS, make_model  # noqa: E402

COLUMNS = ("MAE", "MSE", "RMSE", "R2", "MeanR2", "CosineSimilarity", "PearsonMean", "PearsonStd", "PearsonValid")


def build_parser(kind):
    ap = argparse.ArgumentParser(description=f"{KINDS[kind]['title']} imputation metrics on MI355X")
    hostlib.add_dataset_args(ap)
    hostlib.add_model_args(ap, n_sites=True)
    ap.add_argument("--batch-size", type=int, default=4096)
    hostlib.add_precision_args(ap)
    ap.add_argument("--checkpoint", default=None, help="state_dict as the trainers save it (default: the run named by latest_<tag>_run_id.txt)")
    ap.add_argument("--checkpoint-dir", default=Config.CHECKPOINT_DIR)
    ap.add_argument("--seed", type=int, default=Config.RANDOM_SEED, help="Philox stream of eps")
    ap.add_argument("--knn", type=int, default=0, metavar="K", help="add a kNN(k=K) imputation row per target modality (0 = off)")
    ap.add_argument("--knn-by-site", action="store_true", help="with --knn / --knn-tune: add the per-site (conditioned) k-NN rows as well")
    ap.add_argument("--knn-tune", action="store_true", help="add the tuned k-NN row per target modality: the winner of the reference's 16-point grid")
    ap.add_argument("--knn-tune-out", default=None, help="with --knn-tune: write the grids, the winners and the per-sample MSE summaries as JSON here")
    ap.add_argument("--out", default=None, help="write the table rows as JSON here")
    ap.add_argument("--clustering", action="store_true", help="add the clustering table: silhouette and neighbourhood hit (k=5) by site")
    ap.add_argument("--clustering-out", default=None, help="with --clustering: write that table's rows as JSON here")
    ap.add_argument("--clustering-pca", type=int, default=0, metavar="K",
                    help="with --clustering: add silhouette and neighbourhood hit of the K-component PCA projection (0 = off)")
    ap.add_argument("--clustering-tsne", action="store_true",
                    help="with --clustering: add silhouette and neighbourhood hit of the 2-D t-SNE embedding (PCA(50) first beyond 50 features)")
    ap.add_argument("--tsne-perplexity", type=float, default=30.0, help="with --clustering-tsne: perplexity (capped at rows - 1)")
    ap.add_argument("--tsne-iters", type=int, default=1000, help="with --clustering-tsne: iterations (at least 250)")
    ap.add_argument("--downstream", action="store_true", help="add the downstream task: site classification from original and estimated modalities")
    ap.add_argument("--downstream-folds", type=int, default=5, help="with --downstream: stratified folds per scenario")
    ap.add_argument("--downstream-epochs", type=int, default=100, help="with --downstream: most epochs per fold (early stopping may end sooner)")
    ap.add_argument("--downstream-out", default=None, help="with --downstream: write the table, per-class rows included, as JSON here")
    return ap


def routes(kind):
    """[(route name, forward kwargs over the batch (a, b, s), [(index into the forward's outputs, target 'a' | 'b')])]"""
    if kind == "rna2dna":
        return [("rna+site->dna", lambda a, b, s: dict(rna=a, site=s), [(0, "b")])]
    if kind == "dna2rna":
        return [("dna+site->rna", lambda a, b, s: dict(dna=b, site=s), [(0, "a")])]
    return [("a->b", lambda a, b, s: dict(a=a), [(1, "b")]),
            ("b->a", lambda a, b, s: dict(b=b), [(0, "a")]),
            ("a+b+site->a,b", lambda a, b, s: dict(a=a, b=b, site=s), [(0, "a"), (1, "b")])]


MOD, NAMES = {"a": 0, "b": 1}, {"a": "RNA", "b": "DNA"}         # a modality's place in a batch (a, b, s), and its name in the tables
KnnBaseline = namedtuple("KnnBaseline", "route name regressor by_site source target")      # source, target: 'a' | 'b'


def batches(va, B):
    """(i, a, b, s): rows i .. i + B of the split (a, b, s), in order"""
    for i in range(0, va[0].shape[0], B):
        yield i, va[0][i:i + B], va[1][i:i + B], va[2][i:i + B]


def knn_predict(kb, a, b, s):
    x = (a, b)[MOD[kb.source]]
    return kb.regressor.predict(x, s) if kb.by_site else kb.regressor.predict(x)


def _summary(v):
    """min, quartiles, max and mean of a float64 device vector: what a box plot draws"""
    q = torch.quantile(v, torch.tensor([0.25, 0.5, 0.75], dtype=v.dtype, device=v.device))
    return {"min": float(v.min()), "q1": float(q[0]), "median": float(q[1]), "q3": float(q[2]), "max": float(v.max()), "mean": float(v.mean())}


def _row(route, modality, model_name, result):
    return {"Route": route, "Modality": modality, "Model": model_name, **{k: result[k] for k in COLUMNS}}


def print_table(rows):
    w = max([16] + [len(r["Model"]) + 1 for r in rows])          # the tuned k-NN rows carry their parameters in the name
    head = f"{'Route':<16}{'Modality':<9}{'Model':<{w}}" + "".join(f"{c:>17}" for c in COLUMNS)
    print(head)
    print("-" * len(head))
    for r in rows:
        print(f"{r['Route']:<16}{r['Modality']:<9}{r['Model']:<{w}}"
              + "".join(f"{r[c]:>17d}" if c == "PearsonValid" else f"{r[c]:>17.6f}" for c in COLUMNS))


def print_clustering_table(rows):
    cols = CLUSTERING_COLUMNS + (PCA_COLUMNS if rows and PCA_COLUMNS[0] in rows[0] else ()) \
        + (TSNE_COLUMNS if rows and TSNE_COLUMNS[0] in rows[0] else ())
    head = f"{'Features':<16}{'Model':<16}" + "".join(f"{c:>{max(17, len(c) + 2)}}" for c in cols)
    print(head)
    print("-" * len(head))
    for r in rows:
        print(f"{r['Features']:<16}{r['Model']:<16}" + "".join(f"{r[c]:>{max(17, len(c) + 2)}.6f}" for c in cols))


def clustering_table(entries, va, dims, B, pca_k=0, tsne=None):
    """[(features, model name, target, fill)] -> table rows.  fill(a, b, s) gives the imputed target modality of that batch, or is None
    for the true features.  ONE (rows, A + D) fp32 matrix is filled batch by batch, standardised, judged and reused.  pca_k > 0: the
    same two numbers on the standardised matrix's projection onto its first pca_k principal components as well.  tsne = (perplexity,
    iterations, seed): and on its t-SNE embedding."""
    n_val, labels = va[0].shape[0], va[2]
    n_labels = int(torch.unique(labels).numel())
    if not clustering.can_judge(n_labels, n_val):
        print(f"clustering table skipped: {n_labels} distinct sites among {n_val} validation rows "
              f"(need 2 .. min(rows - 1, {SIL_MAXC}))")
        return []
    feats = torch.empty(n_val, dims["a"] + dims["b"], dtype=torch.float32, device=labels.device)
    part = {"a": feats[:, :dims["a"]], "b": feats[:, dims["a"]:]}
    rows = []
    for features, model_name, tgt, fill in entries:
        for i, a, b, s in batches(va, B):
            for m, true in (("a", a), ("b", b)):
                part[m][i:i + B].copy_(fill(a, b, s) if m == tgt else true)
        z = clustering.standardize(feats)
        rows.append({"Features": features, "Model": model_name, **clustering.judge_matrix(z, labels, pca_k=pca_k, tsne=tsne)})
        del z
    return rows


DOWNSTREAM_COLUMNS = (("Accuracy", None), ("Precision", "precision"), ("Recall", "recall"), ("F1", "f1-score"))


def downstream_scenarios(kind, orig, est):
    """{scenario name: [feature blocks]}: downstream_task.py:436-445 for the MultiModalVAE; for a directional model the five scenarios
    its one route can fill.  orig / est: {'a': RNA, 'b': DNA} matrices (est holds the estimated target only for a directional kind)."""
    if kind == "multimodal":
        return {"Orig. RNA": [orig["a"]], "Orig. DNA": [orig["b"]], "Orig. RNA + Est. DNA": [orig["a"], est["b"]],
                "Orig. DNA + Est. RNA": [orig["b"], est["a"]], "Orig. RNA + Orig. DNA": [orig["a"], orig["b"]], "Est. DNA": [est["b"]],
                "Est. RNA": [est["a"]], "Est. RNA + Est. DNA": [est["a"], est["b"]]}
    (src, tgt), n = ("a", "b") if kind == "rna2dna" else ("b", "a"), NAMES
    return {f"Orig. {n[src]}": [orig[src]], f"Orig. {n[tgt]}": [orig[tgt]], f"Orig. {n[src]} + Est. {n[tgt]}": [orig[src], est[tgt]],
            f"Est. {n[tgt]}": [est[tgt]], f"Orig. {n[src]} + Orig. {n[tgt]}": [orig[src], orig[tgt]]}


def downstream_table(kind, model, va, B, folds, epochs, seed):
    """{scenario: the aggregated report of run_classification_scenario}, or {} with a message when the validation split cannot carry the
    task.  Classes with fewer than 2 validation rows are dropped and the labels re-encoded contiguously (downstream_task.py:417-424)."""
    from mmvae import downstream
    site = va[2]
    ids, inverse, counts = torch.unique(site, return_inverse=True, return_counts=True)
    keep_class = counts >= 2
    rows = keep_class[inverse].nonzero().squeeze(1)
    kept = ids[keep_class]
    if not 2 <= kept.numel() <= WCE_MAXC or folds < 2 or rows.numel() < folds or int(counts[keep_class].max()) < folds:
        print(f"downstream table skipped: {kept.numel()} sites with at least 2 of the {site.numel()} validation rows (need 2 .. {WCE_MAXC}), "
              f"{rows.numel()} rows for {folds} folds")
        return {}
    recode = torch.full((int(ids.max()) + 1,), -1, dtype=torch.int64, device=site.device)
    recode[kept] = torch.arange(kept.numel(), device=site.device)
    labels = recode[site[rows]]
    names = [str(int(i)) for i in kept]
    # the kept rows in the inputs' storage (bf16 inputs keep their padded rows: the model reads them as it does above)
    fa, fb = (to_bf16_rows(t[rows]) if t.dtype == torch.bfloat16 else t[rows].contiguous() for t in va[:2])
    fs = site[rows].contiguous()
    orig = {"a": fa.float().contiguous(), "b": fb.float().contiguous()}
    est = {}
    with torch.no_grad():
        for _, kwargs, outs in routes(kind):
            if len(outs) != 1:                                   # the single-target routes, in routes()' order: a -> b before b -> a
                continue
            j, tgt = outs[0]
            est[tgt] = torch.empty_like(orig[tgt])
            for i, a, b, s in batches((fa, fb, fs), B):
                est[tgt][i:i + B].copy_(model(**kwargs(a, b, s))[j])
    arch = dict(hidden=(256, 128), layer_norm=True, dropout=(0.3, 0.2)) if kind == "multimodal" else dict(hidden=(128,), layer_norm=False, dropout=(0.2,))
    return {name: downstream.cross_validate(blocks[0] if len(blocks) == 1 else torch.cat(blocks, dim=1), labels, names, folds, epochs=epochs,
                                            seed=seed, **arch) for name, blocks in downstream_scenarios(kind, orig, est).items()}


def print_downstream_table(table):
    head = f"{'Scenario':<26}" + "".join(f"{c:>20}" for c, _ in DOWNSTREAM_COLUMNS)
    print(head)
    print("-" * len(head))
    for name, r in table.items():
        cells = [(r["accuracy"], r["accuracy_std"])] + [(r["weighted avg"][k], r["weighted avg"][k + "_std"]) for _, k in DOWNSTREAM_COLUMNS[1:]]
        print(f"{name:<26}" + "".join(f"{f'{m:.4f} +- {sd:.4f}':>20}" for m, sd in cells))


PCA_RANGE = f"--clustering-pca {{}} outside [0, min({PCA_MAXK}, validation rows, features)]"


def check_args(args):
    """Every flag combination and range the script refuses; needs neither data nor device (load_split holds --clustering-pca to the split's shape)."""
    if args.knn_tune_out and not args.knn_tune:
        raise SystemExit("--knn-tune-out needs --knn-tune")
    if args.knn_by_site and not (args.knn > 0 or args.knn_tune):
        raise SystemExit("--knn-by-site needs --knn K or --knn-tune")
    for flag in ("clustering_out", "clustering_pca", "clustering_tsne"):
        if getattr(args, flag) and not args.clustering:
            raise SystemExit(f"--{flag.replace('_', '-')} needs --clustering")
    if args.clustering_tsne and (not args.tsne_perplexity > 0 or args.tsne_iters < 250):
        raise SystemExit("--tsne-perplexity must be positive and --tsne-iters at least 250")
    if not 0 <= args.clustering_pca <= PCA_MAXK:
        raise SystemExit(PCA_RANGE.format(args.clustering_pca))
    if args.downstream_out and not args.downstream:
        raise SystemExit("--downstream-out needs --downstream")
    if args.downstream and (args.downstream_folds < 2 or args.downstream_epochs < 1):
        raise SystemExit("--downstream-folds must be at least 2 and --downstream-epochs at least 1")


def load_split(args, dev):
    """((tpm, beta, site) on the host, training indices, the validation split on the device as the model reads it, the training column
    means) of --data or of the synthetic set.  --data sets the dims and the site count of `args`."""
    tpm, beta_v, site, (args.input_dim_a, args.input_dim_b, args.n_sites) = load_matched(
        args.data, args.samples, args.input_dim_a, args.input_dim_b, args.n_sites, Config.RANDOM_SEED)
    val_idx, train_idx = split_indices(tpm.shape[0])
    if val_idx.numel() == 0:
        raise SystemExit(f"{tpm.shape[0]} samples leave no validation rows")
    if args.clustering_pca > min(val_idx.numel(), args.input_dim_a + args.input_dim_b):
        raise SystemExit(PCA_RANGE.format(args.clustering_pca))
    va = [t[val_idx].to(dev).contiguous() for t in (tpm, beta_v, site)]
    # mean imputation: the column means of the TRAINING rows, one row for every validation sample
    means = {"a": tpm[train_idx].double().mean(dim=0).float().to(dev), "b": beta_v[train_idx].double().mean(dim=0).float().to(dev)}
    if args.input_dtype == "bf16":
        va[:2] = [to_bf16_rows(t) for t in va[:2]]
    return (tpm, beta_v, site), train_idx, va, means


def load_model(kind, args, dev):
    """(the model of --checkpoint, or of the run the trainer named last, in eval mode at --precision; the checkpoint's path)"""
    path, cause = hostlib.resolve_checkpoint(kind, args.checkpoint, args.checkpoint_dir)
    if path is None:
        raise SystemExit(f"no --checkpoint given and {cause[1]} (written by the trainer) is not here" if cause[0] == hostlib.NO_RUN_ID
                         else f"checkpoint {cause[1]} not found")
    model = make_model(kind, args.input_dim_a, args.input_dim_b, args.n_sites, args.latent_dim)
    state = torch.load(path, map_location="cpu")
    own = model.state_dict()
    bad = [f"{k}: checkpoint {tuple(state[k].shape)}, model {tuple(v.shape)}" for k, v in own.items()
           if k in state and tuple(state[k].shape) != tuple(v.shape)]
    missing = [k for k in own if k not in state]
    if bad or missing:
        raise SystemExit(f"{path} is not a {KINDS[kind]['title']} of RNA {args.input_dim_a} / DNA {args.input_dim_b} / {args.n_sites} sites / latent "
                         f"{args.latent_dim}: " + "; ".join(bad[:4] + [f"missing {k}" for k in missing[:4]]))
    model.load_state_dict(state)
    return model.to(dev).set_precision(args.precision).eval(), path


@torch.no_grad()
def imputation_rows(model, title, plan, targets, va, means, dims, B):
    """The model's row per (route, target) and the mean imputation's per target: one pass, every route's forward on every batch."""
    acc = {(name, tgt): ImputationMetrics(dims[tgt], va[2].device) for name, _, outs in plan for _, tgt in outs}
    base = {tgt: ImputationMetrics(dims[tgt], va[2].device) for tgt in targets}
    for _, a, b, s in batches(va, B):
        truth = {"a": a, "b": b}
        for name, kwargs, outs in plan:
            res = model(**kwargs(a, b, s))
            for j, tgt in outs:
                acc[(name, tgt)].update(truth[tgt], res[j])
        for tgt in targets:
            base[tgt].update(truth[tgt], means[tgt])
    return [_row(name, NAMES[tgt], title, acc[(name, tgt)].compute()) for name, _, outs in plan for _, tgt in outs] \
        + [_row("train mean", NAMES[tgt], "MeanImputation", base[tgt].compute()) for tgt in targets]


def knn_baselines(args, targets, host, train_idx, va, dims, B):
    """(table rows, [KnnBaseline], what --knn-tune-out holds per tuned regressor): per target modality the plain, per-site and tuned k-NN
    regressors the flags ask for, fitted on the training rows, and their rows on the validation split.  No model forward."""
    if not (args.knn > 0 or args.knn_tune):
        return [], [], []
    from mmvae.knn import ConditionedKNeighborsRegressor, KNeighborsRegressor, optimize_knn
    tr = [t[train_idx].to(va[2].device).contiguous() for t in host]
    if args.input_dtype == "bf16":
        tr[:2] = [to_bf16_rows(t) for t in tr[:2]]
    rows, baselines, tuned = [], [], []
    for tgt in targets:
        src = "b" if tgt == "a" else "a"
        x_tr, y_tr, x_va, y_va = tr[MOD[src]], tr[MOD[tgt]], va[MOD[src]], va[MOD[tgt]]
        route = {False: f"{src}->{tgt}", True: f"{src}+site->{tgt}"}
        found = []
        if args.knn > 0:
            found.append((f"kNN(k={args.knn})", KNeighborsRegressor(args.knn).fit(x_tr, y_tr), False))
        if args.knn > 0 and args.knn_by_site:
            found.append((f"kNN-site(k={args.knn})", ConditionedKNeighborsRegressor(args.knn).fit(x_tr, y_tr, tr[2]), True))
        for by_site in ([False, True] if args.knn_by_site else [False]) if args.knn_tune else []:
            # the grid's k reaches 50: with fewer training rows the plain grid keeps the k that fit (the per-site form clips k itself)
            params = dict(TUNE_GRID, n_neighbors=[k for k in TUNE_GRID["n_neighbors"] if by_site or k <= tr[0].shape[0]])
            best, p, grid = optimize_knn(x_tr, y_tr, x_va, y_va, tr[2] if by_site else None, va[2] if by_site else None, params=params,
                                         conditioned=by_site)
            found.append((f"kNN-{'site-' if by_site else ''}tuned(k={p['n_neighbors']},w={p['weights']},m={p['metric']})", best, by_site))
            tuned.append({"Route": route[by_site], "Modality": NAMES[tgt], "Model": found[-1][0], "conditioned": by_site, "best": p,
                          "best_mse": min(m for _, m in grid), "grid": [dict(q, mse=m) for q, m in grid]})
        for kb in (KnnBaseline(route[by_site], name, reg, by_site, src, tgt) for name, reg, by_site in found):
            m = ImputationMetrics(dims[tgt], va[2].device)
            for _, a, b, s in batches(va, B):
                m.update((a, b)[MOD[tgt]], knn_predict(kb, a, b, s))
            rows.append(_row(kb.route, NAMES[tgt], kb.name, m.compute()))
            baselines.append(kb)
    return rows, baselines, tuned


def clustering_entries(model, title, plan, means, baselines):
    """clustering_table's entries: the true features, and per single-target route (the full reconstruction is not an imputation) its
    target as the model, the training means and that target's k-NN baselines impute it.  Only the model's entries run forwards."""
    def of_route(name, kwargs, j, tgt):                  # a scope of its own: the lambdas hold THIS route's kwargs, j and tgt
        return [(name, title, tgt, lambda a, b, s: model(**kwargs(a, b, s))[j]),
                (name, "MeanImputation", tgt, lambda a, b, s: means[tgt].expand(a.shape[0], -1))] \
            + [(kb.route, kb.name, tgt, partial(knn_predict, kb)) for kb in baselines if kb.target == tgt]
    return [("a|b", "original", None, None)] + [e for name, kwargs, outs in plan if len(outs) == 1 for e in of_route(name, kwargs, *outs[0])]


@torch.no_grad()
def tuned_summaries(tuned, model, title, plan, va, baselines, B):
    """tuned[*]['per_sample_mse']: the box-plot numbers of every tuned regressor beside the model's on its route; one forward per batch each"""
    by_name = {(kb.route, kb.name): kb for kb in baselines}
    for t in tuned:
        kb = by_name[(t["Route"], t["Model"])]
        route_fw = [(kwargs, outs[0][0]) for _, kwargs, outs in plan if len(outs) == 1 and outs[0][1] == kb.target]
        per = {t["Model"]: [], title: []}
        for _, a, b, s in batches(va, B):
            y = (a, b)[MOD[kb.target]].double()
            per[t["Model"]].append((knn_predict(kb, a, b, s).double() - y).pow(2).mean(dim=1))
            if route_fw:
                kwargs, j = route_fw[0]
                per[title].append((model(**kwargs(a, b, s))[j].double() - y).pow(2).mean(dim=1))
        t["per_sample_mse"] = {k: _summary(torch.cat(v)) for k, v in per.items() if v}


def _dump(obj, path):
    if path:
        with open(path, "w") as f:
            json.dump(obj, f, indent=1)


def run(kind, argv=None, return_clustering=False):
    args = build_parser(kind).parse_args(argv)
    check_args(args)
    hostlib.require_device("evaluate.py")
    dev = torch.device("cuda", torch.cuda.current_device())
    host, train_idx, va, means = load_split(args, dev)
    model, path = load_model(kind, args, dev)
    title, plan = KINDS[kind]["title"], routes(kind)
    targets = sorted({tgt for _, _, outs in plan for _, tgt in outs})
    dims = {"a": args.input_dim_a, "b": args.input_dim_b}
    B, n_val = args.batch_size, va[0].shape[0]
    torch.manual_seed(args.seed)
    # The model draws eps from ONE Philox stream, per forward, so what a stage computes depends on every forward before it.  No table may
    # depend on another table's flag, and THIS ORDER is what guarantees it: a stage behind a flag runs its forwards after every stage
    # whose output that flag must not change.  (The k-NN stage runs no forward; where it stands does not matter.)
    rows = imputation_rows(model, title, plan, targets, va, means, dims, B)                    # 1. always: every route on every batch
    knn_rows, baselines, tuned = knn_baselines(args, targets, host, train_idx, va, dims, B)
    rows += knn_rows
    print(f"{title}: {path}  ({n_val} validation rows, batch {B}, {args.precision}, {args.input_dtype} inputs)")
    print_table(rows)
    _dump(rows, args.out)
    crows = []
    if args.clustering:                                                                         # 2. a forward per batch and single-target route
        with torch.no_grad():
            crows = clustering_table(clustering_entries(model, title, plan, means, baselines), va, dims, B, args.clustering_pca,
                                     (args.tsne_perplexity, args.tsne_iters, args.seed) if args.clustering_tsne else None)
        if crows:
            print(f"clustering by site: standardised [a | b] features, silhouette and neighbourhood hit (k={NH_K})"
                  + (f"; PCA columns: the same on the first {args.clustering_pca} principal components" if args.clustering_pca else "")
                  + (f"; TSNE columns: the same on the 2-D t-SNE embedding (perplexity {min(args.tsne_perplexity, n_val - 1):g}, "
                     f"{args.tsne_iters} iterations)" if args.clustering_tsne else ""))
            print_clustering_table(crows)
        _dump(crows, args.clustering_out)
    if args.downstream:                                                                         # 3. the estimated modalities, then the classifiers
        table = downstream_table(kind, model, va, B, args.downstream_folds, args.downstream_epochs, args.seed)
        if table:
            print(f"downstream task: site classification, {args.downstream_folds} stratified folds, at most {args.downstream_epochs} epochs; "
                  "accuracy and weighted averages, mean +- std over the folds")
            print_downstream_table(table)
        _dump(table, args.downstream_out)
    if args.knn_tune_out:                                                                       # 4. a forward per batch and tuned regressor
        tuned_summaries(tuned, model, title, plan, va, baselines, B)
        _dump(tuned, args.knn_tune_out)
    return (rows, crows) if return_clustering else rows


if __name__ == "__main__":
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--kind", default="multimodal", choices=sorted(KINDS))
    known, rest = pre.parse_known_args()
    run(known.kind, rest)
