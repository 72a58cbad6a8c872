"""K-fold cross-validation of the imputers on the device: the reference's vae_cross_modality_cv.py (mean baseline, kNN and the
directional VAE over the same shuffled folds, compared with paired t-tests).

The k-NN part is ONE search: every row searches the whole matrix among the rows outside its own fold at the largest k
(ops.knn_search_grouped with differ=(fold, fold)); every smaller k is a prefix of that answer, every fold a subset of its rows.  The
reference runs folds x len(k_values) fits on host copies (vae_cross_modality_cv.py:314-322).  The site-conditioned baseline under the
same folds (models "knn_site") adds same=(site, site) to the same search.

    fold = kfold_assignments(n, 10)                                   # sklearn's KFold(10, shuffle=True, random_state=42)
    results = cross_validate(X, Y, site, fold, "DNA -> RNA", ("mean", "knn", "vae"), (5, 10), epochs=200, batch_size=32)
    comparisons = compare(results, "Mean R2")

The host part (fold / subset / inner-split index sets, the paired t-test, the comparison) is float64 numpy, pure, and needs no device.
"""
import math
import time

import numpy as np

METRIC_KEYS = {"Mean R2": "MeanR2", "Global R2": "R2", "MSE": "MSE", "MAE": "MAE", "Cosine Sim": "CosineSimilarity", "Pearson": "PearsonMean"}
DIRECTIONS = {"DNA -> RNA": "dna2rna", "RNA -> DNA": "rna2dna"}
MODELS = ("mean", "knn", "knn_site", "vae")
# The non-variational baselines are asked for as "autoencoder"; their result rows carry the reference's model name "ae".  The name
# "ae" itself stays refused among `models` (the refusal predates the AE models and is pinned by tests).
AE_MODEL, AE_ROW = "autoencoder", "ae"
AE_KINDS = {"dna2rna": "dna2rna_ae", "rna2dna": "rna2dna_ae"}
HIGHER_IS_BETTER = ("R2", "Cosine", "Pearson")              # perform_statistical_comparison: substrings of the metric name


# ---------------------------------------------------------------------------------------------------------------------------------
# host: index sets
# ---------------------------------------------------------------------------------------------------------------------------------
def kfold_assignments(n, folds, seed=42):
    """int32 (n,): the fold whose TEST set holds each row under sklearn's KFold(folds, shuffle=True, random_state=seed): the shuffled
    arange cut into contiguous slices of n // folds rows, one more for the first n % folds."""
    n, folds = int(n), int(folds)
    if not 2 <= folds <= n:
        raise ValueError(f"kfold_assignments: folds = {folds} outside [2, {n} rows]")
    indices = np.arange(n)
    np.random.RandomState(seed).shuffle(indices)
    sizes = np.full(folds, n // folds, dtype=np.int64)
    sizes[:n % folds] += 1
    code = np.empty(n, np.int32)
    code[indices] = np.repeat(np.arange(folds, dtype=np.int32), sizes)
    return code


def subset_rows(n, frac, seed=42):
    """the rows of DataFrame.sample(frac=frac, random_state=seed), in its order"""
    return np.random.RandomState(seed).choice(int(n), round(frac * int(n)), replace=False)


def inner_split(n, seed=42):
    """(train rows, validation rows) of sklearn's train_test_split(test_size=0.1, random_state=seed) over n rows"""
    n = int(n)
    n_val = int(math.ceil(0.1 * n))
    if n_val >= n:
        raise ValueError(f"inner_split: {n} rows leave no training rows")
    perm = np.random.RandomState(seed).permutation(n)
    return perm[n_val:], perm[:n_val]


# ---------------------------------------------------------------------------------------------------------------------------------
# host: the paired t-test (scipy.stats.ttest_rel, two-sided) without scipy
# ---------------------------------------------------------------------------------------------------------------------------------
def _betacf(a, b, x):
    """continued fraction of the incomplete beta function (modified Lentz), float64"""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 10000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h


def betainc(a, b, x):
    """the regularised incomplete beta function I_x(a, b) in float64"""
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, 1.0 - x) / b


def paired_ttest(a, b):
    """(t, p, df) of scipy.stats.ttest_rel(a, b): two-sided, df = n - 1, p = I_{df / (df + t^2)}(df / 2, 1 / 2).  Identical samples give
    (nan, nan), a constant non-zero difference (+-inf, 0.0), as scipy does."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or a.ndim != 1 or a.size < 2:
        raise ValueError(f"paired_ttest: two 1-D samples of one length >= 2, got {a.shape} and {b.shape}")
    n = a.size
    df = n - 1
    d = a - b
    with np.errstate(divide="ignore", invalid="ignore"):
        t = float(np.mean(d) / np.sqrt(np.var(d, ddof=1) / n))
    if math.isnan(t):
        return t, float("nan"), df
    if math.isinf(t):
        return t, 0.0, df
    return t, betainc(0.5 * df, 0.5, df / (df + t * t)), df


# ---------------------------------------------------------------------------------------------------------------------------------
# host: the comparison (perform_statistical_comparison as data)
# ---------------------------------------------------------------------------------------------------------------------------------
def _pair(name_a, a, name_b, b, metric):
    sa, sb = a["fold_metrics"][metric], b["fold_metrics"][metric]
    t, p, df = paired_ttest(sa, sb)
    ma, mb = float(np.mean(sa)), float(np.mean(sb))
    winner = None
    if p < 0.05:
        higher = any(x in metric for x in HIGHER_IS_BETTER)
        winner = name_a if (ma > mb if higher else ma < mb) else name_b
    return {"a": name_a, "b": name_b, "t": t, "p": p, "df": df, "mean_a": ma, "mean_b": mb, "winner": winner}


def compare(results, metric="Mean R2"):
    """The reference's perform_statistical_comparison as data: per direction (in order of appearance; one without kNN or VAE results is
    left out, as there) the best kNN and the best VAE by mean_Mean R2 compared on `metric`, VAE against the mean baseline and, when
    present, the best site-conditioned kNN against the VAE.  Every pair: t, p, df, the two means and the winner under the reference's
    rule (p < 0.05; higher is better for R2 / Cosine / Pearson metrics, lower otherwise), None without a significant difference.
    With AE rows (model "ae") an entry also has best_ae, ae_vs_vae and ae_vs_knn: the best AE by mean_Mean R2 against the best VAE and
    the best kNN (vae_cross_modality_cv.py:491-502); without them the entries are what they were."""
    out = []
    for direction in dict.fromkeys(r["direction"] for r in results):
        rows = [r for r in results if r["direction"] == direction]
        by = {m: [r for r in rows if r["model"] == m] for m in MODELS + (AE_ROW,)}
        if not by["knn"] or not by["vae"]:
            continue
        best = {m: max(by[m], key=lambda r: r["mean_Mean R2"]) for m in by if by[m]}
        entry = {"direction": direction, "metric": metric, "best_knn": best["knn"]["param_value"], "best_vae": best["vae"]["param_value"],
                 "knn_vs_vae": _pair("kNN", best["knn"], "VAE", best["vae"], metric)}
        if by["mean"]:
            entry["vae_vs_mean"] = _pair("VAE", best["vae"], "Mean", by["mean"][0], metric)
        if by["knn_site"]:
            entry["best_knn_site"] = best["knn_site"]["param_value"]
            entry["knn_site_vs_vae"] = _pair("kNN-site", best["knn_site"], "VAE", best["vae"], metric)
        if by[AE_ROW]:
            entry["best_ae"] = best[AE_ROW]["param_value"]
            entry["ae_vs_vae"] = _pair("AE", best[AE_ROW], "VAE", best["vae"], metric)
            entry["ae_vs_knn"] = _pair("AE", best[AE_ROW], "kNN", best["knn"], metric)
        out.append(entry)
    return out


def aggregate(direction, model, param_name, param_value, elapsed, fold_metrics):
    """the reference's aggregated_results dict (vae_cross_modality_cv.py:395-407): np.mean and the population np.std per metric"""
    res = {"direction": direction, "model": model, "param_name": param_name, "param_value": param_value, "time": elapsed, "fold_metrics": fold_metrics}
    for name, scores in fold_metrics.items():
        res[f"mean_{name}"] = float(np.mean(scores))
        res[f"std_{name}"] = float(np.std(scores))
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------------------------------------
def _rows(t, idx):
    """rows idx of a device matrix in its storage: padded bf16 rows stay padded bf16 rows"""
    import torch
    from . import ops
    g = t[idx]
    return ops.to_bf16_rows(g) if t.dtype == torch.bfloat16 else g


def _fold_metrics(Y_folds, pred_of_fold):
    """{reference key: [one score per fold]} from ImputationMetrics on each fold's rows; pred_of_fold(f) -> (rows, F) or (F,)"""
    from .metrics import ImputationMetrics
    scores = {k: [] for k in METRIC_KEYS}
    for f, Yf in enumerate(Y_folds):
        m = ImputationMetrics(Yf.shape[1], Yf.device).update(Yf, pred_of_fold(f)).compute()
        for k, src in METRIC_KEYS.items():
            scores[k].append(float(m[src]))
    return scores


class BestState:
    """The early-stop bookkeeping of train_vae (vae_cross_modality_cv.py:129-194): the best validation loss, the epochs since, and the
    best epoch's state.  The state is a CLONE of the state_dict.  The reference keeps model.state_dict() itself, whose tensors go on
    training, so that what it restores is whatever came last; restoring the best epoch is deliberate here and differs from it."""

    def __init__(self, patience):
        self.patience, self.best, self.trigger, self.state, self.best_epoch = int(patience), float("inf"), 0, None, None

    def update(self, val_loss, model, epoch):
        """-> True when training stops"""
        if val_loss < self.best:
            self.best, self.trigger, self.best_epoch = val_loss, 0, epoch
            self.state = {k: v.detach().clone() for k, v in model.state_dict().items()}
            return False
        self.trigger += 1
        return self.trigger >= self.patience

    def restore(self, model):
        if self.state is not None:
            model.load_state_dict(self.state)


def fit_vae(kind, A, B, S, dims, *, epochs, batch_size, seed=42, fold=0, precision="bf16", eager=False, val_loss_fn=None):
    """train_vae of the reference (vae_cross_modality_cv.py:110-196) with the objects of trainer.run: a fresh DNA2RNAVAE / RNA2DNAVAE
    (kind "dna2rna" / "rna2dna") on the training rows A (RNA), B (DNA), S (int64 sites): inner_split() for early stopping, FusedAdamW,
    ReduceLROnPlateau, the beta warm-up, Config.PATIENCE, the captured GraphedTrainStep unless `eager`, drop_last batches of
    min(batch_size, inner training rows) rows from a device randperm seeded by (seed, fold, epoch), and the best epoch's state restored
    (BestState).  The model's initialisation and its noise stream are functions of (seed, fold): the Philox offset of the device is
    reset.  dims: (input_dim_a, input_dim_b, n_sites, latent_dim).  val_loss_fn(model, epoch) replaces the validation pass (tests).
    Returns (model in eval mode, BestState)."""
    from src.models import forward_loss, make_model
    return _fit(kind, lambda: make_model(kind, *dims), lambda model, a, b, s, beta: forward_loss(kind, model, a, b, s, beta, None),
                True, A, B, S, epochs=epochs, batch_size=batch_size, seed=seed, fold=fold, precision=precision, eager=eager, val_loss_fn=val_loss_fn)


def _ae_forward_loss(kind, model, a, b, s):
    """one reference-shaped AE forward + loss (vae_cross_modality_cv.py:225-237) -> the loss tensor"""
    from src.utils.ae_losses import dna2rna_ae_loss, rna2dna_ae_loss
    if kind == "dna2rna":
        return dna2rna_ae_loss(model(dna=b, site=s)[0], a)[0]
    return rna2dna_ae_loss(model(rna=a, site=s)[0], b)[0]


def fit_ae(kind, A, B, S, dims, *, epochs, batch_size, seed=42, fold=0, precision="bf16", eager=False, val_loss_fn=None):
    """train_ae of the reference (vae_cross_modality_cv.py:198-283) with the objects and the loop of fit_vae: a fresh DNA2RNAAE / RNA2DNAAE
    (kind "dna2rna" / "rna2dna"), the reconstruction loss alone (dna2rna_ae_loss / rna2dna_ae_loss), no beta warm-up; the captured
    step is GraphedTrainStep's kind "dna2rna_ae" / "rna2dna_ae".  Arguments and results as fit_vae."""
    from src.models import DNA2RNAAE, RNA2DNAAE
    cls = DNA2RNAAE if kind == "dna2rna" else RNA2DNAAE
    return _fit(AE_KINDS[kind], lambda: cls(dims[0], dims[1], dims[2], dims[3]), lambda model, a, b, s, beta: _ae_forward_loss(kind, model, a, b, s),
                False, A, B, S, epochs=epochs, batch_size=batch_size, seed=seed, fold=fold, precision=precision, eager=eager, val_loss_fn=val_loss_fn)


def _fit(step_kind, make_model, forward_loss, warm_beta, A, B, S, *, epochs, batch_size, seed, fold, precision, eager, val_loss_fn):
    """The training loop fit_vae and fit_ae share.  step_kind: the GraphedTrainStep kind; make_model() -> the fresh model (called after
    the seed is set); forward_loss(model, a, b, s, beta) -> the loss tensor of the eager step and of the validation pass; warm_beta:
    the KL weight follows the beta warm-up (else it stays 0)."""
    import torch
    from src.config import Config
    from . import engine
    from .graphs import GraphedTrainStep
    from .optim import FusedAdamW

    dev = A.device
    tr_rows, va_rows = (torch.from_numpy(r).to(dev) for r in inner_split(A.shape[0]))
    tr = [_rows(A, tr_rows), _rows(B, tr_rows), S[tr_rows].contiguous()]
    va = [_rows(A, va_rows), _rows(B, va_rows), S[va_rows].contiguous()]
    n_train = tr[0].shape[0]
    Bsz = min(int(batch_size), n_train)
    steps = n_train // Bsz
    run_seed = (int(seed) * 1000 + int(fold)) * 100003
    torch.manual_seed(run_seed)
    engine.GLOBAL_NOISE.load_state_dict({"offset": 0}, dev)
    model = make_model().to(dev).set_precision(precision)
    optimizer = FusedAdamW(model.parameters(), lr=Config.LEARNING_RATE, weight_decay=Config.WEIGHT_DECAY)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=Config.LR_SCHEDULER_FACTOR, patience=Config.LR_SCHEDULER_PATIENCE)
    graphed = None if eager else GraphedTrainStep(model, optimizer, beta=0.0, gamma=Config.GAMMA, warmup=1, preserve_state=True, kind=step_kind,
                                                  dataset=tuple(tr), batch_size=Bsz)
    perm_gen = torch.Generator(device=dev)
    best = BestState(Config.PATIENCE)
    for epoch in range(int(epochs)):
        model.train()
        beta = min(1.0, epoch / Config.BETA_WARMUP_EPOCHS) * Config.BETA_START if warm_beta else 0.0
        perm_gen.manual_seed(run_seed + 1 + epoch)
        order = torch.randperm(n_train, device=dev, generator=perm_gen)
        if graphed is not None:
            graphed.set_beta(beta)
            for i in range(steps):
                graphed.set_indices(order[i * Bsz:(i + 1) * Bsz])
                graphed.step_logged()
            graphed.flush_logged()
            graphed.reset_logged()
        else:
            for i in range(steps):
                idx = order[i * Bsz:(i + 1) * Bsz]
                loss = forward_loss(model, _rows(tr[0], idx), _rows(tr[1], idx), tr[2][idx], beta)
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
        model.eval()
        if val_loss_fn is not None:
            val_loss = float(val_loss_fn(model, epoch))
        else:
            total, nb = 0.0, 0
            with torch.no_grad():
                for i in range(0, va[0].shape[0], Bsz):
                    total += forward_loss(model, va[0][i:i + Bsz], va[1][i:i + Bsz], va[2][i:i + Bsz], beta).item()
                    nb += 1
            val_loss = total / max(nb, 1)
        scheduler.step(val_loss)
        if best.update(val_loss, model, epoch):
            break
    best.restore(model)
    model.eval()
    return model, best


def _predict(kind, model, X, S, chunk=4096):
    """one eval-mode forward of the rows -> fp32 (rows, outputs): the first of a VAE's three results (eps is drawn in eval mode too, as
    the reference's models do) or of an AE's two"""
    import torch
    out = []
    with torch.no_grad():
        for i in range(0, X.shape[0], chunk):
            x, s = X[i:i + chunk], S[i:i + chunk]
            rec = model(dna=x, site=s)[0] if kind == "dna2rna" else model(rna=x, site=s)[0]
            out.append(rec.float())
    return torch.cat(out)


def masked_neighbours(X, fold32, k, site32=None):
    """int32 (N, k): for every row its k nearest rows (euclidean, shift = the column means) outside its own fold -- and, with site32,
    inside its own site -- from ONE grouped search; -1 behind a list of fewer than k.  With sites the rows are stably sorted by site
    first, so that the search skips the tiles of other sites, and the answer is mapped back to the caller's row numbers."""
    import torch
    from . import ops
    shift = ops._column_means(X)
    if site32 is None:
        return ops.knn_search_grouped(X, X, k, differ=(fold32, fold32), shift=shift, dist=False)[0]
    order = torch.argsort(site32, stable=True)
    Xs, fs, ss = _rows(X, order), fold32[order].contiguous(), site32[order].contiguous()
    idx, _ = ops.knn_search_grouped(Xs, Xs, k, same=(ss, ss), differ=(fs, fs), shift=shift, dist=False)
    mapped = torch.where(idx >= 0, order[idx.clamp(min=0).long()].int(), idx)
    out = torch.empty_like(mapped)
    out[order] = mapped
    return out


def knn_predictions(X, Y, fold32, k_values, site32=None):
    """{k: fp32 (N, outputs)}: every row predicted as the mean of the Y rows of its k nearest admitted rows, for all k from ONE
    masked_neighbours() at max(k_values) (neighbours come ascending by (key, index): the first k columns are the k-search).  Without
    sites a row with fewer than max(k_values) candidates raises ValueError, as sklearn's kneighbors does.  With sites a row with
    0 < c < k candidates averages its c (the reference's conditioned regressor takes k = min(n_neighbors, rows of the site)) and one
    with none predicts zeros (conditioned_knn.py:78-85)."""
    import torch
    from . import ops
    ks = sorted({int(k) for k in k_values})
    kmax = ks[-1]
    idx = masked_neighbours(X, fold32, kmax, site32)
    if site32 is None:
        if bool((idx[:, kmax - 1] < 0).any()):
            raise ValueError(f"cross-validation k-NN: some row has fewer than n_neighbors = {kmax} rows outside its fold")
        return {k: ops.knn_mean_rows(idx[:, :k], Y) for k in ks}
    found = (idx >= 0).sum(dim=1)                                             # lists are filled from the front
    out = {}
    for k in ks:
        pred = torch.zeros(X.shape[0], Y.shape[1], dtype=torch.float32, device=X.device)
        c = torch.clamp(found, max=k)
        for cv in torch.unique(c).tolist():                                   # rows grouped by their count: -1 never reaches knn_mean_rows
            if cv > 0:
                rows = torch.nonzero(c == cv).squeeze(1)
                pred[rows] = ops.knn_mean_rows(idx[rows][:, :cv].contiguous(), Y)
        out[k] = pred
    return out


def cross_validate(X, Y, site, fold, direction, models=("mean", "knn", "vae"), k_values=(5, 10), *, epochs=200, batch_size=32, seed=42,
                   precision="bf16", eager=False, latent_dim=None, n_sites=None, log=None, predictions=None):
    """run_cross_validation of the reference for one direction ("DNA -> RNA" / "RNA -> DNA") on the device.  X (N, Fx) inputs and
    Y (N, Fy) targets: fp32 or padded-bf16-row device matrices; site (N,) and fold (N,) integer codes (host or device; fold from
    kfold_assignments).  models: any of "mean", "knn", "knn_site", "vae", "autoencoder".  Returns the reference's aggregated_results dicts
    in the reference's order: mean, knn per k, knn_site per k, vae, ae.  Fold metrics are ImputationMetrics on that fold's rows under the
    reference's six keys (METRIC_KEYS).
      mean      per fold the column means of the other folds' Y rows, float64 (total column sums minus the fold's)
      knn       knn_predictions(): one fold-masked search for all folds and all k
      knn_site  the same with the site condition
      vae       per fold fit_vae() on the other folds' rows, then one eval-mode forward of the fold's rows
      autoencoder  the same with fit_ae(): the rows carry the reference's model name "ae" (the name "ae" itself is refused here)
    log(result) is called as results arrive.  predictions: a dict that receives {(model, param_value): fp32 (N, Fy)}, every row as its
    own fold's model predicted it (the mean baseline's rows are not materialised)."""
    import torch
    from . import ops
    if direction not in DIRECTIONS:
        raise ValueError(f"direction must be one of {sorted(DIRECTIONS)}")
    unknown = [m for m in models if m not in MODELS + (AE_MODEL,)]
    if unknown:
        raise ValueError(f"models {unknown}: any of {MODELS + (AE_MODEL,)}")
    X, Y = ops._device_matrix(X, "X", "cross_validate"), ops._device_matrix(Y, "Y", "cross_validate")
    N, dev = X.shape[0], X.device
    site = torch.as_tensor(site).to(dev).long().reshape(-1)
    fold_h = np.asarray(fold.cpu() if isinstance(fold, torch.Tensor) else fold).astype(np.int64).reshape(-1)
    if Y.shape[0] != N or site.shape[0] != N or fold_h.shape[0] != N:
        raise ValueError(f"cross_validate: X {tuple(X.shape)}, Y {tuple(Y.shape)}, {site.shape[0]} sites, {fold_h.shape[0]} fold codes")
    n_folds = int(fold_h.max()) + 1
    if fold_h.min() < 0 or n_folds < 2 or len(np.unique(fold_h)) != n_folds:
        raise ValueError("cross_validate: fold codes must be 0 .. folds - 1, every fold present, at least 2 folds")
    say = log if log is not None else (lambda *_: None)
    fold_rows = [torch.from_numpy(np.flatnonzero(fold_h == f)).to(dev) for f in range(n_folds)]          # ascending, as X[val_index]
    Y_folds = [_rows(Y, r) for r in fold_rows]
    fold32 = torch.from_numpy(fold_h.astype(np.int32)).to(dev)
    results = []

    if "mean" in models:
        t0 = time.time()
        Y64 = Y.double()
        total = Y64.sum(dim=0)
        means = [((total - Y64[r].sum(dim=0)) / (N - r.numel())).float().contiguous() for r in fold_rows]
        scores = _fold_metrics(Y_folds, lambda f: means[f])
        results.append(aggregate(direction, "mean", "dummy", 0, time.time() - t0, scores))
        say(results[-1])
    for model, sites in (("knn", None), ("knn_site", site.int().contiguous())):
        if model not in models:
            continue
        t0 = time.time()
        preds = knn_predictions(X, Y, fold32, k_values, sites)
        torch.cuda.synchronize(dev)
        t_search = time.time() - t0
        if predictions is not None:
            predictions.update({(model, k): p for k, p in preds.items()})
        for k in k_values:
            t1 = time.time()
            scores = _fold_metrics(Y_folds, lambda f: preds[int(k)][fold_rows[f]])
            results.append(aggregate(direction, model, "k", int(k), t_search / len(k_values) + time.time() - t1, scores))
            say(results[-1])
    for name, row_name, fit in (("vae", "vae", fit_vae), (AE_MODEL, AE_ROW, fit_ae)):
        if name not in models:
            continue
        kind = DIRECTIONS[direction]
        A, B = (Y, X) if kind == "dna2rna" else (X, Y)
        from src.config import Config
        dims = (A.shape[1], B.shape[1], int(n_sites) if n_sites is not None else int(site.max()) + 1,
                int(latent_dim) if latent_dim is not None else Config.LATENT_DIM)
        t0 = time.time()
        preds = []
        for f in range(n_folds):
            rows = torch.from_numpy(np.flatnonzero(fold_h != f)).to(dev)
            model, _ = fit(kind, _rows(A, rows), _rows(B, rows), site[rows].contiguous(), dims, epochs=epochs, batch_size=batch_size,
                           seed=seed, fold=f, precision=precision, eager=eager)
            preds.append(_predict(kind, model, _rows(X, fold_rows[f]), site[fold_rows[f]].contiguous()))
        scores = _fold_metrics(Y_folds, lambda f: preds[f])
        torch.cuda.synchronize(dev)
        if predictions is not None:
            full = torch.zeros(N, Y.shape[1], dtype=torch.float32, device=dev)
            for r, p in zip(fold_rows, preds):
                full.index_add_(0, r, p)                                      # a row predicted twice would show
            predictions[(row_name, int(epochs))] = full
        results.append(aggregate(direction, row_name, "epochs", int(epochs), time.time() - t0, scores))
        say(results[-1])
    return results
