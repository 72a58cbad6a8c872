"""The downstream task of the reference (downstream_task.py, downstream_task_directional.py): does a site classifier learn as well
from the model's estimated modality as from the measured one?  SiteClassifier is its SimpleMLP -- Linear -> [LayerNorm] -> ReLU ->
Dropout blocks and a Linear head -- trained on the device: a step is gather_rows of the shuffled batch, per layer mmvae_gemm_nt (fp32
MFMA) -> mmvae_ln_act_fwd, mmvae_wce_mean, per layer backwards mmvae_ln_act_bwd -> mmvae_gemm_nt on the transposed weight ->
mmvae_gemm_tn, and ONE mmvae_adam_step over the parameter arena.  Learning rate, step count and Philox offset live on the device: the
step has no host synchronisation, the full-batch step is captured once as a hipGraph and replayed, the last shorter batch of an epoch
runs eagerly.  fit() follows the reference's loop (Adam(1e-3, weight_decay=1e-4), ReduceLROnPlateau(min, 0.5, 5) on the mean of the
per-batch validation losses, early stopping on validation accuracy with patience 10) with one host read-back per epoch.

There is no CPU fallback: a CPU tensor raises."""
import math

import numpy as np
import torch

from . import _lib as L
from . import ops
from .clustering import standardize
from .data import balanced_class_weights

BATCH_SIZE = 32                 # Config.BATCH_SIZE of the reference
LN_EPS = 1e-5                   # nn.LayerNorm's default
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


def _ceil4(n):
    return (n + 3) // 4 * 4


# --------------------------------------------------------------------------------------------
# host arithmetic: the report, the folds
# --------------------------------------------------------------------------------------------
def classification_report(confusion, names):
    """The dict of sklearn.metrics.classification_report(y_true, y_pred, target_names=names, labels=arange(C), output_dict=True,
    zero_division=0) from the C x C counts confusion[true][predicted]."""
    cm = np.asarray(confusion.cpu() if isinstance(confusion, torch.Tensor) else confusion).astype(np.int64)
    Cn = cm.shape[0]
    if cm.shape != (Cn, Cn) or len(names) != Cn:
        raise ValueError(f"classification_report: confusion is {cm.shape} for {len(names)} names")
    tp = np.diag(cm).astype(np.float64)
    support = cm.sum(axis=1)
    predicted = cm.sum(axis=0)
    total = int(cm.sum())

    def ratio(num, den):
        return np.divide(num, den, out=np.zeros_like(num, dtype=np.float64), where=den != 0)
    precision, recall = ratio(tp, predicted.astype(np.float64)), ratio(tp, support.astype(np.float64))
    f1 = ratio(2 * precision * recall, precision + recall)
    report = {str(n): {"precision": float(precision[c]), "recall": float(recall[c]), "f1-score": float(f1[c]), "support": float(support[c])}
              for c, n in enumerate(names)}
    report["accuracy"] = float(tp.sum() / total) if total else 0.0

    def average(w):
        if w is not None and w.sum() == 0:
            return 0.0, 0.0, 0.0
        return tuple(float(np.average(x, weights=w)) for x in (precision, recall, f1))
    for key, w in (("macro avg", None), ("weighted avg", support.astype(np.float64))):
        p, r, f = average(w)
        report[key] = {"precision": p, "recall": r, "f1-score": f, "support": float(total)}
    return report


def stratified_kfold(labels, n_splits, seed):
    """[(train_idx, test_idx)] of a shuffled stratified n_splits-fold split.  The number of rows of every class in every test fold equals
    sklearn's StratifiedKFold (its allocation rule: the sorted class codes dealt round-robin over the folds); which rows of a class go to
    which fold is drawn from numpy's default_rng(seed), not from sklearn's RandomState -- membership is not sklearn's bit for bit."""
    y = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
    n = y.shape[0]
    if not 2 <= n_splits <= n:
        raise ValueError(f"stratified_kfold: n_splits = {n_splits} outside [2, {n}]")
    _, first, inv = np.unique(y, return_index=True, return_inverse=True)
    rank = np.empty(first.shape[0], dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.shape[0])         # classes numbered in order of first appearance
    code = rank[inv]
    k = first.shape[0]
    counts = np.bincount(code, minlength=k)
    if (counts < n_splits).all():
        raise ValueError(f"stratified_kfold: n_splits = {n_splits} exceeds the rows of every class")
    order = np.sort(code)
    allocation = np.stack([np.bincount(order[i::n_splits], minlength=k) for i in range(n_splits)])
    rng = np.random.default_rng(seed)
    fold = np.empty(n, dtype=np.int64)
    for c in range(k):
        f = np.repeat(np.arange(n_splits), allocation[:, c])
        rng.shuffle(f)
        fold[code == c] = f
    idx = np.arange(n)
    return [(idx[fold != i], idx[fold == i]) for i in range(n_splits)]


class ReduceLROnPlateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', factor, patience) with its defaults threshold = 1e-4 (relative), cooldown 0,
    min_lr 0, eps 1e-8, on a plain number."""

    def __init__(self, lr, factor=0.5, patience=5, threshold=1e-4, eps=1e-8):
        self.lr, self.factor, self.patience, self.threshold, self.eps = float(lr), factor, patience, threshold, eps
        self.best, self.bad = math.inf, 0

    def step(self, metric):
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            new = self.lr * self.factor
            if self.lr - new > self.eps:
                self.lr = new
            self.bad = 0
        return self.lr


class EarlyStopping:
    """The reference's rule (downstream_task.py:135-143): a strictly better validation accuracy resets the count; `patience` epochs in a
    row without one stop the run."""

    def __init__(self, patience=10):
        self.patience, self.best, self.count, self.best_epoch = patience, 0.0, 0, -1

    def step(self, accuracy, epoch):
        """-> (improved, stop)"""
        if accuracy > self.best:
            self.best, self.count, self.best_epoch = accuracy, 0, epoch
            return True, False
        self.count += 1
        return False, self.count >= self.patience


# --------------------------------------------------------------------------------------------
# the classifier
# --------------------------------------------------------------------------------------------
class _Buffers:
    """Activations and gradients of one batch size"""

    def __init__(self, net, rows, train):
        dev, f32 = net.device, torch.float32
        self.rows = rows
        self.z = [torch.empty(rows, h, dtype=f32, device=dev) for h in net.hidden]
        self.y = [torch.empty(rows, h, dtype=f32, device=dev) for h in net.hidden]
        self.mean = [torch.empty(rows, dtype=f32, device=dev) if net.layer_norm else None for _ in net.hidden]
        self.rstd = [torch.empty(rows, dtype=f32, device=dev) if net.layer_norm else None for _ in net.hidden]
        self.logits = torch.empty(rows, _ceil4(net.n_classes), dtype=f32, device=dev)[:, :net.n_classes]
        if not train:
            return
        # rows padded with zeros to a multiple of 4 columns: the first GEMM then reads 16-byte words at any input width (the prepared
        # weight is zero there too); self.x is the view the batch is gathered into
        self.x_pad = torch.zeros(rows, _ceil4(net.input_dim), dtype=f32, device=dev)
        self.x = self.x_pad[:, :net.input_dim]
        self.labels = torch.empty(rows, dtype=torch.int64, device=dev)
        self.idx = torch.zeros(rows, dtype=torch.int64, device=dev)
        self.masks = [torch.empty(rows, h, dtype=torch.uint8, device=dev) if p > 0 else None for h, p in zip(net.hidden, net.dropout)]
        self.g = torch.empty(rows, _ceil4(net.n_classes), dtype=f32, device=dev)[:, :net.n_classes]
        self.dy = [torch.empty(rows, h, dtype=f32, device=dev) for h in net.hidden]
        self.dz = [torch.empty(rows, h, dtype=f32, device=dev) for h in net.hidden]
        self.work = [ops._workspace(ops.ln_act_bwd_work_bytes(rows, h, net.layer_norm), dev) for h in net.hidden]


class SiteClassifier:
    """SimpleMLP of the reference on the device.  hidden=(256, 128), layer_norm=True, dropout=(0.3, 0.2): downstream_task.py:55-72;
    hidden=(128,), layer_norm=False, dropout=(0.2,): downstream_task_directional.py:151-162.  state_dict() has the keys of the reference's
    nn.Sequential (fc.0.weight, ...), so a checkpoint of either side loads in the other."""

    def __init__(self, input_dim, n_classes, hidden=(256, 128), layer_norm=True, dropout=(0.3, 0.2), seed=0, device=None,
                 lr=1e-3, weight_decay=1e-4, batch_size=BATCH_SIZE):
        hidden, dropout = tuple(int(h) for h in hidden), tuple(float(p) for p in dropout)
        if input_dim < 1 or not 2 <= n_classes <= L.WCE_MAXC:
            raise ValueError(f"SiteClassifier: input_dim = {input_dim}, n_classes = {n_classes} (2 .. {L.WCE_MAXC})")
        if not hidden or len(hidden) != len(dropout) or any(h % 4 or not 4 <= h <= L.LN_MAXN for h in hidden):
            raise ValueError(f"SiteClassifier: hidden = {hidden} needs one dropout probability per layer and widths that are multiples of 4 up to {L.LN_MAXN}")
        if any(not 0.0 <= p < 1.0 for p in dropout) or batch_size < 1 or lr <= 0 or weight_decay < 0:
            raise ValueError("SiteClassifier: dropout in [0, 1), batch_size >= 1, lr > 0, weight_decay >= 0")
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("SiteClassifier: needs a CUDA/HIP device; there is no CPU fallback")
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("SiteClassifier: needs a CUDA/HIP device; there is no CPU fallback")
        self.input_dim, self.n_classes, self.hidden, self.layer_norm, self.dropout = int(input_dim), int(n_classes), hidden, bool(layer_norm), dropout
        self.device, self.seed, self.batch_size, self.weight_decay = device, int(seed), int(batch_size), float(weight_decay)
        self.training = True
        # one arena each for parameters, gradients and the two moments: one record for mmvae_adam_step, one memset for the gradients
        dims = (self.input_dim,) + hidden + (self.n_classes,)
        stride = 4 if self.layer_norm else 3
        layout, off = [], 0
        for l in range(len(dims) - 1):
            entries = [(f"fc.{stride * l}.weight", (dims[l + 1], dims[l])), (f"fc.{stride * l}.bias", (dims[l + 1],))]
            if self.layer_norm and l < len(hidden):
                entries += [(f"fc.{stride * l + 1}.weight", (dims[l + 1],)), (f"fc.{stride * l + 1}.bias", (dims[l + 1],))]
            for key, shape in entries:
                layout.append((key, shape, off))
                off += _ceil4(int(np.prod(shape)))                 # every tensor starts 16-byte aligned
        self._flat = {k: torch.zeros(off, dtype=torch.float32, device=device) for k in ("p", "g", "m", "v")}

        def views(flat):
            return {key: flat[o:o + int(np.prod(shape))].view(shape) for key, shape, o in layout}
        self.params, self.grads = views(self._flat["p"]), views(self._flat["g"])
        self._keys = [k for k, _, _ in layout]
        self._linear_keys = [f"fc.{stride * l}" for l in range(len(dims) - 1)]
        self._ln_keys = [f"fc.{stride * l + 1}" for l in range(len(hidden))] if self.layer_norm else []
        self._init_parameters()
        self._prep = [ops.PreparedLinear([self.params[k + ".weight"]], [self.params[k + ".bias"]], L.PREC_F32, device) for k in self._linear_keys]
        self._weight_prep = ops.WeightPrep(self._prep, device)
        self._slab = torch.empty(max(dims[l + 1] * dims[l] for l in range(len(dims) - 1)), dtype=torch.float32, device=device)
        self._adam_items = (L.AdamWItem * 1)(L.AdamWItem(*(self._flat[k].data_ptr() for k in ("p", "g", "m", "v")), off))
        self._lr = torch.tensor([float(lr)], dtype=torch.float32, device=device)
        self.lr = float(lr)
        self._step = torch.zeros(L.CTR_COPIES, dtype=torch.int64, device=device)
        self._offset = torch.zeros(1, dtype=torch.int64, device=device)                # Philox offset of the dropout masks
        self.loss_sums = torch.zeros(3, dtype=torch.float64, device=device)        # sum w nll, sum w, bad labels of the training steps so far
        self._train_buf, self._eval_buf, self._graph = {}, {}, None
        self._data = None
        self._weight_prep.run()

    # ---- parameters ------------------------------------------------------------------------
    def _init_parameters(self):
        """nn.Linear's default (kaiming_uniform(a = sqrt 5): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for weight and bias) and nn.LayerNorm's
        (ones, zeros), drawn on the host from torch.Generator(seed)."""
        gen = torch.Generator().manual_seed(self.seed)
        for k in self._linear_keys:
            w = self.params[k + ".weight"]
            bound = 1.0 / math.sqrt(w.shape[1])
            w.copy_((torch.rand(w.shape, generator=gen) * 2 - 1) * bound)
            b = self.params[k + ".bias"]
            b.copy_((torch.rand(b.shape, generator=gen) * 2 - 1) * bound)
        for k in self._ln_keys:
            self.params[k + ".weight"].fill_(1.0)
            self.params[k + ".bias"].zero_()

    def state_dict(self):
        return {k: self.params[k].detach().clone() for k in self._keys}

    def load_state_dict(self, state):
        missing = [k for k in self._keys if k not in state]
        bad = [k for k in self._keys if k in state and tuple(state[k].shape) != tuple(self.params[k].shape)]
        if missing or bad:
            raise ValueError(f"SiteClassifier.load_state_dict: missing {missing[:4]}, shape mismatch {bad[:4]}")
        for k in self._keys:
            self.params[k].copy_(state[k].to(torch.float32))
        self._weight_prep.run()

    def reset_optimizer(self, lr=None):
        self._flat["m"].zero_(); self._flat["v"].zero_(); self._step.zero_()
        if lr is not None:
            self.set_lr(lr)

    def set_lr(self, lr):
        """the device scalar every step reads: a captured graph follows the scheduler without re-capture"""
        if float(lr) != self.lr:
            self.lr = float(lr)
            self._lr.fill_(self.lr)

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    # ---- forward / backward ----------------------------------------------------------------
    def _forward(self, x, buf, masks):
        a, K = x, x.shape[1]                                       # the training buffers' padded rows, or the caller's matrix as it is
        for l, h in enumerate(self.hidden):
            pl = self._prep[l]
            ops.gemm_nt(L.PREC_F32, a, pl.w, h, K, buf.z[l], bias=pl.bias)
            gamma = self.params[self._ln_keys[l] + ".weight"] if self.layer_norm else None
            beta = self.params[self._ln_keys[l] + ".bias"] if self.layer_norm else None
            mask = masks[l] if masks is not None else None
            ops.ln_act_fwd(buf.z[l], gamma, beta, mask, self.dropout[l] if mask is not None else 0.0, LN_EPS,
                           y_out=buf.y[l], mean_out=buf.mean[l], rstd_out=buf.rstd[l])
            a, K = buf.y[l], h
        pl = self._prep[-1]
        ops.gemm_nt(L.PREC_F32, a, pl.w, self.n_classes, K, buf.logits, bias=pl.bias)
        return buf.logits

    def _backward(self, x, buf):
        n = len(self.hidden)
        head = self._linear_keys[-1]
        ops.gemm_nt(L.PREC_F32, buf.g, self._prep[-1].wt, self.hidden[-1], self.n_classes, buf.dy[-1])
        ops.gemm_tn(L.PREC_F32, buf.g, buf.y[-1], self.grads[head + ".weight"], self.grads[head + ".bias"], self.n_classes, self.hidden[-1],
                    nsplit=1, slab=self._slab)
        for l in range(n - 1, -1, -1):
            ln = self._ln_keys[l] if self.layer_norm else None
            ops.ln_act_bwd(buf.dy[l], buf.z[l], buf.mean[l], buf.rstd[l], self.params[ln + ".weight"] if ln else None,
                           self.params[ln + ".bias"] if ln else None, buf.masks[l], self.dropout[l], dz_out=buf.dz[l],
                           dgamma_out=self.grads[ln + ".weight"] if ln else None, dbeta_out=self.grads[ln + ".bias"] if ln else None, work=buf.work[l])
            K = self.hidden[l - 1] if l else self.input_dim
            if l:                                                  # the first layer's input needs no gradient
                ops.gemm_nt(L.PREC_F32, buf.dz[l], self._prep[l].wt, K, self.hidden[l], buf.dy[l - 1])
            key = self._linear_keys[l]
            ops.gemm_tn(L.PREC_F32, buf.dz[l], buf.y[l - 1] if l else x, self.grads[key + ".weight"], self.grads[key + ".bias"], self.hidden[l], K,
                        nsplit=1, slab=self._slab)

    def _train_buffers(self, rows):
        if rows not in self._train_buf:
            self._train_buf[rows] = _Buffers(self, rows, True)
        return self._train_buf[rows]

    def _draw_masks(self, buf):
        # One device counter for all layers, moved by a one-thread launch behind them.  Not the self-advancing form of mmvae_noise: its
        # launch rewrites CTR_COPIES copies of the counter, grid-many at a time, and a 32 x 256 mask is a grid of two workgroups -- 0.3 ms
        # per mask, three quarters of the whole step when it was measured (profiles/downstream_bench.json has the step without it).
        used = 0
        for mask, p in zip(buf.masks, self.dropout):
            if mask is not None:
                used += ops.noise(mask, None, 1.0 - p, self.seed, used, offset_dev=self._offset)
        if used:
            ops.counter_add(self._offset, used)

    def _step_on(self, buf, class_weights, masks_given=False):
        """One optimiser step on the batch in buf.x / buf.labels: launches only, nothing is read back."""
        if not masks_given:
            self._draw_masks(buf)
        self._forward(buf.x_pad, buf, buf.masks)
        ops.wce_mean(buf.logits, buf.labels, class_weights, sums=self.loss_sums, grad_out=buf.g)
        self._flat["g"].zero_()                                    # mmvae_gemm_tn accumulates
        self._backward(buf.x, buf)
        ops.adam_step(self._adam_items, self.lr, ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, self.weight_decay, 1.0, 1.0, step_dev=self._step,
                      lr_dev=self._lr)
        self._weight_prep.run()

    def train_step(self, x, labels, class_weights=None, masks=None):
        """One eager step on the batch (x fp32 (B, input_dim), labels int64 (B,)) on the device.  masks: uint8 keep masks per hidden layer to
        use instead of drawing them.  Returns the buffers of the step (logits, gradients and masks stay readable until the next one)."""
        self._check_xy(x, labels)
        buf = self._train_buffers(x.shape[0])
        buf.x.copy_(x); buf.labels.copy_(labels)
        if masks is not None:
            for dst, src in zip(buf.masks, masks):
                if dst is not None:
                    dst.copy_(src)
        self._step_on(buf, self._weights(class_weights), masks_given=masks is not None)
        return buf

    def _check_xy(self, x, labels=None):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("SiteClassifier: features must be a CUDA/HIP tensor; there is no CPU fallback")
        if x.dim() != 2 or x.shape[1] != self.input_dim or x.dtype != torch.float32 or x.shape[0] < 1:
            raise ValueError(f"SiteClassifier: features must be fp32 (rows, {self.input_dim}), got {tuple(x.shape)} {x.dtype}")
        if labels is not None:
            if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
                raise RuntimeError("SiteClassifier: labels must be a CUDA/HIP tensor; there is no CPU fallback")
            if labels.dtype != torch.int64 or tuple(labels.shape) != (x.shape[0],):
                raise ValueError(f"SiteClassifier: labels must be int64 ({x.shape[0]},)")

    def _weights(self, class_weights):
        if class_weights is None:
            return None
        w = torch.as_tensor(class_weights, dtype=torch.float32).to(self.device).contiguous()
        if tuple(w.shape) != (self.n_classes,):
            raise ValueError(f"SiteClassifier: class_weights must have {self.n_classes} entries")
        return w

    # ---- an epoch over a device-resident training set --------------------------------------
    def set_data(self, X, y, class_weights=None, graph=True):
        """The training set of train_epoch(): X fp32 (n, input_dim) and y int64 (n,) on the device.  graph: capture the full-batch step as a
        hipGraph (the first call of train_epoch does it) and replay it; the last shorter batch runs eagerly either way."""
        self._check_xy(X, y)
        bad = int(((y < 0) | (y >= self.n_classes)).sum())
        if bad:
            raise ValueError(f"SiteClassifier: {bad} labels outside [0, {self.n_classes})")
        self._data = (X.contiguous(), y.contiguous(), self._weights(class_weights))
        self._use_graph, self._graph = bool(graph), None

    def _batch_launches(self, buf, n):
        X, y, w = self._data
        ops.gather_rows([(X, buf.x), (y, buf.labels)], buf.idx, n)
        self._step_on(buf, w)

    def train_epoch(self, generator=None):
        """One pass over set_data()'s rows in shuffled batches of batch_size, the last shorter one included (the reference's DataLoader does
        not drop it).  Enqueues only."""
        X, y, w = self._data
        n, B = X.shape[0], self.batch_size
        perm = torch.randperm(n, generator=generator).to(self.device, non_blocking=True) if generator is not None \
            else torch.randperm(n, device=self.device)
        full = n // B
        if full:
            buf = self._train_buffers(B)
            if self._use_graph and self._graph is None:
                buf.idx.copy_(perm[:B])
                self._graph = self._capture(buf, n)
            for i in range(full):
                buf.idx.copy_(perm[i * B:(i + 1) * B])
                if self._graph is not None:
                    self._graph.replay()
                else:
                    self._batch_launches(buf, n)
        if n % B:
            tail = self._train_buffers(n % B)
            tail.idx.copy_(perm[full * B:])
            self._batch_launches(tail, n)

    def _capture(self, buf, n):
        """The full-batch step as a hipGraph.  Capture only records the launches: no counter moves and no parameter changes until a replay."""
        # an eager warm-up first (kernels are loaded on their first launch, which a capture does not allow), then everything it moved is put back
        state = [(t, t.clone()) for t in (self._flat["p"], self._flat["m"], self._flat["v"], self._step, self._offset, self.loss_sums)]
        self._batch_launches(buf, n)
        for t, saved in state:
            t.copy_(saved)
        self._weight_prep.run()
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._batch_launches(buf, n)
        return graph

    # ---- evaluation ------------------------------------------------------------------------
    def logits(self, x):
        """eval-mode forward: fp32 (rows, n_classes), a view of a buffer that the next call of the same size overwrites"""
        self._check_xy(x)
        rows = x.shape[0]
        if rows not in self._eval_buf:
            self._eval_buf = {rows: _Buffers(self, rows, False)}
        return self._forward(x.contiguous(), self._eval_buf[rows], None)

    def evaluate(self, x, labels, class_weights=None, batch_size=None):
        """Eval-mode pass over (x, labels) as ONE batch (LayerNorm is per row: the result does not depend on the batching).  Returns device
        tensors, nothing is read back: stats float64 (3,) = [mean of the per-batch weighted mean losses over consecutive batches of
        batch_size rows, as the reference's validation loop forms it; correct predictions; labels out of range], pred int32 (rows,) and
        confusion int32 (C, C)."""
        self._check_xy(x, labels)
        w = self._weights(class_weights)
        B = batch_size or self.batch_size
        logits = self.logits(x)
        rows = x.shape[0]
        sums = torch.zeros(3, dtype=torch.float64, device=self.device)
        confusion = torch.zeros(self.n_classes, self.n_classes, dtype=torch.int32, device=self.device)
        _, pred, nll = ops.wce_mean(logits, labels, w, sums=sums, pred=True, nll=True, confusion=confusion)
        wr = (w[labels.clamp(0, self.n_classes - 1)] if w is not None else torch.ones(rows, device=self.device)).double()
        pad = (-rows) % B
        num = torch.nn.functional.pad(wr * nll.double(), (0, pad)).view(-1, B).sum(dim=1)
        den = torch.nn.functional.pad(wr, (0, pad)).view(-1, B).sum(dim=1)
        stats = torch.stack([(num / den).mean(), (pred == labels).sum().double(), sums[2]])
        return stats, pred, confusion

    # ---- the reference's training loop -----------------------------------------------------
    def fit(self, X_tr, y_tr, X_val, y_val, class_weights=None, *, epochs=100, lr=1e-3, factor=0.5, lr_patience=5, patience=10,
            restore_best=False, graph=True, generator=None, log=None):
        """train_and_evaluate_fold's loop (downstream_task.py:74-159).  One host read-back per epoch: three numbers.  restore_best=False keeps
        the reference's observable behaviour -- its `best_model_state = model.state_dict()` aliases the live tensors, so its "load best"
        restores nothing and the reported model is the last epoch's; restore_best=True reports the epoch of the best validation accuracy.
        Returns dict(confusion (C, C) int64 numpy of the reported model on the validation rows, epochs run, best_epoch, best_acc, history
        [(val loss, val acc, lr)])."""
        self.set_data(X_tr, y_tr, class_weights, graph=graph)
        self._check_xy(X_val, y_val)
        self.reset_optimizer(lr)
        sched, stop = ReduceLROnPlateau(lr, factor, lr_patience), EarlyStopping(patience)
        best_state, history = None, []
        for epoch in range(epochs):
            self.train()
            self.train_epoch(generator)
            self.eval()
            stats, _, confusion = self.evaluate(X_val, y_val, self._data[2])
            val_loss, correct, bad = stats.tolist()                 # the epoch's one read-back
            if bad:
                raise ValueError(f"SiteClassifier.fit: {int(bad)} validation labels outside [0, {self.n_classes})")
            acc = 100.0 * correct / X_val.shape[0]
            history.append((val_loss, acc, self.lr))
            if log is not None:
                log(epoch, val_loss, acc, self.lr)
            self.set_lr(sched.step(val_loss))
            improved, done = stop.step(acc, epoch)
            if improved and restore_best:
                best_state = (self.state_dict(), confusion)
            if done:
                break
        if restore_best and best_state is not None:
            self.load_state_dict(best_state[0])
            confusion = best_state[1]
        return dict(confusion=confusion.cpu().numpy().astype(np.int64), epochs=len(history), best_epoch=stop.best_epoch, best_acc=stop.best,
                    history=history)


# --------------------------------------------------------------------------------------------
# a scenario: standardise, stratified folds, a classifier per fold, the aggregated report
# --------------------------------------------------------------------------------------------
def aggregate_reports(reports, names):
    """The aggregated dict of run_classification_scenario (downstream_task.py:190-228): means and _std of accuracy, of the weighted
    averages and of the per-class rows over the folds."""
    out = {"accuracy": float(np.mean([r["accuracy"] for r in reports])), "accuracy_std": float(np.std([r["accuracy"] for r in reports]))}

    def block(key):
        d = {}
        for m in ("precision", "recall", "f1-score"):
            vals = [r[key][m] for r in reports if key in r]
            d[m], d[m + "_std"] = float(np.mean(vals)), float(np.std(vals))
        return d
    out["weighted avg"] = block("weighted avg")
    for n in names:
        if str(n) in reports[0]:
            out[str(n)] = block(str(n))
    return out


def cross_validate(features, labels, names, n_folds=5, *, epochs=100, seed=42, hidden=(256, 128), layer_norm=True, dropout=(0.3, 0.2),
                   restore_best=False, graph=True, log=None):
    """run_classification_scenario on the device: features (n, F) and labels int64 (n,) in [0, len(names)) on the device.  The features
    are standardised (clustering.standardize = StandardScaler), split into n_folds stratified folds (stratified_kfold(seed)), one
    SiteClassifier is trained per fold with the fold's balanced class weights, and the folds' classification reports are aggregated."""
    if not isinstance(features, torch.Tensor) or not features.is_cuda or not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise RuntimeError("cross_validate: features and labels must be CUDA/HIP tensors; there is no CPU fallback")
    n_classes = len(names)
    z = standardize(features.float())
    labels = labels.to(torch.int64).contiguous()
    reports = []
    for fold, (tr, te) in enumerate(stratified_kfold(labels, n_folds, seed)):
        tr, te = (torch.from_numpy(i).to(z.device) for i in (tr, te))
        weights = balanced_class_weights(labels[tr].cpu(), n_classes)
        net = SiteClassifier(z.shape[1], n_classes, hidden, layer_norm, dropout, seed=seed + fold, device=z.device)
        gen = torch.Generator().manual_seed(seed + fold)
        res = net.fit(z[tr], labels[tr], z[te], labels[te], weights, epochs=epochs, restore_best=restore_best, graph=graph, generator=gen,
                      log=(lambda *a, fold=fold: log(fold, *a)) if log is not None else None)
        reports.append(classification_report(res["confusion"], names))
        del net
    return aggregate_reports(reports, names)
