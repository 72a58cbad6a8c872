"""Float64 numpy restatement of the site classifier's kernels (include/mmvae_hip.h: mmvae_ln_act_fwd, mmvae_ln_act_bwd, mmvae_wce_mean,
mmvae_adam_step) and of one whole training step of mmvae.downstream.SiteClassifier.  tests/test_downstream_ref_cpu.py holds it to
stock torch in float64; the GPU tests hold the kernels to it within tests/downstream_bounds.py."""
import numpy as np

LN_EPS = 1e-5


def ln_act_fwd(z, gamma=None, beta=None, keep=None, p=0.0, eps=LN_EPS):
    """-> (y, mean, rstd, xhat, pre): Dropout(ReLU(LayerNorm(z))); gamma None: no LayerNorm (mean = 0, rstd = 1, pre = z)"""
    z = np.asarray(z, np.float64)
    if gamma is None:
        mean, rstd, xhat, pre = np.zeros(z.shape[0]), np.ones(z.shape[0]), z, z
    else:
        mean = z.mean(axis=1)
        var = ((z - mean[:, None]) ** 2).mean(axis=1)
        rstd = 1.0 / np.sqrt(var + eps)
        xhat = (z - mean[:, None]) * rstd[:, None]
        pre = xhat * gamma + beta
    scale = 1.0 if keep is None else np.asarray(keep, np.float64) / (1.0 - p)
    return np.maximum(pre, 0.0) * scale, mean, rstd, xhat, pre


def ln_act_bwd(dy, z, gamma=None, beta=None, keep=None, p=0.0, eps=LN_EPS):
    """-> (dz, dgamma, dbeta, g)"""
    dy = np.asarray(dy, np.float64)
    _, _, rstd, xhat, pre = ln_act_fwd(z, gamma, beta, None, 0.0, eps)
    scale = 1.0 if keep is None else np.asarray(keep, np.float64) / (1.0 - p)
    g = dy * scale * (pre > 0)
    if gamma is None:
        return g, None, None, g
    gg = g * gamma
    dz = rstd[:, None] * (gg - gg.mean(axis=1, keepdims=True) - xhat * (gg * xhat).mean(axis=1, keepdims=True))
    return dz, (g * xhat).sum(axis=0), g.sum(axis=0), g


def wce_mean(logits, labels, w=None):
    """-> dict(loss = sum w nll / sum w, sum_wnll, sum_w, g, pred (first maximum), nll, confusion [label][pred])"""
    x = np.asarray(logits, np.float64)
    M, C = x.shape
    y = np.asarray(labels, np.int64)
    w = np.ones(C) if w is None else np.asarray(w, np.float64)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    se = e.sum(axis=1, keepdims=True)
    nll = (m + np.log(se))[:, 0] - x[np.arange(M), y]
    wy = w[y]
    onehot = np.zeros((M, C))
    onehot[np.arange(M), y] = 1.0
    g = wy[:, None] * (e / se - onehot) / wy.sum()
    pred = x.argmax(axis=1)                                        # numpy's argmax returns the first maximum
    confusion = np.zeros((C, C), np.int64)
    np.add.at(confusion, (y, pred), 1)
    return dict(loss=(wy * nll).sum() / wy.sum(), sum_wnll=(wy * nll).sum(), sum_w=wy.sum(), g=g, pred=pred, nll=nll, confusion=confusion)


def adam_step(p, g, m, v, t, lr, wd, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam(lr, weight_decay=wd) at step count t (1 for the first step) -> (p, m, v)"""
    g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    return p - lr / bc1 * m / (np.sqrt(v) / np.sqrt(bc2) + eps), m, v


def adamw_step(p, g, m, v, t, lr, wd, b1=0.9, b2=0.999, eps=1e-8):
    """the decoupled form, for the list of mistakes"""
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    return p - lr / bc1 * m / (np.sqrt(v) / np.sqrt(bc2) + eps), m, v


class Net:
    """SimpleMLP in float64 with the state_dict keys of the reference's nn.Sequential"""

    def __init__(self, state, hidden, layer_norm, dropout):
        self.P = {k: np.asarray(v, np.float64).copy() for k, v in state.items()}
        self.hidden, self.layer_norm, self.dropout = tuple(hidden), layer_norm, tuple(dropout)
        self.stride = 4 if layer_norm else 3
        self.m = {k: np.zeros_like(v) for k, v in self.P.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.P.items()}
        self.t = 0

    def lin(self, l):
        return f"fc.{self.stride * l}"

    def ln(self, l):
        return f"fc.{self.stride * l + 1}"

    def forward(self, x, keeps=None):
        """-> (logits, cache); keeps: per hidden layer a 0 / 1 array or None (eval mode when keeps is None)"""
        a, cache = np.asarray(x, np.float64), []
        for l in range(len(self.hidden)):
            z = a @ self.P[self.lin(l) + ".weight"].T + self.P[self.lin(l) + ".bias"]
            gamma = self.P[self.ln(l) + ".weight"] if self.layer_norm else None
            beta = self.P[self.ln(l) + ".bias"] if self.layer_norm else None
            keep = keeps[l] if keeps is not None else None
            y = ln_act_fwd(z, gamma, beta, keep, self.dropout[l])[0]
            cache.append((a, z, keep))
            a = y
        n = len(self.hidden)
        return a @ self.P[self.lin(n) + ".weight"].T + self.P[self.lin(n) + ".bias"], cache + [(a, None, None)]

    def gradients(self, x, labels, w, keeps):
        """-> (loss, grads by key, logits)"""
        logits, cache = self.forward(x, keeps)
        r = wce_mean(logits, labels, w)
        G, n = {}, len(self.hidden)
        d = r["g"]
        G[self.lin(n) + ".weight"], G[self.lin(n) + ".bias"] = d.T @ cache[n][0], d.sum(axis=0)
        d = d @ self.P[self.lin(n) + ".weight"]
        for l in range(n - 1, -1, -1):
            a, z, keep = cache[l]
            gamma = self.P[self.ln(l) + ".weight"] if self.layer_norm else None
            beta = self.P[self.ln(l) + ".bias"] if self.layer_norm else None
            dz, dg, db, _ = ln_act_bwd(d, z, gamma, beta, keep, self.dropout[l])
            if self.layer_norm:
                G[self.ln(l) + ".weight"], G[self.ln(l) + ".bias"] = dg, db
            G[self.lin(l) + ".weight"], G[self.lin(l) + ".bias"] = dz.T @ a, dz.sum(axis=0)
            d = dz @ self.P[self.lin(l) + ".weight"]
        return r["loss"], G, logits

    def train_step(self, x, labels, w, keeps, lr=1e-3, wd=1e-4):
        loss, G, _ = self.gradients(x, labels, w, keeps)
        self.t += 1
        for k in self.P:
            self.P[k], self.m[k], self.v[k] = adam_step(self.P[k], G[k], self.m[k], self.v[k], self.t, lr, wd)
        return loss, G
