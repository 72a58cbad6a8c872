"""tests/downstream_ref.py (float64 numpy) against stock torch on the CPU in float64 -- nn.LayerNorm, F.cross_entropy(weight=...),
torch.optim.Adam(weight_decay=...) and autograd through an nn.Sequential built here -- and the host arithmetic of mmvae.downstream
(classification_report, stratified_kfold, the scheduler and the stopping rule) against sklearn and torch."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import downstream_ref as R
from mmvae import downstream

EPS64 = 2.0 ** -52


def close(got, want, ulps, scale=None):
    """|got - want| <= ulps float64 ulps of `scale` (default: the largest |want|)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    s = np.abs(want).max() if scale is None else scale
    return np.abs(got - want).max() <= ulps * EPS64 * max(s, 1e-300)


def sequential(input_dim, C, hidden, layer_norm, dropout):
    mods, k = [], input_dim
    for h, p in zip(hidden, dropout):
        mods.append(nn.Linear(k, h))
        if layer_norm:
            mods.append(nn.LayerNorm(h))
        mods += [nn.ReLU(), nn.Dropout(p)]
        k = h
    mods.append(nn.Linear(k, C))

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Sequential(*mods)

        def forward(self, x):
            return self.fc(x)
    return M().double()


@pytest.mark.parametrize("M,N", [(1, 128), (33, 256), (5, 72)])
def test_layer_norm_forward_and_backward_equal_torch(M, N):
    g = np.random.default_rng(M * N)
    z, gamma, beta = 3 + 2 * g.standard_normal((M, N)), 1 + 0.3 * g.standard_normal(N), 0.2 * g.standard_normal(N)
    keep, p, dy = (g.random((M, N)) > 0.3).astype(np.float64), 0.3, g.standard_normal((M, N))
    y, mean, rstd, _, _ = R.ln_act_fwd(z, gamma, beta, keep, p)
    zt, gt, bt = (torch.tensor(a, requires_grad=True) for a in (z, gamma, beta))
    yt = F.relu(F.layer_norm(zt, (N,), gt, bt, 1e-5)) * torch.tensor(keep) / (1 - p)
    yt.backward(torch.tensor(dy))
    assert close(y, yt.detach().numpy(), 16)
    assert close(mean, z.mean(axis=1), 4) and close(rstd, 1 / np.sqrt(z.var(axis=1) + 1e-5), 4)
    dz, dg, db, _ = R.ln_act_bwd(dy, z, gamma, beta, keep, p)
    # a term of dz is bounded by rstd |g gamma|: the three terms cancel, the ulps are those of the terms
    assert close(dz, zt.grad.numpy(), 64, scale=(rstd[:, None] * np.abs(dy / (1 - p) * gamma)).max())
    assert close(dg, gt.grad.numpy(), 64, scale=np.abs(dy / (1 - p)).sum(axis=0).max() * 4)
    assert close(db, bt.grad.numpy(), 64, scale=np.abs(dy / (1 - p)).sum(axis=0).max())
    # the form without LayerNorm
    y2 = R.ln_act_fwd(z - 3, None, None, keep, p)[0]
    assert close(y2, np.maximum(z - 3, 0) * keep / (1 - p), 4)
    assert close(R.ln_act_bwd(dy, z - 3, None, None, keep, p)[0], dy * keep / (1 - p) * (z - 3 > 0), 4)


@pytest.mark.parametrize("C", [2, 7, 24, 64])
def test_weighted_cross_entropy_equals_torch(C):
    g = np.random.default_rng(C)
    M = 33
    x, y, w = 4 * g.standard_normal((M, C)), g.integers(0, C, M), 0.2 + g.random(C)
    x[3, :] = x[3, 0]                                              # a row of ties: the first maximum
    x[5, C - 1] = x[5, 0] = x[5].max() + 1
    for weights in (w, None):
        r = R.wce_mean(x, y, weights)
        xt = torch.tensor(x, requires_grad=True)
        loss = F.cross_entropy(xt, torch.tensor(y), weight=None if weights is None else torch.tensor(weights))
        loss.backward()
        assert close(r["loss"], loss.item(), 32)
        assert close(r["g"], xt.grad.numpy(), 32, scale=np.abs(xt.grad.numpy()).max())
        assert np.array_equal(r["pred"], torch.max(torch.tensor(x), 1)[1].numpy())
        assert r["pred"][3] == 0 and r["pred"][5] == 0
        assert close(r["nll"], F.cross_entropy(torch.tensor(x), torch.tensor(y), reduction="none").numpy(), 32)
        assert r["confusion"].sum() == M and all(r["confusion"][a, b] == ((y == a) & (r["pred"] == b)).sum() for a in range(C) for b in range(C))


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_adam_equals_torch(wd):
    g = np.random.default_rng(5)
    p = g.standard_normal(257)
    pt = torch.tensor(p, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=1e-3, weight_decay=wd)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in range(1, 6):
        grad = g.standard_normal(257) * 10.0 ** g.integers(-6, 1, 257)
        pt.grad = torch.tensor(grad)
        opt.step()
        p, m, v = R.adam_step(p, grad, m, v, t, 1e-3, wd)
        assert close(p, pt.detach().numpy(), 8)
        assert close(m, opt.state[pt]["exp_avg"].numpy(), 8) and close(v, opt.state[pt]["exp_avg_sq"].numpy(), 8)
    if wd:
        assert not close(R.adamw_step(p, grad, m, v, 6, 1e-3, 0.1)[0], R.adam_step(p, grad, m, v, 6, 1e-3, 0.1)[0], 1e6)


@pytest.mark.parametrize("hidden,layer_norm,dropout", [((256, 128), True, (0.3, 0.2)), ((128,), False, (0.2,)), ((72, 36), True, (0.5, 0.0))])
def test_whole_training_steps_equal_autograd_and_adam(hidden, layer_norm, dropout):
    torch.manual_seed(3)
    g = np.random.default_rng(11)
    D, C, B = 40, 6, 32
    model = sequential(D, C, hidden, layer_norm, dropout)
    with torch.no_grad():
        for prm in model.parameters():                             # LayerNorm's ones and zeros would hide a swapped gamma / beta
            prm.add_(0.1 * torch.randn_like(prm))
    net = R.Net({k: v.detach().numpy() for k, v in model.state_dict().items()}, hidden, layer_norm, dropout)
    assert set(net.P) == set(model.state_dict())
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    w = 0.5 + g.random(C)
    for step in range(3):
        x, y = g.standard_normal((B, D)), g.integers(0, C, B)
        keeps = [(g.random((B, h)) >= p).astype(np.float64) for h, p in zip(hidden, dropout)]
        # stock torch with the same masks: the Dropout modules are switched off and the masks applied behind the ReLUs
        model.eval()
        a, ki = torch.tensor(x), 0
        for mod in model.fc:
            if isinstance(mod, nn.Dropout):
                a = a * torch.tensor(keeps[ki]) / (1 - dropout[ki])
                ki += 1
            else:
                a = mod(a)
        loss = F.cross_entropy(a, torch.tensor(y), weight=torch.tensor(w))
        opt.zero_grad()
        loss.backward()
        got_loss, G = net.train_step(x, y, w, keeps)
        assert close(got_loss, loss.item(), 64)
        for k, prm in model.named_parameters():
            assert close(G[k], prm.grad.numpy(), 512, scale=max(np.abs(prm.grad.numpy()).max(), 1e-3)), (step, k)
        opt.step()
        for k, prm in model.named_parameters():
            assert np.abs(net.P[k] - prm.detach().numpy()).max() <= 1e-11, (step, k)
    # eval mode
    xe = g.standard_normal((7, D))
    assert close(net.forward(xe)[0], model.eval()(torch.tensor(xe)).detach().numpy(), 64)


def test_classification_report_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    g = np.random.default_rng(2)
    for trial in range(12):
        C = int(g.integers(2, 9))
        cm = g.integers(0, 6, (C, C))
        if trial % 3 == 0:
            cm[int(g.integers(0, C)), :] = 0                       # a class without rows
        if trial % 4 == 0:
            cm[:, int(g.integers(0, C))] = 0                       # a class never predicted
        if cm.sum() == 0:
            cm[0, 0] = 1
        yt, yp = [], []
        for a in range(C):
            for b in range(C):
                yt += [a] * int(cm[a, b]); yp += [b] * int(cm[a, b])
        names = [f"site{c}" for c in range(C)]
        want = metrics.classification_report(yt, yp, target_names=names, labels=np.arange(C), output_dict=True, zero_division=0)
        got = downstream.classification_report(cm, names)
        if "accuracy" not in want:                                 # sklearn names it "micro avg" when a label has no row or prediction
            want["accuracy"] = metrics.accuracy_score(yt, yp)
            want.pop("micro avg", None)
        assert set(got) == set(want), trial
        for k, v in want.items():
            if isinstance(v, dict):
                for kk, vv in v.items():
                    assert abs(got[k][kk] - vv) <= 1e-12, (trial, k, kk)
            else:
                assert abs(got[k] - v) <= 1e-12, (trial, k)
    with pytest.raises(ValueError):
        downstream.classification_report(np.zeros((3, 3)), ["a", "b"])


def test_stratified_kfold_has_sklearns_fold_sizes_per_class():
    ms = pytest.importorskip("sklearn.model_selection")
    g = np.random.default_rng(8)
    for sizes, k in (((300, 150, 90, 40, 17, 3), 5), ((7, 7, 2), 2), ((11, 5, 5, 5), 3), ((2, 2, 2, 2), 2)):
        y = g.permutation(np.repeat(np.arange(len(sizes)) * 3 + 1, sizes))          # labels need not be 0 .. C-1
        folds = downstream.stratified_kfold(y, k, seed=42)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = list(ms.StratifiedKFold(n_splits=k, shuffle=True, random_state=42).split(np.zeros((y.size, 1)), y))
        assert len(folds) == k
        seen = np.zeros(y.size, int)
        for (tr, te), (_, wte) in zip(folds, want):
            assert np.array_equal(np.bincount(y[te], minlength=20), np.bincount(y[wte], minlength=20))
            assert np.array_equal(np.sort(np.concatenate([tr, te])), np.arange(y.size))
            seen[te] += 1
        assert (seen == 1).all()
        again = downstream.stratified_kfold(y, k, seed=42)
        assert all(np.array_equal(a[1], b[1]) for a, b in zip(folds, again))
        other = downstream.stratified_kfold(y, k, seed=43)
        assert sum(sizes) < 10 or any(not np.array_equal(a[1], b[1]) for a, b in zip(folds, other))
    with pytest.raises(ValueError):
        downstream.stratified_kfold(np.zeros(4, int), 5, 0)


def test_plateau_scheduler_equals_torchs_and_early_stopping_follows_the_reference():
    g = np.random.default_rng(1)
    seq = list(np.concatenate([np.linspace(2, 1, 8), 1 + 0.01 * g.random(30), [0.5], 0.5 + 0.01 * g.random(10)]))
    prm = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([prm], lr=1e-3)
    ts = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=5)
    mine = downstream.ReduceLROnPlateau(1e-3, 0.5, 5)
    lrs = []
    for v in seq:
        ts.step(v)
        lrs.append(mine.step(v))
        assert lrs[-1] == opt.param_groups[0]["lr"]
    assert lrs[0] == 1e-3 and lrs[-1] < 1e-3 / 8 + 1e-12                 # it acted, several times
    stop = downstream.EarlyStopping(10)
    acc = [50, 60, 60, 59] + [60] * 9
    out = [stop.step(a, i) for i, a in enumerate(acc)]
    assert out[1] == (True, False) and out[2] == (False, False)          # an equal accuracy is no improvement
    assert [o[1] for o in out] == [False] * 11 + [True, True] and stop.best_epoch == 1 and stop.best == 60
