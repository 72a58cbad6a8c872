"""Training steps of mmvae.downstream.SiteClassifier on the MI355X against the float64 restatement (tests/downstream_ref.py) on the fixed
batches of tests/golden/downstream.npz (tools/make_downstream_fixture.py), the hipGraph replay against the eager step, and the
state_dict against an nn.Sequential built here."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import downstream_bounds as DB
import downstream_ref as R
from elementwise_bounds import SECOND, U
from mmvae import downstream

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "downstream.npz")
HIDDEN, DROPOUT = (256, 128), (0.3, 0.2)
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    state = {k[len("step_state_"):]: z[k] for k in z.files if k.startswith("step_state_")}
    return dict(state=state, x=z["step_x"], y=z["step_y"], w=z["step_w"], keeps=[z["step_keep0"], z["step_keep1"]],
                loss64=z["step_loss_fp64"], err32=float(z["step_loss_err_fp32"]))


def classifier(gold, **kw):
    net = downstream.SiteClassifier(40, 6, HIDDEN, True, DROPOUT, seed=1, device=DEV, **kw)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in gold["state"].items()})
    return net


def gemm_tol(a, b):
    """|a| @ |b| sums K products of fp32 values on the exact-fp32 MFMA path: K roundings of the running sum, one per product"""
    K = a.shape[1]
    return SECOND * 2 * K * U * (np.abs(a) @ np.abs(b))


def test_five_steps_against_the_float64_restatement(gold):
    net = classifier(gold)
    ref = R.Net(gold["state"], HIDDEN, True, DROPOUT)
    w = gold["w"]
    losses = []
    for s in range(5):
        x, y = gold["x"][s], gold["y"][s]
        keeps = [k[s] for k in gold["keeps"]]
        before = net.loss_sums.clone()
        buf = net.train_step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(w),
                             masks=[torch.from_numpy(k).to(DEV) for k in keeps])
        d = (net.loss_sums - before).cpu().numpy()
        losses.append(d[0] / d[1])
        if s == 0:
            # first-step gradients per element.  The head's: g^T y2 and column sums of g, from operands inside their own bounds -- the
            # logits' error enters g through the softmax (|dg| <= 2 |dlogit|_max per unit of weight share), y2's through the product.
            loss64, G, logits64 = ref.gradients(x, y, w, keeps)
            r = R.wce_mean(logits64, y, w)
            got_logits = buf.logits.cpu().numpy().astype(np.float64)
            a2 = ref.forward(x, keeps)[1][2][0]                       # the head's input in float64
            # forward error budget of the logits: three fp32 GEMMs (K = 40, 256, 128) and two LayerNorms whose outputs are O(1);
            # each stage's relative error is below (2 K + 40) U of its terms and is carried with gain <= 4 through a LayerNorm with
            # |gamma| <= 1.5 and rstd <= 4 -- a budget of 2^-13 of the logits' magnitude terms, not fitted
            dl = 2.0 ** -13 * (np.abs(a2) @ np.abs(ref.P["fc.8.weight"]).T + np.abs(ref.P["fc.8.bias"]))
            assert (np.abs(got_logits - logits64) <= dl).all()
            wy = w.astype(np.float64)[y]
            dg = DB.wce_tol(logits64, y, w)[2] + 2 * dl.max() * wy[:, None] / wy.sum()
            got_g = buf.g.cpu().numpy().astype(np.float64)
            assert (np.abs(got_g - r["g"]) <= dg).all()
            got_dw = net.grads["fc.8.weight"].cpu().numpy().astype(np.float64)
            tol_dw = gemm_tol(r["g"].T, a2) + dg.T @ np.abs(a2) + np.abs(r["g"]).T @ (2.0 ** -13 * np.abs(a2) + 1e-6)
            assert (np.abs(got_dw - G["fc.8.weight"]) <= tol_dw).all()
            got_db = net.grads["fc.8.bias"].cpu().numpy().astype(np.float64)
            assert (np.abs(got_db - G["fc.8.bias"]) <= 32 * U * np.abs(r["g"]).sum(axis=0) + dg.sum(axis=0)).all()
            # every other tensor: within 2^-11 of the tensor's largest gradient (the same budget carried back through two more layers)
            for k, want in G.items():
                got = net.grads[k].cpu().numpy().astype(np.float64)
                assert np.abs(got - want).max() <= 2.0 ** -11 * np.abs(want).max(), k
        want_loss, _ = ref.train_step(x, y, w, keeps)
        assert abs(gold["loss64"][s] - want_loss) <= 1e-9, "the restatement is the fixture's float64 torch run"
    # stock torch in float32 on the CPU strays from float64 by err32 over these five steps; 8x that is allowed here: another summation
    # order than the CPU BLAS, and Adam's m / sqrt(v) amplifying the rounding of near-zero gradients
    err = np.abs(np.array(losses) - gold["loss64"]).max()
    print(f"max |loss - loss_fp64| over five steps: device {err:.3e}, stock torch fp32 on the CPU {gold['err32']:.3e}")
    assert err <= 8 * gold["err32"]
    for k, v in ref.P.items():                                     # five updates of at most lr each
        assert np.abs(net.params[k].cpu().numpy() - v).max() <= 5e-3 * 2.0 ** -6, k


def test_graph_replay_and_eager_give_identical_parameters(gold):
    g = np.random.default_rng(3)
    X = torch.from_numpy(g.standard_normal((96, 40)).astype(np.float32)).to(DEV)
    y = torch.from_numpy(g.integers(0, 6, 96)).to(DEV)
    out = []
    for graph in (True, False):
        net = classifier(gold)
        net.set_data(X, y, torch.from_numpy(gold["w"]), graph=graph)
        net.train_epoch(torch.Generator().manual_seed(5))           # three full batches: the same shuffle, the same Philox stream
        assert (net._graph is not None) == graph
        torch.cuda.synchronize()
        assert int(net._step[0]) == 3 and bool((net._step == 3).all())
        out.append((net.state_dict(), net.loss_sums.clone()))
    for k in out[0][0]:
        assert torch.equal(out[0][0][k], out[1][0][k]), k
        assert not torch.equal(out[0][0][k], torch.from_numpy(gold["state"][k]).to(DEV)), k
    assert out[0][1][1] == out[1][1][1] and abs(float(out[0][1][0] - out[1][1][0])) <= 1e-9 * float(out[0][1][0])


def test_the_last_shorter_batch_is_not_dropped(gold):
    g = np.random.default_rng(4)
    X = torch.from_numpy(g.standard_normal((70, 40)).astype(np.float32)).to(DEV)
    y = torch.from_numpy(g.integers(0, 6, 70)).to(DEV)
    net = classifier(gold)
    net.set_data(X, y, None)
    net.train_epoch()
    torch.cuda.synchronize()
    assert int(net._step[0]) == 3 and net.loss_sums[1].item() == 70                    # 32 + 32 + 6 rows, weight 1 each
    with pytest.raises(ValueError):
        net.set_data(X, y + 1, None)                                                   # a label outside [0, 6)


def test_state_dict_round_trips_into_a_sequential(gold):
    net = classifier(gold)
    seq = nn.Sequential(nn.Linear(40, 256), nn.LayerNorm(256), nn.ReLU(), nn.Dropout(0.3), nn.Linear(256, 128), nn.LayerNorm(128), nn.ReLU(),
                        nn.Dropout(0.2), nn.Linear(128, 6))

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = seq
    model = M()
    model.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})           # strict: the keys are the Sequential's
    x = torch.from_numpy(gold["x"].reshape(-1, 40))
    want = model.eval().double().fc(x.double()).detach().numpy()
    got = net.eval().logits(x.to(DEV)).cpu().numpy()
    assert np.abs(got - want).max() <= 2.0 ** -13 * max(np.abs(want).max(), 1.0)
    # and back: a freshly initialised classifier takes the Sequential's parameters
    other = downstream.SiteClassifier(40, 6, HIDDEN, True, DROPOUT, seed=9, device=DEV)
    assert not torch.equal(other.params["fc.0.weight"], net.params["fc.0.weight"])
    other.load_state_dict(model.float().state_dict())
    assert torch.equal(other.eval().logits(x.to(DEV)), net.logits(x.to(DEV)))
    # nn.Linear's and nn.LayerNorm's initialisation
    w0 = other.__class__(40, 6, HIDDEN, True, DROPOUT, seed=9, device=DEV).params
    assert w0["fc.0.weight"].abs().max() <= 1 / np.sqrt(40) and w0["fc.0.weight"].abs().max() > 0.9 / np.sqrt(40)
    assert w0["fc.4.bias"].abs().max() <= 1 / 16 and (w0["fc.1.weight"] == 1).all() and (w0["fc.5.bias"] == 0).all()
    # the directional script's model: no LayerNorm, keys fc.0 and fc.3
    small = downstream.SiteClassifier(40, 6, (128,), False, (0.2,), seed=1, device=DEV)
    assert sorted(small.state_dict()) == ["fc.0.bias", "fc.0.weight", "fc.3.bias", "fc.3.weight"]
    buf = small.train_step(x[:32].to(DEV), torch.from_numpy(gold["y"][0]).to(DEV))
    ref = R.Net({k: v.cpu().numpy() for k, v in downstream.SiteClassifier(40, 6, (128,), False, (0.2,), seed=1, device=DEV).state_dict().items()},
                (128,), False, (0.2,))
    _, G, _ = ref.gradients(x[:32].numpy(), gold["y"][0], None, [buf.masks[0].cpu().numpy()])
    for k, want in G.items():
        assert np.abs(small.grads[k].cpu().numpy() - want).max() <= 2.0 ** -11 * np.abs(want).max(), k


def test_an_input_width_that_is_no_multiple_of_four(gold):
    """the training batch lives in rows padded to 4 columns: the gradients must not know"""
    g = np.random.default_rng(6)
    D = 42
    x, y = g.standard_normal((32, D)).astype(np.float32), gold["y"][1]
    net = downstream.SiteClassifier(D, 6, HIDDEN, True, DROPOUT, seed=2, device=DEV)
    ref = R.Net({k: v.cpu().numpy() for k, v in net.state_dict().items()}, HIDDEN, True, DROPOUT)
    X = torch.from_numpy(x).to(DEV)
    net.set_data(X, torch.from_numpy(y).to(DEV), torch.from_numpy(gold["w"]), graph=False)
    buf = net._train_buffers(32)
    buf.idx.copy_(torch.arange(32, device=DEV))
    net._batch_launches(buf, 32)                                   # gather into the padded rows, then the step
    assert torch.equal(buf.x, X) and (buf.x_pad[:, D:] == 0).all()
    _, G, logits = ref.gradients(x, y, gold["w"], [m.cpu().numpy() for m in buf.masks])
    assert np.abs(buf.logits.cpu().numpy() - logits).max() <= 2.0 ** -13 * max(np.abs(logits).max(), 1.0)
    for k, want in G.items():
        assert np.abs(net.grads[k].cpu().numpy() - want).max() <= 2.0 ** -11 * np.abs(want).max(), k
