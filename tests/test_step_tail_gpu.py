"""The riders of the grouped dW launch (mmvae_gemm_tn_group_riders, csrc/gemm_tn.hip) against the three launches they replace --
mmvae_gemm_tn_group + mmvae_embed_table_bwd + mmvae_loss_finalize -- on the same inputs, and the engine's use of them and of the
merged head-of-step launch (mmvae_step_head) in the captured training step.

  kernel   M = 256, one batch split per problem; a heads problem (N = 40, K = 128, BatchNorm + ReLU + Dropout prologue with a
           mask) and a class problem (N = 24, K = 64, fp32 P); EncoderC backward at (S, E, L) = (24, 32, 20), 8 table copies;
           beta / gamma by value and from the device pair.  Bitwise (torch.equal): dW and db of both problems, EncoderC's five gradients, out5.  Each
           stand-alone form is first run twice: only where it reproduces itself bit for bit is the rider form held to its bits;
           otherwise to the derived bound that form is already held to (gemm_bounds.dw_order_tol, elementwise_bounds).
  LDS      the rider's LDS image lives in the group launch's dynamic LDS (72 KiB) and takes no more than the stand-alone launch
           does (64 KiB).  (24, 32, 128) needs 59 KiB and rides; (40, 32, 128) needs 77 KiB: refused, nothing enqueued.
  key 14   off: refused, nothing enqueued.
  engine   one eager step of the captured work at B = 256: tags with keys 13 / 14 on and off, same losses and gradients; after the
           parameters are overwritten in place between two replays the prepared operands are those of the new values.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import elementwise_bounds as E  # noqa: E402
import gemm_bounds as G  # noqa: E402
from mmvae import _lib as L  # noqa: E402
from mmvae import engine, ops  # noqa: E402
from mmvae.ops import PREC_BF16, PREC_F32  # noqa: E402
from test_elementwise_gpu import DEV, ERR_ARG, _embed_params, dev, host, inside, rnd, snapshot, stream, unchanged  # noqa: E402
from test_gemm_folded_gpu import GroupProblem, group_call  # noqa: E402

M = 256
FILL = -777.0
_PROBLEMS = {}


def _problems(prec):
    if prec not in _PROBLEMS:
        _PROBLEMS[prec] = [GroupProblem(prec, 0, M, 40, 128, masked=True), GroupProblem(prec, 2, M, 24, 64)]
    return _PROBLEMS[prec]


class Tail:
    """Inputs of the two riders; run() makes fresh destinations every time, so every form starts from the same state."""

    def __init__(self, prec, S, Ed, Ld, copies=8, seed=1):
        rng = np.random.default_rng(seed + S + Ld)
        self.prec, self.S, self.Ed, self.Ld = prec, S, Ed, Ld
        self.emb, self.wm, _, self.wl, _ = _embed_params(rng, S, Ed, Ld)
        self.dT = [rnd(rng, S, 2 * Ld) for _ in range(copies)]
        self.old = (rnd(rng, S, Ed), rnd(rng, 2 * Ld, Ed), rnd(rng, 2 * Ld))       # the gradients are accumulated into
        self.sums = np.array([1234.5678, 987.125, 3.25, 41.0625, 2.0]) * np.array([1e3, 1e2, 1.0, 1.0, 1.0])
        self.beta, self.gamma = 1e-3, 0.7
        self.t_emb, self.t_wm, self.t_wl, self.t_dT = dev(self.emb), dev(self.wm), dev(self.wl), dev(np.stack(self.dT))
        self.t_sums = dev(self.sums)
        self.pair = dev(np.array([self.beta, self.gamma], np.float32))

    def fresh(self):
        Ld = self.Ld
        o = dict(arenas=[pr.outputs() for pr in _problems(self.prec)],
                 d_emb=dev(self.old[0]), d_wm=dev(self.old[1][:Ld]), d_wl=dev(self.old[1][Ld:]), d_bm=dev(self.old[2][:Ld]), d_bl=dev(self.old[2][Ld:]),
                 out5=torch.full((5 + 3,), FILL, device=DEV))
        return o

    def embed_args(self, o):
        return (self.t_emb, self.t_wm, self.t_wl, self.t_dT, o["d_emb"], o["d_wm"], o["d_bm"], o["d_wl"], o["d_bl"])

    def loss_args(self, o, on_device):
        # on the device: the by-value pair must be ignored
        return (self.t_sums, 123.0 if on_device else self.beta, -5.0 if on_device else self.gamma, o["out5"], self.pair if on_device else None)

    def group_args(self, o):
        """The problems' argument records with ONE batch split each: with more (fp32 mode takes two at M = 256) db is added to by
        fp32 atomics from several workgroups and even the stand-alone launch does not reproduce itself bit for bit."""
        out = []
        for pr, a in zip(_problems(self.prec), o["arenas"]):
            g = pr.args(a)
            g.nsplit = 1
            out.append(g)
        return out

    def alone(self, on_device=False):
        o = self.fresh()
        assert group_call(self.group_args(o), o["arenas"]) == 0
        ops.embed_table_bwd(*self.embed_args(o))
        ops.loss_finalize(*self.loss_args(o, on_device))
        torch.cuda.synchronize()
        return o

    def riders(self, on_device=False, embed=True, loss=True, o=None):
        """-> (status, destinations)."""
        o = o or self.fresh()
        r = ops.tn_riders(self.embed_args(o) if embed else None, self.loss_args(o, on_device) if loss else None)
        gs = self.group_args(o)
        arr = (L.GemmTnArgs * len(gs))(*gs)
        status = L.load().mmvae_gemm_tn_group_riders(C.cast(arr, C.c_void_p), len(gs), C.byref(r), stream())
        torch.cuda.synchronize()
        return status, o


def _tensors(o):
    out = {k: v for k, v in o.items() if k != "arenas"}
    for i, a in enumerate(o["arenas"]):
        out[f"arena{i}"] = a.buf
    return out


def _held_to(t, got, ref, ref_again, what):
    """Bit for bit where the stand-alone form reproduces itself; else each tensor within the bound that form is held to."""
    tg, tr, ta = _tensors(got), _tensors(ref), _tensors(ref_again)
    Ld = t.Ld
    for name in tr:
        if torch.equal(tr[name], ta[name]):
            assert torch.equal(tg[name], tr[name]), f"{what}: {name} differs from the stand-alone launches"
            continue
        print(f"{what}: {name} is not bit-reproducible in the stand-alone form: held to its derived bound")
        if name.startswith("arena"):
            i = int(name[5:])
            pr = _problems(t.prec)[i]
            ow, ob = G.dw_order_tol(pr.p_host, pr.q_host, pr.old_dw, pr.old_db)
            inside(host(got["arenas"][i].views[0]), host(ref["arenas"][i].views[0]), ow, f"{what} dW{i}")
            inside(host(got["arenas"][i].views[1]), host(ref["arenas"][i].views[1]), ob, f"{what} db{i}")
        elif name == "out5":
            inside(host(tg[name][:5]), E.loss_finalize(t.sums, t.beta, t.gamma, np.float64), E.loss_finalize_tol(t.sums, t.beta, t.gamma), what + " out5")
        else:
            refs, tol = E.embed_bwd(t.dT, t.emb, t.wm, t.wl, t.old, np.float64), E.embed_bwd_tol(t.dT, t.emb, t.wm, t.wl, t.old)
            k, sl = {"d_emb": (0, slice(None)), "d_wm": (1, slice(0, Ld)), "d_wl": (1, slice(Ld, None)), "d_bm": (2, slice(0, Ld)), "d_bl": (2, slice(Ld, None))}[name]
            inside(host(tg[name]), refs[k][sl], np.broadcast_to(tol[k], refs[k].shape)[sl], f"{what} {name}")


def _written(t, o, what):
    """Every destination moved, by about what it should (the comparison is not between untouched buffers), and guards are intact."""
    assert (o["out5"][5:] == FILL).all() and (o["out5"][:5] != FILL).all(), what
    inside(host(o["out5"][:5]), E.loss_finalize(t.sums, t.beta, t.gamma, np.float64), E.loss_finalize_tol(t.sums, t.beta, t.gamma), what + " out5")
    refs, tol = E.embed_bwd(t.dT, t.emb, t.wm, t.wl, t.old, np.float64), E.embed_bwd_tol(t.dT, t.emb, t.wm, t.wl, t.old)
    inside(host(o["d_emb"]), refs[0], tol[0], what + " d_emb")
    inside(np.concatenate([host(o["d_wm"]), host(o["d_wl"])]), refs[1], tol[1], what + " d_W")
    inside(np.concatenate([host(o["d_bm"]), host(o["d_bl"])]), refs[2], tol[2], what + " d_b")
    for i, (pr, a) in enumerate(zip(_problems(t.prec), o["arenas"])):
        pr.check(a, f"{what} problem {i}")


@pytest.mark.parametrize("on_device", [False, True], ids=["by value", "device pair"])
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_F32], ids=["bf16", "fp32"])
def test_riders_equal_the_three_launches(prec, on_device):
    t = Tail(prec, 24, 32, 20)
    ref, ref_again = t.alone(on_device), t.alone(on_device)
    status, got = t.riders(on_device)
    assert status == 0
    what = f"riders {'bf16' if prec == PREC_BF16 else 'fp32'}"
    _written(t, got, what)
    _held_to(t, got, ref, ref_again, what)


@pytest.mark.parametrize("embed,loss", [(True, False), (False, True)], ids=["EncoderC alone", "loss alone"])
def test_one_rider_alone(embed, loss):
    t = Tail(PREC_BF16, 24, 32, 20)
    ref, ref_again = t.alone(), t.alone()
    untouched = t.fresh()
    status, got = t.riders(embed=embed, loss=loss)
    assert status == 0
    absent = ["out5"] if embed else ["d_emb", "d_wm", "d_wl", "d_bm", "d_bl"]
    for name in absent:                                   # the rider that was not named wrote nothing
        assert torch.equal(got[name], untouched[name]), name
        ref[name] = ref_again[name] = got[name]
    _held_to(t, got, ref, ref_again, "one rider")


def test_rider_at_59_kib_of_lds_rides_and_at_77_kib_is_refused():
    lds = lambda S, Ed, Ld: (S * 2 * Ld + S * Ed + 2 * Ld * Ed) * 4
    group_lds = 4 * 64 * 256 + 8192                       # gemm_tn_group_kernel's dynamic LDS
    assert lds(24, 32, 128) <= 64 * 1024 < group_lds < lds(40, 32, 128)
    t = Tail(PREC_BF16, 24, 32, 128)
    ref, ref_again = t.alone(), t.alone()
    status, got = t.riders()
    assert status == 0
    _held_to(t, got, ref, ref_again, "riders L = 128")

    t = Tail(PREC_BF16, 40, 32, 128)
    o = t.fresh()
    before = {k: snapshot(v) for k, v in _tensors(o).items()}
    status, o = t.riders(o=o)
    assert status == ERR_ARG
    assert all(unchanged(v, before[k]) for k, v in _tensors(o).items()), "a refused call wrote something"
    # the group without riders takes the same problems: the caller's fallback
    assert group_call(_problems(PREC_BF16), o["arenas"]) == 0
    torch.cuda.synchronize()
    for i, (pr, a) in enumerate(zip(_problems(PREC_BF16), o["arenas"])):
        pr.check(a, f"fallback problem {i}")


def test_key_14_off_refuses_with_nothing_enqueued():
    t = Tail(PREC_BF16, 24, 32, 20)
    o = t.fresh()
    before = {k: snapshot(v) for k, v in _tensors(o).items()}
    try:
        assert L.load().mmvae_set_tuning(14, 0) == 0
        status, o = t.riders(o=o)
        assert status == ERR_ARG
    finally:
        assert L.load().mmvae_set_tuning(14, 1) == 0
    assert all(unchanged(v, before[k]) for k, v in _tensors(o).items()), "a refused call wrote something"
    status, o = t.riders(o=o)                             # the key is back on
    assert status == 0
    _written(t, o, "after key 14")


# ----------------------------------------------------------------------------------------------------------------------------------
# the captured training step through the engine
# ----------------------------------------------------------------------------------------------------------------------------------
B, A_DIM, D_DIM, S, LAT = 256, 782, 572, 24, 20
ATOMIC = ("encoder_c.",)              # behind mmvae_fuse_reparam_bwd's unordered fp32 atomics: see tests/test_class_tail_gpu.py


def _set_keys(on):
    for key in (13, 14):
        L.check(L.load().mmvae_set_tuning(key, int(on)), "mmvae_set_tuning")


def _batch():
    g = torch.Generator().manual_seed(5)
    a = torch.randn(B, A_DIM, generator=g).to(DEV)
    b = (torch.rand(B, D_DIM, generator=g) < 0.3).float().to(DEV)
    site = torch.randint(0, S, (B,), generator=g).to(DEV)
    return a, b, site


def _graphed(a, b, site):
    from mmvae.graphs import GraphedTrainStep
    from mmvae.optim import FusedAdamW
    from src.models import MultiModalVAE
    torch.manual_seed(321)
    m = MultiModalVAE(A_DIM, D_DIM, S, LAT).to(DEV).train()
    engine.GLOBAL_NOISE.offset_tensor(torch.device(DEV, torch.cuda.current_device())).zero_()
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    return m, GraphedTrainStep(m, opt, a, b, site, warmup=1, preserve_state=True)


def test_eager_step_takes_the_merged_launches_and_equals_the_step_without_them():
    a, b, site = _batch()
    res = []
    for on in (False, False, True):
        _set_keys(on)
        try:
            m, gs = _graphed(a, b, site)
            ops.PROBE = ops.KernelProbe()
            try:
                out5 = gs.run_eager().cpu().numpy()
                torch.cuda.synchronize()
                tags = set(ops.PROBE.records)
            finally:
                ops.PROBE = None
            res.append((out5, {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}, tags))
        finally:
            _set_keys(True)
    (l0, g0, tags0), (_, g0b, _), (l1, g1, tags1) = res
    assert "step_head" in tags1 and not ({"noise", "prep_weights"} & tags1), sorted(tags1)
    assert "step_head" not in tags0 and {"noise", "prep_weights"} <= tags0, sorted(tags0)
    assert "tiny_dW.heads" in tags0 and "tiny_dW.heads" in tags1
    assert np.array_equal(l0, l1) and np.isfinite(l1).all() and l1[0] > 0, (l0, l1)
    assert len(g0) == 39
    for k in g0:
        if k.startswith(ATOMIC):          # within 4 x what the step without the merged launches differs from itself by, at least an ulp
            floor = max(float(np.abs(g0[k] - g0b[k]).max()), float(np.abs(g0[k]).max()) * 2.0 ** -23)
            assert float(np.abs(g0[k] - g1[k]).max()) <= 4.0 * floor, (k, float(np.abs(g0[k] - g1[k]).max()), floor)
        else:
            assert np.array_equal(g0[k], g1[k]), k


def test_parameters_overwritten_between_replays_are_prepared_afresh():
    """The stale-weights case the head placement exists for: the prepared operands a replay leaves behind are those of the masters
    as they were when it BEGAN (AdamW changes the masters at its end), also when the caller rewrote them in place since the last one."""
    a, b, site = _batch()
    m, gs = _graphed(a, b, site)
    gs()
    torch.cuda.synchronize()
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(100 + i)).to(DEV) * 0.05 + (1.0 if p.dim() == 1 else 0.0))
    began = {id(p): p.detach().clone() for p in m.parameters()}
    gs()
    torch.cuda.synchronize()
    out5 = gs.out4.cpu().numpy()
    assert np.isfinite(out5).all() and out5[4] == 0.0
    g = m._graph()
    prec, linears = g._prep.key[0], g._prep.prep.linears
    assert len(linears) >= 10
    for pl in linears:
        fresh = ops.PreparedLinear([began[id(w)] for w in pl.srcs], [began[id(x)] for x in pl.bias_srcs], prec, torch.device(DEV))
        with ops.pinned_stream():
            ops.WeightPrep([fresh], torch.device(DEV)).run()
        torch.cuda.synchronize()
        assert torch.equal(fresh.w, pl.w) and torch.equal(fresh.wt, pl.wt), (pl.N, pl.K)
        if pl._bias_cat is not None:
            assert torch.equal(fresh.bias, pl.bias)
