"""The three GEMM paths that run on every training step behind an MMVAE_ERR_ARG fallback, each called directly and held against
float64, element by element:

  (a) mmvae_gemm_nt with pro_finalize  -- mmvae_bn_finalize folded into the consumer GEMM (BnFin, csrc/gemm_src.h), on each kernel
      that implements it: the register-staged tile kernel in its 128 x 128 form (bf16 and fp32 mode) and its 128 x 256 form, and
      the wave-specialised persistent kernel (gemm_ntp.h);
  (b) mmvae_gemm_tn with MMVAE_PRO_BN_BWD_APPLY and p_coef == NULL -- mmvae_bn_bwd_finalize folded into the wide-tile dW kernels
      (csrc/gemm_tn_wide.hip), both tile forms;
  (c) mmvae_gemm_tn_group -- up to 8 small dW problems in one launch plus one reduce.

Every folded case asserts that its entry point returned 0 (ops.gemm_nt / ops.gemm_tn raise on anything else, the grouped entry is
called through ctypes): a case that fell back would test nothing.  Every bound is an expression of tests/gemm_bounds.py or
tests/elementwise_bounds.py (derived by counting roundings; tests/test_gemm_bounds_cpu.py shows that they hold and that they bite);
no tolerance here is a literal, and no element is excluded from any comparison.  Which kernel runs is decided by the dispatch
conditions of the entry points; the cases assert those conditions (sizes, alignments, tuning keys), and every mmvae_set_tuning
change is undone in `finally`.  Refusal tests use only arguments the entry points reject before they launch anything.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import elementwise_bounds as E  # noqa: E402
import gemm_bounds as G  # noqa: E402
from mmvae import _lib as L  # noqa: E402
from mmvae import ops  # noqa: E402
from mmvae.ops import PREC_BF16, PREC_F32  # noqa: E402
from test_elementwise_gpu import DEV, ERR_ARG, NAN, _bn_data, bits, dev, host, inside, rnd, snapshot, stream, unchanged  # noqa: E402

F32, F64 = np.float32, np.float64
TUNING_DEFAULTS = {0: 32768, 3: 0, 4: 1, 8: 1, 9: 16384}
SENTINEL = -12345.678


class tuning:
    """mmvae_set_tuning for the span of a `with`, every changed key back at its default afterwards."""

    def __init__(self, **keys):
        self.keys = {int(k[1:]): v for k, v in keys.items()}

    def __enter__(self):
        for k, v in self.keys.items():
            assert L.load().mmvae_set_tuning(k, v) == 0
        return self

    def __exit__(self, *exc):
        for k in self.keys:
            L.load().mmvae_set_tuning(k, TUNING_DEFAULTS[k])
        return False


def status(fn, *a, **k):
    """Return value of the entry point behind an ops wrapper: 0, MMVAE_ERR_ARG (-1) or MMVAE_ERR_DTYPE (-2)."""
    try:
        fn(*a, **k)
        return 0
    except L.MMVAEArgError as e:
        return ERR_ARG if "invalid argument" in str(e) else -2


def guarded(values, pad=3, dtype=torch.float32):
    """Device vector of len(values) + pad elements: the values, then NaN guards."""
    t = torch.full((len(values) + pad,), NAN, dtype=dtype, device=DEV)
    t[:len(values)] = dev(np.asarray(values))
    return t


def to_act(x, prec, ld=None, fill=0.0):
    """Host float array [M][C] -> device matrix of the activation type, as a view of an [M][ld] buffer whose pad columns hold `fill`."""
    dt = ops.act_dtype(prec)
    ld = ld or x.shape[1]
    buf = torch.full((x.shape[0], ld), fill, dtype=dt, device=DEV)
    buf[:, :x.shape[1]] = dev(np.asarray(x, F32)).to(dt)
    return buf[:, :x.shape[1]]


def prep(W, b, prec):
    pl = ops.PreparedLinear([dev(W)], [dev(b)], prec, DEV)
    ops.WeightPrep([pl], DEV).run()
    return pl


class Arena:
    """Gradient views inside one sentinel-filled buffer, as the engine's gradient arena hands them over; guards() are the elements
    outside every view."""

    def __init__(self, shapes, gap=64):
        self.off, total = [], gap
        for s in shapes:
            self.off.append(total)
            total += -(-int(np.prod(s)) // gap) * gap + gap
        self.buf = torch.full((total,), SENTINEL, dtype=torch.float32, device=DEV)
        self.views = [self.buf[o:o + int(np.prod(s))].view(*s) for o, s in zip(self.off, shapes)]
        self.mask = torch.ones(total, dtype=torch.bool, device=DEV)
        for o, s in zip(self.off, shapes):
            self.mask[o:o + int(np.prod(s))] = False
        self.before = snapshot(self.buf[self.mask])

    def guards_unchanged(self):
        return unchanged(self.buf[self.mask], self.before)


# =============================================================================================
# (a) mmvae_gemm_nt with pro_finalize
# =============================================================================================
def _kernel_setup(kernel, prec, M, N, K):
    """Tuning keys that make `kernel` the one that runs, after asserting that the problem is one of its (gemm_nt.hip launch_nt /
    nt_wide_ok, gemm_ntp.hip ntp_dispatch)."""
    if kernel == "tile128":
        return tuning(k8=0, k0=1 << 30)                       # not the wave-specialised kernel, never 128 x 256 tiles
    if kernel == "tile256":
        assert prec == PREC_BF16 and N % 256 == 0
        return tuning(k8=0, k0=1)
    assert kernel == "ntp" and prec == PREC_BF16 and M % 128 == 0 and N % 128 == 0 and 64 < K <= 512 and K % 64 == 0 and M >= 256
    return tuning(k8=1, k9=256)


class ProFinCase:
    """Operands of one consumer GEMM behind the BatchNorm + ReLU + Dropout prologue, and the state mmvae_bn_finalize writes."""

    def __init__(self, prec, M, N, K, masked, running, seed, y=None, stats=None):
        rng = np.random.default_rng(seed)
        self.prec, self.M, self.N, self.K, self.running = prec, M, N, K, running
        bf = prec == PREC_BF16
        x, gamma, beta, rm, rv = _bn_data(rng, M, K)
        self.gamma, self.beta, self.rm, self.rv = gamma, beta, rm, rv
        self.y = to_act(x, prec) if y is None else y                         # [M][K], activation type
        self.y_host = host(self.y)                                            # the values actually stored
        self.s_exact = np.stack([self.y_host.sum(0), (self.y_host ** 2).sum(0)])
        self.stats = dev(self.s_exact) if stats is None else stats
        self.mask_host = (rng.random((M, K)) < 0.9).astype(np.uint8) if masked else None
        self.mask = dev(self.mask_host) if masked else None
        self.inv_keep = 1.0 / 0.9 if masked else 1.0
        W, b = rnd(rng, N, K, scale=K ** -0.5), rnd(rng, N)
        self.pl = prep(W, b, prec)
        self.W_host, self.b_host = host(self.pl.w[:N, :K]), b.astype(F64)     # the prepared (rounded) weights
        self.out_bf16 = bf and N != 40
        self.with_stats = N != 40
        self.ldc = 48 if N == 40 else N
        self.d_gamma, self.d_beta = dev(gamma), dev(beta)

    def state(self):
        K = self.K
        t = {k: torch.full((K + 3,), NAN, device=DEV) for k in ("mean", "rstd", "scale", "shift")}
        t["rm"], t["rv"] = guarded(self.rm), guarded(self.rv)
        t["nbt"] = torch.tensor([41], dtype=torch.int64, device=DEV)
        return t

    def fin_args(self, t, stats=None):
        r = self.running
        return ops.bn_finalize_args(self.M, self.K, self.stats if stats is None else stats, self.d_gamma, self.d_beta, t["rm"] if r else None,
                                    t["rv"] if r else None, t["nbt"] if r else None, t["mean"], t["rstd"], t["scale"], t["shift"])

    def outputs(self):
        c = torch.full((self.M, self.ldc), 7.0, dtype=torch.bfloat16 if self.out_bf16 else torch.float32, device=DEV)
        st = torch.zeros(2, self.N, dtype=torch.float64, device=DEV) if self.with_stats else None
        return c, st

    def gemm(self, t, c, st, fin=None, pro_out=None):
        pro = ops.Prologue(t["scale"], t["shift"], self.mask, self.inv_keep)
        return status(ops.gemm_nt, self.prec, self.y, self.pl.w, self.N, self.K, c[:, :self.N], bias=self.pl.bias, prologue=pro, stats=st,
                      pro_finalize=fin, pro_out=pro_out)


def _check_finalize(case, t, tag, s1, s2, sums_rel=0.0):
    """The vectors mmvae_bn_finalize writes, against float64 from the sums (s1, s2)."""
    K, M = case.K, case.M
    args = (s1, s2, M, case.gamma, case.beta, ops.BN_EPS, ops.BN_MOMENTUM, case.rm if case.running else None, case.rv if case.running else None)
    ref, tol = E.bn_finalize(*args, F64), E.bn_finalize_tol(*args, sums_rel=sums_rel)
    for k in ("mean", "rstd", "scale", "shift"):
        inside(host(t[k][:K]), ref[k], tol[k], f"{tag} {k}")
        assert torch.isnan(t[k][K:]).all(), f"{k}: written past its K elements"
    if not np.ndim(sums_rel):
        # the constant column's variance cancels to about +-1e-10 (exactly 0 for a bf16 constant) and must clamp at 0
        assert host(t["rstd"][:1])[0] <= 1.0 / np.sqrt(float(F32(ops.BN_EPS))) * (1 + 2 * E.U), "constant column: rstd beyond 1 / sqrt(eps)"
    assert torch.isnan(t["rm"][K:]).all() and torch.isnan(t["rv"][K:]).all()
    if not case.running:
        assert unchanged(t["rm"], bits(guarded(case.rm))) and unchanged(t["rv"], bits(guarded(case.rv))) and t["nbt"].item() == 41
        return
    assert t["nbt"].item() == 42, "num_batches_tracked must move by exactly one"
    # exactly ONE momentum step from non-trivial values: a second application moves the result by momentum * (new - old), far outside
    inside(host(t["rm"][:K]), ref["running_mean"], tol["running_mean"], f"{tag} running_mean")
    inside(host(t["rv"][:K]), ref["running_var"], tol["running_var"], f"{tag} running_var")


def _check_product(case, t, c, st, rows, tag):
    """C against the float64 product of the operand rebuilt from the DEVICE's own fp32 tables, with the at-risk allowance; the column
    statistics against the float64 sums of the stored C."""
    K, N = case.K, case.N
    bf = case.prec == PREC_BF16
    h, dh = G.prologue_operand(case.y_host, host(t["scale"][:K]), host(t["shift"][:K]), case.inv_keep, case.mask_host, bf)
    ref = G.nt_ref(h, case.W_host, case.b_host)
    got = host(c[:, :N])
    inside(got, ref, G.nt_tol(h, case.W_host, case.b_host, dh, out_bf16=case.out_bf16, ref=ref), f"{tag} C")
    pad = c[:, N:].float()
    assert torch.all((pad == 7.0) | (pad == 0.0)), "pad columns of C: neither untouched nor zeroed"
    if st is not None:
        inside(host(st), G.stats_ref(got), G.stats_tol(got, rows), f"{tag} statistics")
    return h, dh


PRO_FIN_CASES = [  # kernel, prec, M, N, K, masked, running
    ("tile128", PREC_BF16, 2, 40, 64, True, True), ("tile128", PREC_BF16, 389, 40, 128, False, False),
    ("tile128", PREC_BF16, 4096, 256, 256, True, True), ("tile128", PREC_BF16, 389, 512, 512, True, False),
    ("tile128", PREC_BF16, 65536, 256, 512, False, True),
    ("tile128", PREC_F32, 2, 256, 64, False, True), ("tile128", PREC_F32, 389, 40, 256, True, True),
    ("tile128", PREC_F32, 4096, 256, 512, False, False), ("tile128", PREC_F32, 4096, 40, 128, True, True),
    ("tile128", PREC_F32, 65536, 256, 64, True, True),
    ("tile256", PREC_BF16, 389, 256, 128, True, True), ("tile256", PREC_BF16, 2, 512, 64, False, True),
    ("tile256", PREC_BF16, 4096, 512, 512, False, False), ("tile256", PREC_BF16, 65536, 256, 256, True, True),
    ("ntp", PREC_BF16, 4096, 256, 128, True, True), ("ntp", PREC_BF16, 4096, 512, 256, False, False),
    ("ntp", PREC_BF16, 65536, 256, 512, True, True), ("ntp", PREC_BF16, 65536, 256, 256, False, True),
]


@pytest.mark.parametrize("kernel,prec,M,N,K,masked,running", PRO_FIN_CASES,
                         ids=[f"{c[0]}-{'bf16' if c[1] == PREC_BF16 else 'fp32'}-M{c[2]}-N{c[3]}-K{c[4]}-{'mask' if c[5] else 'nomask'}-{'running' if c[6] else 'norunning'}"
                              for c in PRO_FIN_CASES])
def test_pro_finalize(kernel, prec, M, N, K, masked, running):
    case = ProFinCase(prec, M, N, K, masked, running, seed=M + 3 * N + 7 * K)
    tag = f"pro_finalize {kernel} {'bf16' if prec == PREC_BF16 else 'fp32'} M{M} N{N} K{K}"
    rows = G.ntp_rows(M, N) if kernel == "ntp" else G.ROWS_TILE
    with _kernel_setup(kernel, prec, M, N, K):
        # the folded form
        t1 = case.state()
        c1, st1 = case.outputs()
        keep = kernel == "ntp" and ops.can_keep_pro_out(prec, M, N, K, case.y, c1)
        assert keep == (kernel == "ntp" and M >= 16384)
        H = torch.full((M, K), 7.0, dtype=torch.bfloat16, device=DEV) if keep else None
        assert case.gemm(t1, c1, st1, fin=case.fin_args(t1), pro_out=H) == 0
        # the two-launch form it replaces, on state of its own
        t2 = case.state()
        c2, st2 = case.outputs()
        ops.bn_finalize_launch(case.fin_args(t2))
        assert case.gemm(t2, c2, st2) == 0
        torch.cuda.synchronize()
    _check_finalize(case, t1, tag, case.s_exact[0], case.s_exact[1])
    for k in t1:          # bit-identical to what mmvae_bn_finalize writes from the same sums (include/mmvae_hip.h promises it)
        assert unchanged(t1[k], snapshot(t2[k])), f"{tag}: {k} differs from mmvae_bn_finalize"
    h, dh = _check_product(case, t1, c1, st1, rows, tag)
    assert np.array_equal(bits(c1), bits(c2)), f"{tag}: C differs from the two-launch form"
    if st1 is not None:   # equal up to the order of summation: each inside the statistics bound of the same stored values
        inside(host(st1), host(st2), 2 * G.stats_tol(host(c1[:, :N]), rows), f"{tag} statistics against the two-launch form")
    if keep:              # the operand after the prologue: exact wherever it is not at risk
        inside(host(H), h, dh, f"{tag} pro_out")


def test_pro_finalize_chained_from_the_producing_gemm():
    """The real hand-off: GEMM 1 writes y (bf16) and accumulates its column statistics with atomics, GEMM 2 consumes them through
    pro_finalize.  Against float64 from the DATA (the stored y): E.bn_finalize_tol with sums_rel from the statistics bound."""
    M, K0, K, N = 4096, 96, 256, 40
    rng = np.random.default_rng(11)
    x = rnd(rng, M, K0)
    W0, b0 = rnd(rng, K, K0, scale=K0 ** -0.5) * rng.uniform(0.2, 3.0, (K, 1)).astype(F32), rnd(rng, K)
    W0[0], b0[0] = 0.0, 1000.0 + 1.0 / 3.0                     # a constant output column with a large mean
    pl0 = prep(W0, b0, PREC_BF16)
    y = torch.full((M, K), NAN, dtype=torch.bfloat16, device=DEV)
    stats = torch.zeros(2, K, dtype=torch.float64, device=DEV)
    with _kernel_setup("tile128", PREC_BF16, M, K, K0):
        ops.gemm_nt(PREC_BF16, dev(x), pl0.w, K, K0, y, bias=pl0.bias, stats=stats)
        case = ProFinCase(PREC_BF16, M, N, K, True, True, seed=12, y=y, stats=stats)
        t = case.state()
        c, _ = case.outputs()
        assert case.gemm(t, c, None, fin=case.fin_args(t)) == 0
        torch.cuda.synchronize()
    tag = "pro_finalize chained"
    inside(host(stats), case.s_exact, G.stats_tol(case.y_host, G.ROWS_TILE), f"{tag} statistics of GEMM 1")
    _check_finalize(case, t, tag, case.s_exact[0], case.s_exact[1], sums_rel=G.sums_rel(case.y_host, G.ROWS_TILE))
    dsum = host(stats)
    _check_finalize(case, t, tag + " (device sums)", dsum[0], dsum[1])
    _check_product(case, t, c, None, G.ROWS_TILE, tag)


def test_pro_finalize_refusals():
    M, N, K = 4096, 40, 128
    case = ProFinCase(PREC_BF16, M, N, K, True, True, seed=5)
    t = case.state()
    for k in ("mean", "rstd", "scale", "shift"):
        t[k].fill_(5.0)
    c, _ = case.outputs()
    st = torch.full((2, N), 3.0, dtype=torch.float64, device=DEV)
    watched = list(t.values()) + [c, st]
    before = [snapshot(x) for x in watched]
    good = case.fin_args(t)
    fields = [f for f, _ in L.BnFinalizeArgs._fields_]

    def fin(**change):
        return L.BnFinalizeArgs(*[change.get(f, getattr(good, f)) for f in fields])
    assert case.gemm(t, c, st, fin=fin(N=K - 64)) == ERR_ARG                        # fin->N != K
    assert case.gemm(t, c, st, fin=fin(M=1)) == ERR_ARG                             # fin->M < 2
    for f in ("sum", "sumsq", "gamma", "beta", "mean", "rstd", "scale", "shift"):   # a required pointer NULL
        assert case.gemm(t, c, st, fin=fin(**{f: None})) == ERR_ARG, f
    # prologue == NONE together with a pro_finalize
    g = L.GemmNtArgs()
    g.prec, g.M, g.N, g.K = PREC_BF16, M, N, K
    g.a, g.a_dtype, g.lda = case.y.data_ptr(), L.BF16, K
    g.w, g.ldw, g.c, g.c_dtype, g.ldc, g.bias = case.pl.w.data_ptr(), case.pl.w.stride(0), c.data_ptr(), L.F32, case.ldc, case.pl.bias.data_ptr()
    g.pro_finalize = C.addressof(good)
    assert L.load().mmvae_gemm_nt(C.byref(g), stream()) == ERR_ARG
    # the row-block path: every block would step the running statistics
    with tuning(k3=17):
        assert M * K * 2 >= 1 << 17
        assert case.gemm(t, c, st, fin=good) == ERR_ARG
    # K = 576: beyond the prologue's 512-column tables
    K2 = 576
    wide = ProFinCase(PREC_BF16, M, N, K2, True, True, seed=6)
    t2 = wide.state()
    for k in ("mean", "rstd", "scale", "shift"):
        t2[k].fill_(5.0)
    before2 = [snapshot(x) for x in t2.values()]
    assert wide.gemm(t2, c, st, fin=wide.fin_args(t2)) == ERR_ARG
    torch.cuda.synchronize()
    assert all(unchanged(x, b) for x, b in zip(watched, before)), "a refused call wrote something"
    assert all(unchanged(x, b) for x, b in zip(t2.values(), before2))


# =============================================================================================
# (b) the dW GEMM with mmvae_bn_bwd_finalize folded in
# =============================================================================================
# launch_tn_wide's forms of a BatchNorm-corrected bf16 P and an fp32 Q, as gemm_gpu_util.tn_wide_plan names them (that module
# imports this one, so the tests below import it when they run)
WIDE_FORMS = {"A": ("dma", (256, 288)), "B": ("reg", (128, 448))}


class BnDwCase:
    def __init__(self, M, N, K, ldq, d_pad, seed):
        rng = np.random.default_rng(seed)
        self.M, self.N, self.K = M, N, K
        d = rnd(rng, M, N) + rnd(rng, N, scale=0.5)                      # column means: sum_d / M is not negligible
        y = rnd(rng, M, N, scale=2.0) + F32(0.3)
        self.d, self.y = to_act(d, PREC_BF16, ld=N + d_pad, fill=7.0), to_act(y, PREC_BF16, fill=7.0)
        self.d_host, self.y_host = host(self.d), host(self.y)
        self.mean, self.rstd, self.gamma = rnd(rng, N, scale=0.2), rng.uniform(0.5, 1.5, N).astype(F32), rnd(rng, N) + 1.5
        xh = (self.y_host - self.mean) * self.rstd
        self.sd, self.sdx = self.d_host.sum(0), (self.d_host * xh).sum(0)       # the f64 column sums of the statistics phase
        q = rnd(rng, M, K) + F32(0.5)                                    # an input batch: not centred
        self.q = torch.full((M, ldq), 7.0, device=DEV)[:, :K]
        self.q.copy_(dev(q))
        self.q_host = G.q_bf16(q)                                        # rounded to bf16 on load, exactly
        self.old = dict(dw=rnd(rng, N, K), db=rnd(rng, N), dgamma=rnd(rng, N), dbeta=rnd(rng, N))
        self.t = dict(mean=dev(self.mean), rstd=dev(self.rstd), gamma=dev(self.gamma), stats=dev(np.stack([self.sd, self.sdx])))
        self.slab = torch.empty(1 << 25, device=DEV)

    def outputs(self):
        a = Arena([(self.N, self.K), (self.N,)])
        a.views[0].copy_(dev(self.old["dw"])); a.views[1].copy_(dev(self.old["db"]))
        return a, guarded(self.old["dgamma"]), guarded(self.old["dbeta"])

    def folded(self, a, dgamma, dbeta, eval_mode, prec=PREC_BF16, slab="own", nsplit=0, rows=None, cols=None, kcols=None, nulls=()):
        """-> status of mmvae_gemm_tn with the finalisation folded in, on the first rows / cols / kcols of the operands."""
        M, N, K = rows or self.M, cols or self.N, kcols or self.K
        fin = ops.BnBwdFinalize(self.t["stats"], self.t["gamma"], dgamma, dbeta, eval_mode)
        pro = ops.BnBwdApply(self.y[:M, :N], self.t["mean"], self.t["rstd"], fin=fin)
        dw, db = a.views[0].view(-1)[:N * K].view(N, K), a.views[1][:N]
        g = ops._tn_args(prec, self.d[:M, :N], self.q[:M, :K], dw, db, N, K, None, pro, nsplit, self.slab if slab == "own" else slab)
        for f in nulls:
            setattr(g, f, None)
        return L.load().mmvae_gemm_tn(C.byref(g), stream())


BN_DW_CASES = [  # M, N, K, ldq, extra columns of d's row stride, eval mode, form
    (8192, 512, 572, 572, 0, False, "A"),            # two N tiles, two K tiles
    (16384, 512, 572, 576, 0, True, "A"),
    (8192 + 96, 512, 280, 280, 0, False, "A"),       # a short last split, N tiles only
    (8192, 384, 300, 300, 0, True, "B"),             # least padded output: 3 x 1 tiles of 128 x 448 (256 x 288 would pad 384 -> 512, 300 -> 576)
    (8192 + 96, 128, 782, 782, 0, False, "B"),       # 8-byte fp32 rows: vectors of 2
    (16384, 128, 782, 782, 8, True, "B"),            # d's row stride differs from y's
    (8192 + 96, 384, 300, 300, 16, False, "B"),
]


@pytest.mark.parametrize("M,N,K,ldq,d_pad,eval_mode,form", BN_DW_CASES)
def test_tn_bn_bwd_finalize_folded(M, N, K, ldq, d_pad, eval_mode, form):
    case = BnDwCase(M, N, K, ldq, d_pad, seed=M + N + K)
    from gemm_gpu_util import tn_wide_plan
    plan = tn_wide_plan(M, N, K, True, "f32", ldq, N + d_pad, N, q_aligned=case.q.data_ptr() % 16 == 0)
    assert plan and plan[:2] == WIDE_FORMS[form] and plan[2] <= 32 and plan[3] >= 2 and plan[3] * N * K <= case.slab.numel(), plan
    tag = f"folded dW {form} M{M} N{N} K{K} {'eval' if eval_mode else 'train'}"
    a1, dg1, db1 = case.outputs()
    assert case.folded(a1, dg1, db1, eval_mode) == 0
    # the two-launch form on the same inputs
    a2, dg2, db2 = case.outputs()
    coef = torch.full((3, N), NAN, device=DEV)
    ops.bn_bwd_finalize(M, N, case.t["stats"], case.t["gamma"], case.t["rstd"], dg2, db2, coef, eval_mode)
    ops.gemm_tn(PREC_BF16, case.d, case.q, a2.views[0], a2.views[1], N, K,
                p_prologue=ops.BnBwdApply(case.y, case.t["mean"], case.t["rstd"], coef), slab=case.slab)
    torch.cuda.synchronize()
    # dgamma / dbeta: added ONCE per column, whatever the number of K tiles, N tiles and splits
    for got, old, s, name in ((dg1, case.old["dgamma"], case.sdx, "dgamma"), (db1, case.old["dbeta"], case.sd, "dbeta"),
                              (dg2, case.old["dgamma"], case.sdx, "dgamma, two launches"), (db2, case.old["dbeta"], case.sd, "dbeta, two launches")):
        inside(host(got[:N]), E.accum(old, s, F64), E.accum_tol(old, s), f"{tag} {name}")
        assert torch.isnan(got[N:]).all()
    p, dp = G.bn_bwd_operand(case.d_host, case.y_host, case.mean, case.rstd, case.sd, case.sdx, M, case.gamma, eval_mode)
    if eval_mode:
        assert np.array_equal(p, G.q_bf16((case.gamma * case.rstd).astype(F64) * case.d_host))       # gamma rstd d exactly
    rw, rb = G.dw_ref(p, case.q_host, case.old["dw"], case.old["db"])
    tw, tb = G.dw_tol(p, case.q_host, case.old["dw"], case.old["db"], dp=dp)
    for a, name in ((a1, ""), (a2, ", two launches")):
        inside(host(a.views[0]), rw, tw, f"{tag} dW{name}")
        inside(host(a.views[1]), rb, tb, f"{tag} db{name}")
        assert a.guards_unchanged(), "the gradient arena was written outside dw / db"


def test_tn_bn_bwd_finalize_folded_refusals():
    M, N, K = 8192, 128, 256
    case = BnDwCase(M, N, K, K, 0, seed=9)
    from gemm_gpu_util import tn_wide_plan
    assert tn_wide_plan(M, N, K, True, "f32", K, N, N)[:2] == WIDE_FORMS["B"]
    a, dg, db = case.outputs()
    watched = [a.buf, dg, db]
    before = [snapshot(x) for x in watched]
    f = lambda **k: case.folded(a, dg, db, False, **k)
    assert f(rows=4096) == ERR_ARG and f(cols=64) == ERR_ARG and f(kcols=128) == ERR_ARG
    assert f(slab=None) == ERR_ARG                                                   # no slab
    assert f(slab=case.slab[:N * K]) == ERR_ARG                                      # a slab below nsplit * N * K
    assert f(nsplit=3) == ERR_ARG
    for name in ("p_sum_d", "p_sum_dx", "p_gamma", "p_dgamma", "p_dbeta"):
        assert f(nulls=(name,)) == ERR_ARG, name
    with tuning(k4=0):
        assert f() == ERR_ARG                                                        # the wide-tile kernels switched off
    with tuning(k3=17):
        assert f() == ERR_ARG                                                        # the row-block path
    # fp32 mode (activation-typed d and y are fp32 there)
    d32, y32 = dev(case.d_host.astype(F32)), dev(case.y_host.astype(F32))
    fin = ops.BnBwdFinalize(case.t["stats"], case.t["gamma"], dg, db, False)
    assert status(ops.gemm_tn, PREC_F32, d32, case.q, a.views[0], a.views[1], N, K,
                  p_prologue=ops.BnBwdApply(y32, case.t["mean"], case.t["rstd"], fin=fin), slab=case.slab) == ERR_ARG
    torch.cuda.synchronize()
    assert all(unchanged(x, b) for x, b in zip(watched, before)), "a refused call wrote something"
    assert f() == 0                                                                  # the same arguments, unrestricted: taken


# =============================================================================================
# (c) mmvae_gemm_tn_group
# =============================================================================================
class GroupProblem:
    """One small dW problem.  combo 0: fp32 P, Q through the BatchNorm + ReLU + Dropout prologue; 1: P and Q activation-typed;
    2: fp32 P, activation-typed Q (in fp32 mode every plain operand is fp32: combos 1 and 2 coincide)."""

    def __init__(self, prec, combo, M, N, K, masked=False, seed=0, odd_ldp=False):
        rng = np.random.default_rng(seed + M + 3 * N + 7 * K + combo)
        bf = prec == PREC_BF16
        self.prec, self.combo, self.M, self.N, self.K = prec, combo, M, N, K
        P, Q = rnd(rng, M, N), rnd(rng, M, K, scale=1.5)
        pad = 8 if bf else 4
        if combo == 1:
            self.p = to_act(P, prec, ld=ops.ceil_to(N, pad), fill=7.0)
        else:
            self.p = torch.full((M, N + 1 if odd_ldp else N), 7.0, device=DEV)[:, :N]
            self.p.copy_(dev(P))
        self.q = to_act(Q, prec, ld=ops.ceil_to(K, pad), fill=7.0)
        ph, qh = host(self.p), host(self.q)
        self.p_host = G.q_bf16(ph) if bf else ph                          # an fp32 P is rounded to bf16 on load, exactly
        self.dq, self.pro = None, None
        if combo == 0:
            scale, shift = rng.uniform(0.5, 1.5, K).astype(F32), rnd(rng, K, scale=0.3)
            mask = (rng.random((M, K)) < 0.9).astype(np.uint8) if masked else None
            ik = 1.0 / 0.9 if masked else 1.0
            self.pro = ops.Prologue(dev(scale), dev(shift), dev(mask) if masked else None, ik)
            self.q_host, self.dq = G.prologue_operand(qh, scale, shift, ik, mask, bf)
        else:
            self.q_host = qh
        self.old_dw, self.old_db = rnd(rng, N, K), rnd(rng, N)
        self.slab = torch.empty(ops.TN_GROUP_SPLITS * N * K, device=DEV)

    def outputs(self):
        a = Arena([(self.N, self.K), (self.N,)])
        a.views[0].copy_(dev(self.old_dw)); a.views[1].copy_(dev(self.old_db))
        return a

    def args(self, a, slab="own"):
        return ops._tn_args(self.prec, self.p, self.q, a.views[0], a.views[1], self.N, self.K, self.pro, None, 0, self.slab if slab == "own" else slab)

    def as_dict(self, a):
        return dict(p=self.p, q=self.q, dw=a.views[0], db=a.views[1], N=self.N, K=self.K, q_prologue=self.pro)

    def check(self, a, tag, alone=None):
        rw, rb = G.dw_ref(self.p_host, self.q_host, self.old_dw, self.old_db)
        tw, tb = G.dw_tol(self.p_host, self.q_host, self.old_dw, self.old_db, dq=self.dq)
        inside(host(a.views[0]), rw, tw, f"{tag} dW"); inside(host(a.views[1]), rb, tb, f"{tag} db")
        assert a.guards_unchanged(), "the gradient arena was written outside dw / db"
        if alone is not None:         # the same problem through mmvae_gemm_tn: the same operands, another order of the fp32 sums
            ow, ob = G.dw_order_tol(self.p_host, self.q_host, self.old_dw, self.old_db)
            inside(host(a.views[0]), host(alone.views[0]), ow, f"{tag} dW against the single launch")
            inside(host(a.views[1]), host(alone.views[1]), ob, f"{tag} db against the single launch")


def group_call(problems, arenas, n=None):
    arr = (L.GemmTnArgs * max(len(problems), 1))()
    for j, (pr, a) in enumerate(zip(problems, arenas)):
        arr[j] = pr if isinstance(pr, L.GemmTnArgs) else pr.args(a)
    return L.load().mmvae_gemm_tn_group(C.cast(arr, C.c_void_p), len(problems) if n is None else n, stream())


def _group(prec, size):
    """Problems of different M, N, K for one launch: the production shapes (encoder heads N = 40 with K = 128 / 256, the merged decoder
    stems 448 x 20, DecoderC's class width 24 x 64), ragged ones (24 x 72), one at the engine's _TINY_DW_MAX (64 x 256 = 16 384)."""
    from mmvae import engine
    assert 64 * 256 == engine._TINY_DW_MAX
    P = lambda *a, **k: GroupProblem(prec, *a, **k)
    if size == 1:
        return [P(1, 4096, 24, 72)]
    if size == 3:
        return [P(0, 130, 40, 128), P(1, 65536, 64, 20), P(2, 2, 24, 64)]
    return [P(0, 4096, 40, 128, masked=True), P(0, 65536, 40, 256), P(1, 4096, 448, 20), P(1, 130, 448, 20),
            P(2, 4096, 24, 64), P(1, 2, 24, 72), P(0, 130, 64, 256, masked=True), P(2, 65536, 24, 64)]


@pytest.mark.parametrize("size", [1, 3, 8])
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_F32], ids=["bf16", "fp32"])
def test_tn_group(prec, size):
    problems = _group(prec, size)
    if prec == PREC_BF16:      # activation-typed P and Q: one M the LDS-DMA form takes (whole 64-row steps) and one it does not
        ms = [pr.M % 64 == 0 for pr in problems if pr.combo == 1]
        assert size < 8 or (any(ms) and not all(ms))
    arenas = [pr.outputs() for pr in problems]
    assert group_call(problems, arenas) == 0
    alone = [pr.outputs() for pr in problems]
    for pr, a in zip(problems, alone):
        assert L.load().mmvae_gemm_tn(C.byref(pr.args(a)), stream()) == 0
    torch.cuda.synchronize()
    for i, (pr, a, b) in enumerate(zip(problems, arenas, alone)):
        pr.check(a, f"group of {size} {'bf16' if prec == PREC_BF16 else 'fp32'} #{i} combo{pr.combo} M{pr.M} N{pr.N} K{pr.K}", alone=b)


@pytest.mark.parametrize("prec", [PREC_BF16, PREC_F32], ids=["bf16", "fp32"])
def test_tn_group_refusals(prec):
    mk = lambda i, **k: GroupProblem(prec, i % 3, 4096, 40, 128, seed=i, **k)
    problems = [mk(i) for i in range(9)]
    arenas = [pr.outputs() for pr in problems]
    before = [snapshot(a.buf) for a in arenas]
    base = lambda n=3: [problems[i].args(arenas[i]) for i in range(n)]

    def changed(i, n=3, **fields):
        gs = base(n)
        for f, v in fields.items():
            setattr(gs[i], f, v)
        return gs
    assert group_call(base(), arenas, n=0) == ERR_ARG
    assert group_call(base(9), arenas, n=9) == ERR_ARG
    assert group_call(changed(2, slab=problems[0].slab.data_ptr()), arenas) == ERR_ARG            # two problems sharing a slab
    assert group_call(changed(1, prec=PREC_F32 if prec == PREC_BF16 else PREC_BF16), arenas) == ERR_ARG
    assert group_call(changed(1, p_prologue=ops.PRO_BN_BWD_APPLY), arenas) == ERR_ARG
    assert group_call(changed(2, lddw=128 + 8), arenas) == ERR_ARG
    assert group_call(changed(0, slab=None, slab_elems=0), arenas) == ERR_ARG
    assert group_call(changed(2, slab_elems=40 * 128), arenas) == ERR_ARG                        # one split's worth: the plan needs more
    # an ineligible problem (fp32 P with an odd row stride) in position 5 of 8: nothing of the group may have been launched
    odd = GroupProblem(prec, 2, 4096, 40, 128, seed=99, odd_ldp=True)
    assert ops._ld(odd.p) % 2 == 1
    group8 = problems[:4] + [odd] + problems[5:8]
    arenas8 = arenas[:4] + [odd.outputs()] + arenas[5:8]
    odd_before = snapshot(arenas8[4].buf)
    assert group_call(group8, arenas8) == ERR_ARG
    torch.cuda.synchronize()
    assert all(unchanged(a.buf, b) for a, b in zip(arenas, before)), "a refused call wrote something"
    assert unchanged(arenas8[4].buf, odd_before)
    # through ops.gemm_tn_group the per-problem fallback still computes every problem of that group
    slab = torch.empty(ops.TN_GROUP_SPLITS * sum(pr.N * pr.K for pr in group8), device=DEV)
    ops.gemm_tn_group(prec, [pr.as_dict(a) for pr, a in zip(group8, arenas8)], slab)
    torch.cuda.synchronize()
    for i, (pr, a) in enumerate(zip(group8, arenas8)):
        pr.check(a, f"group fallback {'bf16' if prec == PREC_BF16 else 'fp32'} #{i}")
