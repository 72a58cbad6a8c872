"""Tensor-level wrappers over the C ABI (include/mmvae_hip.h).  PyTorch is used here only as
the owner of device memory and streams; all arithmetic happens in libmmvae_hip.so."""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L
from ._lib import (F32, BF16, PREC_F32, PREC_BF16, PRO_NONE, PRO_BN_RELU_DROP, PRO_BN_BWD_APPLY, EPI_STORE, EPI_RELU_MASK,
                   EPI_BN_BWD, EPI_LOSS_MSE, EPI_LOSS_BCE_LOGIT, ACT_NONE, ACT_RELU, ACT_SIGMOID, TILE)

DROP_P = 0.1                      # nn.Dropout(0.1), reference src/models/encoders.py:16,34,38
BN_EPS, BN_MOMENTUM = 1e-5, 0.1   # nn.BatchNorm1d defaults, encoders.py:14,32,36


class KernelProbe:
    """Optional per-launch timer: HIP events recorded on the launch stream around tagged GEMM
    launches (bench.py uses it for the live roofline numbers).  Off (None) by default."""

    def __init__(self, only=None):
        self.records = {}          # tag -> [(start_event, end_event, meta)]
        self.only = only           # optional set of tags to time (None = all)

    def wants(self, tag):
        return tag is not None and (self.only is None or tag in self.only)

    def begin(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        return ev

    def end(self, tag, start, meta):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        self.records.setdefault(tag, []).append((start, ev, meta))

    def summary(self):
        """tag -> dict(calls, mean_ms, meta); call after torch.cuda.synchronize()."""
        out = {}
        for tag, recs in self.records.items():
            ms = [s.elapsed_time(e) for s, e, _ in recs]
            out[tag] = dict(calls=len(ms), mean_ms=sum(ms) / len(ms), meta=recs[0][2])
        return out


PROBE = None


class probe_span:
    """`with probe_span(tag, meta)`: brackets a launch with events when a KernelProbe is installed (bench.py's survey of the step);
    `meta` is the record's dict or a callable producing it (called only when the span is timed).  A launch the library refused
    (it enqueued nothing) leaves no record."""

    def __init__(self, tag, meta):
        self.tag, self.meta, self.t0 = tag, meta, None

    def __enter__(self):
        if PROBE is not None and PROBE.wants(self.tag):
            self.t0 = PROBE.begin()
        return self

    def __exit__(self, exc_type, *exc):
        if self.t0 is not None and exc_type is None:
            PROBE.end(self.tag, self.t0, self.meta() if callable(self.meta) else self.meta)
        return False


def stream_span(tag, nbytes):
    """probe_span of a non-GEMM launch; `nbytes` = its algorithmic HBM bytes (operands read once + results written once), or a
    callable producing them."""
    return probe_span(tag, lambda: dict(kind="stream", bytes=int(nbytes() if callable(nbytes) else nbytes)))


def ceil_to(x, m):
    return (x + m - 1) // m * m


def act_dtype(prec):
    return torch.bfloat16 if prec == PREC_BF16 else torch.float32


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _p(t):
    return None if t is None else t.data_ptr()


_STREAM_OVERRIDE = None     # raw hipStream_t handle pinned by engine code for a span of launches (torch.cuda.current_stream()
                            # costs ~10 us per query, more than building the argument struct)


def _stream():
    return _STREAM_OVERRIDE if _STREAM_OVERRIDE is not None else torch.cuda.current_stream().cuda_stream


class pinned_stream:
    """Context manager: resolve the current stream ONCE and use its handle for every launch inside."""

    def __init__(self, stream=None):
        self.handle = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream

    def __enter__(self):
        global _STREAM_OVERRIDE
        self.prev, _STREAM_OVERRIDE = _STREAM_OVERRIDE, self.handle
        return self

    def __exit__(self, *exc):
        global _STREAM_OVERRIDE
        _STREAM_OVERRIDE = self.prev
        return False


def _mat(t, name):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: need a 2-D tensor with unit inner stride, got {tuple(t.shape)} / {t.stride()}")
    if not t.is_cuda:
        raise ValueError(f"{name}: must live on the GPU")
    return t


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _no_cpu(t, name, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: {name} must be a CUDA/HIP tensor; there is no CPU fallback")


def _device_matrix(t, name, what):
    """ACCEPT AND NORMALISE what a user hands over: t, detached, as a 2-D fp32 / bf16 device matrix the kernels can read in place (a
    1-D tensor is one column; copied to contiguous only where rows overlap or the inner stride is not 1); `what` names the caller.
    The wrappers below do not normalise: they check with _operand and refuse."""
    _no_cpu(t, name, what)
    if t.dim() == 1:
        t = t.unsqueeze(1)
    if t.dim() != 2 or t.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{what}: {name} must be a 2-D fp32 or bf16 tensor, got {tuple(t.shape)} {t.dtype}")
    t = t.detach()
    return t if t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]) else t.contiguous()


def _column_means(x):
    return x.double().mean(dim=0).float().contiguous()


# --------------------------------------------------------------------------------------------
# inputs in bf16 storage ("padded bf16 rows", include/mmvae_hip.h: mmvae_rows_to_bf16)
# --------------------------------------------------------------------------------------------
def is_bf16_rows(t):
    """t is a (B, F) bf16 device matrix in the padded-row layout: unit inner stride, leading dimension a multiple of 8 elements,
    16-byte aligned base.  (The pad columns F .. ld-1 must hold zeros; that is the producer's promise -- to_bf16_rows keeps it.)"""
    return (t.dtype == torch.bfloat16 and t.dim() == 2 and t.is_cuda and t.shape[0] > 0 and t.stride(1) == 1 and _ld(t) % 8 == 0
            and _ld(t) >= t.shape[1] and t.data_ptr() % 16 == 0)


def rows_to_bf16(src, dst):
    """dst (a padded-bf16-rows view, see is_bf16_rows) <- bf16(src) with the pad columns zeroed, ONE launch (mmvae_rows_to_bf16).
    src: fp32 or bf16 (B, F) with unit inner stride and any row stride; rounding is bit-identical to torch's .to(torch.bfloat16)."""
    _mat(src, "src"); _mat(dst, "dst")
    if tuple(src.shape) != tuple(dst.shape) or not is_bf16_rows(dst):
        raise ValueError(f"rows_to_bf16: {tuple(src.shape)} {src.dtype} -> {tuple(dst.shape)} {dst.dtype} / {dst.stride()}")
    B, F = src.shape
    ld = _ld(dst)
    if dst.untyped_storage().nbytes() < dst.storage_offset() * 2 + B * ld * 2:
        raise ValueError("rows_to_bf16: dst must own whole padded rows (B x ld elements)")
    with stream_span("rows_to_bf16", B * F * src.element_size() + B * ld * 2):
        L.check(L.load().mmvae_rows_to_bf16(src.data_ptr(), _dt(src), _ld(src), dst.data_ptr(), ld, B, F, _stream()), "mmvae_rows_to_bf16")
    return dst


def zeros_bf16_rows(B, F, device):
    """A zeroed (B, F) view of a (B, ceil8(F)) bf16 buffer: a static batch buffer in the padded-row layout."""
    return torch.zeros(B, ceil_to(F, 8), dtype=torch.bfloat16, device=device)[:, :F]


def to_bf16_rows(x):
    """(N, F) fp32 or bf16 device tensor -> a NEW (N, F) bf16 view of an (N, ceil8(F)) buffer in the padded-row layout, pads zeroed,
    values rounded as x.to(torch.bfloat16).  Convert a dataset once and hand it to the model / GraphedTrainStep(dataset=...): the
    first-layer GEMMs, their dW GEMMs and the reconstruction losses then read 2 bytes per element instead of 4."""
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 1:          # a vector has no padded rows; _device_matrix would make it a column
        raise ValueError(f"to_bf16_rows: need a 2-D fp32 or bf16 tensor, got {tuple(x.shape)} {x.dtype}")
    x = _device_matrix(x, "x", "to_bf16_rows")
    N, F = x.shape
    out = torch.empty(N, ceil_to(F, 8), dtype=torch.bfloat16, device=x.device)[:, :F]
    if N == 0 or F == 0:
        return out
    if _STREAM_OVERRIDE is not None:        # inside the engine's pinned span
        return rows_to_bf16(x, out)
    with pinned_stream():
        return rows_to_bf16(x, out)


# --------------------------------------------------------------------------------------------
# prepared weights
# --------------------------------------------------------------------------------------------
class PreparedLinear:
    """MFMA operand copies of one (possibly row-concatenated) Linear: W [ceil128(N)][ceil64(K)]
    and W^T [ceil128(K)][ceil64(N)] in the compute type, plus the fp32 bias (concatenated if
    the sources are)."""

    def __init__(self, weights, biases, prec, device):
        self.N = sum(w.shape[0] for w in weights)
        self.K = weights[0].shape[1]
        self.prec = prec
        dt = act_dtype(prec)
        self.w = torch.zeros(ceil_to(self.N, TILE), ceil_to(self.K, 64), dtype=dt, device=device)
        self.wt = torch.zeros(ceil_to(self.K, TILE), ceil_to(self.N, 64), dtype=dt, device=device)
        self.srcs = list(weights)
        self.bias_srcs = list(biases)
        if len(biases) == 1:
            self.bias = biases[0]
            self._bias_cat = None
        else:
            self._bias_cat = torch.zeros(self.N, dtype=torch.float32, device=device)
            self.bias = self._bias_cat

    def items(self):
        out = []
        dtc = _dt(self.w)
        row = 0
        esz = self.w.element_size()
        for i, w in enumerate(self.srcs):
            n = w.shape[0]
            last = i == len(self.srcs) - 1
            # plain copy: rows [row, row+n) (the last item also clears the padding rows)
            rows = (self.w.shape[0] - row) if last else n
            out.append(L.PrepItem(w.data_ptr(), self.w.data_ptr() + row * self.w.stride(0) * esz, n, self.K, w.stride(0),
                                  rows, self.w.shape[1], self.w.stride(0), 0, dtc))
            # transposed copy: columns [row, row+n)
            cols = (self.wt.shape[1] - row) if last else n
            out.append(L.PrepItem(w.data_ptr(), self.wt.data_ptr() + row * esz, n, self.K, w.stride(0),
                                  self.wt.shape[0], cols, self.wt.stride(0), 1, dtc))
            if self._bias_cat is not None:
                b = self.bias_srcs[i]
                out.append(L.PrepItem(b.data_ptr(), self._bias_cat.data_ptr() + row * 4, 1, n, n, 1, n, n, 0, F32))
            row += n
        return out


class WeightPrep:
    """All PreparedLinears of a module tree, refreshed from the fp32 masters in ONE launch."""

    def __init__(self, linears, device):
        self.linears = list(linears)
        items = [it for pl in self.linears for it in pl.items()]
        self.n = len(items)
        arr = (L.PrepItem * self.n)(*items)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.table = host.to(device)

    def nbytes(self):
        return sum(6 * w.numel() for pl in self.linears for w in pl.srcs)

    def run(self):
        with stream_span("prep_weights", self.nbytes):
            L.check(L.load().mmvae_prep_weights(self.table.data_ptr(), self.n, _stream()), "mmvae_prep_weights")


# --------------------------------------------------------------------------------------------
# GEMMs
# --------------------------------------------------------------------------------------------
def can_keep_pro_out(prec, M, N, K, a, out):
    """Will mmvae_gemm_nt write `pro_out` for this problem?  Mirrors the conditions of the wave-specialised kernel's prologue variant
    (include/mmvae_hip.h, gemm_ntp.hip): the library answers MMVAE_ERR_ARG when asked for pro_out outside them."""
    return (prec == PREC_BF16 and a.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and M >= 16384 and M % 128 == 0
            and N % 128 == 0 and N <= 256 and K % 64 == 0 and 64 < K <= 512 and _ld(a) % 8 == 0 and _ld(out) % 64 == 0
            and M * _ld(a) * 2 < 2 ** 31            # one launch: the row-block path of >= 4 GiB operands refuses pro_out
            and a.data_ptr() % 16 == 0 and out.data_ptr() % 128 == 0)


# The operand records of the GEMMs.  The wrappers below unpack them by position, so a plain tuple of the same fields serves too.
# Prologue: BatchNorm + ReLU + Dropout applied to an operand on load, relu(x * scale + shift) * mask * inv_keep (mask None: no dropout).
Prologue = namedtuple("Prologue", "scale shift mask inv_keep")
# BnBwdEpilogue: the `bn=` operand of EPI_BN_BWD -- the layer's BatchNorm vectors and the dropout mask its output went through.
BnBwdEpilogue = namedtuple("BnBwdEpilogue", "scale shift mean rstd mask inv_keep")
# BnBwdFinalize: operands of mmvae_bn_bwd_finalize folded into the launch that consumes the backward sums (stats: float64 [2][N]).
BnBwdFinalize = namedtuple("BnBwdFinalize", "stats gamma dgamma dbeta eval_mode")
# BnBwdApply: `p_prologue` of a dW GEMM -- the BatchNorm-backward correction applied on the load of p, from the three constants per
# column (`coef`) or, with the finalisation folded into the GEMM, from the sums themselves (`fin`, a BnBwdFinalize).
BnBwdApply = namedtuple("BnBwdApply", "y mean rstd coef fin", defaults=(None, None))


def _fill_prologue(g, prologue):
    """The BN+ReLU+Dropout prologue fields that GemmNtArgs and GemmTnArgs share; -> the prologue code."""
    sc, sh, mask, inv_keep = prologue
    g.pro_scale, g.pro_shift, g.pro_mask = sc.data_ptr(), sh.data_ptr(), _p(mask)
    g.ld_pro_mask = _ld(mask) if mask is not None else 0
    g.pro_inv_keep = inv_keep
    return PRO_BN_RELU_DROP


def gemm_nt(prec, a, w_lp, N, K, out, *, bias=None, act=ACT_NONE, accumulate=False, prologue=None,
            epilogue=EPI_STORE, h=None, bn=None, bn_coef=None, bn_phase=None, stats=None, loss_sum=None, tag=None, pro_out=None,
            pro_finalize=None):
    """out[M,N] = epi( pro(a)[M,K] @ W[N,K]^T ).  prologue = Prologue / (scale, shift, mask|None, inv_keep);
    bn = BnBwdEpilogue / (scale, shift, mean, rstd, mask|None, inv_keep) for EPI_BN_BWD (out=None, stats given:
    statistics phase; out and bn_coef given: apply phase).  stats: zeroed float64 [2][N] accumulator.
    EPI_LOSS_MSE / EPI_LOSS_BCE_LOGIT: h = fp32 or bf16 target (rows 2-byte aligned; padded bf16 rows give the widest loads),
    out = bf16 gradient, loss_sum = one-element float64 view that is added to."""
    _mat(a, "a"); _mat(w_lp, "w")
    if out is not None:
        _mat(out, "out")
    M = a.shape[0]
    g = L.GemmNtArgs()
    g.prec, g.M, g.N, g.K = prec, M, N, K
    g.a, g.a_dtype, g.lda = a.data_ptr(), _dt(a), _ld(a)
    if prologue is not None:
        g.prologue = _fill_prologue(g, prologue)
        if pro_out is not None:                 # the operand after the prologue (bf16 [M][>= K]); see can_keep_pro_out()
            g.pro_out, g.ld_pro_out = pro_out.data_ptr(), _ld(pro_out)
        if pro_finalize is not None:            # BnFinalizeArgs of the layer that produced `a` (bn_finalize_args()): finalised inside this launch
            g.pro_finalize = C.addressof(pro_finalize)
    g.w, g.ldw = w_lp.data_ptr(), w_lp.stride(0)
    g.epilogue = epilogue
    if out is not None:
        g.c, g.c_dtype, g.ldc = out.data_ptr(), _dt(out), _ld(out)
    g.bias, g.act, g.accumulate = _p(bias), act, int(accumulate)
    if h is not None:
        g.h, g.ldh = h.data_ptr(), _ld(h)
    if bn is not None:
        sc, sh, mean, rstd, mask, inv_keep = bn
        g.bn_scale, g.bn_shift, g.bn_mean, g.bn_rstd = sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), rstd.data_ptr()
        g.epi_mask, g.ld_epi_mask, g.epi_inv_keep = _p(mask), (_ld(mask) if mask is not None else 0), inv_keep
        g.bn_coef = _p(bn_coef)
        g.bn_phase = bn_phase if bn_phase is not None else int(bn_coef is not None)
    if stats is not None:
        assert stats.dtype == torch.float64 and stats.shape[0] == 2 and stats.shape[1] >= N and stats.stride(1) == 1
        g.stat1, g.stat2 = stats[0].data_ptr(), stats[1].data_ptr()
    if loss_sum is not None:
        assert loss_sum.dtype == torch.float64 and h is not None and h.dtype in (torch.float32, torch.bfloat16)
        g.stat1, g.h_dtype = loss_sum.data_ptr(), _dt(h)
    with probe_span(tag, lambda: dict(kind="nt", M=M, N=N, K=K, a_bytes=a.element_size(),
                                      c_bytes=0 if out is None else out.element_size(),
                                      pro=prologue is not None, pro_mask=g.pro_mask is not None,
                                      epi=epilogue, epi_mask=g.epi_mask is not None, act_bytes=2 if prec == PREC_BF16 else 4)):
        L.check(L.load().mmvae_gemm_nt(C.byref(g), _stream()), "mmvae_gemm_nt")
    return out


def _tn_args(prec, p, q, dw, db, N, K, q_prologue, p_prologue, nsplit, slab):
    _mat(p, "p"); _mat(q, "q")
    g = L.GemmTnArgs()
    g.prec, g.M, g.N, g.K = prec, p.shape[0], N, K
    g.p, g.p_dtype, g.ldp = p.data_ptr(), _dt(p), _ld(p)
    g.q, g.q_dtype, g.ldq = q.data_ptr(), _dt(q), _ld(q)
    if q_prologue is not None:
        g.q_prologue = _fill_prologue(g, q_prologue)
    if p_prologue is not None:
        py, mean, rstd, coef, *fin = p_prologue             # (y, mean, rstd, coef), or a BnBwdApply with its fifth field
        _mat(py, "p_y")
        g.p_prologue = PRO_BN_BWD_APPLY
        g.p_y, g.ld_py, g.p_mean, g.p_rstd = py.data_ptr(), _ld(py), mean.data_ptr(), rstd.data_ptr()
        if coef is not None:
            assert py.dtype == p.dtype and coef.shape[0] == 3 and coef.shape[1] == N and coef.is_contiguous()
            g.p_coef = coef.data_ptr()
        else:
            stats, gamma, dgamma, dbeta, eval_mode = fin[0]   # BnBwdFinalize: mmvae_bn_bwd_finalize folded into the GEMM
            assert py.dtype == p.dtype and stats.dtype == torch.float64 and stats.shape[0] == 2 and stats.stride(1) == 1
            g.p_sum_d, g.p_sum_dx, g.p_gamma = stats[0].data_ptr(), stats[1].data_ptr(), gamma.data_ptr()
            g.p_dgamma, g.p_dbeta, g.p_eval_mode = dgamma.data_ptr(), dbeta.data_ptr(), int(eval_mode)
    assert dw.dtype == torch.float32 and dw.is_contiguous()
    g.dw, g.lddw, g.db = dw.data_ptr(), K, _p(db)
    g.nsplit = nsplit
    if slab is not None:
        g.slab, g.slab_elems = slab.data_ptr(), slab.numel()
    return g


TN_GROUP_SPLITS = 256        # MMVAE_TN_GROUP_SPLITS: most batch splits a problem of a grouped launch can get (slab sizing)


def tn_riders(embed_bwd=None, loss=None):
    """-> TnRiders of mmvae_gemm_tn_group_riders.  embed_bwd: embed_table_bwd's arguments (a tuple); loss: loss_finalize's
    (sums, beta, gamma, out5, beta_gamma_dev)."""
    r = L.TnRiders()
    if embed_bwd is not None:
        emb, w_mu, w_lv, d_table, d_emb, d_w_mu, d_b_mu, d_w_lv, d_b_lv = embed_bwd
        r.S, r.E, r.L = emb.shape[0], emb.shape[1], w_mu.shape[0]
        r.table_copies = d_table.shape[0] if d_table.dim() == 3 else 1
        r.emb, r.w_mu, r.w_lv, r.d_table = emb.data_ptr(), w_mu.data_ptr(), w_lv.data_ptr(), d_table.data_ptr()
        r.d_emb, r.d_w_mu, r.d_b_mu, r.d_w_lv, r.d_b_lv = (t.data_ptr() for t in (d_emb, d_w_mu, d_b_mu, d_w_lv, d_b_lv))
    if loss is not None:
        sums, beta, gamma, out5, beta_gamma_dev = loss
        assert sums.dtype == torch.float64 and sums.numel() >= 5 and out5.numel() >= 5
        r.sums, r.beta, r.gamma, r.beta_gamma_dev, r.out5 = sums.data_ptr(), beta, gamma, _p(beta_gamma_dev), out5.data_ptr()
    return r


def gemm_tn_group(prec, problems, slab, tag="tiny_dW.group", riders=None):
    """problems: list of dicts(p, q, dw, db, N, K, q_prologue=None): SMALL-output dW GEMMs (latent / class widths) launched as
    ONE grouped GEMM + ONE reduce.  `slab`: fp32 workspace carved into one region per problem.
    riders: a TnRiders (tn_riders()) whose work runs as extra workgroups of the first grouped launch.  Returns whether it did: the
    library refuses riders it cannot carry with nothing enqueued, the group then runs without them and the caller issues their
    stand-alone launches."""
    lib = L.load()
    rode = False
    for i in range(0, len(problems), L.TN_GROUP_MAX):
        chunk = problems[i:i + L.TN_GROUP_MAX]
        arr = (L.GemmTnArgs * len(chunk))()
        off, nbytes = 0, 0
        for j, pr in enumerate(chunk):
            need = TN_GROUP_SPLITS * pr["N"] * pr["K"]
            if off + need > slab.numel():
                raise RuntimeError("gemm_tn_group: slab workspace too small")
            arr[j] = _tn_args(prec, pr["p"], pr["q"], pr["dw"], pr["db"], pr["N"], pr["K"], pr.get("q_prologue"), None, 0, slab[off:off + need])
            off += need
            nbytes += pr["p"].shape[0] * (pr["N"] * pr["p"].element_size() + pr["K"] * pr["q"].element_size()) + 4 * pr["N"] * pr["K"]
        # the record says which form ran: `grouped` (False: one launch per problem), `riders` (they rode in this launch); built only
        # when a probe is installed -- probe_span ignores it otherwise
        meta = dict(kind="stream", bytes=int(nbytes), grouped=True, riders=False) if PROBE is not None else {}
        with probe_span(tag if i == 0 else f"{tag}.{i}", meta):
            if i == 0 and riders is not None:
                status = lib.mmvae_gemm_tn_group_riders(C.cast(arr, C.c_void_p), len(chunk), C.byref(riders), _stream())
                if status != -1:
                    L.check(status, "mmvae_gemm_tn_group_riders")
                    rode = meta["riders"] = True
                    continue
            status = lib.mmvae_gemm_tn_group(C.cast(arr, C.c_void_p), len(chunk), _stream())
            if status == -1:
                meta["grouped"] = False
                # a problem outside the grouped kernel's operand combinations (odd widths / alignments): the entry point checks
                # every problem before it launches anything, so the same argument records go through the one-problem entry
                for j in range(len(chunk)):
                    L.check(lib.mmvae_gemm_tn(C.byref(arr[j]), _stream()), "mmvae_gemm_tn")
            else:
                L.check(status, "mmvae_gemm_tn_group")
    return rode


def gemm_tn(prec, p, q, dw, db, N, K, *, q_prologue=None, p_prologue=None, nsplit=0, slab=None, tag=None):
    """dw[N,K] += pro_p(p)[M,N]^T @ pro(q)[M,K] ; db[N] += colsum(pro_p(p)).  dw/db fp32, pre-zeroed.
    q_prologue: as gemm_nt's prologue.  p_prologue = BnBwdApply / (y, mean, rstd, coef): the BatchNorm-backward correction of mmvae_bn_bwd_apply applied on the load of p."""
    g = _tn_args(prec, p, q, dw, db, N, K, q_prologue, p_prologue, nsplit, slab)
    with probe_span(tag, lambda: dict(kind="tn", M=p.shape[0], N=N, K=K, p_bytes=p.element_size() * (2 if p_prologue is not None else 1),
                                      q_bytes=q.element_size(), pro_mask=g.pro_mask is not None)):
        L.check(L.load().mmvae_gemm_tn(C.byref(g), _stream()), "mmvae_gemm_tn")


# --------------------------------------------------------------------------------------------
# BatchNorm pieces
# --------------------------------------------------------------------------------------------
def bn_finalize_args(M, N, stats, gamma, beta, running_mean, running_var, nbt, mean, rstd, scale, shift,
                     eps=BN_EPS, momentum=BN_MOMENTUM):
    """The argument struct of mmvae_bn_finalize: launched on its own (bn_finalize) or handed to the consumer GEMM (gemm_nt(pro_finalize=))."""
    if M < 2:
        # same failure mode as torch.nn.BatchNorm1d in training mode
        raise ValueError(f"Expected more than 1 value per channel when training, got input size [{M}, {N}]")
    return L.BnFinalizeArgs(M, N, stats[0].data_ptr(), stats[1].data_ptr(),
                            gamma.data_ptr(), beta.data_ptr(), eps, momentum, _p(running_mean), _p(running_var), _p(nbt),
                            mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr())


def bn_finalize_launch(args):
    """mmvae_bn_finalize on a prebuilt BnFinalizeArgs (bn_finalize_args())."""
    L.check(L.load().mmvae_bn_finalize(C.byref(args), _stream()), "mmvae_bn_finalize")


def bn_finalize(M, N, stats, gamma, beta, running_mean, running_var, nbt, mean, rstd, scale, shift,
                eps=BN_EPS, momentum=BN_MOMENTUM):
    bn_finalize_launch(bn_finalize_args(M, N, stats, gamma, beta, running_mean, running_var, nbt, mean, rstd, scale, shift, eps, momentum))


def bn_eval_coeffs(gamma, beta, running_mean, running_var, scale, shift, eps=BN_EPS, mean=None, rstd=None):
    L.check(L.load().mmvae_bn_eval_coeffs(gamma.numel(), gamma.data_ptr(), beta.data_ptr(), running_mean.data_ptr(),
                                          running_var.data_ptr(), eps, scale.data_ptr(), shift.data_ptr(), _p(mean), _p(rstd), _stream()),
            "mmvae_bn_eval_coeffs")


def bn_bwd_finalize(M, N, stats, gamma, rstd, dgamma, dbeta, coef, eval_mode=False):
    a = L.BnBwdFinalizeArgs(M, N, stats[0].data_ptr(), stats[1].data_ptr(),
                            gamma.data_ptr(), rstd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), coef.data_ptr(), int(eval_mode))
    L.check(L.load().mmvae_bn_bwd_finalize(C.byref(a), _stream()), "mmvae_bn_bwd_finalize")


def bn_bwd_finalize_apply(d, y, M, N, mean, rstd, stats, gamma, dgamma, dbeta, eval_mode=False):
    """mmvae_bn_bwd_finalize + mmvae_bn_bwd_apply in one launch (the hidden widths of the model; raises for others)."""
    with stream_span(f"bn_bwd_apply.N{N}", 3 * d.shape[0] * N * d.element_size()):
        L.check(L.load().mmvae_bn_bwd_finalize_apply(_dt(d), M, N, d.data_ptr(), _ld(d), y.data_ptr(), _ld(y), mean.data_ptr(), rstd.data_ptr(),
                                                     stats[0].data_ptr(), stats[1].data_ptr(), gamma.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                                     int(eval_mode), _stream()), "mmvae_bn_bwd_finalize_apply")


def bn_bwd_apply(d, y, N, mean, rstd, coef):
    with stream_span(f"bn_bwd_apply.N{N}", 3 * d.shape[0] * N * d.element_size()):
        L.check(L.load().mmvae_bn_bwd_apply(_dt(d), d.shape[0], N, d.data_ptr(), _ld(d), y.data_ptr(), _ld(y),
                                            mean.data_ptr(), rstd.data_ptr(), coef.data_ptr(), _stream()), "mmvae_bn_bwd_apply")


# --------------------------------------------------------------------------------------------
# EncoderC table, fusion, loss, noise, optimiser
# --------------------------------------------------------------------------------------------
def embed_table_fwd(emb, w_mu, b_mu, w_lv, b_lv, table):
    S, E = emb.shape
    L.check(L.load().mmvae_embed_table_fwd(S, E, w_mu.shape[0], emb.data_ptr(), w_mu.data_ptr(), b_mu.data_ptr(),
                                           w_lv.data_ptr(), b_lv.data_ptr(), table.data_ptr(), _stream()), "mmvae_embed_table_fwd")


def embed_table_bwd(emb, w_mu, w_lv, d_table, d_emb, d_w_mu, d_b_mu, d_w_lv, d_b_lv):
    """d_table: [S][2L] or [copies][S][2L] (the copies mmvae_fuse_reparam_bwd scattered into; summed here)."""
    S, E = emb.shape
    copies = d_table.shape[0] if d_table.dim() == 3 else 1
    L.check(L.load().mmvae_embed_table_bwd(S, E, w_mu.shape[0], emb.data_ptr(), w_mu.data_ptr(), w_lv.data_ptr(),
                                           d_table.data_ptr(), copies, d_emb.data_ptr(), d_w_mu.data_ptr(), d_b_mu.data_ptr(),
                                           d_w_lv.data_ptr(), d_b_lv.data_ptr(), _stream()), "mmvae_embed_table_bwd")


def fuse_reparam_fwd(B, Ld, heads_a, heads_b, table, site, eps, mu, logvar, z):
    n_mod = (heads_a is not None) + (heads_b is not None) + (table is not None)
    hd = heads_a if heads_a is not None else heads_b
    a = L.FuseFwdArgs(B, Ld, n_mod, _p(heads_a), _p(heads_b), _ld(hd) if hd is not None else 0,
                      _p(table), _p(site), table.shape[0] if table is not None else 0,
                      eps.data_ptr(), mu.data_ptr(), logvar.data_ptr(), z.data_ptr(), _dt(z), _ld(z))
    with stream_span("fuse_reparam_fwd", B * (8 * Ld * (n_mod - (table is not None)) + 8 * (table is not None) + 12 * Ld + z.element_size() * _ld(z))):
        L.check(L.load().mmvae_fuse_reparam_fwd(C.byref(a), _stream()), "mmvae_fuse_reparam_fwd")


# LatentEncoder: what an encoder hands to the fused latent launch instead of running its heads -- its last hidden layer's pre-BatchNorm
# output `y`, that layer's Prologue, the BatchNorm finalisation still owed (BnFinalizeArgs or None) and the heads' PreparedLinear.
LatentEncoder = namedtuple("LatentEncoder", "y prologue fin heads")


def _latent_enc(e, enc):
    sc, sh, mask, inv_keep = enc.prologue
    e.y, e.ldy, e.K = _mat(enc.y, "y").data_ptr(), _ld(enc.y), enc.heads.K
    e.scale, e.shift, e.mask, e.ld_mask, e.inv_keep = sc.data_ptr(), sh.data_ptr(), _p(mask), (_ld(mask) if mask is not None else 0), inv_keep
    if enc.fin is not None:
        e.finalize = C.addressof(enc.fin)
    e.w, e.ldw, e.bias = enc.heads.w.data_ptr(), enc.heads.w.stride(0), _p(enc.heads.bias)


def _latent_common(a, table, site, z, stem, h0):
    """The fields LatentFwdArgs and AELatentFwdArgs share -- site table, z, first decoder layer(s), h0 -- -> their HBM bytes per row."""
    if table is not None:
        a.table, a.site, a.S = table.data_ptr(), _p(site), table.shape[0]
    a.z, a.ldz = z.data_ptr(), _ld(z)
    a.w_stem, a.ldw_stem, a.bias_stem, a.N_stem = stem.w.data_ptr(), stem.w.stride(0), _p(stem.bias), stem.N
    a.h0, a.ldh0 = h0.data_ptr(), _ld(h0)
    return z.element_size() * _ld(z) + h0.element_size() * stem.N + 8 * (table is not None)


def latent_fwd_args(prec, B, Ld, enc_a, enc_b, table, site, eps, mu, logvar, z, stem, h0):
    """-> (LatentFwdArgs of mmvae_latent_fwd, its algorithmic HBM bytes).  The struct holds addresses only: the tensors and the
    encoders' BnFinalizeArgs must outlive the call."""
    a = L.LatentFwdArgs()
    a.prec, a.B, a.L = prec, B, Ld
    a.n_mod = (enc_a is not None) + (enc_b is not None) + (table is not None)
    nbytes = 12 * Ld + _latent_common(a, table, site, z, stem, h0)
    for e, enc in ((a.enc_a, enc_a), (a.enc_b, enc_b)):
        if enc is not None:
            _latent_enc(e, enc)
            nbytes += enc.heads.K * (enc.y.element_size() + (enc.prologue[2] is not None))
    a.eps, a.mu, a.logvar = eps.data_ptr(), mu.data_ptr(), logvar.data_ptr()
    return a, B * nbytes


def latent_fwd(prec, B, Ld, enc_a, enc_b, table, site, eps, mu, logvar, z, stem, h0):
    """mmvae_latent_fwd: heads of the encoders present (LatentEncoder or None), mean fusion + reparameterisation and the decoders'
    merged first layers (`stem`, a PreparedLinear; h0 = relu(z @ stem^T + b)) in ONE launch.  eps, mu and logvar are contiguous
    (B, Ld).  Raises MMVAEArgError, with nothing enqueued, for what the kernel does not take: the caller then issues the launches it
    replaces."""
    for t in (eps, mu, logvar):
        if tuple(t.shape) != (B, Ld) or not t.is_contiguous():
            raise ValueError(f"latent_fwd: eps / mu / logvar must be contiguous ({B}, {Ld}), got {tuple(t.shape)} / {t.stride()}")
    a, nbytes = latent_fwd_args(prec, B, Ld, enc_a, enc_b, table, site, eps, mu, logvar, z, stem, h0)
    with stream_span("latent.fwd", nbytes):
        L.check(L.load().mmvae_latent_fwd(C.byref(a), _stream()), "mmvae_latent_fwd")


def fuse_reparam_bwd(B, Ld, n_mod, g_mu, g_lv, dzs, eps, logvar, d_heads, d_table, site, d_heads_lp=None):
    """dzs: 1..3 fp32 (B, Ld) tensors with one leading dimension (dL/dz of each decoder); they are summed.
    d_table: zeroed [S][2L] or [copies][S][2L] (workgroups spread their scatter-adds over the copies)."""
    dzs = list(dzs) + [None] * (3 - len(dzs))
    copies = d_table.shape[0] if (d_table is not None and d_table.dim() == 3) else 1
    a = L.FuseBwdArgs(B, Ld, n_mod, _p(g_mu), _p(g_lv), dzs[0].data_ptr(), _p(dzs[1]), _p(dzs[2]), _ld(dzs[0]), eps.data_ptr(), logvar.data_ptr(),
                      d_heads.data_ptr(), _ld(d_heads), _p(d_table), _p(site), d_table.shape[-2] if d_table is not None else 0,
                      _p(d_heads_lp), _ld(d_heads_lp) if d_heads_lp is not None else 0, copies)
    n_dz = sum(1 for d in dzs if d is not None)
    with stream_span("fuse_reparam_bwd", B * Ld * 4 * (n_dz + (g_mu is not None) + (g_lv is not None) + 2 + 2)):
        L.check(L.load().mmvae_fuse_reparam_bwd(C.byref(a), _stream()), "mmvae_fuse_reparam_bwd")


def embed_proj_fwd(emb, w, b, table):
    """table (S, L) = emb (S, E) @ w (L, E)^T + b: the autoencoders' Embedding -> Linear, the one-head case of embed_table_fwd."""
    S, E = emb.shape
    L.check(L.load().mmvae_embed_proj_fwd(S, E, w.shape[0], emb.data_ptr(), w.data_ptr(), b.data_ptr(), table.data_ptr(), _stream()),
            "mmvae_embed_proj_fwd")


def embed_proj_bwd(emb, w, d_table, d_emb, d_w, d_b):
    """d_table: (S, L) or (copies, S, L) (the copies fuse_mean_bwd scattered into; summed here); d_emb, d_w, d_b are accumulated into."""
    S, E = emb.shape
    copies = d_table.shape[0] if d_table.dim() == 3 else 1
    L.check(L.load().mmvae_embed_proj_bwd(S, E, w.shape[0], emb.data_ptr(), w.data_ptr(), d_table.data_ptr(), copies,
                                          d_emb.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), _stream()), "mmvae_embed_proj_bwd")


def fuse_mean_fwd(B, Ld, head, table, site, latent, z):
    """latent (B, Ld) fp32 contiguous = the mean of the modalities present (head (B, >= Ld) fp32, the table row of site); z: the same in
    the activation type, pad columns zeroed."""
    if tuple(latent.shape) != (B, Ld) or not latent.is_contiguous() or latent.dtype != torch.float32:
        raise ValueError(f"fuse_mean_fwd: latent must be contiguous fp32 ({B}, {Ld}), got {tuple(latent.shape)} / {latent.stride()}")
    n_mod = (head is not None) + (table is not None)
    a = L.FuseMeanFwdArgs(B, Ld, n_mod, _p(head), _ld(head) if head is not None else 0,
                          _p(table), _p(site), table.shape[0] if table is not None else 0,
                          latent.data_ptr(), z.data_ptr(), _dt(z), _ld(z))
    with stream_span("fuse_mean_fwd", B * (4 * Ld * (head is not None) + 8 * (table is not None) + 4 * Ld + z.element_size() * _ld(z))):
        L.check(L.load().mmvae_fuse_mean_fwd(C.byref(a), _stream()), "mmvae_fuse_mean_fwd")


def fuse_mean_bwd(B, Ld, n_mod, dz, g_latent, d_head, d_table, site, d_head_lp=None):
    """d_head (B, >= Ld) fp32 = (dz + g_latent) / n_mod (g_latent: contiguous (B, Ld) fp32 or None), the optional bf16 copy d_head_lp, and
    the scatter-add into the zeroed d_table (S, Ld) or (copies, S, Ld) by site."""
    if g_latent is not None and (tuple(g_latent.shape) != (B, Ld) or not g_latent.is_contiguous() or g_latent.dtype != torch.float32):
        raise ValueError(f"fuse_mean_bwd: g_latent must be contiguous fp32 ({B}, {Ld})")
    copies = d_table.shape[0] if (d_table is not None and d_table.dim() == 3) else 1
    a = L.FuseMeanBwdArgs(B, Ld, n_mod, dz.data_ptr(), _ld(dz), _p(g_latent), d_head.data_ptr(), _ld(d_head),
                          _p(d_head_lp), _ld(d_head_lp) if d_head_lp is not None else 0,
                          _p(d_table), _p(site), d_table.shape[-2] if d_table is not None else 0, copies)
    with stream_span("fuse_mean_bwd", B * Ld * 4 * (2 + (g_latent is not None) + 1)):
        L.check(L.load().mmvae_fuse_mean_bwd(C.byref(a), _stream()), "mmvae_fuse_mean_bwd")


def ae_latent_fwd_args(prec, B, Ld, enc, table, site, latent, z, first, h0):
    """-> (AELatentFwdArgs of mmvae_ae_latent_fwd, its algorithmic HBM bytes).  The struct holds addresses only."""
    a = L.AELatentFwdArgs()
    a.prec, a.B, a.L = prec, B, Ld
    a.n_mod = (enc is not None) + (table is not None)
    nbytes = 4 * Ld + _latent_common(a, table, site, z, first, h0)
    if enc is not None:
        _latent_enc(a.enc, enc)
        nbytes += enc.heads.K * (enc.y.element_size() + (enc.prologue[2] is not None))
    a.latent = latent.data_ptr()
    return a, B * nbytes


def ae_latent_fwd(prec, B, Ld, enc, table, site, latent, z, first, h0):
    """mmvae_ae_latent_fwd: the head of the encoder (a LatentEncoder or None), the plain mean with the site's table row and the decoder's
    first layer (`first`, a PreparedLinear; h0 = relu(z @ first^T + b)) in ONE launch.  latent is contiguous fp32 (B, Ld).  Raises
    MMVAEArgError, with nothing enqueued, for what the kernel does not take: the caller then issues the three launches it replaces."""
    if tuple(latent.shape) != (B, Ld) or not latent.is_contiguous() or latent.dtype != torch.float32:
        raise ValueError(f"ae_latent_fwd: latent must be contiguous fp32 ({B}, {Ld}), got {tuple(latent.shape)} / {latent.stride()}")
    a, nbytes = ae_latent_fwd_args(prec, B, Ld, enc, table, site, latent, z, first, h0)
    with stream_span("ae_latent.fwd", nbytes):
        L.check(L.load().mmvae_ae_latent_fwd(C.byref(a), _stream()), "mmvae_ae_latent_fwd")


def loss_workspace(device):
    """-> (sums float64[5] zeroed, out5 float32[5]): the accumulators of mmvae_vae_loss and the tuple mmvae_loss_finalize makes of them."""
    buf = torch.zeros(5 * 8 + 5 * 4 + 4, dtype=torch.uint8, device=device)
    return buf[:40].view(torch.float64), buf[40:60].view(torch.float32)


def vae_loss(B, *, recon_a=None, a=None, recon_b=None, b=None, logits=None, site=None, class_weights=None,
             mu=None, logvar=None, beta=1e-3, gamma=1.0, sums=None, g_a=None, g_b=None, grad_b_wrt_logit=False,
             g_c=None, g_mu=None, g_lv=None, beta_gamma_dev=None):
    """sums: zeroed float64[5] (four loss sums + the count of labels outside [0, S)).  beta_gamma_dev: optional device
    float32[2] = {beta, gamma} that overrides the by-value hyper-parameters (hipGraph replays follow the beta warm-up)."""
    x = L.LossArgs()
    x.B = B
    if recon_a is not None:                 # targets a / b: fp32 or bf16 (any row stride)
        x.A, x.recon_a, x.a, x.ld_ra, x.ld_a, x.a_dtype = recon_a.shape[1], recon_a.data_ptr(), a.data_ptr(), _ld(recon_a), _ld(a), _dt(a)
    if recon_b is not None:
        x.D, x.recon_b, x.b, x.ld_rb, x.ld_b, x.b_dtype = recon_b.shape[1], recon_b.data_ptr(), b.data_ptr(), _ld(recon_b), _ld(b), _dt(b)
    if logits is not None:
        x.S, x.logits, x.ld_logits, x.site, x.class_weights = logits.shape[1], logits.data_ptr(), _ld(logits), site.data_ptr(), _p(class_weights)
    if mu is not None:
        x.L, x.mu, x.logvar = mu.shape[1], mu.data_ptr(), logvar.data_ptr()
    x.beta, x.gamma, x.sums = beta, gamma, sums.data_ptr()
    if g_a is not None:
        x.g_a, x.g_a_dtype, x.ld_ga = g_a.data_ptr(), _dt(g_a), _ld(g_a)
    if g_b is not None:
        x.g_b, x.g_b_dtype, x.ld_gb, x.grad_b_wrt_logit = g_b.data_ptr(), _dt(g_b), _ld(g_b), int(grad_b_wrt_logit)
    if g_c is not None:
        x.g_c, x.ld_gc = g_c.data_ptr(), _ld(g_c)
    x.g_mu, x.g_lv = _p(g_mu), _p(g_lv)
    x.beta_gamma_dev = _p(beta_gamma_dev)
    assert sums.dtype == torch.float64 and sums.numel() >= 5

    def nbytes():
        n = 0
        for pred, tgt, g in ((recon_a, a, g_a), (recon_b, b, g_b), (logits, None, g_c)):
            if pred is not None:
                n += B * pred.shape[1] * (4 + (4 if tgt is None else tgt.element_size())) + (0 if g is None else B * pred.shape[1] * g.element_size())
        if mu is not None:
            n += B * mu.shape[1] * 4 * (2 + (g_mu is not None) + (g_lv is not None))
        return n
    with stream_span("vae_loss", nbytes):
        L.check(L.load().mmvae_vae_loss(C.byref(x), _stream()), "mmvae_vae_loss")


def class_tail_fits(prec, S, hidden, Ld, ldh0, ldd0):
    """Would mmvae_class_tail take a class head of these shapes (and is its tuning key on)?  The library's own limits: a forward
    asks before it leaves the class decoder's last Linear to that launch."""
    return L.load().mmvae_class_tail_fits(prec, S, hidden, Ld, ldh0, ldd0) == 0


def class_tail_args(prec, B, h0, head, site, class_weights, mu, logvar, beta, gamma, sums, g_c, d0, g_mu, g_lv, beta_gamma_dev=None):
    """-> (ClassTailArgs of mmvae_class_tail, its algorithmic HBM bytes).  The struct holds addresses only."""
    a = L.ClassTailArgs()
    a.prec, a.B, a.S, a.L, a.hidden = prec, B, head.N, mu.shape[1], head.K
    a.h0, a.ldh0 = _mat(h0, "h0").data_ptr(), _ld(h0)
    a.w, a.ldw, a.wt, a.ldwt, a.bias = head.w.data_ptr(), head.w.stride(0), head.wt.data_ptr(), head.wt.stride(0), _p(head.bias)
    a.site, a.class_weights = site.data_ptr(), _p(class_weights)
    a.mu, a.logvar = mu.data_ptr(), logvar.data_ptr()
    a.beta, a.gamma, a.beta_gamma_dev, a.sums = beta, gamma, _p(beta_gamma_dev), sums.data_ptr()
    a.g_c, a.ld_gc = _mat(g_c, "g_c").data_ptr(), _ld(g_c)
    a.d0, a.ldd0 = _mat(d0, "d0").data_ptr(), _ld(d0)
    a.g_mu, a.g_lv = g_mu.data_ptr(), g_lv.data_ptr()
    # h0 slice read, d0 slice written (bf16), labels, fp32 class gradient written, mu / logvar read, their gradients written
    nbytes = B * (2 * head.K * h0.element_size() + 8 + 4 * head.N + 16 * mu.shape[1])
    return a, nbytes


def class_tail(prec, B, h0, head, site, class_weights, mu, logvar, beta, gamma, sums, g_c, d0, g_mu, g_lv, beta_gamma_dev=None):
    """mmvae_class_tail: the class decoder's last Linear (`head`, a PreparedLinear) on its hidden activation h0 (B, 64), the class +
    KL terms of vae_loss with their gradients (g_c fp32 (B, S), g_mu / g_lv) and the Linear's dX behind the ReLU mask (d0, the
    (B, 64) column slice of the merged stem gradient) in ONE launch.  mu, logvar, g_mu and g_lv are contiguous (B, L).  Raises
    MMVAEArgError, with nothing enqueued, for what the kernel does not take: the caller then issues the launches it replaces."""
    for t in (mu, logvar, g_mu, g_lv):
        if tuple(t.shape) != (B, mu.shape[1]) or not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError(f"class_tail: mu / logvar / g_mu / g_lv must be contiguous fp32 ({B}, L), got {tuple(t.shape)} / {t.stride()}")
    assert sums.dtype == torch.float64 and sums.numel() >= 5 and site.dtype == torch.int64 and site.is_contiguous()
    a, nbytes = class_tail_args(prec, B, h0, head, site, class_weights, mu, logvar, beta, gamma, sums, g_c, d0, g_mu, g_lv, beta_gamma_dev)
    with stream_span("class_tail", nbytes):
        L.check(L.load().mmvae_class_tail(C.byref(a), _stream()), "mmvae_class_tail")


GROUP_MOMENTS_MAX_G = TILE      # rows of the kernel's tile: a group must fit into one


def group_moments_fits(prec, B, G, N, K, act=ACT_NONE, with_std=False, lda=None, ldw=None):
    """Would mmvae_gemm_nt_group_moments take this shape?  The library's own limits (lda / ldw default to the padded widths)."""
    lda = ceil_to(K, 8) if lda is None else lda
    ldw = ceil_to(K, 64) if ldw is None else ldw
    return L.load().mmvae_gemm_nt_group_moments_fits(prec, B, G, N, K, act, int(with_std), lda, ldw) == 0


def gemm_nt_group_moments(prec, a, pl_w, N, K, G, mean, std=None, bias=None, act=ACT_NONE):
    """mmvae_gemm_nt_group_moments: x = act(a[B G, K] @ W[N, K]^T + bias) reduced over every G consecutive rows, on chip, to
    mean (B, N) and, if given, the unbiased std (B, N) -- both fp32 views with unit inner stride whose columns >= N stay untouched.
    a: bf16 padded rows (is_bf16_rows); pl_w: the prepared weight of a PreparedLinear.  Raises MMVAEArgError, with nothing
    enqueued, for what the kernel does not take (fp32 mode, G > 128, ...): the caller then issues gemm_nt and the reduction."""
    what = "gemm_nt_group_moments"
    a = _operand(a, "a", what, dtypes=None)
    if G < 1 or a.shape[0] % G:
        raise ValueError(f"{what}: a has {a.shape[0]} rows, not a multiple of G = {G}")
    B, dev = a.shape[0] // G, a.device
    pl_w = _operand(pl_w, "w", what, dtypes=None, dev=dev)
    mean = _operand(mean, "mean", what, dtypes=(torch.float32,), rows=B, dev=dev)
    if std is not None:
        std = _operand(std, "std", what, dtypes=(torch.float32,), rows=B, dev=dev)
    if mean.shape[1] < N or (std is not None and std.shape[1] < N) or a.shape[1] < K:
        raise ValueError(f"{what}: a needs >= {K} columns, mean / std >= {N}")
    if N < 1 or pl_w.shape[0] < ceil_to(N, TILE) or pl_w.shape[1] < K:      # the kernel reads whole 128-row tiles of W
        raise ValueError(f"{what}: w must be a prepared operand of at least ({ceil_to(max(N, 1), TILE)}, {K}), got {tuple(pl_w.shape)}")
    if a.dtype != torch.bfloat16 or pl_w.dtype != torch.bfloat16:        # the fp32 compute mode: MMVAE_ERR_DTYPE, as the library answers it
        raise L.MMVAEArgError(f"{what} failed: dtype not supported for this precision")
    g = L.GroupMomentsArgs()
    g.prec, g.B, g.G, g.N, g.K, g.act = prec, B, G, N, K, act
    g.a, g.lda = a.data_ptr(), _ld(a)
    g.w, g.ldw, g.bias = pl_w.data_ptr(), pl_w.stride(0), _p(bias)
    g.mean, g.ld_mean = mean.data_ptr(), _ld(mean)
    g.std, g.ld_std = _p(std), _ld0(std)
    with stream_span(what, B * G * K * 2 + N * K * 2 + B * N * 4 * (1 + (std is not None))):
        L.check(L.load().mmvae_gemm_nt_group_moments(C.byref(g), _stream()), "mmvae_gemm_nt_group_moments")
    return mean, std


def loss_finalize(sums, beta, gamma, out5, beta_gamma_dev=None):
    assert out5.numel() >= 5
    L.check(L.load().mmvae_loss_finalize(sums.data_ptr(), beta, gamma, _p(beta_gamma_dev), out5.data_ptr(), _stream()), "mmvae_loss_finalize")


def sigmoid_bwd(g, p, out):
    L.check(L.load().mmvae_sigmoid_bwd(g.shape[0], g.shape[1], g.data_ptr(), _ld(g), p.data_ptr(), _ld(p), out.data_ptr(),
                                       _dt(out), _ld(out), _stream()), "mmvae_sigmoid_bwd")


def scale_many(tensors, scale):
    """x *= *scale (device scalar) unless it is 1, for every tensor of the list, in one launch per 8 tensors."""
    ts = [t for t in tensors if t is not None]
    for i in range(0, len(ts), 8):
        chunk = ts[i:i + 8]
        items = (L.ScaleItem * len(chunk))(*[L.ScaleItem(t.data_ptr(), t.numel(), _dt(t), 0) for t in chunk])
        L.check(L.load().mmvae_scale_many(items, len(chunk), scale.data_ptr(), _stream()), "mmvae_scale_many")


def scale_if_needed(x, scale):
    L.check(L.load().mmvae_scale_if_needed(x.data_ptr(), _dt(x), x.numel(), scale.data_ptr(), _stream()), "mmvae_scale_if_needed")


def noise(mask, eps, keep_prob, seed, offset, offset_dev=None, advance=False):
    """Fill `mask` (uint8, any shape, contiguous; may be None) and `eps` (fp32; may be None) from the Philox stream
    (seed, offset [+ *offset_dev]).  Returns the number of counter values consumed.  advance=True: offset_dev is an
    int64[CTR_COPIES] tensor of identical copies of the counter and the launch itself moves them past what it consumed."""
    n_mask = 0 if mask is None else mask.numel()
    n_eps = 0 if eps is None else eps.numel()
    if advance:
        assert offset_dev is not None and offset_dev.numel() == L.CTR_COPIES and offset_dev.dtype == torch.int64
    with stream_span("noise", n_mask + 4 * n_eps):
        L.check(L.load().mmvae_noise(_p(mask), n_mask, keep_prob, _p(eps), n_eps, seed, offset, _p(offset_dev), int(advance), _stream()), "mmvae_noise")
    return (n_mask + 15) // 16 * 4 + (n_eps + 3) // 4


def step_head(noise_args=None, prep=None, zero=(), table_args=None):
    """mmvae_step_head: the four independent launches a training forward begins with, as one.  noise_args: noise()'s positional
    arguments (mask, eps, keep_prob, seed, offset, offset_dev, advance); prep: a WeightPrep; zero: uint8 tensors to fill with zeros
    (16-byte aligned, a multiple of 16 bytes each); table_args: embed_table_fwd()'s arguments.  Any of them may be absent.  Raises
    MMVAEArgError, with nothing enqueued, where the library refuses: the caller then issues the four launches."""
    a = L.StepHeadArgs()
    nbytes = 0
    if noise_args is not None:
        mask, eps, keep_prob, seed, offset, offset_dev, advance = noise_args
        a.mask, a.n_mask = _p(mask), 0 if mask is None else mask.numel()
        a.eps, a.n_eps = _p(eps), 0 if eps is None else eps.numel()
        if advance:
            assert offset_dev is not None and offset_dev.numel() == L.CTR_COPIES and offset_dev.dtype == torch.int64
        a.keep_prob, a.seed, a.offset, a.offset_dev, a.advance = keep_prob, seed, offset, _p(offset_dev), int(advance)
        nbytes += a.n_mask + 4 * a.n_eps
    if prep is not None:
        a.prep_items, a.n_prep = prep.table.data_ptr(), prep.n
        nbytes += prep.nbytes()
    zero = [z for z in zero if z is not None and z.numel()]
    if len(zero) > L.HEAD_ZERO_MAX:
        raise L.MMVAEArgError(f"step_head: more than {L.HEAD_ZERO_MAX} zero ranges")
    a.n_zero = len(zero)
    for k, z in enumerate(zero):
        assert z.is_contiguous()
        a.zero_ptr[k], a.zero_bytes[k] = z.data_ptr(), z.numel() * z.element_size()
        nbytes += a.zero_bytes[k]
    if table_args is not None:
        emb, w_mu, b_mu, w_lv, b_lv, table = table_args
        a.S, a.E, a.L = emb.shape[0], emb.shape[1], w_mu.shape[0]
        a.emb, a.w_mu, a.b_mu, a.w_lv, a.b_lv, a.table = (t.data_ptr() for t in table_args)
        nbytes += 4 * (emb.numel() + w_mu.numel() + w_lv.numel() + b_mu.numel() + b_lv.numel() + table.numel())
    with stream_span("step_head", nbytes):
        L.check(L.load().mmvae_step_head(C.byref(a), _stream()), "mmvae_step_head")


def dropout_mask(mask, keep_prob, seed, offset):
    return noise(mask, None, keep_prob, seed, offset)


def randn(out, seed, offset):
    return noise(None, out, 1.0, seed, offset)


def counter_add(counter, inc):
    L.check(L.load().mmvae_counter_add(counter.data_ptr(), inc, _stream()), "mmvae_counter_add")


def _gather_row(t):
    """(row stride in bytes, bytes to move per row) of a gather operand: contiguous, or a (N, F) row-strided view with unit inner
    stride -- padded bf16 rows move WHOLE padded rows (their pads are zeros on both sides), other views their F elements."""
    es = t.element_size()
    if t.is_contiguous():
        n = t[0].numel() * es if t.dim() > 1 else es
        return n, n
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        if is_bf16_rows(t) and t.untyped_storage().nbytes() >= (t.storage_offset() + t.shape[0] * t.stride(0)) * es:
            return t.stride(0) * es, ceil_to(t.shape[1], 8) * es
        return t.stride(0) * es, t.shape[1] * es
    raise ValueError(f"gather_rows: need contiguous tensors or (N, F) row-strided views, got {tuple(t.shape)} / {t.stride()}")


def gather_rows(pairs, idx, src_rows):
    """pairs: [(src (N, ...) row-major, dst (B, ...))]: dst[i] = src[idx[i]] for every pair in ONE launch (idx: int64 (B,) on the
    device).  The minibatch assembly of a device-resident dataset (reference: Dataset.__getitem__ + default collate per sample).
    2-D operands may be row-strided views (stride(1) == 1); a padded-bf16-rows pair copies whole padded rows, so the pads stay zero."""
    items = (L.GatherItem * len(pairs))()
    B = idx.shape[0]
    nbytes = 0
    for j, (src, dst) in enumerate(pairs):
        if src.dtype != dst.dtype or src.shape[1:] != dst.shape[1:] or dst.shape[0] != B or src.shape[0] != src_rows:
            raise ValueError(f"gather_rows: pair {j}: {tuple(src.shape)} {src.dtype} -> {tuple(dst.shape)} {dst.dtype}")
        if not (src.is_cuda and dst.is_cuda):
            raise ValueError("gather_rows needs device tensors")
        (s_ld, s_row), (d_ld, d_row) = _gather_row(src), _gather_row(dst)
        row = min(s_row, d_row)                 # a padded pair: both move ceil8(F) elements; a padded side with a plain one: F elements
        items[j] = L.GatherItem(src.data_ptr(), dst.data_ptr(), s_ld, d_ld, row, 0)
        nbytes += 2 * B * row
    if idx.dtype != torch.int64 or not idx.is_cuda or not idx.is_contiguous():
        raise ValueError("gather_rows: idx must be a contiguous int64 device tensor")
    with stream_span("gather_rows", nbytes):
        L.check(L.load().mmvae_gather_rows(C.cast(items, C.c_void_p), len(pairs), idx.data_ptr(), B, src_rows, _stream()), "mmvae_gather_rows")


def recon_metrics(pred, target, col_shift, col_acc, row_pearson, row_cosine):
    """One streaming pass over (prediction, target) (mmvae_recon_metrics): row_pearson / row_cosine (fp32 (M,)) are written,
    col_acc (float64 (4, N): sum (y - c), sum (y - c)^2, sum (p - y)^2, sum |p - y| per column, c = col_shift or 0) is ACCUMULATED
    into -- zero it once per evaluation.  target: (M, N) fp32 or bf16, unit inner stride, any row stride (padded bf16 rows included);
    pred: the same, or a 1-D (N,) tensor = one prediction row for every sample."""
    _mat(target, "target")
    M, N = target.shape
    if M < 1 or N < 1:
        raise ValueError(f"recon_metrics: empty target {tuple(target.shape)}")
    t_dt, t_ld = _dt(_operand(target, "target", "recon_metrics", dtypes=None)), _ld(target)
    if pred.dim() == 1:
        if not pred.is_cuda or pred.shape[0] != N or pred.stride(0) != 1:
            raise ValueError(f"recon_metrics: a broadcast prediction must be a contiguous ({N},) device tensor, got {tuple(pred.shape)}")
        p_dt, p_ld, p_rows = _dt(pred), 0, 1
    else:
        _mat(pred, "pred")                       # a host tensor is a ValueError here, as for the target
        p_dt, p_ld, p_rows = _dt(_operand(pred, "pred", "recon_metrics", dtypes=None, rows=M, cols=N)), _ld(pred), M
    for t, name, dt, shape in ((col_shift, "col_shift", torch.float32, (N,)), (col_acc, "col_acc", torch.float64, (4, N)),
                               (row_pearson, "row_pearson", torch.float32, (M,)), (row_cosine, "row_cosine", torch.float32, (M,))):
        if t is None and name == "col_shift":
            continue
        if not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"recon_metrics: {name} must be a contiguous {dt} device tensor of shape {shape}")
    if len({t.device for t in (pred, target, col_acc, row_pearson, row_cosine)} | ({col_shift.device} if col_shift is not None else set())) != 1:
        raise ValueError("recon_metrics: all operands must live on one device")
    a = L.MetricsArgs(M, N, pred.data_ptr(), p_dt, p_ld, target.data_ptr(), t_dt, t_ld, _p(col_shift), col_acc.data_ptr(), row_pearson.data_ptr(),
                      row_cosine.data_ptr())
    nbytes = M * N * target.element_size() + p_rows * N * pred.element_size() + 8 * M + 2 * 32 * N + (4 * N if col_shift is not None else 0)
    with stream_span("recon_metrics", nbytes):
        L.check(L.load().mmvae_recon_metrics(C.byref(a), _stream()), "mmvae_recon_metrics")


# --------------------------------------------------------------------------------------------
# what the evaluation wrappers (recon_metrics above, k-NN, silhouette, PCA, t-SNE and the site classifier below) share: ONE in-place
# operand check, and the vector, output and workspace checks
# --------------------------------------------------------------------------------------------
def _operand(t, name, what, *, dtypes=(torch.float32, torch.bfloat16), rows=None, cols=None, dev=None, align=0, ld_multiple=0, contiguous=False):
    """t, if it is a device matrix a kernel can read or write IN PLACE: 2-D, at least 1 x 1, unit inner stride, rows that do not overlap,
    a dtype among `dtypes` (None: left to the caller's _dt and its TypeError), and as asked: exactly `rows` / `cols`, on `dev`, the base
    address a multiple of `align` bytes, the row stride a multiple of `ld_multiple` elements, contiguous.  Anything else is refused; the
    caller takes data_ptr(), _dt() and _ld() of what comes back."""
    _no_cpu(t, name, what)
    if (t.dim() != 2 or (dtypes is not None and t.dtype not in dtypes) or t.shape[0] < 1 or t.shape[1] < 1 or t.stride(1) != 1
            or (t.shape[0] > 1 and t.stride(0) < t.shape[1]) or (rows is not None and t.shape[0] != rows)
            or (cols is not None and t.shape[1] != cols) or (dev is not None and t.device != dev) or (align and t.data_ptr() % align)
            or (ld_multiple and _ld(t) % ld_multiple) or (contiguous and not t.is_contiguous())):
        need = [f"({'rows >= 1' if rows is None else rows}, {'cols >= 1' if cols is None else cols}) matrix"
                + ("" if dtypes is None else " of " + " / ".join(str(d) for d in dtypes)),
                "contiguous" if contiguous else "unit inner stride, rows that do not overlap"]
        need += ["on the operands' device"] * (dev is not None) + [f"{align}-byte aligned"] * bool(align)
        need += [f"row stride a multiple of {ld_multiple}"] * bool(ld_multiple)
        raise ValueError(f"{what}: {name} must be a {', '.join(need)}; got {tuple(t.shape)} {t.dtype} / {t.stride()}")
    return t


def _vector(t, name, what, dt, n, dev, strided=False):
    """t, a `dt` (n,) tensor on `dev`: contiguous, or (strided) a view with unit stride"""
    ok = isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and tuple(t.shape) == (n,) and t.device == dev
    if ok and strided:
        ok = n <= 1 or t.stride(0) == 1
    elif ok:
        ok = t.is_contiguous()
    if not ok:
        raise ValueError(f"{what}: {name} must be a {'' if strided else 'contiguous '}{dt} ({n},) tensor on the operand's device")
    return t


def _shift(shift, what, F, dev):
    return None if shift is None else _vector(shift, "shift", what, torch.float32, F, dev)


def _out_view(out, name, what, dt, rows, cols, dev):
    """`out`, a `dt` (rows, cols) tensor on `dev` with unit inner stride (a view is allowed), or a new one"""
    if out is None:
        return torch.empty(rows, cols, dtype=dt, device=dev)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != dt or tuple(out.shape) != (rows, cols) or out.stride(1) != 1 \
            or (rows > 1 and out.stride(0) < cols) or out.device != dev:
        raise ValueError(f"{what}: {name} must be a {dt} ({rows}, {cols}) tensor on the operand's device with unit inner stride")
    return out


def _out_vector(out, name, what, dt, n, dev, strided=False):
    """`out`, a `dt` (n,) tensor on `dev` as _vector checks it, or a new one"""
    return torch.empty(n, dtype=dt, device=dev) if out is None else _vector(out, name, what, dt, n, dev, strided)


def _ld0(t):
    return 0 if t is None else _ld(t)


def _workspace(nbytes, dev):
    """8-byte aligned device scratch of at least nbytes; None for 0"""
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev) if nbytes else None


def _work(work, nbytes, what, dev):
    """The caller's workspace if it is a contiguous int64 tensor of at least nbytes on `dev`, or a new one (None for 0 bytes)"""
    if work is None:
        return _workspace(nbytes, dev)
    if not isinstance(work, torch.Tensor) or work.dtype != torch.int64 or not work.is_contiguous() or work.numel() * 8 < nbytes or work.device != dev:
        raise ValueError(f"{what}: work must be a contiguous int64 tensor of at least {nbytes} bytes on the operand's device")
    return work


def _plan(symbol, *args, outs=(C.c_int32,)):
    """The answer(s) of a planning entry point (`*_splits`, `*_work_bytes`: sizes in, integers out; needs no device)."""
    vals = [t(0) for t in outs]
    L.check(getattr(L.load(), symbol)(*args, *(C.byref(v) for v in vals)), symbol)
    return vals[0].value if len(vals) == 1 else tuple(v.value for v in vals)


def _splits_arg(splits, what):
    splits = int(splits)
    if not 0 <= splits <= 64:
        raise ValueError(f"{what}: splits = {splits} outside [0, 64]")
    return splits


# --------------------------------------------------------------------------------------------
# k nearest neighbours (include/mmvae_hip.h: mmvae_knn_search, mmvae_knn_mean_rows)
# --------------------------------------------------------------------------------------------
def knn_splits(Mq, Nt):
    """(splits, training rows per split) of the decomposition knn_search uses for these sizes (mmvae_knn_splits); needs no device."""
    return _plan("mmvae_knn_splits", Mq, Nt, outs=(C.c_int32, C.c_int32))


def knn_work_bytes(Mq, Nt, k):
    return _plan("mmvae_knn_work_bytes", Mq, Nt, k, outs=(C.c_int64,))


def knn_l1_work_bytes(Mq, Nt, k):
    return _plan("mmvae_knn_l1_work_bytes", Mq, Nt, k, outs=(C.c_int64,))


def _knn_search(what, work_bytes, kind, q, t, k, shift, idx_out, dist_out, dist_name, work):
    """The one body of knn_search and knn_search_l1: entry point mmvae_<what>, workspace size work_bytes(Mq, Nt, k), probe kind `kind`;
    dist_out is False for no distances, else the caller's `dist_name` or None; work: the caller's workspace or None."""
    _operand(q, "q", what)
    Mq, F = q.shape
    _operand(t, "t", what, cols=F)
    Nt = t.shape[0]
    k = int(k)
    if not 1 <= k <= min(Nt, L.KNN_MAXK):
        raise ValueError(f"{what}: k = {k} outside [1, min({Nt} training rows, {L.KNN_MAXK})]")
    if t.device != q.device:
        raise ValueError(f"{what}: all operands must live on one device")
    shift = _shift(shift, what, F, q.device)
    idx = _out_view(idx_out, "idx_out", what, torch.int32, Mq, k, q.device)
    d = None if dist_out is False else _out_view(dist_out, dist_name, what, torch.float32, Mq, k, q.device)
    work = _work(work, work_bytes(Mq, Nt, k), what, q.device)
    a = L.KnnArgs(q.data_ptr(), t.data_ptr(), _p(shift), idx.data_ptr(), _p(d), _p(work), _ld(q), _ld(t), _ld(idx), _ld0(d),
                  work.numel() * 8 if work is not None else 0, Mq, Nt, F, k, _dt(q), _dt(t))
    with probe_span(what, lambda: dict(kind=kind, flops=2.0 * Mq * Nt * F, M=Mq, N=Nt, K=F)):
        L.check(getattr(L.load(), "mmvae_" + what)(C.byref(a), _stream()), "mmvae_" + what)
    return idx, d


def knn_search(q, t, k, shift=None, dist2=True, *, idx_out=None, dist2_out=None, work=None):
    """The k nearest training rows (euclidean) of every query row (mmvae_knn_search): idx int32 (Mq, k) ascending by (distance key,
    training index), and the squared distances fp32 (Mq, k) unless dist2 is False (then None).  q (Mq, F), t (Nt, F): fp32 or bf16,
    unit inner stride, any row stride (padded bf16 rows included).  shift (F,) fp32 is subtracted from both operands on load (pass the
    training column means: the distances do not change, their rounding does).  idx_out / dist2_out: write into these (views allowed).
    work: a workspace to use (an int64 tensor of at least knn_work_bytes(Mq, Nt, k) bytes, any contents)."""
    return _knn_search("knn_search", knn_work_bytes, "gemm", q, t, k, shift, idx_out, dist2_out if dist2 else False, "dist2_out", work)


def knn_search_l1(q, t, k, dist=True, *, idx_out=None, dist_out=None, work=None):
    """The k nearest training rows of every query row under the manhattan distance (mmvae_knn_search_l1): idx int32 (Mq, k) ascending
    by (distance, training index), and the L1 distances themselves -- not squared -- fp32 (Mq, k) unless dist is False (then None).
    Every distance is one fp32 chain of |q - t| over the columns in ascending order.  Operands as knn_search; there is no shift.
    work: a workspace to use (an int64 tensor of at least knn_l1_work_bytes(Mq, Nt, k) bytes, any contents)."""
    return _knn_search("knn_search_l1", knn_l1_work_bytes, "valu", q, t, k, None, idx_out, dist_out if dist else False, "dist_out", work)


_KNN_METRICS = {"euclidean": 0, "manhattan": 1}


def knn_group_work_bytes(Mq, Nt, k, metric="euclidean"):
    """Workspace bytes of knn_search_grouped (mmvae_knn_group_work_bytes): the ungrouped size of the metric + 16 per tile of 128 rows."""
    if metric not in _KNN_METRICS:
        raise ValueError(f"knn_group_work_bytes: metric must be one of {sorted(_KNN_METRICS)}, got {metric!r}")
    return _plan("mmvae_knn_group_work_bytes", Mq, Nt, k, _KNN_METRICS[metric], outs=(C.c_int64,))


def knn_search_grouped(q, t, k, *, same=None, differ=None, metric="euclidean", shift=None, dist=True, idx_out=None, dist_out=None, work=None):
    """knn_search (metric "euclidean": squared distances) or knn_search_l1 ("manhattan": the distances themselves) among the candidates
    a query may see (mmvae_knn_search_grouped): same = (q_codes, t_codes) admits the candidates whose code equals the query's, differ =
    (q_codes, t_codes) those whose code differs; both may be given, one must be.  Codes are int32 device vectors of Mq and Nt entries.
    Among the admitted candidates the result is, bit for bit, that of the plain search over them.  A query with c < k admitted candidates
    gets c entries and then idx -1 / distance +inf.  Rows sorted by the `same` code let whole tiles be skipped.  There is no CPU fallback.
    work: a workspace to use (an int64 tensor of at least knn_group_work_bytes(Mq, Nt, k, metric) bytes, any contents)."""
    what = "knn_search_grouped"
    if metric not in _KNN_METRICS:
        raise ValueError(f"{what}: metric must be one of {sorted(_KNN_METRICS)}, got {metric!r}")
    if same is None and differ is None:
        raise ValueError(f"{what}: give same=(q_codes, t_codes), differ=(q_codes, t_codes) or both; without codes use knn_search / knn_search_l1")
    if metric == "manhattan" and shift is not None:
        raise ValueError(f"{what}: the manhattan search takes no shift")
    _operand(q, "q", what)
    Mq, F = q.shape
    _operand(t, "t", what, cols=F)
    Nt = t.shape[0]
    k = int(k)
    if not 1 <= k <= min(Nt, L.KNN_MAXK):
        raise ValueError(f"{what}: k = {k} outside [1, min({Nt} training rows, {L.KNN_MAXK})]")
    if t.device != q.device:
        raise ValueError(f"{what}: all operands must live on one device")
    codes = []
    for name, pair in (("same", same), ("differ", differ)):
        if pair is None:
            codes += [None, None]
            continue
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError(f"{what}: {name} must be a (q_codes, t_codes) pair")
        codes += [_vector(pair[0], f"{name}[0]", what, torch.int32, Mq, q.device), _vector(pair[1], f"{name}[1]", what, torch.int32, Nt, q.device)]
    shift = _shift(shift, what, F, q.device)
    idx = _out_view(idx_out, "idx_out", what, torch.int32, Mq, k, q.device)
    d = None if dist is False else _out_view(dist_out, "dist_out", what, torch.float32, Mq, k, q.device)
    work = _work(work, knn_group_work_bytes(Mq, Nt, k, metric), what, q.device)
    base = L.KnnArgs(q.data_ptr(), t.data_ptr(), _p(shift), idx.data_ptr(), _p(d), _p(work), _ld(q), _ld(t), _ld(idx), _ld0(d),
                     work.numel() * 8, Mq, Nt, F, k, _dt(q), _dt(t))
    a = L.KnnGroupArgs(base, *(_p(c) for c in codes), _KNN_METRICS[metric])
    with probe_span(what, lambda: dict(kind="valu" if metric == "manhattan" else "gemm", flops=2.0 * Mq * Nt * F, M=Mq, N=Nt, K=F)):
        L.check(L.load().mmvae_knn_search_grouped(C.byref(a), _stream()), "mmvae_knn_search_grouped")
    return idx, d


def _knn_idx(idx, what):
    """(Mq, k) of idx, the int32 (Mq, 1 <= k <= KNN_MAXK) neighbour lists of a search (the first k columns of a wider one are allowed)"""
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 2 or idx.stride(1) != 1 or idx.shape[0] < 1 \
            or not 1 <= idx.shape[1] <= L.KNN_MAXK:
        raise ValueError(f"{what}: idx must be an int32 (Mq, 1 <= k <= {L.KNN_MAXK}) device tensor with unit inner stride")
    return idx.shape


def knn_mean_rows(idx, y, out=None):
    """out[i] = mean over n of y[idx[i][n]] in fp32, summed in ascending n (mmvae_knn_mean_rows): uniform k-NN regression.
    idx int32 (Mq, k), y (Ny, Fy) fp32 or bf16, out fp32 (Mq, Fy); indices outside [0, Ny) are clamped."""
    _operand(y, "y", "knn_mean_rows")
    Mq, k = _knn_idx(idx, "knn_mean_rows")
    Ny, Fy = y.shape
    if idx.device != y.device:
        raise ValueError("knn_mean_rows: all operands must live on one device")
    out = _out_view(out, "out", "knn_mean_rows", torch.float32, Mq, Fy, y.device)
    with stream_span("knn_mean_rows", Mq * k * (4 + Fy * y.element_size()) + 4 * Mq * Fy):
        L.check(L.load().mmvae_knn_mean_rows(idx.data_ptr(), _ld(idx), y.data_ptr(), _dt(y), _ld(y), out.data_ptr(), _ld(out), Mq, k, Ny, Fy,
                                             _stream()), "mmvae_knn_mean_rows")
    return out


def knn_weighted_rows(idx, dist, y, squared, out=None):
    """out[i] = sum_n w_n y[idx[i][n]] / sum_n w_n in fp32 with sklearn's weights='distance' (mmvae_knn_weighted_rows): w = 1 / d, or
    the indicator of d == 0 where a row has zero distances; d = dist, or sqrt(dist) when `squared` (the dist2 of knn_search).
    idx int32 (Mq, k) and dist fp32 (Mq, k) may be the first k columns of a wider search; y (Ny, Fy) fp32 or bf16, out fp32 (Mq, Fy)."""
    _operand(y, "y", "knn_weighted_rows")
    Mq, k = _knn_idx(idx, "knn_weighted_rows")
    if not isinstance(dist, torch.Tensor) or not dist.is_cuda or dist.dtype != torch.float32 or tuple(dist.shape) != (Mq, k) or dist.stride(1) != 1:
        raise ValueError(f"knn_weighted_rows: dist must be a float32 ({Mq}, {k}) device tensor with unit inner stride")
    Ny, Fy = y.shape
    if idx.device != y.device or dist.device != y.device:
        raise ValueError("knn_weighted_rows: all operands must live on one device")
    out = _out_view(out, "out", "knn_weighted_rows", torch.float32, Mq, Fy, y.device)
    with stream_span("knn_weighted_rows", Mq * k * (8 + Fy * y.element_size()) + 4 * Mq * Fy):
        L.check(L.load().mmvae_knn_weighted_rows(idx.data_ptr(), _ld(idx), dist.data_ptr(), _ld(dist), 1 if squared else 0, y.data_ptr(), _dt(y),
                                                 _ld(y), out.data_ptr(), _ld(out), Mq, k, Ny, Fy, _stream()), "mmvae_knn_weighted_rows")
    return out


# --------------------------------------------------------------------------------------------
# silhouette coefficient (include/mmvae_hip.h: mmvae_silhouette_samples)
# --------------------------------------------------------------------------------------------
def silhouette_splits(N, n_classes, splits=0):
    """The number of column splits silhouette_samples uses for these sizes and this request (mmvae_silhouette_splits); needs no device."""
    return _plan("mmvae_silhouette_splits", N, n_classes, splits)


def silhouette_work_bytes(N, n_classes, splits=0):
    return _plan("mmvae_silhouette_work_bytes", N, n_classes, splits, outs=(C.c_int64,))


def silhouette_samples(x, order, class_start, shift=None, *, splits=0, s_out=None, intra_out=None, inter_out=None, work=None):
    """Silhouette coefficient of every row of x (mmvae_silhouette_samples): (s, intra, inter), fp32 (N,) each in x's row order.
    x (N, F): fp32 or bf16, unit inner stride, any row stride (padded bf16 rows included).  order: int32 (N,) row indices grouped by
    class, or None when the rows are already grouped; class_start: int32 (C + 1,) positions, class c owns order[class_start[c] :
    class_start[c + 1]].  shift (F,) fp32 is subtracted from every element on load (pass the column means).  splits: 0 = the library's
    choice, 1 .. 64 forces that many column splits.  *_out: write into these (views allowed).  work: a workspace to use (an int64 tensor
    of at least silhouette_work_bytes(N, C, splits) bytes, any contents)."""
    what = "silhouette_samples"
    _operand(x, "x", what)
    N, F = x.shape
    dev = x.device
    if not isinstance(class_start, torch.Tensor) or class_start.dim() != 1:
        raise ValueError("silhouette_samples: class_start must be an int32 (C + 1,) device tensor")
    nc = class_start.shape[0] - 1
    if N < 2 or not 1 <= nc <= L.SIL_MAXC:
        raise ValueError(f"silhouette_samples: N = {N}, C = {nc} outside N >= 2, 1 <= C <= {L.SIL_MAXC}")
    _vector(class_start, "class_start", what, torch.int32, nc + 1, dev)
    if order is not None:
        _vector(order, "order", what, torch.int32, N, dev)
    shift = _shift(shift, what, F, dev)
    splits = _splits_arg(splits, what)
    outs = [_out_vector(o, name, what, torch.float32, N, dev, strided=True) for o, name in ((s_out, "s_out"), (intra_out, "intra_out"), (inter_out, "inter_out"))]
    work = _work(work, silhouette_work_bytes(N, nc, splits), what, dev)
    a = L.SilhouetteArgs(x.data_ptr(), _p(shift), _p(order), class_start.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                         work.data_ptr(), _ld(x), work.numel() * 8, N, F, nc, splits, _dt(x), 0)
    with probe_span("silhouette_samples", lambda: dict(kind="gemm", flops=2.0 * N * N * F, M=N, N=N, K=F)):
        L.check(L.load().mmvae_silhouette_samples(C.byref(a), _stream()), "mmvae_silhouette_samples")
    return tuple(outs)


# --------------------------------------------------------------------------------------------
# PCA: centred scatter matrix and projection (include/mmvae_hip.h: mmvae_pca_scatter, mmvae_pca_project)
# --------------------------------------------------------------------------------------------
def pca_scatter_splits(N, F, splits=0):
    """The number of row splits pca_scatter uses for these sizes and this request (mmvae_pca_scatter_splits); needs no device."""
    return _plan("mmvae_pca_scatter_splits", N, F, splits)


def pca_scatter_work_bytes(N, F, splits=0):
    return _plan("mmvae_pca_scatter_work_bytes", N, F, splits, outs=(C.c_int64,))


def pca_scatter(x, shift, splits=0, out=None, *, work=None):
    """S = (x - shift)^T (x - shift), fp32 (F, F), bitwise symmetric (mmvae_pca_scatter).  x (N, F): fp32 or bf16, unit inner stride, any
    row stride (padded bf16 rows included); shift (F,) fp32 or None is subtracted from every element on load (pass the column means).
    splits: 0 = the library's choice, 1 .. 64 forces that many row splits.  out: write into this (a view is allowed).  work: a workspace
    to use (an int64 tensor of at least pca_scatter_work_bytes(N, F, splits) bytes, any contents)."""
    _operand(x, "x", "pca_scatter")
    N, F = x.shape
    shift = _shift(shift, "pca_scatter", F, x.device)
    splits = _splits_arg(splits, "pca_scatter")
    s = _out_view(out, "out", "pca_scatter", torch.float32, F, F, x.device)
    nbytes = pca_scatter_work_bytes(N, F, splits)
    work = _work(work, nbytes, "pca_scatter", x.device)
    a = L.PcaScatterArgs(x.data_ptr(), _p(shift), s.data_ptr(), _p(work), _ld(x), _ld(s), work.numel() * 8 if work is not None else 0, N, F, splits, _dt(x))
    with probe_span("pca_scatter", lambda: dict(kind="gemm", flops=1.0 * N * F * F, M=F, N=F, K=N)):
        L.check(L.load().mmvae_pca_scatter(C.byref(a), _stream()), "mmvae_pca_scatter")
    return s


def pca_project(x, shift, v, out=None):
    """y = (x - shift) v^T, fp32 (N, k) (mmvae_pca_project).  x, shift as pca_scatter; v (k, F) fp32 with unit inner stride,
    1 <= k <= PCA_MAXK.  A row of y depends on that row of x, shift and v alone."""
    _operand(x, "x", "pca_project")
    N, F = x.shape
    shift = _shift(shift, "pca_project", F, x.device)
    k = _operand(v, "v", "pca_project", dtypes=(torch.float32,), cols=F, dev=x.device).shape[0]
    if k > L.PCA_MAXK:
        raise ValueError(f"pca_project: v has {k} rows, more than {L.PCA_MAXK}")
    y = _out_view(out, "out", "pca_project", torch.float32, N, k, x.device)
    a = L.PcaProjectArgs(x.data_ptr(), _p(shift), v.data_ptr(), y.data_ptr(), _ld(x), _ld(v), _ld(y), N, F, k, _dt(x))
    with probe_span("pca_project", lambda: dict(kind="gemm", flops=2.0 * N * F * k, M=N, N=k, K=F)):
        L.check(L.load().mmvae_pca_project(C.byref(a), _stream()), "mmvae_pca_project")
    return y


# --------------------------------------------------------------------------------------------
# StandardScaler on column blocks (include/mmvae_hip.h: mmvae_standardize_fit, mmvae_standardize_apply)
# --------------------------------------------------------------------------------------------
def standardize_fit_splits(rows, F, splits=0):
    """The number of row splits standardize_fit uses for these sizes and this request (mmvae_standardize_fit_splits); needs no device."""
    return _plan("mmvae_standardize_fit_splits", rows, F, splits)


def standardize_fit_work_bytes(rows, F, splits=0):
    return _plan("mmvae_standardize_fit_work_bytes", rows, F, splits, outs=(C.c_int64,))


def _std_parts(parts, what, rows=None):
    """(parts, rows, F, device, bytes read) of a feature matrix given as column blocks: one tensor or a sequence of 1 .. STD_MAX_PARTS,
    each a 2-D fp32 / bf16 device matrix (checked with _operand) or a 1-D tensor: one row that stands for every sample."""
    if isinstance(parts, torch.Tensor):
        parts = (parts,)
    parts = tuple(parts)
    if not 1 <= len(parts) <= L.STD_MAX_PARTS:
        raise ValueError(f"{what}: {len(parts)} parts, need 1 .. {L.STD_MAX_PARTS}")
    dev = None
    for i, t in enumerate(parts):
        _no_cpu(t, f"parts[{i}]", what)
        dev = t.device if dev is None else dev
        if t.dim() == 1:
            if t.dtype not in (torch.float32, torch.bfloat16) or t.shape[0] < 1 or (t.shape[0] > 1 and t.stride(0) != 1) or t.device != dev:
                raise ValueError(f"{what}: parts[{i}] (one row) must be a fp32 / bf16 (cols >= 1,) tensor with unit stride on the operands' "
                                 f"device; got {tuple(t.shape)} {t.dtype} / {t.stride()}")
        else:
            _operand(t, f"parts[{i}]", what, rows=rows, dev=dev)
            rows = t.shape[0]
    if rows is None:
        raise ValueError(f"{what}: every part is one row: the row count must come from a matrix part or from rows=")
    F = sum(t.shape[-1] for t in parts)
    nbytes = sum((1 if t.dim() == 1 else rows) * t.shape[-1] * t.element_size() for t in parts)
    return parts, int(rows), F, dev, nbytes


def _std_fill(a, parts):
    for i, t in enumerate(parts):
        a.part[i] = L.StdPart(t.data_ptr(), 0 if t.dim() == 1 else _ld(t), t.shape[-1], _dt(t), int(t.dim() == 1), 0)
    a.n_parts = len(parts)


def standardize_fit(parts, *, splits=0, mean_out=None, var_out=None, scale_out=None, work=None):
    """StandardScaler().fit of the matrix whose column blocks are `parts` (mmvae_standardize_fit): (mean, var, scale), float64 (F,) each.
    parts: see _std_parts; at least one is a matrix.  splits: 0 = the library's choice, 1 .. 64 forces that many row splits.  *_out:
    write into these.  work: a workspace to use (an int64 tensor of at least standardize_fit_work_bytes(rows, F, splits) bytes, any
    contents)."""
    what = "standardize_fit"
    parts, rows, F, dev, nbytes = _std_parts(parts, what)
    if all(t.dim() == 1 for t in parts):
        raise ValueError(f"{what}: every part is one row: at least one matrix part is required")
    splits = _splits_arg(splits, what)
    outs = [_out_vector(o, name, what, torch.float64, F, dev) for o, name in ((mean_out, "mean_out"), (var_out, "var_out"), (scale_out, "scale_out"))]
    work = _work(work, standardize_fit_work_bytes(rows, F, splits), what, dev)
    a = L.StandardizeFitArgs()
    _std_fill(a, parts)
    a.mean, a.var, a.scale, a.work, a.work_bytes = outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), work.data_ptr(), work.numel() * 8
    a.rows, a.splits = rows, splits
    with stream_span("standardize_fit", nbytes + 24 * F):
        L.check(L.load().mmvae_standardize_fit(C.byref(a), _stream()), "mmvae_standardize_fit")
    return tuple(outs)


def standardize_apply(parts, mean, scale, *, rows=None, out=None):
    """StandardScaler.transform of the matrix whose column blocks are `parts` (mmvae_standardize_apply): z = (float)(((double)x - mean) /
    scale), fp32 (rows, F).  mean, scale: float64 (F,), from any fit.  rows: only where every part is one row.  out: write into this
    (a view with a row stride >= F is allowed; its other columns are not written); it may not share STORAGE with a part: the refusal
    compares the storages, not the extents, so disjoint views of one buffer are refused too (an `out` allocated here shares nothing)."""
    what = "standardize_apply"
    parts, rows, F, dev, nbytes = _std_parts(parts, what, rows)
    mean = _vector(mean, "mean", what, torch.float64, F, dev)
    scale = _vector(scale, "scale", what, torch.float64, F, dev)
    z = _out_view(out, "out", what, torch.float32, rows, F, dev)
    if out is not None and any(t.untyped_storage().data_ptr() == z.untyped_storage().data_ptr() for t in parts):
        raise ValueError(f"{what}: out shares its storage with a part")
    a = L.StandardizeApplyArgs()
    _std_fill(a, parts)
    a.mean, a.scale, a.z, a.ldz, a.rows = mean.data_ptr(), scale.data_ptr(), z.data_ptr(), _ld(z), rows
    with stream_span("standardize_apply", nbytes + 16 * F + 4 * rows * F):
        L.check(L.load().mmvae_standardize_apply(C.byref(a), _stream()), "mmvae_standardize_apply")
    return z


# --------------------------------------------------------------------------------------------
# t-SNE (include/mmvae_hip.h: mmvae_tsne_affinities, mmvae_tsne_gradient, mmvae_tsne_update)
# --------------------------------------------------------------------------------------------
def tsne_affinities(dist2, perplexity, *, p_out=None, beta_out=None):
    """(p, beta): the conditional p_{j|i} fp32 (N, k) of sklearn's _binary_search_perplexity on a row's k squared neighbour distances
    dist2 fp32 (N, k) (the row itself not among them), and the precision fp32 (N,) each row's search ended on (mmvae_tsne_affinities)."""
    what = "tsne_affinities"
    d = _operand(dist2, "dist2", what, dtypes=(torch.float32,))
    N, k = d.shape
    perplexity = float(perplexity)
    if not 0.0 < perplexity < k:
        raise ValueError(f"{what}: perplexity = {perplexity} outside (0, k = {k})")
    p = _out_view(p_out, "p_out", what, torch.float32, N, k, d.device)
    beta = _out_vector(beta_out, "beta_out", what, torch.float32, N, d.device, strided=True)
    a = L.TsneAffinitiesArgs(d.data_ptr(), p.data_ptr(), beta.data_ptr(), _ld(d), _ld(p), N, k, perplexity, 0)
    with stream_span(what, 8 * N * k):
        L.check(L.load().mmvae_tsne_affinities(C.byref(a), _stream()), "mmvae_tsne_affinities")
    return p, beta


def tsne_gradient_splits(N, splits=0):
    """The number of column splits tsne_gradient uses for N points and this request (mmvae_tsne_gradient_splits); needs no device."""
    return _plan("mmvae_tsne_gradient_splits", N, splits)


def tsne_gradient_work_bytes(N, splits=0):
    return _plan("mmvae_tsne_gradient_work_bytes", N, splits, outs=(C.c_int64,))


def tsne_gradient(y, row_ptr, col, val, exaggeration=1.0, *, error=False, z_row=False, splits=0, grad_out=None, work=None):
    """(grad fp32 (N, 2), Z fp32 (1,), err fp32 (N,) or None, z_row fp32 (N,) or None) of the t-SNE objective at the embedding y fp32
    (N, 2) contiguous, for the symmetric P in CSR (row_ptr int32 (N + 1,), col int32 (nnz,), val fp32 (nnz,)) (mmvae_tsne_gradient).
    err.double().sum() is the KL divergence over the stored entries.  splits: 0 = the library's choice, 1 .. 64 forces that many column
    splits.  work: a workspace from an earlier call's sizes (an int64 tensor of tsne_gradient_work_bytes(N, splits) / 8 elements)."""
    what = "tsne_gradient"
    N, dev = _operand(y, "y", what, dtypes=(torch.float32,), cols=2, contiguous=True).shape[0], y.device
    if N < 2:
        raise ValueError(f"{what}: y must have at least 2 rows")
    _vector(row_ptr, "row_ptr", what, torch.int32, N + 1, dev)
    if not isinstance(col, torch.Tensor) or col.dim() != 1:
        raise ValueError(f"{what}: col must be an int32 (nnz,) device tensor")
    nnz = col.shape[0]
    _vector(col, "col", what, torch.int32, nnz, dev)
    _vector(val, "val", what, torch.float32, nnz, dev)
    splits = _splits_arg(splits, what)
    grad = _out_view(grad_out, "grad_out", what, torch.float32, N, 2, dev)
    if not grad.is_contiguous():
        raise ValueError(f"{what}: grad_out must be contiguous")
    z = torch.empty(1, dtype=torch.float32, device=dev)
    err = torch.empty(N, dtype=torch.float32, device=dev) if error else None
    zr = torch.empty(N, dtype=torch.float32, device=dev) if z_row else None
    work = _work(work, tsne_gradient_work_bytes(N, splits), what, dev)
    a = L.TsneGradientArgs(y.data_ptr(), row_ptr.data_ptr(), _p(col) if nnz else None, _p(val) if nnz else None, grad.data_ptr(), z.data_ptr(),
                           _p(err), _p(zr), work.data_ptr(), nnz, work.numel() * 8, N, splits, float(exaggeration), 0)
    with probe_span(what, lambda: dict(kind="valu", flops=10.0 * N * N, M=N, N=N, K=2)):
        L.check(L.load().mmvae_tsne_gradient(C.byref(a), _stream()), "mmvae_tsne_gradient")
    return grad, z, err, zr


def tsne_update_work_bytes(N):
    return _plan("mmvae_tsne_update_work_bytes", N, outs=(C.c_int64,))


def tsne_update(y, update, gains, grad, momentum, learning_rate, *, grad_norm=False, work=None):
    """One step of sklearn's _gradient_descent in place on y, update, gains (fp32 (N, 2), contiguous) from grad (mmvae_tsne_update).
    Returns |gains * grad|_2 as an fp32 (1,) device tensor when grad_norm is set, else None."""
    what = "tsne_update"
    N, dev = _operand(y, "y", what, dtypes=(torch.float32,), cols=2, contiguous=True).shape[0], y.device
    for t, name in ((update, "update"), (gains, "gains"), (grad, "grad")):
        _operand(t, name, what, dtypes=(torch.float32,), rows=N, cols=2, dev=dev, contiguous=True)
    gn = torch.empty(1, dtype=torch.float32, device=dev) if grad_norm else None
    if grad_norm or work is not None:
        work = _work(work, tsne_update_work_bytes(N), what, dev)
    a = L.TsneUpdateArgs(y.data_ptr(), update.data_ptr(), gains.data_ptr(), grad.data_ptr(), _p(gn), _p(work),
                         work.numel() * 8 if work is not None else 0, N, float(momentum), float(learning_rate), 0)
    with stream_span(what, 7 * 8 * N):
        L.check(L.load().mmvae_tsne_update(C.byref(a), _stream()), "mmvae_tsne_update")
    return gn


# --------------------------------------------------------------------------------------------
# The site classifier of the downstream task (include/mmvae_hip.h: mmvae_ln_act_fwd, mmvae_ln_act_bwd, mmvae_wce_mean)
# --------------------------------------------------------------------------------------------
_LN_ROWS = dict(dtypes=(torch.float32,), align=16, ld_multiple=4)        # _operand: fp32 rows the kernels read and write as 16-byte chunks


def _ln_mask(mask, p, what, M, N, dev):
    """(mask, inv_keep): the uint8 keep mask of ops.noise for dropout probability p, or (None, 1) in eval mode / at p = 0"""
    if mask is None:
        return None, 1.0
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{what}: dropout probability {p} outside [0, 1)")
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype != torch.uint8 or tuple(mask.shape) != (M, N) or mask.stride(1) != 1 \
            or _ld(mask) % 4 or mask.data_ptr() % 4 or mask.device != dev:
        raise ValueError(f"{what}: mask must be a uint8 ({M}, {N}) tensor on the operand's device, 4-byte aligned, row stride a multiple of 4")
    return mask, 1.0 / (1.0 - p)


def _ln_width(N, what):
    if N % 4 or not 4 <= N <= L.LN_MAXN:
        raise ValueError(f"{what}: width {N} must be a multiple of 4 in [4, {L.LN_MAXN}]")


def _ln_affine(gamma, beta, what, N, dev):
    for t, name in ((gamma, "gamma"), (beta, "beta")):
        if _vector(t, name, what, torch.float32, N, dev).data_ptr() % 16:
            raise ValueError(f"{what}: {name} must be 16-byte aligned")


def ln_act_fwd(z, gamma=None, beta=None, mask=None, p=0.0, eps=1e-5, *, y_out=None, mean_out=None, rstd_out=None):
    """(y, mean, rstd): Dropout(ReLU(LayerNorm(z))) of z fp32 (M, N) in one launch (mmvae_ln_act_fwd).  mask: the uint8 keep mask of
    ops.noise for dropout probability p, None = no dropout.  gamma = beta = None: no LayerNorm, y = relu(z) keep / (1 - p) and mean,
    rstd are None."""
    what = "ln_act_fwd"
    (M, N), dev = _operand(z, "z", what, **_LN_ROWS).shape, z.device
    _ln_width(N, what)
    ln = gamma is not None
    if ln != (beta is not None):
        raise ValueError(f"{what}: gamma and beta come together")
    y = torch.empty(M, N, dtype=torch.float32, device=dev) if y_out is None else _operand(y_out, "y_out", what, rows=M, cols=N, dev=dev, **_LN_ROWS)
    mean = rstd = None
    if ln:
        _ln_affine(gamma, beta, what, N, dev)
        mean = _out_vector(mean_out, "mean_out", what, torch.float32, M, dev)
        rstd = _out_vector(rstd_out, "rstd_out", what, torch.float32, M, dev)
    mask, inv_keep = _ln_mask(mask, p, what, M, N, dev)
    a = L.LnActFwdArgs(z.data_ptr(), _p(gamma), _p(beta), _p(mask), y.data_ptr(), _p(mean), _p(rstd), _ld(z), _ld0(mask), _ld(y), M, N, int(ln), float(eps), inv_keep, 0)
    with stream_span(what, 9 * M * N):
        L.check(L.load().mmvae_ln_act_fwd(C.byref(a), _stream()), "mmvae_ln_act_fwd")
    return y, mean, rstd


def ln_act_bwd_work_bytes(M, N, layer_norm=True):
    return _plan("mmvae_ln_act_bwd_work_bytes", M, N, int(layer_norm), outs=(C.c_int64,))


def ln_act_bwd(dy, z, mean=None, rstd=None, gamma=None, beta=None, mask=None, p=0.0, *, dz_out=None, dgamma_out=None, dbeta_out=None, work=None):
    """(dz, dgamma, dbeta): the backward of ln_act_fwd from dy = dL/dy and the forward's operands (mmvae_ln_act_bwd); dgamma and dbeta
    are written, bit-identical from run to run.  gamma = None: the form without LayerNorm, dz = dy keep / (1 - p) [z > 0]."""
    what = "ln_act_bwd"
    (M, N), dev = _operand(z, "z", what, **_LN_ROWS).shape, z.device
    _ln_width(N, what)
    _operand(dy, "dy", what, rows=M, cols=N, dev=dev, **_LN_ROWS)
    dz = torch.empty(M, N, dtype=torch.float32, device=dev) if dz_out is None else _operand(dz_out, "dz_out", what, rows=M, cols=N, dev=dev, **_LN_ROWS)
    ln = gamma is not None
    dgamma = dbeta = None
    if ln:
        _ln_affine(gamma, beta, what, N, dev)
        _vector(mean, "mean", what, torch.float32, M, dev)
        _vector(rstd, "rstd", what, torch.float32, M, dev)
        dgamma = _out_vector(dgamma_out, "dgamma_out", what, torch.float32, N, dev)
        dbeta = _out_vector(dbeta_out, "dbeta_out", what, torch.float32, N, dev)
    mask, inv_keep = _ln_mask(mask, p, what, M, N, dev)
    work = _work(work, ln_act_bwd_work_bytes(M, N, ln), what, dev)
    a = L.LnActBwdArgs(dy.data_ptr(), z.data_ptr(), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(mask), dz.data_ptr(), _p(dgamma), _p(dbeta), _p(work),
                       _ld(dy), _ld(z), _ld0(mask), _ld(dz), work.numel() * 8 if work is not None else 0, M, N, int(ln),
                       inv_keep)
    with stream_span(what, 13 * M * N):
        L.check(L.load().mmvae_ln_act_bwd(C.byref(a), _stream()), "mmvae_ln_act_bwd")
    return dz, dgamma, dbeta


def wce_mean(logits, labels, class_weights=None, *, sums=None, grad=False, pred=False, nll=False, confusion=None, grad_out=None, pred_out=None):
    """(g, pred, nll) of nn.CrossEntropyLoss(weight=class_weights) with its mean reduction over logits fp32 (M, C) and labels int64 (M,)
    (mmvae_wce_mean).  sums: a float64 (3,) device tensor that is ADDED to: sum w nll, sum w, labels out of range (the loss is
    sums[0] / sums[1]; a non-zero sums[2] is the caller's to raise on).  g fp32 (M, C): the gradient of that mean w.r.t. the logits;
    pred int32 (M,): the argmax, the first maximum on ties; nll fp32 (M,): the unweighted row terms; confusion: an int32 (C, C) device
    tensor whose [label][prediction] counts are incremented.  Outputs that are not asked for are None."""
    what = "wce_mean"
    x = _operand(logits, "logits", what, dtypes=(torch.float32,))
    (M, Cn), dev = x.shape, x.device
    if not 2 <= Cn <= L.WCE_MAXC:
        raise ValueError(f"{what}: {Cn} classes outside [2, {L.WCE_MAXC}]")
    _vector(labels, "labels", what, torch.int64, M, dev)
    if class_weights is not None:
        _vector(class_weights, "class_weights", what, torch.float32, Cn, dev)
    if sums is not None:
        _vector(sums, "sums", what, torch.float64, 3, dev)
    g = _out_view(grad_out, "grad_out", what, torch.float32, M, Cn, dev) if grad or grad_out is not None else None
    pr = _out_vector(pred_out, "pred_out", what, torch.int32, M, dev) if pred or pred_out is not None else None
    nl = torch.empty(M, dtype=torch.float32, device=dev) if nll else None
    if confusion is not None and (not isinstance(confusion, torch.Tensor) or not confusion.is_cuda or confusion.dtype != torch.int32
                                  or tuple(confusion.shape) != (Cn, Cn) or not confusion.is_contiguous() or confusion.device != dev):
        raise ValueError(f"{what}: confusion must be a contiguous int32 ({Cn}, {Cn}) tensor on the operand's device")
    if sums is None and g is None and pr is None and nl is None and confusion is None:
        raise ValueError(f"{what}: no output asked for")
    a = L.WceArgs(x.data_ptr(), labels.data_ptr(), _p(class_weights), _p(sums), _p(g), _p(pr), _p(nl), _p(confusion), _ld(x), _ld0(g), M, Cn)
    with stream_span(what, 8 * M * Cn):
        L.check(L.load().mmvae_wce_mean(C.byref(a), _stream()), "mmvae_wce_mean")
    return g, pr, nl


def _adam_launch(symbol, span, items, lr, b1, b2, eps, wd, bc1, bc2, maximize, step_dev, lr_dev):
    tick = step_dev is not None and len(items) <= 64
    if step_dev is not None:
        assert step_dev.numel() == L.CTR_COPIES and step_dev.dtype == torch.int64
    with stream_span(span, lambda: 28 * sum(it.n for it in items)):
        L.check(getattr(L.load(), symbol)(C.cast(items, C.c_void_p), len(items), lr, b1, b2, eps, wd, bc1, bc2, int(maximize),
                                          _p(step_dev), int(tick), _p(lr_dev), _stream()), symbol)
    if step_dev is not None and not tick:
        step_dev.add_(1)


def adamw_step(items, lr, b1, b2, eps, wd, bc1, bc2, maximize=False, step_dev=None, lr_dev=None):
    """items: ctypes array of AdamWItem in host memory (device pointers inside).  step_dev: int64[CTR_COPIES] tensor of
    identical copies of the step count: bias corrections from the device counter, which the launch itself increments
    (<= 64 tensors; beyond that the copies are advanced by a fill after the launches)."""
    _adam_launch("mmvae_adamw_step", "adamw", items, lr, b1, b2, eps, wd, bc1, bc2, maximize, step_dev, lr_dev)


def adam_step(items, lr, b1, b2, eps, wd, bc1, bc2, maximize=False, step_dev=None, lr_dev=None):
    """adamw_step with torch.optim.Adam's decay: wd * p joins the gradient instead of scaling p (mmvae_adam_step)."""
    _adam_launch("mmvae_adam_step", "adam", items, lr, b1, b2, eps, wd, bc1, bc2, maximize, step_dev, lr_dev)
