"""The bounds of tests/loss_bounds.py on the CPU, on the inputs tests/test_loss_kernel_gpu.py gives the device (tests/loss_cases.py):

  * a float32 numpy restatement of every expression of the loss kernel stays inside its bound against the float64 reference -- no
    bound is tighter than float32 arithmetic; the half wave's butterfly counts as one more summation order;
  * every deliberate mistake in the restatement falls outside its bound on those inputs -- no bound is so wide that it hides one;
  * the generators contain the edges they claim (counts of saturated, denormal, clamped, ignored and out-of-range entries);
  * the restated launcher choices (vector width, class path, grid, length of the fp32 chains) at the shapes the GPU test relies on.
"""
import numpy as np
import pytest

import loss_bounds as LB
import loss_cases as LC

F32, F64 = np.float32, np.float64


def ratio(got, ref, tol):
    """Largest err / bound; inf where an element is outside (or not a number)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    tol = np.broadcast_to(np.asarray(tol, F64), ref.shape)
    err = np.abs(got - ref)
    if not (err <= tol).all():
        return float("inf")
    nz = tol > 0
    return float(np.max(err[nz] / tol[nz])) if nz.any() else 0.0


def inside(got, ref, tol, what):
    r = ratio(got, ref, tol)
    assert r <= 1.0, f"{what}: float32 restatement outside the bound"
    return r


def outside(got, ref, tol, what):
    assert ratio(got, ref, tol) == float("inf"), f"{what}: the mistake stays inside the bound"


# ---------------------------------------------------------------------------------------------
# streaming parts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_bf16", [False, True])
@pytest.mark.parametrize("g_bf16", [False, True])
def test_mse_bound(t_bf16, g_bf16):
    x, t = LC.mse_case(np.random.default_rng(1), 41, 333, t_bf16)
    assert (x == 0).sum() > 1000 and (t == 0).sum() > 1000 and ((x == t) & (x != 0)).sum() > 500
    assert np.log10(np.abs(x[x != 0]).max() / np.abs(x[x != 0]).min()) > 6                      # mixed magnitudes
    (g_ref, term_ref), (tol_g, tol_t) = LB.mse(x, t, F64), LB.mse_tol(x, t)
    rd = (lambda v: LB.q_bf16(v)) if g_bf16 else (lambda v: v)
    tol_g = LB.bf16_out(tol_g, g_ref) if g_bf16 else tol_g
    g, term = LB.mse(x, t, F32)
    inside(rd(g), g_ref, tol_g, "mse gradient")
    inside(term, term_ref, tol_t, "mse term")
    outside(rd(LB.mse(x, t, F32, "factor 1")[0]), g_ref, tol_g, "mse gradient factor 1")


@pytest.mark.parametrize("t_bf16", [False, True])
@pytest.mark.parametrize("wrt_logit", [False, True])
def test_bce_bound_and_edges(wrt_logit, t_bf16):
    p, t = LC.bce_case(np.random.default_rng(2), 29, 333, t_bf16)
    c = LC.bce_edge_counts(p, t)
    assert c["zero"] == 3 and c["one"] == 3 and c["denormal"] == 9, c             # each against the targets 0, 1, fractional
    assert c["clamped"] >= 3 * 9 and c["unclamped_near"] >= 3 and c["hard_targets"] >= 2 * len(LC.P_EDGES), c
    (g_ref, term_ref), (tol_g, tol_t) = LB.bce(p, t, wrt_logit, F64), LB.bce_tol(p, t, wrt_logit)
    assert term_ref.max() == 100.0 and np.isfinite(g_ref).all() and np.isfinite(tol_g).all()
    if not wrt_logit:
        assert np.abs(g_ref).max() >= 9e11                                             # (p - t) / 1e-12
    g, term = LB.bce(p, t, wrt_logit, F32)
    inside(g, g_ref, tol_g, "bce gradient")
    inside(LB.q_bf16(g), g_ref, LB.bf16_out(tol_g, g_ref), "bce gradient bf16")
    inside(term, term_ref, tol_t, "bce term")
    outside(LB.bce(p, t, wrt_logit, F32, "clamp -88")[1], term_ref, tol_t, "bce clamp at -88")
    if wrt_logit:
        outside(LB.bce(p, t, True, F32, "no min factor")[0], g_ref, tol_g, "bce gradient without min(pq 1e12, 1)")
    else:
        outside(LB.bce(p, t, False, F32, "clamp 1e-6")[0], g_ref, tol_g, "bce d/dp clamp at 1e-6")


def test_bce_denormal_p_flushed_to_zero_is_outside():
    """What an instruction that reads a denormal p as 0 would return: the clamp, -100, instead of ln p = -87.3 ... -103."""
    p = np.array([1e-40, 1e-38, 2.0 ** -140], F32)
    t = np.ones(3, F32)
    _, term_ref = LB.bce(p, t, True, F64)
    outside(np.full(3, 100.0), term_ref, LB.bce_tol(p, t, True)[1], "denormal p flushed")
    inside(LB.bce(p, t, True, F32)[1], term_ref, LB.bce_tol(p, t, True)[1], "denormal p")


# ---------------------------------------------------------------------------------------------
# class term
# ---------------------------------------------------------------------------------------------
CE_FORMS = [("softmax", "seq"), ("softmax", "tree"), ("scalar", "seq")]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("S", [1, 4, 22, 24, 31, 32, 33, 40])
def test_class_bound_edges_and_mistakes(S, weighted):
    B, gamma = 515, 1.7
    x, y, cw = LC.class_case(np.random.default_rng(10 * S + weighted), B, S, weighted)
    c = LC.class_edge_counts(x, y, cw)
    assert c["ignored"] == 74 and c["bad"] == 6 and c["equal_rows"] >= 103, c
    if S > 1:
        assert c["underflow_rows"] == 103 and c["overflow_rows"] >= 30 and c["label_is_max"] >= 40 and c["label_not_max"] >= 40, c
    if weighted and S > 1:
        assert cw[S // 2] == 0 and ((cw > 0.3) | (cw == 0)).all() and (c["zero_weight_rows"] >= 1 or S > 8), c
    for form, order in CE_FORMS:
        if order == "tree" and S > 32:
            continue
        term_ref, g_ref, n_bad = LB.ce(x, y, cw, gamma, form, F64)
        tol_t, tol_g = LB.ce_tol(x, y, cw, gamma, form)
        assert n_bad == 6 and np.isfinite(term_ref).all() and np.isfinite(g_ref).all()
        assert (tol_g[y == -100] == 0).all() and (g_ref[y == -100] == 0).all() and (term_ref[y == -100] == 0).all()
        term, g, _ = LB.ce(x, y, cw, gamma, form, F32, order)
        inside(term, term_ref, tol_t, f"class term {form} {order}")
        inside(g, g_ref, tol_g, f"class gradient {form} {order}")
        assert (g[y == -100] == 0).all()
        if S == 1:
            continue
        mistakes = ["onehot y+1", "gamma dropped", "ignore as class 0", "bad label kept", "no max"] + (["wrong weight"] if weighted else [])
        for mk in mistakes:
            term, g, _ = LB.ce(x, y, cw, gamma, form, F32, order, mistake=mk)
            if mk not in ("onehot y+1", "gamma dropped"):
                outside(term, term_ref, tol_t, f"class term {form}: {mk}")
            outside(g, g_ref, tol_g, f"class gradient {form}: {mk}")


def test_softmax_and_scalar_references_agree():
    """The two gradient expressions are the same function: their float64 values agree far inside either bound."""
    x, y, cw = LC.class_case(np.random.default_rng(5), 515, 24, True)
    a, b = LB.ce(x, y, cw, 0.7, "softmax", F64), LB.ce(x, y, cw, 0.7, "scalar", F64)
    assert ratio(a[1], b[1], 1e-3 * LB.ce_tol(x, y, cw, 0.7, "softmax")[1] + 1e-300) < 1 and np.array_equal(a[0], b[0])


# ---------------------------------------------------------------------------------------------
# KL term
# ---------------------------------------------------------------------------------------------
def test_kl_bound_edges_and_mistakes():
    mu, lv = LC.kl_case(np.random.default_rng(3), 4099, 20)
    c = LC.kl_edge_counts(mu, lv)
    assert c["big_mu"] >= 800 and all(c[f"lv {v:g}"] >= 1200 for v in LC.LV_EDGES), c
    assert lv.max() == 80 and np.exp(lv.astype(F64)).max() < np.finfo(F32).max and np.exp(F32(-110)) == 0
    beta = 0.25
    ref, tol = LB.kl(mu, lv, beta, F64), LB.kl_tol(mu, lv, beta)
    got = LB.kl(mu, lv, beta, F32)
    for k, nm in enumerate(("term", "g_mu", "g_lv")):
        inside(got[k], ref[k], tol[k], f"kl {nm}")
    outside(LB.kl(mu, lv, beta, F32, "g_lv sign")[2], ref[2], tol[2], "kl g_lv sign")
    bad = LB.kl(mu, lv, beta, F32, "exp half")
    outside(bad[0], ref[0], tol[0], "kl term exp(lv / 2)")
    one = LC.kl_case(np.random.default_rng(4), 1, 1)
    assert one[0].shape == (1, 1)


# ---------------------------------------------------------------------------------------------
# sums and the launcher's choices
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n32", [1, 7, 64, 1024])
def test_sum_bound(n32):
    rng = np.random.default_rng(n32)
    x, t = LC.mse_case(rng, 300, 333)
    term_ref, tol_t = LB.mse(x, t, F64)[1].ravel(), LB.mse_tol(x, t)[1].ravel()
    term = LB.mse(x, t, F32)[1].ravel()
    n = len(term) // n32 * n32
    for perm in (np.arange(n), rng.permutation(n)):
        chunks = term[:n][perm].reshape(-1, n32)
        part = np.cumsum(chunks, axis=1, dtype=F32)[:, -1]                 # a sequential fp32 sum per chain
        got = float(part.astype(F64).sum())
        tol = LB.sum_tol(term_ref[:n], tol_t[:n], n32)
        assert abs(got - float(term_ref[:n].sum())) <= tol
    # a term that is dropped is outside
    assert abs(float(term_ref[:n].sum()) - float(term_ref[1:n].sum())) > LB.sum_tol(term_ref[:n], tol_t[:n], n32) or term_ref[0] == 0
    k = int(np.argmax(term_ref[:n]))
    assert term_ref[k] > LB.sum_tol(term_ref[:n], tol_t[:n], n32)


def test_launcher_restated():
    # vector widths: by the width, by the address, by the leading dimension
    assert LB.vec_width(572, [(4096, 572, 4)] * 3) == 4 and LB.vec_width(782, [(4096, 782, 4)] * 3) == 2
    assert LB.vec_width(333, [(4096, 333, 4)]) == 1
    assert LB.vec_width(572, [(4096, 572, 4), (4100, 572, 4)]) == 1 and LB.vec_width(572, [(4096, 572, 4), (4104, 572, 4)]) == 2
    assert LB.vec_width(572, [(4096, 573, 4)]) == 1 and LB.vec_width(572, [(4096, 574, 2)]) == 2
    assert LB.vec_width(572, [(4096, 572, 4), (4100, 572, 2), (None, 0, 4)]) == 2       # bf16 rows on a 4-byte boundary
    # class paths
    assert LB.ce_path(24, 24, 4096, 24, 4096) == "thread" and LB.ce_path(24, 25, 4096) == "half"
    assert LB.ce_path(24, 24, 4096, 26, 4096) == "half" and LB.ce_path(24, 24, 4096, 24, 4100) == "half"
    assert LB.ce_path(22, 22, 4096) == "half" and LB.ce_path(33, 33, 4096) == "scalar" and LB.ce_path(32, 32, 4096) == "thread"
    # grids
    assert LB.launch(4099, A=782, va=2, D=572, vd=4) == (1024, False)
    assert LB.launch(1, A=333) == (1, False) and LB.launch(3, A=2051) == (7, False)
    assert LB.launch(131077, S=4, path="thread") == (512, True) and LB.launch(515, S=24, path="thread") == (3, True)
    assert LB.launch(40000, S=22, path="half") == (512, True) and LB.launch(131077, S=33, path="scalar") == (512, True)
    assert LB.launch(65537, L=24) == (512, True) and LB.launch(300, S=24, path="thread", L=24) == (2, True)
    # fp32 chains
    assert LB.fp32_chain("class", 512, True, 131077, path="thread") == 1 and LB.fp32_chain("kl", 512, True, 65537, W=24) == 1
    assert LB.fp32_chain("class", 512, True, 40000, path="half") == 10 and LB.fp32_chain("class", 512, True, 131077, path="scalar") == 2
    assert LB.fp32_chain("class", 1024, False, 40000, path="half") == 64 * 5
    assert LB.fp32_chain("stream", 1024, False, 4099, W=782, V=2) == 64 * 2 * 7
