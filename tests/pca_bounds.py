"""Derived bounds for mmvae_pca_scatter, mmvae_pca_project and mmvae.pca.PCA around the float64 restatement of tests/pca_ref.py.
Nothing here is tuned to what the device gives.  u = 2^-24, gamma(n) = n u / (1 - n u).

Scatter.  |S_ab - S*_ab| <= E_ab = gamma(N + 2) sum_i |x_ia - c_a| |x_ib - c_b|, S* the float64 scatter matrix about the SAME fp32 c.
    The kernel as built (csrc/pca.hip): each centred operand is one fp32 subtraction (1 rounding each, 2 per term); a term then enters
    a chain of fused multiply-adds over the rows of its split (the product is not rounded on its own; n_s roundings at most for the
    first term of a split of n_s rows) and the splits' partial sums are added in ascending order (splits - 1 more).  Every split is
    non-empty, so n_s + splits - 1 <= N: at most N + 2 roundings on any term's path, in any order of the rows.  Rows that pad the
    last chunk are staged as exact zeros and add nothing.
Projection, given the v the kernel received.  |y_ij - y*_ij| <= gamma(F + 2) sum_f |x_if - c_f| |v_jf|: one rounding for the centred
    operand and a chain of F fused multiply-adds (F + 1 <= F + 2).
Eigenvalues.  Weyl: |lam_j - lam*_j| <= |E|_F, plus the float64 solver's backward error, budgeted F 2^-53 |S|_2, plus N |m - c|^2 for
    centring at the fp32-rounded mean c instead of the exact mean m (S_c = S_m + N (m - c)(m - c)^T).
Component j with eigengap g_j = min(lam*_{j-1} - lam*_j, lam*_j - lam*_{j+1}):  sin angle(v_j, v*_j) <= 2 |E|_F / g_j (Davis-Kahan as
    in Yu, Wang and Samworth 2015).  Span of the first k:  |P - P*|_2 <= 2 |E|_F / (lam*_k - lam*_{k+1}).
End to end.  |y_ij - y*_ij| <= |x_i - c|_2 (sqrt(2) sin-bound_j + u) + the projection bound: sign-aligned unit vectors at angle t
    differ by at most sqrt(2) sin t, the fp32 rounding of a component moves it by at most u.
The variance vectors follow from the eigenvalue bound: / (N - 1); |sqrt(l) - sqrt(l*)| <= bound / sqrt(l*); the ratio with the trace's
    own bound sum_a E_aa + N |m - c|^2."""
import numpy as np

import pca_ref as PR

U = 2.0 ** -24
MAX_COMPONENT_BOUND = 1e-3          # what a case used for per-component checks must reach
MAX_SPAN_BOUND = 1e-2               # ... and the k = 50 case for its span


def gamma(n):
    return n * U / (1.0 - n * U)


def scatter_bound(x, c):
    """E (F, F): c the fp32 shift (None = 0)"""
    A = np.abs(np.asarray(x, np.float64) - (0.0 if c is None else np.asarray(c, np.float64)))
    return gamma(len(A) + 2) * (A.T @ A)


def project_bound(x, c, v):
    A = np.abs(np.asarray(x, np.float64) - (0.0 if c is None else np.asarray(c, np.float64)))
    return gamma(A.shape[1] + 2) * (A @ np.abs(np.asarray(v, np.float64)).T)


def analyse(x, k):
    """everything the checks of a PCA(k) of x need, from float64"""
    x = np.asarray(x, np.float32)
    N, F = x.shape
    c = PR.column_means(x)
    ref = PR.fit(x, k)                                       # about the exact mean, as sklearn
    E = scatter_bound(x, c)
    EF = np.sqrt((E * E).sum())
    dm = ref["mean"] - c.astype(np.float64)
    centre = N * (dm * dm).sum()
    lam = ref["lam_all"]
    eig = EF + F * 2.0 ** -53 * lam[0] + centre
    lam_pad = np.concatenate([[np.inf], lam, [-np.inf]])
    gap = np.minimum(lam_pad[:k] - lam_pad[1:k + 1], lam_pad[1:k + 1] - lam_pad[2:k + 2])
    span_gap = lam[k - 1] - (lam[k] if k < len(lam) else 0.0)
    xc = x.astype(np.float64) - c.astype(np.float64)
    return dict(x=x, N=N, F=F, k=k, c=c, ref=ref, S_c=PR.scatter(x, c), E=E, EF=EF, centre=centre, eig=eig, sin=2.0 * EF / gap,
                span=2.0 * EF / span_gap if span_gap > 0 else np.inf, trace_err=np.trace(E) + centre, rownorm=np.sqrt((xc * xc).sum(axis=1)),
                y_ref=PR.transform(x, c, ref["components"]))


def check_scatter(S, x, c, label=""):
    """S float32 (F, F) from the device or an emulation: bitwise symmetric and inside E around the float64 matrix about c.  Returns
    the list of violations and the largest error / bound."""
    S = np.asarray(S)
    bad = []
    if not np.array_equal(S.view(np.int32), S.T.copy().view(np.int32)):
        bad.append(f"{label}: S is not bitwise symmetric")
    E = scatter_bound(x, c)
    err = np.abs(S.astype(np.float64) - PR.scatter(x, c))
    ratio = float((err / np.maximum(E, 1e-300)).max())
    if not (err <= E).all():
        bad.append(f"{label}: scatter error {ratio:.3g} of its bound")
    return bad, ratio


def check_project(y, x, c, v, label=""):
    y = np.asarray(y, np.float64)
    B = project_bound(x, c, v)
    err = np.abs(y - PR.transform(x, c if c is not None else 0.0, v))
    ratio = float((err / np.maximum(B, 1e-300)).max())
    return ([] if (err <= B).all() else [f"{label}: projection error {ratio:.3g} of its bound"]), ratio


def check_fit(an, got, per_component, label=""):
    """got: components (k, F) fp32, explained_variance, explained_variance_ratio, singular_values (float64 (k,)).  Returns (violations,
    {check: largest error / bound})."""
    N, F, k, ref = an["N"], an["F"], an["k"], an["ref"]
    bad, ratios = [], {}
    tiny = 8.0 * 2.0 ** -53                                   # the float64 arithmetic behind the vectors themselves

    def within(name, err, bound):
        ratios[name] = float((err / np.maximum(bound, 1e-300)).max())
        if not (err <= bound).all():
            bad.append(f"{label}: {name} {ratios[name]:.3g} of its bound")

    ev, evr, sv = (np.asarray(got[n], np.float64) for n in ("explained_variance", "explained_variance_ratio", "singular_values"))
    lam = ref["lam_all"][:k]
    within("explained_variance", np.abs(ev - ref["explained_variance"]), an["eig"] / (N - 1) + tiny * ref["explained_variance"])
    within("singular_values", np.abs(sv - ref["singular_values"]), an["eig"] / np.sqrt(lam) + tiny * ref["singular_values"])
    t = np.trace(ref["S"])
    t_lo = t - an["trace_err"]
    within("explained_variance_ratio", np.abs(evr - ref["explained_variance_ratio"]),
           an["eig"] / t_lo + lam * an["trace_err"] / (t * t_lo) + tiny * ref["explained_variance_ratio"])
    V = np.asarray(got["components"], np.float64)
    within("orthonormality", np.abs(V @ V.T - np.eye(k)), np.full((k, k), 2.0 * U + U * U + 64.0 * F * 2.0 ** -53))
    Vr = ref["components"]
    P, Pr = V.T @ V, Vr.T @ Vr
    within("span", np.array([np.linalg.norm(P - Pr, 2)]), np.array([an["span"]]))
    if per_component:
        dots = (V * Vr).sum(axis=1)
        resid = V - dots[:, None] * Vr
        sin = np.sqrt((resid * resid).sum(axis=1)) / np.sqrt((V * V).sum(axis=1))
        within("component angle", sin, an["sin"])
        if not (dots > 0).all():
            bad.append(f"{label}: sign of components {np.flatnonzero(dots <= 0).tolist()}")
    return bad, ratios


def check_end_to_end(an, y, components, label=""):
    """y = transform(x) of the fitted device PCA against the float64 restatement's, for cases with per-component bounds"""
    y = np.asarray(y, np.float64)
    B = an["rownorm"][:, None] * (np.sqrt(2.0) * an["sin"] + U)[None, :] + project_bound(an["x"], an["c"], components)
    err = np.abs(y - an["y_ref"])
    ratio = float((err / B).max())
    return ([] if (err <= B).all() else [f"{label}: end-to-end error {ratio:.3g} of its bound"]), ratio
