"""The autoencoders' latent-path kernels (mmvae_embed_proj_fwd / _bwd, mmvae_fuse_mean_fwd / _bwd) restated in numpy at a chosen
precision, with the bounds their float32 results are held to around float64.  The projected table is the one-head case of EncoderC's:
its formulas and bounds are elementwise_bounds.embed_* with an empty second head.  The mean of one or two terms is exact after the one
addition (the factor 1 / 2 is a power of two), so the fusion is held BIT-EQUAL to its float32 chain, and only the scatter-add of the
backward has a bound (elementwise_bounds.scatter_tol).

`mistake=` plants one wrong step into a restatement: tests/test_ae_bounds_cpu.py shows that each of them leaves the bounds."""
import numpy as np

import elementwise_bounds as E

U = E.U
MISTAKES = ("n_plus_one", "no_table", "mean_twice", "no_bias", "wrong_column", "dirty_pads")


def _a(x, dt):
    return np.asarray(x).astype(dt)


# --- Embedding -> Linear(embed, latent): table[S][L] = emb x w^T + b ---------------------------------------------------------------
def proj_fwd(emb, w, b, dt, mistake=None):
    if mistake == "no_bias":
        b = np.zeros_like(b)
    if mistake == "wrong_column":
        w = np.roll(w, 1, axis=0)
    return E.embed_fwd(emb, w, b, w[:0], b[:0], dt)


def proj_fwd_tol(emb, w, b):
    return E.embed_fwd_tol(emb, w, b, w[:0], b[:0])


def proj_bwd(d_table_copies, emb, w, old, dt):
    """old = (d_emb, d_w, d_b): accumulated into -> the three new gradients"""
    return E.embed_bwd(d_table_copies, emb, w, w[:0], old, dt)


def proj_bwd_tol(d_table_copies, emb, w, old):
    return E.embed_bwd_tol(d_table_copies, emb, w, w[:0], old)


# --- the plain mean ------------------------------------------------------------------------------------------------------------------
def fuse_mean_fwd(head, table, site, L, ldz, dt, zdt=None, mistake=None):
    """head: (B, >= L) or None; table (S, L) + site (B,) or None -> (latent (B, L) in dt, z (B, ldz) as float64 values of the z type:
    zdt = "bf16" rounds to bf16, pad columns zero).  The sum is formed in the order head, table row; a label outside [0, S) poisons
    its row with NaN."""
    terms = []
    if head is not None:
        h = _a(head, dt)
        terms.append(np.roll(h[:, :L], 1, axis=1) if mistake == "wrong_column" else h[:, :L])
    if table is not None and mistake != "no_table":
        S = table.shape[0]
        ok = (site >= 0) & (site < S)
        rows = _a(table, dt)[np.where(ok, site, 0)]
        rows[~ok] = np.nan
        terms.append(rows)
    n = (head is not None) + (table is not None)
    s = terms[0] if len(terms) == 1 else terms[0] + terms[1]
    if n > 1:
        inv = dt(1) / dt(n + 1 if mistake == "n_plus_one" else n)
        s = s * inv
        if mistake == "mean_twice":
            s = s * inv
    latent = s.astype(dt)
    z = np.full((latent.shape[0], ldz), 1.0 if mistake == "dirty_pads" else 0.0)
    z[:, :L] = bf16(latent) if zdt == "bf16" else latent
    return latent, z


def bf16(x):
    """round-to-nearest-even to bf16, as float64 values (NaN stays NaN)"""
    x32 = np.ascontiguousarray(np.asarray(x, np.float32))
    b = x32.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    out = r.view(np.float32).astype(np.float64)
    out[np.isnan(x32)] = np.nan
    return out


def fuse_mean_bwd(dz, g_latent, n_mod, dt, mistake=None):
    """d_head = (dz + g_latent) * (1 / n_mod) in dt"""
    d = _a(dz, dt) if g_latent is None else _a(dz, dt) + _a(g_latent, dt)
    if n_mod > 1:
        d = d * (dt(1) / dt(n_mod + 1 if mistake == "n_plus_one" else n_mod))
        if mistake == "mean_twice":
            d = d * (dt(1) / dt(n_mod))
    return d


def fuse_mean_bwd_tol(dz, g_latent, n_mod):
    """one addition when a gradient arrived at the latent (U |sum|); the factor 1 or 1 / 2 is exact"""
    if g_latent is None:
        return np.zeros(np.shape(dz))
    return E.SECOND * U * np.abs(_a(dz, np.float64) + _a(g_latent, np.float64))


# --- the fused latent launch (mmvae_ae_latent_fwd): head GEMM -> mean -> z -> the decoder's first layer ------------------------------
BF16_HALF_ULP = 2.0 ** -9


def fused_latent(x, w, b, table, site, w0, b0, dt, mistake=None):
    """x (B, K): the head GEMM's operand AFTER its prologue, bf16 values; w (L, K), w0 (N, L): bf16 values; b, b0, table: fp32.
    head = x w^T + b accumulated over k ascending from 0, the bias added last (the MFMA chain); latent = mean(head, table[site]);
    z = bf16(latent); h0 = bf16(relu(z w0^T + b0)).  -> (latent (B, L) in dt, z and h0 as float64 values)"""
    w0 = _a(w0, dt)
    L, head = w0.shape[1], None
    if x is not None:                                    # None: no encoder (site only)
        x, w = _a(x, dt), _a(w, dt)
        acc = np.zeros((x.shape[0], L), dt)
        for k in range(x.shape[1]):
            acc = acc + x[:, k, None] * w[None, :, k]
        head = acc if mistake == "no_bias" else acc + _a(b, dt)
    latent, z = fuse_mean_fwd(head, table, site, L, L, dt, "bf16", mistake=mistake)
    zz = z[:, :L].astype(dt)
    acc0 = np.zeros((zz.shape[0], w0.shape[0]), dt)
    for k in range(L):
        acc0 = acc0 + zz[:, k, None] * w0[None, :, k]
    h0 = bf16(np.maximum(acc0 + _a(b0, dt), 0).astype(np.float32))
    return latent, z, h0


def fused_latent_tol(x, w, b, table, site, w0, b0):
    """-> (bound on latent, on z, on h0) around the float64 restatement fused_latent(..., np.float64).
    head: K products (exact in fp32 for bf16 operands) and K + 1 additions, (K + 1) U (|b| + |x||w|^T); the mean halves it and adds the
    one rounding of the sum; a site-only latent is a copy.  z: both sides round to bf16 (half an ulp, 2^-9 relative, each).  The first
    layer carries z's bound through |w0|, adds the (L + 1) U of its own chain, and both sides round the result to bf16 again."""
    lat64, _, _ = fused_latent(x, w, b, table, site, w0, b0, np.float64)
    ax, aw, aw0 = (np.abs(_a(v, np.float64)) for v in (x, w, w0)) if x is not None else (None, None, np.abs(_a(w0, np.float64)))
    if x is None:
        lat_tol = np.zeros_like(lat64)
    else:
        head_tol = (x.shape[1] + 1) * U * (np.abs(_a(b, np.float64))[None, :] + ax @ aw.T)
        lat_tol = head_tol if table is None else 0.5 * head_tol + U * np.abs(lat64)
    lat_tol = E.SECOND * np.nan_to_num(lat_tol)
    lat = np.nan_to_num(np.abs(lat64))
    z_tol = lat_tol + 2 * BF16_HALF_ULP * (lat + lat_tol)
    L = aw0.shape[1]
    mag = np.abs(_a(b0, np.float64))[None, :] + (lat + z_tol) @ aw0.T
    pre_tol = z_tol @ aw0.T + (L + 1) * U * mag
    return lat_tol, z_tol, E.SECOND * (pre_tol + 2 * BF16_HALF_ULP * (mag + pre_tol))
