"""Reconstruction from the directional VAEs as an imputer uses it: the mean of several draws of z -- and, for samples without a
primary site, of all sites -- with the spread across them as its uncertainty.

The reference (reconstruct_unmatched.py) runs ONE forward per sample: one eps (vae.py:73 samples in eval mode too) and, for
DNA-only samples, `site=None`; it names "iterate through all possible sites and average" as the alternative it does not do.
Here every sample owns G = draws (x sites) consecutive rows of the decoder's input; the decoder's last Linear reduces each
group on chip (ops.gemm_nt_group_moments), so the B G x N reconstructions are never stored.
"""
import numpy as np
import torch

from . import _lib as L_, engine, ops
from .ops import ceil_to, act_dtype, ACT_NONE, ACT_RELU, ACT_SIGMOID

# Rows are processed in chunks of whole groups so that what a chunk allocates -- z, the decoder's hidden activations and, on the
# unfused path, the fp32 output of the last layer -- stays below this many bytes (one group at least, whatever it needs).
CHUNK_BYTES = 256 << 20


class Reconstructor:
    """reconstruct() for an RNA2DNAVAE or a DNA2RNAVAE (any module whose _graph() is a VAEGraph with ONE data encoder, a site
    encoder and one decoder)."""

    def __init__(self, model):
        g = model._graph()
        encs = [e for e in (g.enc_a, g.enc_b) if e is not None]
        if type(g) is not engine.VAEGraph or len(encs) != 1 or g.enc_c is None or len(g.decoders) != 1:
            raise TypeError(f"Reconstructor: {type(model).__name__} is not a directional VAE (one data encoder, a site encoder, one decoder)")
        self.model, self.graph, self.enc, self.dec = model, g, encs[0], g.decoders[0]
        self.flatten = g.enc_a is None or g.flatten_a          # input b is always flattened (encoders.py:44 view)
        self.n_sites = g.enc_c.embedding.weight.shape[0]
        self.last_fused = None                                  # whether the last call's final layer ran as the fused launch

    def group_size(self, draws, sites):
        return draws * (self.n_sites if sites == "all" else 1)

    def chunk_groups(self, G, fused):
        """Samples per row chunk: CHUNK_BYTES over the bytes a group allocates, rounded down to whole tiles of the fused kernel
        (floor(128 / G) groups each; one group for G > 128), at least one tile."""
        esz = 2 if self.model._prec() == ops.PREC_BF16 else 4
        row = esz * (ceil_to(self.graph.latent, 8) + sum(ceil_to(pl.N, 8) for pl in self.dec.pl[:-1])) + 12 * self.graph.latent
        if not fused:
            row += 4 * self.dec.pl[-1].N
        gpt = max(1, ops.GROUP_MOMENTS_MAX_G // G)
        return max(gpt, CHUNK_BYTES // (row * G) // gpt * gpt)

    @torch.no_grad()
    def reconstruct(self, x, site=None, *, draws=1, sites="given", return_std=False):
        """x: (B, features) of the model's input modality; site: (B,) class indices for sites="given".
        sites: "given" (every sample's own site), "none" (the data encoder alone, the reference's DNA-only form) or "all" (every
        site in turn).  Group member g = s * draws + k of sample b is site s, draw k; eps is ONE (B G, latent) draw of the model's
        NoiseSource in that row order.  -> (mean (B, N) fp32, std (B, N) fp32 | None): mean and unbiased std over the group; with
        G == 1 the plain forward's output and None."""
        if sites not in ("given", "none", "all"):
            raise ValueError(f"reconstruct: sites must be 'given', 'none' or 'all', got {sites!r}")
        if int(draws) != draws or draws < 1:
            raise ValueError(f"reconstruct: draws must be a positive integer, got {draws!r}")
        if sites == "given" and site is None:
            raise ValueError("reconstruct: sites='given' needs `site`")
        if sites != "given" and site is not None:
            raise ValueError(f"reconstruct: sites={sites!r} takes no `site`")
        G = self.group_size(int(draws), sites)
        if return_std and G == 1:
            raise ValueError("reconstruct: the spread of one reconstruction is undefined (draws == 1 and one site)")
        was_training = self.model.training
        self.model.eval()
        try:
            if G == 1:
                self.last_fused = None
                return self.model(x, site)[0], None
            with ops.pinned_stream():
                return self._grouped(x, site, int(draws), sites, G, return_std)
        finally:
            self.model.train(was_training)

    def reconstruct_batched(self, x, site, *, draws, sites, batch_size, seed):
        """reconstruct() over the host float32 rows x (site: host int64 or None) in batches, from the Philox position (seed, offset 0) set
        ONCE before the first batch -> (mean, std or None for a group of one) as host float32 arrays"""
        dev = next(self.model.parameters()).device
        torch.manual_seed(seed)
        engine.GLOBAL_NOISE.load_state_dict({"offset": 0}, dev)
        want_std = self.group_size(draws, sites) > 1
        means, stds = [], []
        for i in range(0, x.shape[0], batch_size):
            xb = torch.from_numpy(x[i:i + batch_size]).to(dev)
            sb = torch.from_numpy(site[i:i + batch_size]).to(dev) if site is not None else None
            m, s = self.reconstruct(xb, sb, draws=draws, sites=sites, return_std=want_std)
            means.append(m.cpu().numpy())
            if want_std:
                stds.append(s.cpu().numpy())
        return np.concatenate(means), (np.concatenate(stds) if want_std else None)

    def _grouped(self, x, site, draws, sites, G, return_std):
        g, enc, dec, prec = self.graph, self.enc, self.dec, self.model._prec()
        x = engine._check_input(x.reshape(x.shape[0], -1) if self.flatten else x, "x", enc.in_dim, prec)
        B, dev, Ld = x.shape[0], x.device, g.latent
        g._prep.ensure(prec, dev, g.param_list(), g._prepare)
        heads = enc.forward(prec, x, False, None, heads=True)[0]              # (B, 2 L) fp32: ONE pass of the data encoder
        table = None if sites == "none" else g.enc_c.table()
        eps = g.noise.draw(B * G, [], Ld, dev)[1]
        if sites == "given":
            site = site.to(device=dev, dtype=torch.int64).contiguous()
            if tuple(site.shape) != (B,):
                raise ValueError(f"reconstruct: site must have shape ({B},), got {tuple(site.shape)}")
        elif sites == "all":
            member_site = torch.arange(self.n_sites, device=dev).repeat_interleave(draws)            # site of group member g
        last = dec.pl[-1]
        act = ACT_SIGMOID if dec.final_sigmoid else ACT_NONE
        fused = ops.group_moments_fits(prec, 1, G, last.N, last.K, act, return_std)
        self.last_fused = fused
        mean = torch.empty(B, last.N, dtype=torch.float32, device=dev)
        std = torch.empty(B, last.N, dtype=torch.float32, device=dev) if return_std else None
        step = self.chunk_groups(G, fused)
        for b0 in range(0, B, step):
            bc = min(step, B - b0)
            rows = bc * G
            heads_r = heads[b0:b0 + bc].repeat_interleave(G, dim=0)
            if sites == "given":
                site_r = site[b0:b0 + bc].repeat_interleave(G)
            else:
                site_r = member_site.repeat(bc) if sites == "all" else None
            mu = torch.empty(rows, Ld, dtype=torch.float32, device=dev)
            logvar = torch.empty(rows, Ld, dtype=torch.float32, device=dev)
            z = torch.empty(rows, ceil_to(Ld, 8), dtype=act_dtype(prec), device=dev)
            if enc is g.enc_a:
                ops.fuse_reparam_fwd(rows, Ld, heads_r, None, table, site_r, eps[b0 * G:b0 * G + rows], mu, logvar, z)
            else:
                ops.fuse_reparam_fwd(rows, Ld, None, heads_r, table, site_r, eps[b0 * G:b0 * G + rows], mu, logvar, z)
            h = z
            for j, pl in enumerate(dec.pl[:-1]):
                out = torch.empty(rows, ceil_to(pl.N, 8), dtype=act_dtype(prec), device=dev)
                ops.gemm_nt(prec, h, pl.w, pl.N, pl.K, out, bias=pl.bias, act=ACT_RELU, tag=f"{dec.name}.L{j}.fwd")
                h = out
            m_c, s_c = mean[b0:b0 + bc], (std[b0:b0 + bc] if return_std else None)
            if fused:
                try:
                    ops.gemm_nt_group_moments(prec, h, last.w, last.N, last.K, G, m_c, s_c, bias=last.bias, act=act)
                    continue
                except L_.MMVAEArgError:               # refused before anything was enqueued: the launches it replaces
                    self.last_fused = fused = False
            full = torch.empty(rows, last.N, dtype=torch.float32, device=dev)
            ops.gemm_nt(prec, h, last.w, last.N, last.K, full, bias=last.bias, act=act, tag=f"{dec.name}.L{len(dec.pl) - 1}.fwd")
            full = full.view(bc, G, last.N)
            torch.mean(full, dim=1, out=m_c)
            if return_std:
                torch.std(full, dim=1, out=s_c)
        return mean, std
