#!/usr/bin/env python3
"""Generate tests/golden/ae_b32.npz by running the REAL reference autoencoders (src/models/directional_ae.py, src/utils/ae_losses.py)
on the CPU in float64, in the manner of oracle/make_fixtures.py.  Build machine only; only arrays and name lists are written.

    python tools/make_ae_fixture.py --reference /path/to/reference

Noise is pinned as there: torch.nn.functional.dropout is patched for the duration of a reference call so that it consumes the keep
masks recorded in the file.  Everything else (Linear, BatchNorm1d, Embedding, the losses, autograd) is the reference's code and stock
torch.  Parameters are drawn on a coarse grid (tests/ae_oracle.make_codes: int8 codes times a power of two) so that the file holds
them exactly in one byte each; tensors with more than FULL_LIMIT elements are stored as a fixed sample plus their sum and sum of
squares (tests/golden_util.py reads both forms).  Input widths are reduced (the hidden widths are the models').

Per kind ("rna2dna" / "dna2rna"), keys prefixed by it:
  names / shapes                      the reference's state_dict keys and shapes
  code.<key> / scale.<key>            parameters and buffers (value = code * scale)
  rna / dna / site / mask.<name>      a batch of 32 and the dropout keep masks
  s0.out / s0.latent / s0.loss / s0.grad.<key> / s0.after.<buffer>    one training step (forward, loss, backward), buffers afterwards
  eval.both.* / eval.nosite.* / eval.siteonly.*                       eval-mode forwards of the initial state: out and latent"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FULL_LIMIT = 3000
SAMPLE = 1024
DIMS = (50, 44, 6, 20, 32)      # rna, dna, sites, latent, embed
B = 32


def pack(name, arr, out):
    arr = np.asarray(arr)
    if arr.size <= FULL_LIMIT:
        out[name] = arr
        return
    idx = np.sort(np.random.default_rng(sum(map(ord, name))).choice(arr.size, SAMPLE, replace=False))
    flat = arr.reshape(-1).astype(np.float64)
    out[name + "@idx"], out[name + "@val"] = idx.astype(np.int64), flat[idx]
    out[name + "@sum"], out[name + "@sumsq"] = np.float64(flat.sum()), np.float64((flat ** 2).sum())
    out[name + "@shape"] = np.asarray(arr.shape, np.int64)


@contextlib.contextmanager
def injected_masks(mask_list):
    import torch.nn.functional as F
    masks, state, orig = [torch.from_numpy(m.astype(np.float64)) for m in mask_list], {"i": 0}, F.dropout

    def drop(input, p=0.5, training=True, inplace=False):
        if not training:
            return input
        m = masks[state["i"]]
        state["i"] += 1
        assert m.shape == input.shape, (m.shape, input.shape)
        return input * m / (1.0 - p)
    F.dropout = drop
    try:
        yield
    finally:
        F.dropout = orig


def t2n(t):
    return t.detach().cpu().numpy().copy()


def case(kind, seed, out, models, losses, AO):
    A, D, S, L, E = DIMS
    k = kind + "."
    codes, scales = AO.make_codes(seed, kind, A, D, S, L, E)
    P, Bf = AO.decode(codes, scales)
    model = models[kind](A, D, S, L, embed_dim=E).double()
    sd = model.state_dict()
    out[k + "names"] = np.asarray(list(sd))
    out[k + "shapes"] = np.asarray([",".join(str(n) for n in v.shape) for v in sd.values()])
    for key, c in codes.items():
        out[k + "code." + key], out[k + "scale." + key] = c, np.float64(scales[key])
    model.load_state_dict({key: torch.from_numpy(np.asarray(v)) for key, v in list(P.items()) + list(Bf.items())}, strict=True)
    rng = np.random.default_rng(seed + 1)
    rna = rng.standard_normal((B, A))
    dna = rng.uniform(0.02, 0.98, (B, D))
    site = rng.integers(0, S, B).astype(np.int64)
    widths = AO.HIDDEN[kind]
    masks = {n: (rng.random((B, w)) >= 0.1).astype(np.uint8) for n, w in zip(AO.mask_names(kind), widths)}
    out[k + "rna"], out[k + "dna"], out[k + "site"] = rna, dna, site
    for n, m in masks.items():
        out[k + "mask." + n] = m
    x, target = (rna, dna) if kind == "rna2dna" else (dna, rna)
    tx, tt, ts = torch.from_numpy(x), torch.from_numpy(target), torch.from_numpy(site)
    kw = "rna" if kind == "rna2dna" else "dna"
    model.eval()
    with torch.no_grad():
        for tag, args in (("both", {kw: tx, "site": ts}), ("nosite", {kw: tx}), ("siteonly", {"site": ts})):
            rec, lat = model(**args)
            pack(k + f"eval.{tag}.out", t2n(rec), out)
            pack(k + f"eval.{tag}.latent", t2n(lat), out)
    model.train()
    with injected_masks([masks[n] for n in AO.mask_names(kind)]):
        rec, lat = model(**{kw: tx, "site": ts})
        loss, val = losses[kind](rec, tt)
    loss.backward()
    pack(k + "s0.out", t2n(rec), out)
    pack(k + "s0.latent", t2n(lat), out)
    out[k + "s0.loss"] = np.float64(loss.item())
    for key, p in model.named_parameters():
        pack(k + "s0.grad." + key, t2n(p.grad), out)
    for key, v in model.state_dict().items():
        if AO.is_buffer(key):
            out[k + "s0.after." + key] = t2n(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("MMVAE_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ae_b32.npz"))
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit("--reference (or MMVAE_REFERENCE) must name the reference checkout")
    sys.path.insert(0, args.reference)          # `src` resolves to the REFERENCE package in this process
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ae_oracle as AO
    from src.models.directional_ae import RNA2DNAAE, DNA2RNAAE          # reference
    from src.utils.ae_losses import rna2dna_ae_loss, dna2rna_ae_loss    # reference
    torch.set_num_threads(8)
    out = {"dims": np.asarray(DIMS, np.int64), "B": np.int64(B)}
    models = {"rna2dna": RNA2DNAAE, "dna2rna": DNA2RNAAE}
    losses = {"rna2dna": rna2dna_ae_loss, "dna2rna": dna2rna_ae_loss}
    for kind, seed in (("rna2dna", 61), ("dna2rna", 71)):
        case(kind, seed, out, models, losses, AO)
    np.savez_compressed(args.out, **out)
    print(args.out, f"{os.path.getsize(args.out) / 1e6:.2f} MB", {k: float(out[k + '.s0.loss']) for k in models})


if __name__ == "__main__":
    main()
