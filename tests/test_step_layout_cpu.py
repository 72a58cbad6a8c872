"""The layout of what one training step needs zeroed (engine.VAEGraph.zero_pack) and of the flat gradient arena
(engine.carve_arena), built on the CPU device: ONE allocation, regions in a fixed order at 16-byte rounded offsets.  A wrong
layout would not raise on the GPU; it would give wrong gradients."""
import pytest
import torch

import src.models as M
from mmvae import _lib, engine

A, D, S, L = 782, 572, 24, 20
CPU = torch.device("cpu")
F64, F32 = torch.float64, torch.float32
WIDTHS_A, WIDTHS_B = [128], [512, 256]


def _graph(kind):
    model = {"multimodal": M.MultiModalVAE, "dna2rna": M.DNA2RNAVAE, "rna2dna": M.RNA2DNAVAE}[kind](A, D, S, L)
    return model, model._graph()


def _regions(z):
    """The record's tensors in the order of its fields, as (name, tensor)."""
    out = [(f"fwd_stats[{i}]", t) for i, t in enumerate(z.fwd_stats)]
    if z.loss_ws is not None:
        out += [("loss sums", z.loss_ws[0]), ("loss out5", z.loss_ws[1])]
    if z.arena is not None:
        out.append(("arena", z.arena))
    out += [(f"bwd_stats[{i}]", t) for i, t in enumerate(z.bwd_stats)]
    if z.d_table is not None:
        out.append(("d_table", z.d_table))
    return out


def _check_pack(z, want):
    """want: [(shape, dtype)] of every region in order.  Every region is zero, 16-byte aligned, starts where the one before it
    ends (rounded up to 16 bytes) and lies inside the one allocation."""
    got = _regions(z)
    assert [(tuple(t.shape), t.dtype) for _, t in got] == want, [(n, tuple(t.shape), t.dtype) for n, t in got]
    storage = got[0][1].untyped_storage()
    base, end = storage.data_ptr(), storage.data_ptr() + storage.nbytes()
    at = base
    for name, t in got:
        assert t.untyped_storage().data_ptr() == base, name                      # one allocation
        assert t.is_contiguous() and not t.any(), name
        nbytes = t.numel() * t.element_size()
        assert (t.data_ptr() - base) % 16 == 0 and t.data_ptr() == at, (name, t.data_ptr() - base, at - base)
        at = t.data_ptr() + (nbytes + 15) // 16 * 16
    return at - base, end - base


def _stats(widths):
    return [((2, w), F64) for w in widths]


@pytest.mark.parametrize("kind,has_a,has_b,has_site", [
    ("multimodal", True, True, True), ("multimodal", True, False, False), ("multimodal", False, False, True),
    ("dna2rna", False, True, True), ("rna2dna", True, False, True)])
def test_zero_pack_layout(kind, has_a, has_b, has_site):
    model, g = _graph(kind)
    total = sum(p.numel() for p in model.parameters())
    widths = (WIDTHS_A if has_a else []) + (WIDTHS_B if has_b else [])
    table = [((_lib.TABLE_COPIES, S, 2 * L), F32)] if has_site else []
    bwd_half = [((total,), F32)] + _stats(widths) + table

    z = g.zero_pack(CPU, has_a, has_b, has_site, fwd=True, bwd=True)           # training step, backward to follow
    used, size = _check_pack(z, _stats(widths) + [((5,), F64), ((5,), F32)] + bwd_half)
    # a step without the site encoder still reserves one float where the table gradient would be (the max(n_tab, 1) floor)
    assert size == used + (0 if has_site else 16)
    if has_site:
        assert z.d_table.numel() == S * 2 * L * _lib.TABLE_COPIES
    else:
        assert z.d_table is None

    z = g.zero_pack(CPU, has_a, has_b, has_site, fwd=False, bwd=True)          # backward after a forward that zeroed nothing for it
    assert z.fwd_stats == [] and z.loss_ws is None
    _check_pack(z, bwd_half)

    z = g.zero_pack(CPU, has_a, has_b, has_site, fwd=True, bwd=False)          # training forward, no backward to follow
    assert z.loss_ws is None and z.arena is None and z.bwd_stats == [] and z.d_table is None
    if widths:
        _check_pack(z, _stats(widths))


def test_multimodal_sizes():
    model, g = _graph("multimodal")
    params = g.param_list()
    assert len(params) == 39 and sum(p.numel() for p in params) == 1_081_114
    z = g.zero_pack(CPU, True, True, True, fwd=True, bwd=True)
    assert z.arena.numel() == 1_081_114 and z.d_table.numel() == 24 * 40 * _lib.TABLE_COPIES
    assert [tuple(t.shape) for t in z.fwd_stats] == [(2, 128), (2, 512), (2, 256)] == [tuple(t.shape) for t in z.bwd_stats]
    assert tuple(z.loss_ws[0].shape) == (5,) and tuple(z.loss_ws[1].shape) == (5,)
    # the early all-reduce bucket starts at the first large decoder tensor
    views = engine.carve_arena(z.arena, params)
    assert g.early_cut() == 555_216
    assert views[model.decoder_a.fc[2].weight].data_ptr() == z.arena.data_ptr() + 4 * 555_216


@pytest.mark.parametrize("kind", ["multimodal", "dna2rna", "rna2dna"])
def test_arena_views_tile_the_arena_in_param_list_order(kind):
    model, g = _graph(kind)
    params = g.param_list()
    assert {id(p) for p in params} == {id(p) for p in model.parameters()} and len(params) == len(list(model.parameters()))
    flat = torch.zeros(sum(p.numel() for p in params))
    views = engine.carve_arena(flat, params)
    assert len(views) == len(params)
    at = flat.data_ptr()
    for p in params:
        v = views[p]
        assert v.shape == p.shape and v.dtype == F32 and v.is_contiguous() and v.data_ptr() == at
        at += 4 * p.numel()
    assert at == flat.data_ptr() + 4 * flat.numel()
    cut = g.early_cut()
    starts = {views[p].data_ptr() for p in params}
    assert flat.data_ptr() + 4 * cut in starts                                  # the cut falls on a parameter boundary


def test_model_and_graph_are_freed_by_reference_counting():
    """Dropping a model frees its VAEGraph, blocks, block runtimes and parameters at once, and a preparation cache that was used
    keeps nothing of its owner alive (it is handed the owner's bound `build` on every call and must not store it).  A cycle would
    leave a dropped model's gradients and prepared weights in HBM until the cyclic GC happens to run -- possibly in the middle
    of a stream capture."""
    import gc
    import weakref

    class Owner:                                     # what VAEGraph / BlockRuntime are to their cache; nothing to prepare, so no launch
        def __init__(self):
            self.cache = engine.PrepCache()
            self.weight = torch.nn.Parameter(torch.zeros(3))

        def build(self, prec, device):
            return []

    gc.collect()
    gc.disable()
    try:
        owner = Owner()
        owner.cache.ensure(engine.PREC_BF16, CPU, [owner.weight], owner.build)
        assert owner.cache.key is not None
        refs = [weakref.ref(owner), weakref.ref(owner.weight)]
        del owner
        assert all(r() is None for r in refs)
        for kind in ("multimodal", "dna2rna", "rna2dna"):
            model, g = _graph(kind)
            refs = [weakref.ref(g), weakref.ref(g.decoders[0]), weakref.ref(next(model.parameters()))]
            enc = M.EncoderB(D, L)
            enc._block()
            refs += [weakref.ref(enc._rt), weakref.ref(enc.fc_mu.weight)]
            del model, g, enc
            assert all(r() is None for r in refs), kind
    finally:
        gc.enable()
