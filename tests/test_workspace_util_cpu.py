"""tests/workspace_util.py on CPU tensors: the layout and alignment arithmetic of a guarded workspace, the three fills, and that check()
reports a one-byte write into the first and the last byte of either guard with its offset and no write inside the work region."""
import pytest
import torch

import workspace_util as W

SIZES = [8, 24, 4096, 20012 + 4, 65536 + 8]


@pytest.mark.parametrize("phase", [8, 4, 0, 12])
@pytest.mark.parametrize("nbytes", SIZES)
def test_layout_and_alignment(nbytes, phase):
    g = W.guarded(nbytes, "zero", "cpu", phase)
    base = g.buf.data_ptr()
    assert g.nbytes == nbytes and g.work.numel() == nbytes and g.ptr == base + g.start == g.work.data_ptr()
    assert g.ptr % 16 == phase
    assert g.start >= W.GUARD and g.buf.numel() - g.end >= W.GUARD                 # both guards are at least 4096 bytes
    assert g.start - W.GUARD < 16                                                  # and the front one no more than the phase costs
    assert (g.buf[:g.start] == W.GUARD_BYTE).all() and (g.buf[g.end:] == W.GUARD_BYTE).all() and (g.work == 0).all()
    g.check()
    if phase % 8 == 0 and nbytes % 8 == 0:
        t = g.tensor
        assert t.dtype == torch.int64 and t.numel() * 8 == nbytes and t.data_ptr() == g.ptr and t.is_contiguous()
    else:
        with pytest.raises(ValueError):
            g.tensor
    f = g.f32
    assert f.dtype == torch.float32 and f.numel() * 4 == nbytes and f.data_ptr() == g.ptr
    assert (f.data_ptr() // 4) % 2 == (1 if phase in (4, 12) else 0)                # phase 4: the slab starts on an odd float


def test_default_phase_is_eight_bytes_and_no_more():
    g = W.guarded(64, "ones", "cpu")
    assert g.ptr % 16 == 8 and g.ptr % 8 == 0


def test_no_bytes():
    g = W.guarded(0, "ones", "cpu")
    assert g.ptr == 0 and g.tensor is None and g.f32 is None and g.nbytes == 0
    g.check()
    g.buf[g.start] = 0                                                             # the guards meet: still watched
    assert g.first_changed() is not None


def test_fills():
    assert (W.guarded(40, "zero", "cpu").work == 0x00).all()
    assert (W.guarded(40, "ones", "cpu").work == 0xFF).all()
    assert W.guarded(40, "ones", "cpu").tensor.tolist() == [-1] * 5
    img = bytes(range(1, 11))
    g = W.guarded(24, img, "cpu")                                                  # shorter than the region: repeated
    assert bytes(g.work.tolist()) == (img * 3)[:24]
    g = W.guarded(8, img, "cpu")                                                   # longer: its first nbytes bytes
    assert bytes(g.work.tolist()) == img[:8]
    t = torch.arange(6, dtype=torch.float32)                                       # a tensor image: its memory, whatever the dtype
    g = W.guarded(16, t, "cpu")
    assert torch.equal(g.f32, t[:4])
    g = W.guarded(32, t.view(2, 3).t(), "cpu")                                     # made contiguous first: the values in logical order
    assert torch.equal(g.f32[:6], t.view(2, 3).t().contiguous().view(-1)) and torch.equal(g.f32[6:], g.f32[:2])
    g.check()
    with pytest.raises(ValueError):
        W.guarded(8, "poison", "cpu")
    with pytest.raises(ValueError):
        W.guarded(8, b"", "cpu")
    with pytest.raises(TypeError):
        W.guarded(8, 3, "cpu")
    g = W.guarded(16, "zero", "cpu")
    g.fill("ones")                                                                 # refilled in place, the guards stay
    assert (g.work == 0xFF).all()
    g.check()


@pytest.mark.parametrize("nbytes", [8, 4096 + 24])
def test_a_one_byte_write_into_either_end_of_either_guard_is_reported_with_its_offset(nbytes):
    for where, which, offset in ((lambda g: 0, "front", lambda g: -g.start), (lambda g: g.start - 1, "front", lambda g: -1),
                                 (lambda g: g.end, "back", lambda g: 0), (lambda g: g.buf.numel() - 1, "back", lambda g: g.buf.numel() - 1 - g.end)):
        g = W.guarded(nbytes, "ones", "cpu")
        g.buf[where(g)] = W.GUARD_BYTE ^ 0x01                                      # one bit
        assert g.first_changed() == (which, offset(g))
        with pytest.raises(AssertionError, match=f"the {which} guard .* offset {offset(g)} from"):
            g.check("case")
    g = W.guarded(nbytes, "zero", "cpu")                                           # the first changed byte is the one named
    g.buf[g.end + 7] = 0
    g.buf[g.end + 3] = 0
    assert g.first_changed() == ("back", 3)
    g.buf[5] = 0
    assert g.first_changed() == ("front", 5 - g.start)


@pytest.mark.parametrize("fill", ["zero", "ones", bytes([W.GUARD_BYTE])])
def test_writes_inside_the_work_region_are_not_reported(fill):
    g = W.guarded(4096 + 24, fill, "cpu")
    before = g.image()
    g.work[0] = 0x11
    g.work[-1] = 0x22
    g.work[1000:2000] = W.GUARD_BYTE ^ 0xFF
    g.tensor[3] = -12345
    g.f32[-2] = float("nan")
    g.check()
    assert g.first_changed() is None
    assert g.word_changed(0, before) and g.word_changed(g.nbytes - 4, before) and g.word_changed(24, before)
    assert not g.word_changed(8, before) and not g.word_changed(2000, before)
    assert before.data_ptr() != g.work.data_ptr()                                  # image() is a copy
