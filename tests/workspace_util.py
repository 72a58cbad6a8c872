"""A caller-owned workspace between two guards, for the tests of the workspace contract of include/mmvae_hip.h: an entry point needs no
more than its planner says (`work_bytes` / `slab_elems`), assumes nothing about the contents and writes nothing outside.

    [ front guard: >= 4096 bytes of 0xA5 | work: exactly nbytes, filled as asked | back guard: >= 4096 bytes of 0xA5 ]

The work region starts at an address that is `phase` modulo 16: 8 by default, the 8-byte alignment the header promises for `work` and no
more; 4 puts a float slab on an odd float (the header gives a slab the alignment of a float).  Works on CPU tensors too
(tests/test_workspace_util_cpu.py)."""
import torch

GUARD = 4096
GUARD_BYTE = 0xA5
FILLS = ("zero", "ones")            # and a bytes / tensor image


def as_bytes(image):
    """a bytes object or a tensor (any dtype, any device) as a flat uint8 tensor of its memory image"""
    if isinstance(image, (bytes, bytearray)):
        return torch.frombuffer(bytearray(image), dtype=torch.uint8)
    if isinstance(image, torch.Tensor):
        return image.detach().contiguous().reshape(-1).view(torch.uint8)
    raise TypeError(f"a fill is 'zero', 'ones', bytes or a tensor, not {type(image).__name__}")


class Guarded:
    def __init__(self, nbytes, fill, device, phase=8):
        nbytes = int(nbytes)
        if nbytes < 0 or phase % 4 or not 0 <= phase < 16:
            raise ValueError(f"guarded: nbytes = {nbytes}, phase = {phase}")
        self.nbytes, self.phase = nbytes, phase
        self.buf = torch.full((2 * GUARD + nbytes + 16,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.start = GUARD + (phase - self.buf.data_ptr() - GUARD) % 16           # the first offset >= GUARD at the asked phase
        self.end = self.start + nbytes
        assert self.start >= GUARD and self.buf.numel() - self.end >= GUARD and (self.buf.data_ptr() + self.start) % 16 == phase
        self.fill(fill)

    # ---- the work region ---------------------------------------------------------------------
    @property
    def work(self):
        """the work region, uint8 (nbytes,)"""
        return self.buf[self.start:self.end]

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.start if self.nbytes else 0

    @property
    def tensor(self):
        """the work region as the int64 tensor the `work=` keywords of mmvae.ops take; None for 0 bytes"""
        if not self.nbytes:
            return None
        if self.nbytes % 8 or self.phase % 8:
            raise ValueError(f"guarded: {self.nbytes} bytes at phase {self.phase} are no whole int64 elements")
        return self.work.view(torch.int64)

    @property
    def f32(self):
        """the work region as the float32 tensor the `slab=` keywords take; None for 0 bytes"""
        if not self.nbytes:
            return None
        if self.nbytes % 4:
            raise ValueError(f"guarded: {self.nbytes} bytes are no whole floats")
        return self.work.view(torch.float32)

    def fill(self, fill):
        """'zero': 0x00, 'ones': 0xFF, or an image (bytes / tensor): its first min(len, nbytes) bytes, repeated if it is shorter"""
        if isinstance(fill, str):
            if fill not in FILLS:
                raise ValueError(f"guarded: fill {fill!r} is none of {FILLS} and no image")
            self.work.fill_(0x00 if fill == "zero" else 0xFF)
            return
        img = as_bytes(fill)
        if self.nbytes and not img.numel():
            raise ValueError("guarded: an empty image")
        if self.nbytes:
            reps = -(-self.nbytes // img.numel())
            self.work.copy_((img.repeat(reps) if reps > 1 else img)[:self.nbytes].to(self.buf.device))

    def image(self):
        """a copy of the work region's bytes"""
        return self.work.clone()

    def word_changed(self, byte_offset, since):
        """does the 4-byte word at byte_offset of the work region differ from the same word of the image `since`?"""
        assert 0 <= byte_offset and byte_offset + 4 <= self.nbytes
        return not torch.equal(self.work[byte_offset:byte_offset + 4], since[byte_offset:byte_offset + 4])

    # ---- the guards --------------------------------------------------------------------------
    def first_changed(self):
        """None, or (which guard, offset): the first changed byte of the front guard as a NEGATIVE offset from the start of the work
        region (-1: the byte just in front of it), of the back guard as an offset from its end (0: the byte just behind it)"""
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)
        for which, lo, hi, origin in (("front", 0, self.start, self.start), ("back", self.end, self.buf.numel(), self.end)):
            bad = torch.nonzero(self.buf[lo:hi] != GUARD_BYTE)
            if bad.numel():
                return which, lo + int(bad[0]) - origin
        return None

    def check(self, label=""):
        bad = self.first_changed()
        assert bad is None, (f"{label}: the {bad[0]} guard of a {self.nbytes}-byte workspace was written; first changed byte at offset {bad[1]} "
                             f"from the {'start' if bad[0] == 'front' else 'end'} of the work region")


def guarded(nbytes, fill, device, phase=8):
    return Guarded(nbytes, fill, device, phase)
