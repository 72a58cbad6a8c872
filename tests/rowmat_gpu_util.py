"""Operands of the GPU tests of the kernels that read fp32 / bf16 row matrices in place (tests/test_knn_gpu.py, test_silhouette_gpu.py,
test_pca_gpu.py, test_metrics_gpu.py): views of wider NaN-filled buffers and padded bf16 rows with NaN pads, so that a kernel that reads
outside its operand shows it in its result."""
import torch

from mmvae import to_bf16_rows

DEV = "cuda"


def in_nan_frame(x, top, left, right, dtype=torch.float32):
    """x (numpy (M, F)) as a device view of a wider and taller NaN-filled buffer: `left` / `right` NaN columns, `top` NaN rows"""
    M, F = x.shape
    buf = torch.full((M + top + 1, left + F + right), float("nan"), dtype=dtype, device=DEV)
    view = buf[top:top + M, left:left + F]
    view.copy_(torch.from_numpy(x).to(DEV))
    return view


def bf16_rows_nan_pads(x):
    """padded bf16 rows of x with the pad columns overwritten by NaN: the kernel must not read them as data"""
    t = to_bf16_rows(torch.from_numpy(x).to(DEV))
    ld = t.stride(0)
    if ld > t.shape[1]:
        torch.as_strided(t, (t.shape[0], ld - t.shape[1]), (ld, 1), t.storage_offset() + t.shape[1]).fill_(float("nan"))
    return t


def operand(x, bf16, left):
    """left 8: rows on 16-byte boundaries (padded bf16 rows / a frame whose width is a multiple of 64); left 7: rows aligned to one
    element only"""
    if bf16:
        return bf16_rows_nan_pads(x) if left == 8 else in_nan_frame(x, 2, left, 3, torch.bfloat16)
    return in_nan_frame(x, 2, left, 64 - (left + x.shape[1]) % 64 if left == 8 else 3)
