"""What the evaluation wrappers of mmvae.ops refuse in Python, before any launch: one table of malformed calls per wrapper (a transposed
view, rows that overlap, a wrong dtype, a wrong width, outputs of the wrong shape or stride, a short workspace, k / splits out of range,
misaligned LayerNorm operands) and the exception type each raises.  Operands are at most 8 x 8 (more rows only where an entry must need a
workspace to be given a short one: 33 x 8 for the LayerNorm backward and two row splits of the scatter matrix, 5000 training rows for
the split lists of the manhattan search); a call that got as far as asking for the launch stream fails the test, whatever it raises."""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvae import _lib, ops  # noqa: E402

DEV = "cuda"
F32, BF16, F64, I32, I64, U8 = torch.float32, torch.bfloat16, torch.float64, torch.int32, torch.int64, torch.uint8


def z(*shape, dt=F32):
    return torch.zeros(*shape, dtype=dt, device=DEV)


def transposed(rows, cols, dt=F32):
    """(rows, cols) with strides (1, rows)"""
    return z(cols, rows, dt=dt).t()


def expanded(rows, cols, dt=F32):
    """(rows, cols) with stride(0) = 0: every row is the same memory"""
    return z(1, cols, dt=dt).expand(rows, cols)


def inner2(rows, cols, dt=F32):
    """(rows, cols) with inner stride 2"""
    return z(rows, 2 * cols, dt=dt)[:, ::2]


def every_other(n, dt=F32):
    """(n,) with stride 2"""
    return z(2 * n, dt=dt)[::2]


def off_by_one(rows, cols, dt=F32):
    """a contiguous (rows, cols) matrix one element past an aligned base"""
    return z(rows * cols + 1, dt=dt)[1:].view(rows, cols)


@functools.lru_cache(maxsize=None)
def good():
    """well-formed operands, never written to: every call below is refused"""
    g = types.SimpleNamespace()
    g.x, g.t, g.y2 = z(8, 8), z(8, 8), z(8, 2)
    g.shift = z(8)
    g.idx, g.dist = z(8, 5, dt=I32), z(8, 5)
    g.class_start = torch.tensor([0, 4, 8], dtype=I32, device=DEV)
    g.order = torch.arange(8, dtype=I32, device=DEV)
    g.v = z(2, 8)
    g.row_ptr, g.col, g.val = z(9, dt=I32), z(4, dt=I32), z(4)
    g.col_acc, g.vec = z(4, 8, dt=F64), z(8)
    g.gamma, g.beta, g.mask = z(8), z(8), z(8, 8, dt=U8)
    g.logits, g.labels = z(8, 4), z(8, dt=I64)
    return g


def _short(nbytes):
    """a workspace one element short of nbytes (the sizes below all need one)"""
    assert nbytes >= 8
    return z((nbytes + 7) // 8 - 1, dt=I64)


def recon_metrics_cases(g):
    f = ops.recon_metrics
    ok = (g.shift, g.col_acc, g.vec, g.vec.clone())
    return [("target_transposed", ValueError, lambda: f(g.x, transposed(8, 8), *ok)),
            ("target_expanded", ValueError, lambda: f(g.x, expanded(8, 8), *ok)),
            ("pred_transposed", ValueError, lambda: f(transposed(8, 8), g.t, *ok)),
            ("pred_expanded", ValueError, lambda: f(expanded(8, 8), g.t, *ok)),
            ("pred_inner_stride", ValueError, lambda: f(inner2(8, 8), g.t, *ok)),
            ("target_dtype", TypeError, lambda: f(g.x, z(8, 8, dt=F64), *ok)),
            ("pred_dtype", TypeError, lambda: f(z(8, 8, dt=torch.float16), g.t, *ok)),
            ("pred_cols", ValueError, lambda: f(z(8, 7), g.t, *ok)),
            ("pred_rows", ValueError, lambda: f(z(7, 8), g.t, *ok)),
            ("pred_row_length", ValueError, lambda: f(z(7), g.t, *ok)),
            ("pred_row_stride", ValueError, lambda: f(every_other(8), g.t, *ok)),
            ("empty_target", ValueError, lambda: f(z(0, 8), z(0, 8), *ok)),
            ("col_shift_length", ValueError, lambda: f(g.x, g.t, z(7), *ok[1:])),
            ("col_acc_shape", ValueError, lambda: f(g.x, g.t, g.shift, z(3, 8, dt=F64), g.vec, g.vec)),
            ("col_acc_dtype", ValueError, lambda: f(g.x, g.t, g.shift, z(4, 8), g.vec, g.vec)),
            ("row_pearson_length", ValueError, lambda: f(g.x, g.t, g.shift, g.col_acc, z(7), g.vec)),
            ("row_cosine_stride", ValueError, lambda: f(g.x, g.t, g.shift, g.col_acc, g.vec, every_other(8)))]


def _search_cases(f, dist_name, with_shift, work_bytes):
    def cases(g):
        out = [("q_transposed", ValueError, lambda: f(transposed(8, 8), g.t, 5)),
               ("q_expanded", ValueError, lambda: f(expanded(8, 8), g.t, 5)),
               ("t_transposed", ValueError, lambda: f(g.x, transposed(8, 8), 5)),
               ("t_expanded", ValueError, lambda: f(g.x, expanded(8, 8), 5)),
               ("q_dtype", ValueError, lambda: f(z(8, 8, dt=F64), g.t, 5)),
               ("t_dtype", ValueError, lambda: f(g.x, z(8, 8, dt=torch.float16), 5)),
               ("q_one_dimensional", ValueError, lambda: f(z(8), g.t, 5)),
               ("t_cols", ValueError, lambda: f(g.x, z(8, 7), 5)),
               ("k_zero", ValueError, lambda: f(g.x, g.t, 0)),
               ("k_above_rows", ValueError, lambda: f(g.x, g.t, 9)),
               ("k_above_max", ValueError, lambda: f(g.x, g.t, _lib.KNN_MAXK + 1)),
               ("idx_out_shape", ValueError, lambda: f(g.x, g.t, 5, idx_out=z(8, 4, dt=I32))),
               ("idx_out_dtype", ValueError, lambda: f(g.x, g.t, 5, idx_out=z(8, 5, dt=I64))),
               ("idx_out_inner_stride", ValueError, lambda: f(g.x, g.t, 5, idx_out=inner2(8, 5, I32))),
               ("idx_out_expanded", ValueError, lambda: f(g.x, g.t, 5, idx_out=expanded(8, 5, I32))),
               ("dist_out_shape", ValueError, lambda: f(g.x, g.t, 5, **{dist_name: z(7, 5)})),
               ("dist_out_dtype", ValueError, lambda: f(g.x, g.t, 5, **{dist_name: z(8, 5, dt=F64)})),
               ("dist_out_inner_stride", ValueError, lambda: f(g.x, g.t, 5, **{dist_name: inner2(8, 5)})),
               # 3 queries among 5000 rows: the training rows are split and both searches need a workspace for the lists
               ("work_short", ValueError, lambda: f(z(3, 8), z(5000, 8), 5, work=_short(work_bytes(3, 5000, 5)))),
               ("work_dtype", ValueError, lambda: f(g.x, g.t, 5, work=z(1024, dt=I32))),
               ("work_strided", ValueError, lambda: f(g.x, g.t, 5, work=every_other(1024, I64)))]
        if with_shift:
            out += [("shift_length", ValueError, lambda: f(g.x, g.t, 5, z(7))),
                    ("shift_dtype", ValueError, lambda: f(g.x, g.t, 5, z(8, dt=BF16))),
                    ("shift_stride", ValueError, lambda: f(g.x, g.t, 5, every_other(8)))]
        return out
    return cases


def knn_search_grouped_cases(g):
    f = ops.knn_search_grouped
    codes = (z(8, dt=I32), z(8, dt=I32))
    return [("no_codes", ValueError, lambda: f(g.x, g.t, 5)),
            ("metric", ValueError, lambda: f(g.x, g.t, 5, differ=codes, metric="cosine")),
            ("half_a_pair", ValueError, lambda: f(g.x, g.t, 5, same=(codes[0],))),
            ("codes_length", ValueError, lambda: f(g.x, g.t, 5, differ=(codes[0], z(7, dt=I32)))),
            ("codes_dtype", ValueError, lambda: f(g.x, g.t, 5, same=(z(8, dt=I64), codes[1]))),
            ("manhattan_shift", ValueError, lambda: f(g.x, g.t, 5, differ=codes, metric="manhattan", shift=g.shift)),
            ("k_above_rows", ValueError, lambda: f(g.x, g.t, 9, differ=codes)),
            ("t_cols", ValueError, lambda: f(g.x, z(8, 7), 5, differ=codes)),
            ("work_short_euclidean", ValueError, lambda: f(g.x, g.t, 5, differ=codes, work=_short(ops.knn_group_work_bytes(8, 8, 5)))),
            ("work_short_manhattan", ValueError,
             lambda: f(g.x, g.t, 5, same=codes, metric="manhattan", work=_short(ops.knn_group_work_bytes(8, 8, 5, "manhattan")))),
            ("work_dtype", ValueError, lambda: f(g.x, g.t, 5, differ=codes, work=z(1024, dt=I32)))]


def _rows_cases(f, weighted):
    def cases(g):
        def call(idx=g.idx, y=g.x, out=None, dist=g.dist):
            return f(idx, dist, y, True, out) if weighted else f(idx, y, out)
        out = [("y_transposed", ValueError, lambda: call(y=transposed(8, 8))),
               ("y_expanded", ValueError, lambda: call(y=expanded(8, 8))),
               ("y_dtype", ValueError, lambda: call(y=z(8, 8, dt=F64))),
               ("idx_dtype", ValueError, lambda: call(idx=z(8, 5, dt=I64))),
               ("idx_transposed", ValueError, lambda: call(idx=transposed(8, 5, I32))),
               ("idx_one_dimensional", ValueError, lambda: call(idx=z(8, dt=I32))),
               ("idx_no_columns", ValueError, lambda: call(idx=z(8, 0, dt=I32))),
               ("out_shape", ValueError, lambda: call(out=z(8, 7))),
               ("out_rows", ValueError, lambda: call(out=z(7, 8))),
               ("out_dtype", ValueError, lambda: call(out=z(8, 8, dt=BF16))),
               ("out_inner_stride", ValueError, lambda: call(out=inner2(8, 8))),
               ("out_expanded", ValueError, lambda: call(out=expanded(8, 8)))]
        if weighted:
            out += [("dist_shape", ValueError, lambda: call(dist=z(8, 4))),
                    ("dist_dtype", ValueError, lambda: call(dist=z(8, 5, dt=BF16))),
                    ("dist_transposed", ValueError, lambda: call(dist=transposed(8, 5)))]
        return out
    return cases


def silhouette_cases(g):
    f = ops.silhouette_samples
    return [("x_transposed", ValueError, lambda: f(transposed(8, 8), g.order, g.class_start)),
            ("x_expanded", ValueError, lambda: f(expanded(8, 8), g.order, g.class_start)),
            ("x_dtype", ValueError, lambda: f(z(8, 8, dt=F64), g.order, g.class_start)),
            ("x_one_row", ValueError, lambda: f(z(1, 8), None, g.class_start)),
            ("class_start_two_dimensional", ValueError, lambda: f(g.x, g.order, z(3, 1, dt=I32))),
            ("class_start_dtype", ValueError, lambda: f(g.x, g.order, z(3, dt=I64))),
            ("class_start_no_class", ValueError, lambda: f(g.x, g.order, z(1, dt=I32))),
            ("class_start_stride", ValueError, lambda: f(g.x, g.order, every_other(3, I32))),
            ("order_length", ValueError, lambda: f(g.x, z(7, dt=I32), g.class_start)),
            ("order_dtype", ValueError, lambda: f(g.x, z(8, dt=I64), g.class_start)),
            ("shift_length", ValueError, lambda: f(g.x, g.order, g.class_start, z(7))),
            ("splits_above", ValueError, lambda: f(g.x, g.order, g.class_start, splits=65)),
            ("splits_negative", ValueError, lambda: f(g.x, g.order, g.class_start, splits=-1)),
            ("s_out_length", ValueError, lambda: f(g.x, g.order, g.class_start, s_out=z(7))),
            ("intra_out_dtype", ValueError, lambda: f(g.x, g.order, g.class_start, intra_out=z(8, dt=F64))),
            ("inter_out_stride", ValueError, lambda: f(g.x, g.order, g.class_start, inter_out=every_other(8))),
            ("work_short", ValueError, lambda: f(g.x, g.order, g.class_start, work=_short(ops.silhouette_work_bytes(8, 2)))),
            ("work_short_split", ValueError, lambda: f(g.x, g.order, g.class_start, splits=2, work=_short(ops.silhouette_work_bytes(8, 2, 2)))),
            ("work_dtype", ValueError, lambda: f(g.x, g.order, g.class_start, work=z(1024, dt=I32)))]


def pca_scatter_cases(g):
    f = ops.pca_scatter
    return [("x_transposed", ValueError, lambda: f(transposed(8, 8), g.shift)),
            ("x_expanded", ValueError, lambda: f(expanded(8, 8), g.shift)),
            ("x_dtype", ValueError, lambda: f(z(8, 8, dt=F64), g.shift)),
            ("shift_length", ValueError, lambda: f(g.x, z(7))),
            ("shift_dtype", ValueError, lambda: f(g.x, z(8, dt=F64))),
            ("splits_above", ValueError, lambda: f(g.x, g.shift, 65)),
            ("splits_negative", ValueError, lambda: f(g.x, g.shift, -1)),
            ("out_shape", ValueError, lambda: f(g.x, g.shift, out=z(8, 7))),
            ("out_dtype", ValueError, lambda: f(g.x, g.shift, out=z(8, 8, dt=F64))),
            ("out_inner_stride", ValueError, lambda: f(g.x, g.shift, out=inner2(8, 8))),
            ("out_expanded", ValueError, lambda: f(g.x, g.shift, out=expanded(8, 8))),
            # 33 rows are two chunks of 32: the fewest at which two row splits, and with them a workspace, exist
            ("work_short", ValueError, lambda: f(z(33, 8), g.shift, 2, work=_short(ops.pca_scatter_work_bytes(33, 8, 2)))),
            ("work_dtype", ValueError, lambda: f(g.x, g.shift, work=z(1024, dt=I32)))]


def pca_project_cases(g):
    f = ops.pca_project
    return [("x_transposed", ValueError, lambda: f(transposed(8, 8), g.shift, g.v)),
            ("x_expanded", ValueError, lambda: f(expanded(8, 8), g.shift, g.v)),
            ("x_dtype", ValueError, lambda: f(z(8, 8, dt=F64), g.shift, g.v)),
            ("shift_length", ValueError, lambda: f(g.x, z(7), g.v)),
            ("v_cols", ValueError, lambda: f(g.x, g.shift, z(2, 7))),
            ("v_bf16", ValueError, lambda: f(g.x, g.shift, z(2, 8, dt=BF16))),
            ("v_transposed", ValueError, lambda: f(g.x, g.shift, transposed(2, 8))),
            ("v_expanded", ValueError, lambda: f(g.x, g.shift, expanded(2, 8))),
            ("out_shape", ValueError, lambda: f(g.x, g.shift, g.v, out=z(8, 3))),
            ("out_inner_stride", ValueError, lambda: f(g.x, g.shift, g.v, out=inner2(8, 2)))]


def tsne_affinities_cases(g):
    f = ops.tsne_affinities
    return [("dist2_transposed", ValueError, lambda: f(transposed(8, 5), 2.0)),
            ("dist2_expanded", ValueError, lambda: f(expanded(8, 5), 2.0)),
            ("dist2_dtype", ValueError, lambda: f(z(8, 5, dt=BF16), 2.0)),
            ("dist2_one_dimensional", ValueError, lambda: f(z(8), 2.0)),
            ("perplexity_zero", ValueError, lambda: f(g.dist, 0.0)),
            ("perplexity_k", ValueError, lambda: f(g.dist, 5.0)),
            ("p_out_shape", ValueError, lambda: f(g.dist, 2.0, p_out=z(8, 4))),
            ("p_out_inner_stride", ValueError, lambda: f(g.dist, 2.0, p_out=inner2(8, 5))),
            ("beta_out_length", ValueError, lambda: f(g.dist, 2.0, beta_out=z(7))),
            ("beta_out_stride", ValueError, lambda: f(g.dist, 2.0, beta_out=every_other(8)))]


def tsne_gradient_cases(g):
    f = ops.tsne_gradient
    csr = (g.row_ptr, g.col, g.val)
    return [("y_transposed", ValueError, lambda: f(transposed(8, 2), *csr)),
            ("y_expanded", ValueError, lambda: f(expanded(8, 2), *csr)),
            ("y_dtype", ValueError, lambda: f(z(8, 2, dt=BF16), *csr)),
            ("y_cols", ValueError, lambda: f(z(8, 3), *csr)),
            ("y_row_stride", ValueError, lambda: f(z(8, 4)[:, :2], *csr)),
            ("y_one_row", ValueError, lambda: f(z(1, 2), z(2, dt=I32), g.col, g.val)),
            ("row_ptr_length", ValueError, lambda: f(g.y2, z(8, dt=I32), g.col, g.val)),
            ("row_ptr_dtype", ValueError, lambda: f(g.y2, z(9, dt=I64), g.col, g.val)),
            ("col_dtype", ValueError, lambda: f(g.y2, g.row_ptr, z(4, dt=I64), g.val)),
            ("col_two_dimensional", ValueError, lambda: f(g.y2, g.row_ptr, z(4, 1, dt=I32), g.val)),
            ("val_length", ValueError, lambda: f(g.y2, g.row_ptr, g.col, z(3))),
            ("val_stride", ValueError, lambda: f(g.y2, g.row_ptr, g.col, every_other(4))),
            ("splits_above", ValueError, lambda: f(g.y2, *csr, splits=65)),
            ("grad_out_shape", ValueError, lambda: f(g.y2, *csr, grad_out=z(7, 2))),
            ("grad_out_row_stride", ValueError, lambda: f(g.y2, *csr, grad_out=z(8, 4)[:, :2])),
            ("work_short", ValueError, lambda: f(g.y2, *csr, work=_short(ops.tsne_gradient_work_bytes(8)))),
            ("work_dtype", ValueError, lambda: f(g.y2, *csr, work=z(1024, dt=I32)))]


def tsne_update_cases(g):
    f = ops.tsne_update
    y = (g.y2,) * 4
    return [("y_transposed", ValueError, lambda: f(transposed(8, 2), *y[1:], 0.5, 1.0)),
            ("y_cols", ValueError, lambda: f(z(8, 3), *y[1:], 0.5, 1.0)),
            ("update_rows", ValueError, lambda: f(g.y2, z(7, 2), g.y2, g.y2, 0.5, 1.0)),
            ("gains_row_stride", ValueError, lambda: f(g.y2, g.y2, z(8, 4)[:, :2], g.y2, 0.5, 1.0)),
            ("gains_expanded", ValueError, lambda: f(g.y2, g.y2, expanded(8, 2), g.y2, 0.5, 1.0)),
            ("grad_dtype", ValueError, lambda: f(g.y2, g.y2, g.y2, z(8, 2, dt=BF16), 0.5, 1.0)),
            ("work_short", ValueError, lambda: f(*y, 0.5, 1.0, grad_norm=True, work=_short(ops.tsne_update_work_bytes(8)))),
            ("work_dtype", ValueError, lambda: f(*y, 0.5, 1.0, grad_norm=True, work=z(1024, dt=I32)))]


def ln_act_fwd_cases(g):
    f = ops.ln_act_fwd
    return [("z_transposed", ValueError, lambda: f(transposed(8, 8))),
            ("z_expanded", ValueError, lambda: f(expanded(8, 8))),
            ("z_dtype", ValueError, lambda: f(z(8, 8, dt=BF16))),
            ("z_width", ValueError, lambda: f(z(8, 6))),
            ("z_base_misaligned", ValueError, lambda: f(off_by_one(8, 8))),
            ("z_row_stride", ValueError, lambda: f(z(8, 10)[:, :8])),
            ("gamma_alone", ValueError, lambda: f(g.x, g.gamma)),
            ("gamma_length", ValueError, lambda: f(g.x, z(7), g.beta)),
            ("gamma_misaligned", ValueError, lambda: f(g.x, z(9)[1:], g.beta)),
            ("beta_stride", ValueError, lambda: f(g.x, g.gamma, every_other(8))),
            ("y_out_shape", ValueError, lambda: f(g.x, y_out=z(8, 4))),
            ("y_out_base_misaligned", ValueError, lambda: f(g.x, y_out=off_by_one(8, 8))),
            ("y_out_row_stride", ValueError, lambda: f(g.x, y_out=z(8, 10)[:, :8])),
            ("y_out_inner_stride", ValueError, lambda: f(g.x, y_out=inner2(8, 8))),
            ("mean_out_length", ValueError, lambda: f(g.x, g.gamma, g.beta, mean_out=z(7))),
            ("rstd_out_stride", ValueError, lambda: f(g.x, g.gamma, g.beta, rstd_out=every_other(8))),
            ("mask_dtype", ValueError, lambda: f(g.x, mask=z(8, 8, dt=torch.bool), p=0.5)),
            ("mask_shape", ValueError, lambda: f(g.x, mask=z(8, 4, dt=U8), p=0.5)),
            ("mask_base_misaligned", ValueError, lambda: f(g.x, mask=off_by_one(8, 8, U8), p=0.5)),
            ("mask_row_stride", ValueError, lambda: f(g.x, mask=z(8, 10, dt=U8)[:, :8], p=0.5)),
            ("p_one", ValueError, lambda: f(g.x, mask=g.mask, p=1.0))]


def ln_act_bwd_cases(g):
    f = ops.ln_act_bwd
    ln = (g.vec, g.vec, g.gamma, g.beta)
    return [("z_transposed", ValueError, lambda: f(g.x, transposed(8, 8))),
            ("z_width", ValueError, lambda: f(z(8, 6), z(8, 6))),
            ("z_base_misaligned", ValueError, lambda: f(g.x, off_by_one(8, 8))),
            ("dy_rows", ValueError, lambda: f(z(7, 8), g.x)),
            ("dy_expanded", ValueError, lambda: f(expanded(8, 8), g.x)),
            ("dy_dtype", ValueError, lambda: f(z(8, 8, dt=BF16), g.x)),
            ("dy_base_misaligned", ValueError, lambda: f(off_by_one(8, 8), g.x)),
            ("dy_row_stride", ValueError, lambda: f(z(8, 10)[:, :8], g.x)),
            ("dz_out_shape", ValueError, lambda: f(g.x, g.x, dz_out=z(4, 8))),
            ("dz_out_base_misaligned", ValueError, lambda: f(g.x, g.x, dz_out=off_by_one(8, 8))),
            ("mean_missing", ValueError, lambda: f(g.x, g.x, None, g.vec, g.gamma, g.beta)),
            ("rstd_length", ValueError, lambda: f(g.x, g.x, g.vec, z(7), g.gamma, g.beta)),
            ("beta_missing", ValueError, lambda: f(g.x, g.x, g.vec, g.vec, g.gamma, None)),
            ("gamma_misaligned", ValueError, lambda: f(g.x, g.x, g.vec, g.vec, z(9)[1:], g.beta)),
            ("dgamma_out_length", ValueError, lambda: f(g.x, g.x, *ln, dgamma_out=z(7))),
            ("dbeta_out_dtype", ValueError, lambda: f(g.x, g.x, *ln, dbeta_out=z(8, dt=F64))),
            ("mask_base_misaligned", ValueError, lambda: f(g.x, g.x, mask=off_by_one(8, 8, U8), p=0.5)),
            # 33 rows: the fewest at which the LayerNorm backward needs a workspace at all
            ("work_short", ValueError, lambda: f(z(33, 8), z(33, 8), z(33), z(33), g.gamma, g.beta, work=_short(ops.ln_act_bwd_work_bytes(33, 8, True)))),
            ("work_dtype", ValueError, lambda: f(g.x, g.x, *ln, work=z(1024, dt=I32)))]


def wce_mean_cases(g):
    f = ops.wce_mean
    sums = z(3, dt=F64)
    return [("logits_transposed", ValueError, lambda: f(transposed(8, 4), g.labels, sums=sums)),
            ("logits_expanded", ValueError, lambda: f(expanded(8, 4), g.labels, sums=sums)),
            ("logits_dtype", ValueError, lambda: f(z(8, 4, dt=BF16), g.labels, sums=sums)),
            ("one_class", ValueError, lambda: f(z(8, 1), g.labels, sums=sums)),
            ("labels_dtype", ValueError, lambda: f(g.logits, z(8, dt=I32), sums=sums)),
            ("labels_length", ValueError, lambda: f(g.logits, z(7, dt=I64), sums=sums)),
            ("class_weights_length", ValueError, lambda: f(g.logits, g.labels, z(3), sums=sums)),
            ("sums_dtype", ValueError, lambda: f(g.logits, g.labels, sums=z(3))),
            ("sums_length", ValueError, lambda: f(g.logits, g.labels, sums=z(2, dt=F64))),
            ("grad_out_shape", ValueError, lambda: f(g.logits, g.labels, grad_out=z(8, 3))),
            ("grad_out_inner_stride", ValueError, lambda: f(g.logits, g.labels, grad_out=inner2(8, 4))),
            ("pred_out_dtype", ValueError, lambda: f(g.logits, g.labels, pred_out=z(8, dt=I64))),
            ("pred_out_stride", ValueError, lambda: f(g.logits, g.labels, pred_out=every_other(8, I32))),
            ("confusion_shape", ValueError, lambda: f(g.logits, g.labels, confusion=z(4, 3, dt=I32))),
            ("confusion_dtype", ValueError, lambda: f(g.logits, g.labels, confusion=z(4, 4, dt=I64))),
            ("no_output", ValueError, lambda: f(g.logits, g.labels))]


TABLES = {"recon_metrics": recon_metrics_cases,
          "knn_search": _search_cases(ops.knn_search, "dist2_out", True, ops.knn_work_bytes),
          "knn_search_l1": _search_cases(ops.knn_search_l1, "dist_out", False, ops.knn_l1_work_bytes),
          "knn_search_grouped": knn_search_grouped_cases,
          "knn_mean_rows": _rows_cases(ops.knn_mean_rows, False),
          "knn_weighted_rows": _rows_cases(ops.knn_weighted_rows, True),
          "silhouette_samples": silhouette_cases,
          "pca_scatter": pca_scatter_cases,
          "pca_project": pca_project_cases,
          "tsne_affinities": tsne_affinities_cases,
          "tsne_gradient": tsne_gradient_cases,
          "tsne_update": tsne_update_cases,
          "ln_act_fwd": ln_act_fwd_cases,
          "ln_act_bwd": ln_act_bwd_cases,
          "wce_mean": wce_mean_cases}


@pytest.mark.parametrize("wrapper", sorted(TABLES))
def test_malformed_calls_are_refused_before_a_launch(wrapper, monkeypatch):
    def no_launch():
        raise AssertionError(f"{wrapper}: the call reached its launch")
    monkeypatch.setattr(ops, "_stream", no_launch)              # every launch asks for the stream while its arguments are evaluated
    cases = TABLES[wrapper](good())
    assert len({name for name, _, _ in cases}) == len(cases)
    wrong = []
    for name, exc, call in cases:
        try:
            call()
            got = None
        except Exception as e:          # noqa: BLE001 -- the type is what is compared
            got = type(e)
        if got is not exc:
            wrong.append((name, exc.__name__, getattr(got, "__name__", "accepted")))
    assert not wrong, wrong
