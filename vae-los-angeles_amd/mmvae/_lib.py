"""ctypes binding of libmmvae_hip.so (C ABI declared in include/mmvae_hip.h).

The product path has NO fallback: if the shared library is missing or its ABI version does
not match, importing the kernels raises.  Build it with `python __graft_entry__.py` (or
`make -C vae-los-angeles_amd/csrc`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMVAE_LIB_PATH") or os.path.join(_HERE, "libmmvae_hip.so")     # override: experimental builds
ABI_VERSION = 20

F32, BF16 = 0, 1
PREC_F32, PREC_BF16 = 0, 1
PRO_NONE, PRO_BN_RELU_DROP, PRO_BN_BWD_APPLY = 0, 1, 2
TABLE_COPIES = 8          # MMVAE_TABLE_COPIES
EPI_STORE, EPI_RELU_MASK, EPI_BN_BWD, EPI_LOSS_MSE, EPI_LOSS_BCE_LOGIT = 0, 1, 2, 3, 4
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
TILE = 128
TN_GROUP_MAX = 8        # MMVAE_TN_GROUP_MAX
KNN_MAXK = 96           # MMVAE_KNN_MAXK
SIL_MAXC = 64           # MMVAE_SIL_MAXC
PCA_MAXK = 64           # MMVAE_PCA_MAXK
LN_MAXN = 1024          # MMVAE_LN_MAXN
WCE_MAXC = 64           # MMVAE_WCE_MAXC
STD_MAX_PARTS = 4       # MMVAE_STD_MAX_PARTS
CTR_COPIES = 16384      # MMVAE_CTR_COPIES: self-advancing device counters are stored as this many identical int64 copies

i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class PrepItem(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("src_rows", i32), ("src_cols", i32), ("src_ld", i64),
                ("dst_rows", i32), ("dst_cols", i32), ("dst_ld", i64), ("transpose", i32), ("dst_dtype", i32)]


class GemmNtArgs(C.Structure):
    _fields_ = [("prec", i32), ("M", i32), ("N", i32), ("K", i32),
                ("a", vp), ("a_dtype", i32), ("lda", i64),
                ("prologue", i32),
                ("pro_scale", vp), ("pro_shift", vp), ("pro_mask", vp), ("ld_pro_mask", i64), ("pro_inv_keep", f32),
                ("w", vp), ("ldw", i64),
                ("epilogue", i32),
                ("c", vp), ("c_dtype", i32), ("ldc", i64),
                ("bias", vp), ("act", i32), ("accumulate", i32),
                ("h", vp), ("ldh", i64),
                ("bn_scale", vp), ("bn_shift", vp), ("bn_mean", vp), ("bn_rstd", vp),
                ("epi_mask", vp), ("ld_epi_mask", i64), ("epi_inv_keep", f32),
                ("bn_coef", vp), ("bn_phase", i32),
                ("stat1", vp), ("stat2", vp),
                ("pro_out", vp), ("ld_pro_out", i64), ("pro_finalize", vp), ("h_dtype", i32)]


class GemmTnArgs(C.Structure):
    _fields_ = [("prec", i32), ("M", i32), ("N", i32), ("K", i32),
                ("p", vp), ("p_dtype", i32), ("ldp", i64),
                ("q", vp), ("q_dtype", i32), ("ldq", i64),
                ("q_prologue", i32),
                ("pro_scale", vp), ("pro_shift", vp), ("pro_mask", vp), ("ld_pro_mask", i64), ("pro_inv_keep", f32),
                ("dw", vp), ("lddw", i64), ("db", vp),
                ("nsplit", i32), ("slab", vp), ("slab_elems", i64),
                ("p_prologue", i32), ("p_y", vp), ("ld_py", i64), ("p_mean", vp), ("p_rstd", vp), ("p_coef", vp),
                ("p_sum_d", vp), ("p_sum_dx", vp), ("p_gamma", vp), ("p_dgamma", vp), ("p_dbeta", vp), ("p_eval_mode", i32)]


class TnRiders(C.Structure):
    _fields_ = [("S", i32), ("E", i32), ("L", i32), ("table_copies", i32),
                ("emb", vp), ("w_mu", vp), ("w_lv", vp), ("d_table", vp),
                ("d_emb", vp), ("d_w_mu", vp), ("d_b_mu", vp), ("d_w_lv", vp), ("d_b_lv", vp),
                ("sums", vp), ("beta", f32), ("gamma", f32), ("beta_gamma_dev", vp), ("out5", vp)]


HEAD_ZERO_MAX = 4       # MMVAE_HEAD_ZERO_MAX


class StepHeadArgs(C.Structure):
    _fields_ = [("S", i32), ("E", i32), ("L", i32), ("n_zero", i32),
                ("emb", vp), ("w_mu", vp), ("b_mu", vp), ("w_lv", vp), ("b_lv", vp), ("table", vp),
                ("zero_ptr", vp * HEAD_ZERO_MAX), ("zero_bytes", i64 * HEAD_ZERO_MAX),
                ("prep_items", vp), ("n_prep", i32),
                ("advance", i32),
                ("mask", vp), ("n_mask", i64), ("eps", vp), ("n_eps", i64),
                ("seed", C.c_uint64), ("offset", C.c_uint64), ("offset_dev", vp), ("keep_prob", f32), ("pad_", i32)]


class ScaleItem(C.Structure):
    _fields_ = [("x", vp), ("n", i64), ("dtype", i32), ("pad_", i32)]


class BnFinalizeArgs(C.Structure):
    _fields_ = [("M", i32), ("N", i32), ("sum", vp), ("sumsq", vp),
                ("gamma", vp), ("beta", vp), ("eps", f32), ("momentum", f32),
                ("running_mean", vp), ("running_var", vp), ("num_batches_tracked", vp),
                ("mean", vp), ("rstd", vp), ("scale", vp), ("shift", vp)]


class BnBwdFinalizeArgs(C.Structure):
    _fields_ = [("M", i32), ("N", i32), ("sum_d", vp), ("sum_dx", vp),
                ("gamma", vp), ("rstd", vp), ("dgamma", vp), ("dbeta", vp), ("coef", vp), ("eval_mode", i32)]


class FuseFwdArgs(C.Structure):
    _fields_ = [("B", i32), ("L", i32), ("n_mod", i32),
                ("heads_a", vp), ("heads_b", vp), ("ld_heads", i64),
                ("table", vp), ("site", vp), ("S", i32),
                ("eps", vp), ("mu", vp), ("logvar", vp),
                ("z", vp), ("z_dtype", i32), ("ldz", i64)]


class LatentEnc(C.Structure):
    _fields_ = [("y", vp), ("ldy", i64), ("K", i32), ("scale", vp), ("shift", vp),
                ("mask", vp), ("ld_mask", i64), ("inv_keep", f32), ("finalize", vp),
                ("w", vp), ("ldw", i64), ("bias", vp)]


class LatentFwdArgs(C.Structure):
    _fields_ = [("prec", i32), ("B", i32), ("L", i32), ("n_mod", i32),
                ("enc_a", LatentEnc), ("enc_b", LatentEnc),
                ("table", vp), ("site", vp), ("S", i32),
                ("eps", vp), ("mu", vp), ("logvar", vp),
                ("z", vp), ("ldz", i64),
                ("w_stem", vp), ("ldw_stem", i64), ("bias_stem", vp), ("N_stem", i32),
                ("h0", vp), ("ldh0", i64)]


class AELatentFwdArgs(C.Structure):
    _fields_ = [("prec", i32), ("B", i32), ("L", i32), ("n_mod", i32),
                ("enc", LatentEnc),
                ("table", vp), ("site", vp), ("S", i32),
                ("latent", vp),
                ("z", vp), ("ldz", i64),
                ("w_stem", vp), ("ldw_stem", i64), ("bias_stem", vp), ("N_stem", i32),
                ("h0", vp), ("ldh0", i64)]


class ClassTailArgs(C.Structure):
    _fields_ = [("prec", i32), ("B", i32), ("S", i32), ("L", i32), ("hidden", i32),
                ("h0", vp), ("ldh0", i64),
                ("w", vp), ("ldw", i64), ("wt", vp), ("ldwt", i64), ("bias", vp),
                ("site", vp), ("class_weights", vp),
                ("mu", vp), ("logvar", vp),
                ("beta", f32), ("gamma", f32), ("beta_gamma_dev", vp),
                ("sums", vp),
                ("g_c", vp), ("ld_gc", i64),
                ("d0", vp), ("ldd0", i64),
                ("g_mu", vp), ("g_lv", vp)]


class GroupMomentsArgs(C.Structure):
    _fields_ = [("prec", i32), ("B", i32), ("G", i32), ("N", i32), ("K", i32), ("act", i32),
                ("a", vp), ("lda", i64),
                ("w", vp), ("ldw", i64), ("bias", vp),
                ("mean", vp), ("ld_mean", i64),
                ("std", vp), ("ld_std", i64)]


class FuseBwdArgs(C.Structure):
    _fields_ = [("B", i32), ("L", i32), ("n_mod", i32),
                ("g_mu", vp), ("g_lv", vp), ("dz", vp), ("dz2", vp), ("dz3", vp), ("lddz", i64),
                ("eps", vp), ("logvar", vp),
                ("d_heads", vp), ("ld_heads", i64),
                ("d_table", vp), ("site", vp), ("S", i32), ("d_heads_lp", vp), ("ld_heads_lp", i64), ("table_copies", i32)]


class FuseMeanFwdArgs(C.Structure):
    _fields_ = [("B", i32), ("L", i32), ("n_mod", i32),
                ("head", vp), ("ld_head", i64),
                ("table", vp), ("site", vp), ("S", i32),
                ("latent", vp),
                ("z", vp), ("z_dtype", i32), ("ldz", i64)]


class FuseMeanBwdArgs(C.Structure):
    _fields_ = [("B", i32), ("L", i32), ("n_mod", i32),
                ("dz", vp), ("lddz", i64),
                ("g_latent", vp),
                ("d_head", vp), ("ld_head", i64),
                ("d_head_lp", vp), ("ld_head_lp", i64),
                ("d_table", vp), ("site", vp), ("S", i32), ("table_copies", i32)]


class LossArgs(C.Structure):
    _fields_ = [("B", i32), ("A", i32), ("D", i32), ("S", i32), ("L", i32),
                ("recon_a", vp), ("a", vp), ("ld_ra", i64), ("ld_a", i64),
                ("recon_b", vp), ("b", vp), ("ld_rb", i64), ("ld_b", i64),
                ("logits", vp), ("ld_logits", i64), ("site", vp), ("class_weights", vp),
                ("mu", vp), ("logvar", vp),
                ("beta", f32), ("gamma", f32),
                ("sums", vp),
                ("g_a", vp), ("g_a_dtype", i32), ("ld_ga", i64),
                ("g_b", vp), ("g_b_dtype", i32), ("ld_gb", i64), ("grad_b_wrt_logit", i32),
                ("g_c", vp), ("ld_gc", i64),
                ("g_mu", vp), ("g_lv", vp), ("beta_gamma_dev", vp), ("a_dtype", i32), ("b_dtype", i32)]


class MetricsArgs(C.Structure):
    _fields_ = [("M", i32), ("N", i32),
                ("pred", vp), ("pred_dtype", i32), ("ld_pred", i64),
                ("target", vp), ("target_dtype", i32), ("ld_target", i64),
                ("col_shift", vp), ("col_acc", vp), ("row_pearson", vp), ("row_cosine", vp)]


class KnnArgs(C.Structure):
    _fields_ = [("q", vp), ("t", vp), ("shift", vp), ("idx", vp), ("dist2", vp), ("work", vp),
                ("ld_q", i64), ("ld_t", i64), ("ld_idx", i64), ("ld_dist2", i64), ("work_bytes", i64),
                ("Mq", i32), ("Nt", i32), ("F", i32), ("k", i32), ("q_dtype", i32), ("t_dtype", i32)]


class KnnGroupArgs(C.Structure):
    _fields_ = [("base", KnnArgs), ("q_same", vp), ("t_same", vp), ("q_differ", vp), ("t_differ", vp), ("metric", i32)]


class SilhouetteArgs(C.Structure):
    _fields_ = [("x", vp), ("shift", vp), ("order", vp), ("class_start", vp), ("s", vp), ("intra", vp), ("inter", vp), ("work", vp),
                ("ld_x", i64), ("work_bytes", i64),
                ("N", i32), ("F", i32), ("C", i32), ("splits", i32), ("x_dtype", i32), ("pad_", i32)]


class PcaScatterArgs(C.Structure):
    _fields_ = [("x", vp), ("shift", vp), ("s", vp), ("work", vp),
                ("ld_x", i64), ("ld_s", i64), ("work_bytes", i64),
                ("N", i32), ("F", i32), ("splits", i32), ("x_dtype", i32)]


class PcaProjectArgs(C.Structure):
    _fields_ = [("x", vp), ("shift", vp), ("v", vp), ("y", vp),
                ("ld_x", i64), ("ld_v", i64), ("ld_y", i64),
                ("N", i32), ("F", i32), ("k", i32), ("x_dtype", i32)]


class StdPart(C.Structure):
    _fields_ = [("x", vp), ("ld", i64), ("cols", i32), ("dtype", i32), ("one_row", i32), ("pad_", i32)]


class StandardizeFitArgs(C.Structure):
    _fields_ = [("part", StdPart * STD_MAX_PARTS),
                ("mean", vp), ("var", vp), ("scale", vp), ("work", vp),
                ("work_bytes", i64),
                ("rows", i32), ("n_parts", i32), ("splits", i32), ("pad_", i32)]


class StandardizeApplyArgs(C.Structure):
    _fields_ = [("part", StdPart * STD_MAX_PARTS),
                ("mean", vp), ("scale", vp), ("z", vp),
                ("ldz", i64),
                ("rows", i32), ("n_parts", i32)]


class TsneAffinitiesArgs(C.Structure):
    _fields_ = [("dist2", vp), ("p", vp), ("beta", vp),
                ("ld_dist2", i64), ("ld_p", i64),
                ("N", i32), ("k", i32), ("perplexity", f32), ("pad_", i32)]


class TsneGradientArgs(C.Structure):
    _fields_ = [("y", vp), ("row_ptr", vp), ("col", vp), ("val", vp), ("grad", vp), ("z", vp), ("err", vp), ("z_row", vp), ("work", vp),
                ("nnz", i64), ("work_bytes", i64),
                ("N", i32), ("splits", i32), ("exaggeration", f32), ("pad_", i32)]


class TsneUpdateArgs(C.Structure):
    _fields_ = [("y", vp), ("update", vp), ("gains", vp), ("grad", vp), ("grad_norm", vp), ("work", vp),
                ("work_bytes", i64),
                ("N", i32), ("momentum", f32), ("learning_rate", f32), ("pad_", i32)]


class LnActFwdArgs(C.Structure):
    _fields_ = [("z", vp), ("gamma", vp), ("beta", vp), ("mask", vp), ("y", vp), ("mean", vp), ("rstd", vp),
                ("ldz", i64), ("ld_mask", i64), ("ldy", i64),
                ("M", i32), ("N", i32), ("layer_norm", i32), ("eps", f32), ("inv_keep", f32), ("pad_", i32)]


class LnActBwdArgs(C.Structure):
    _fields_ = [("dy", vp), ("z", vp), ("mean", vp), ("rstd", vp), ("gamma", vp), ("beta", vp), ("mask", vp),
                ("dz", vp), ("dgamma", vp), ("dbeta", vp), ("work", vp),
                ("lddy", i64), ("ldz", i64), ("ld_mask", i64), ("lddz", i64), ("work_bytes", i64),
                ("M", i32), ("N", i32), ("layer_norm", i32), ("inv_keep", f32)]


class WceArgs(C.Structure):
    _fields_ = [("logits", vp), ("labels", vp), ("class_weights", vp), ("sums", vp), ("g", vp), ("pred", vp), ("nll", vp), ("confusion", vp),
                ("ld", i64), ("ldg", i64),
                ("M", i32), ("C", i32)]


class GatherItem(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("src_row_stride", i64), ("dst_row_stride", i64), ("row_bytes", i32), ("pad_", i32)]


class AdamWItem(C.Structure):
    _fields_ = [("p", vp), ("g", vp), ("m", vp), ("v", vp), ("n", i64)]


# name -> (argtypes); every function returns int; those that launch take the stream last
_SIGNATURES = {
    "mmvae_set_tuning": [i32, i32],
    "mmvae_prep_weights": [vp, i32, vp],
    "mmvae_gemm_nt": [C.POINTER(GemmNtArgs), vp],
    "mmvae_gemm_tn": [C.POINTER(GemmTnArgs), vp],
    "mmvae_gemm_tn_group": [vp, i32, vp],
    "mmvae_gemm_tn_group_riders": [vp, i32, C.POINTER(TnRiders), vp],
    "mmvae_step_head": [C.POINTER(StepHeadArgs), vp],
    "mmvae_bn_finalize": [C.POINTER(BnFinalizeArgs), vp],
    "mmvae_bn_eval_coeffs": [i32, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp],
    "mmvae_bn_bwd_finalize": [C.POINTER(BnBwdFinalizeArgs), vp],
    "mmvae_bn_bwd_apply": [i32, i32, i32, vp, i64, vp, i64, vp, vp, vp, vp],
    "mmvae_bn_bwd_finalize_apply": [i32, i32, i32, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, vp],
    "mmvae_embed_table_fwd": [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp],
    "mmvae_embed_table_bwd": [i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp],
    "mmvae_fuse_reparam_fwd": [C.POINTER(FuseFwdArgs), vp],
    "mmvae_fuse_reparam_bwd": [C.POINTER(FuseBwdArgs), vp],
    "mmvae_embed_proj_fwd": [i32, i32, i32, vp, vp, vp, vp, vp],
    "mmvae_embed_proj_bwd": [i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp],
    "mmvae_fuse_mean_fwd": [C.POINTER(FuseMeanFwdArgs), vp],
    "mmvae_fuse_mean_bwd": [C.POINTER(FuseMeanBwdArgs), vp],
    "mmvae_latent_fwd": [C.POINTER(LatentFwdArgs), vp],
    "mmvae_ae_latent_fwd": [C.POINTER(AELatentFwdArgs), vp],
    "mmvae_class_tail": [C.POINTER(ClassTailArgs), vp],
    "mmvae_class_tail_fits": [i32, i32, i32, i32, i64, i64],
    "mmvae_gemm_nt_group_moments": [C.POINTER(GroupMomentsArgs), vp],
    "mmvae_gemm_nt_group_moments_fits": [i32, i32, i32, i32, i32, i32, i32, i64, i64],
    "mmvae_vae_loss": [C.POINTER(LossArgs), vp],
    "mmvae_loss_finalize": [vp, f32, f32, vp, vp, vp],
    "mmvae_recon_metrics": [C.POINTER(MetricsArgs), vp],
    "mmvae_knn_search": [C.POINTER(KnnArgs), vp],
    "mmvae_knn_work_bytes": [i32, i32, i32, C.POINTER(i64)],
    "mmvae_knn_splits": [i32, i32, C.POINTER(i32), C.POINTER(i32)],
    "mmvae_knn_mean_rows": [vp, i64, vp, i32, i64, vp, i64, i32, i32, i32, i32, vp],
    "mmvae_knn_search_l1": [C.POINTER(KnnArgs), vp],
    "mmvae_knn_l1_work_bytes": [i32, i32, i32, C.POINTER(i64)],
    "mmvae_knn_weighted_rows": [vp, i64, vp, i64, i32, vp, i32, i64, vp, i64, i32, i32, i32, i32, vp],
    "mmvae_knn_search_grouped": [C.POINTER(KnnGroupArgs), vp],
    "mmvae_knn_group_work_bytes": [i32, i32, i32, i32, C.POINTER(i64)],
    "mmvae_silhouette_samples": [C.POINTER(SilhouetteArgs), vp],
    "mmvae_silhouette_work_bytes": [i32, i32, i32, C.POINTER(i64)],
    "mmvae_silhouette_splits": [i32, i32, i32, C.POINTER(i32)],
    "mmvae_pca_scatter": [C.POINTER(PcaScatterArgs), vp],
    "mmvae_pca_scatter_splits": [i32, i32, i32, C.POINTER(i32)],
    "mmvae_pca_scatter_work_bytes": [i32, i32, i32, C.POINTER(i64)],
    "mmvae_pca_project": [C.POINTER(PcaProjectArgs), vp],
    "mmvae_standardize_fit": [C.POINTER(StandardizeFitArgs), vp],
    "mmvae_standardize_fit_splits": [i32, i64, i32, C.POINTER(i32)],
    "mmvae_standardize_fit_work_bytes": [i32, i64, i32, C.POINTER(i64)],
    "mmvae_standardize_apply": [C.POINTER(StandardizeApplyArgs), vp],
    "mmvae_tsne_affinities": [C.POINTER(TsneAffinitiesArgs), vp],
    "mmvae_tsne_gradient": [C.POINTER(TsneGradientArgs), vp],
    "mmvae_tsne_gradient_splits": [i32, i32, C.POINTER(i32)],
    "mmvae_tsne_gradient_work_bytes": [i32, i32, C.POINTER(i64)],
    "mmvae_tsne_update": [C.POINTER(TsneUpdateArgs), vp],
    "mmvae_tsne_update_work_bytes": [i32, C.POINTER(i64)],
    "mmvae_ln_act_fwd": [C.POINTER(LnActFwdArgs), vp],
    "mmvae_ln_act_bwd": [C.POINTER(LnActBwdArgs), vp],
    "mmvae_ln_act_bwd_work_bytes": [i32, i32, i32, C.POINTER(i64)],
    "mmvae_wce_mean": [C.POINTER(WceArgs), vp],
    "mmvae_gather_rows": [vp, i32, vp, i32, i64, vp],
    "mmvae_rows_to_bf16": [vp, i32, i64, vp, i64, i32, i32, vp],
    "mmvae_sigmoid_bwd": [i32, i32, vp, i64, vp, i64, vp, i32, i64, vp],
    "mmvae_scale_if_needed": [vp, i32, i64, vp, vp],
    "mmvae_scale_many": [C.POINTER(ScaleItem), i32, vp, vp],
    "mmvae_noise": [vp, i64, f32, vp, i64, C.c_uint64, C.c_uint64, vp, i32, vp],
    "mmvae_counter_add": [vp, C.c_uint64, vp],
    "mmvae_adamw_step": [vp, i32, f32, f32, f32, f32, f32, f32, f32, i32, vp, i32, vp, vp],
    "mmvae_adam_step": [vp, i32, f32, f32, f32, f32, f32, f32, f32, i32, vp, i32, vp, vp],
}
EXPORTED = ["mmvae_abi_version"] + sorted(_SIGNATURES)

_lib = None


class MMVAELibraryError(RuntimeError):
    pass


class MMVAEArgError(RuntimeError):
    """The library refused the arguments (MMVAE_ERR_ARG / MMVAE_ERR_DTYPE) and enqueued nothing (mmvae_hip.h)."""


def load():
    """Load libmmvae_hip.so once; raise loudly if it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MMVAELibraryError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU / eager fallback). "
            "Build it with `python __graft_entry__.py` or `make -C vae-los-angeles_amd/csrc`.")
    lib = C.CDLL(LIB_PATH)
    lib.mmvae_abi_version.restype = C.c_int
    v = lib.mmvae_abi_version()
    if v != ABI_VERSION:
        raise MMVAELibraryError(f"libmmvae_hip.so ABI {v} != binding ABI {ABI_VERSION}; rebuild")
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(status, what):
    if status in (-1, -2):
        kind = "invalid argument" if status == -1 else "dtype not supported for this precision"
        raise MMVAEArgError(f"{what} failed: {kind}")
    if status != 0:
        raise RuntimeError(f"{what} failed: hipError {status}")
