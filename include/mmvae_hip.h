/* mmvae_hip.h -- C ABI of libmmvae_hip.so: the MI355X (gfx950) kernels behind the
 * MultiModalVAE training hot path of marcin119a/vae-los-angeles.
 *
 * The reference has no FFI of its own: its "operator interface" for this path is the set of
 * stock PyTorch ops its modules call.  Each entry point below names the reference call sites
 * (file:line, relative to the reference repo) whose device work it replaces.  The host side
 * (the mmvae Python package under vae-los-angeles_amd/) binds these with ctypes and keeps the reference's
 * src.models / src.utils.losses class surface on top.
 *
 * Conventions
 *   - plain pointers to DEVICE memory and sizes; no framework types.  The library never
 *     allocates or frees device memory and keeps no state between calls.
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); nothing
 *     synchronises, so calls are graph-capturable.
 *   - return value: 0 = ok; <0 = argument check failed (MMVAE_ERR_*); >0 = hipError_t of the launch.
 *     A call that returns MMVAE_ERR_ARG or MMVAE_ERR_DTYPE has enqueued NOTHING: the caller may issue another form of the same work
 *     (a separate finalisation launch, a call without pro_out) and nothing is counted twice.
 *   - the library reads no environment variables: one build is one configuration (mmvae_set_tuning only serves tests).
 *   - matrices are row-major with an explicit leading dimension in ELEMENTS.
 *   - "activation type" = float in MMVAE_PREC_F32 mode, bfloat16 in MMVAE_PREC_BF16 mode.
 */
#ifndef MMVAE_HIP_H
#define MMVAE_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMVAE_OK 0
#define MMVAE_ERR_ARG (-1)
#define MMVAE_ERR_DTYPE (-2)

enum { MMVAE_F32 = 0, MMVAE_BF16 = 1 };                 /* storage dtype of a buffer   */
enum { MMVAE_PREC_F32 = 0, MMVAE_PREC_BF16 = 1 };       /* MFMA operand precision      */
enum { MMVAE_PRO_NONE = 0, MMVAE_PRO_BN_RELU_DROP = 1, MMVAE_PRO_BN_BWD_APPLY = 2 };
enum { MMVAE_EPI_STORE = 0, MMVAE_EPI_RELU_MASK = 1, MMVAE_EPI_BN_BWD = 2, MMVAE_EPI_LOSS_MSE = 3, MMVAE_EPI_LOSS_BCE_LOGIT = 4 };
enum { MMVAE_ACT_NONE = 0, MMVAE_ACT_RELU = 1, MMVAE_ACT_SIGMOID = 2 };

#define MMVAE_TILE 128          /* GEMM output tile edge */

int mmvae_abi_version(void);    /* bumped on any struct change; the ctypes binding checks it */
/* Tuning knobs (tests compare kernel forms inside one process): key 0 = minimum M for the 128x256-tile NT kernels (default 32768); key 2 = LDS-DMA generation of the
 * NT kernel (gemm_nt2.h) on/off; key 3 = log2 of the operand size in bytes from which row blocks are used (17..32; 0 = default 32):
 * mmvae_gemm_nt / mmvae_gemm_tn address their row operands with 32-bit offsets, so an operand of 4 GiB or more (65 536 x 27 000 fp32
 * at the scaled omics widths) is processed in row blocks of at most half that threshold inside the entry point, and key 3 lowers it so
 * that tests reach that path at moderate sizes; key 4 = wide-tile kernel for the large weight gradients (gemm_tn_wide.hip) on/off;
 * key 6 / key 7 = row-coalesced LDS form of the BatchNorm-backward / ReLU-mask dX epilogue on/off; key 8 = wave-specialised NT kernel
 * (gemm_ntp.h: producer / consumer waves) on/off, key 9 = its minimum M (default 16384); key 10 = the fused latent launch
 * (mmvae_latent_fwd) on/off: off, it returns MMVAE_ERR_ARG and the caller issues the launches it replaces; key 12 = the fused class-head
 * launch (mmvae_class_tail) on/off, in the same way; key 13 = the merged head-of-step launch (mmvae_step_head) on/off and key 14 = the
 * riders of the grouped dW launch (mmvae_gemm_tn_group_riders) on/off, in the same way; key 15 = the autoencoders' fused latent launch
 * (mmvae_ae_latent_fwd) on/off, in the same way.  Other keys: MMVAE_ERR_ARG. */
int mmvae_set_tuning(int32_t key, int32_t value);

/* ---------------------------------------------------------------------------------------------
 * Weight preparation: fp32 master weights -> zero-padded MFMA operand copies (compute type),
 * plain and transposed, plus concatenations (fc_mu|fc_logvar heads).  One launch for a whole
 * table of items held in device memory.
 *   dst[r][c] (r < dst_rows, c < dst_cols, leading dim dst_ld) =
 *       transpose ? src[c][r] : src[r][c]   if inside src's logical [src_rows][src_cols], else 0
 * Replaces: the implicit weight reads of every aten::addmm / mm on the path.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const float* src; void* dst;
    int32_t src_rows, src_cols; int64_t src_ld;
    int32_t dst_rows, dst_cols; int64_t dst_ld;
    int32_t transpose; int32_t dst_dtype;
} mmvae_prep_item;
int mmvae_prep_weights(const mmvae_prep_item* items_dev, int32_t n_items, void* stream);

/* ---------------------------------------------------------------------------------------------
 * C[M,N] = epilogue( prologue(A)[M,K] x W[N,K]^T )          (gemm_nt.hip)
 *   W        prepared operand [ceil128(N)][ceil64(K)] in compute type, ldw % 64 == 0
 *   A (bf16) rows are padded to a multiple of 8 elements and the pad columns must hold ZEROS (every producer in this library writes
 *            them): the LDS-DMA kernels move whole 16-byte chunks and multiply the pads with the zero padding of W -- 0 x NaN bits is NaN
 *   h, masks are [M][ld] matrices whose rows hold N elements rounded up to the padding of the activation buffers (8 elements; masks:
 *            4 bytes): a kernel reads nothing beyond that from a row's first element, so h may be a column slice of a wider buffer
 *            (the merged first layers of the decoders) without any tail padding
 *   prologue MMVAE_PRO_BN_RELU_DROP: A is the previous layer's PRE-BatchNorm output (activation
 *            type); the kernel applies relu(A*pro_scale[k]+pro_shift[k]) * keep/(1-p) on the fly
 *            (encoders.py:14-16,32-34,36-38).  pro_mask: uint8 keep mask [M][ld_pro_mask], bytes 0 or 1 (mmvae_noise), or NULL.
 *   epilogue MMVAE_EPI_STORE    : C = act(acc + bias) (+ C if accumulate); optional per-column
 *                                 (sum, sum of squares) of the stored values, accumulated into
 *                                 stat1/stat2 (BatchNorm batch statistics)
 *            MMVAE_EPI_RELU_MASK: C = acc * (h > 0)                (ReLU backward, decoders)
 *            MMVAE_EPI_BN_BWD   : d = acc * keep/(1-p) * (h*bn_scale+bn_shift > 0), h = pre-BN output
 *                                 (Dropout+ReLU backward), then BatchNorm backward in two launches:
 *                                 bn_phase 0: nothing stored, stat1/stat2 += (sum d, sum d*xhat);
 *                                 bn_phase 1: C = coef0*(d - coef1 - xhat*coef2), coef from
 *                                 mmvae_bn_bwd_finalize.  d is recomputed from the f32 accumulators, so
 *                                 the subtraction happens before the one rounding to the activation type.
 *            MMVAE_EPI_LOSS_MSE / MMVAE_EPI_LOSS_BCE_LOGIT: the reconstruction loss of a decoder's last layer inside its GEMM
 *                                 (bf16 mode, bf16 A, K > 64): x = acc + bias is not stored; *stat1 (ONE f64) += sum (x - h)^2, or
 *                                 += sum BCE(sigmoid(x), h) with the log clamp at -100 (losses.py:31,34); C (bf16, ldc % 8 == 0,
 *                                 pad columns zeroed) = 2 (x - h), or sigmoid(x) - h = the gradient w.r.t. the logit; h = fp32 target
 *                                 [M][ldh] of h_dtype.  Same arithmetic as mmvae_vae_loss on the stored output; saves writing and re-reading it.
 *                                 h_dtype MMVAE_BF16: the target is read as bf16 (rows aligned to 2 bytes; padded bf16 rows, see
 *                                 mmvae_rows_to_bf16, give the widest loads) and widened to fp32 on load: on equal values the gradient
 *                                 elements are bit-identical to the fp32-target form and the loss sum differs only by the f64 atomics' order.
 * Replaces: nn.Linear forward = aten::addmm (encoders.py:13,18-19,31,35,40-41,54-55;
 *   decoders.py:13,15,27,29,31,44,46), relu/sigmoid (decoders.py:14,28,30,32), batch-norm
 *   statistics, and the dX mm of each Linear backward (optimize_hyperparameters.py:112).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t prec, M, N, K;
    const void* a; int32_t a_dtype; int64_t lda;
    int32_t prologue;
    const float* pro_scale; const float* pro_shift; const uint8_t* pro_mask; int64_t ld_pro_mask; float pro_inv_keep;
    const void* w; int64_t ldw;
    int32_t epilogue;
    void* c; int32_t c_dtype; int64_t ldc;
    const float* bias; int32_t act; int32_t accumulate;
    const void* h; int64_t ldh;
    const float* bn_scale; const float* bn_shift; const float* bn_mean; const float* bn_rstd;
    const uint8_t* epi_mask; int64_t ld_epi_mask; float epi_inv_keep;
    const float* bn_coef; int32_t bn_phase;       /* MMVAE_EPI_BN_BWD: 0 = statistics, 1 = apply (recompute), 2 = statistics + store d */
    double* stat1; double* stat2;                 /* optional [N] f64 accumulators (atomic adds; zero them first) */
    /* optional, MMVAE_PRO_BN_RELU_DROP with a bf16 A only: the operand AFTER the prologue -- relu(a * scale + shift) * keep / (1 - p),
       i.e. the previous layer's post-activation (encoders.py:33-34,37-38) -- is also written here ([M][ld_pro_out] bf16, K columns) so
       that the layer's dW GEMM can read it as a plain operand.  Only the wave-specialised kernel writes it (its producer waves hold the
       values anyway): MMVAE_ERR_ARG when the problem is not one of its (M >= 16384, M % 128 == 0, N % 128 == 0, N <= 256, K % 64 == 0,
       K <= 512, bf16 C with whole 128-byte rows, operands below 4 GiB: the row-block path refuses pro_out before its first block). */
    void* pro_out; int64_t ld_pro_out;
    /* optional, MMVAE_PRO_BN_RELU_DROP: `const mmvae_bn_finalize_args*` (host memory, read during the call).  mmvae_bn_finalize of the
       layer that produced A is folded into this launch: every workgroup forms scale / shift of A's columns from the f64 column sums
       (pro_scale / pro_shift are then ignored), and ONE workgroup writes what mmvae_bn_finalize writes -- mean, rstd, scale, shift, the
       running statistics and num_batches_tracked -- for the backward pass.  fin->N must equal K.  Not for operands of 4 GiB or more
       (MMVAE_ERR_ARG: the row blocks would each update the running statistics). */
    const void* pro_finalize;
    /* element type of h for MMVAE_EPI_LOSS_MSE / MMVAE_EPI_LOSS_BCE_LOGIT: MMVAE_F32 (0, the zero-initialised default) or MMVAE_BF16.
       Ignored by the other epilogues (their h is activation-typed). */
    int32_t h_dtype;
} mmvae_gemm_nt_args;
int mmvae_gemm_nt(const mmvae_gemm_nt_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * dW[N,K] += P[M,N]^T x Q[M,K] ;  db[N] += column sums of P      (gemm_tn.hip)
 *   P = gradient w.r.t. the layer output, Q = the layer input (optionally through the same
 *   BN+ReLU+Dropout prologue as above).  dW/db are fp32 and ACCUMULATED (dW through the slab workspace or f32
 *   atomics, db with atomics): zero them first.  nsplit <= 0 lets the library choose the batch split (<= 64).
 * Replaces: the dW mm and db sum of each Linear backward (optimize_hyperparameters.py:112).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t prec, M, N, K;
    const void* p; int32_t p_dtype; int64_t ldp;
    const void* q; int32_t q_dtype; int64_t ldq;
    int32_t q_prologue;
    const float* pro_scale; const float* pro_shift; const uint8_t* pro_mask; int64_t ld_pro_mask; float pro_inv_keep;
    float* dw; int64_t lddw; float* db;
    int32_t nsplit;
    float* slab; int64_t slab_elems;   /* optional workspace: when it holds nsplit*N*K floats the splits store partial tiles there
                                          and a second launch sums them in fixed order (deterministic dW, no atomics); else atomics */
    /* optional prologue on P (MMVAE_PRO_BN_BWD_APPLY): P = coef0 * (p - coef1 - xhat * coef2), xhat = (p_y - mean) * rstd, i.e.
       mmvae_bn_bwd_apply folded into the operand load (first layers: nothing else consumes dL/dy).  p_y has p's dtype;
       p_coef is [3][N] as written by mmvae_bn_bwd_finalize. */
    int32_t p_prologue;
    const void* p_y; int64_t ld_py; const float* p_mean; const float* p_rstd; const float* p_coef;
    /* p_coef == NULL with MMVAE_PRO_BN_BWD_APPLY: mmvae_bn_bwd_finalize folded into this launch.  The kernel forms the three
       constants per column from the f64 sums of MMVAE_EPI_BN_BWD (coef = {gamma * rstd, sum_d / M, sum_dx / M}; p_eval_mode != 0:
       {gamma * rstd, 0, 0}) and ONE workgroup per column tile adds dgamma += sum_dx, dbeta += sum_d.  Only the wide-tile kernels do
       this (M >= 8192, N >= 128, K >= 256, bf16, slab given): MMVAE_ERR_ARG otherwise -- call mmvae_bn_bwd_finalize and pass p_coef. */
    const double* p_sum_d; const double* p_sum_dx; const float* p_gamma; float* p_dgamma; float* p_dbeta; int32_t p_eval_mode;
} mmvae_gemm_tn_args;
int mmvae_gemm_tn(const mmvae_gemm_tn_args* args, void* stream);
/* Up to MMVAE_TN_GROUP_MAX small-output problems (same prec; the latent / class-width layers: encoder heads, decoder first
 * layers, DecoderC) in ONE GEMM launch + ONE reduce launch: alone each is a latency chain of ~25 us for a few MB.  Every
 * problem needs a slab workspace of its own (MMVAE_TN_GROUP_SPLITS * N * K floats covers any split), lddw == K and no P prologue; operand
 * combinations: P f32 with Q through the BN+ReLU+Dropout prologue, P and Q activation-typed, P f32 with Q activation-typed.
 * Returns MMVAE_ERR_ARG when a problem does not fit: launch that one with mmvae_gemm_tn. */
#define MMVAE_TN_GROUP_MAX 8
#define MMVAE_TN_GROUP_SPLITS 256
int mmvae_gemm_tn_group(const mmvae_gemm_tn_args* args, int32_t n, void* stream);
/* The same grouped launch with RIDERS: small launches of the end of the backward that neither feed nor read the group run as extra
 * workgroups appended to its grid instead of as latency chains of their own (10 + 5 us per step beside a 52 us launch).
 *   EncoderC backward (S > 0): mmvae_embed_table_bwd's arguments, workgroups and LDS image; results bit-identical to that call.
 *     It writes EncoderC's five gradient tensors, which no problem of the group may alias.
 *   Loss finalisation (sums != NULL): mmvae_loss_finalize's arguments, one thread.
 * Returns MMVAE_ERR_ARG, with nothing enqueued, when riders is NULL or names no rider, a rider's arguments are incomplete, the
 * EncoderC rider's LDS need (S*2L + S*E + 2L*E floats) exceeds the dynamic LDS the group kernel is launched with (72 KiB) or
 * 64 KiB (24 sites x latent 128 x embed 32 ride, 59 KiB; mmvae_embed_table_bwd alone takes up to 160 KiB), tuning key 14 is off, or
 * mmvae_gemm_tn_group would refuse the problems: the caller then issues the launches this one replaces. */
typedef struct {
    int32_t S, E, L, table_copies;
    const float* emb; const float* w_mu; const float* w_lv; const float* d_table;
    float* d_emb; float* d_w_mu; float* d_b_mu; float* d_w_lv; float* d_b_lv;
    const double* sums; float beta, gamma; const float* beta_gamma_dev; float* out5;
} mmvae_tn_riders;
int mmvae_gemm_tn_group_riders(const mmvae_gemm_tn_args* args, int32_t n, const mmvae_tn_riders* riders, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm1d, training mode (encoders.py:14,32,36): from the column sums compute
 * mean / biased var, emit scale = gamma*rstd and shift = beta - mean*scale for the consumer's
 * prologue, save mean/rstd for backward, update running stats (momentum, UNBIASED variance)
 * and num_batches_tracked.  Eval mode: coefficients from the running stats.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t M, N; const double* sum; const double* sumsq;        /* [N] each, from MMVAE_EPI_STORE stat1/stat2 */
    const float* gamma; const float* beta; float eps; float momentum;
    float* running_mean; float* running_var; int64_t* num_batches_tracked;   /* may be NULL */
    float* mean; float* rstd; float* scale; float* shift;
} mmvae_bn_finalize_args;
int mmvae_bn_finalize(const mmvae_bn_finalize_args* args, void* stream);
/* eval mode: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale; optionally (non-NULL) also
 * mean = running_mean and rstd = 1 / sqrt(running_var + eps), which a backward pass through an eval-mode forward needs. */
int mmvae_bn_eval_coeffs(int32_t N, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, float* scale, float* shift, float* mean, float* rstd, void* stream);

/* BatchNorm backward reductions: from the sums (sum d, sum d*xhat) of MMVAE_EPI_BN_BWD phase 0:
 *   dgamma += sum d*xhat ; dbeta += sum d ; coef[3][N] = {gamma*rstd, dbeta/M, dgamma/M}
 * eval_mode != 0 (the forward ran on the running statistics, torch's batch_norm(training=False) backward): the
 * normalisation does not depend on the batch, coef = {gamma*rstd, 0, 0}; dgamma / dbeta as above. */
typedef struct {
    int32_t M, N; const double* sum_d; const double* sum_dx;      /* [N] each, from MMVAE_EPI_BN_BWD phase 0 */
    const float* gamma; const float* rstd;
    float* dgamma; float* dbeta; float* coef;           /* coef: [3][N] */
    int32_t eval_mode;
} mmvae_bn_bwd_finalize_args;
int mmvae_bn_bwd_finalize(const mmvae_bn_bwd_finalize_args* args, void* stream);
/* d <- coef0 * (d - coef1 - xhat*coef2), xhat = (y-mean)*rstd, in place on the activation-typed buffer d written by
 * MMVAE_EPI_BN_BWD bn_phase 2 (the one-contraction form of BatchNorm backward). */
int mmvae_bn_bwd_apply(int32_t dtype, int32_t M, int32_t N, void* d, int64_t ldd, const void* y, int64_t ldy,
                       const float* mean, const float* rstd, const float* coef, void* stream);
/* mmvae_bn_bwd_finalize + mmvae_bn_bwd_apply in ONE launch: the constants are formed from the f64 sums by every thread for its own
 * columns, the threads of the first rows add dgamma += sum_dx, dbeta += sum_d.  Same argument limits as mmvae_bn_bwd_apply, and the
 * column-resident form only (256 % (N / 8) == 0 for bf16, 256 % (N / 4) == 0 for f32: every hidden width of the model); else ERR_ARG. */
int mmvae_bn_bwd_finalize_apply(int32_t dtype, int32_t M, int32_t N, void* d, int64_t ldd, const void* y, int64_t ldy,
                                const float* mean, const float* rstd, const double* sum_d, const double* sum_dx, const float* gamma,
                                float* dgamma, float* dbeta, int32_t eval_mode, void* stream);

/* ---------------------------------------------------------------------------------------------
 * EncoderC (encoders.py:57-61): Embedding + two heads == a per-class table
 *   T[S][2L] = emb[S][E] x [Wmu;Wlv]^T + [bmu;blv]      (fp32), gathered per sample later.
 * Backward: from dT[S][2L]: dEmb, dWmu, dWlv, dbmu, dblv (all accumulated).
 *   Capacity: every workgroup of mmvae_embed_table_bwd keeps its three operands in LDS, so the call returns MMVAE_ERR_ARG (nothing
 *   enqueued) when (S*2L + S*E + 2L*E) * 4 bytes exceed 160 KiB, the CU's LDS: every (latent <= 100, embed <= 64) of the reference's
 *   hyperparameter search fits up to 106 sites.  Up to 64 KiB the launch is the one it always was; beyond, the same kernel runs with
 *   the dynamic-LDS attribute raised (same per-thread arithmetic and accumulation order).  The attribute is set once per process,
 *   on the device that is current at the first call past 64 KiB, and the flag is not guarded against concurrent first calls: one
 *   device per process and one calling thread, as for the other launches here that take more than 64 KiB (ranks are processes).
 * ------------------------------------------------------------------------------------------- */
int mmvae_embed_table_fwd(int32_t S, int32_t E, int32_t L, const float* emb, const float* w_mu, const float* b_mu,
                          const float* w_lv, const float* b_lv, float* table, void* stream);
int mmvae_embed_table_bwd(int32_t S, int32_t E, int32_t L, const float* emb, const float* w_mu, const float* w_lv,
                          const float* d_table, int32_t table_copies, float* d_emb, float* d_w_mu, float* d_b_mu, float* d_w_lv,
                          float* d_b_lv, void* stream);      /* d_table: [table_copies][S][2L] (see mmvae_fuse_bwd_args), summed here */

/* ---------------------------------------------------------------------------------------------
 * Mean-fusion over the modalities present + reparameterisation (vae.py:65-73, 11-15):
 *   mu = mean_m mu_m ; logvar = mean_m logvar_m ; z = mu + eps * exp(0.5*logvar)
 *   heads_x: [B][2L] fp32 (mu | logvar) or NULL; table/site: EncoderC table + int64 labels or NULL.
 *   z is written in activation type with leading dim ldz (pad columns are zeroed).
 * Backward: d_heads[B][2L] = [ (g_mu + dz)/n | (g_lv + dz*eps*std/2)/n ], and the same rows
 *   scatter-added into d_table[site] when the site modality is present.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t B, L, n_mod;
    const float* heads_a; const float* heads_b; int64_t ld_heads;
    const float* table; const int64_t* site; int32_t S;
    const float* eps;
    float* mu; float* logvar;
    void* z; int32_t z_dtype; int64_t ldz;
} mmvae_fuse_fwd_args;
int mmvae_fuse_reparam_fwd(const mmvae_fuse_fwd_args* args, void* stream);

typedef struct {
    int32_t B, L, n_mod;
    const float* g_mu; const float* g_lv;           /* may be NULL (treated as 0) */
    const float* dz; const float* dz2; const float* dz3; int64_t lddz;   /* dL/dz per decoder (dz2, dz3 may be NULL); summed */
    const float* eps; const float* logvar;
    float* d_heads; int64_t ld_heads;
    float* d_table; const int64_t* site; int32_t S;  /* may be NULL */
    void* d_heads_lp; int64_t ld_heads_lp;   /* optional bf16 copy of d_heads ([B][>= 2L], pad columns zeroed): the A operand of the heads' dX
                                              * GEMMs in bf16 mode (they round d_heads to bf16 on load anyway), which lets them run the
                                              * LDS-DMA kernel with the row-coalesced BatchNorm-backward epilogue */
    int32_t table_copies;   /* d_table is [table_copies][S][2L], zeroed; workgroup w adds into copy w % table_copies (0 = 1).  Every
                             * workgroup ends with S x 2L atomic adds onto the same addresses: 512 workgroups on ONE copy spent 19 of
                             * the kernel's 32 us there.  mmvae_embed_table_bwd sums the copies. */
} mmvae_fuse_bwd_args;
#define MMVAE_TABLE_COPIES 8
int mmvae_fuse_reparam_bwd(const mmvae_fuse_bwd_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The latent path of the non-variational baselines RNA2DNAAE / DNA2RNAAE (directional_ae.py:46-64): the encoder ends in ONE
 * Linear(hidden, latent), the site enters through Embedding -> Linear(embed, latent), the fusion is the plain mean.
 *
 * mmvae_embed_proj_fwd / _bwd: the one-head case of mmvae_embed_table_fwd / _bwd (the same kernels' bodies with one head):
 *   table[S][L] = emb[S][E] x w[L][E]^T + b   (fp32; every element accumulates from the bias over e ascending)
 *   backward, from d_table[table_copies][S][L] (the copies are summed in fixed order): d_emb, d_w, d_b are accumulated into.
 *   Capacity as mmvae_embed_table_bwd, for one head: MMVAE_ERR_ARG (nothing enqueued) when (S*L + S*E + L*E) * 4 bytes exceed 160 KiB.
 *
 * mmvae_fuse_mean_fwd:  latent = (head + table[site]) * (1 / n_mod), the sum formed in the order head, table row, multiplied only
 *   when n_mod > 1 (one or two terms: exact after the one addition).  head: fp32 [B][ld_head] or NULL; table / site / S: the
 *   projected table [S][L] fp32 + int64 labels, or NULL; n_mod must equal the number of modalities present (>= 1), else
 *   MMVAE_ERR_ARG.  latent: CONTIGUOUS fp32 [B][L]; z: the same values in z_dtype (MMVAE_F32 / MMVAE_BF16) with leading dimension
 *   ldz >= L, pad columns zeroed.  A label outside [0, S) poisons its own row with NaN and reads nothing outside the table.
 * mmvae_fuse_mean_bwd:  d_head[B][ld_head] = (dz + g_latent) * (1 / n_mod) (g_latent: the gradient that arrived at the returned
 *   latent, contiguous [B][L] or NULL), an optional bf16 copy d_head_lp (pad columns zeroed), and -- d_table given -- the same rows
 *   scatter-added into d_table[w % table_copies][site[b]] by workgroup w (0 copies = 1), through LDS when S*L*4 <= 48 KiB, with
 *   global atomics otherwise; rows with a label outside [0, S) are not scattered.
 * ------------------------------------------------------------------------------------------- */
int mmvae_embed_proj_fwd(int32_t S, int32_t E, int32_t L, const float* emb, const float* w, const float* b, float* table, void* stream);
int mmvae_embed_proj_bwd(int32_t S, int32_t E, int32_t L, const float* emb, const float* w, const float* d_table, int32_t table_copies,
                         float* d_emb, float* d_w, float* d_b, void* stream);
typedef struct {
    int32_t B, L, n_mod;
    const float* head; int64_t ld_head;
    const float* table; const int64_t* site; int32_t S;
    float* latent;
    void* z; int32_t z_dtype; int64_t ldz;
} mmvae_fuse_mean_fwd_args;
int mmvae_fuse_mean_fwd(const mmvae_fuse_mean_fwd_args* args, void* stream);
typedef struct {
    int32_t B, L, n_mod;
    const float* dz; int64_t lddz;
    const float* g_latent;
    float* d_head; int64_t ld_head;
    void* d_head_lp; int64_t ld_head_lp;
    float* d_table; const int64_t* site; int32_t S; int32_t table_copies;
} mmvae_fuse_mean_bwd_args;
int mmvae_fuse_mean_bwd(const mmvae_fuse_mean_bwd_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The latent path of the forward in ONE launch (latent.hip): from the encoders' last PRE-BatchNorm outputs to the decoders' first
 * hidden activation, per 16-row slab without leaving the CU --
 *   per encoder present:  heads = bf16(relu(y * scale + shift) * keep * inv_keep) x Wheads^T + bias   (the arithmetic of
 *                         mmvae_gemm_nt with MMVAE_PRO_BN_RELU_DROP, K ascending; fp32, NOT stored)
 *   mean fusion + reparameterisation exactly as mmvae_fuse_reparam_fwd (sum in the order a, b, table row of site[b]; a label outside
 *                         [0, S) poisons its own row with NaN and touches nothing outside the table): mu, logvar (fp32) and z (bf16,
 *                         pad columns zeroed) are written
 *   stems:                h0 = bf16(relu(z x Wstem^T + bias_stem))   (mmvae_gemm_nt with MMVAE_ACT_RELU on the merged first layers)
 * i.e. what vae.py:65-73 and the first Linear + ReLU of every decoder (decoders.py:13-14,27-28,44-45) compute, bit for bit what the
 * four launches it replaces (two heads GEMMs, mmvae_fuse_reparam_fwd, the stem GEMM) write.
 *   enc_x.y == NULL: that encoder is absent.  enc_x.finalize: `const mmvae_bn_finalize_args*` (host memory, read during the call) as
 *   mmvae_gemm_nt's pro_finalize: every workgroup forms scale / shift from the f64 column sums, workgroup 0 writes mean / rstd /
 *   scale / shift, the running statistics and num_batches_tracked; NULL: scale / shift are read (eval mode, or finalised before).
 *   mask: uint8 keep mask [B][ld_mask] or NULL.  w: prepared heads weight ([>= 48][ldw] bf16, rows >= 2L zero), bias fp32 [2L].
 *   n_mod must equal the number of modalities present (>= 1), as mmvae_fuse_reparam_fwd checks.
 * Limits (anything else: MMVAE_ERR_ARG / MMVAE_ERR_DTYPE before anything is enqueued; the caller then issues the four launches):
 *   prec == MMVAE_PREC_BF16 (MMVAE_ERR_DTYPE otherwise); B >= 1, 1 <= L <= 24 (2L <= 48 head columns: three MFMA tiles; the scaled
 *   config's latent 128 does not fit) and B * L < 2^31; eps, mu, logvar, z, w_stem and h0 given;
 *   per encoder: K % 32 == 0 and 32 <= K <= 256; ldy % 8 == 0, ldy >= K and y 16-byte aligned; ld_mask % 8 == 0, ld_mask >= K and
 *   mask 8-byte aligned; w given, 16-byte aligned, ldw % 64 == 0 and ldw >= K; scale and shift given unless finalize is; finalize->N
 *   == K, finalize->M == B >= 2 and its sums, gamma, beta, mean, rstd, scale, shift given;
 *   ldz % 8 == 0, L <= ldz <= 32, z 16-byte aligned; N_stem % 64 == 0 and 64 <= N_stem <= 448; w_stem 16-byte aligned,
 *   ldw_stem % 64 == 0 and ldw_stem >= 32; h0 rows are whole 128-byte lines (ldh0 % 64 == 0, ldh0 >= N_stem, 128-byte aligned base);
 *   site given and 1 <= S, S * 2L <= 1024 when the table is; every row operand (y, mask, h0) below 4 GiB; tuning key 10 on
 *   (mmvae_set_tuning).
 * Not checked, the caller's contract: eps, mu and logvar are CONTIGUOUS [B][L] fp32; the head weights have at least 48 readable rows
 *   (rows 2L..47 zero) and the stem weights 32 readable columns (columns L..31 zero) -- what mmvae_prep_weights writes into a
 *   [ceil128(N)][ceil64(K)] operand; the table is [S][2L] fp32, site int64 [B].
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const void* y; int64_t ldy; int32_t K;          /* last hidden layer's pre-BatchNorm output, bf16 [B][ldy] */
    const float* scale; const float* shift;         /* [K]; ignored when finalize is given */
    const uint8_t* mask; int64_t ld_mask; float inv_keep;
    const void* finalize;
    const void* w; int64_t ldw; const float* bias;
} mmvae_latent_enc;
typedef struct {
    int32_t prec, B, L, n_mod;
    mmvae_latent_enc enc_a, enc_b;
    const float* table; const int64_t* site; int32_t S;
    const float* eps;
    float* mu; float* logvar;
    void* z; int64_t ldz;
    const void* w_stem; int64_t ldw_stem; const float* bias_stem; int32_t N_stem;
    void* h0; int64_t ldh0;
} mmvae_latent_fwd_args;
int mmvae_latent_fwd(const mmvae_latent_fwd_args* args, void* stream);

/* The autoencoders' latent path of the forward in ONE launch: the deterministic instantiation of mmvae_latent_fwd's kernel
 * (latent.hip), per 16-row slab without leaving the CU --
 *   head   = bf16(relu(y * scale + shift) * keep * inv_keep) x Wproj^T + bias   (mmvae_gemm_nt with MMVAE_PRO_BN_RELU_DROP, K ascending,
 *            with the folded BatchNorm finalisation through enc.finalize; fp32, NOT stored)
 *   latent = (head + table[site]) * (1 / n_mod) as mmvae_fuse_mean_fwd forms it, written as contiguous fp32 [B][L]; z: bf16, pads zeroed
 *   h0     = bf16(relu(z x W0^T + b0))   (mmvae_gemm_nt with MMVAE_ACT_RELU on the ONE decoder's first layer)
 * bit for bit what the three launches it replaces write.  No eps is read, no logvar written.  enc.y == NULL: the encoder is absent
 * (site only); table == NULL: no site.  n_mod must equal the number of modalities present (>= 1).
 * Limits, those of mmvae_latent_fwd restated for one head (anything else: MMVAE_ERR_ARG, fp32: MMVAE_ERR_DTYPE, before anything is
 * enqueued; the caller then issues the three launches): 1 <= L <= 24, B * L < 2^31; enc: K % 32 == 0, 32 <= K <= 256 and the operand
 * alignments of mmvae_latent_enc; the prepared head weight has at least 48 readable rows, rows >= L zero; ldz % 8 == 0, L <= ldz <= 32,
 * z 16-byte aligned; N_stem % 64 == 0, 64 <= N_stem <= 448 (DecoderA's 128 and DecoderB's 256 fit), ldw_stem % 64 == 0, >= 32; h0 rows
 * whole 128-byte lines (ldh0 % 64 == 0, >= N_stem, base 128-byte aligned); S * L <= 1024 with site given; row operands below 4 GiB;
 * tuning key 15 on. */
typedef struct {
    int32_t prec, B, L, n_mod;
    mmvae_latent_enc enc;
    const float* table; const int64_t* site; int32_t S;
    float* latent;
    void* z; int64_t ldz;
    const void* w_stem; int64_t ldw_stem; const float* bias_stem; int32_t N_stem;
    void* h0; int64_t ldh0;
} mmvae_ae_latent_fwd_args;
int mmvae_ae_latent_fwd(const mmvae_ae_latent_fwd_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The class head of the training step in ONE launch (class_tail.hip): the class decoder's last Linear, the weighted cross-entropy
 * and KL terms of vae_loss with their gradients, and the back-propagation through that Linear and the ReLU in front of it, per
 * 16-row slab without leaving the CU --
 *   logits = h0 x W^T + bias                    (mmvae_gemm_nt on the bf16 hidden activation, K ascending; fp32, NOT stored)
 *   sums[2] += sum_i w[site_i] * nll_i, sums[4] += labels outside [0, S), g_c = gamma * w[y] * (softmax - onehot)   (fp32, stored)
 *   d0 = (h0 > 0) ? bf16(g_c) x W : 0           (mmvae_gemm_nt with MMVAE_EPI_RELU_MASK on the fp32 g_c; bf16, whole rows of d0)
 *   sums[3] += KL, g_mu = beta * mu, g_lv = -0.5 * beta * (1 - exp(logvar))
 * i.e. what mmvae_gemm_nt (the Linear), mmvae_vae_loss with only logits / mu / logvar given and mmvae_gemm_nt (its dX) compute:
 * g_c, d0, g_mu, g_lv and the count in sums[4] bit for bit, sums[2] and sums[3] up to the order of their f64 additions.
 *   h0 / d0: the class decoder's 64 columns of the merged hidden activation and of its gradient (column slices: ldh0 / ldd0 are the
 *   leading dimensions of the whole buffers).  w: prepared weight ([>= 32][ldw] bf16, rows >= S zero); wt: its prepared transpose
 *   ([>= 64][ldwt] bf16, columns >= S zero) -- what mmvae_prep_weights writes.  class_weights: fp32 [S] or NULL.  mu / logvar /
 *   g_mu / g_lv: CONTIGUOUS [B][L] fp32.  beta_gamma_dev as in mmvae_loss_args.  sums: double[5] as mmvae_vae_loss.
 * Limits (anything else: MMVAE_ERR_ARG before anything is enqueued; the caller then issues the three launches):
 *   prec == MMVAE_PREC_BF16; hidden == 64; 4 <= S <= 32 and S % 4 == 0 (the row-per-thread class path
 *   of mmvae_vae_loss, whose arithmetic this is); 1 <= L <= 24; B >= 1 and B * max(L, S) < 2^31; every pointer but class_weights and
 *   beta_gamma_dev given; h0 16-byte aligned, ldh0 % 8 == 0, ldh0 >= 64; d0 rows are whole 128-byte lines (128-byte aligned,
 *   ldd0 % 64 == 0); w and wt 16-byte aligned, ldw % 8 == 0, ldw >= 64, ldwt % 8 == 0, ldwt >= 32; g_c 16-byte aligned,
 *   ld_gc % 4 == 0, ld_gc >= S; tuning key 12 on (mmvae_set_tuning).
 * mmvae_class_tail_fits answers the shape part of these limits (and the tuning key) without operands: 0, or the error
 * mmvae_class_tail would return.  A forward that wants to leave the Linear to this launch asks it first.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t prec, B, S, L, hidden;
    const void* h0; int64_t ldh0;
    const void* w; int64_t ldw; const void* wt; int64_t ldwt; const float* bias;
    const int64_t* site; const float* class_weights;
    const float* mu; const float* logvar;
    float beta, gamma; const float* beta_gamma_dev;
    double* sums;
    float* g_c; int64_t ld_gc;
    void* d0; int64_t ldd0;
    float* g_mu; float* g_lv;
} mmvae_class_tail_args;
int mmvae_class_tail(const mmvae_class_tail_args* args, void* stream);
int mmvae_class_tail_fits(int32_t prec, int32_t S, int32_t hidden, int32_t L, int64_t ldh0, int64_t ldd0);

/* ---------------------------------------------------------------------------------------------
 * A Linear whose output rows are reduced in groups ON CHIP (group_moments.hip): the decoder's last layer of a multiple-draw /
 * all-site reconstruction, where each of B samples owns G consecutive rows of the operand (one per draw and site) and only the
 * mean and the spread across them are wanted --
 *   x[b*G + g][j] = act( sum_k a[b*G + g][k] * w[j][k] + bias[j] )     g < G; act = MMVAE_ACT_NONE | MMVAE_ACT_SIGMOID
 *   mean[b][j]    = (1/G) sum_g x[b*G + g][j]                           (g ascending, one division)
 *   std[b][j]     = sqrt( sum_g (x[b*G + g][j] - mean[b][j])^2 / (G - 1) )    (optional; a second pass over the stored tile)
 * i.e. what mmvae_gemm_nt with an fp32 C of B*G rows and a mean / unbiased std over its view [B][G][N] compute, without that C.
 * x is formed from the fp32 accumulators as mmvae_gemm_nt's store epilogue forms it (bias added in fp32, sigmoid = rcp(1 + exp(-v)))
 * and is NOT rounded to a storage type.
 *   a: bf16 [B*G][lda], rows padded to 8 elements with zeroed pad columns, as mmvae_gemm_nt takes its bf16 A.  w / bias: the
 *   prepared operand ([ceil128(N)][ceil64(K)] bf16, what mmvae_prep_weights writes) and the fp32 bias (or NULL) of the Linear.
 *   mean / std: fp32 [B][ld_mean] / [B][ld_std]; columns >= N are not touched.  std == NULL: no standard deviation.
 * Limits (anything else: MMVAE_ERR_ARG / MMVAE_ERR_DTYPE before anything is enqueued; the caller then issues mmvae_gemm_nt and
 * the reduction this launch replaces):
 *   prec == MMVAE_PREC_BF16 (MMVAE_PREC_F32: MMVAE_ERR_DTYPE); B >= 1; 1 <= G <= 128 (a 128-row tile holds floor(128 / G) whole
 *   groups); std only with G >= 2; K % 64 == 0 and 64 <= K <= 512; N >= 1; act one of the two above; a and w 16-byte aligned,
 *   lda % 8 == 0, lda >= K, ldw % 64 == 0, ldw >= K; mean and std 4-byte aligned, ld_mean >= N, ld_std >= N; B*G*lda*2 and
 *   (N + 256)*ldw*4 below 2^32 (the 32-bit offsets of the NT kernels; there are no row blocks here).
 * mmvae_gemm_nt_group_moments_fits answers everything but the pointers and the output strides without operands: 0, or the
 * error mmvae_gemm_nt_group_moments would return (with_std: std != NULL).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t prec, B, G, N, K, act;
    const void* a; int64_t lda;
    const void* w; int64_t ldw; const float* bias;
    float* mean; int64_t ld_mean;
    float* std; int64_t ld_std;
} mmvae_group_moments_args;
int mmvae_gemm_nt_group_moments(const mmvae_group_moments_args* args, void* stream);
int mmvae_gemm_nt_group_moments_fits(int32_t prec, int32_t B, int32_t G, int32_t N, int32_t K, int32_t act, int32_t with_std,
                                     int64_t lda, int64_t ldw);

/* ---------------------------------------------------------------------------------------------
 * vae_loss (src/utils/losses.py:8-46) and the directional losses
 * (src/utils/directional_losses.py:8-55), one pass, optional terms (NULL pointers skip a term):
 *   sums[0] += sum (recon_a-a)^2                               (losses.py:31)
 *   sums[1] += sum -[b*max(log p,-100) + (1-b)*max(log(1-p),-100)]   (losses.py:34)
 *   sums[2] += sum_i w[site_i] * nll_i                          (losses.py:39)
 *   sums[3] += -0.5 * sum(1 + lv - mu^2 - exp(lv))              (losses.py:42)
 *   sums[4] += number of labels outside [0, S)  (torch's cross_entropy device-asserts on them; here such a row is
 *              computed as class 0 and COUNTED: the host wrapper raises when the count it reads back is not 0).  A label of -100
 *              is F.cross_entropy's default ignore_index: that row adds no loss and gets a zero gradient, and is not counted
 * `sums` is double[5], zeroed by the caller; mmvae_loss_finalize turns it into the tuple of losses.py:44,46 (a last-block
 * finalisation inside the kernel was measured: ~1000 tickets on one address + the fences cost 50 us against a 5 us launch).
 * Gradients of total = s0+s1+gamma*s2+beta*s3:
 *   g_a = 2(recon_a-a) ; g_b = (p-b)/max(p(1-p),1e-12)  [grad_b_wrt_logit: times p(1-p)] ;
 *   g_c = gamma*w[y]*(softmax - onehot) ; g_mu = beta*mu ; g_lv = -0.5*beta*(1-exp(lv)).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t B, A, D, S, L;
    const float* recon_a; const void* a; int64_t ld_ra, ld_a;          /* a: element type a_dtype (below) */
    const float* recon_b; const void* b; int64_t ld_rb, ld_b;          /* b: element type b_dtype (below) */
    const float* logits; int64_t ld_logits; const int64_t* site; const float* class_weights;
    const float* mu; const float* logvar;
    float beta, gamma;
    double* sums;
    void* g_a; int32_t g_a_dtype; int64_t ld_ga;
    void* g_b; int32_t g_b_dtype; int64_t ld_gb; int32_t grad_b_wrt_logit;
    float* g_c; int64_t ld_gc;
    float* g_mu; float* g_lv;
    const float* beta_gamma_dev;      /* optional {beta, gamma} in device memory: overrides the by-value fields, so a captured hipGraph
                                         follows the beta warm-up (optimize_hyperparameters.py:103) without re-capture */
    /* element types of the MSE / BCE targets a and b: MMVAE_F32 (0, the zero-initialised default) or MMVAE_BF16 (a dataset kept in
       bf16 storage; any row stride, rows 2-byte aligned).  bf16 targets are widened on load: on equal values the gradients are
       bit-identical to the fp32-target call and the sums differ only by the order of the f64 atomics. */
    int32_t a_dtype, b_dtype;
} mmvae_loss_args;
int mmvae_vae_loss(const mmvae_loss_args* args, void* stream);
/* out5 = {recon + gamma*class + beta*kld, recon, class, kld, labels out of range} (float) from sums[5]. */
int mmvae_loss_finalize(const double* sums, float beta, float gamma, const float* beta_gamma_dev, float* out5, void* stream);

/* out = g * p * (1-p): Sigmoid backward for gradients that arrive w.r.t. recon_b (decoders.py:32). */
int mmvae_sigmoid_bwd(int32_t M, int32_t N, const float* g, int64_t ldg, const float* p, int64_t ldpp,
                      void* out, int32_t out_dtype, int64_t ldo, void* stream);

/* x *= *scale unless *scale == 1 (loss.backward(gradient=...) support); n elements of dtype. */
int mmvae_scale_if_needed(void* x, int32_t dtype, int64_t n, const float* scale_dev, void* stream);
/* the same for up to MMVAE_SCALE_MAX tensors in ONE launch (the records travel in the kernel arguments) */
#define MMVAE_SCALE_MAX 8
typedef struct { void* x; int64_t n; int32_t dtype; int32_t pad_; } mmvae_scale_item;
int mmvae_scale_many(const mmvae_scale_item* items_host, int32_t n_items, const float* scale_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Noise: Philox4x32-10 streams keyed by (seed, offset).  Dropout keep mask (nn.Dropout(0.1),
 * encoders.py:16,34,38; replaces aten::bernoulli_) and standard normal eps
 * (torch.randn_like, vae.py:14).
 * ------------------------------------------------------------------------------------------- */
/* One launch: n_mask keep-mask bytes (P(1) = keep_prob) and n_eps standard normals.  The Philox counter starts at
 * offset + *offset_dev (offset_dev may be NULL); a device-resident offset lets a captured hipGraph draw fresh noise on
 * every replay.  The call consumes ceil(n_mask/16)*4 + ceil(n_eps/4) counter values.  advance != 0: offset_dev is an array of
 * MMVAE_CTR_COPIES identical copies of the counter (block L reads copy L; no block reads a word another one writes) and the
 * launch itself moves every copy past what it consumed -- no separate counter launch. */
#define MMVAE_CTR_COPIES 16384
int mmvae_noise(uint8_t* mask, int64_t n_mask, float keep_prob, float* eps, int64_t n_eps, uint64_t seed, uint64_t offset,
                uint64_t* offset_dev, int32_t advance, void* stream);
int mmvae_counter_add(uint64_t* counter_dev, uint64_t inc, void* stream);      /* *counter_dev += inc */

/* ---------------------------------------------------------------------------------------------
 * Head of a training step: the four mutually independent launches a forward begins with, as ONE launch whose workgroups take
 * roles by block range.  Three of them are latency chains (9 + 5 + 5 us) that fit under the one with real work, the Philox
 * arithmetic of the noise (25 us): they get the lowest block indices, in the order below, and the noise blocks follow.
 *   table : mmvae_embed_table_fwd's arguments (S > 0)
 *   zero  : up to MMVAE_HEAD_ZERO_MAX ranges (16-byte aligned, a whole multiple of 16 bytes each) filled with zeros --
 *           the step's one memset
 *   prep  : mmvae_prep_weights' arguments (n_prep > 0)
 *   noise : mmvae_noise's arguments (n_mask + n_eps > 0), the same counter values consumed and the same advance
 * Every role runs the device code of the stand-alone entry point named with it: results are bit-identical to those calls.
 * A role whose count is 0 is empty.  Returns MMVAE_ERR_ARG, with nothing enqueued, when every role is empty, a role's arguments
 * would be refused by its own entry point, a zero range is misaligned, or tuning key 13 is off.
 * ------------------------------------------------------------------------------------------- */
#define MMVAE_HEAD_ZERO_MAX 4
typedef struct {
    int32_t S, E, L, n_zero;
    const float* emb; const float* w_mu; const float* b_mu; const float* w_lv; const float* b_lv; float* table;
    void* zero_ptr[MMVAE_HEAD_ZERO_MAX]; int64_t zero_bytes[MMVAE_HEAD_ZERO_MAX];
    const mmvae_prep_item* prep_items; int32_t n_prep;
    int32_t advance;
    uint8_t* mask; int64_t n_mask; float* eps; int64_t n_eps;
    uint64_t seed, offset; uint64_t* offset_dev; float keep_prob; int32_t pad_;
} mmvae_step_head_args;
int mmvae_step_head(const mmvae_step_head_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Minibatch assembly from a device-resident dataset: dst_t[i][:] = src_t[idx[i]][:], i < rows, for up to MMVAE_GATHER_MAX
 * row-major tensors sharing one int64 index vector (rows / strides in BYTES, multiples of 4; 8-byte words are moved when everything
 * is a multiple of 8).  Indices outside
 * [0, src_rows) are clamped.  Replaces: MultiModalDataset.__getitem__ + the DataLoader's default collate
 * (src/data/dataset.py:28-39, optimize_hyperparameters.py:55-65) -- one Python call and one torch.tensor() per SAMPLE.
 * ------------------------------------------------------------------------------------------- */
#define MMVAE_GATHER_MAX 4
typedef struct { const void* src; void* dst; int64_t src_row_stride; int64_t dst_row_stride; int32_t row_bytes; int32_t pad_; } mmvae_gather_item;
int mmvae_gather_rows(const mmvae_gather_item* items_host, int32_t n_items, const int64_t* idx_dev, int32_t rows,
                      int64_t src_rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Inputs in bf16 storage ("padded bf16 rows"): a bf16 matrix [rows][ld_dst] with ld_dst % 8 == 0, a 16-byte aligned base and ZEROS in
 * the pad columns cols .. ld_dst-1 -- the layout of every bf16 A operand above, so the first-layer GEMMs, their dW GEMMs (Q) and the
 * loss epilogues read such a dataset directly.  One launch (graph-capturable):
 *   dst[r][c] = bf16(src[r][c]) for c < cols, 0 for cols <= c < ld_dst;  src: fp32 or bf16 (src_dtype), any row stride ld_src, rows
 *   aligned to the element size.  dst holds rows * ld_dst elements.  fp32 values are rounded to nearest even exactly as
 *   torch.Tensor.to(torch.bfloat16) does (every NaN -> 0x7FC0, +-Inf kept, denormals rounded, not flushed); bf16 is copied bit for bit.
 * Replaces: the per-step fp32 -> bf16 conversion the GEMM producers do on fp32 inputs (a dataset is converted once per run).
 * ------------------------------------------------------------------------------------------- */
int mmvae_rows_to_bf16(const void* src, int32_t src_dtype, int64_t ld_src, void* dst, int64_t ld_dst, int32_t rows, int32_t cols,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Imputation metrics of a reconstruction against its target in ONE streaming pass (metrics.hip): what compute_metrics
 * (compare_directional_imputation.py:167-210) and calculate_metrics (vae_cross_modality_cv.py:71-108) take from an N x N
 * cosine_similarity matrix and a Python loop of scipy.stats.pearsonr over host copies.  y = target, p = prediction, [M][N]:
 *   row_pearson[i] = Pearson r of (y_i, p_i), clamped to [-1, 1]; NaN when every element of y_i, or every element of p_i, compares
 *                    equal to that row's first element (scipy's constant-input rule, decided on the values)
 *   row_cosine[i]  = sum y p / (|y_i| |p_i|), a zero norm replaced by 1 (sklearn's normalize: a zero row gives 0)
 *   col_acc[0][j] += sum_i (y_ij - c_j)      col_acc[1][j] += sum_i (y_ij - c_j)^2      c = col_shift, NULL = 0
 *   col_acc[2][j] += sum_i (p_ij - y_ij)^2   col_acc[3][j] += sum_i |p_ij - y_ij|
 * col_acc is double[4][N] and ACCUMULATED (f64 atomics; zero it once per evaluation, as `sums` of mmvae_vae_loss): MAE / MSE / RMSE
 * and the flat and per-feature R^2 follow from it on the host, additive over batches; col_shift (one fixed vector per evaluation,
 * e.g. the first target row) keeps the column moments well conditioned and is undone there.  row_* are fp32 [M], written.
 * Values are widened to f64 on load and every sum is f64; Pearson uses the moments of the row shifted by its own first element.
 * Non-finite inputs give non-finite outputs.  Results are not bit-reproducible between runs (order of the atomics).
 *   pred / target: MMVAE_F32 or MMVAE_BF16, row-major, leading dimension in elements, any row stride >= N (padded bf16 rows, see
 *   mmvae_rows_to_bf16, included; loads are as wide as base and stride allow; pad columns are never read).  ld_pred == 0: ONE prediction row for every sample (the
 *   mean-imputation baseline, compare_directional_imputation.py:213-232, without its np.tile).  1 <= M, N < 2^31; row offsets are
 *   64-bit, there is no operand size limit.
 * MMVAE_ERR_ARG (nothing enqueued): a null struct or null pred / target / col_acc / row_pearson / row_cosine, M < 1, N < 1, a leading
 *   dimension below N (other than ld_pred == 0), a dtype that is neither, a pointer not aligned to its element size.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t M, N;
    const void* pred; int32_t pred_dtype; int64_t ld_pred;
    const void* target; int32_t target_dtype; int64_t ld_target;
    const float* col_shift;
    double* col_acc;
    float* row_pearson; float* row_cosine;
} mmvae_metrics_args;
int mmvae_recon_metrics(const mmvae_metrics_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Brute-force k nearest neighbours (euclidean) of every query row among the training rows, as a GEMM whose epilogue is a running
 * top-k (knn.hip): the Mq x Nt scores never reach memory, only k indices (and distances) per query do.  Replaces the neighbour
 * search of sklearn's KNeighborsRegressor(n_neighbors=5) / ConditionedKNeighborsRegressor (compare_directional_imputation.py:235-254,
 * vae_cross_modality_cv.py:320, src/clustering_evaluation/cluster_imputation_methods.py:297-403, src/models/conditioned_knn.py:18-93)
 * and of calculate_neighborhood_hit (src/clustering_evaluation/metrics_utils.py:19-38), which run on host copies.
 *   q [Mq][F], t [Nt][F]: MMVAE_F32 or MMVAE_BF16 each, row-major, leading dimension in elements >= F (padded bf16 rows, see
 *   mmvae_rows_to_bf16, included; loads are as wide as base and stride allow; pad columns and rows outside the matrices are never
 *   read).  shift [F] (fp32, NULL = 0) is subtracted from both operands in fp32 on load: distances do not change, the conditioning
 *   of the GEMM form does (pass the training column means).
 * Ranking key of candidate j for query i:  key = |t_j - c|^2 - 2 (q_i - c).(t_j - c),  products and sums in fp32 on the exact-f32
 * MFMA path; bf16 storage is widened, never multiplied as bf16.  The key of a (query row, training row) pair depends only on the
 * values of the two rows and of shift -- not on where the rows sit, on Mq, Nt, k or on how the work was split: duplicate training
 * rows tie bit for bit.
 *   idx [Mq][k] (int32, leading dimension ld_idx >= k): the k candidates with the smallest keys, ascending by (key, j): among
 *   equal keys the smaller training index first.  A NaN key orders after every other key (+inf included); -0 and +0 are one key.
 *   dist2 [Mq][k] (fp32, optional, ld_dist2 >= k): key + |q_i - c|^2, negative values replaced by 0.
 * Results are bit-reproducible from run to run (no float atomics; partial lists are merged in a fixed order).
 * A workgroup owns 128 query rows and walks the training rows in tiles of 128, the rows' current k-best lists live in LDS.  When Mq
 * alone gives too few workgroups, the training rows are split across workgroups (mmvae_knn_splits says how), the partial lists go to
 * `work` and a second small launch merges them.  work: caller-owned, 8-byte aligned, at least mmvae_knn_work_bytes(Mq, Nt, k) bytes
 * = 4 (Mq + Nt) for the rows' squared norms (one more streaming launch) + 8 Mq k splits when split; the library allocates nothing.
 * Limits: Mq, Nt, F >= 1 (any F); 1 <= k <= min(Nt, MMVAE_KNN_MAXK); row offsets are 64-bit.  MMVAE_KNN_MAXK = 96 covers the 92 of t-SNE at
 *   perplexity 30 (91 neighbours and the row itself); a row's list takes k rounded up to 16 entries of LDS, so k <= 64 runs as it did at 64.
 * MMVAE_ERR_ARG (nothing enqueued): a null struct, null q / t / idx / work, a size < 1, k out of range, a leading dimension below its
 *   width, a pointer not aligned to its element (work: 8 bytes), work_bytes below mmvae_knn_work_bytes.  MMVAE_ERR_DTYPE: a dtype
 *   that is neither MMVAE_F32 nor MMVAE_BF16.
 * ------------------------------------------------------------------------------------------- */
#define MMVAE_KNN_MAXK 96
typedef struct {
    const void* q; const void* t; const float* shift;
    int32_t* idx; float* dist2; void* work;
    int64_t ld_q, ld_t, ld_idx, ld_dist2, work_bytes;
    int32_t Mq, Nt, F, k, q_dtype, t_dtype;
} mmvae_knn_args;
int mmvae_knn_search(const mmvae_knn_args* args, void* stream);
/* needs no device; MMVAE_ERR_ARG for sizes < 1, k out of range or a null result pointer */
int mmvae_knn_work_bytes(int32_t Mq, int32_t Nt, int32_t k, int64_t* bytes);
/* the decomposition mmvae_knn_search uses for these sizes: *splits workgroups per query block, each over *rows_per_split consecutive
 * training rows (a multiple of 128, capped at 2^31 - 128; the last split takes the rest).  *splits == 1: no workspace lists, no merge
 * launch. */
int mmvae_knn_splits(int32_t Mq, int32_t Nt, int32_t* splits, int32_t* rows_per_split);

/* The manhattan (L1) search: the k nearest training rows of every query row under sum_c |q_ic - t_jc|, for the tuned k-NN baseline of
 * the reference (src/knn_comparison/run_comparison.py:56-94, metric='manhattan').  Takes mmvae_knn_args unchanged; q, t, idx, the
 * order (key, j) ascending with the smaller training index first among equal keys, NaN after +inf, the limits, the decomposition
 * (mmvae_knn_splits), the merge and the refusals are those of mmvae_knn_search.  What differs:
 *   shift must be NULL (MMVAE_ERR_ARG otherwise): differences are formed directly, there is nothing to condition.
 *   key = sum_{c = 0 .. F-1} |fl(q_ic - t_jc)| in fp32, bf16 widened exactly: ONE chain of plain adds in ascending column order,
 *   starting from +0 -- ((|d_0| + |d_1|) + |d_2|) + ..., never reassociated.  The key of a pair depends only on the two rows' values
 *   and F (not on position, Mq, Nt, k or the split), duplicate training rows tie bit for bit, and a sequential float32 loop on the
 *   host gives the same bits.  Columns beyond F that a chunk pads with zeros add +0.
 *   dist2 (optional) receives the L1 distance ITSELF, which is the key: it is NOT squared in this entry.
 *   work holds only the split lists: mmvae_knn_l1_work_bytes = 8 Mq k splits bytes when split, else 0; work may then be NULL.  There
 *   is no norms launch.
 * The distances are VALU work (a subtract and an add with |.| per pair and column), not a GEMM. */
int mmvae_knn_search_l1(const mmvae_knn_args* args, void* stream);
int mmvae_knn_l1_work_bytes(int32_t Mq, int32_t Nt, int32_t k, int64_t* bytes);

/* The grouped search: either search above with a say in which candidates a query may see, for k-fold cross-validation on ONE search
 * over the whole matrix (every row searches the rows outside its own fold; vae_cross_modality_cv.py:300-340 fits per fold and k) and
 * for the site-conditioned baseline in one launch (src/models/conditioned_knn.py:18-93 fits per site).
 *   base: operands, outputs and work exactly as mmvae_knn_search (metric 0, euclidean) / mmvae_knn_search_l1 (metric 1, manhattan).
 *   q_same [Mq], t_same [Nt] and q_differ [Mq], t_differ [Nt]: int32 codes (any value, negative included); a pair is given or NULL.
 * Candidate j is admitted for query i iff (the same pair is NULL or t_same[j] == q_same[i]) and (the differ pair is NULL or
 * t_differ[j] != q_differ[i]).  Among the admitted candidates everything is what the ungrouped entry of that metric specifies: the key
 * arithmetic, the order (key, j) ascending with the smaller index first among equal keys, NaN after +inf, dist2 (euclidean: squared;
 * manhattan: the distance itself), shift (NULL for manhattan), dtypes, limits (1 <= k <= min(Nt, MMVAE_KNN_MAXK)), the decomposition
 * of mmvae_knn_splits and bit-reproducibility.  Since a pair's key depends only on the two rows' values and the shift, the result
 * equals, bit for bit, the ungrouped search over the admitted subset with the indices mapped back.
 * Short lists: a query with c < k admitted candidates (c = 0 included) gets c ordered entries; positions c .. k-1 hold idx -1 and
 * distance +inf.  Nothing outside idx [Mq][k] / dist2 [Mq][k] is written.
 * Tile skip: one small launch first writes the min and max of t_same and of t_differ per tile of 128 candidate rows into work; a
 * workgroup reduces the same over its 128 query rows and walks only tiles that can hold an admitted pair: a tile is skipped iff
 * (same given and the two code ranges do not meet) or (differ given and tile and block each carry one code, the same one).  The
 * per-pair predicate holds in every tile that is walked, so results never depend on the skip; with rows sorted by group a same-group
 * search does sum n_g^2 work instead of N^2.
 * work: always needed, 8-byte aligned, at least mmvae_knn_group_work_bytes(Mq, Nt, k, metric) = the ungrouped size of that metric +
 * 16 ceil(Nt / 128) bytes; the tile codes lie behind the ungrouped layout.
 * MMVAE_ERR_ARG (nothing enqueued): everything the ungrouped entry refuses, a null struct, both pairs NULL (use the plain entry), half
 * a pair, a code pointer not 4-byte aligned, metric outside {0, 1}, work_bytes below mmvae_knn_group_work_bytes. */
typedef struct {
    mmvae_knn_args base;
    const int32_t* q_same;   const int32_t* t_same;
    const int32_t* q_differ; const int32_t* t_differ;
    int32_t metric;
} mmvae_knn_group_args;
int mmvae_knn_search_grouped(const mmvae_knn_group_args* args, void* stream);
int mmvae_knn_group_work_bytes(int32_t Mq, int32_t Nt, int32_t k, int32_t metric, int64_t* bytes);

/* Uniform k-NN regression from the indices of mmvae_knn_search:  out[i][:] = (sum_{n<k} y[idx[i][n]][:]) / k, in fp32, summed in
 * ascending n (deterministic; what KNeighborsRegressor.predict with uniform weights computes, conditioned_knn.py:84-91).
 * y [Ny][Fy]: MMVAE_F32 or MMVAE_BF16 rows (ld_y >= Fy), out [Mq][Fy] fp32 (ld_out >= Fy), idx [Mq][k] int32 (ld_idx >= k); indices
 * outside [0, Ny) are clamped, as mmvae_gather_rows does.  A streaming gather: y[idx].mean(1) in torch materialises Mq k Fy values.
 * MMVAE_ERR_ARG: null / misaligned pointers, sizes < 1, k > MMVAE_KNN_MAXK, a leading dimension below its width, Fy > 65535 * 256;
 * MMVAE_ERR_DTYPE: another y_dtype. */
int mmvae_knn_mean_rows(const int32_t* idx, int64_t ld_idx, const void* y, int32_t y_dtype, int64_t ld_y, float* out, int64_t ld_out,
                        int32_t Mq, int32_t k, int32_t Ny, int32_t Fy, void* stream);

/* Inverse-distance k-NN regression (sklearn's weights='distance', sklearn.neighbors._base._get_weights) from the indices and distances
 * of a search:  d_n = dist[i][n], or with dist_is_squared = 1 (the euclidean dist2) its correctly rounded square root.  If any d_n == 0
 * in the row, w_n = 1 where d_n == 0 and 0 elsewhere; otherwise w_n = 1 / d_n (correctly rounded).  Then
 *   out[i][:] = (sum_n w_n y[idx[i][n]][:]) / (sum_n w_n)   in fp32, both sums in ascending n (each product rounded, then added), one
 * correctly rounded division.  A NaN or negative distance in a row gives a NaN row, no fault.
 * idx [Mq][k] int32 and dist [Mq][k] fp32 with ld_idx, ld_dist >= k: the first k columns of a wider search can be passed in place.
 * y, out, the index clamp, the limits and the refusals are those of mmvae_knn_mean_rows; also MMVAE_ERR_ARG: a null or misaligned
 * dist, ld_dist < k, dist_is_squared outside {0, 1}.  A streaming gather: a row's k weights are computed once per workgroup. */
int mmvae_knn_weighted_rows(const int32_t* idx, int64_t ld_idx, const float* dist, int64_t ld_dist, int32_t dist_is_squared,
                            const void* y, int32_t y_dtype, int64_t ld_y, float* out, int64_t ld_out,
                            int32_t Mq, int32_t k, int32_t Ny, int32_t Fy, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Silhouette coefficient of every row (sklearn.metrics.silhouette_samples, euclidean) as a distance GEMM whose epilogue is a square
 * root and a per-class row sum (silhouette.hip): the N x N distances never reach memory.  Replaces silhouette_score over host copies
 * (src/clustering_evaluation/cluster_imputation_methods.py:478-504, cluster_reconstructed.py:299-317).
 * For rows x_i with class l_i in [0, C) and class sizes n_c:
 *   S_ic = sum_{j : l_j = c} |x_i - x_j|  (the pair j = i contributes exactly 0)
 *   a_i = S_{i,l_i} / (n_{l_i} - 1)       b_i = min over c != l_i with n_c > 0 of S_ic / n_c       s_i = (b_i - a_i) / max(a_i, b_i)
 *   s_i = 0 and a_i = 0 when n_{l_i} = 1; s_i = 0 when max(a_i, b_i) = 0 (sklearn's nan_to_num).  A row without any other non-empty
 *   class (sklearn raises) gets b_i = +inf and s_i = 0.
 *   x [N][F]: MMVAE_F32 or MMVAE_BF16, row-major, ld_x >= F in elements (padded bf16 rows, see mmvae_rows_to_bf16, included; loads are
 *   as wide as base and stride allow; pad columns and rows outside the matrix are never read).  shift [F] (fp32, NULL = 0) is subtracted
 *   from every element in fp32 on load, as in mmvae_knn_search: pass the column means.
 *   order [N] (int32, NULL = the rows are already grouped): the row indices grouped by class, class 0 first; the kernels read row
 *   order[p] for position p, values outside [0, N) are clamped as in mmvae_gather_rows.  No gathered copy of x is needed.
 *   class_start [C + 1] (int32, device): class c owns the positions class_start[c] .. class_start[c + 1] - 1; class_start[0] = 0,
 *   non-decreasing, class_start[C] = N; empty classes are allowed and skipped in b.  It cannot be validated at the call: in the
 *   kernels the values are clamped to [0, N], made non-decreasing and the two ends forced to 0 and N, so a bad vector gives wrong
 *   numbers but no access out of range.
 *   s (required), intra (= a, optional), inter (= b, optional): fp32 [N] in the caller's ROW order (written at index order[p]).
 * d_ij = sqrt(max(|x_i - c|^2 + |x_j - c|^2 - 2 (x_i - c).(x_j - c), 0)), products and sums in fp32 on the exact-f32 MFMA path, bf16
 * storage widened; correctly rounded square root and divisions.  Every sum has one fixed order (a lane's four columns, a butterfly
 * over the 16 lanes of a row, the two column waves, the tiles of a class, the splits in ascending order): no float atomics, results
 * are bit-identical from run to run for the same arguments and split count.
 * A workgroup owns 128 positions as query rows and walks the columns class by class in tiles of 128 that never cross a class
 * boundary.  splits: 0 = the library chooses (as mmvae_knn_search does: below 4 x 256 row blocks the column tiles are split),
 * 1 .. 64 forces that many; either is clamped to an upper bound of the number of column tiles that needs no device,
 * min(N, (N + 127 C) / 128), and mmvae_silhouette_splits returns the count used.  With more than one split every split writes [C]
 * partial sums per row to `work` and a second small launch adds them in ascending split order.
 * work: caller-owned, 8-byte aligned, at least mmvae_silhouette_work_bytes(N, C, splits) bytes = 4 N (rounded up to 8) for the rows'
 * squared norms (one more streaming launch) + 4 N C splits_used when split; the library allocates nothing.
 * Limits: 2 <= N < 2^31, F >= 1, 1 <= C <= MMVAE_SIL_MAXC; row offsets are 64-bit; class sizes are exact in fp32 below 2^24 rows.
 * MMVAE_ERR_ARG (nothing enqueued): a null struct, null x / class_start / s / work, a size out of range, ld_x < F, a pointer not
 *   aligned to its element (work: 8 bytes), work_bytes too small, splits outside [0, 64].  MMVAE_ERR_DTYPE: an x_dtype that is neither
 *   MMVAE_F32 nor MMVAE_BF16.
 * ------------------------------------------------------------------------------------------- */
#define MMVAE_SIL_MAXC 64
typedef struct {
    const void* x; const float* shift; const int32_t* order; const int32_t* class_start;
    float* s; float* intra; float* inter; void* work;
    int64_t ld_x, work_bytes;
    int32_t N, F, C, splits, x_dtype, pad_;
} mmvae_silhouette_args;
int mmvae_silhouette_samples(const mmvae_silhouette_args* args, void* stream);
/* need no device; MMVAE_ERR_ARG for N < 2, C outside [1, MMVAE_SIL_MAXC], splits outside [0, 64] or a null result pointer.
 * *splits_used: the number of column splits mmvae_silhouette_samples uses for (N, C, splits). */
int mmvae_silhouette_work_bytes(int32_t N, int32_t C, int32_t splits, int64_t* bytes);
int mmvae_silhouette_splits(int32_t N, int32_t C, int32_t splits, int32_t* splits_used);

/* ---------------------------------------------------------------------------------------------
 * The two passes of an exact PCA over the data (pca.hip): the centred scatter matrix and the projection onto the components.  With
 * the eigen-solve of the F x F matrix between them (the caller's) they replace PCA(n_components=2, random_state=42).fit_transform(
 * StandardScaler().fit_transform(features)) and the PCA(50) in front of t-SNE over host copies
 * (src/clustering_evaluation/cluster_imputation_methods.py:140-187).
 *
 * mmvae_pca_scatter:  S[a][b] = sum_i (x_ia - c_a)~ (x_ib - c_b)~   (~: rounded to fp32)
 *   x [N][F]: MMVAE_F32 or MMVAE_BF16, row-major, ld_x >= F in elements (padded bf16 rows, see mmvae_rows_to_bf16, included; loads are
 *   as wide as base and stride allow; pad columns and rows outside the matrix are never read).  shift [F] (fp32, NULL = 0) is
 *   subtracted from every element in fp32 on load, as in mmvae_knn_search: pass the column means.  s [F][F]: fp32, ld_s >= F.
 * Products and sums in fp32 on the exact-f32 MFMA path, bf16 storage widened, never multiplied as bf16.  The rows are the GEMM's K
 * dimension; both operands are column tiles of one row tile of x, so no load is transposed.  Only the T (T + 1) / 2 pairs of 128 x 128
 * tiles on or above the diagonal are computed, T = ceil(F / 128); element (a, b), a <= b, is stored at S[a][b] and at S[b][a], inside
 * a diagonal tile too: S is bitwise symmetric.  Every element is one fused-multiply-add chain over its split's rows in ascending
 * order, then the splits in ascending order: no float atomics, the same arguments and split count give the same bits.
 * Rounding steps on the longest path of a term: 1 per centred operand, then at most N (rows_of_split fused multiply-adds +
 * splits_used - 1 additions <= N, every split being non-empty).
 * splits: 0 = the library chooses, 1 .. 64 forces that many; mmvae_pca_scatter_splits returns the count used:
 *   P = T (T + 1) / 2,  chunks = ceil(N / 32)
 *   want = splits > 0 ? splits : max(1, min(floor(512 / P), floor(chunks / 8)))      (512: the workgroups resident at once)
 *   want = min(want, 64, chunks);  chunks_per_split = ceil(chunks / want);  splits_used = ceil(chunks / chunks_per_split)
 * Split s takes the rows 32 s chunks_per_split .. (consecutive runs, none empty).  With more than one split every split writes its whole
 * partial tiles to `work` and a second small launch adds them in ascending split order and writes both triangles; with one split the
 * main kernel writes S itself and work may be NULL.
 * work: caller-owned, 8-byte aligned, at least mmvae_pca_scatter_work_bytes(N, F, splits) bytes = 65 536 P splits_used when
 * splits_used > 1, else 0; the library allocates nothing.
 * Limits: N >= 1, 1 <= F <= 4 194 304 (P is a grid dimension); row offsets are 64-bit.
 * MMVAE_ERR_ARG (nothing enqueued): a null struct, null x / s, null work where bytes > 0, a size < 1, ld_x < F or ld_s < F, a pointer
 *   not aligned to its element (work: 8 bytes), work_bytes too small, splits outside [0, 64].  MMVAE_ERR_DTYPE: an x_dtype that is
 *   neither MMVAE_F32 nor MMVAE_BF16.
 *
 * mmvae_pca_project:  y[i][j] = sum_f (x_if - c_f)~ v[j][f]
 *   x, shift as above; v [k][F]: fp32, ld_v >= F; y [N][k]: fp32, ld_y >= k; 1 <= k <= MMVAE_PCA_MAXK (the reference's 2 and 50).
 * A workgroup owns 128 rows and walks F in chunks of 32 columns, staging the chunk of all k components in LDS (v does not fit whole).
 * y[i][j] is one fused-multiply-add chain over f in ascending order on the exact-f32 MFMA path: its bits depend only on row i's
 * values, shift and v -- not on N, on where the row sits or on a leading dimension.  Rounding steps per term: 1 for the centred
 * operand, then at most F.
 * MMVAE_ERR_ARG (nothing enqueued): a null struct, null x / v / y, a size < 1, k outside [1, MMVAE_PCA_MAXK], a leading dimension
 *   below its width, a pointer not aligned to its element.  MMVAE_ERR_DTYPE: another x_dtype.
 * ------------------------------------------------------------------------------------------- */
#define MMVAE_PCA_MAXK 64
typedef struct {
    const void* x; const float* shift; float* s; void* work;
    int64_t ld_x, ld_s, work_bytes;
    int32_t N, F, splits, x_dtype;
} mmvae_pca_scatter_args;
int mmvae_pca_scatter(const mmvae_pca_scatter_args* args, void* stream);
/* need no device; MMVAE_ERR_ARG for N < 1, F outside [1, 4 194 304], splits outside [0, 64] or a null result pointer.
 * *splits_used: the number of row splits mmvae_pca_scatter uses for (N, F, splits). */
int mmvae_pca_scatter_splits(int32_t N, int32_t F, int32_t splits, int32_t* splits_used);
int mmvae_pca_scatter_work_bytes(int32_t N, int32_t F, int32_t splits, int64_t* bytes);
typedef struct {
    const void* x; const float* shift; const float* v; float* y;
    int64_t ld_x, ld_v, ld_y;
    int32_t N, F, k, x_dtype;
} mmvae_pca_project_args;
int mmvae_pca_project(const mmvae_pca_project_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * sklearn.preprocessing.StandardScaler on the device (standardize.hip), the first step of every row of the clustering tables
 * (src/clustering_evaluation/cluster_imputation_methods.py:112-118, cluster_reconstructed.py), on a feature matrix that is GIVEN AS
 * COLUMN BLOCKS and assembled while it is standardised: the [original | imputed] matrix never exists unstandardised.
 *
 * Operand: `rows` samples and n_parts (1 .. MMVAE_STD_MAX_PARTS) parts.  A part is x, dtype (MMVAE_F32 / MMVAE_BF16), cols >= 1 and
 *   either a (rows, cols) row-major matrix with ld >= cols (in elements), or, with one_row != 0, ONE row of cols values that stands
 *   for every sample (ld is ignored).  F = the sum of the parts' cols (64-bit: no upper limit); column j of the matrix lies in exactly
 *   one part.  A part's pointer is aligned to its element and to nothing more; pad columns and rows outside a part are never read.
 *
 * mmvae_standardize_fit: StandardScaler().fit on float32 data.  mean, var, scale: float64 [F] each.
 *   a_i = (double)x_ij - (double)x_0j  (the column's first row is the shift, the same in every split)
 *   S0 = sum_i a_i,  S1 = sum_i a_i^2,  d = S0 / rows,  mean = x_0j + d,  var = max(S1 / rows - d^2, 0)     (all float64)
 *   scale = 1 where var <= rows eps var + (rows mean eps)^2 (eps of float64: sklearn's constant-feature rule), else sqrt(var).
 *   A column of one value, and every column of a one-row part, has a_i = 0: mean = the value, var = 0 and scale = 1 exactly.
 *   The rows are cut into splits_used consecutive runs of rows_per_split = ceil(rows / want) rows (the last may be short, none is empty):
 *     ctiles = ceil(F / 64);  want = splits > 0 ? splits : max(1, min(floor(2048 / ctiles), floor(rows / 32)))
 *     want = min(want, 64, rows);  splits_used = ceil(rows / rows_per_split)                (mmvae_standardize_fit_splits)
 *   Inside a split the rows r0 + w, r0 + w + 4, ... are summed in ascending order by wave w = 0 .. 3, the four waves are added in wave
 *   order, the pair (S0, S1) of a split goes to work[split][2][F], and a second launch adds the splits in ascending order.  No
 *   floating-point atomics: the same arguments and split count give the same bits, whatever `work` held before (every slot that is
 *   read is written first by the same call).  Additions on the longest path of a sum: at most rows + 3 + splits_used.
 *   work: caller-owned, 8-byte aligned, at least mmvae_standardize_fit_work_bytes(rows, F, splits) = 16 F splits_used bytes.
 *   MMVAE_ERR_ARG (nothing enqueued): a null struct, rows < 1, n_parts outside 1 .. MMVAE_STD_MAX_PARTS, a part with cols < 1, a null
 *   or misaligned x, or (a matrix part) ld < cols; no matrix part at all; null or misaligned (8 bytes) mean / var / scale / work;
 *   work_bytes too small; splits outside [0, 64].  MMVAE_ERR_DTYPE: a part's dtype that is neither MMVAE_F32 nor MMVAE_BF16.
 *
 * mmvae_standardize_apply: StandardScaler.transform.  mean, scale: float64 [F], from any fit.  z [rows][ldz]: fp32, ldz >= F.
 *   z_ij = (float)(((double)x_ij - mean_j) / scale_j): one float64 subtraction, one float64 DIVISION (not a multiplication by a
 *   reciprocal), one rounding to fp32, nothing contracted -- the bits of numpy's ((x.astype(f8) - mean) / scale).astype(f4).
 *   Columns F .. ldz - 1 of z are not written.  z must not overlap a part.  Parts may all be one-row here.
 *   MMVAE_ERR_ARG (nothing enqueued): as above for rows and the parts; null mean / scale / z or one not aligned to its element;
 *   ldz < F.  MMVAE_ERR_DTYPE: as above.
 * ------------------------------------------------------------------------------------------- */
#define MMVAE_STD_MAX_PARTS 4
typedef struct { const void* x; int64_t ld; int32_t cols, dtype, one_row, pad_; } mmvae_std_part;
typedef struct {
    mmvae_std_part part[MMVAE_STD_MAX_PARTS];
    double* mean; double* var; double* scale; void* work;
    int64_t work_bytes;
    int32_t rows, n_parts, splits, pad_;
} mmvae_standardize_fit_args;
int mmvae_standardize_fit(const mmvae_standardize_fit_args* args, void* stream);
/* need no device; MMVAE_ERR_ARG for rows < 1, F < 1, splits outside [0, 64] or a null result pointer */
int mmvae_standardize_fit_splits(int32_t rows, int64_t F, int32_t splits, int32_t* splits_used);
int mmvae_standardize_fit_work_bytes(int32_t rows, int64_t F, int32_t splits, int64_t* bytes);
typedef struct {
    mmvae_std_part part[MMVAE_STD_MAX_PARTS];
    const double* mean; const double* scale; float* z;
    int64_t ldz;
    int32_t rows, n_parts;
} mmvae_standardize_apply_args;
int mmvae_standardize_apply(const mmvae_standardize_apply_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * t-SNE in two dimensions with the exact all-pairs repulsion (tsne.hip): sklearn's TSNE(2, method="barnes_hut") at angle = 0 -- the
 * sparse P of the int(3 perplexity + 1) nearest neighbours, every pair in the repulsion -- with no tree.  Replaces
 * TSNE(n_components=2, random_state=42, perplexity=min(30, n - 1)) over host copies
 * (src/clustering_evaluation/cluster_imputation_methods.py:140-187).  fp32 throughout, no atomics; every sum has one fixed order, so
 * the same arguments and split count give the same bits.  The neighbour search in front is mmvae_knn_search, the symmetrisation of P
 * (a sort of 64-bit keys) is the caller's.
 *
 * mmvae_tsne_affinities: sklearn's _binary_search_perplexity, a wave per row.
 *   dist2 [N][k] (fp32, ld_dist2 >= k): a row's squared distances to its k neighbours, the row itself not among them.
 *   p [N][k] (fp32, ld_p >= k): p_{j|i} = exp(-beta_i (d_ij - m_i)) / sum_j exp(-beta_i (d_ij - m_i)), m_i = min_j d_ij (p and the entropy
 *   do not depend on m; with it the largest exponential is exp(0) = 1 and the sum cannot underflow, where sklearn adds an epsilon).
 *   beta [N]: the precision the search ended on, the one p was evaluated at.  The search: beta = 1; H = log(sum) + beta sum_j (d - m) p_j;
 *   done when |H - log(perplexity)| <= 1e-5; H too large: beta doubles while no upper bracket exists, else bisects upwards; otherwise it
 *   halves while no lower bracket exists, else bisects downwards; at most 100 evaluations whatever the data (a row of equal distances
 *   runs all 100 and gets p = 1 / k; a row with inf or NaN ends too, with NaN in p).  A row's lanes add its terms 64 apart, then a fixed
 *   butterfly: at most ceil(k / 64) + 6 additions deep.  expf, logf: the device library's (1 ulp); the division is correctly rounded.
 *   MMVAE_ERR_ARG (nothing enqueued): a null struct or pointer, N < 1, k < 1, perplexity <= 0 or >= k (or NaN), a leading dimension
 *   below k, a pointer not aligned to 4 bytes.
 *
 * mmvae_tsne_gradient: the gradient of KL(P || Q) at the embedding y, two launches.
 *   y [N][2] (fp32, contiguous, 8-byte aligned).  P as CSR: row_ptr [N + 1], col [nnz] (int32), val [nnz] (fp32); it cannot be
 *   validated at the call: row_ptr is clamped to [0, nnz] and made non-decreasing per row, col to [0, N), so a bad matrix gives wrong
 *   numbers but no access out of range.  No order of a row's entries is assumed; the attraction's bits depend on it.
 *   w_ij = 1 / (1 + |y_i - y_j|^2)        A_i = sum_{j in P(i)} p_ij w_ij (y_i - y_j)        R_i = sum_{j != i} w_ij^2 (y_i - y_j)
 *   Z = sum_{i != j} w_ij                  grad [N][2] = 4 (exaggeration A_i - R_i / Z)
 *   z [1]: Z.  err [N] (optional): err_i = sum_{j in P(i), p_ij > 0} p_ij (log p_ij + log(1 + |y_i - y_j|^2) + log Z); their sum is
 *   sklearn's Barnes-Hut error sum p log(p / q) over the stored entries (the caller adds them: in float64, in one fixed order).  p is
 *   used as given: with exaggeration != 1 sklearn's error would take exaggeration p inside the logarithm too.  z_row [N] (optional):
 *   z_i = sum_{j != i} w_ij.
 *   1 + d^2 is fma(dy, dy, fma(dx, dx, 1)); w is v_rcp_f32 of it (1 ulp); the diagonal pair gets w = 0, so it adds exactly 0 to R_i and
 *   nothing to z_i; columns >= N are never walked.
 *   Repulsion launch: a workgroup owns 512 rows (a lane rows t and t + 256 of the block, in registers) and walks its split's columns in
 *   ascending order, 1024 at a time through LDS (every lane reads the same y_j: a broadcast): R_i and z_i of a split are single chains of
 *   its columns.  The columns are cut into splits_used consecutive runs of 64-column chunks:
 *     blocks = ceil(N / 512),  chunks = ceil(N / 64)
 *     want = splits > 0 ? splits : (blocks >= 2048 ? 1 : ceil(2048 / blocks));   want = min(want, 64, chunks)
 *     chunks_per_split = ceil(chunks / want);   splits_used = ceil(chunks / chunks_per_split)        (mmvae_tsne_gradient_splits)
 *   Every split writes (R_x, R_y, z_i) per row, and every workgroup one fp32 sum of its rows' z_i (a lane's two rows, a 6-step butterfly
 *   over the wave, the four waves in order: at most 1 + 6 + 3 additions on top of z_i), to `work`.
 *   Second launch: Z = the float64 sum of the splits_used x blocks workgroup sums (256 strided chains, then a binary tree of 8 levels; the
 *   same in every workgroup), rounded to fp32.  A wave per row: the row's partials in ascending split order; the row's entries 64 apart
 *   per lane (any row length), the lane sums of A_i and err_i by a 6-step butterfly; R_i / Z is a correctly rounded division.
 *   work: caller-owned, 8-byte aligned, at least mmvae_tsne_gradient_work_bytes(N, splits) = 12 N splits_used + 4 splits_used blocks
 *   bytes (each rounded up to 8); the library allocates nothing.
 *   Limits: 2 <= N, 0 <= nnz < 2^31.  Z underflows to 0 (and grad is not finite) only when every |y_i - y_j|^2 exceeds about 1e38.
 *   MMVAE_ERR_ARG (nothing enqueued): a null struct, null y / row_ptr / grad / z / work, null col or val with nnz > 0, N < 2, nnz < 0,
 *   splits outside [0, 64], a pointer not aligned to its element (y, work: 8 bytes), work_bytes too small.
 *
 * mmvae_tsne_update: one step of sklearn's _gradient_descent, in place, an element e of the 2 N per thread:
 *   gains_e = max(update_e grad_e < 0 ? gains_e + 0.2 : 0.8 gains_e, 0.01);   update_e = fma(momentum, update_e, -(learning_rate (grad_e gains_e)));
 *   y_e += update_e.
 *   grad_norm [1] (optional): |gains * grad|_2, the norm sklearn's stopping rule reads (it takes it after grad *= gains): squares added
 *   by a butterfly per wave, the four waves in order, then the workgroups' sums in float64 by a second one-workgroup launch (256
 *   strided chains and a binary tree), the square root rounded to fp32.  It needs work: 8-byte aligned, at least
 *   mmvae_tsne_update_work_bytes(N) = 4 ceil(2 N / 256) bytes (rounded up to 8).
 *   MMVAE_ERR_ARG (nothing enqueued): a null struct, null y / update / gains / grad, N < 1, a misaligned pointer, grad_norm without
 *   enough work.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const float* dist2; float* p; float* beta;
    int64_t ld_dist2, ld_p;
    int32_t N, k; float perplexity; int32_t pad_;
} mmvae_tsne_affinities_args;
int mmvae_tsne_affinities(const mmvae_tsne_affinities_args* args, void* stream);
typedef struct {
    const float* y; const int32_t* row_ptr; const int32_t* col; const float* val;
    float* grad; float* z; float* err; float* z_row; void* work;
    int64_t nnz, work_bytes;
    int32_t N, splits; float exaggeration; int32_t pad_;
} mmvae_tsne_gradient_args;
int mmvae_tsne_gradient(const mmvae_tsne_gradient_args* args, void* stream);
/* need no device; MMVAE_ERR_ARG for N < 2, splits outside [0, 64] or a null result pointer. */
int mmvae_tsne_gradient_splits(int32_t N, int32_t splits, int32_t* splits_used);
int mmvae_tsne_gradient_work_bytes(int32_t N, int32_t splits, int64_t* bytes);
typedef struct {
    float* y; float* update; float* gains; const float* grad; float* grad_norm; void* work;
    int64_t work_bytes;
    int32_t N; float momentum, learning_rate; int32_t pad_;
} mmvae_tsne_update_args;
int mmvae_tsne_update(const mmvae_tsne_update_args* args, void* stream);
int mmvae_tsne_update_work_bytes(int32_t N, int64_t* bytes);

/* ---------------------------------------------------------------------------------------------
 * The site classifier of the downstream task (classifier.hip): what SimpleMLP's training step (downstream_task.py:55-159; the
 * directional script's MLP, downstream_task_directional.py, has no LayerNorm) needs beside the fp32 GEMMs.  fp32 in and out, a wave
 * per row; no float atomics on anything a gradient is read from, every sum has one fixed order: the same arguments give the same bits.
 *
 * mmvae_ln_act_fwd: nn.LayerNorm(N) -> ReLU -> Dropout (downstream_task.py:58-66) in one pass over z [M][ldz], the row in registers.
 *   mean_i = sum_j z_ij / N        var_i = sum_j (z_ij - mean_i)^2 / N   (biased, about the mean)        rstd_i = 1 / sqrt(var_i + eps)
 *   y_ij = relu(xhat_ij gamma_j + beta_j) keep_ij inv_keep,   xhat_ij = (z_ij - mean_i) rstd_i;   mean [M] and rstd [M] are written.
 *   mask: the uint8 keep mask of mmvae_noise ([M][ld_mask], bytes 0 or 1), inv_keep = 1 / (1 - p); NULL (eval mode, p = 0): no scaling.
 *   layer_norm == 0: y = relu(z) keep inv_keep; gamma, beta, mean, rstd and eps are not read.
 *   A lane adds its chunks' four elements pairwise, chunks 64 apart, then a 6-step butterfly: at most 2 + ceil(N / 256) + 6 additions deep.
 *   Limits: M >= 1; N a multiple of 4, 4 <= N <= MMVAE_LN_MAXN (a lane holds N / 256 16-byte chunks); leading dimensions multiples of 4
 *   and >= N; z, y, gamma, beta 16-byte aligned, the mask 4-byte aligned.
 *   MMVAE_ERR_ARG (nothing enqueued): a null struct, null z / y, with layer_norm null gamma / beta / mean / rstd or eps <= 0, a size or
 *   leading dimension outside the limits, a misaligned pointer, a mask with inv_keep < 1.
 *
 * mmvae_ln_act_bwd: from dy = dL/dy and the forward's z, mean, rstd, gamma, beta, mask:
 *   g_ij = dy_ij keep_ij inv_keep [xhat_ij gamma_j + beta_j > 0]
 *   dz_ij = rstd_i (g_ij gamma_j - mean_j(g gamma) - xhat_ij mean_j(g gamma xhat))        dgamma_j = sum_i g_ij xhat_ij        dbeta_j = sum_i g_ij
 *   dgamma, dbeta [N] are WRITTEN.  A workgroup owns 32 consecutive rows: a wave adds its rows (w, w + 4, ...) in ascending order, the four
 *   waves are added in order, and with more than one workgroup the partial sums go to `work` and a second small launch adds them in
 *   ascending workgroup order; a launch of one workgroup (M <= 32, the training batch) writes dgamma / dbeta itself.
 *   work: caller-owned, 8-byte aligned, at least mmvae_ln_act_bwd_work_bytes(M, N, layer_norm) = 8 N ceil(M / 32) bytes when layer_norm
 *   and M > 32, else 0 (work may then be NULL).  layer_norm == 0: dz = dy keep inv_keep [z > 0], nothing else is read or written.
 *   Limits and refusals as mmvae_ln_act_fwd, for dy / z / dz (16-byte aligned, leading dimensions multiples of 4); also null dgamma /
 *   dbeta with layer_norm, a missing, misaligned or short workspace.
 *
 * mmvae_wce_mean: nn.CrossEntropyLoss(weight = w) with its mean reduction and torch.max(outputs, 1) (downstream_task.py:83,101,123).
 *   logits [M][ld] fp32, 2 <= C <= MMVAE_WCE_MAXC, labels int64 [M], class_weights fp32 [C] or NULL (= 1).  A wave per row, a lane per class.
 *   nll_i = max_i + log(sum_j exp(x_ij - max_i)) - x_{i,y_i}                  sums[0] += sum_i w_{y_i} nll_i,  sums[1] += sum_i w_{y_i}   (f64)
 *   g_ij = w_{y_i} (softmax_ij - [j == y_i]) / W,   W = sum_i w_{y_i} over ALL M rows of the call: the gradient of sums[0] / sums[1].
 *   W is formed by every workgroup from all M labels in one order (float64; thread t of 256 the labels t, t + 256, ..., a butterfly
 *   per wave, the four waves in order; rounded to fp32): the same bits in every workgroup, no launch in front.  All weights zero: g is NaN,
 *   as torch's.
 *   pred [M] (int32): the argmax, the FIRST maximum on ties (a row holding NaN gives 0).  nll [M] (fp32, optional): the unweighted row
 *   terms, from which the host forms the mean of per-batch means of one evaluation launch.  confusion [C][C] (int32, optional):
 *   += 1 at [y_i][pred_i] (integer atomics: exact).
 *   Labels as in mmvae_vae_loss: -100 is ignored (weight 0, not counted in confusion); any other label outside [0, C) is counted in
 *   sums[2] and computed as class 0 (not counted in confusion) -- the caller raises.
 *   Every one of sums (f64 [3], accumulated: zero it first), g (ldg >= C), pred, nll, confusion may be NULL, not all of them.
 *   MMVAE_ERR_ARG (nothing enqueued): a null struct, null logits / labels, M < 1, C outside [2, MMVAE_WCE_MAXC], ld or ldg below C, a
 *   pointer not aligned to its element, no output at all.
 * ------------------------------------------------------------------------------------------- */
#define MMVAE_LN_MAXN 1024
#define MMVAE_WCE_MAXC 64
typedef struct {
    const float* z; const float* gamma; const float* beta; const uint8_t* mask;
    float* y; float* mean; float* rstd;
    int64_t ldz, ld_mask, ldy;
    int32_t M, N, layer_norm; float eps, inv_keep; int32_t pad_;
} mmvae_ln_act_fwd_args;
int mmvae_ln_act_fwd(const mmvae_ln_act_fwd_args* args, void* stream);
typedef struct {
    const float* dy; const float* z; const float* mean; const float* rstd; const float* gamma; const float* beta; const uint8_t* mask;
    float* dz; float* dgamma; float* dbeta; void* work;
    int64_t lddy, ldz, ld_mask, lddz, work_bytes;
    int32_t M, N, layer_norm; float inv_keep;
} mmvae_ln_act_bwd_args;
int mmvae_ln_act_bwd(const mmvae_ln_act_bwd_args* args, void* stream);
/* needs no device; MMVAE_ERR_ARG for M < 1, an N outside the limits or a null result pointer */
int mmvae_ln_act_bwd_work_bytes(int32_t M, int32_t N, int32_t layer_norm, int64_t* bytes);
typedef struct {
    const float* logits; const int64_t* labels; const float* class_weights;
    double* sums; float* g; int32_t* pred; float* nll; int32_t* confusion;
    int64_t ld, ldg;
    int32_t M, C;
} mmvae_wce_args;
int mmvae_wce_mean(const mmvae_wce_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * AdamW (torch.optim.AdamW, constructed by the caller: optimize_hyperparameters.py:93-97,
 * train_dna2rna.py:185-189), all tensors in one launch per 64 tensors (every record is checked before the first launch).  `items_host` is an array in HOST memory
 * (device pointers inside); it is copied into the kernel arguments, so nothing is uploaded and the call is graph-capturable:
 *   p *= 1-lr*wd ; m = b1*m+(1-b1)g ; v = b2*v+(1-b2)g^2 ; p -= lr/bc1 * m/(sqrt(v)/sqrt(bc2)+eps)
 * ------------------------------------------------------------------------------------------- */
typedef struct { float* p; const float* g; float* m; float* v; int64_t n; } mmvae_adamw_item;
int mmvae_adamw_step(const mmvae_adamw_item* items_host, int32_t n_items, float lr, float beta1,
                     float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, int32_t maximize,
                     uint64_t* step_dev, int32_t advance, const float* lr_dev, void* stream);
/* step_dev != NULL: bias corrections are computed in the kernel from t = *step_dev + 1 (graph-capturable) and
 * bias_corr1/2 are ignored.  advance != 0 (n_items <= 64): step_dev holds MMVAE_CTR_COPIES identical copies of the count and
 * the launch increments all of them itself (see mmvae_noise); otherwise advance the counter with mmvae_counter_add.
 * lr_dev != NULL: the learning rate is read from device memory (a captured graph follows ReduceLROnPlateau,
 * train_dna2rna.py:190-195,216, without re-capture). */

/* Adam with the weight decay COUPLED into the gradient (torch.optim.Adam(lr, weight_decay), downstream_task.py:84): the same kernel
 * source, items, by-value batch and step_dev / advance / lr_dev forms as mmvae_adamw_step, only the decay differs:
 *   g' = g + wd*p ; m = b1*m+(1-b1)g' ; v = b2*v+(1-b2)g'^2 ; p -= lr/bc1 * m/(sqrt(v)/sqrt(bc2)+eps)
 * (maximize negates g before the decay is added, as torch does). */
int mmvae_adam_step(const mmvae_adamw_item* items_host, int32_t n_items, float lr, float beta1,
                    float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, int32_t maximize,
                    uint64_t* step_dev, int32_t advance, const float* lr_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_HIP_H */
