// The class head of the training step in ONE launch (gfx950): mmvae_class_tail (include/mmvae_hip.h lists the limits).
//
// Replaces, in the captured MultiModalVAE step: the last Linear of DecoderC (reference src/models/decoders.py:46: 64 -> n_sites), the
// class + KL part of vae_loss (src/utils/losses.py:39,42) and that Linear's dX GEMM behind the ReLU mask -- three launches that each
// move a few MB, hand the logits and the class gradient to each other through HBM and read the hidden activation twice.
//
// One persistent workgroup of 8 waves per CU.  W (32 x 64), W^T (64 x 32), the bias and the class weights stay in LDS for the whole
// launch.  A wave owns 16-row slabs and carries each from the hidden activation to its gradient:
//   * the slab's h0 rows are loaded straight in MFMA fragment layout (lane (li, lg): row li, k = 32 j + 8 lg ..), with the labels and
//     the slab's mu / logvar elements; the NEXT slab's loads are issued before the current slab is worked on;
//   * logits: 2 MFMAs per 16 columns with the operands swapped as in the tile kernels (gemm_nt_epi.h), K ascending, bias in fp32;
//   * cross-entropy (loss_terms.h, the arithmetic of vae_loss_kernel's row-per-thread path): the row maximum over the row's four
//     lanes, one exp per logit, the exps through a wave-private LDS image so that every lane of the row adds them in ascending
//     order; the fp32 gradient leaves through the same image as contiguous 16-byte pieces;
//   * dX: the gradient rounded to bf16 is the MFMA operand (a wave-private LDS image: element order of the fragment), one MFMA per
//     16 hidden columns, two column blocks of 32 interleaved so that a lane owns 8 consecutive columns -- the columns of the h0
//     fragments it still holds, which are the ReLU mask; halves swapped between lanes li and li ^ 8 (DPP): whole 128-byte lines;
//   * KL: the slab's 16 L elements, up to 6 per lane.
// No workgroup barrier between the set-up and the final reduction of the three sums: the waves never wait for each other.
#include "common.h"
#include "mmvae_hip.h"
#include "loss_terms.h"
#include "wave_slab.h"

namespace mm {

constexpr int CT_WAVES = 8, CT_THREADS = 64 * CT_WAVES;
constexpr int CT_SP = 32;                         // class columns in LDS: two MFMA tiles
constexpr int CT_HID = 64;                        // hidden width
constexpr int CT_KU = 6;                          // KL elements per lane and slab: 16 rows x L <= 24
constexpr int CT_WROW = 2 * CT_HID + 16;          // W row (64 bf16) + the pad chunk of every LDS row (wave_slab.h)
constexpr int CT_TROW = 2 * CT_SP + 16;           // W^T row and gradient-image row (32 bf16)
constexpr int CT_XLD = CT_SP + 4;                 // floats per row of the logit / exp images
constexpr int CT_OFF_WT = CT_SP * CT_WROW;
constexpr int CT_OFF_BIAS = CT_OFF_WT + CT_HID * CT_TROW;
constexpr int CT_OFF_CW = CT_OFF_BIAS + CT_SP * 4;
constexpr int CT_OFF_RED = CT_OFF_CW + CT_SP * 4;                    // [8][3] doubles
constexpr int CT_OFF_SCR = CT_OFF_RED + CT_WAVES * 3 * 8;
constexpr int CT_SCR_E = 16 * CT_XLD * 4;                            // per wave: logit image (then fp32 gradient), exp image,
constexpr int CT_SCR_G = 2 * CT_SCR_E;                               // bf16 gradient image
constexpr int CT_SCR = CT_SCR_G + 16 * CT_TROW;
constexpr int CT_LDS = CT_OFF_SCR + CT_WAVES * CT_SCR;               // 56 KB
static_assert(CT_OFF_SCR % 16 == 0 && CT_SCR % 16 == 0 && CT_SCR_E % 16 == 0, "16-byte LDS vectors");

struct CtArgs {
    int B, S, L, nslabs;
    const bf16* h0; long ldh; const bf16* w; long ldw; const bf16* wt; long ldwt; const float* bias;
    const long long* site; const float* cw; const float* mu; const float* lv;
    float beta, gamma; const float* bg; double* sums;
    float* gc; long ldgc; bf16* d0; long ldd; float* gmu; float* glv;
};

__global__ __launch_bounds__(CT_THREADS) void class_tail_kernel(const CtArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    float* const sbias = (float*)(smem + CT_OFF_BIAS);
    float* const scw = (float*)(smem + CT_OFF_CW);
    double* const red = (double*)(smem + CT_OFF_RED);
    unsigned char* const scr = smem + CT_OFF_SCR + wid * CT_SCR;
    float* const sx = (float*)scr;
    float* const sexp = (float*)(scr + CT_SCR_E);
    unsigned char* const sg = scr + CT_SCR_G;
    float beta = a.beta, gamma = a.gamma;
    if (a.bg) { beta = a.bg[0]; gamma = a.bg[1]; }                    // hyper-parameters a captured graph can change
    const int S = a.S, L = a.L, total = a.B * L;

    bf16x8 hn[2];
    long long yn = 0;
    float mun[CT_KU] = {}, lvn[CT_KU] = {};
    auto fetch = [&](int slab) __attribute__((always_inline)) {
        const int row = min(slab * 16 + li, a.B - 1);                 // clamped: the loads always issue
        const bf16* hp = a.h0 + (long)row * a.ldh + 8 * lg;
        hn[0] = *(const bf16x8*)hp;
        hn[1] = *(const bf16x8*)(hp + 32);
        yn = a.site[row];
#pragma unroll
        for (int i = 0; i < CT_KU; ++i) {
            if (64 * i >= 16 * L) break;                              // kernel-uniform, around loads only
            const int idx = min(slab * 16 * L + lane + 64 * i, total - 1);
            mun[i] = a.mu[idx]; lvn[i] = a.lv[idx];
        }
    };

    const int nw = gridDim.x * CT_WAVES;
    int slab = blockIdx.x * CT_WAVES + wid;
    if (slab < a.nslabs) fetch(slab);          // the first slab's loads fly under the set-up: they depend on nothing in LDS

    // ---------------------------------------------------------------------------------- once per workgroup
    stage_rows<CT_THREADS>(smem, CT_WROW, a.w, a.ldw, CT_SP, 8, tid, EpiCols<false>::wrow);
    stage_rows<CT_THREADS>(smem + CT_OFF_WT, CT_TROW, a.wt, a.ldwt, CT_HID, 4, tid, EpiCols<true>::wrow);      // a lane's 8 dX accumulators of a tile pair: 8 consecutive columns
    if (tid < CT_SP) {
        sbias[tid] = (a.bias && tid < S) ? a.bias[tid] : 0.f;
        scw[tid] = (a.cw && tid < S) ? a.cw[tid] : 1.f;
    }
    __syncthreads();

    double dcls = 0.0, dkl = 0.0;
    float nbad = 0.f;
    const int vpr = S >> 2;                                            // 16-byte pieces per gradient row
    for (; slab < a.nslabs; slab += nw) {
        const bf16x8 hv[2] = {hn[0], hn[1]};
        const long long yl = yn;
        float mu[CT_KU], lv[CT_KU];
#pragma unroll
        for (int i = 0; i < CT_KU; ++i) { mu[i] = mun[i]; lv[i] = lvn[i]; }
        if (slab + nw < a.nslabs) fetch(slab + nw);                    // the next slab's loads fly under this one
        const int row = slab * 16 + li;
        const bool rok = row < a.B;

        // ------------------------------------------------------------------------------ logits: K ascending, bias in fp32
        f32x4 x[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bf16x8 wf = *(const bf16x8*)(smem + (16 * n + li) * CT_WROW + (4 * j + lg) * 16);
                Mma<bf16>::mma(acc, wf, hv[j]);                       // swapped operands: the lane holds row li, columns 16 n + 4 lg ..
            }
            x[n] = acc + *(const f32x4*)(sbias + 16 * n + 4 * lg);
        }
        // ------------------------------------------------------------------------------ cross-entropy of the row (loss_terms.h)
        float m = -INFINITY;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (16 * n + 4 * lg + j >= S) x[n][j] = -INFINITY;
                m = fmaxf(m, x[n][j]);
            }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        f32x4 e[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
#pragma unroll
            for (int j = 0; j < 4; ++j) e[n][j] = (16 * n + 4 * lg + j < S) ? ce_exp(x[n][j], m) : 0.f;
            *(f32x4*)(sx + li * CT_XLD + 16 * n + 4 * lg) = x[n];
            *(f32x4*)(sexp + li * CT_XLD + 16 * n + 4 * lg) = e[n];
        }
        wave_lds_sync();
        float se = 0.f;                                                // every lane of the row: the same sum in ascending order
#pragma unroll
        for (int c = 0; c < CT_SP / 4; ++c) {
            const f32x4 v = *(const f32x4*)(sexp + li * CT_XLD + 4 * c);
#pragma unroll
            for (int j = 0; j < 4; ++j) se += v[j];
        }
        const CeLabel lb = ce_label(yl, S, scw);
        const float xy = sx[li * CT_XLD + lb.y];
        if (lg == 0 && rok) {
            dcls += (double)ce_term(lb.w, m, se, xy);
            if (lb.bad) nbad += 1.f;
        }
        const float gw = gamma * lb.w;
        f32x4 g[2];
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = 16 * n + 4 * lg + j;
                g[n][j] = c < S ? ce_grad(gw, e[n][j], se, c == lb.y) : 0.f;
            }
        wave_lds_sync();                                                // the logit image is read: it takes the fp32 gradient
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            *(f32x4*)(sx + li * CT_XLD + 16 * n + 4 * lg) = g[n];
            const bf16x4 gb = {(bf16)g[n][0], (bf16)g[n][1], (bf16)g[n][2], (bf16)g[n][3]};      // as SrcPlain<bf16, float> rounds it
            *(bf16x4*)(sg + li * CT_TROW + (16 * n + 4 * lg) * 2) = gb;
        }
        wave_lds_sync();
        // the fp32 class gradient (the grouped dW launch reads it): the slab's rows as consecutive 16-byte pieces
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int v = lane + 64 * it;
            const int r = v / vpr, c4 = v - r * vpr;
            if (v < 16 * vpr && slab * 16 + r < a.B)
                *(f32x4*)(a.gc + (long)(slab * 16 + r) * a.ldgc + 4 * c4) = *(const f32x4*)(sx + r * CT_XLD + 4 * c4);
        }
        // ------------------------------------------------------------------------------ dX behind the ReLU mask
        const bf16x8 gf = *(const bf16x8*)(sg + li * CT_TROW + lg * 16);
        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bf16x8 wf = *(const bf16x8*)(smem + CT_OFF_WT + (16 * q + li) * CT_TROW + lg * 16);
            acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            Mma<bf16>::mma(acc[q], wf, gf);
        }
        uint32_t pk[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const f32x4 v = qd < 2 ? acc[2 * h] : acc[2 * h + 1];
                const int e0 = 2 * qd;                                 // hidden columns 32 h + 8 lg + e0, + 1: the lane's own h0 values
                const float o0 = (float)hv[h][e0] > 0.f ? v[2 * (qd & 1)] : 0.f;
                const float o1 = (float)hv[h][e0 + 1] > 0.f ? v[2 * (qd & 1) + 1] : 0.f;
                const bf16x2 t = {(bf16)o0, (bf16)o1};
                pk[h][qd] = __builtin_bit_cast(uint32_t, t);
            }
        }
        SWAP_HALVES(pk, li < 8, st0, st1);
        const int rbase = slab * 16 + (li & 7);
        bf16* const crow = line_col(a.d0 + (long)rbase * a.ldd, li, lg);
        if (rbase < a.B) *(uint4*)crow = uint4{st0[0], st0[1], st0[2], st0[3]};
        if (rbase + 8 < a.B) *(uint4*)(crow + 8 * a.ldd) = uint4{st1[0], st1[1], st1[2], st1[3]};

        // ------------------------------------------------------------------------------ KL of the slab's 16 L elements
#pragma unroll
        for (int i = 0; i < CT_KU; ++i) {
            if (64 * i >= 16 * L) break;
            const int idx = slab * 16 * L + lane + 64 * i;
            if (lane + 64 * i < 16 * L && idx < total) {
                float gm, gl;
                dkl += (double)kl_elem(mu[i], lv[i], beta, gm, gl);
                a.gmu[idx] = gm; a.glv[idx] = gl;
            }
        }
        wave_lds_sync();                               // the images are free for the next slab
    }

    // ---------------------------------------------------------------------------------- the three sums: one f64 atomic each
    const double vc = wave_sum_f64(dcls), vk = wave_sum_f64(dkl);
    const float vb = wave_sum(nbad);
    if (lane == 0) { red[wid * 3] = vc; red[wid * 3 + 1] = vk; red[wid * 3 + 2] = (double)vb; }
    __syncthreads();
    if (tid < 3) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < CT_WAVES; ++w) v += red[w * 3 + tid];
        if (v != 0.0) unsafeAtomicAdd(a.sums + 2 + tid, v);
    }
}

}  // namespace mm

extern "C" int mmvae_class_tail_fits(int32_t prec, int32_t S, int32_t hidden, int32_t L, int64_t ldh0, int64_t ldd0) {
    using namespace mm;
    if (!g_tuning.class_tail_on) return MMVAE_ERR_ARG;
    if (prec != MMVAE_PREC_BF16) return MMVAE_ERR_ARG;
    if (hidden != CT_HID || S < 4 || S > CT_SP || S % 4 || L < 1 || 16 * L > 64 * CT_KU) return MMVAE_ERR_ARG;
    if (ldh0 % 8 || ldh0 < CT_HID || ldd0 % 64 || ldd0 < CT_HID) return MMVAE_ERR_ARG;
    return 0;
}

extern "C" int mmvae_class_tail(const mmvae_class_tail_args* a, void* stream) {
    using namespace mm;
    if (!a) return MMVAE_ERR_ARG;
    { const int rc = mmvae_class_tail_fits(a->prec, a->S, a->hidden, a->L, a->ldh0, a->ldd0); if (rc) return rc; }
    const long wide = a->L > a->S ? a->L : a->S;
    if (a->B <= 0 || (long)a->B * wide >= (1L << 31)) return MMVAE_ERR_ARG;
    if (!a->h0 || !a->w || !a->wt || !a->bias || !a->site || !a->mu || !a->logvar || !a->sums || !a->g_c || !a->d0 || !a->g_mu || !a->g_lv)
        return MMVAE_ERR_ARG;
    if (((uintptr_t)a->h0 & 15) || ((uintptr_t)a->d0 & 127) || ((uintptr_t)a->w & 15) || ((uintptr_t)a->wt & 15)) return MMVAE_ERR_ARG;
    if (a->ldw % 8 || a->ldw < CT_HID || a->ldwt % 8 || a->ldwt < CT_SP) return MMVAE_ERR_ARG;
    if (((uintptr_t)a->g_c & 15) || a->ld_gc % 4 || a->ld_gc < a->S) return MMVAE_ERR_ARG;
    CtArgs k{};
    k.B = a->B; k.S = a->S; k.L = a->L; k.nslabs = (a->B + 15) / 16;
    k.h0 = (const bf16*)a->h0; k.ldh = a->ldh0; k.w = (const bf16*)a->w; k.ldw = a->ldw; k.wt = (const bf16*)a->wt; k.ldwt = a->ldwt;
    k.bias = a->bias; k.site = (const long long*)a->site; k.cw = a->class_weights; k.mu = a->mu; k.lv = a->logvar;
    k.beta = a->beta; k.gamma = a->gamma; k.bg = a->beta_gamma_dev; k.sums = a->sums;
    k.gc = a->g_c; k.ldgc = a->ld_gc; k.d0 = (bf16*)a->d0; k.ldd = a->ldd0; k.gmu = a->g_mu; k.glv = a->g_lv;
    return launch_lds<class_tail_kernel>(dim3(persistent_grid(k.nslabs, CT_WAVES)), dim3(CT_THREADS), CT_LDS, (hipStream_t)stream, k);
}
