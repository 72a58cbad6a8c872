// The site classifier of the downstream task (reference downstream_task.py:55-159, downstream_task_directional.py): what its 32-row
// training step needs beside the GEMMs -- LayerNorm + ReLU + Dropout forward and backward, a wave per row with the row in registers,
// and the mean-reduced weighted cross-entropy with predictions and a confusion matrix.  fp32 in and out, no float atomics on anything
// a gradient is read from: every sum has one fixed order.  (mmvae_adam_step lives beside mmvae_adamw_step in elementwise.hip: one
// kernel source for both decay forms.)
#include "common.h"
#include "loss_terms.h"

namespace mm {

constexpr int LN_ROWS_FWD = 4;       // rows per workgroup of the forward: one per wave
constexpr int LN_ROWS_BWD = 32;      // rows per workgroup of the backward: 8 per wave, so that 32-row batches need no second launch
constexpr int WCE_ROWS = 64;         // rows per workgroup of the loss: 16 per wave

// A wave's row: lane l holds the 16-byte chunks l, l + 64, ... (J of them) of the row's N / 4.
template <int J> struct RowRegs {
    f32x4 v[J];
    __device__ __forceinline__ void load(const float* row, int lane, int nchunks) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = lane + 64 * j;
            v[j] = c < nchunks ? *(const f32x4*)(row + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
};

// keep / (1 - p) of a chunk's four elements: the bytes of mmvae_noise are 0 or 1
__device__ __forceinline__ f32x4 keep_scale(const uint8_t* mrow, int c, float inv_keep) {
    if (!mrow) return f32x4{1.f, 1.f, 1.f, 1.f};
    const uint32_t m = *(const uint32_t*)(mrow + 4 * c);
    return f32x4{(m & 0xffu) ? inv_keep : 0.f, (m & 0xff00u) ? inv_keep : 0.f, (m & 0xff0000u) ? inv_keep : 0.f, (m & 0xff000000u) ? inv_keep : 0.f};
}

// the row's mean, then its biased variance ABOUT that mean (the centred form: E[x^2] - E[x]^2 cancels for rows far from zero)
template <int J>
__device__ __forceinline__ void row_moments(const RowRegs<J>& x, int lane, int nchunks, int N, float& mean, float& var) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) s += (x.v[j][0] + x.v[j][1]) + (x.v[j][2] + x.v[j][3]);          // chunks past the row hold zeros
    mean = wave_sum(s) / (float)N;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j)
        if (lane + 64 * j < nchunks) {
            const f32x4 d = x.v[j] - mean;
            q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
    var = wave_sum(q) / (float)N;
}

template <bool LN, int J>
__global__ __launch_bounds__(256) void ln_act_fwd_kernel(const mmvae_ln_act_fwd_args a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * LN_ROWS_FWD + (threadIdx.x >> 6);
    if (row >= a.M) return;
    const int nchunks = a.N >> 2;
    RowRegs<J> x;
    x.load(a.z + (long)row * a.ldz, lane, nchunks);
    float mean = 0.f, rstd = 1.f;
    if constexpr (LN) {
        float var;
        row_moments<J>(x, lane, nchunks, a.N, mean, var);
        rstd = 1.f / sqrtf(var + a.eps);
        if (lane == 0) { a.mean[row] = mean; a.rstd[row] = rstd; }
    }
    const uint8_t* mrow = a.mask ? a.mask + (long)row * a.ld_mask : nullptr;
    float* yrow = a.y + (long)row * a.ldy;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = lane + 64 * j;
        if (c >= nchunks) break;
        f32x4 pre = x.v[j];
        if constexpr (LN) pre = (x.v[j] - mean) * rstd * *(const f32x4*)(a.gamma + 4 * c) + *(const f32x4*)(a.beta + 4 * c);
        const f32x4 k = keep_scale(mrow, c, a.inv_keep);
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = pre[e] > 0.f ? pre[e] * k[e] : 0.f;
        *(f32x4*)(yrow + 4 * c) = y;
    }
}

// One workgroup owns LN_ROWS_BWD consecutive rows, wave w the rows w, w + 4, ... of them in ascending order.  A lane adds its columns'
// g xhat and g over its wave's rows in registers; the four waves' sums go through LDS and are added in wave order; the workgroup's
// sums go to `work` (or, from a launch of one workgroup, to dgamma / dbeta) and ln_partials_kernel adds them in workgroup order.
template <bool LN, int J>
__global__ __launch_bounds__(256) void ln_act_bwd_kernel(const mmvae_ln_act_bwd_args a) {
    extern __shared__ float lds[];                    // LN: [4 waves][2][N]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nchunks = a.N >> 2;
    const float inv_n = 1.f / (float)a.N;
    f32x4 dg[J], db[J];
#pragma unroll
    for (int j = 0; j < J; ++j) dg[j] = db[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int r_end = min(a.M, ((int)blockIdx.x + 1) * LN_ROWS_BWD);
    for (int row = blockIdx.x * LN_ROWS_BWD + wave; row < r_end; row += 4) {
        RowRegs<J> x, d;
        x.load(a.z + (long)row * a.ldz, lane, nchunks);
        d.load(a.dy + (long)row * a.lddy, lane, nchunks);
        const uint8_t* mrow = a.mask ? a.mask + (long)row * a.ld_mask : nullptr;
        float* orow = a.dz + (long)row * a.lddz;
        if constexpr (!LN) {
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int c = lane + 64 * j;
                if (c >= nchunks) break;
                const f32x4 k = keep_scale(mrow, c, a.inv_keep);
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = x.v[j][e] > 0.f ? d.v[j][e] * k[e] : 0.f;
                *(f32x4*)(orow + 4 * c) = o;
            }
        } else {
            const float mean = a.mean[row], rstd = a.rstd[row];
            f32x4 gg[J];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int c = lane + 64 * j;
                gg[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (c >= nchunks) { x.v[j] = gg[j]; continue; }
                const f32x4 gam = *(const f32x4*)(a.gamma + 4 * c), bet = *(const f32x4*)(a.beta + 4 * c);
                const f32x4 xh = (x.v[j] - mean) * rstd;
                const f32x4 k = keep_scale(mrow, c, a.inv_keep);
                f32x4 g;
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = xh[e] * gam[e] + bet[e] > 0.f ? d.v[j][e] * k[e] : 0.f;
                dg[j] += g * xh;
                db[j] += g;
                gg[j] = g * gam;
                x.v[j] = xh;
                const f32x4 t = gg[j] * xh;
                s1 += (gg[j][0] + gg[j][1]) + (gg[j][2] + gg[j][3]);
                s2 += (t[0] + t[1]) + (t[2] + t[3]);
            }
            s1 = wave_sum(s1) * inv_n;
            s2 = wave_sum(s2) * inv_n;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int c = lane + 64 * j;
                if (c >= nchunks) break;
                *(f32x4*)(orow + 4 * c) = (gg[j] - s1 - x.v[j] * s2) * rstd;
            }
        }
    }
    if constexpr (LN) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = lane + 64 * j;
            if (c >= nchunks) break;
            *(f32x4*)(lds + (wave * 2 + 0) * a.N + 4 * c) = dg[j];
            *(f32x4*)(lds + (wave * 2 + 1) * a.N + 4 * c) = db[j];
        }
        __syncthreads();
        // [2][N] values per workgroup, the waves in ascending order
        float* out_g = gridDim.x == 1 ? a.dgamma : (float*)a.work + (long)blockIdx.x * 2 * a.N;
        float* out_b = gridDim.x == 1 ? a.dbeta : out_g + a.N;
        for (int i = threadIdx.x; i < 2 * a.N; i += 256) {
            const int which = i >= a.N, col = i - which * a.N;
            float s = lds[which * a.N + col];
            for (int w = 1; w < 4; ++w) s += lds[(w * 2 + which) * a.N + col];
            (which ? out_b : out_g)[col] = s;
        }
    }
}

// dgamma | dbeta = the workgroups' partial sums in ascending workgroup order
__global__ __launch_bounds__(256) void ln_partials_kernel(const float* __restrict__ work, int nblocks, int N, float* dgamma, float* dbeta) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * N) return;
    float s = work[i];
    for (int b = 1; b < nblocks; ++b) s += work[(long)b * 2 * N + i];
    if (i < N) dgamma[i] = s; else dbeta[i - N] = s;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// A wave per row, a lane per class.  The divisor of the gradient, the batch's sum of w[y], is formed by EVERY workgroup from all M
// labels in one order (thread t the labels t, t + 256, ... in float64, a butterfly per wave, the four waves in order): the same bits
// everywhere, without a launch in front.
__global__ __launch_bounds__(256) void wce_mean_kernel(const mmvae_wce_args a) {
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float total = 0.f;
    if (a.g) {
        double s = 0.0;
        for (int i = threadIdx.x; i < a.M; i += 256) s += (double)ce_label(a.labels[i], a.C, a.class_weights).w;
        s = wave_sum_f64(s);
        if (lane == 0) wsum[wave] = s;
        __syncthreads();
        total = (float)(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
    }
    const int r_end = min(a.M, ((int)blockIdx.x + 1) * WCE_ROWS);
    double loss = 0.0, wtot = 0.0, nbad = 0.0;
    for (int row = blockIdx.x * WCE_ROWS + wave; row < r_end; row += 4) {
        const CeLabel lab = ce_label(a.labels[row], a.C, a.class_weights);
        const bool live = lane < a.C;
        const float x = live ? a.logits[(long)row * a.ld + lane] : -INFINITY;
        const float m = wave_max(x);
        int pred = wave_min_int(live && x == m ? lane : 64);           // the first maximum
        if (pred >= a.C) pred = 0;                                     // a row with NaN: no lane equals the maximum
        const float e = live ? ce_exp(x, m) : 0.f;
        const float se = wave_sum(e);
        const float xy = __shfl(x, lab.y, 64);
        const float nll = ce_term(1.f, m, se, xy);
        if (a.g && live) a.g[(long)row * a.ldg + lane] = ce_grad(lab.w, e, se, lane == lab.y) / total;
        if (lane == 0) {
            if (a.pred) a.pred[row] = pred;
            if (a.nll) a.nll[row] = nll;
            const bool ignored = a.labels[row] == -100;
            if (a.confusion && !lab.bad && !ignored) atomicAdd(&a.confusion[lab.y * a.C + pred], 1);
            loss += (double)lab.w * (double)nll;
            wtot += (double)lab.w;
            nbad += lab.bad ? 1.0 : 0.0;
        }
    }
    if (a.sums && lane == 0) {
        atomicAdd(&a.sums[0], loss);
        atomicAdd(&a.sums[1], wtot);
        if (nbad != 0.0) atomicAdd(&a.sums[2], nbad);
    }
}

static inline bool misaligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

template <bool LN>
static int launch_ln_fwd(const mmvae_ln_act_fwd_args& a, hipStream_t st) {
    const dim3 grid((a.M + LN_ROWS_FWD - 1) / LN_ROWS_FWD), block(256);
    if (a.N <= 256) hipLaunchKernelGGL((ln_act_fwd_kernel<LN, 1>), grid, block, 0, st, a);
    else if (a.N <= 512) hipLaunchKernelGGL((ln_act_fwd_kernel<LN, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((ln_act_fwd_kernel<LN, 4>), grid, block, 0, st, a);
    MM_CHECK_LAUNCH();
    return 0;
}

template <bool LN>
static int launch_ln_bwd(const mmvae_ln_act_bwd_args& a, int nblocks, hipStream_t st) {
    const dim3 grid(nblocks), block(256);
    const int lds = LN ? 4 * 2 * a.N * (int)sizeof(float) : 0;          // <= 32 KiB at MMVAE_LN_MAXN
    if (a.N <= 256) hipLaunchKernelGGL((ln_act_bwd_kernel<LN, 1>), grid, block, lds, st, a);
    else if (a.N <= 512) hipLaunchKernelGGL((ln_act_bwd_kernel<LN, 2>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((ln_act_bwd_kernel<LN, 4>), grid, block, lds, st, a);
    MM_CHECK_LAUNCH();
    return 0;
}

static bool ln_shape_ok(int M, int N) { return M >= 1 && N >= 4 && N <= MMVAE_LN_MAXN && N % 4 == 0; }

}  // namespace mm

using namespace mm;

extern "C" int mmvae_ln_act_fwd(const mmvae_ln_act_fwd_args* args, void* stream) {
    if (!args) return MMVAE_ERR_ARG;
    const mmvae_ln_act_fwd_args& a = *args;
    if (!ln_shape_ok(a.M, a.N) || !a.z || !a.y || a.ldz < a.N || a.ldy < a.N || a.ldz % 4 || a.ldy % 4) return MMVAE_ERR_ARG;
    if (misaligned(a.z, 16) || misaligned(a.y, 16)) return MMVAE_ERR_ARG;
    if (a.layer_norm && (!a.gamma || !a.beta || !a.mean || !a.rstd || misaligned(a.gamma, 16) || misaligned(a.beta, 16) ||
                         misaligned(a.mean, 4) || misaligned(a.rstd, 4) || !(a.eps > 0.f))) return MMVAE_ERR_ARG;
    if (a.mask && (a.ld_mask < a.N || a.ld_mask % 4 || misaligned(a.mask, 4) || !(a.inv_keep >= 1.f))) return MMVAE_ERR_ARG;
    return a.layer_norm ? launch_ln_fwd<true>(a, (hipStream_t)stream) : launch_ln_fwd<false>(a, (hipStream_t)stream);
}

extern "C" int mmvae_ln_act_bwd_work_bytes(int32_t M, int32_t N, int32_t layer_norm, int64_t* bytes) {
    if (!bytes || !ln_shape_ok(M, N)) return MMVAE_ERR_ARG;
    const int64_t nblocks = (M + LN_ROWS_BWD - 1) / LN_ROWS_BWD;
    *bytes = layer_norm && nblocks > 1 ? nblocks * 2 * N * (int64_t)sizeof(float) : 0;
    return 0;
}

extern "C" int mmvae_ln_act_bwd(const mmvae_ln_act_bwd_args* args, void* stream) {
    if (!args) return MMVAE_ERR_ARG;
    const mmvae_ln_act_bwd_args& a = *args;
    if (!ln_shape_ok(a.M, a.N) || !a.dy || !a.z || !a.dz || a.lddy < a.N || a.ldz < a.N || a.lddz < a.N || a.lddy % 4 || a.ldz % 4 || a.lddz % 4)
        return MMVAE_ERR_ARG;
    if (misaligned(a.dy, 16) || misaligned(a.z, 16) || misaligned(a.dz, 16)) return MMVAE_ERR_ARG;
    if (a.mask && (a.ld_mask < a.N || a.ld_mask % 4 || misaligned(a.mask, 4) || !(a.inv_keep >= 1.f))) return MMVAE_ERR_ARG;
    int64_t need = 0;
    mmvae_ln_act_bwd_work_bytes(a.M, a.N, a.layer_norm, &need);
    const int nblocks = (a.M + LN_ROWS_BWD - 1) / LN_ROWS_BWD;
    if (a.layer_norm) {
        if (!a.gamma || !a.beta || !a.mean || !a.rstd || !a.dgamma || !a.dbeta) return MMVAE_ERR_ARG;
        if (misaligned(a.gamma, 16) || misaligned(a.beta, 16) || misaligned(a.mean, 4) || misaligned(a.rstd, 4) || misaligned(a.dgamma, 4) ||
            misaligned(a.dbeta, 4)) return MMVAE_ERR_ARG;
        if (need > 0 && (!a.work || misaligned(a.work, 8) || a.work_bytes < need)) return MMVAE_ERR_ARG;
    }
    const int rc = a.layer_norm ? launch_ln_bwd<true>(a, nblocks, (hipStream_t)stream) : launch_ln_bwd<false>(a, nblocks, (hipStream_t)stream);
    if (rc || !a.layer_norm || nblocks == 1) return rc;
    hipLaunchKernelGGL(ln_partials_kernel, dim3((2 * a.N + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)a.work, nblocks, a.N,
                       a.dgamma, a.dbeta);
    MM_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmvae_wce_mean(const mmvae_wce_args* args, void* stream) {
    if (!args) return MMVAE_ERR_ARG;
    const mmvae_wce_args& a = *args;
    if (a.M < 1 || a.C < 2 || a.C > MMVAE_WCE_MAXC || !a.logits || !a.labels || a.ld < a.C) return MMVAE_ERR_ARG;
    if (a.g && a.ldg < a.C) return MMVAE_ERR_ARG;
    if (misaligned(a.logits, 4) || misaligned(a.labels, 8) || misaligned(a.class_weights, 4) || misaligned(a.sums, 8) || misaligned(a.g, 4) ||
        misaligned(a.pred, 4) || misaligned(a.nll, 4) || misaligned(a.confusion, 4)) return MMVAE_ERR_ARG;
    if (!a.sums && !a.g && !a.pred && !a.nll && !a.confusion) return MMVAE_ERR_ARG;              // nothing to compute
    hipLaunchKernelGGL(wce_mean_kernel, dim3((a.M + WCE_ROWS - 1) / WCE_ROWS), dim3(256), 0, (hipStream_t)stream, a);
    MM_CHECK_LAUNCH();
    return 0;
}
