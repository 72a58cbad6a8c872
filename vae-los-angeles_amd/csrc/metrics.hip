// Imputation metrics of a reconstruction against its target in ONE streaming pass (mmvae_recon_metrics, include/mmvae_hip.h):
// per row the Pearson r and the cosine similarity, per column four f64 sums from which the host forms MAE / MSE / RMSE / R^2.
//
// Decomposition: a workgroup (4 waves) owns `rpb` consecutive rows and walks the columns in tiles of 256.  Inside a tile a lane owns
// 4 consecutive columns (one 16-byte load of fp32, one 8-byte load of bf16, where the alignment allows) and a wave takes every 4th
// row of the block, so
//   - the COLUMN partials of a tile live in the lane's registers (4 sums x 4 columns, f64) for all rows of the wave; the four waves
//     meet in LDS once per tile and the workgroup issues ONE f64 atomic per column and sum, contiguous over the tile
//     (4 / rpb of the streamed bytes);
//   - the eight ROW sums of a (row, tile) are reduced across the wave with a halving butterfly (10 exchanges instead of 48) and
//     added to the row's slot in LDS; a row is finalised by one thread after the last tile.
// Workgroups start at different tiles (blockIdx rotates the tile order) so that concurrent flushes hit different columns.
// Everything is accumulated in f64 from values loaded as fp32 / bf16.  Pearson uses the moments of the row SHIFTED by its own first
// element: raw moments of an ill-conditioned row (1000 +- 1e-3) lose 1e-4 of r even in f64.
#include "common.h"

namespace mm {

constexpr int MET_THREADS = 256;
constexpr int MET_V = 4;                    // columns per lane and tile: measured against 8 (twice the column registers, 2 waves per
                                            // SIMD instead of 4): 65 536 x 572 fp32 in 110 us against 141 us, bf16 rows 93 against 157
constexpr int MET_CT = WAVE * MET_V;        // columns per tile
constexpr int MET_MAXR = 128;               // most rows per workgroup (LDS row slots)
constexpr int MET_CS = 72;                  // padded lane stride of the LDS column partials (2-way conflicts on the flush)
constexpr int MET_TARGET_WG = 1024;         // workgroups asked for: one resident round at 4 per CU (2048 measured 10 % slower:
                                            // twice the atomics)

struct MetP {
    int M, N, rpb;
    const void* pred; long ldp; int vp;
    const void* tgt; long ldt; int vt;
    const float* shift; double* col; float* rp; float* rc;
};

// MET_V consecutive elements starting at a column that is a multiple of MET_V, with loads of `vec` elements (what base and ld allow)
__device__ __forceinline__ void met_load(const float* p, int vec, float (&o)[MET_V]) {
    if (vec == 4) {
#pragma unroll
        for (int j = 0; j < MET_V; j += 4) VLoad<float, 4>::ld(p + j, o + j);
    } else if (vec == 2) {
#pragma unroll
        for (int j = 0; j < MET_V; j += 2) VLoad<float, 2>::ld(p + j, o + j);
    } else {
#pragma unroll
        for (int j = 0; j < MET_V; ++j) o[j] = p[j];
    }
}
__device__ __forceinline__ void met_load(const bf16* p, int vec, float (&o)[MET_V]) {
    if (vec >= 4) {
#pragma unroll
        for (int j = 0; j < MET_V; j += 4) VLoad<bf16, 4>::ld(p + j, o + j);
    } else if (vec == 2) {
#pragma unroll
        for (int j = 0; j < MET_V; j += 2) VLoad<bf16, 2>::ld(p + j, o + j);
    } else {
#pragma unroll
        for (int j = 0; j < MET_V; ++j) o[j] = (float)p[j];
    }
}
// the scalar tail: the first nv (< MET_V) elements, nothing beyond them is read
template <typename T>
__device__ __forceinline__ void met_load_tail(const T* p, int nv, float (&o)[MET_V]) {
#pragma unroll
    for (int j = 0; j < MET_V; ++j) { o[j] = 0.f; if (j < nv) o[j] = to_f32(p[j]); }
}

__device__ __forceinline__ double met_shfl_xor(double v, int m) { return __shfl_xor(v, m, WAVE); }

// One element: s = {Sa, Sb, Saa, Sbb, Sab, Syp, Syy, Spp} of the row, c = the four column sums of this lane's column
__device__ __forceinline__ void met_elem(float yf, float pf, double y0, double p0, double cs, double (&s)[8], double& c0, double& c1,
                                         double& c2, double& c3, bool& ney, bool& nep) {
    const double y = (double)yf, p = (double)pf;
    const double a = y - y0, b = p - p0;
    ney |= (a != 0.0); nep |= (b != 0.0);
    s[0] += a; s[1] += b; s[2] += a * a; s[3] += b * b; s[4] += a * b;
    s[5] += y * p; s[6] += y * y; s[7] += p * p;
    const double t = y - cs, d = p - y;
    c0 += t; c1 += t * t; c2 += d * d; c3 += fabs(d);
}

// Halving butterfly over the wave: after the steps 32, 16, 8 every lane holds ONE of the eight sums, index (lane >> 3) & 7, and the
// steps 4, 2, 1 finish it: 10 exchanges instead of 48.  The total of sum k ends in s[0] of the lanes with (lane >> 3) & 7 == k.
__device__ __forceinline__ void met_reduce8(double (&s)[8], int lane) {
    {
        const bool h = lane & 32;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double send = h ? s[i] : s[i + 4], keep = h ? s[i + 4] : s[i]; s[i] = keep + met_shfl_xor(send, 32); }
    }
    {
        const bool h = lane & 16;
#pragma unroll
        for (int i = 0; i < 2; ++i) { const double send = h ? s[i] : s[i + 2], keep = h ? s[i + 2] : s[i]; s[i] = keep + met_shfl_xor(send, 16); }
    }
    {
        const bool h = lane & 8;
        const double send = h ? s[0] : s[1], keep = h ? s[1] : s[0];
        s[0] = keep + met_shfl_xor(send, 8);
    }
    s[0] += met_shfl_xor(s[0], 4);
    s[0] += met_shfl_xor(s[0], 2);
    s[0] += met_shfl_xor(s[0], 1);
}

template <typename TT, typename TP>
__global__ __launch_bounds__(MET_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void metrics_kernel(MetP a) {
    __shared__ double s_row[MET_MAXR][8];
    __shared__ int s_flag[MET_MAXR];
    __shared__ double s_col[4][MET_V][MET_CS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long r0 = (long)blockIdx.x * a.rpb;
    const int nr = (int)((long)a.M - r0 < a.rpb ? (long)a.M - r0 : a.rpb);
    for (int i = tid; i < MET_MAXR * 8; i += MET_THREADS) (&s_row[0][0])[i] = 0.0;
    for (int i = tid; i < MET_MAXR; i += MET_THREADS) s_flag[i] = 0;
    for (int i = tid; i < 4 * MET_V * MET_CS; i += MET_THREADS) (&s_col[0][0][0])[i] = 0.0;
    __syncthreads();

    const TT* tgt = (const TT*)a.tgt;
    const TP* pred = (const TP*)a.pred;
    const long ntiles = ((long)a.N + MET_CT - 1) / MET_CT;
    for (long tt = 0; tt < ntiles; ++tt) {
        const long t = (tt + blockIdx.x) % ntiles;
        const long c0 = t * MET_CT + lane * MET_V;
        const int nv = c0 >= a.N ? 0 : (a.N - c0 >= MET_V ? MET_V : (int)(a.N - c0));
        float cs[MET_V];
#pragma unroll
        for (int j = 0; j < MET_V; ++j) { cs[j] = 0.f; if (a.shift && j < nv) cs[j] = a.shift[c0 + j]; }
        double ca[4][MET_V];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < MET_V; ++j) ca[k][j] = 0.0;

        for (int r = wave; r < nr; r += 4) {                             // a wave takes every 4th row of the block
            const TT* yr = tgt + (r0 + r) * a.ldt;
            const TP* pr = pred + (r0 + r) * a.ldp;
            const double y0 = (double)to_f32(yr[0]), p0 = (double)to_f32(pr[0]);
            float y[MET_V], p[MET_V];
            double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            bool ney = false, nep = false;
            if (nv == MET_V) {
                met_load(yr + c0, a.vt, y); met_load(pr + c0, a.vp, p);
#pragma unroll
                for (int j = 0; j < MET_V; ++j) met_elem(y[j], p[j], y0, p0, (double)cs[j], s, ca[0][j], ca[1][j], ca[2][j], ca[3][j], ney, nep);
            } else if (nv > 0) {
                met_load_tail(yr + c0, nv, y); met_load_tail(pr + c0, nv, p);
#pragma unroll
                for (int j = 0; j < MET_V; ++j)
                    if (j < nv) met_elem(y[j], p[j], y0, p0, (double)cs[j], s, ca[0][j], ca[1][j], ca[2][j], ca[3][j], ney, nep);
            }
            met_reduce8(s, lane);
            const int fy = __any(ney) ? 1 : 0, fp = __any(nep) ? 2 : 0;
            if ((lane & 7) == 0) s_row[r][(lane >> 3) & 7] += s[0];         // only this wave touches row r's slots
            if (lane == 0) s_flag[r] |= fy | fp;
        }
        // the four waves' column partials meet in LDS; then one atomic per column and sum, contiguous over the tile
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < MET_V; ++j) atomicAdd(&s_col[k][j][lane], ca[k][j]);
        __syncthreads();
        for (int i = tid; i < 4 * MET_CT; i += MET_THREADS) {
            const int k = i / MET_CT, c = i % MET_CT;
            const double v = s_col[k][c % MET_V][c / MET_V];
            s_col[k][c % MET_V][c / MET_V] = 0.0;
            const long col = t * MET_CT + c;
            if (col < a.N && v != 0.0) unsafeAtomicAdd(a.col + (long)k * a.N + col, v);
        }
        __syncthreads();
    }

    if (tid < nr) {
        const double* s = s_row[tid];
        const double n = (double)a.N;
        const double cov = s[4] - s[0] * s[1] / n, vy = s[2] - s[0] * s[0] / n, vp = s[3] - s[1] * s[1] / n;
        double rr = cov / (sqrt(vy) * sqrt(vp));
        rr = rr > 1.0 ? 1.0 : (rr < -1.0 ? -1.0 : rr);                     // a NaN stays a NaN
        if (s_flag[tid] != 3) rr = __builtin_nan("");                      // a constant target or prediction row (scipy's rule)
        double ny = sqrt(s[6]), np = sqrt(s[7]);
        if (ny == 0.0) ny = 1.0;                                           // sklearn's normalize: a zero row gives 0
        if (np == 0.0) np = 1.0;
        a.rp[r0 + tid] = (float)rr;
        a.rc[r0 + tid] = (float)(s[5] / (ny * np));
    }
}

// elements per vector load (at most 16 bytes) that the base address and the leading dimension allow.  Not row_tile.h's rt_vec, which
// stops at 4 elements: bf16 rows may answer 8 here (met_load takes any answer >= 4 as 4).
static int met_vec(const void* p, long ld, int esize) {
    for (int v = 16 / esize; v > 1; v >>= 1)
        if (ld % v == 0 && ((uintptr_t)p % (uintptr_t)(v * esize)) == 0) return v;
    return 1;
}

}  // namespace mm

extern "C" int mmvae_recon_metrics(const mmvae_metrics_args* a, void* stream) {
    using namespace mm;
    if (!a || !a->pred || !a->target || !a->col_acc || !a->row_pearson || !a->row_cosine) return MMVAE_ERR_ARG;
    if (a->M < 1 || a->N < 1) return MMVAE_ERR_ARG;
    if ((a->pred_dtype != MMVAE_F32 && a->pred_dtype != MMVAE_BF16) || (a->target_dtype != MMVAE_F32 && a->target_dtype != MMVAE_BF16))
        return MMVAE_ERR_ARG;
    if (a->ld_target < a->N || (a->ld_pred != 0 && a->ld_pred < a->N)) return MMVAE_ERR_ARG;
    const int ep = a->pred_dtype == MMVAE_BF16 ? 2 : 4, et = a->target_dtype == MMVAE_BF16 ? 2 : 4;
    if ((uintptr_t)a->pred % ep || (uintptr_t)a->target % et) return MMVAE_ERR_ARG;
    if ((uintptr_t)a->col_shift % 4 || (uintptr_t)a->col_acc % 8 || (uintptr_t)a->row_pearson % 4 || (uintptr_t)a->row_cosine % 4)
        return MMVAE_ERR_ARG;
    MetP p;
    p.M = a->M; p.N = a->N;
    long rpb = ((long)a->M + MET_TARGET_WG - 1) / MET_TARGET_WG;
    rpb = (rpb + 3) & ~3L;
    p.rpb = (int)(rpb < 4 ? 4 : (rpb > MET_MAXR ? MET_MAXR : rpb));
    p.pred = a->pred; p.ldp = a->ld_pred; p.vp = met_vec(a->pred, a->ld_pred, ep);
    p.tgt = a->target; p.ldt = a->ld_target; p.vt = met_vec(a->target, a->ld_target, et);
    p.shift = a->col_shift; p.col = a->col_acc; p.rp = a->row_pearson; p.rc = a->row_cosine;
    const unsigned grid = (unsigned)(((long)a->M + p.rpb - 1) / p.rpb);
    hipStream_t st = (hipStream_t)stream;
    if (a->target_dtype == MMVAE_F32) {
        if (a->pred_dtype == MMVAE_F32) hipLaunchKernelGGL((metrics_kernel<float, float>), dim3(grid), dim3(MET_THREADS), 0, st, p);
        else hipLaunchKernelGGL((metrics_kernel<float, bf16>), dim3(grid), dim3(MET_THREADS), 0, st, p);
    } else {
        if (a->pred_dtype == MMVAE_F32) hipLaunchKernelGGL((metrics_kernel<bf16, float>), dim3(grid), dim3(MET_THREADS), 0, st, p);
        else hipLaunchKernelGGL((metrics_kernel<bf16, bf16>), dim3(grid), dim3(MET_THREADS), 0, st, p);
    }
    MM_CHECK_LAUNCH();
    return MMVAE_OK;
}
