// t-SNE in two dimensions with the exact all-pairs repulsion (mmvae_tsne_affinities, mmvae_tsne_gradient, mmvae_tsne_update,
// include/mmvae_hip.h): sklearn's method="barnes_hut" at angle = 0 -- the sparse P of the 3 x perplexity nearest neighbours, every pair
// in the repulsion -- with no tree.  fp32 throughout, no atomics, every sum in one fixed order.
//
// Affinities: a wave per row runs sklearn's _binary_search_perplexity on the row's k squared distances; the row's smallest distance is
// subtracted first (p and H do not change, the largest exponential is exp(0) = 1 and the row sum never underflows).
// Gradient, repulsion launch: a workgroup of 256 threads owns TS_BM = 512 rows, a lane TS_RPT = 2 of them in registers (rows tid and
// tid + 256 of the block: coalesced), and walks its split's columns j in tiles of TS_TJ = 1024 points staged in LDS; every lane of a
// wave reads the same y_j (a broadcast read, no bank conflict) and spends per pair 2 subtractions, 4 fused multiply-adds, a multiply, an
// add and one v_rcp_f32; the lane's two rows are the two halves of packed fp32 instructions (v_pk_fma_f32, v_pk_mul_f32, v_pk_add_f32:
// the same IEEE operation per half, so the same bits as the scalar form; measured 9 % faster).  Columns >= N are never walked (the loop ends at the split's last column), rows >= N are computed on zeros and
// never written, and the diagonal pair gets w = 0 in the tiles that can hold it (the other tiles run without the compare).
// Split: grid.y workgroups per row block take consecutive runs of 64-column chunks; each writes R_x, R_y, z_i per row and one sum of
// its z_i per workgroup (a lane's two rows, a butterfly over the wave, the four waves in order) to the workspace.
// Gradient, second launch: a workgroup first adds the workgroup sums of z in float64 (256 strided chains, then a fixed binary tree):
// every workgroup holds the same bits of Z.  Then a wave per row adds the row's partials in ascending split order, walks the row's CSR
// entries 64 at a time (attraction and error terms, any row length), reduces the lane sums by a fixed butterfly and writes the row.
// Update: sklearn's _gradient_descent step, an element per thread; the squared norm of the gained gradient is reduced per workgroup
// and a one-workgroup launch adds the workgroup sums in float64.
#include "common.h"

namespace mm {

constexpr int TS_THREADS = 256;
constexpr int TS_RPT = 2;                       // rows of a lane
constexpr int TS_BM = TS_THREADS * TS_RPT;      // rows of a workgroup
constexpr int TS_TJ = 1024;                     // columns of an LDS tile
constexpr int TS_JU = 64;                       // columns per chunk, the unit of the split
constexpr int TS_TARGET_WG = 8 * NUM_CU;        // below this many row blocks the columns are split
constexpr int TS_MAX_SPLITS = 64;
constexpr int TS_FIN_ROWS = 16;                 // rows of a workgroup of the second launch, 4 per wave
constexpr int TS_AFF_STEPS = 100;               // sklearn's n_steps
constexpr float TS_AFF_TOL = 1e-5f;             // sklearn's PERPLEXITY_TOLERANCE

// sum over the 64 lanes, in every one of them: after the step with distance d the values repeat with period d, so every lane adds the
// same pair and all hold one bit pattern
__device__ __forceinline__ float ts_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}
__device__ __forceinline__ float ts_wave_min(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d, WAVE));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// affinities
// ---------------------------------------------------------------------------------------------------------------------------------
struct TsAffP { const float* d; float* p; float* beta; long ldd, ldp; int N, k; float log_perp; };

__global__ __launch_bounds__(TS_THREADS) void tsne_affinities_kernel(TsAffP a) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (TS_THREADS / WAVE) + (threadIdx.x >> 6);
    if (row >= a.N) return;                                // whole waves leave: no barrier below
    const float* d = a.d + row * a.ldd;
    const int k = a.k;
    float dmin = INFINITY;
    for (int j = lane; j < k; j += WAVE) dmin = fminf(dmin, d[j]);
    dmin = ts_wave_min(dmin);
    float beta = 1.f, lo = -INFINITY, hi = INFINITY, beta_at = 1.f, s_at = 1.f;
    for (int step = 0; step < TS_AFF_STEPS; ++step) {      // every quantity below is wave-uniform: the branches do not diverge
        float s = 0.f, sd = 0.f;
        for (int j = lane; j < k; j += WAVE) {
            const float x = d[j] - dmin;
            const float e = expf(-x * beta);
            s += e;
            sd = fmaf(x, e, sd);
        }
        s = ts_wave_sum(s);
        sd = ts_wave_sum(sd);
        beta_at = beta; s_at = s;
        const float diff = (logf(s) + beta * (sd / s)) - a.log_perp;
        if (fabsf(diff) <= TS_AFF_TOL) break;
        if (diff > 0.f) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.f : (beta + hi) * 0.5f;
        } else {                                           // a NaN entropy comes here too: the search still ends after its 100 steps
            hi = beta;
            beta = lo == -INFINITY ? beta * 0.5f : (beta + lo) * 0.5f;
        }
    }
    float* p = a.p + row * a.ldp;
    for (int j = lane; j < k; j += WAVE) p[j] = expf(-(d[j] - dmin) * beta_at) / s_at;
    if (lane == 0) a.beta[row] = beta_at;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// gradient
// ---------------------------------------------------------------------------------------------------------------------------------
struct TsGradP {
    const float* y; const int* row_ptr; const int* col; const float* val;
    float* grad; float* z; float* err; float* zrow;
    float* part;                               // [nsplit][N][3]
    float* zpart;                              // [nsplit][nblocks]
    int N, nnz, nsplit, cps, nblocks;          // cps: 64-column chunks per split
    float exaggeration;
};

template <bool DIAG>
__device__ __forceinline__ void ts_tile(const float2* __restrict__ sY, int jn, long j0, const long (&row)[TS_RPT], const float (&xi)[TS_RPT],
                                        const float (&yi)[TS_RPT], float (&rx)[TS_RPT], float (&ry)[TS_RPT], float (&z)[TS_RPT]) {
    static_assert(TS_RPT == 2, "the packed form holds a lane's two rows in one register pair");
    const f32x2 X = {xi[0], xi[1]}, Yv = {yi[0], yi[1]}, one = {1.f, 1.f};
    f32x2 RX = {rx[0], rx[1]}, RY = {ry[0], ry[1]}, ZZ = {z[0], z[1]};
#pragma unroll 4
    for (int jj = 0; jj < jn; ++jj) {
        const float2 yj = sY[jj];
        const f32x2 dx = X - yj.x, dy = Yv - yj.y;
        const f32x2 q = __builtin_elementwise_fma(dy, dy, __builtin_elementwise_fma(dx, dx, one));
        f32x2 w = {__builtin_amdgcn_rcpf(q[0]), __builtin_amdgcn_rcpf(q[1])};
        if (DIAG) { w[0] = j0 + jj == row[0] ? 0.f : w[0]; w[1] = j0 + jj == row[1] ? 0.f : w[1]; }
        const f32x2 w2 = w * w;
        RX = __builtin_elementwise_fma(w2, dx, RX);
        RY = __builtin_elementwise_fma(w2, dy, RY);
        ZZ += w;
    }
    rx[0] = RX[0]; rx[1] = RX[1]; ry[0] = RY[0]; ry[1] = RY[1]; z[0] = ZZ[0]; z[1] = ZZ[1];
}

__global__ __launch_bounds__(TS_THREADS) void tsne_repulsion_kernel(TsGradP a) {
    __shared__ float2 sY[TS_TJ];
    __shared__ float sZ[TS_THREADS / WAVE];
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * TS_BM;
    const int split = blockIdx.y;
    const long jlo = (long)split * a.cps * TS_JU;
    const long jhi = jlo + (long)a.cps * TS_JU < a.N ? jlo + (long)a.cps * TS_JU : (long)a.N;
    const float2* __restrict__ Y = (const float2*)a.y;
    long row[TS_RPT];
    float xi[TS_RPT], yi[TS_RPT], rx[TS_RPT], ry[TS_RPT], z[TS_RPT];
#pragma unroll
    for (int r = 0; r < TS_RPT; ++r) {
        row[r] = r0 + tid + TS_THREADS * r;
        const float2 v = row[r] < a.N ? Y[row[r]] : make_float2(0.f, 0.f);
        xi[r] = v.x; yi[r] = v.y;
        rx[r] = ry[r] = z[r] = 0.f;
    }
    for (long j0 = jlo; j0 < jhi; j0 += TS_TJ) {
        const int jn = (int)(jhi - j0 < TS_TJ ? jhi - j0 : TS_TJ);
        __syncthreads();                                   // the previous tile has been walked
        for (int t = tid; t < jn; t += TS_THREADS) sY[t] = Y[j0 + t];
        __syncthreads();
        if (j0 < r0 + TS_BM && j0 + jn > r0) ts_tile<true>(sY, jn, j0, row, xi, yi, rx, ry, z);
        else ts_tile<false>(sY, jn, j0, row, xi, yi, rx, ry, z);
    }
    float zs = 0.f;
#pragma unroll
    for (int r = 0; r < TS_RPT; ++r) {
        if (row[r] < a.N) {
            float* P = a.part + ((long)split * a.N + row[r]) * 3;
            P[0] = rx[r]; P[1] = ry[r]; P[2] = z[r];
            zs += z[r];
        }
    }
    zs = ts_wave_sum(zs);
    if ((tid & 63) == 0) sZ[tid >> 6] = zs;
    __syncthreads();
    if (tid == 0) a.zpart[(long)split * a.nblocks + blockIdx.x] = ((sZ[0] + sZ[1]) + sZ[2]) + sZ[3];
}

__global__ __launch_bounds__(TS_THREADS) void tsne_finish_kernel(TsGradP a) {
    __shared__ double sD[TS_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const long n = (long)a.nsplit * a.nblocks;
        double v = 0.0;
        for (long t = tid; t < n; t += TS_THREADS) v += (double)a.zpart[t];
        sD[tid] = v;
        __syncthreads();
        for (int s = TS_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) sD[tid] += sD[tid + s];
            __syncthreads();
        }
    }
    const float Z = (float)sD[0];
    if (blockIdx.x == 0 && tid == 0) a.z[0] = Z;
    const float logZ = logf(Z);
    const float2* Y = (const float2*)a.y;
    constexpr int RPW = TS_FIN_ROWS / (TS_THREADS / WAVE);
    for (int t = 0; t < RPW; ++t) {
        const long i = (long)blockIdx.x * TS_FIN_ROWS + wave * RPW + t;
        if (i >= a.N) break;                               // wave-uniform
        float rx = 0.f, ry = 0.f, zr = 0.f;
        for (int s = 0; s < a.nsplit; ++s) {               // every lane the same addresses and the same sums
            const float* P = a.part + ((long)s * a.N + i) * 3;
            rx += P[0]; ry += P[1]; zr += P[2];
        }
        int e0 = a.row_ptr[i], e1 = a.row_ptr[i + 1];      // clamped: a bad row_ptr gives wrong numbers, no access out of range
        e0 = e0 < 0 ? 0 : (e0 > a.nnz ? a.nnz : e0);
        e1 = e1 < e0 ? e0 : (e1 > a.nnz ? a.nnz : e1);
        const float2 yi = Y[i];
        float ax = 0.f, ay = 0.f, kl = 0.f;
        for (int e = e0 + lane; e < e1; e += WAVE) {
            int j = a.col[e];
            j = j < 0 ? 0 : (j >= a.N ? a.N - 1 : j);
            const float p = a.val[e];
            const float2 yj = Y[j];
            const float dx = yi.x - yj.x, dy = yi.y - yj.y;
            const float q = fmaf(dy, dy, fmaf(dx, dx, 1.f));
            const float pw = p * __builtin_amdgcn_rcpf(q);
            ax = fmaf(pw, dx, ax);
            ay = fmaf(pw, dy, ay);
            if (a.err && p > 0.f) kl = fmaf(p, (logf(p) + logf(q)) + logZ, kl);     // p log(p / (w / Z)), w = 1 / q
        }
        ax = ts_wave_sum(ax);
        ay = ts_wave_sum(ay);
        if (a.err) kl = ts_wave_sum(kl);
        if (lane == 0) {
            a.grad[2 * i] = 4.f * (a.exaggeration * ax - rx / Z);
            a.grad[2 * i + 1] = 4.f * (a.exaggeration * ay - ry / Z);
            if (a.err) a.err[i] = kl;
            if (a.zrow) a.zrow[i] = zr;
        }
    }
}

static bool ts_grad_sizes_ok(int N, long nnz, int splits) { return N >= 2 && nnz >= 0 && nnz <= 2147483647L && splits >= 0 && splits <= TS_MAX_SPLITS; }

static void ts_plan(int N, int request, int* nsplit, int* cps, int* nblocks) {
    const long nb = ((long)N + TS_BM - 1) / TS_BM, chunks = ((long)N + TS_JU - 1) / TS_JU;
    long want = request > 0 ? request : (nb >= TS_TARGET_WG ? 1 : (TS_TARGET_WG + nb - 1) / nb);
    if (want > TS_MAX_SPLITS) want = TS_MAX_SPLITS;
    if (want > chunks) want = chunks;
    *cps = (int)((chunks + want - 1) / want);
    *nsplit = (int)((chunks + *cps - 1) / *cps);
    *nblocks = (int)nb;
}

static long ts_part_bytes(int N, int nsplit) { return (12L * N * nsplit + 7) & ~7L; }

// ---------------------------------------------------------------------------------------------------------------------------------
// update
// ---------------------------------------------------------------------------------------------------------------------------------
struct TsUpdP { float* y; float* update; float* gains; const float* grad; float* gnorm; float* part; long n; int nblocks; float momentum, lr; };

__global__ __launch_bounds__(TS_THREADS) void tsne_update_kernel(TsUpdP a) {
    __shared__ float sG[TS_THREADS / WAVE];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * TS_THREADS + tid;
    float gg = 0.f;
    if (i < a.n) {
        const float g = a.grad[i], u = a.update[i];
        float gain = u * g < 0.f ? a.gains[i] + 0.2f : a.gains[i] * 0.8f;
        gain = fmaxf(gain, 0.01f);
        gg = g * gain;
        const float un = fmaf(a.momentum, u, -(a.lr * gg));
        a.gains[i] = gain;
        a.update[i] = un;
        a.y[i] += un;
    }
    if (!a.gnorm) return;
    float s = ts_wave_sum(gg * gg);
    if ((tid & 63) == 0) sG[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) a.part[blockIdx.x] = ((sG[0] + sG[1]) + sG[2]) + sG[3];
}

__global__ __launch_bounds__(TS_THREADS) void tsne_norm_kernel(TsUpdP a) {
    __shared__ double sD[TS_THREADS];
    const int tid = threadIdx.x;
    double v = 0.0;
    for (int t = tid; t < a.nblocks; t += TS_THREADS) v += (double)a.part[t];
    sD[tid] = v;
    __syncthreads();
    for (int s = TS_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) sD[tid] += sD[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.gnorm[0] = (float)sqrt(sD[0]);
}

static long ts_update_blocks(int N) { return (2L * N + TS_THREADS - 1) / TS_THREADS; }

}  // namespace mm

extern "C" int mmvae_tsne_affinities(const mmvae_tsne_affinities_args* a, void* stream) {
    using namespace mm;
    if (!a || !a->dist2 || !a->p || !a->beta) return MMVAE_ERR_ARG;
    if (a->N < 1 || a->k < 1 || !(a->perplexity > 0.f) || !(a->perplexity < (float)a->k)) return MMVAE_ERR_ARG;
    if (a->ld_dist2 < a->k || a->ld_p < a->k) return MMVAE_ERR_ARG;
    if ((uintptr_t)a->dist2 % 4 || (uintptr_t)a->p % 4 || (uintptr_t)a->beta % 4) return MMVAE_ERR_ARG;
    TsAffP p;
    p.d = a->dist2; p.p = a->p; p.beta = a->beta; p.ldd = a->ld_dist2; p.ldp = a->ld_p; p.N = a->N; p.k = a->k;
    p.log_perp = logf(a->perplexity);
    constexpr int RPB = TS_THREADS / WAVE;
    hipLaunchKernelGGL(tsne_affinities_kernel, dim3((unsigned)(((long)a->N + RPB - 1) / RPB)), dim3(TS_THREADS), 0, (hipStream_t)stream, p);
    MM_CHECK_LAUNCH();
    return MMVAE_OK;
}

extern "C" int mmvae_tsne_gradient_splits(int32_t N, int32_t splits, int32_t* splits_used) {
    using namespace mm;
    if (!splits_used || !ts_grad_sizes_ok(N, 0, splits)) return MMVAE_ERR_ARG;
    int ns, cps, nb;
    ts_plan(N, splits, &ns, &cps, &nb);
    *splits_used = ns;
    return MMVAE_OK;
}

extern "C" int mmvae_tsne_gradient_work_bytes(int32_t N, int32_t splits, int64_t* bytes) {
    using namespace mm;
    if (!bytes || !ts_grad_sizes_ok(N, 0, splits)) return MMVAE_ERR_ARG;
    int ns, cps, nb;
    ts_plan(N, splits, &ns, &cps, &nb);
    *bytes = ts_part_bytes(N, ns) + ((4L * ns * nb + 7) & ~7L);
    return MMVAE_OK;
}

extern "C" int mmvae_tsne_gradient(const mmvae_tsne_gradient_args* a, void* stream) {
    using namespace mm;
    if (!a || !a->y || !a->row_ptr || !a->grad || !a->z || !a->work) return MMVAE_ERR_ARG;
    if (!ts_grad_sizes_ok(a->N, a->nnz, a->splits) || (a->nnz > 0 && (!a->col || !a->val))) return MMVAE_ERR_ARG;
    if ((uintptr_t)a->y % 8 || (uintptr_t)a->row_ptr % 4 || (uintptr_t)a->col % 4 || (uintptr_t)a->val % 4 || (uintptr_t)a->grad % 4 ||
        (uintptr_t)a->z % 4 || (uintptr_t)a->err % 4 || (uintptr_t)a->z_row % 4 || (uintptr_t)a->work % 8)
        return MMVAE_ERR_ARG;
    int64_t need;
    if (mmvae_tsne_gradient_work_bytes(a->N, a->splits, &need) != MMVAE_OK || a->work_bytes < need) return MMVAE_ERR_ARG;
    TsGradP p;
    p.y = a->y; p.row_ptr = a->row_ptr; p.col = a->col; p.val = a->val;
    p.grad = a->grad; p.z = a->z; p.err = a->err; p.zrow = a->z_row;
    p.N = a->N; p.nnz = (int)a->nnz; p.exaggeration = a->exaggeration;
    ts_plan(a->N, a->splits, &p.nsplit, &p.cps, &p.nblocks);
    p.part = (float*)a->work;
    p.zpart = (float*)((char*)a->work + ts_part_bytes(a->N, p.nsplit));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tsne_repulsion_kernel, dim3((unsigned)p.nblocks, (unsigned)p.nsplit), dim3(TS_THREADS), 0, st, p);
    MM_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsne_finish_kernel, dim3((unsigned)(((long)a->N + TS_FIN_ROWS - 1) / TS_FIN_ROWS)), dim3(TS_THREADS), 0, st, p);
    MM_CHECK_LAUNCH();
    return MMVAE_OK;
}

extern "C" int mmvae_tsne_update_work_bytes(int32_t N, int64_t* bytes) {
    using namespace mm;
    if (!bytes || N < 1) return MMVAE_ERR_ARG;
    *bytes = (4L * ts_update_blocks(N) + 7) & ~7L;
    return MMVAE_OK;
}

extern "C" int mmvae_tsne_update(const mmvae_tsne_update_args* a, void* stream) {
    using namespace mm;
    if (!a || !a->y || !a->update || !a->gains || !a->grad || a->N < 1) return MMVAE_ERR_ARG;
    if ((uintptr_t)a->y % 4 || (uintptr_t)a->update % 4 || (uintptr_t)a->gains % 4 || (uintptr_t)a->grad % 4 || (uintptr_t)a->grad_norm % 4 ||
        (uintptr_t)a->work % 8)
        return MMVAE_ERR_ARG;
    int64_t need;
    mmvae_tsne_update_work_bytes(a->N, &need);
    if (a->grad_norm && (!a->work || a->work_bytes < need)) return MMVAE_ERR_ARG;
    TsUpdP p;
    p.y = a->y; p.update = a->update; p.gains = a->gains; p.grad = a->grad; p.gnorm = a->grad_norm; p.part = (float*)a->work;
    p.n = 2L * a->N; p.nblocks = (int)ts_update_blocks(a->N); p.momentum = a->momentum; p.lr = a->learning_rate;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)p.nblocks), dim3(TS_THREADS), 0, st, p);
    MM_CHECK_LAUNCH();
    if (p.gnorm) {
        hipLaunchKernelGGL(tsne_norm_kernel, dim3(1), dim3(TS_THREADS), 0, st, p);
        MM_CHECK_LAUNCH();
    }
    return MMVAE_OK;
}
