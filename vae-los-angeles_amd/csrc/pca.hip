// The two passes of an exact PCA over the data (include/mmvae_hip.h): the centred scatter matrix S = (X - c)^T (X - c)
// (mmvae_pca_scatter) and the projection Y = (X - c) V^T onto k <= 64 components (mmvae_pca_project).  The F x F eigen-solve between
// them is the caller's (mmvae/pca.py: a library call).
//
// Scatter.  The rows are the GEMM's K dimension and BOTH operands are column tiles of the same row tile of X, so the lanes of every
// global load run along the contiguous feature axis and nothing is read transposed.  A workgroup (4 waves, 2 x 2, 64 x 64 each) owns
// one 128 x 128 tile of S on or above the diagonal (grid.x enumerates the T (T + 1) / 2 pairs ta <= tb, T = ceil(F / 128)) and walks
// its rows in chunks of PCA_BR = 32 with the row-tile pipeline (row_tile.h): the next chunk is loaded into registers (as wide as base and
// stride allow, pads never read) while the current one is multiplied out of the single LDS buffer.  The shift is subtracted in fp32
// when a chunk is staged; a row outside the matrix is staged as ZERO (not as -shift): it is a term of every sum.  LDS holds the chunk
// as it lies in memory, [row][feature]; the fragment of the exact-f32 MFMA wants, per lane, one feature (lane & 15) and the four rows
// 4 (lane >> 4) .. + 3: four ds_read_b32 whose 64 lanes hit 64 different banks (rt_frag_kmajor; PCA_LDF = 132: four rows are 16 banks apart).  A
// diagonal tile stages its one operand once, and its wave below the diagonal (wr = 1, wc = 0) multiplies nothing.
// Element (a, b), a <= b, of a tile is stored at S[a][b] AND S[b][a]; elements below the diagonal of a diagonal tile are dropped, so S
// is bitwise symmetric by construction.  Each element is ONE fmaf chain over the rows in ascending order (v_mfma_f32_16x16x4_f32 is an
// fmaf chain over its four k): no atomics, bit-identical runs.
// Split: grid.y workgroups per tile take consecutive runs of row chunks and write their whole partial tile to the workspace;
// pca_reduce_kernel adds the partial tiles in ascending split order and writes both triangles.
//
// Projection.  A workgroup owns PRJ_BM = 128 rows (a wave 32 of them) and walks F in chunks of RT_BK = 32 columns, staging the x chunk
// (shifted) and the chunk of all k <= 64 components in LDS: v does not fit whole (64 x 1 354 floats).  y[i][j] is one fmaf chain over
// the columns in ascending order: a function of row i's values, shift and v alone.
#include "common.h"
#include "row_tile.h"

namespace mm {

constexpr int PCA_BT = 128;                    // edge of a tile of S
constexpr int PCA_BR = RT_BK;                  // rows per chunk
constexpr int PCA_LDF = PCA_BT + 4;            // floats per LDS row: 16-byte aligned rows, 4 rows = 16 banks (rt_frag_kmajor)
constexpr int PCA_TARGET_WG = 2 * NUM_CU;      // workgroups resident at once (2 per CU at 148 VGPRs): the rows are split up to this many
constexpr int PCA_MAX_SPLITS = 64;
constexpr int PCA_MIN_CHUNKS = 8;              // an automatic split keeps at least this many chunks (256 rows): a split costs a 64 KiB tile
constexpr int PCA_MAX_F = PCA_BT * 32768;      // T (T + 1) / 2 is a grid dimension
constexpr int PRJ_BM = 128;                    // rows of a workgroup
static_assert(MMVAE_PCA_MAXK == 64, "pca_project_kernel: four 16-column accumulator tiles per wave");

struct PcaSP {
    const void* x; const float* shift;
    long ldx; int vec;
    int N, F, T, nsplit, cps;                  // T: tiles per edge; cps: row chunks per split
    long npairs;
    float* part;                               // [nsplit][npairs][128][128], NULL when nsplit == 1
    float* s; long lds;
};

// tile pair p -> (ta, tb), ta <= tb: row ta of the upper triangle holds T - ta pairs
__device__ __forceinline__ void pca_pair(int p, int T, int& ta, int& tb) {
    ta = 0;
    while (p >= T - ta) { p -= T - ta; ++ta; }
    tb = ta + p;
}

template <typename T>
__global__ __launch_bounds__(RT_THREADS) void pca_scatter_kernel(PcaSP a) {
    __shared__ __align__(16) float sA[PCA_BR * PCA_LDF];
    __shared__ __align__(16) float sB[PCA_BR * PCA_LDF];
    const int tid = threadIdx.x;
    const RtMap m(tid);
    int ta, tb;
    pca_pair((int)blockIdx.x, a.T, ta, tb);
    const bool diag = ta == tb;
    const bool active = !(diag && m.wr > m.wc);
    const int a0 = ta * PCA_BT, b0 = tb * PCA_BT;
    const int split = blockIdx.y;
    const long nchunks = ((long)a.N + PCA_BR - 1) / PCA_BR;
    const long ch_lo = (long)split * a.cps;
    const long ch_hi = ch_lo + a.cps < nchunks ? ch_lo + a.cps : nchunks;

    // The staging map is this kernel's own (a tile row is 128 columns, not 32): a thread stages columns 4 cq .. of rows rr, rr + 8, ..
    // of both operands, and a row outside the matrix as zero.
    const T* xb = (const T*)a.x;
    const int cq = tid & 31, rr = tid >> 5;
    const int ca = a0 + 4 * cq, cb = b0 + 4 * cq;
    float shA[4], shB[4];
    rt_shift4(a.shift, ca, a.F, shA);
    rt_shift4(a.shift, cb, a.F, shB);
    RtStage<T, 4, 8, PCA_LDF> rA, rB;                      // rB is neither loaded nor stored on a diagonal tile
    bool rok[4];
    auto issue = [&](long ch) {
        const T* row[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long r = ch * PCA_BR + rr + 8 * i;
            rok[i] = r < a.N;
            row[i] = xb + (rok[i] ? r : 0L) * a.ldx;
        }
        rA.issue(row, rok, ca, a.F, a.vec);
        if (!diag) rB.issue(row, rok, cb, a.F, a.vec);     // a diagonal tile stages its one operand once
    };

    f32x4 acc[4][4];
    zero_acc(acc);
    const float* sBr = diag ? sA : sB;
    if (ch_lo < ch_hi) issue(ch_lo);
    for (long ch = ch_lo; ch < ch_hi; ++ch) {
        __syncthreads();                                   // the previous chunk has been multiplied
        rA.store_zero_missing(sA, rr, cq, shA, rok);
        if (!diag) rB.store_zero_missing(sB, rr, cq, shB, rok);
        __syncthreads();
        if (ch + 1 < ch_hi) issue(ch + 1);
        if (active) {
            // the multiply stays written out here: handed to a function by reference, the accumulators of this kernel are kept in
            // VGPRs across the loop and the second resident workgroup is lost (193 + 64 registers against 148 + 64)
#pragma unroll
            for (int kk = 0; kk < PCA_BR / 16; ++kk) {
                f32x4 fa[4], fb[4];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) fa[mi] = rt_frag_kmajor<PCA_LDF>(sA, 16 * kk + 4 * m.lg, m.wr * 64 + 16 * mi + m.li);
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) fb[ni] = rt_frag_kmajor<PCA_LDF>(sBr, 16 * kk + 4 * m.lg, m.wc * 64 + 16 * ni + m.li);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) Mma<float>::mma(acc[mi][ni], fa[mi], fb[ni]);
            }
        }
    }
    // acc[mi][ni][r] = S[a0 + acc_row][b0 + acc_col]
    float* pt = a.part ? a.part + ((long)split * a.npairs + blockIdx.x) * (PCA_BT * PCA_BT) : nullptr;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m.acc_row(m.wr * 64, mi, r), col = m.acc_col(m.wc * 64, ni);
                const float v = acc[mi][ni][r];
                if (pt) pt[row * PCA_BT + col] = v;
                else {
                    const long ga = a0 + row, gb = b0 + col;
                    if (ga < a.F && gb < a.F && (!diag || col >= row)) {
                        a.s[ga * a.lds + gb] = v;
                        if (ga != gb) a.s[gb * a.lds + ga] = v;
                    }
                }
            }
}

// a thread per element of a tile: the splits' partial tiles are added in ascending split order, both triangles are written
__global__ __launch_bounds__(RT_THREADS) void pca_reduce_kernel(PcaSP a) {
    int ta, tb;
    pca_pair((int)blockIdx.x, a.T, ta, tb);
    const int e = blockIdx.y * RT_THREADS + threadIdx.x;
    const int row = e / PCA_BT, col = e - row * PCA_BT;
    const long ga = (long)ta * PCA_BT + row, gb = (long)tb * PCA_BT + col;
    if (ga >= a.F || gb >= a.F || (ta == tb && col < row)) return;
    const float* P = a.part + (long)blockIdx.x * (PCA_BT * PCA_BT) + e;
    const long stride = a.npairs * (PCA_BT * PCA_BT);
    float v = P[0];
    for (int s = 1; s < a.nsplit; ++s) v += P[s * stride];
    a.s[ga * a.lds + gb] = v;
    if (ga != gb) a.s[gb * a.lds + ga] = v;
}

struct PcaPP {
    const void* x; const float* shift; const float* v; float* y;
    long ldx, ldv, ldy; int vx, vv;
    int N, F, k;
};

// The projection is the pipeline's documented exception: it shares the thread map, the loads (rt_ld4) and the accumulator coordinates,
// but its issue, store and multiply steps are written in place, the issue step at both of its sites.  Handed to RtStage, rt_shift4,
// mma_chunk, a function or a lambda -- anything that takes the kernel's register arrays by reference -- this small latency-bound
// kernel compiles to other code and measured 1 to 10 % slower at k = 2 (profiles/row_tile_refactor_bench.json); as written here its
// machine code is the parent's up to the names and order of a few scalar instructions.  The components rv are fp32 rows, stored as they are.
template <typename T>
__global__ __launch_bounds__(RT_THREADS) void pca_project_kernel(PcaPP a) {
    __shared__ __align__(16) float sX[PRJ_BM * RT_LDR];
    __shared__ __align__(16) float sV[MMVAE_PCA_MAXK * RT_LDR];
    const RtMap m(threadIdx.x);
    const long q0 = (long)blockIdx.x * PRJ_BM;
    const int nr = (int)((long)a.N - q0 < PRJ_BM ? (long)a.N - q0 : PRJ_BM);
    const int nch = (a.F + RT_BK - 1) / RT_BK;
    const int nt = (a.k + 15) >> 4;                        // 16-column tiles of y

    const T* xb = (const T*)a.x;
    T rx[4][4];                                            // a thread stages columns 4 cq .. of x rows rb, rb + 32, .. and v rows rb, rb + 32
    float rv[2][4], sh[4];
    f32x4 acc[2][4];
    zero_acc(acc);
    {
        const int c0 = 0 * RT_BK + 4 * m.cq;
#pragma unroll
        for (int j = 0; j < 4; ++j) { sh[j] = 0.f; if (a.shift && c0 + j < a.F) sh[j] = a.shift[c0 + j]; }
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int r = m.rb + 32 * i; rt_ld4(xb + (r < nr ? q0 + r : 0L) * a.ldx, r < nr, c0, a.F, a.vx, rx[i]); }
#pragma unroll
        for (int i = 0; i < 2; ++i) { const int r = m.rb + 32 * i; rt_ld4(a.v + (r < a.k ? (long)r : 0L) * a.ldv, r < a.k, c0, a.F, a.vv, rv[i]); }
    }
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();                                   // the previous chunk has been multiplied
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 vx;
#pragma unroll
            for (int j = 0; j < 4; ++j) vx[j] = to_f32(rx[i][j]) - sh[j];
            *(f32x4*)(sX + (m.rb + 32 * i) * RT_LDR + 4 * m.cq) = vx;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) *(f32x4*)(sV + (m.rb + 32 * i) * RT_LDR + 4 * m.cq) = f32x4{rv[i][0], rv[i][1], rv[i][2], rv[i][3]};
        __syncthreads();
        if (ch + 1 < nch)                                  // the issue step again, for the next chunk
        {
            const int c0 = (ch + 1) * RT_BK + 4 * m.cq;
#pragma unroll
            for (int j = 0; j < 4; ++j) { sh[j] = 0.f; if (a.shift && c0 + j < a.F) sh[j] = a.shift[c0 + j]; }
#pragma unroll
            for (int i = 0; i < 4; ++i) { const int r = m.rb + 32 * i; rt_ld4(xb + (r < nr ? q0 + r : 0L) * a.ldx, r < nr, c0, a.F, a.vx, rx[i]); }
#pragma unroll
            for (int i = 0; i < 2; ++i) { const int r = m.rb + 32 * i; rt_ld4(a.v + (r < a.k ? (long)r : 0L) * a.ldv, r < a.k, c0, a.F, a.vv, rv[i]); }
        }
#pragma unroll
        for (int kk = 0; kk < RT_BK / 16; ++kk) {
            f32x4 fa[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) fa[mi] = *(const f32x4*)(sX + (m.wave * 32 + 16 * mi + m.li) * RT_LDR + 16 * kk + 4 * m.lg);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                if (ni < nt) {
                    const f32x4 fb = *(const f32x4*)(sV + (16 * ni + m.li) * RT_LDR + 16 * kk + 4 * m.lg);
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) Mma<float>::mma(acc[mi][ni], fa[mi], fb);
                }
            }
        }
    }
    // acc[mi][ni][r] = y[q0 + acc_row][acc_col]
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m.acc_row(m.wave * 32, mi, r), col = m.acc_col(0, ni);
                if (row < nr && col < a.k) a.y[(q0 + row) * a.ldy + col] = acc[mi][ni][r];
            }
}

static bool pca_sizes_ok(int N, int F) { return N >= 1 && F >= 1 && F <= PCA_MAX_F; }

static long pca_pairs(int F) {
    const long T = ((long)F + PCA_BT - 1) / PCA_BT;
    return T * (T + 1) / 2;
}

// the number of splits used and the row chunks per split: every split owns at least one chunk
static int pca_plan(int N, int F, int want_in, int* cps) {
    const long P = pca_pairs(F);
    const long nch = ((long)N + PCA_BR - 1) / PCA_BR;
    long want = want_in;
    if (want_in <= 0) {
        want = PCA_TARGET_WG / P;                          // rounded down: one resident round, no tail of a few workgroups
        const long most = nch / PCA_MIN_CHUNKS;
        if (want > most) want = most;
        if (want < 1) want = 1;
    }
    if (want > PCA_MAX_SPLITS) want = PCA_MAX_SPLITS;
    if (want > nch) want = nch;
    const long c = (nch + want - 1) / want;
    *cps = (int)c;
    return (int)((nch + c - 1) / c);
}

}  // namespace mm

extern "C" int mmvae_pca_scatter_splits(int32_t N, int32_t F, int32_t splits, int32_t* splits_used) {
    using namespace mm;
    if (!splits_used || !pca_sizes_ok(N, F) || splits < 0 || splits > PCA_MAX_SPLITS) return MMVAE_ERR_ARG;
    int cps;
    *splits_used = pca_plan(N, F, splits, &cps);
    return MMVAE_OK;
}

extern "C" int mmvae_pca_scatter_work_bytes(int32_t N, int32_t F, int32_t splits, int64_t* bytes) {
    using namespace mm;
    if (!bytes || !pca_sizes_ok(N, F) || splits < 0 || splits > PCA_MAX_SPLITS) return MMVAE_ERR_ARG;
    int cps;
    const int ns = pca_plan(N, F, splits, &cps);
    *bytes = ns > 1 ? 4L * PCA_BT * PCA_BT * pca_pairs(F) * ns : 0L;
    return MMVAE_OK;
}

extern "C" int mmvae_pca_scatter(const mmvae_pca_scatter_args* a, void* stream) {
    using namespace mm;
    if (!a || !a->x || !a->s) return MMVAE_ERR_ARG;
    if (!pca_sizes_ok(a->N, a->F) || a->splits < 0 || a->splits > PCA_MAX_SPLITS) return MMVAE_ERR_ARG;
    RtOperand ox;
    if (const int rc = rt_operand(a->x, a->x_dtype, a->ld_x, a->F, &ox)) return rc;
    if (a->ld_s < a->F || (uintptr_t)a->shift % 4 || (uintptr_t)a->s % 4 || (uintptr_t)a->work % 8) return MMVAE_ERR_ARG;
    int64_t need;
    if (mmvae_pca_scatter_work_bytes(a->N, a->F, a->splits, &need) != MMVAE_OK) return MMVAE_ERR_ARG;
    if (need > 0 && (!a->work || a->work_bytes < need)) return MMVAE_ERR_ARG;

    PcaSP p;
    p.x = a->x; p.shift = a->shift; p.ldx = a->ld_x; p.vec = ox.vec;
    p.N = a->N; p.F = a->F; p.T = (int)(((long)a->F + PCA_BT - 1) / PCA_BT);
    p.nsplit = pca_plan(a->N, a->F, a->splits, &p.cps);
    p.npairs = pca_pairs(a->F);
    p.part = p.nsplit > 1 ? (float*)a->work : nullptr;
    p.s = a->s; p.lds = a->ld_s;
    hipStream_t st = (hipStream_t)stream;

    const dim3 grid((unsigned)p.npairs, (unsigned)p.nsplit);
    if (a->x_dtype == MMVAE_F32) hipLaunchKernelGGL((pca_scatter_kernel<float>), grid, dim3(RT_THREADS), 0, st, p);
    else hipLaunchKernelGGL((pca_scatter_kernel<bf16>), grid, dim3(RT_THREADS), 0, st, p);
    MM_CHECK_LAUNCH();
    if (p.nsplit > 1) {
        hipLaunchKernelGGL(pca_reduce_kernel, dim3((unsigned)p.npairs, PCA_BT * PCA_BT / RT_THREADS), dim3(RT_THREADS), 0, st, p);
        MM_CHECK_LAUNCH();
    }
    return MMVAE_OK;
}

extern "C" int mmvae_pca_project(const mmvae_pca_project_args* a, void* stream) {
    using namespace mm;
    if (!a || !a->x || !a->v || !a->y) return MMVAE_ERR_ARG;
    if (a->N < 1 || a->F < 1 || a->k < 1 || a->k > MMVAE_PCA_MAXK) return MMVAE_ERR_ARG;
    RtOperand ox, ov;
    if (const int rc = rt_operand(a->x, a->x_dtype, a->ld_x, a->F, &ox)) return rc;
    if (rt_operand(a->v, MMVAE_F32, a->ld_v, a->F, &ov) || a->ld_y < a->k || (uintptr_t)a->shift % 4 || (uintptr_t)a->y % 4) return MMVAE_ERR_ARG;

    PcaPP p;
    p.x = a->x; p.shift = a->shift; p.v = a->v; p.y = a->y;
    p.ldx = a->ld_x; p.ldv = a->ld_v; p.ldy = a->ld_y;
    p.vx = ox.vec; p.vv = ov.vec;
    p.N = a->N; p.F = a->F; p.k = a->k;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(((long)a->N + PRJ_BM - 1) / PRJ_BM));
    if (a->x_dtype == MMVAE_F32) hipLaunchKernelGGL((pca_project_kernel<float>), grid, dim3(RT_THREADS), 0, st, p);
    else hipLaunchKernelGGL((pca_project_kernel<bf16>), grid, dim3(RT_THREADS), 0, st, p);
    MM_CHECK_LAUNCH();
    return MMVAE_OK;
}
