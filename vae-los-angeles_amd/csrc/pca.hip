// The two passes of an exact PCA over the data (include/mmvae_hip.h): the centred scatter matrix S = (X - c)^T (X - c)
// (mmvae_pca_scatter) and the projection Y = (X - c) V^T onto k <= 64 components (mmvae_pca_project).  The F x F eigen-solve between
// them is the caller's (mmvae/pca.py: a library call).
//
// Scatter.  The rows are the GEMM's K dimension and BOTH operands are column tiles of the same row tile of X, so the lanes of every
// global load run along the contiguous feature axis and nothing is read transposed.  A workgroup (4 waves, 2 x 2, 64 x 64 each) owns
// one 128 x 128 tile of S on or above the diagonal (grid.x enumerates the T (T + 1) / 2 pairs ta <= tb, T = ceil(F / 128)) and walks
// its rows in chunks of PCA_BR = 32 with knn.hip's pipeline: the next chunk is loaded into registers (row_tile.h: as wide as base and
// stride allow, pads never read) while the current one is multiplied out of the single LDS buffer.  The shift is subtracted in fp32
// when a chunk is staged; a row outside the matrix is staged as ZERO (not as -shift): it is a term of every sum.  LDS holds the chunk
// as it lies in memory, [row][feature]; the fragment of the exact-f32 MFMA wants, per lane, one feature (lane & 15) and the four rows
// 4 (lane >> 4) .. + 3: four ds_read_b32 whose 64 lanes hit 64 different banks (PCA_LDF = 132: four rows are 16 banks apart).  A
// diagonal tile stages its one operand once, and its wave below the diagonal (wr = 1, wc = 0) multiplies nothing.
// Element (a, b), a <= b, of a tile is stored at S[a][b] AND S[b][a]; elements below the diagonal of a diagonal tile are dropped, so S
// is bitwise symmetric by construction.  Each element is ONE fmaf chain over the rows in ascending order (v_mfma_f32_16x16x4_f32 is an
// fmaf chain over its four k): no atomics, bit-identical runs.
// Split: grid.y workgroups per tile take consecutive runs of row chunks and write their whole partial tile to the workspace;
// pca_reduce_kernel adds the partial tiles in ascending split order and writes both triangles.
//
// Projection.  A workgroup owns PRJ_BM = 128 rows (a wave 32 of them) and walks F in chunks of PRJ_BK = 32 columns, staging the x chunk
// (shifted) and the chunk of all k <= 64 components in LDS: v does not fit whole (64 x 1 354 floats).  y[i][j] is one fmaf chain over
// the columns in ascending order: a function of row i's values, shift and v alone.
#include "common.h"
#include "row_tile.h"

namespace mm {

constexpr int PCA_THREADS = 256;
constexpr int PCA_BT = 128;                    // edge of a tile of S
constexpr int PCA_BR = 32;                     // rows per chunk
constexpr int PCA_LDF = PCA_BT + 4;            // floats per LDS row: 16-byte aligned rows, 4 rows = 16 banks
constexpr int PCA_TARGET_WG = 2 * NUM_CU;      // workgroups resident at once (2 per CU at 148 VGPRs): the rows are split up to this many
constexpr int PCA_MAX_SPLITS = 64;
constexpr int PCA_MIN_CHUNKS = 8;              // an automatic split keeps at least this many chunks (256 rows): a split costs a 64 KiB tile
constexpr int PCA_MAX_F = PCA_BT * 32768;      // T (T + 1) / 2 is a grid dimension
constexpr int PRJ_BM = 128, PRJ_BK = 32;
constexpr int PRJ_LDR = PRJ_BK + 4;            // floats per LDS row: padded by one 16-byte chunk (as KNN_LDR)
static_assert(PCA_LDF % 4 == 0 && (4 * PCA_LDF) % 64 == 16, "pca_scatter_kernel: fragment reads are bank-conflict free");
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
__global__ __launch_bounds__(PCA_THREADS) void pca_scatter_kernel(PcaSP a) {
    __shared__ __align__(16) float sA[PCA_BR * PCA_LDF];
    __shared__ __align__(16) float sB[PCA_BR * PCA_LDF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4, wr = wave >> 1, wc = wave & 1;
    int ta, tb;
    pca_pair((int)blockIdx.x, a.T, ta, tb);
    const bool diag = ta == tb;
    const bool active = !(diag && wr > wc);
    const int a0 = ta * PCA_BT, b0 = tb * PCA_BT;
    const int split = blockIdx.y;
    const long nchunks = ((long)a.N + PCA_BR - 1) / PCA_BR;
    const long ch_lo = (long)split * a.cps;
    const long ch_hi = ch_lo + a.cps < nchunks ? ch_lo + a.cps : nchunks;

    const T* xb = (const T*)a.x;
    const int cq = tid & 31, rr = tid >> 5;                // a thread stages columns 4 cq .. of rows rr, rr + 8, .. of both operands
    const int ca = a0 + 4 * cq, cb = b0 + 4 * cq;
    float shA[4], shB[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        shA[j] = (a.shift && ca + j < a.F) ? a.shift[ca + j] : 0.f;
        shB[j] = (a.shift && cb + j < a.F) ? a.shift[cb + j] : 0.f;
    }
    T rA[4][4], rB[4][4];
    bool rok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) rB[i][j] = (T)0.f;     // a diagonal tile never loads its second operand
#define PCA_ISSUE(ch_) \
    { \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) { \
            const long r_ = (ch_) * PCA_BR + rr + 8 * i; \
            rok[i] = r_ < a.N; \
            const T* row_ = xb + (rok[i] ? r_ : 0L) * a.ldx; \
            knn_ld4(row_, rok[i], ca, a.F, a.vec, rA[i]); \
            if (!diag) knn_ld4(row_, rok[i], cb, a.F, a.vec, rB[i]); \
        } \
    }

    f32x4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    const float* sBr = diag ? sA : sB;
    if (ch_lo < ch_hi) PCA_ISSUE(ch_lo)
    for (long ch = ch_lo; ch < ch_hi; ++ch) {
        __syncthreads();                                   // the previous chunk has been multiplied
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 va, vb;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                va[j] = rok[i] ? to_f32(rA[i][j]) - shA[j] : 0.f;      // a row outside the matrix adds nothing
                vb[j] = rok[i] ? to_f32(rB[i][j]) - shB[j] : 0.f;
            }
            *(f32x4*)(sA + (rr + 8 * i) * PCA_LDF + 4 * cq) = va;
            if (!diag) *(f32x4*)(sB + (rr + 8 * i) * PCA_LDF + 4 * cq) = vb;
        }
        __syncthreads();
        if (ch + 1 < ch_hi) PCA_ISSUE(ch + 1)
        if (active) {
#pragma unroll
            for (int kk = 0; kk < PCA_BR / 16; ++kk) {
                f32x4 fa[4], fb[4];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int s = 0; s < 4; ++s) fa[mi][s] = sA[(16 * kk + 4 * lg + s) * PCA_LDF + wr * 64 + 16 * mi + li];
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int s = 0; s < 4; ++s) fb[ni][s] = sBr[(16 * kk + 4 * lg + s) * PCA_LDF + wc * 64 + 16 * ni + li];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) Mma<float>::mma(acc[mi][ni], fa[mi], fb[ni]);
            }
        }
    }
#undef PCA_ISSUE
    // acc[mi][ni][r] = S[a0 + row][b0 + col], row = wr*64 + 16 mi + 4 lg + r, col = wc*64 + 16 ni + li
    float* pt = a.part ? a.part + ((long)split * a.npairs + blockIdx.x) * (PCA_BT * PCA_BT) : nullptr;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr * 64 + 16 * mi + 4 * lg + r, col = wc * 64 + 16 * ni + li;
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
__global__ __launch_bounds__(PCA_THREADS) void pca_reduce_kernel(PcaSP a) {
    int ta, tb;
    pca_pair((int)blockIdx.x, a.T, ta, tb);
    const int e = blockIdx.y * PCA_THREADS + threadIdx.x;
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

template <typename T>
__global__ __launch_bounds__(PCA_THREADS) void pca_project_kernel(PcaPP a) {
    __shared__ __align__(16) float sX[PRJ_BM * PRJ_LDR];
    __shared__ __align__(16) float sV[MMVAE_PCA_MAXK * PRJ_LDR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const long q0 = (long)blockIdx.x * PRJ_BM;
    const int nr = (int)((long)a.N - q0 < PRJ_BM ? (long)a.N - q0 : PRJ_BM);
    const int nch = (a.F + PRJ_BK - 1) / PRJ_BK;
    const int nt = (a.k + 15) >> 4;                        // 16-column tiles of y

    const T* xb = (const T*)a.x;
    const int cq = tid & 7, rb = tid >> 3;                 // a thread stages columns 4 cq .. of x rows rb, rb + 32, .. and v rows rb, rb + 32
    T rx[4][4];
    float rv[2][4], sh[4];
#define PRJ_ISSUE(ch_) \
    { \
        const int c0_ = (ch_) * PRJ_BK + 4 * cq; \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) { sh[j] = 0.f; if (a.shift && c0_ + j < a.F) sh[j] = a.shift[c0_ + j]; } \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) { \
            const int r_ = rb + 32 * i; \
            knn_ld4(xb + (r_ < nr ? q0 + r_ : 0L) * a.ldx, r_ < nr, c0_, a.F, a.vx, rx[i]); \
        } \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) { \
            const int r_ = rb + 32 * i; \
            knn_ld4(a.v + (r_ < a.k ? (long)r_ : 0L) * a.ldv, r_ < a.k, c0_, a.F, a.vv, rv[i]); \
        } \
    }

    f32x4 acc[2][4];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    PRJ_ISSUE(0)
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();                                   // the previous chunk has been multiplied
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 vx;
#pragma unroll
            for (int j = 0; j < 4; ++j) vx[j] = to_f32(rx[i][j]) - sh[j];
            *(f32x4*)(sX + (rb + 32 * i) * PRJ_LDR + 4 * cq) = vx;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) *(f32x4*)(sV + (rb + 32 * i) * PRJ_LDR + 4 * cq) = f32x4{rv[i][0], rv[i][1], rv[i][2], rv[i][3]};
        __syncthreads();
        if (ch + 1 < nch) PRJ_ISSUE(ch + 1)
#pragma unroll
        for (int kk = 0; kk < PRJ_BK / 16; ++kk) {
            f32x4 fa[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) fa[mi] = *(const f32x4*)(sX + (wave * 32 + 16 * mi + li) * PRJ_LDR + 16 * kk + 4 * lg);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                if (ni < nt) {
                    const f32x4 fb = *(const f32x4*)(sV + (16 * ni + li) * PRJ_LDR + 16 * kk + 4 * lg);
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) Mma<float>::mma(acc[mi][ni], fa[mi], fb);
                }
            }
        }
    }
#undef PRJ_ISSUE
    // acc[mi][ni][r] = y[q0 + row][col], row = wave*32 + 16 mi + 4 lg + r, col = 16 ni + li
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wave * 32 + 16 * mi + 4 * lg + r, col = 16 * ni + li;
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
    if (a->x_dtype != MMVAE_F32 && a->x_dtype != MMVAE_BF16) return MMVAE_ERR_DTYPE;
    if (a->ld_x < a->F || a->ld_s < a->F) return MMVAE_ERR_ARG;
    const int es = a->x_dtype == MMVAE_BF16 ? 2 : 4;
    if ((uintptr_t)a->x % es || (uintptr_t)a->shift % 4 || (uintptr_t)a->s % 4 || (uintptr_t)a->work % 8) return MMVAE_ERR_ARG;
    int64_t need;
    if (mmvae_pca_scatter_work_bytes(a->N, a->F, a->splits, &need) != MMVAE_OK) return MMVAE_ERR_ARG;
    if (need > 0 && (!a->work || a->work_bytes < need)) return MMVAE_ERR_ARG;

    PcaSP p;
    p.x = a->x; p.shift = a->shift; p.ldx = a->ld_x; p.vec = knn_vec(a->x, a->ld_x, es);
    p.N = a->N; p.F = a->F; p.T = (int)(((long)a->F + PCA_BT - 1) / PCA_BT);
    p.nsplit = pca_plan(a->N, a->F, a->splits, &p.cps);
    p.npairs = pca_pairs(a->F);
    p.part = p.nsplit > 1 ? (float*)a->work : nullptr;
    p.s = a->s; p.lds = a->ld_s;
    hipStream_t st = (hipStream_t)stream;

    const dim3 grid((unsigned)p.npairs, (unsigned)p.nsplit);
    if (a->x_dtype == MMVAE_F32) hipLaunchKernelGGL((pca_scatter_kernel<float>), grid, dim3(PCA_THREADS), 0, st, p);
    else hipLaunchKernelGGL((pca_scatter_kernel<bf16>), grid, dim3(PCA_THREADS), 0, st, p);
    MM_CHECK_LAUNCH();
    if (p.nsplit > 1) {
        hipLaunchKernelGGL(pca_reduce_kernel, dim3((unsigned)p.npairs, PCA_BT * PCA_BT / PCA_THREADS), dim3(PCA_THREADS), 0, st, p);
        MM_CHECK_LAUNCH();
    }
    return MMVAE_OK;
}

extern "C" int mmvae_pca_project(const mmvae_pca_project_args* a, void* stream) {
    using namespace mm;
    if (!a || !a->x || !a->v || !a->y) return MMVAE_ERR_ARG;
    if (a->N < 1 || a->F < 1 || a->k < 1 || a->k > MMVAE_PCA_MAXK) return MMVAE_ERR_ARG;
    if (a->x_dtype != MMVAE_F32 && a->x_dtype != MMVAE_BF16) return MMVAE_ERR_DTYPE;
    if (a->ld_x < a->F || a->ld_v < a->F || a->ld_y < a->k) return MMVAE_ERR_ARG;
    const int es = a->x_dtype == MMVAE_BF16 ? 2 : 4;
    if ((uintptr_t)a->x % es || (uintptr_t)a->shift % 4 || (uintptr_t)a->v % 4 || (uintptr_t)a->y % 4) return MMVAE_ERR_ARG;

    PcaPP p;
    p.x = a->x; p.shift = a->shift; p.v = a->v; p.y = a->y;
    p.ldx = a->ld_x; p.ldv = a->ld_v; p.ldy = a->ld_y;
    p.vx = knn_vec(a->x, a->ld_x, es); p.vv = knn_vec(a->v, a->ld_v, 4);
    p.N = a->N; p.F = a->F; p.k = a->k;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(((long)a->N + PRJ_BM - 1) / PRJ_BM));
    if (a->x_dtype == MMVAE_F32) hipLaunchKernelGGL((pca_project_kernel<float>), grid, dim3(PCA_THREADS), 0, st, p);
    else hipLaunchKernelGGL((pca_project_kernel<bf16>), grid, dim3(PCA_THREADS), 0, st, p);
    MM_CHECK_LAUNCH();
    return MMVAE_OK;
}
