// The fp32 row-tile pipeline of the evaluation kernels (knn.hip, silhouette.hip, pca.hip; DESIGN.md "The fp32 row-tile pipeline"): an
// exact-f32 MFMA GEMM over operand tiles of fp32 / bf16 row matrices, RT_BK = 32 columns at a time.  A kernel's loop is six steps --
//   issue (before the loop) | barrier, store, barrier, issue the next chunk, multiply
// -- built from the pieces below: the chunk of every operand is loaded into registers (RtStage::issue: four consecutive columns per
// thread and row, as wide as base and stride allow, pads never read) while the previous chunk is multiplied out of the ONE LDS buffer
// (mma_chunk); the shift is subtracted in fp32 when the chunk is stored to LDS (RtStage::store).  What "next" means (tile list, row
// chunk, column chunk) and the epilogue are the kernel's own.  Also here: the streaming squared norms (rt_norms_launch, row_tile.hip)
// and the host side the entry points share (operand validation, vector width, split count, dynamic-LDS launch).
#pragma once
#include "common.h"

namespace mm {

constexpr int RT_THREADS = 256;                // 4 waves, 2 x 2
constexpr int RT_BK = 32;                      // columns per chunk
constexpr int RT_LDR = RT_BK + 4;              // floats per LDS row: padded by one 16-byte chunk (wave_slab.h: stage_rows)

// A thread's places.  Staging: columns 4 cq .. 4 cq + 3 of the chunk, rows rb, rb + 32, ..  MFMA: wave (wr, wc) of the 2 x 2, lane
// (li, lg) of the 16 x 4 fragment.  Accumulator element acc[mi][ni][r] of a wave whose tile starts at (row0, col0) is
//   row = row0 + 16 mi + 4 lg + r,   col = col0 + 16 ni + li.
struct RtMap {
    int lane, wave, li, lg, wr, wc, cq, rb;
    __device__ __forceinline__ RtMap(int tid)
        : lane(tid & 63), wave(tid >> 6), li(lane & 15), lg(lane >> 4), wr(wave >> 1), wc(wave & 1), cq(tid & 7), rb(tid >> 3) {}
    __device__ __forceinline__ int acc_row(int row0, int mi, int r) const { return row0 + 16 * mi + 4 * lg + r; }
    __device__ __forceinline__ int acc_col(int col0, int ni) const { return col0 + 16 * ni + li; }
};

__device__ __forceinline__ void rt_vld(const float* p, int vec, float (&r)[4]) {
    if (vec >= 4) { const f32x4 v = *(const f32x4*)p; r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3]; }
    else if (vec == 2) { const f32x2 a = *(const f32x2*)p, b = *(const f32x2*)(p + 2); r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1]; }
    else { r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3]; }
}
__device__ __forceinline__ void rt_vld(const bf16* p, int vec, bf16 (&r)[4]) {
    if (vec >= 4) { const bf16x4 v = *(const bf16x4*)p; r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3]; }
    else if (vec == 2) { const bf16x2 a = *(const bf16x2*)p, b = *(const bf16x2*)(p + 2); r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1]; }
    else { r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3]; }
}
// columns c0 .. c0 + 3 (c0 a multiple of 4) of a row, as stored: zeros for a row outside the matrix and for columns >= F, which are
// not read
template <typename T>
__device__ __forceinline__ void rt_ld4(const T* row, bool rowok, int c0, int F, int vec, T (&r)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = (T)0.f;
    if (!rowok || c0 >= F) return;
    if (c0 + 4 <= F) rt_vld(row + c0, vec, r);
    else {
#pragma unroll
        for (int j = 0; j < 3; ++j) if (c0 + j < F) r[j] = row[c0 + j];
    }
}

// the shift of columns c0 .. c0 + 3: zero beyond F and without a shift
__device__ __forceinline__ void rt_shift4(const float* shift, int c0, int F, float (&sh)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { sh[j] = 0.f; if (shift && c0 + j < F) sh[j] = shift[c0 + j]; }
}

// One operand's chunk on its way to LDS: NI rows per thread, STEP rows apart, of an LDS buffer of LD floats per row.
template <typename T, int NI, int STEP, int LD>
struct RtStage {
    T r[NI][4];
    __device__ __forceinline__ void issue(const T* const (&row)[NI], const bool (&rowok)[NI], int c0, int F, int vec) {
#pragma unroll
        for (int i = 0; i < NI; ++i) rt_ld4(row[i], rowok[i], c0, F, vec, r[i]);
    }
    // a row outside the matrix is stored as 0 - shift
    __device__ __forceinline__ void store(float* s, int rb, int cq, const float (&sh)[4]) const { put<false>(s, rb, cq, sh, nullptr); }
    // .. as 0 (rowok as given to issue): where the rows are the reduction, a missing row is a term of every sum
    __device__ __forceinline__ void store_zero_missing(float* s, int rb, int cq, const float (&sh)[4], const bool (&rowok)[NI]) const {
        put<true>(s, rb, cq, sh, rowok);
    }

private:
    template <bool ZERO_MISSING>
    __device__ __forceinline__ void put(float* s, int rb, int cq, const float (&sh)[4], const bool* rowok) const {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (ZERO_MISSING && !rowok[i]) ? 0.f : to_f32(r[i][j]) - sh[j];
            *(f32x4*)(s + (rb + STEP * i) * LD + 4 * cq) = v;
        }
    }
};

template <int MI, int NI>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[MI][NI]) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc[mi][ni] += A rows rowA0 + 16 mi .. x B rows rowB0 + 16 ni .. over the chunk in sA, sB ([row][k], RT_LDR floats per row): every
// element one fmaf chain over k ascending.
template <int MI, int NI>
__device__ __forceinline__ void mma_chunk(f32x4 (&acc)[MI][NI], const float* sA, int rowA0, const float* sB, int rowB0, const RtMap& m) {
#pragma unroll
    for (int kk = 0; kk < RT_BK / 16; ++kk) {
        f32x4 fa[MI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) fa[mi] = *(const f32x4*)(sA + (rowA0 + 16 * mi + m.li) * RT_LDR + 16 * kk + 4 * m.lg);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const f32x4 fb = *(const f32x4*)(sB + (rowB0 + 16 * ni + m.li) * RT_LDR + 16 * kk + 4 * m.lg);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) Mma<float>::mma(acc[mi][ni], fa[mi], fb);
        }
    }
}

// The transposed sibling of mma_chunk's fragment read, for a chunk that lies [k][column] (LD floats per row, the rows are the
// reduction): a lane's fragment is one column and the four rows k0 .. k0 + 3, k0 = 16 kk + 4 lg -- four ds_read_b32 whose 64 lanes hit
// 64 different banks, because four rows are 16 banks apart.
template <int LD>
__device__ __forceinline__ f32x4 rt_frag_kmajor(const float* s, int k0, int col) {
    static_assert(LD % 4 == 0 && (4 * LD) % 64 == 16, "rt_frag_kmajor: fragment reads are bank-conflict free");
    return f32x4{s[k0 * LD + col], s[(k0 + 1) * LD + col], s[(k0 + 2) * LD + col], s[(k0 + 3) * LD + col]};
}

// the row of position p: order[p] clamped to [0, rows), or p itself without `order`
__device__ __forceinline__ long rt_row(const int* order, long p, int rows) {
    if (!order) return p;
    const long r = order[p];
    return r < 0 ? 0 : (r >= rows ? (long)rows - 1 : r);
}

// |x - c|^2 of the row of F elements at `base` (dt: MMVAE_F32 / MMVAE_BF16), by one wave: a lane sums every 64th column and the
// butterfly adds the lanes -- a function of the row's values alone; every lane returns the sum.
__device__ __forceinline__ float row_sqnorm(const char* base, int dt, int F, const float* shift, int lane) {
    float s = 0.f;
    for (int c = lane; c < F; c += WAVE) {
        const float x = (dt == MMVAE_BF16 ? (float)((const bf16*)base)[c] : ((const float*)base)[c]) - (shift ? shift[c] : 0.f);
        s += x * x;
    }
    return wave_sum(s);
}

// ---- host side ------------------------------------------------------------------------------
// `rows` rows of a row matrix, by position when `order` is given (rt_row)
struct RtRows { const void* base; long ld; int dt; int rows; const int* order; };

// out[p] = |row p - shift|^2 for the positions of s0, then of s1 (s1.rows may be 0), in ONE launch of a wave per row.  The kernel is
// defined once, in row_tile.hip.
int rt_norms_launch(const RtRows& s0, const RtRows& s1, int F, const float* shift, float* out, hipStream_t st);

// elements per vector load (at most 4) that the base address and the leading dimension allow
static inline int rt_vec(const void* p, long ld, int esize) {
    for (int v = 4; v > 1; v >>= 1)
        if (ld % v == 0 && ((uintptr_t)p % (uintptr_t)(v * esize)) == 0) return v;
    return 1;
}

// A row-matrix operand of F columns: MMVAE_ERR_DTYPE unless fp32 or bf16, MMVAE_ERR_ARG unless the base is aligned to an element and
// ld >= F; else MMVAE_OK with the element size and the vector width.
struct RtOperand { int esize, vec; };
static inline int rt_operand(const void* p, int dtype, long ld, int F, RtOperand* o) {
    if (dtype != MMVAE_F32 && dtype != MMVAE_BF16) return MMVAE_ERR_DTYPE;
    o->esize = dtype == MMVAE_BF16 ? 2 : 4;
    if (ld < F || (uintptr_t)p % o->esize) return MMVAE_ERR_ARG;
    o->vec = rt_vec(p, ld, o->esize);
    return MMVAE_OK;
}

// Workgroups per row block: the request, or as many as bring `nblocks` row blocks to `target` workgroups; at most `max_splits` and
// one per work item.
static inline long rt_splits(long nblocks, int request, int target, int max_splits, long items) {
    long want = request > 0 ? request : (nblocks >= target ? 1 : (target + nblocks - 1) / nblocks);
    if (want > max_splits) want = max_splits;
    return want > items ? items : want;
}

// Launch of a kernel whose dynamic LDS exceeds 64 KiB: the attribute is set once per kernel and process, to the most it ever needs.
template <auto KERNEL, int MAX_LDS, typename P>
static int rt_launch_dyn_lds(const P& p, dim3 grid, int lds, hipStream_t st) {
    static_assert(MAX_LDS > 64 * 1024 && MAX_LDS <= 160 * 1024, "rt_launch_dyn_lds: dynamic LDS");
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS);
        if (e != hipSuccess) return (int)e;
        attr_done = true;
    }
    hipLaunchKernelGGL(KERNEL, grid, dim3(RT_THREADS), lds, st, p);
    return (int)hipGetLastError();
}

}  // namespace mm
