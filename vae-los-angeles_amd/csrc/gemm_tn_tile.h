// The pieces every dW (TN) GEMM kernel shares (gemm_tn.hip: 128 x 128 tiles; gemm_tn_wide.hip: 256 x 288 and 128 x 448 tiles):
// the swizzled bf16 tile in LDS and its transposed fragment read, the mapping of a block to (output tile, batch split), and the
// epilogues (accumulator zero, column sums of P -> db, partial tile -> slab).  Everything is __device__ __forceinline__ or constexpr.
#pragma once
#include "common.h"

namespace mm {

// ---- bf16 tile geometry -----------------------------------------------------------------------
// A tile sits row-major in LDS, one batch row per `rowb` bytes (a multiple of 256).  Every 256-byte panel of a row (128 columns)
// has its eight 32-byte units XOR-ed with a key of the row, so that ds_read_b64_tr_b16 (the gfx950 transpose read: 16 lanes
// fetch 8 bytes each of 4 rows) meets no bank conflict.  The key does not change when a row moves by 4 or by 32.
__device__ __forceinline__ int tn_key(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }
// 16-byte chunk ch (0..15) of a panel of row r is stored at position tn_swz(r, ch) -- and, the map being an involution, the chunk
// whose position is pos is tn_swz(r, pos): what an LDS-DMA, whose destination is lane-linear, applies to its SOURCE address.
__device__ __forceinline__ int tn_swz(int r, int ch) { return (((ch >> 1) ^ tn_key(r)) << 1) | (ch & 1); }
// byte offset of 16-byte chunk ch (8 columns; any panel) of row r
__device__ __forceinline__ int tn_chunk_off(int r, int ch, int rowb) { return r * rowb + (ch >> 4) * 256 + (tn_swz(r, ch & 15) << 4); }
// Transposed MFMA operand of columns [colbase, colbase + 16) over the 32 rows from row0 (a multiple of 32) of `tile`: two
// transpose reads, after which a lane holds rows row0 + 8g .. row0 + 8g + 7 (g = lane >> 4) of column colbase + (lane & 15), the
// 8 reduction elements of one 16x16x32 MFMA.
__device__ __forceinline__ bf16x8 tn_frag_bf16(const unsigned char* tile, int rowb, int colbase, int lane, int row0 = 0) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int r = row0 + 8 * g + q;
    const int c32 = colbase >> 4;
    const int off0 = r * rowb + (c32 >> 3) * 256 + (((c32 & 7) ^ tn_key(r)) << 5) + (p << 3);
    const int off1 = off0 + 4 * rowb;               // rows +4: the key is unchanged
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + off0));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + off1));
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = lo; u.s.b = hi;
    return u.v;
}

// ---- block -> (output tile, batch split) ------------------------------------------------------
// Blocks are dealt to the XCDs round-robin, so split zz = 8 j + (L & 7) keeps ALL tiles of a batch split on one XCD: its rows of
// P and Q come from HBM once and are shared in that L2.  The grid is padded to whole groups of 8 splits; the blocks of the padding
// have no work (zz < 0).  linear (fewer than 8 splits, very wide outputs): tile-major, every XCD gets tiles.
struct TnBlock { int tile, zz; };
__device__ __forceinline__ TnBlock tn_block(int L, int ntiles, int nsplit, bool linear) {
    int tile, zz;
    if (linear) { tile = L % ntiles; zz = L / ntiles; }
    else { const int slot = L >> 3; tile = slot % ntiles; zz = (slot / ntiles) * 8 + (L & 7); }
    return {tile, zz < nsplit ? zz : -1};
}
constexpr int tn_grid(int nsplit, int ntiles, bool linear = false) { return (linear ? nsplit : (nsplit + 7) / 8 * 8) * ntiles; }

// ---- epilogues --------------------------------------------------------------------------------
// The MFMA operands are swapped (Q fragment as "A", P fragment as "B"), so accumulator (a, b) of a wave whose piece of the output
// starts at (n_w, k_w) holds, in lane (li = lane & 15, lg = lane >> 4), dW[n_w + 16 a + li][k_w + 16 b + 4 lg + j], j = 0..3:
// FOUR CONSECUTIVE k.  bsum[a] collects the lane's share of the column sum of P for column n_w + 16 a + li.
template <int A, int B>
__device__ __forceinline__ void tn_zero(f32x4 (&acc)[A][B], float (&bsum)[A]) {
#pragma unroll
    for (int a = 0; a < A; ++a) {
#pragma unroll
        for (int b = 0; b < B; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        bsum[a] = 0.f;
    }
}
// column sums of P straight from the P fragments of a step (VALU is idle under the MFMAs)
template <typename CT, int A>
__device__ __forceinline__ void tn_db_add(float (&bsum)[A], const typename Mma<CT>::frag (&pf)[A]) {
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
        for (int j = 0; j < Mma<CT>::EPC; ++j) bsum[a] += to_f32(pf[a][j]);
}
// db[n] += the sum over the four lane groups, by lanes 0..15
template <int A>
__device__ __forceinline__ void tn_db_store(const float (&bsum)[A], float* __restrict__ db, int n_w, int N, int lane) {
#pragma unroll
    for (int a = 0; a < A; ++a) {
        float v = bsum[a];
        v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
        const int n = n_w + a * 16 + lane;
        if (lane < 16 && n < N) unsafeAtomicAdd(db + n, v);
    }
}
// Split zz's partial tile -> slab[zz][N][K], stored plainly (tn_reduce_kernel sums the splits).  The widest store that K and the
// slab's alignment allow, both workgroup-uniform: 16 bytes (16 instead of 64 store instructions per lane: the scalar form cost
// 10-29 k cycles per workgroup, more than the 4 batch steps of a tiny-output GEMM), 8 bytes for an even K (782), else single floats.
template <int A, int B>
__device__ __forceinline__ void tn_store_slab(const f32x4 (&acc)[A][B], float* __restrict__ slab, int zz, int n_w, int k_w, int N, int K, int lane) {
    const uintptr_t al = (uintptr_t)slab;
    const bool v4 = (K & 3) == 0 && (al & 15) == 0, v2 = (K & 1) == 0 && (al & 7) == 0;
    float* sl = slab + (long)zz * N * K;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const int n = n_w + a * 16 + (lane & 15);
        if (n >= N) continue;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int k = k_w + b * 16 + (lane >> 4) * 4;
            if (k >= K) continue;
            float* sp = sl + (long)n * K + k;
            if (v4) *(f32x4*)sp = acc[a][b];                     // K % 4 == 0: k + 4 <= K
            else if (v2) {
                *(f32x2*)sp = f32x2{acc[a][b][0], acc[a][b][1]};
                if (k + 2 < K) *(f32x2*)(sp + 2) = f32x2{acc[a][b][2], acc[a][b][3]};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (k + j < K) sp[j] = acc[a][b][j];
            }
        }
    }
}

}  // namespace mm
