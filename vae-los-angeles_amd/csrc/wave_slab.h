// What the kernels whose waves carry 16-row slabs through MFMAs with SWAPPED operands (W fragment as "A", activation fragment as "B":
// lane (li = lane & 15, lg = lane >> 4) holds row li and columns 4 lg .. of a 16 x 16 tile) share -- the tile epilogues (gemm_nt_epi.h,
// gemm_ntp.h) and the fused per-CU kernels (latent.hip, class_tail.hip): the W-row order that gives a lane 8 consecutive 2-byte columns
// with its whole-line store, the wave-level LDS hand-off, padded-row weight staging and the grid of one persistent workgroup per CU.
#pragma once
#include "common.h"

namespace mm {

// the wave's LDS writes are visible to its other lanes (LDS operations of a wave execute in order)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }

// Column order of a wave's 64 output columns inside its 4 MFMA n-tiles.
template <bool PAIR> struct EpiCols {
    static constexpr int G = PAIR ? 8 : 4;            // consecutive columns a lane owns per group
    static constexpr int NG = 16 / G;                 // groups per lane (x 4 rows m)
    // W row (relative to the wave's 64) that goes to LDS row x = 16*n + i of the wave's W block: tiles (2g, 2g+1) interleaved
    static constexpr __host__ __device__ __forceinline__ int wrow(int x) {
        if constexpr (!PAIR) return x;
        const int n = x >> 4, i = x & 15;
        return 32 * (n >> 1) + 8 * (i >> 2) + 4 * (n & 1) + (i & 3);
    }
    // first column (relative to the wave's 64) of group g for lane group lg; element e of the group is accumulator
    // (n, j) = (PAIR ? 2g + (e >> 2) : g, e & 3)
    static constexpr __host__ __device__ __forceinline__ int base(int g, int lg) { return PAIR ? 32 * g + 8 * lg : 16 * g + 4 * lg; }
    static constexpr __host__ __device__ __forceinline__ int tile(int g, int e) { return PAIR ? 2 * g + (e >> 2) : g; }
};
// wrow (what is staged) and base / tile (what is stored) are right only as a pair -- a lane's G accumulators of a group are G consecutive
// columns -- and a mismatch gives plausible numbers in the wrong columns: it does not compile
template <typename EC> constexpr bool epi_cols_agree() {
    for (int g = 0; g < EC::NG; ++g)
        for (int lg = 0; lg < 4; ++lg)
            for (int e = 0; e < EC::G; ++e)
                if (EC::wrow(16 * EC::tile(g, e) + 4 * lg + (e & 3)) != EC::base(g, lg) + e) return false;
    return true;
}
static_assert(epi_cols_agree<EpiCols<true>>() && epi_cols_agree<EpiCols<false>>(), "EpiCols: staged W-row order and stored column order disagree");

// Whole-line stores of a 16 x 64 block of 2-byte outputs.  A lane packs its two groups (columns 8 lg .. and 32 + 8 lg .. of row li) into
// pk[0] and pk[1]: two 64-byte halves of different lines.  Lanes li < 8 (lowl) give away their second half and get row li + 8's first
// half, lanes li >= 8 the other way round (row_ror:8 == lane li ^ 8: one DPP move, no ds_bpermute round trip): st0 is 16 bytes of row
// li & 7 and st1 of row (li & 7) + 8, both at column line_col(li, lg) -- 8 lanes x 16 bytes = one FULL line per row and instruction (halves
// from separate instructions: +55 % HBM write traffic, gemm_nt_epi.h).  The caller guarantees 128-byte aligned rows and a block whose
// 64 columns exist, and guards the two rows.
constexpr __host__ __device__ __forceinline__ int line_col(int li, int lg) { return EpiCols<true>::base(li >> 3, lg); }
// on a row pointer, one term at a time: as ONE index the terms merge into one register and the schedule around every address differs
template <typename T> __device__ __forceinline__ T* line_col(T* row, int li, int lg) { return row + line_col(li, 0) + line_col(0, lg); }
// Declares st0 / st1 (uint32_t[4]) from pk (uint32_t[2][4]) and the caller's lowl = li < 8.  A macro, and the predicate formed where the lane's
// other constants are: inlined from a function, gemm_ntp_kernel's epilogues grew by 13-38 instructions (another order, s_nop before the DPPs)
#define SWAP_HALVES(pk, lowl, st0, st1) \
    uint32_t st0[4], st1[4]; \
    _Pragma("unroll") \
    for (int q_ = 0; q_ < 4; ++q_) { \
        const uint32_t got_ = (uint32_t)__builtin_amdgcn_mov_dpp((int)((lowl) ? (pk)[1][q_] : (pk)[0][q_]), 0x128, 0xf, 0xf, true); \
        st0[q_] = (lowl) ? (pk)[0][q_] : got_; \
        st1[q_] = (lowl) ? got_ : (pk)[1][q_]; \
    }

// Weight staging by NT threads: LDS row r < nrows takes the first `chunks` 16-byte chunks of global row map(r) (rows ld elements apart; map:
// EpiCols<>::wrow).  LDS rows lie row_bytes apart, padded by one 16-byte chunk: the 16 lanes of a fragment read hit 16 different bank groups.
template <int NT, typename Map>
__device__ __forceinline__ void stage_rows(unsigned char* lds, int row_bytes, const bf16* g, long ld, int nrows, int chunks, int tid, Map map) {
    for (int c = tid; c < nrows * chunks; c += NT) {
        const int r = c / chunks, ch = c - r * chunks;
        *(uint4*)(lds + r * row_bytes + ch * 16) = *(const uint4*)(g + (long)map(r) * ld + ch * 8);
    }
}

// one persistent workgroup of `waves` waves per CU, or fewer when there are fewer than NUM_CU * waves slabs (a wave owns whole slabs)
inline int persistent_grid(int nslabs, int waves) { const int g = (nslabs + waves - 1) / waves; return g < NUM_CU ? g : NUM_CU; }

}  // namespace mm
