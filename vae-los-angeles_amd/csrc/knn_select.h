// The running top-k of the k-NN searches (knn.hip: knn_kernel, on the MFMA for the euclidean and on the VALU for the manhattan search):
// the order transform of a key, the insert into a row's sorted list, and the "tile complete -> threshold vote -> insert" block over a
// lane's 64 accumulator values for a search whose accumulator is its key.
#pragma once
#include "common.h"
#include "wave_slab.h"
#include "row_tile.h"

namespace mm {

constexpr int KNN_BM = 128, KNN_BN = 128;       // query rows of a workgroup, training rows of a tile
constexpr unsigned long long KNN_EMPTY = ~0ull;

// fp32 key -> unsigned with the same order; -0 = +0, every NaN one value above +inf
__device__ __forceinline__ unsigned knn_order(float key) {
    key += 0.f;
    unsigned b = __float_as_uint(key);
    if (key != key) b = 0x7FC00000u;
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float knn_key(unsigned u) { return __uint_as_float((u >> 31) ? (u ^ 0x80000000u) : ~u); }

// The 16 lanes of a row group (lane >> 4) insert their passing candidates into the group's list, one at a time; the wave's four groups
// in lock step.  L: this lane's group's list (k sorted entries).  S: positions per lane, 16 S >= k.  The kernels are instantiated for
// S = 4 (k <= 64: the code of every search before MMVAE_KNN_MAXK grew, instruction for instruction) and for S = KNN_SLOTS beyond; one
// kernel holding both inserts at its 64 call sites ran the k = 50 search a third slower.
template <int S>
__device__ __forceinline__ void knn_insert(unsigned long long* L, bool pass, unsigned long long cand, int lane, int k) {
    const int li = lane & 15, g0 = lane & 48;
    unsigned long long pend = __ballot(pass);
    while (pend) {
        const unsigned gm = (unsigned)(pend >> g0) & 0xFFFFu;
        const bool act = gm != 0;
        const int src = g0 + (act ? __ffs(gm) - 1 : 0);
        const unsigned long long c = __shfl(cand, src, WAVE);
        unsigned long long nv[S];
        bool wr[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int p = li + 16 * s;
            wr[s] = false;
            nv[s] = 0;
            if (act && p < k) {
                const unsigned long long e = L[p];
                const unsigned long long prev = p ? L[p - 1] : 0ull;
                wr[s] = e > c;
                nv[s] = prev > c ? prev : c;
            }
        }
        wave_lds_sync();                                   // every position is read before any is rewritten
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (wr[s]) L[li + 16 * s] = nv[s];
        wave_lds_sync();
        if (lane == src) pass = false;
        pend = __ballot(pass);
    }
}

// The tile is complete and the accumulator IS the key (the manhattan search): acc[mi][ni][r] belongs to query row
// acc_row(wr * 64, mi, r) of the block and training row j = tile * KNN_BN + acc_col(wc * 64, ni).  A key passes when it does not exceed
// the high word of the row's k-th entry; a wave-wide vote skips the insert when no lane passed.  The two waves that share query rows
// (wc = 0, 1) take turns, one workgroup barrier each.  sL: [KNN_BM][kp] lists.  The euclidean kernel carries the same block written out,
// with its key |t|^2 - 2 q.t in place of the accumulator (knn.hip says why).
// G (the grouped search): candidate j is admitted for a row iff (no same pair or ts[j] == the row's same code) and (no differ pair or
// td[j] != the row's differ code); a tile's candidate codes are loaded once, next to jlo.
// ts, td [Nt]: the candidates' codes in global memory, NULL for a pair that is not given; q_same, q_differ [KNN_BM]: the block's in LDS.
template <int S, bool G = false>
__device__ __forceinline__ void knn_select_tile(const f32x4 (&acc)[4][4], unsigned long long* sL, const RtMap& m, int tile, int Nt, int nr,
                                                int k, int kp, [[maybe_unused]] const int* ts = nullptr, [[maybe_unused]] const int* td = nullptr,
                                                [[maybe_unused]] const int* q_same = nullptr, [[maybe_unused]] const int* q_differ = nullptr) {
    for (int phase = 0; phase < 2; ++phase) {
        if (m.wc == phase) {
            bool jok[4];
            unsigned jlo[4];
            [[maybe_unused]] int tsv[4], tdv[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const long j = (long)tile * KNN_BN + m.acc_col(m.wc * 64, ni);
                jok[ni] = j < Nt;
                jlo[ni] = (unsigned)j;
                if constexpr (G) {
                    tsv[ni] = (ts && jok[ni]) ? ts[j] : 0;
                    tdv[ni] = (td && jok[ni]) ? td[j] : 0;
                }
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = m.acc_row(m.wr * 64, mi, r);
                    unsigned long long* L = sL + row * kp;
                    const unsigned thr = (unsigned)(L[k - 1] >> 32);
                    [[maybe_unused]] int qsv = 0, qdv = 0;
                    if constexpr (G) { qsv = q_same[row]; qdv = q_differ[row]; }
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        const unsigned u = knn_order(acc[mi][ni][r]);
                        bool pass = jok[ni] && row < nr && u <= thr;
                        if constexpr (G) pass = pass && (!ts || tsv[ni] == qsv) && (!td || tdv[ni] != qdv);
                        if (__any(pass)) knn_insert<S>(L, pass, ((unsigned long long)u << 32) | jlo[ni], m.lane, k);
                    }
                }
        }
        __syncthreads();
    }
}

}  // namespace mm
