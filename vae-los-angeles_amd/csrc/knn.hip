// Brute-force k nearest neighbours as a GEMM whose epilogue is a running top-k (mmvae_knn_search, include/mmvae_hip.h), and the uniform
// k-NN regression that follows it (mmvae_knn_mean_rows).
//
// Decomposition: a workgroup (4 waves, 2 x 2, 64 x 64 each) owns KNN_BM = 128 query rows and walks its training rows in tiles of
// KNN_BN = 128.  A tile's 128 x 128 dot products (q_i - c).(t_j - c) are accumulated over F in chunks of RT_BK = 32 columns on the
// exact-f32 MFMA with the row-tile pipeline (row_tile.h): the chunk of both operands is loaded into registers (as wide as base and
// stride allow, widened and shifted in fp32) while the previous chunk is multiplied out of LDS, so one LDS buffer is enough.  At 32 cycles per
// v_mfma_f32_16x16x4_f32 a chunk costs a wave 128 MFMAs = 4096 cycles against 16 ds_read_b128 and 8 global loads per lane, and the
// selection below runs once per F / 4 * 16 MFMAs: LDS and selection are far from the bound.  Operand delivery is not (measured,
// 0.26 of the fp32 MFMA rate from fp32 rows, 0.42 from bf16 rows): every workgroup re-reads its query block per tile.
// Selection: a row's k best live in LDS as ONE sorted list of 64-bit entries (ordered key << 32 | j), so the order (key, j) is one
// unsigned compare and an empty slot is the largest entry.  After a tile a lane holds 64 keys; the compare path is one fp32 FMA, the
// order transform and a compare against the high word of the row's k-th entry, and a wave-wide vote skips the rest when no lane
// passed (after the first tiles: nearly always).  The insert path takes the 16 lanes that share a query row in the MFMA layout: they
// insert one candidate at a time, each lane rewriting the list positions li, li + 16, .. < k (new[p] = old[p] <= c ? old[p] :
// max(old[p-1], c)), the four row groups of the wave in lock step.  The two waves that share query rows take turns (one barrier each).
// Nothing in it depends on the order in which candidates arrive, so the result is a function of the keys alone.
// Split: grid.y workgroups per query block take consecutive runs of tiles; their lists go to the workspace and knn_merge_kernel ranks
// every entry among all lists of its row (own position + binary searches in the others): fixed order, no atomics.
// The squared norms |q_i - c|^2, |t_j - c|^2 come from one streaming launch (rt_norms_launch: a wave per row) into the workspace.
// The manhattan search (mmvae_knn_search_l1) is the same kernel with another inner loop (L1 = true): l1_chunk accumulates |q - t| on
// the VALU in the accumulator layout of the MFMA, one fp32 chain per pair in ascending column order; no norms, no shift.  The
// selection (knn_select.h) is shared.  mmvae_knn_weighted_rows is the inverse-distance sibling of mmvae_knn_mean_rows.
// The grouped search (mmvae_knn_search_grouped, G = true) is the same kernel again with an admission predicate on int32 codes in `pass`
// (same code / other code), the query codes of the block staged in LDS behind the lists, and a tile skip: knn_tile_codes_kernel writes
// the min and max of both candidate codes per tile, a workgroup reduces the same over its query rows and walks only the tiles that can
// hold an admitted pair.  Lists can then be short: the final store and the merge write idx -1 / distance +inf behind the entries.
#include <type_traits>
#include "common.h"
#include "wave_slab.h"
#include "row_tile.h"
#include "knn_select.h"

namespace mm {

constexpr int KNN_TILE_BYTES = (KNN_BM + KNN_BN) * RT_LDR * 4;
constexpr int knn_max_lds(int slots) { return KNN_TILE_BYTES + KNN_BM * 16 * slots * 8; }   // operand tile + 128 lists of 16 slots entries
constexpr int KNN_TARGET_WG = 4 * NUM_CU;      // below this many query blocks the training rows are split
constexpr int KNN_MAX_SPLITS = 64;
constexpr int KNN_SLOTS = MMVAE_KNN_MAXK / 16;  // list positions a lane of a row group rewrites at most
static_assert(MMVAE_KNN_MAXK % 16 == 0 && KNN_SLOTS * 16 == MMVAE_KNN_MAXK, "knn_insert: 16 lanes x KNN_SLOTS positions");
static_assert(knn_max_lds(KNN_SLOTS) <= 160 * 1024, "knn_kernel: operand tile + 128 lists of MMVAE_KNN_MAXK entries in one workgroup's LDS");

struct KnnP {
    const void* q; const void* t; const float* shift;
    long ldq, ldt; int vq, vt;
    int Mq, Nt, F, k, kp;                      // kp: k rounded up to 16, the stride of a row's list
    int nsplit, tps;                           // tiles per split
    const float* qn; const float* tn;
    unsigned long long* part;                  // [Mq][nsplit][k], NULL when nsplit == 1
    int* idx; long ldi; float* dist2; long ldd;
};
// The grouped search's arguments (G): codes of the queries [Mq] and candidates [Nt], a pair NULL when not given; tmm [ntiles][4]: min, max
// of t_same and min, max of t_differ over the tile's rows.  The ungrouped kernels keep taking KnnP: they are what they were, byte for byte.
struct KnnGP : KnnP {
    const int* qs; const int* ts; const int* qd; const int* td; const int* tmm;
};
template <bool G> using KnnArgsT = std::conditional_t<G, KnnGP, KnnP>;

constexpr int KNN_CODE_BYTES = 2 * KNN_BM * 4;  // G: the block's query codes, [2][KNN_BM] behind the lists
static_assert(knn_max_lds(KNN_SLOTS) + KNN_CODE_BYTES <= 160 * 1024, "knn_kernel<G>: the staged query codes fit beside the tile and the lists");

// The manhattan search's sibling of mma_chunk: acc[mi][ni][r] += sum over the chunk's columns of |q_row[c] - t_col[c]|, every element ONE
// chain of plain fp32 adds in ascending column order (a subtract, then an add whose source takes the abs modifier), a lane owning the
// 64 (row, column) pairs it owns in the MFMA accumulator layout so that the selection applies unchanged.  Per 4 columns a lane reads
// 16 q fragments (4 addresses per wave: broadcasts) and 4 t fragments (16 rows, 36 floats apart: conflict free) for 512 VALU operations.
__device__ __forceinline__ void l1_chunk(f32x4 (&acc)[4][4], const float* sQ, int row0, const float* sT, int col0, const RtMap& m) {
#pragma unroll 2
    for (int g = 0; g < RT_BK / 4; ++g) {
        f32x4 ft[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) ft[ni] = *(const f32x4*)(sT + (col0 + 16 * ni + m.li) * RT_LDR + 4 * g);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 fq = *(const f32x4*)(sQ + (row0 + 16 * mi + 4 * m.lg + r) * RT_LDR + 4 * g);
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[mi][ni][r] += __builtin_fabsf(fq[j] - ft[ni][j]);
            }
    }
}

// L1 = false: the euclidean search (keys from the MFMA dot products and the training norms).  L1 = true: the manhattan search
// (mmvae_knn_search_l1): the same pipeline, lists, split and merge; the accumulator is the key and the distance.
// what dist2 receives for a list entry: key + |q_i - c|^2 clamped at 0, or (L1) the key, which is the distance
template <bool L1>
__device__ __forceinline__ float knn_dist(unsigned long long e, const float* qn, long row) {
    const float key = knn_key((unsigned)(e >> 32));
    if constexpr (L1) return key;
    else { const float d = key + qn[row]; return d < 0.f ? 0.f : d; }
}

// may tile `t` hold a pair the predicate admits?  q*: min / max of the block's query codes.  Conservative: false only when no pair can.
__device__ __forceinline__ bool knn_tile_active(const KnnGP& a, int t, int qs_min, int qs_max, int qd_min, int qd_max) {
    const int* c = a.tmm + 4 * (long)t;
    if (a.qs && (c[1] < qs_min || c[0] > qs_max)) return false;
    if (a.qd && c[2] == c[3] && qd_min == qd_max && c[2] == qd_min) return false;
    return true;
}

// the first tile >= t of the range that is active, or tile_hi
__device__ __forceinline__ int knn_next_active(const KnnGP& a, int t, int tile_hi, int qs_min, int qs_max, int qd_min, int qd_max) {
    while (t < tile_hi && !knn_tile_active(a, t, qs_min, qs_max, qd_min, qd_max)) ++t;
    return t;
}

template <typename TQ, typename TT, int S, bool L1, bool G = false>
__global__ __launch_bounds__(RT_THREADS) void knn_kernel(KnnArgsT<G> a) {
    extern __shared__ __align__(16) unsigned char knn_smem[];
    float* sQ = (float*)knn_smem;                          // [KNN_BM][RT_LDR]
    float* sT = sQ + KNN_BM * RT_LDR;                      // [KNN_BN][RT_LDR]
    unsigned long long* sL = (unsigned long long*)(knn_smem + KNN_TILE_BYTES);   // [KNN_BM][kp]
    const int tid = threadIdx.x;
    const RtMap m(tid);
    const int lane = m.lane, wc = m.wc;
    const long q0 = (long)blockIdx.x * KNN_BM;
    const int nr = (int)((long)a.Mq - q0 < KNN_BM ? (long)a.Mq - q0 : KNN_BM);
    const int split = blockIdx.y;
    const int ntiles = (a.Nt + KNN_BN - 1) / KNN_BN;
    const int tile_lo = split * a.tps;
    const int tile_hi = tile_lo + a.tps < ntiles ? tile_lo + a.tps : ntiles;
    const int nch = (a.F + RT_BK - 1) / RT_BK;
    const int k = a.k, kp = a.kp;
    for (int i = tid; i < KNN_BM * kp; i += RT_THREADS) sL[i] = KNN_EMPTY;
    // G: the block's query codes in LDS, their min / max over rows < nr (the same in every thread), and the walk over the active tiles
    [[maybe_unused]] int* sC = (int*)(sL + KNN_BM * kp);   // [2][KNN_BM]: same codes, differ codes
    [[maybe_unused]] int qs_min = 0, qs_max = 0, qd_min = 0, qd_max = 0;
    if constexpr (G) {
        if (tid < KNN_BM) {
            sC[tid] = (a.qs && tid < nr) ? a.qs[q0 + tid] : 0;
            sC[KNN_BM + tid] = (a.qd && tid < nr) ? a.qd[q0 + tid] : 0;
        }
        __syncthreads();
        qs_min = qs_max = sC[0]; qd_min = qd_max = sC[KNN_BM];
        for (int r = 1; r < nr; ++r) {
            const int cs = sC[r], cd = sC[KNN_BM + r];
            qs_min = cs < qs_min ? cs : qs_min; qs_max = cs > qs_max ? cs : qs_max;
            qd_min = cd < qd_min ? cd : qd_min; qd_max = cd > qd_max ? cd : qd_max;
        }
    }

    const TQ* qb = (const TQ*)a.q;
    const TT* tb = (const TT*)a.t;
    RtStage<TQ, 4, 32, RT_LDR> rq;
    RtStage<TT, 4, 32, RT_LDR> rt;
    float sh[4];
    auto issue = [&](int tile, int ch) {
        const int c0 = ch * RT_BK + 4 * m.cq;
        const TQ* qrow[4];
        const TT* trow[4];
        bool qok[4], tok[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = m.rb + 32 * i;
            const long j = (long)tile * KNN_BN + r;
            qrow[i] = qb + (q0 + r) * a.ldq; qok[i] = r < nr;
            trow[i] = tb + j * a.ldt; tok[i] = j < a.Nt;
        }
        rt_shift4(a.shift, c0, a.F, sh);
        rq.issue(qrow, qok, c0, a.F, a.vq);
        rt.issue(trow, tok, c0, a.F, a.vt);
    };

    f32x4 acc[4][4];
    zero_acc(acc);
    int nwalk = tile_hi - tile_lo;
    if constexpr (G) {
        nwalk = 0;
        for (int t = tile_lo; t < tile_hi; ++t) nwalk += knn_tile_active(a, t, qs_min, qs_max, qd_min, qd_max) ? 1 : 0;
    }
    const int nsteps = nwalk * nch;
    int tile = tile_lo, ch = 0;
    if constexpr (G) tile = knn_next_active(a, tile_lo, tile_hi, qs_min, qs_max, qd_min, qd_max);
    if (nsteps > 0) issue(tile, ch);
    for (int s = 0; s < nsteps; ++s) {
        __syncthreads();                                   // the previous chunk has been multiplied (first step: the lists are initialised)
        rq.store(sQ, m.rb, m.cq, sh);
        rt.store(sT, m.rb, m.cq, sh);
        __syncthreads();
        int ntile = tile, nchk = ch + 1;
        if (nchk == nch) {
            nchk = 0;
            if constexpr (G) ntile = knn_next_active(a, ntile + 1, tile_hi, qs_min, qs_max, qd_min, qd_max);   // the same tile in every thread; the prefetch follows it
            else ++ntile;
        }
        if (s + 1 < nsteps) issue(ntile, nchk);
        if constexpr (L1) l1_chunk(acc, sQ, m.wr * 64, sT, wc * 64, m);
        else mma_chunk(acc, sQ, m.wr * 64, sT, wc * 64, m);
        if (nchk == 0) {
            // the tile is complete: acc[mi][ni][r] = (q_row - c).(t_j - c) or |q_row - t_j|_1, row = acc_row, j = tile*128 + acc_col
            // The euclidean kernel keeps the selection written out here, as it always was: calling the shared knn_select_tile instead
            // compiled to 15 more integer multiplies per tile and measured 0.15 - 0.18 % slower, outside the spread of repeats.
            if constexpr (L1) {
                if constexpr (G) knn_select_tile<S, true>(acc, sL, m, tile, a.Nt, nr, k, kp, a.ts, a.td, sC, sC + KNN_BM);
                else knn_select_tile<S>(acc, sL, m, tile, a.Nt, nr, k, kp);
            } else {
                for (int phase = 0; phase < 2; ++phase) {
                    if (wc == phase) {
                        float tnv[4];
                        bool jok[4];
                        unsigned jlo[4];
                        [[maybe_unused]] int tsv[4], tdv[4];
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni) {
                            const long j = (long)tile * KNN_BN + m.acc_col(wc * 64, ni);
                            jok[ni] = j < a.Nt;
                            jlo[ni] = (unsigned)j;
                            tnv[ni] = jok[ni] ? a.tn[j] : 0.f;
                            if constexpr (G) {
                                tsv[ni] = (a.ts && jok[ni]) ? a.ts[j] : 0;
                                tdv[ni] = (a.td && jok[ni]) ? a.td[j] : 0;
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
                                if constexpr (G) { qsv = sC[row]; qdv = sC[KNN_BM + row]; }
#pragma unroll
                                for (int ni = 0; ni < 4; ++ni) {
                                    const unsigned u = knn_order(tnv[ni] - 2.f * acc[mi][ni][r]);
                                    bool pass = jok[ni] && row < nr && u <= thr;
                                    if constexpr (G) pass = pass && (!a.ts || tsv[ni] == qsv) && (!a.td || tdv[ni] != qdv);
                                    if (__any(pass)) knn_insert<S>(L, pass, ((unsigned long long)u << 32) | jlo[ni], lane, k);
                                }
                            }
                    }
                    __syncthreads();
                }
            }
            zero_acc(acc);
        }
        tile = ntile; ch = nchk;
    }
    __syncthreads();
    for (int i = tid; i < nr * k; i += RT_THREADS) {
        const int row = i / k, n = i - row * k;
        const unsigned long long e = sL[row * kp + n];
        if (a.part) a.part[((q0 + row) * a.nsplit + split) * k + n] = e;
        else {
            a.idx[(q0 + row) * a.ldi + n] = (int)(unsigned)e;     // an empty slot (G: a short list): -1
            if (a.dist2) {
                float d = knn_dist<L1>(e, a.qn, q0 + row);
                if constexpr (G) { if (e == KNN_EMPTY) d = __builtin_inff(); }
                a.dist2[(q0 + row) * a.ldd + n] = d;
            }
        }
    }
}

// One wave per query row: the rank of an entry among all lists of the row is its own position plus its lower bounds in the others
// (the entries of a row are distinct: every j is in one split).  Empty slots (a split with fewer than k rows) rank last and are skipped.
// G: the lists of a row can hold fewer than k entries in all; the positions behind them get idx -1 / distance +inf.
template <bool L1, bool G = false>
__global__ __launch_bounds__(WAVE) void knn_merge_kernel(KnnP a) {
    const long row = blockIdx.x;
    const int k = a.k, ns = a.nsplit;
    const unsigned long long* P = a.part + row * ns * k;
    [[maybe_unused]] int filled = 0;
    for (int t = threadIdx.x; t < ns * k; t += WAVE) {
        const unsigned long long v = P[t];
        if (v == KNN_EMPTY) continue;
        if constexpr (G) ++filled;
        const int s = t / k;
        int rank = t - s * k;
        for (int s2 = 0; s2 < ns && rank < k; ++s2) {
            if (s2 == s) continue;
            const unsigned long long* P2 = P + s2 * k;
            int lo = 0, hi = k;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (P2[mid] < v) lo = mid + 1; else hi = mid; }
            rank += lo;
        }
        if (rank < k) {
            a.idx[row * a.ldi + rank] = (int)(unsigned)v;
            if (a.dist2) a.dist2[row * a.ldd + rank] = knn_dist<L1>(v, a.qn, row);
        }
    }
    if constexpr (G) {
        for (int o = WAVE / 2; o > 0; o >>= 1) filled += __shfl_xor(filled, o, WAVE);
        for (int n = filled + threadIdx.x; n < k; n += WAVE) {
            a.idx[row * a.ldi + n] = -1;
            if (a.dist2) a.dist2[row * a.ldd + n] = __builtin_inff();
        }
    }
}

// tmm[tile][4] = min, max of ts and min, max of td over the rows < Nt of the tile (zeros for a pair that is not given): one wave per tile
__global__ __launch_bounds__(WAVE) void knn_tile_codes_kernel(const int* ts, const int* td, int Nt, int* tmm) {
    const long tile = blockIdx.x;
    int v[4] = {2147483647, -2147483647 - 1, 2147483647, -2147483647 - 1};
    for (int r = threadIdx.x; r < KNN_BN; r += WAVE) {
        const long j = tile * KNN_BN + r;
        if (j >= Nt) continue;
        const int cs = ts ? ts[j] : 0, cd = td ? td[j] : 0;
        v[0] = cs < v[0] ? cs : v[0]; v[1] = cs > v[1] ? cs : v[1];
        v[2] = cd < v[2] ? cd : v[2]; v[3] = cd > v[3] ? cd : v[3];
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int w = __shfl_xor(v[i], o, WAVE);
            v[i] = (i & 1) ? (w > v[i] ? w : v[i]) : (w < v[i] ? w : v[i]);
        }
    }
    if (threadIdx.x < 4) tmm[4 * tile + threadIdx.x] = v[threadIdx.x];
}

constexpr int KNN_MEAN_THREADS = 256;           // columns of a row per workgroup
template <typename T>
__global__ __launch_bounds__(KNN_MEAN_THREADS) void knn_mean_kernel(const int* idx, long ldi, const T* y, long ldy, float* out, long ldo, int k,
                                                               int Ny, int Fy) {
    const long row = blockIdx.x;
    const int c = blockIdx.y * KNN_MEAN_THREADS + threadIdx.x;
    if (c >= Fy) return;
    float s = 0.f;
    for (int n = 0; n < k; ++n) {
        long j = idx[row * ldi + n];
        j = j < 0 ? 0 : (j >= Ny ? (long)Ny - 1 : j);
        s += to_f32(y[j * ldy + c]);
    }
    out[row * ldo + c] = s / (float)k;
}

// Inverse-distance k-NN regression (mmvae_knn_weighted_rows): a workgroup owns one query row and 256 output columns.  The row's k
// weights (sklearn's _get_weights: 1 / d, or the indicator of d == 0 when any distance is 0) and clamped indices are computed once, into
// LDS; then every thread streams its column of the k neighbour rows: numerator and weight sum in ascending n, one division.
template <typename T>
__global__ __launch_bounds__(KNN_MEAN_THREADS) void knn_weighted_kernel(const int* idx, long ldi, const float* dist, long ldd, int squared,
                                                                   const T* y, long ldy, float* out, long ldo, int k, int Ny, int Fy) {
    __shared__ float sW[MMVAE_KNN_MAXK];
    __shared__ long sJ[MMVAE_KNN_MAXK];
    __shared__ int sFlag[2];                               // [0]: some distance is 0, [1]: some distance is NaN or negative
    const long row = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid < 2) sFlag[tid] = 0;
    __syncthreads();
    float d = 1.f;
    if (tid < k) {
        d = dist[row * ldd + tid];
        if (squared) d = __fsqrt_rn(d);
        if (d == 0.f) sFlag[0] = 1;                        // every writer stores the same value
        if (!(d >= 0.f)) sFlag[1] = 1;
        long j = idx[row * ldi + tid];
        sJ[tid] = j < 0 ? 0 : (j >= Ny ? (long)Ny - 1 : j);
    }
    __syncthreads();
    if (tid < k) {
        float w = sFlag[0] ? (d == 0.f ? 1.f : 0.f) : __fdiv_rn(1.f, d);
        if (sFlag[1]) w = __uint_as_float(0x7FC00000u);
        sW[tid] = w;
    }
    __syncthreads();
    const int c = blockIdx.y * KNN_MEAN_THREADS + tid;
    if (c >= Fy) return;
    float s = 0.f, ws = 0.f;
    for (int n = 0; n < k; ++n) {
        const float w = sW[n];
        s = __fadd_rn(s, __fmul_rn(w, to_f32(y[sJ[n] * ldy + c])));
        ws += w;
    }
    out[row * ldo + c] = __fdiv_rn(s, ws);
}

template <int S, bool L1, bool G>
static int knn_launch(int q_dtype, int t_dtype, const KnnArgsT<G>& p, dim3 grid, int lds, hipStream_t st) {
    constexpr int MAX_LDS = knn_max_lds(S) + (G ? KNN_CODE_BYTES : 0);
    if (q_dtype == MMVAE_F32)
        return t_dtype == MMVAE_F32 ? rt_launch_dyn_lds<knn_kernel<float, float, S, L1, G>, MAX_LDS>(p, grid, lds, st)
                                    : rt_launch_dyn_lds<knn_kernel<float, bf16, S, L1, G>, MAX_LDS>(p, grid, lds, st);
    return t_dtype == MMVAE_F32 ? rt_launch_dyn_lds<knn_kernel<bf16, float, S, L1, G>, MAX_LDS>(p, grid, lds, st)
                                : rt_launch_dyn_lds<knn_kernel<bf16, bf16, S, L1, G>, MAX_LDS>(p, grid, lds, st);
}

static bool knn_sizes_ok(int Mq, int Nt, int k) { return Mq >= 1 && Nt >= 1 && k >= 1 && k <= Nt && k <= MMVAE_KNN_MAXK; }

static void knn_plan(int Mq, int Nt, int* nsplit, int* tps) {
    const int ntiles = (int)(((long)Nt + KNN_BN - 1) / KNN_BN);
    const long want = rt_splits(((long)Mq + KNN_BM - 1) / KNN_BM, 0, KNN_TARGET_WG, KNN_MAX_SPLITS, ntiles);
    *tps = (int)((ntiles + want - 1) / want);
    *nsplit = (ntiles + *tps - 1) / *tps;
}

static long knn_norm_bytes(int Mq, int Nt) { return (4L * ((long)Mq + Nt) + 7) & ~7L; }

}  // namespace mm

extern "C" int mmvae_knn_work_bytes(int32_t Mq, int32_t Nt, int32_t k, int64_t* bytes) {
    using namespace mm;
    if (!bytes || !knn_sizes_ok(Mq, Nt, k)) return MMVAE_ERR_ARG;
    int nsplit, tps;
    knn_plan(Mq, Nt, &nsplit, &tps);
    *bytes = knn_norm_bytes(Mq, Nt) + (nsplit > 1 ? 8L * Mq * nsplit * k : 0L);
    return MMVAE_OK;
}

extern "C" int mmvae_knn_splits(int32_t Mq, int32_t Nt, int32_t* splits, int32_t* rows_per_split) {
    using namespace mm;
    if (!splits || !rows_per_split || Mq < 1 || Nt < 1) return MMVAE_ERR_ARG;
    int nsplit, tps;
    knn_plan(Mq, Nt, &nsplit, &tps);
    *splits = nsplit;
    const long rps = (long)tps * KNN_BN;                   // one split of more than 2^31 - 128 rows: the largest multiple of 128 that fits
    *rows_per_split = (int32_t)(rps > 2147483520L ? 2147483520L : rps);
    return MMVAE_OK;
}

extern "C" int mmvae_knn_l1_work_bytes(int32_t Mq, int32_t Nt, int32_t k, int64_t* bytes) {
    using namespace mm;
    if (!bytes || !knn_sizes_ok(Mq, Nt, k)) return MMVAE_ERR_ARG;
    int nsplit, tps;
    knn_plan(Mq, Nt, &nsplit, &tps);
    *bytes = nsplit > 1 ? 8L * Mq * nsplit * k : 0L;
    return MMVAE_OK;
}

namespace mm {
static long knn_tile_code_bytes(int Nt) { return 16L * (((long)Nt + KNN_BN - 1) / KNN_BN); }

// the ungrouped workspace of a metric: norms (euclidean) and split lists; the grouped search appends the tile codes
template <bool L1>
static long knn_base_bytes(int Mq, int Nt, int k) {
    int nsplit, tps;
    knn_plan(Mq, Nt, &nsplit, &tps);
    return (L1 ? 0L : knn_norm_bytes(Mq, Nt)) + (nsplit > 1 ? 8L * Mq * nsplit * k : 0L);
}

// all searches: the checks, the plan, (euclidean) the norms launch, (g: grouped) the tile codes launch, the search and the merge
template <bool L1, bool G>
static int knn_search_impl(const mmvae_knn_args* a, const mmvae_knn_group_args* g, void* stream) {
    if (!a || !a->q || !a->t || !a->idx) return MMVAE_ERR_ARG;
    if (L1 ? a->shift != nullptr : !a->work) return MMVAE_ERR_ARG;
    if constexpr (G) {
        if (!g->q_same != !g->t_same || !g->q_differ != !g->t_differ || (!g->q_same && !g->q_differ) || !a->work) return MMVAE_ERR_ARG;
        if ((uintptr_t)g->q_same % 4 || (uintptr_t)g->t_same % 4 || (uintptr_t)g->q_differ % 4 || (uintptr_t)g->t_differ % 4) return MMVAE_ERR_ARG;
    }
    if (a->F < 1 || !knn_sizes_ok(a->Mq, a->Nt, a->k)) return MMVAE_ERR_ARG;
    RtOperand oq, ot;
    const int rq = rt_operand(a->q, a->q_dtype, a->ld_q, a->F, &oq), rt = rt_operand(a->t, a->t_dtype, a->ld_t, a->F, &ot);
    if (rq == MMVAE_ERR_DTYPE || rt == MMVAE_ERR_DTYPE) return MMVAE_ERR_DTYPE;
    if (rq || rt || a->ld_idx < a->k || (a->dist2 && a->ld_dist2 < a->k)) return MMVAE_ERR_ARG;
    if ((uintptr_t)a->shift % 4 || (uintptr_t)a->idx % 4 || (uintptr_t)a->dist2 % 4 || (uintptr_t)a->work % 8) return MMVAE_ERR_ARG;
    const long base_bytes = knn_base_bytes<L1>(a->Mq, a->Nt, a->k);
    const int64_t need = base_bytes + (G ? knn_tile_code_bytes(a->Nt) : 0L);
    if (need > 0 && (!a->work || a->work_bytes < need)) return MMVAE_ERR_ARG;

    KnnArgsT<G> p;
    p.q = a->q; p.t = a->t; p.shift = a->shift;
    p.ldq = a->ld_q; p.ldt = a->ld_t;
    p.vq = oq.vec; p.vt = ot.vec;
    p.Mq = a->Mq; p.Nt = a->Nt; p.F = a->F; p.k = a->k; p.kp = (a->k + 15) & ~15;
    knn_plan(a->Mq, a->Nt, &p.nsplit, &p.tps);
    float* norms = L1 ? nullptr : (float*)a->work;
    p.qn = norms; p.tn = L1 ? nullptr : norms + a->Mq;
    const long lists_at = L1 ? 0 : knn_norm_bytes(a->Mq, a->Nt);
    p.part = p.nsplit > 1 ? (unsigned long long*)((char*)a->work + lists_at) : nullptr;
    p.idx = a->idx; p.ldi = a->ld_idx; p.dist2 = a->dist2; p.ldd = a->ld_dist2;
    hipStream_t st = (hipStream_t)stream;
    if constexpr (G) {
        p.qs = g->q_same; p.ts = g->t_same; p.qd = g->q_differ; p.td = g->t_differ;
        int* tmm = (int*)((char*)a->work + base_bytes);
        p.tmm = tmm;
        hipLaunchKernelGGL(knn_tile_codes_kernel, dim3((unsigned)(((long)a->Nt + KNN_BN - 1) / KNN_BN)), dim3(WAVE), 0, st, p.ts, p.td, a->Nt, tmm);
        MM_CHECK_LAUNCH();
    }

    int rc = 0;
    if (!L1) rc = rt_norms_launch({a->q, a->ld_q, a->q_dtype, a->Mq, nullptr}, {a->t, a->ld_t, a->t_dtype, a->Nt, nullptr}, a->F, a->shift, norms, st);
    if (rc) return rc;

    const dim3 grid((unsigned)(((long)a->Mq + KNN_BM - 1) / KNN_BM), (unsigned)p.nsplit);
    const int lds = KNN_TILE_BYTES + KNN_BM * p.kp * 8 + (G ? KNN_CODE_BYTES : 0);
    rc = p.kp <= 64 ? knn_launch<4, L1, G>(a->q_dtype, a->t_dtype, p, grid, lds, st) : knn_launch<KNN_SLOTS, L1, G>(a->q_dtype, a->t_dtype, p, grid, lds, st);
    if (rc) return rc;
    if (p.nsplit > 1) {
        hipLaunchKernelGGL((knn_merge_kernel<L1, G>), dim3((unsigned)a->Mq), dim3(WAVE), 0, st, static_cast<const KnnP&>(p));
        MM_CHECK_LAUNCH();
    }
    return MMVAE_OK;
}
}  // namespace mm

extern "C" int mmvae_knn_search(const mmvae_knn_args* a, void* stream) { return mm::knn_search_impl<false, false>(a, nullptr, stream); }
extern "C" int mmvae_knn_search_l1(const mmvae_knn_args* a, void* stream) { return mm::knn_search_impl<true, false>(a, nullptr, stream); }

extern "C" int mmvae_knn_group_work_bytes(int32_t Mq, int32_t Nt, int32_t k, int32_t metric, int64_t* bytes) {
    using namespace mm;
    if (!bytes || !knn_sizes_ok(Mq, Nt, k) || (metric != 0 && metric != 1)) return MMVAE_ERR_ARG;
    *bytes = (metric ? knn_base_bytes<true>(Mq, Nt, k) : knn_base_bytes<false>(Mq, Nt, k)) + knn_tile_code_bytes(Nt);
    return MMVAE_OK;
}

extern "C" int mmvae_knn_search_grouped(const mmvae_knn_group_args* g, void* stream) {
    if (!g || (g->metric != 0 && g->metric != 1)) return MMVAE_ERR_ARG;
    return g->metric ? mm::knn_search_impl<true, true>(&g->base, g, stream) : mm::knn_search_impl<false, true>(&g->base, g, stream);
}

extern "C" int mmvae_knn_mean_rows(const int32_t* idx, int64_t ld_idx, const void* y, int32_t y_dtype, int64_t ld_y, float* out, int64_t ld_out,
                                   int32_t Mq, int32_t k, int32_t Ny, int32_t Fy, void* stream) {
    using namespace mm;
    if (!idx || !y || !out || Mq < 1 || k < 1 || k > MMVAE_KNN_MAXK || Ny < 1 || Fy < 1) return MMVAE_ERR_ARG;
    RtOperand oy;
    if (const int rc = rt_operand(y, y_dtype, ld_y, Fy, &oy)) return rc;
    if (ld_idx < k || ld_out < Fy || (uintptr_t)idx % 4 || (uintptr_t)out % 4) return MMVAE_ERR_ARG;
    const long ct = ((long)Fy + KNN_MEAN_THREADS - 1) / KNN_MEAN_THREADS;
    if (ct > 65535) return MMVAE_ERR_ARG;
    const dim3 grid((unsigned)Mq, (unsigned)ct);
    hipStream_t st = (hipStream_t)stream;
    if (y_dtype == MMVAE_F32)
        hipLaunchKernelGGL((knn_mean_kernel<float>), grid, dim3(KNN_MEAN_THREADS), 0, st, idx, (long)ld_idx, (const float*)y, (long)ld_y, out, (long)ld_out, k, Ny, Fy);
    else
        hipLaunchKernelGGL((knn_mean_kernel<bf16>), grid, dim3(KNN_MEAN_THREADS), 0, st, idx, (long)ld_idx, (const bf16*)y, (long)ld_y, out, (long)ld_out, k, Ny, Fy);
    MM_CHECK_LAUNCH();
    return MMVAE_OK;
}

extern "C" int mmvae_knn_weighted_rows(const int32_t* idx, int64_t ld_idx, const float* dist, int64_t ld_dist, int32_t dist_is_squared,
                                       const void* y, int32_t y_dtype, int64_t ld_y, float* out, int64_t ld_out,
                                       int32_t Mq, int32_t k, int32_t Ny, int32_t Fy, void* stream) {
    using namespace mm;
    if (!idx || !dist || !y || !out || Mq < 1 || k < 1 || k > MMVAE_KNN_MAXK || Ny < 1 || Fy < 1) return MMVAE_ERR_ARG;
    RtOperand oy;
    if (const int rc = rt_operand(y, y_dtype, ld_y, Fy, &oy)) return rc;
    if (ld_idx < k || ld_dist < k || ld_out < Fy || (dist_is_squared != 0 && dist_is_squared != 1)) return MMVAE_ERR_ARG;
    if ((uintptr_t)idx % 4 || (uintptr_t)dist % 4 || (uintptr_t)out % 4) return MMVAE_ERR_ARG;
    const long ct = ((long)Fy + KNN_MEAN_THREADS - 1) / KNN_MEAN_THREADS;
    if (ct > 65535) return MMVAE_ERR_ARG;
    const dim3 grid((unsigned)Mq, (unsigned)ct);
    hipStream_t st = (hipStream_t)stream;
    if (y_dtype == MMVAE_F32)
        hipLaunchKernelGGL((knn_weighted_kernel<float>), grid, dim3(KNN_MEAN_THREADS), 0, st, idx, (long)ld_idx, dist, (long)ld_dist, dist_is_squared,
                           (const float*)y, (long)ld_y, out, (long)ld_out, k, Ny, Fy);
    else
        hipLaunchKernelGGL((knn_weighted_kernel<bf16>), grid, dim3(KNN_MEAN_THREADS), 0, st, idx, (long)ld_idx, dist, (long)ld_dist, dist_is_squared,
                           (const bf16*)y, (long)ld_y, out, (long)ld_out, k, Ny, Fy);
    MM_CHECK_LAUNCH();
    return MMVAE_OK;
}
