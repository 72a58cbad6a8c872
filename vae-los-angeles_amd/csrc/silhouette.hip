// Silhouette coefficient of every row (sklearn's silhouette_samples, euclidean) as a distance GEMM whose epilogue is a square root and a
// per-class row sum (mmvae_silhouette_samples, include/mmvae_hip.h): the N x N distances never reach memory.
//
// Rows are addressed by POSITION p in the class-grouped order (row order[p], or p itself without `order`); class c owns the positions
// class_start[c] .. class_start[c + 1) - 1.  Decomposition: a workgroup (4 waves, 2 x 2, 64 x 64 each) owns SIL_BM = 128 positions as
// query rows and walks the column positions class by class in tiles of SIL_BN = 128 that never cross a class boundary (the last tile
// of a class is partial), so a tile's contribution to S[i][c] = sum_{j in c} |x_i - x_j| is a plain row sum.  The tile's dot products
// (x_i - s).(x_j - s) are accumulated over F in chunks of RT_BK = 32 on the exact-f32 MFMA with the row-tile pipeline
// (row_tile.h): the next chunk of both operands is loaded into registers while the current one is multiplied out of the single LDS buffer.
// Tile epilogue: d = sqrt(max(n_i + n_j - 2 dot, 0)), forced to 0 on the diagonal (query position == column position) and beyond the
// class segment; a lane adds its four columns, a DPP butterfly adds the 16 lanes that share the row, the two column waves are added through
// LDS (wave column 0 first) and the sum goes to sS[row][c] in LDS.  Every sum has one fixed order: no atomics, bit-identical runs.
// Split: grid.y workgroups per row block take consecutive runs of tiles (of the device-side tile list: class_start is device data);
// each writes its [C] partial sums per position to the workspace and sil_finish_kernel adds them in ascending split order and forms
// a, b and s.  With one split the main kernel finishes its rows itself.
// The squared norms |x_p - s|^2 come from one streaming launch (rt_norms_launch: a wave per position) into the workspace.
#include "common.h"
#include "row_tile.h"

namespace mm {

constexpr int SIL_BM = 128, SIL_BN = 128;       // positions of a workgroup, most columns of a tile
constexpr int SIL_TILE_BYTES = (SIL_BM + SIL_BN) * RT_LDR * 4;
constexpr int SIL_CLS = MMVAE_SIL_MAXC + 2;    // ints per class table in LDS
constexpr int SIL_HDR_BYTES = (2 * SIL_BM + 2 * SIL_CLS) * 4;          // sQn, sPair, sCs, sTs
constexpr int SIL_MAX_LDS = SIL_TILE_BYTES + SIL_HDR_BYTES + SIL_BM * MMVAE_SIL_MAXC * 4;
constexpr int SIL_TARGET_WG = 4 * NUM_CU;      // below this many row blocks the column tiles are split
constexpr int SIL_MAX_SPLITS = 64;

struct SilP {
    const void* x; const float* shift; const int* order; const int* class_start;
    long ldx; int vec;
    int N, F, C, nsplit;
    const float* norms;                        // [N] by position
    float* part;                               // [N][nsplit][C] by position, NULL when nsplit == 1
    float* s; float* intra; float* inter;      // [N] by row
};

// the row of position p; values of `order` outside [0, N) are clamped
__device__ __forceinline__ long sil_row(const SilP& a, long p) { return rt_row(a.order, p, a.N); }

// Sum over the 16 lanes (lane & 15) that share an accumulator row, in every one of them: a butterfly of four DPP row rotations (by 8,
// 4, 2, 1 lanes inside the 16-lane row; after each step the values repeat with that period, so every lane adds the same pair and all
// 16 hold one bit pattern) -- no LDS round trip as __shfl_xor takes.
__device__ __forceinline__ float sil_row16_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x128, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x124, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x122, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x121, 0xf, 0xf, true));
    return v;
}

// sCs[c]: first position of class c (clamped to [0, N], made non-decreasing, sCs[0] = 0 and sCs[C] = N whatever the vector holds);
// sTs[c]: index of the class's first tile in the list of all column tiles.  Ends with a barrier.
__device__ __forceinline__ void sil_classes(const SilP& a, int* sCs, int* sTs, int tid) {
    for (int c = tid; c <= a.C; c += RT_THREADS) {
        int v = a.class_start[c];
        v = v < 0 ? 0 : (v > a.N ? a.N : v);
        sCs[c] = c == 0 ? 0 : (c == a.C ? a.N : v);
    }
    __syncthreads();
    if (tid == 0) {
        int prev = 0, ts = 0;
        sTs[0] = 0;
        for (int c = 1; c <= a.C; ++c) {
            const int v = sCs[c] > prev ? sCs[c] : prev;
            sCs[c] = v;
            ts += (int)(((long)v - prev + SIL_BN - 1) / SIL_BN);
            sTs[c] = ts;
            prev = v;
        }
    }
    __syncthreads();
}

// a, b and s of position p from its class sums S(c), written at the position's row
template <typename Get>
__device__ __forceinline__ void sil_finish(const SilP& a, const int* sCs, long p, Get S) {
    float av = 0.f, bv = INFINITY;
    int nown = 0;
    for (int c = 0; c < a.C; ++c) {
        const int n = sCs[c + 1] - sCs[c];
        if (n <= 0) continue;                                  // an empty class is no neighbour cluster
        const float sc = S(c);
        if (p >= sCs[c] && p < sCs[c + 1]) { nown = n; av = n > 1 ? sc / (float)(n - 1) : 0.f; }
        else { const float m = sc / (float)n; bv = m < bv ? m : bv; }
    }
    const float mx = av > bv ? av : bv;
    const float sv = (nown > 1 && mx > 0.f && bv < INFINITY) ? (bv - av) / mx : 0.f;
    const long r = sil_row(a, p);
    a.s[r] = sv;
    if (a.intra) a.intra[r] = av;
    if (a.inter) a.inter[r] = bv;
}

template <typename T>
__global__ __launch_bounds__(RT_THREADS) void sil_kernel(SilP a) {
    extern __shared__ __align__(16) unsigned char sil_smem[];
    float* sQ = (float*)sil_smem;                          // [SIL_BM][RT_LDR]
    float* sT = sQ + SIL_BM * RT_LDR;                      // [SIL_BN][RT_LDR]
    float* sQn = (float*)(sil_smem + SIL_TILE_BYTES);      // [SIL_BM] norms of the query positions
    float* sPair = sQn + SIL_BM;                           // [SIL_BM] row sums of wave column 1
    int* sCs = (int*)(sPair + SIL_BM);                     // [C + 1]
    int* sTs = sCs + SIL_CLS;                              // [C + 1]
    float* sS = (float*)(sTs + SIL_CLS);                   // [SIL_BM][C]
    const int tid = threadIdx.x;
    const RtMap m(tid);
    const int li = m.li, wc = m.wc;
    const long q0 = (long)blockIdx.x * SIL_BM;
    const int nr = (int)((long)a.N - q0 < SIL_BM ? (long)a.N - q0 : SIL_BM);
    const int split = blockIdx.y, C = a.C;
    const int nch = (a.F + RT_BK - 1) / RT_BK;
    sil_classes(a, sCs, sTs, tid);
    for (int i = tid; i < SIL_BM * C; i += RT_THREADS) sS[i] = 0.f;
    if (tid < SIL_BM) sQn[tid] = tid < nr ? a.norms[q0 + tid] : 0.f;

    const int ntiles = sTs[C];
    const int tps = (ntiles + a.nsplit - 1) / a.nsplit;
    const int tile_lo = split * tps < ntiles ? split * tps : ntiles;
    const int tile_hi = tile_lo + tps < ntiles ? tile_lo + tps : ntiles;

    const T* xb = (const T*)a.x;
    const T* qrow[4];
    const T* crow[4];
    bool qok[4], cok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        qok[i] = m.rb + 32 * i < nr;
        qrow[i] = xb + (qok[i] ? sil_row(a, q0 + m.rb + 32 * i) : 0L) * a.ldx;
        crow[i] = xb;
        cok[i] = false;
    }
    RtStage<T, 4, 32, RT_LDR> rq, rt;
    float sh[4];
    float tn_cur[4], tn_nxt[4];                            // norms of the lane's four columns: loaded a tile ahead, with the tile's first chunk
    // (class, first position, columns) of the tile being multiplied and of the tile whose loads are being issued
    int cur_c = 0, cur_j0 = 0, cur_jn = 0, nxt_c = 0, nxt_j0 = 0, nxt_jn = 0;
    auto next_tile = [&](int t) {                          // the column rows and norms of tile t of the list
        while (t >= sTs[nxt_c + 1]) ++nxt_c;
        nxt_j0 = sCs[nxt_c] + (t - sTs[nxt_c]) * SIL_BN;
        nxt_jn = sCs[nxt_c + 1] - nxt_j0 < SIL_BN ? sCs[nxt_c + 1] - nxt_j0 : SIL_BN;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            cok[i] = m.rb + 32 * i < nxt_jn;
            crow[i] = xb + (cok[i] ? sil_row(a, (long)nxt_j0 + m.rb + 32 * i) : 0L) * a.ldx;
            const int col = m.acc_col(wc * 64, i);
            tn_nxt[i] = col < nxt_jn ? a.norms[(long)nxt_j0 + col] : 0.f;
        }
    };
    auto issue = [&](int ch) {
        const int c0 = ch * RT_BK + 4 * m.cq;
        rt_shift4(a.shift, c0, a.F, sh);
        rq.issue(qrow, qok, c0, a.F, a.vec);
        rt.issue(crow, cok, c0, a.F, a.vec);
    };
    auto advance = [&]() {                                 // the tile whose loads were issued becomes the tile being multiplied
        cur_c = nxt_c; cur_j0 = nxt_j0; cur_jn = nxt_jn;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) tn_cur[ni] = tn_nxt[ni];
    };

    f32x4 acc[4][4];
    zero_acc(acc);
    const int nsteps = (tile_hi - tile_lo) * nch;
    int tile = tile_lo, ch = 0;
    if (nsteps > 0) {
        next_tile(tile);
        issue(ch);
        advance();
    }
    for (int s = 0; s < nsteps; ++s) {
        __syncthreads();                                   // the previous chunk has been multiplied (first step: sS, sQn are initialised)
        rq.store(sQ, m.rb, m.cq, sh);
        rt.store(sT, m.rb, m.cq, sh);
        __syncthreads();
        int ntile = tile, nchk = ch + 1;
        if (nchk == nch) { nchk = 0; ++ntile; }
        if (s + 1 < nsteps) {
            if (nchk == 0) next_tile(ntile);               // every load of the current tile has been issued
            issue(nchk);
        }
        mma_chunk(acc, sQ, m.wr * 64, sT, wc * 64, m);
        if (nchk == 0) {
            // the tile is complete: acc[mi][ni][r] = (x_i - s).(x_j - s), i = q0 + acc_row, j = cur_j0 + acc_col
            bool jok[4];
            long jpos[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int col = m.acc_col(wc * 64, ni);
                jok[ni] = col < cur_jn;
                jpos[ni] = (long)cur_j0 + col;
            }
            float rsum[4][4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = m.acc_row(m.wr * 64, mi, r);
                    const float qn = sQn[row];
                    float v = 0.f;
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        const float d2 = (qn + tn_cur[ni]) - 2.f * acc[mi][ni][r];
                        float d = sqrtf(d2 > 0.f ? d2 : 0.f);
                        if (!jok[ni] || q0 + row == jpos[ni]) d = 0.f;
                        v += d;
                    }
                    rsum[mi][r] = sil_row16_sum(v);
                }
            if (wc == 1 && li == 0) {
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sPair[m.acc_row(m.wr * 64, mi, r)] = rsum[mi][r];
            }
            __syncthreads();
            if (wc == 0 && li == 0) {
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = m.acc_row(m.wr * 64, mi, r);
                        sS[row * C + cur_c] += rsum[mi][r] + sPair[row];
                    }
            }
            zero_acc(acc);
            advance();
        }
        tile = ntile; ch = nchk;
    }
    __syncthreads();
    if (a.part) {
        for (int i = tid; i < nr * C; i += RT_THREADS) {
            const int row = i / C, c = i - row * C;
            a.part[((q0 + row) * a.nsplit + split) * C + c] = sS[i];
        }
    } else if (tid < nr) {
        const float* S = sS + tid * C;
        sil_finish(a, sCs, q0 + tid, [S](int c) { return S[c]; });
    }
}

// a thread per position: the splits' partial sums of a class are added in ascending split order
__global__ __launch_bounds__(RT_THREADS) void sil_finish_kernel(SilP a) {
    __shared__ int sCs[SIL_CLS], sTs[SIL_CLS];
    sil_classes(a, sCs, sTs, threadIdx.x);
    const long p = (long)blockIdx.x * RT_THREADS + threadIdx.x;
    if (p >= a.N) return;
    const float* P = a.part + p * a.nsplit * a.C;
    const int ns = a.nsplit, C = a.C;
    sil_finish(a, sCs, p, [P, ns, C](int c) {
        float v = P[c];
        for (int s = 1; s < ns; ++s) v += P[s * C + c];
        return v;
    });
}

static bool sil_sizes_ok(int N, int C) { return N >= 2 && C >= 1 && C <= MMVAE_SIL_MAXC; }

// upper bound of the number of column tiles over every class_start of C classes on N rows: a class of n rows has ceil(n / 128) <= n tiles
static long sil_tiles_bound(int N, int C) {
    const long t = ((long)N + (long)(SIL_BN - 1) * C) / SIL_BN;
    return t < N ? t : N;
}

static int sil_plan(int N, int C, int want_in) {
    return (int)rt_splits(((long)N + SIL_BM - 1) / SIL_BM, want_in, SIL_TARGET_WG, SIL_MAX_SPLITS, sil_tiles_bound(N, C));
}

static long sil_norm_bytes(int N) { return (4L * N + 7) & ~7L; }

}  // namespace mm

extern "C" int mmvae_silhouette_splits(int32_t N, int32_t C, int32_t splits, int32_t* splits_used) {
    using namespace mm;
    if (!splits_used || !sil_sizes_ok(N, C) || splits < 0 || splits > SIL_MAX_SPLITS) return MMVAE_ERR_ARG;
    *splits_used = sil_plan(N, C, splits);
    return MMVAE_OK;
}

extern "C" int mmvae_silhouette_work_bytes(int32_t N, int32_t C, int32_t splits, int64_t* bytes) {
    using namespace mm;
    if (!bytes || !sil_sizes_ok(N, C) || splits < 0 || splits > SIL_MAX_SPLITS) return MMVAE_ERR_ARG;
    const int ns = sil_plan(N, C, splits);
    *bytes = sil_norm_bytes(N) + (ns > 1 ? 4L * N * ns * C : 0L);
    return MMVAE_OK;
}

extern "C" int mmvae_silhouette_samples(const mmvae_silhouette_args* a, void* stream) {
    using namespace mm;
    if (!a || !a->x || !a->class_start || !a->s || !a->work) return MMVAE_ERR_ARG;
    if (a->F < 1 || !sil_sizes_ok(a->N, a->C) || a->splits < 0 || a->splits > SIL_MAX_SPLITS) return MMVAE_ERR_ARG;
    RtOperand ox;
    if (const int rc = rt_operand(a->x, a->x_dtype, a->ld_x, a->F, &ox)) return rc;
    if ((uintptr_t)a->shift % 4 || (uintptr_t)a->order % 4 || (uintptr_t)a->class_start % 4 || (uintptr_t)a->s % 4 ||
        (uintptr_t)a->intra % 4 || (uintptr_t)a->inter % 4 || (uintptr_t)a->work % 8)
        return MMVAE_ERR_ARG;
    int64_t need;
    if (mmvae_silhouette_work_bytes(a->N, a->C, a->splits, &need) != MMVAE_OK || a->work_bytes < need) return MMVAE_ERR_ARG;

    SilP p;
    p.x = a->x; p.shift = a->shift; p.order = a->order; p.class_start = a->class_start;
    p.ldx = a->ld_x; p.vec = ox.vec;
    p.N = a->N; p.F = a->F; p.C = a->C; p.nsplit = sil_plan(a->N, a->C, a->splits);
    float* norms = (float*)a->work;
    p.norms = norms;
    p.part = p.nsplit > 1 ? (float*)((char*)a->work + sil_norm_bytes(a->N)) : nullptr;
    p.s = a->s; p.intra = a->intra; p.inter = a->inter;
    hipStream_t st = (hipStream_t)stream;

    int rc = rt_norms_launch({a->x, a->ld_x, a->x_dtype, a->N, a->order}, {nullptr, 0, MMVAE_F32, 0, nullptr}, a->F, a->shift, norms, st);
    if (rc) return rc;
    const dim3 grid((unsigned)(((long)a->N + SIL_BM - 1) / SIL_BM), (unsigned)p.nsplit);
    const int lds = SIL_TILE_BYTES + SIL_HDR_BYTES + SIL_BM * a->C * 4;
    rc = a->x_dtype == MMVAE_F32 ? rt_launch_dyn_lds<sil_kernel<float>, SIL_MAX_LDS>(p, grid, lds, st)
                                 : rt_launch_dyn_lds<sil_kernel<bf16>, SIL_MAX_LDS>(p, grid, lds, st);
    if (rc) return rc;
    if (p.nsplit > 1) {
        hipLaunchKernelGGL(sil_finish_kernel, dim3((unsigned)(((long)a->N + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, st, p);
        MM_CHECK_LAUNCH();
    }
    return MMVAE_OK;
}
