// Brute-force k nearest neighbours as a GEMM whose epilogue is a running top-k (mmvae_knn_search, include/mmvae_hip.h), and the uniform
// k-NN regression that follows it (mmvae_knn_mean_rows).
//
// Decomposition: a workgroup (4 waves, 2 x 2, 64 x 64 each) owns KNN_BM = 128 query rows and walks its training rows in tiles of
// KNN_BN = 128.  A tile's 128 x 128 dot products (q_i - c).(t_j - c) are accumulated over F in chunks of KNN_BK = 32 columns on the
// exact-f32 MFMA (Mma<float>): the chunk of both operands is loaded into registers (as wide as base and stride allow, widened and
// shifted in fp32) while the previous chunk is multiplied out of LDS, so one LDS buffer is enough.  At 32 cycles per
// v_mfma_f32_16x16x4_f32 a chunk costs a wave 128 MFMAs = 4096 cycles against 16 ds_read_b128 and 8 global loads per lane, and the
// selection below runs once per F / 4 * 16 MFMAs: LDS and selection are far from the bound.  Operand delivery is not (measured,
// 0.26 of the fp32 MFMA rate from fp32 rows, 0.42 from bf16 rows): every workgroup re-reads its query block per tile.
// Selection: a row's k best live in LDS as ONE sorted list of 64-bit entries (ordered key << 32 | j), so the order (key, j) is one
// unsigned compare and an empty slot is the largest entry.  After a tile a lane holds 64 keys; the compare path is one fp32 FMA, the
// order transform and a compare against the high word of the row's k-th entry, and a wave-wide vote skips the rest when no lane
// passed (after the first tiles: nearly always).  The insert path takes the 16 lanes that share a query row in the MFMA layout: they
// insert one candidate at a time, each lane rewriting the list positions li, li + 16, .. (new[p] = old[p] <= c ? old[p] :
// max(old[p-1], c)), the four row groups of the wave in lock step.  The two waves that share query rows take turns (one barrier each).
// Nothing in it depends on the order in which candidates arrive, so the result is a function of the keys alone.
// Split: grid.y workgroups per query block take consecutive runs of tiles; their lists go to the workspace and knn_merge_kernel ranks
// every entry among all lists of its row (own position + binary searches in the others): fixed order, no atomics.
// The squared norms |t_j - c|^2, |q_i - c|^2 come from one streaming launch (a wave per row) into the workspace.
#include "common.h"
#include "wave_slab.h"
#include "row_tile.h"

namespace mm {

constexpr int KNN_THREADS = 256;
constexpr int KNN_BM = 128, KNN_BN = 128, KNN_BK = 32;
constexpr int KNN_LDR = KNN_BK + 4;            // floats per LDS row: padded by one 16-byte chunk (wave_slab.h: stage_rows)
constexpr int KNN_TILE_BYTES = (KNN_BM + KNN_BN) * KNN_LDR * 4;
constexpr int KNN_MAX_LDS = KNN_TILE_BYTES + KNN_BM * MMVAE_KNN_MAXK * 8;
constexpr int KNN_TARGET_WG = 4 * NUM_CU;      // below this many query blocks the training rows are split
constexpr int KNN_MAX_SPLITS = 64;
constexpr unsigned long long KNN_EMPTY = ~0ull;
static_assert(MMVAE_KNN_MAXK % 16 == 0 && MMVAE_KNN_MAXK <= 64, "knn_insert: 16 lanes x 4 positions");

struct KnnP {
    const void* q; const void* t; const float* shift;
    long ldq, ldt; int vq, vt;
    int Mq, Nt, F, k, kp;                      // kp: k rounded up to 16, the stride of a row's list
    int nsplit, tps;                           // tiles per split
    const float* qn; const float* tn;
    unsigned long long* part;                  // [Mq][nsplit][k], NULL when nsplit == 1
    int* idx; long ldi; float* dist2; long ldd;
};

// fp32 key -> unsigned with the same order; -0 = +0, every NaN one value above +inf
__device__ __forceinline__ unsigned knn_order(float key) {
    key += 0.f;
    unsigned b = __float_as_uint(key);
    if (key != key) b = 0x7FC00000u;
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float knn_key(unsigned u) { return __uint_as_float((u >> 31) ? (u ^ 0x80000000u) : ~u); }

// The 16 lanes of a row group (lane >> 4) insert their passing candidates into the group's list, one at a time; the wave's four groups
// in lock step.  L: this lane's group's list (k sorted entries).
__device__ __forceinline__ void knn_insert(unsigned long long* L, bool pass, unsigned long long cand, int lane, int k) {
    const int li = lane & 15, g0 = lane & 48;
    unsigned long long pend = __ballot(pass);
    while (pend) {
        const unsigned gm = (unsigned)(pend >> g0) & 0xFFFFu;
        const bool act = gm != 0;
        const int src = g0 + (act ? __ffs(gm) - 1 : 0);
        const unsigned long long c = __shfl(cand, src, WAVE);
        unsigned long long nv[4];
        bool wr[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
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
        for (int s = 0; s < 4; ++s)
            if (wr[s]) L[li + 16 * s] = nv[s];
        wave_lds_sync();
        if (lane == src) pass = false;
        pend = __ballot(pass);
    }
}

template <typename TQ, typename TT>
__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(KnnP a) {
    extern __shared__ __align__(16) unsigned char knn_smem[];
    float* sQ = (float*)knn_smem;                          // [KNN_BM][KNN_LDR]
    float* sT = sQ + KNN_BM * KNN_LDR;                     // [KNN_BN][KNN_LDR]
    unsigned long long* sL = (unsigned long long*)(knn_smem + KNN_TILE_BYTES);   // [KNN_BM][kp]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4, wr = wave >> 1, wc = wave & 1;
    const long q0 = (long)blockIdx.x * KNN_BM;
    const int nr = (int)((long)a.Mq - q0 < KNN_BM ? (long)a.Mq - q0 : KNN_BM);
    const int split = blockIdx.y;
    const int ntiles = (a.Nt + KNN_BN - 1) / KNN_BN;
    const int tile_lo = split * a.tps;
    const int tile_hi = tile_lo + a.tps < ntiles ? tile_lo + a.tps : ntiles;
    const int nch = (a.F + KNN_BK - 1) / KNN_BK;
    const int k = a.k, kp = a.kp;
    for (int i = tid; i < KNN_BM * kp; i += KNN_THREADS) sL[i] = KNN_EMPTY;

    const TQ* qb = (const TQ*)a.q;
    const TT* tb = (const TT*)a.t;
    const int cq = tid & 7, rb = tid >> 3;                 // a thread stages columns 4 cq .. of rows rb, rb + 32, .. of both operands
    TQ rq[4][4];
    TT rt[4][4];
    float sh[4];
#define KNN_ISSUE(tile_, ch_) \
    { \
        const int c0_ = (ch_) * KNN_BK + 4 * cq; \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) { sh[j] = 0.f; if (a.shift && c0_ + j < a.F) sh[j] = a.shift[c0_ + j]; } \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) { \
            const int r_ = rb + 32 * i; \
            const long j_ = (long)(tile_) * KNN_BN + r_; \
            knn_ld4(qb + (q0 + r_) * a.ldq, r_ < nr, c0_, a.F, a.vq, rq[i]); \
            knn_ld4(tb + j_ * a.ldt, j_ < a.Nt, c0_, a.F, a.vt, rt[i]); \
        } \
    }

    f32x4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nsteps = (tile_hi - tile_lo) * nch;
    int tile = tile_lo, ch = 0;
    if (nsteps > 0) KNN_ISSUE(tile, ch)
    for (int s = 0; s < nsteps; ++s) {
        __syncthreads();                                   // the previous chunk has been multiplied (first step: the lists are initialised)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 vq, vt;
#pragma unroll
            for (int j = 0; j < 4; ++j) { vq[j] = to_f32(rq[i][j]) - sh[j]; vt[j] = to_f32(rt[i][j]) - sh[j]; }
            *(f32x4*)(sQ + (rb + 32 * i) * KNN_LDR + 4 * cq) = vq;
            *(f32x4*)(sT + (rb + 32 * i) * KNN_LDR + 4 * cq) = vt;
        }
        __syncthreads();
        int ntile = tile, nchk = ch + 1;
        if (nchk == nch) { nchk = 0; ++ntile; }
        if (s + 1 < nsteps) KNN_ISSUE(ntile, nchk)
#pragma unroll
        for (int kk = 0; kk < KNN_BK / 16; ++kk) {
            f32x4 fa[4], fb[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) fa[mi] = *(const f32x4*)(sQ + (wr * 64 + 16 * mi + li) * KNN_LDR + 16 * kk + 4 * lg);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) fb[ni] = *(const f32x4*)(sT + (wc * 64 + 16 * ni + li) * KNN_LDR + 16 * kk + 4 * lg);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) Mma<float>::mma(acc[mi][ni], fa[mi], fb[ni]);
        }
        if (nchk == 0) {
            // the tile is complete: acc[mi][ni][r] = (q_row - c).(t_j - c), row = wr*64 + 16 mi + 4 lg + r, j = tile*128 + wc*64 + 16 ni + li
            for (int phase = 0; phase < 2; ++phase) {
                if (wc == phase) {
                    float tnv[4];
                    bool jok[4];
                    unsigned jlo[4];
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        const long j = (long)tile * KNN_BN + wc * 64 + 16 * ni + li;
                        jok[ni] = j < a.Nt;
                        jlo[ni] = (unsigned)j;
                        tnv[ni] = jok[ni] ? a.tn[j] : 0.f;
                    }
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = wr * 64 + 16 * mi + 4 * lg + r;
                            unsigned long long* L = sL + row * kp;
                            const unsigned thr = (unsigned)(L[k - 1] >> 32);
#pragma unroll
                            for (int ni = 0; ni < 4; ++ni) {
                                const unsigned u = knn_order(tnv[ni] - 2.f * acc[mi][ni][r]);
                                const bool pass = jok[ni] && row < nr && u <= thr;
                                if (__any(pass)) knn_insert(L, pass, ((unsigned long long)u << 32) | jlo[ni], lane, k);
                            }
                        }
                }
                __syncthreads();
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        tile = ntile; ch = nchk;
    }
#undef KNN_ISSUE
    __syncthreads();
    for (int i = tid; i < nr * k; i += KNN_THREADS) {
        const int row = i / k, n = i - row * k;
        const unsigned long long e = sL[row * kp + n];
        if (a.part) a.part[((q0 + row) * a.nsplit + split) * k + n] = e;
        else {
            a.idx[(q0 + row) * a.ldi + n] = (int)(unsigned)e;
            if (a.dist2) { const float d = knn_key((unsigned)(e >> 32)) + a.qn[q0 + row]; a.dist2[(q0 + row) * a.ldd + n] = d < 0.f ? 0.f : d; }
        }
    }
}

// One wave per query row: the rank of an entry among all lists of the row is its own position plus its lower bounds in the others
// (the entries of a row are distinct: every j is in one split).  Empty slots (a split with fewer than k rows) rank last and are skipped.
__global__ __launch_bounds__(WAVE) void knn_merge_kernel(KnnP a) {
    const long row = blockIdx.x;
    const int k = a.k, ns = a.nsplit;
    const unsigned long long* P = a.part + row * ns * k;
    for (int t = threadIdx.x; t < ns * k; t += WAVE) {
        const unsigned long long v = P[t];
        if (v == KNN_EMPTY) continue;
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
            if (a.dist2) { const float d = knn_key((unsigned)(v >> 32)) + a.qn[row]; a.dist2[row * a.ldd + rank] = d < 0.f ? 0.f : d; }
        }
    }
}

// |x - c|^2 of every query row (out[0 .. Mq)) and training row (out[Mq .. Mq + Nt)): a wave per row, a lane sums every 64th column and
// the butterfly adds the lanes -- a function of the row's values alone.
__global__ __launch_bounds__(KNN_THREADS) void knn_norms_kernel(KnnP a, float* out) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (KNN_THREADS / WAVE) + (threadIdx.x >> 6);
    if (row >= (long)a.Mq + a.Nt) return;
    const bool isq = row < a.Mq;
    const long r = isq ? row : row - a.Mq;
    const int dt = isq ? a.vq >> 8 : a.vt >> 8;            // the host passes the dtype above the vector width here
    const char* base = (const char*)(isq ? a.q : a.t) + r * (isq ? a.ldq : a.ldt) * (dt == MMVAE_BF16 ? 2 : 4);
    const float s = row_sqnorm(base, dt, a.F, a.shift, lane);
    if (lane == 0) out[row] = s;
}

template <typename T>
__global__ __launch_bounds__(KNN_THREADS) void knn_mean_kernel(const int* idx, long ldi, const T* y, long ldy, float* out, long ldo, int k,
                                                               int Ny, int Fy) {
    const long row = blockIdx.x;
    const int c = blockIdx.y * KNN_THREADS + threadIdx.x;
    if (c >= Fy) return;
    float s = 0.f;
    for (int n = 0; n < k; ++n) {
        long j = idx[row * ldi + n];
        j = j < 0 ? 0 : (j >= Ny ? (long)Ny - 1 : j);
        s += to_f32(y[j * ldy + c]);
    }
    out[row * ldo + c] = s / (float)k;
}

static bool knn_sizes_ok(int Mq, int Nt, int k) { return Mq >= 1 && Nt >= 1 && k >= 1 && k <= Nt && k <= MMVAE_KNN_MAXK; }

static void knn_plan(int Mq, int Nt, int* nsplit, int* tps) {
    const long nqb = ((long)Mq + KNN_BM - 1) / KNN_BM;
    const int ntiles = (int)(((long)Nt + KNN_BN - 1) / KNN_BN);
    long want = nqb >= KNN_TARGET_WG ? 1 : (KNN_TARGET_WG + nqb - 1) / nqb;
    if (want > KNN_MAX_SPLITS) want = KNN_MAX_SPLITS;
    if (want > ntiles) want = ntiles;
    *tps = (int)((ntiles + want - 1) / want);
    *nsplit = (ntiles + *tps - 1) / *tps;
}

static long knn_norm_bytes(int Mq, int Nt) { return (4L * ((long)Mq + Nt) + 7) & ~7L; }

template <typename TQ, typename TT>
static int knn_launch(const KnnP& p, dim3 grid, int lds, hipStream_t st) {
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)knn_kernel<TQ, TT>, hipFuncAttributeMaxDynamicSharedMemorySize, KNN_MAX_LDS);
        if (e != hipSuccess) return (int)e;
        attr_done = true;
    }
    hipLaunchKernelGGL((knn_kernel<TQ, TT>), grid, dim3(KNN_THREADS), lds, st, p);
    return (int)hipGetLastError();
}

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

extern "C" int mmvae_knn_search(const mmvae_knn_args* a, void* stream) {
    using namespace mm;
    if (!a || !a->q || !a->t || !a->idx || !a->work) return MMVAE_ERR_ARG;
    if (a->F < 1 || !knn_sizes_ok(a->Mq, a->Nt, a->k)) return MMVAE_ERR_ARG;
    if ((a->q_dtype != MMVAE_F32 && a->q_dtype != MMVAE_BF16) || (a->t_dtype != MMVAE_F32 && a->t_dtype != MMVAE_BF16)) return MMVAE_ERR_DTYPE;
    if (a->ld_q < a->F || a->ld_t < a->F || a->ld_idx < a->k || (a->dist2 && a->ld_dist2 < a->k)) return MMVAE_ERR_ARG;
    const int eq = a->q_dtype == MMVAE_BF16 ? 2 : 4, et = a->t_dtype == MMVAE_BF16 ? 2 : 4;
    if ((uintptr_t)a->q % eq || (uintptr_t)a->t % et || (uintptr_t)a->shift % 4 || (uintptr_t)a->idx % 4 || (uintptr_t)a->dist2 % 4 ||
        (uintptr_t)a->work % 8)
        return MMVAE_ERR_ARG;
    int64_t need;
    if (mmvae_knn_work_bytes(a->Mq, a->Nt, a->k, &need) != MMVAE_OK || a->work_bytes < need) return MMVAE_ERR_ARG;

    KnnP p;
    p.q = a->q; p.t = a->t; p.shift = a->shift;
    p.ldq = a->ld_q; p.ldt = a->ld_t;
    p.vq = knn_vec(a->q, a->ld_q, eq); p.vt = knn_vec(a->t, a->ld_t, et);
    p.Mq = a->Mq; p.Nt = a->Nt; p.F = a->F; p.k = a->k; p.kp = (a->k + 15) & ~15;
    knn_plan(a->Mq, a->Nt, &p.nsplit, &p.tps);
    float* norms = (float*)a->work;
    p.qn = norms; p.tn = norms + a->Mq;
    p.part = p.nsplit > 1 ? (unsigned long long*)((char*)a->work + knn_norm_bytes(a->Mq, a->Nt)) : nullptr;
    p.idx = a->idx; p.ldi = a->ld_idx; p.dist2 = a->dist2; p.ldd = a->ld_dist2;
    hipStream_t st = (hipStream_t)stream;

    KnnP pn = p;
    pn.vq |= a->q_dtype << 8; pn.vt |= a->t_dtype << 8;
    const long nrows = (long)a->Mq + a->Nt;
    hipLaunchKernelGGL(knn_norms_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(KNN_THREADS), 0, st, pn, norms);
    MM_CHECK_LAUNCH();

    const dim3 grid((unsigned)(((long)a->Mq + KNN_BM - 1) / KNN_BM), (unsigned)p.nsplit);
    const int lds = KNN_TILE_BYTES + KNN_BM * p.kp * 8;
    int rc;
    if (a->q_dtype == MMVAE_F32) rc = a->t_dtype == MMVAE_F32 ? knn_launch<float, float>(p, grid, lds, st) : knn_launch<float, bf16>(p, grid, lds, st);
    else rc = a->t_dtype == MMVAE_F32 ? knn_launch<bf16, float>(p, grid, lds, st) : knn_launch<bf16, bf16>(p, grid, lds, st);
    if (rc) return rc;
    if (p.nsplit > 1) {
        hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)a->Mq), dim3(WAVE), 0, st, p);
        MM_CHECK_LAUNCH();
    }
    return MMVAE_OK;
}

extern "C" int mmvae_knn_mean_rows(const int32_t* idx, int64_t ld_idx, const void* y, int32_t y_dtype, int64_t ld_y, float* out, int64_t ld_out,
                                   int32_t Mq, int32_t k, int32_t Ny, int32_t Fy, void* stream) {
    using namespace mm;
    if (!idx || !y || !out || Mq < 1 || k < 1 || k > MMVAE_KNN_MAXK || Ny < 1 || Fy < 1) return MMVAE_ERR_ARG;
    if (y_dtype != MMVAE_F32 && y_dtype != MMVAE_BF16) return MMVAE_ERR_DTYPE;
    if (ld_idx < k || ld_y < Fy || ld_out < Fy) return MMVAE_ERR_ARG;
    if ((uintptr_t)idx % 4 || (uintptr_t)out % 4 || (uintptr_t)y % (y_dtype == MMVAE_BF16 ? 2 : 4)) return MMVAE_ERR_ARG;
    const long ct = ((long)Fy + KNN_THREADS - 1) / KNN_THREADS;
    if (ct > 65535) return MMVAE_ERR_ARG;
    const dim3 grid((unsigned)Mq, (unsigned)ct);
    hipStream_t st = (hipStream_t)stream;
    if (y_dtype == MMVAE_F32)
        hipLaunchKernelGGL((knn_mean_kernel<float>), grid, dim3(KNN_THREADS), 0, st, idx, (long)ld_idx, (const float*)y, (long)ld_y, out, (long)ld_out, k, Ny, Fy);
    else
        hipLaunchKernelGGL((knn_mean_kernel<bf16>), grid, dim3(KNN_THREADS), 0, st, idx, (long)ld_idx, (const bf16*)y, (long)ld_y, out, (long)ld_out, k, Ny, Fy);
    MM_CHECK_LAUNCH();
    return MMVAE_OK;
}
