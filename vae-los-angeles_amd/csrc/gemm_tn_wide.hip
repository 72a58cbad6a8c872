// Wide-tile TN GEMM for the LARGE weight gradients of the step (gfx950, bf16 MFMA):
//     dW[N,K] += P[M,N]^T * Q[M,K],   db[N] += column sums of P
// for the first encoder layers: P = BatchNorm-backward-corrected dY built from the bf16 d and y tensors, Q = the fp32 input batch
// (EncoderB.L0.dW 512 x 572, EncoderA.L0.dW 128 x 782).  Reference op: the autograd mm of nn.Linear's backward behind
// optimize_hyperparameters.py:112 (layers encoders.py:13,31).
//
// Why a second kernel next to gemm_tn.hip's 128 x 128 tiles.  With M = 65 536 batch rows and a 1 MB output, the batch is split
// over all 256 CUs and every workgroup streams its rows of P and Q once PER OUTPUT TILE: 128 x 128 tiles re-ingest P five times
// and Q four times for the 512 x 572 gradient (1.27 GB through the L2 -> CU path, which moves ~60 GB/s per CU: 83 us before any
// arithmetic), and repeat the BatchNorm correction of P and the fp32 -> bf16 conversion of Q as often.  Here a workgroup of
// 8 waves owns a 256 x 288 (or 128 x 448) tile: 2 x 2 tiles for that gradient, P re-read twice and Q twice (0.57 GB),
// 36 MFMAs per wave and batch step on 13 transposed fragments.
//
// Two forms.  gemm_tnw_dma_kernel (256 x 288 tiles, 16-byte aligned fp32 rows; also 128 x 448 with a plain bf16 P -- very wide inputs,
// where the BatchNorm correction runs as a pass of its own): raw tiles by LDS-DMA, everything else at fragment time (below).  gemm_tnw_kernel (128 x 448 tiles; EncoderA.L0: fp32 rows only 8-byte aligned): global -> VGPR -> correction /
// conversion -> LDS with one register set, double-buffered LDS, one barrier per step.  Plain bf16 x bf16 problems (the decoders'
// gradients) were measured on these tiles too and stay with gemm_tn.hip's 128 x 128 LDS-DMA form (57-59 against 58 us, larger reduce).
//
// Layout: a batch step is 32 rows (one 16x16x32 MFMA reduction).  bf16 tiles sit row-major in LDS in the swizzled layout of
// gemm_tn_tile.h, rows padded to a multiple of 256 bytes (whole panels).  The block mapping and the epilogues are that header's too;
// the BatchNorm-backward correction of P is gemm_src.h's (BnBwdCols / BnBwdConst, shared with the 128 x 128 kernel's operand
// source), the LDS-DMA issue common.h's.  Partial tiles of the batch splits go to the slab workspace and are summed by
// gemm_tn.hip's tn_reduce_kernel (fixed order up to 128 splits).
#include "common.h"
#include "mmvae_hip.h"
#include "gemm_src.h"
#include "gemm_tn_tile.h"

namespace mm {

struct TnwArgs {
    const bf16* p; unsigned ldp; const bf16* py; unsigned ldpy;
    // bn.coef == nullptr: mmvae_bn_bwd_finalize folded in -- the constants from the f64 sums, dgamma / dbeta by the (zz == 0, tk == 0) workgroups
    BnBwdCols bn; float* dgamma; float* dbeta;
    const void* q; unsigned ldq;
    int M, N, K, ntk, ntiles, nsplit, rps, linear;
    float* slab; float* db;
};

// dgamma += sum d * xhat, dbeta += sum d: once per column, by the first batch split of the first K tile of every N tile
__device__ __forceinline__ void tnw_bn_grads(const TnwArgs& a, int n0, int nt, int zz, int tk, int tid, int nthreads) {
    if (a.bn.coef || zz != 0 || tk != 0) return;
    for (int c = tid; c < nt; c += nthreads) {
        const int col = n0 + c;
        if (col < a.N) { a.dbeta[col] += (float)a.bn.sum_d[col]; a.dgamma[col] += (float)a.bn.sum_dx[col]; }
    }
}

template <int WN_, int PA_, int WK_, int QB_> struct TnwCfg {
    static constexpr int WN = WN_, PA = PA_, WK = WK_, QB = QB_;
    static constexpr int NT = WN * PA * 16, KT = WK * QB * 16;
    static constexpr int PROW = (NT * 2 + 255) / 256 * 256, QROW = (KT * 2 + 255) / 256 * 256;
    static constexpr int PCH = NT / 8, QCH = KT / 8;                 // 16-byte bf16 chunks per tile row
    static constexpr int MT = 32, THREADS = 512;
    static constexpr int PI = (MT * PCH + THREADS - 1) / THREADS, QI = (MT * QCH + THREADS - 1) / THREADS;
    static constexpr int BUF = MT * (PROW + QROW);
    static constexpr int LDS = 2 * BUF + 4 * NT * 4;
    static_assert(WN * WK == 8, "8 waves");
};

STAMP_BUFFER(tnw)          // cycles per batch step of gemm_tnw_dma_kernel (STAMP_TNW, common.h)

template <typename QT, int VEC> struct TnwQRaw;
template <> struct TnwQRaw<bf16, 8> { bf16x8 v; };
template <int VEC> struct TnwQRaw<float, VEC> { float v[8]; };

template <class C, int PMODE, typename QT, int QVEC>
__global__ __launch_bounds__(512)
void gemm_tnw_kernel(const TnwArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* aux = (float*)(smem + 2 * C::BUF);            // [4][NT]: mean, c0, c0 c2 rstd, c0 c1 of this tile's P columns
    const TnBlock blk = tn_block((int)blockIdx.x, a.ntiles, a.nsplit, a.linear);
    const int tile = blk.tile, zz = blk.zz;
    if (zz < 0) return;
    const int tn = tile / a.ntk, tk = tile % a.ntk;
    const int n0 = tn * C::NT, k0 = tk * C::KT;
    const int M = a.M, N = a.N, K = a.K;
    const int m_begin = zz * a.rps, m_end = min(M, m_begin + a.rps);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wn = wid / C::WK, wk = wid % C::WK;

    if constexpr (PMODE == 1) {
        for (int c = tid; c < C::NT; c += C::THREADS) a.bn.column(n0 + c, n0 + c < N).store(aux, C::NT, c);
        tnw_bn_grads(a, n0, C::NT, zz, tk, tid, C::THREADS);
        __syncthreads();
    }

    f32x4 acc[C::PA][C::QB];
    float bsum[C::PA];
    tn_zero(acc, bsum);
    const bool do_bias = a.db != nullptr && tk == 0 && wk == 0;     // wave-uniform

    struct PRaw { bf16x8 d, y; };
    PRaw rp[C::PI];
    TnwQRaw<QT, QVEC> rq[C::QI];
    const int nt = (m_end - m_begin + C::MT - 1) / C::MT;
    const int ncap = ((N + 7) & ~7) - 8;                  // activation rows are padded to 8 elements
    const QT* qbase = (const QT*)a.q;

    // chunk c of a tile: row r = c / CH, chunk ch = c % CH; threads past the last chunk repeat it (same data to the same place)
    auto fetch = [&](int t) {
#pragma unroll
        for (int i = 0; i < C::PI; ++i) {
            const int c = min(tid + C::THREADS * i, C::MT * C::PCH - 1), r = c / C::PCH, ch = c % C::PCH;
            const unsigned row = (unsigned)min(min(m_begin + t * C::MT + r, m_end - 1), M - 1);
            const unsigned col = (unsigned)min(n0 + ch * 8, ncap);
            rp[i].d = *(const bf16x8*)(a.p + (row * a.ldp + col));
            if constexpr (PMODE == 1) rp[i].y = *(const bf16x8*)(a.py + (row * a.ldpy + col));
        }
#pragma unroll
        for (int i = 0; i < C::QI; ++i) {
            const int c = min(tid + C::THREADS * i, C::MT * C::QCH - 1), r = c / C::QCH, ch = c % C::QCH;
            const unsigned ro = (unsigned)min(min(m_begin + t * C::MT + r, m_end - 1), M - 1) * a.ldq;
            const int col = k0 + ch * 8;
            if constexpr (sizeof(QT) == 2) {
                rq[i].v = *(const bf16x8*)(qbase + (ro + (unsigned)min(col, ((K + 7) & ~7) - 8)));
            } else {
#pragma unroll
                for (int j = 0; j < 8; j += QVEC) VLoad<float, QVEC>::ld(qbase + (ro + (unsigned)min(col + j, K - QVEC)), &rq[i].v[j]);
            }
        }
    };
    // registers -> LDS.  P rows past the split become zeros (they drop out of the reduction); Q is stored unmasked: what lies
    // past K is finite and lands in output columns that are never stored, rows past the split meet the zeroed P rows.
    auto stage = [&](int t, int buf) {
        unsigned char* sP = smem + buf * C::BUF;
        unsigned char* sQ = sP + C::MT * C::PROW;
#pragma unroll
        for (int i = 0; i < C::PI; ++i) {
            const int c = min(tid + C::THREADS * i, C::MT * C::PCH - 1), r = c / C::PCH, ch = c % C::PCH;
            const bool ok = m_begin + t * C::MT + r < m_end;
            bf16x8 o;
            if constexpr (PMODE == 1) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float* ax = aux + ch * 8;
                    const float v = bn_bwd_apply(rp[i].d[e], rp[i].y[e], ax[e], ax[C::NT + e], ax[2 * C::NT + e], ax[3 * C::NT + e]);
                    o[e] = (bf16)(ok ? v : 0.f);
                }
            } else {
                const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
                o = ok ? rp[i].d : z;
            }
            *(bf16x8*)(sP + tn_chunk_off(r, ch, C::PROW)) = o;
        }
#pragma unroll
        for (int i = 0; i < C::QI; ++i) {
            const int c = min(tid + C::THREADS * i, C::MT * C::QCH - 1), r = c / C::QCH, ch = c % C::QCH;
            bf16x8 o;
            if constexpr (sizeof(QT) == 2) o = rq[i].v;
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (bf16)rq[i].v[e];
            }
            *(bf16x8*)(sQ + tn_chunk_off(r, ch, C::QROW)) = o;
        }
    };
    auto compute = [&](int buf) {
        const unsigned char* sP = smem + buf * C::BUF;
        const unsigned char* sQ = sP + C::MT * C::PROW;
        bf16x8 af[C::PA];
#pragma unroll
        for (int i = 0; i < C::PA; ++i) af[i] = tn_frag_bf16(sP, C::PROW, (wn * C::PA + i) * 16, lane);
#pragma unroll
        for (int j = 0; j < C::QB; ++j) {
            const bf16x8 bq = tn_frag_bf16(sQ, C::QROW, (wk * C::QB + j) * 16, lane);
#pragma unroll
            for (int i = 0; i < C::PA; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq, af[i], acc[i][j], 0, 0, 0);   // swapped: a lane holds 4 consecutive k of one n
        }
        if (do_bias) tn_db_add<bf16>(bsum, af);
    };

    fetch(0);
    stage(0, 0);
    if (nt > 1) fetch(1);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        compute(t & 1);
        if (t + 1 < nt) stage(t + 1, (t + 1) & 1);
        if (t + 2 < nt) fetch(t + 2);
        __syncthreads();
    }

    const int n_w = n0 + wn * C::PA * 16, k_w = k0 + wk * C::QB * 16;         // this wave's piece of the tile
    tn_store_slab(acc, a.slab, zz, n_w, k_w, N, K, lane);
    if (do_bias) tn_db_store(bsum, a.db, n_w, N, lane);
}

// ------------------------------------------------------------------------------------------
// LDS-DMA form: the RAW operand tiles (bf16 d and y, fp32 or bf16 Q) are moved global -> LDS by global_load_lds_dwordx4 into a
// two-stage ring and everything else happens on the way from LDS to the MFMA: P fragments are the transposed reads of d and y
// with the BatchNorm-backward correction applied per lane (a lane of a transposed fragment holds 8 batch rows of ONE column, so
// its four column constants live in registers), fp32 Q fragments are 8 plain ds_read_b32 (rows 8g .. 8g+7 of one column)
// converted in pairs.  No VGPR staging, no LDS write pass, no second copy of the tile: the register form above spent its step
// waiting for the loads of its single register set (68 KB per step and CU at the ~25 B/clk a CU ingests) and then converting.
// Swizzles are applied on the SOURCE side of the DMA (the LDS destination of a wave-instruction is lane-linear, 1 KB):
//   bf16 tiles: gemm_tn_tile.h's XOR of the 32-byte units of a 256-byte panel (tn_swz);
//   fp32 Q tile [32][KT]: rows of KT / 16 units of 64 bytes, unit u of row r stored at (u + (r >> 3)) mod units -- the four row
//   groups of a ds_read_b32 (16 lanes x 4 bytes each) then fall into four different 16-bank groups.
// Needs: M % 32 == 0 (every step a full tile), fp32 Q rows 16-byte aligned with K % 4 == 0.  The transfers are issued from
// assembly (lds_dma16, common.h) and waited for only by the counted s_waitcnt vmcnt(N) of the ring below.
// ------------------------------------------------------------------------------------------

template <class C, int PMODE, typename QT, int NSTAGE>
__global__ __launch_bounds__(512)
void gemm_tnw_dma_kernel(const TnwArgs a)
{
    constexpr bool QF = sizeof(QT) == 4;
    constexpr int QROWB = QF ? C::KT * 4 : C::QROW;
    constexpr int QUNITS = C::KT / 16;                     // fp32: 64-byte units per row
    constexpr int PBYTES = C::MT * C::PROW, QBYTES = C::MT * QROWB;
    constexpr int STAGE = PBYTES * (PMODE ? 2 : 1) + QBYTES;
    constexpr int PP = PBYTES / 1024, QP = QBYTES / 1024;  // 1 KB pieces per tile
    static_assert(PBYTES % 1024 == 0 && QBYTES % 1024 == 0, "whole DMA pieces");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef __attribute__((address_space(3))) void lds_void;
    typedef __attribute__((address_space(1))) const void gbl_void;

    const TnBlock blk = tn_block((int)blockIdx.x, a.ntiles, a.nsplit, a.linear);
    const int tile = blk.tile, zz = blk.zz;
    if (zz < 0) return;
    const int tn = tile / a.ntk, tk = tile % a.ntk;
    const int n0 = tn * C::NT, k0 = tk * C::KT;
    const int M = a.M, N = a.N, K = a.K;
    const int m_begin = zz * a.rps, m_end = min(M, m_begin + a.rps);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wv / C::WK, wk = wv % C::WK;
    const int li = lane & 15, g = lane >> 4;

    // per-lane BatchNorm-backward constants of the PA fragment columns this wave multiplies
    BnBwdConst bnc[C::PA];
    if constexpr (PMODE == 1) {
#pragma unroll
        for (int i = 0; i < C::PA; ++i) {
            const int col = n0 + (wn * C::PA + i) * 16 + li;
            bnc[i] = a.bn.column(col, col < N);
        }
        tnw_bn_grads(a, n0, C::NT, zz, tk, tid, C::THREADS);
    }

    // DMA source offsets (elements, relative to the first row of a step) of this lane's chunk in each piece this wave issues
    constexpr int PI = (PP + 7) / 8, QI = (QP + 7) / 8;
    unsigned psrc[PI], qsrc[QI];
    const int ncap = ((N + 7) & ~7) - 8;
#pragma unroll
    for (int i = 0; i < PI; ++i) {
        const int off = (wv + 8 * i) * 1024 + lane * 16;
        const int r = off / C::PROW, s_ = (off % C::PROW) >> 4;
        psrc[i] = (unsigned)r * a.ldp + (unsigned)min(n0 + ((s_ >> 4) * 16 + tn_swz(r, s_ & 15)) * 8, ncap);      // ldp == ldpy is checked by the host
    }
#pragma unroll
    for (int i = 0; i < QI; ++i) {
        const int off = (wv + 8 * i) * 1024 + lane * 16;
        const int r = off / QROWB, s_ = (off % QROWB) >> 4;
        if constexpr (QF) {
            int u = (s_ >> 2) - ((r >> 3) & 3);
            u += u < 0 ? QUNITS : 0;
            qsrc[i] = (unsigned)r * a.ldq + (unsigned)min(k0 + (u * 4 + (s_ & 3)) * 4, K - 4);
        } else qsrc[i] = (unsigned)r * a.ldq + (unsigned)min(k0 + ((s_ >> 4) * 16 + tn_swz(r, s_ & 15)) * 8, ((K + 7) & ~7) - 8);
    }
    auto issue = [&](int t, int st) {
        unsigned char* sD = smem + st * STAGE;
        unsigned char* sQ = sD + PBYTES * (PMODE ? 2 : 1);
        const long m0 = m_begin + (long)t * C::MT;
        const bf16* gd = a.p + m0 * a.ldp;
        const bf16* gy = a.py + m0 * a.ldpy;
        const QT* gq = (const QT*)a.q + m0 * a.ldq;
#pragma unroll
        for (int i = 0; i < PI; ++i) {
            const int p = wv + 8 * i;
            if (PP % 8 == 0 || p < PP) {
                lds_dma16(gd + psrc[i], lds_addr_of(sD + p * 1024));
                if constexpr (PMODE == 1) lds_dma16(gy + psrc[i], lds_addr_of(sD + PBYTES + p * 1024));
            }
        }
#pragma unroll
        for (int i = 0; i < QI; ++i) {
            const int p = wv + 8 * i;
            if (QP % 8 == 0 || p < QP) lds_dma16(gq + qsrc[i], lds_addr_of(sQ + p * 1024));
        }
    };

    f32x4 acc[C::PA][C::QB];
    float bsum[C::PA];
    tn_zero(acc, bsum);
    const bool do_bias = a.db != nullptr && tk == 0 && wk == 0;
    const int nt = (m_end - m_begin) / C::MT;

    auto compute = [&](int st) {
        const unsigned char* sD = smem + st * STAGE;
        const unsigned char* sQ = sD + PBYTES * (PMODE ? 2 : 1);
        bf16x8 af[C::PA];
#pragma unroll
        for (int i = 0; i < C::PA; ++i) {
            const bf16x8 d = tn_frag_bf16(sD, C::PROW, (wn * C::PA + i) * 16, lane);
            if constexpr (PMODE == 1) {
                const bf16x8 y = tn_frag_bf16(sD + PBYTES, C::PROW, (wn * C::PA + i) * 16, lane);
#pragma unroll
                for (int e = 0; e < 8; ++e) af[i][e] = (bf16)bn_bwd_apply(d[e], y[e], bnc[i].mean, bnc[i].c0, bnc[i].c2r, bnc[i].c01);
            } else af[i] = d;
        }
#pragma unroll
        for (int j = 0; j < C::QB; ++j) {
            bf16x8 bq;
            if constexpr (QF) {
                int u = wk * C::QB + j + g;
                u -= u >= QUNITS ? QUNITS : 0;
                const unsigned char* base = sQ + (8 * g) * QROWB + u * 64 + li * 4;
#pragma unroll
                for (int e = 0; e < 8; ++e) bq[e] = (bf16)(*(const float*)(base + e * QROWB));
            } else bq = tn_frag_bf16(sQ, QROWB, (wk * C::QB + j) * 16, lane);
#pragma unroll
            for (int i = 0; i < C::PA; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq, af[i], acc[i][j], 0, 0, 0);
        }
        if (do_bias) tn_db_add<bf16>(bsum, af);
    };

    // NSTAGE-deep ring, NSTAGE - 1 steps of DMA ahead of the MFMAs: with two stages a step lasted as long as ONE tile's trip
    // from HBM (issue -> landed, ~2-3 us under load), not as long as its arithmetic.  vmcnt counts this wave's pieces in issue
    // order: step t has landed when at most the pieces of the NSTAGE - 2 later steps are outstanding.
    constexpr int NP_LO = (PMODE ? 2 : 1) * (PP / 8) + QP / 8;                 // pieces per step of a wave (waves < PP % 8 / QP % 8 issue one more)
    const int extra = ((PP % 8 != 0 && wv < PP % 8) ? (PMODE ? 2 : 1) : 0) + ((QP % 8 != 0 && wv < QP % 8) ? 1 : 0);
    STAMP_ONLY(unsigned long long st_acc[8] = {}; STAMP_T(t_begin);)
#pragma unroll
    for (int s_ = 0; s_ < NSTAGE - 1; ++s_) if (s_ < nt) issue(s_, s_);
    // The ring is unrolled so that every stage address is a compile-time offset: with a run-time stage index hipcc cannot tell
    // the LDS-DMA destination from the stage the fragment reads come from and puts s_waitcnt vmcnt(0) in front of the first
    // ds_read of a step, i.e. right behind the DMA issue -- the whole trip from HBM then sits inside every step.
    for (int t0 = 0; t0 < nt; t0 += NSTAGE) {
#pragma unroll
        for (int u = 0; u < NSTAGE; ++u) {
            const int t = t0 + u;
            if (t >= nt) break;
            STAMP_T(w0);
            if (NSTAGE > 2 && t + NSTAGE - 2 < nt) {             // steady state: NSTAGE - 2 later steps may still be in flight
                if (extra == 0) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NSTAGE - 2) * NP_LO) : "memory");
                else if (extra == 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NSTAGE - 2) * (NP_LO + 1)) : "memory");
                else if (extra == 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NSTAGE - 2) * (NP_LO + 2)) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NSTAGE - 2) * (NP_LO + 3)) : "memory");
            } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            STAMP_T(w1);
            __builtin_amdgcn_s_barrier();                        // everybody's pieces of step t have landed; nobody still reads stage t - 1
            asm volatile("" ::: "memory");
            STAMP_T(w2);
            if (t + NSTAGE - 1 < nt) issue(t + NSTAGE - 1, (u + NSTAGE - 1) % NSTAGE);      // the stage step t - 1 was read from
            STAMP_T(w3);
            compute(u);
            STAMP_ONLY(asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"));
            STAMP_T(w4);
            STAMP_ADD(0, w1 - w0); STAMP_ADD(1, w2 - w1); STAMP_ADD(2, w3 - w2); STAMP_ADD(3, w4 - w3);
        }
    }
    STAMP_T(t_loop_end);

    const int n_w = n0 + wn * C::PA * 16, k_w = k0 + wk * C::QB * 16;         // this wave's piece of the tile
    tn_store_slab(acc, a.slab, zz, n_w, k_w, N, K, lane);
    if (do_bias) tn_db_store(bsum, a.db, n_w, N, lane);
    STAMP_T(t_end);
    STAMP_ADD(4, nt); STAMP_ADD(5, 1); STAMP_ADD(6, t_end - t_begin); STAMP_ADD(7, t_end - t_loop_end);
    STAMP_ONLY(if (tid == 0 && (blockIdx.x & 7) == 3) stamp_flush(stamps_tnw, st_acc));
}

typedef TnwCfg<4, 4, 2, 9> CfgA;        // 256 x 288
typedef TnwCfg<2, 4, 4, 7> CfgB;        // 128 x 448

// one launcher for both forms: the kernel and its dynamic LDS
template <auto Kernel>
static int tnw_go(const TnwArgs& w, int lds, hipStream_t st) {
    return launch_lds<Kernel>(dim3(tn_grid(w.nsplit, w.ntiles, w.linear)), dim3(512), lds, st, w);
}
template <class C, int PMODE, typename QT, int NSTAGE>
static int tnw_dma_launch(const TnwArgs& w, hipStream_t st) {
    constexpr int LDS = NSTAGE * (C::MT * C::PROW * (PMODE ? 2 : 1) + C::MT * (sizeof(QT) == 4 ? C::KT * 4 : C::QROW));      // NSTAGE stages of the kernel's STAGE bytes
    return tnw_go<gemm_tnw_dma_kernel<C, PMODE, QT, NSTAGE>>(w, LDS, st);
}

// Returns 0 after launching the GEMM (the caller then runs the slab reduce over *nsplit_out splits), > 0 on a launch error,
// NOT_TAKEN when the problem is not one of the wide kernel's.
int launch_tn_wide(const mmvae_gemm_tn_args* a, hipStream_t st, int* nsplit_out) {
    constexpr int NA = NOT_TAKEN;
    if (!g_tuning.tn_wide_on || a->prec != MMVAE_PREC_BF16 || a->p_dtype != MMVAE_BF16 || a->q_prologue != MMVAE_PRO_NONE || a->nsplit > 0) return NA;
    if (a->M < 8192 || !a->slab || a->N < 128 || a->K < 256) return NA;
    const int pmode = a->p_prologue == MMVAE_PRO_BN_BWD_APPLY ? 1 : 0;
    if (a->p_prologue != MMVAE_PRO_NONE && !pmode) return NA;
    if (a->ldp % 8 || ((uintptr_t)a->p & 15)) return NA;
    const bool fin = pmode && !a->p_coef;                 // mmvae_bn_bwd_finalize folded in
    if (pmode && (!a->p_y || !a->p_mean || !a->p_rstd || a->ld_py % 8 || ((uintptr_t)a->p_y & 15) || a->N % 8)) return NA;
    if (fin && (!a->p_sum_d || !a->p_sum_dx || !a->p_gamma || !a->p_dgamma || !a->p_dbeta)) return NA;
    int qkind;                                             // 0 bf16, 4 / 2: fp32 in vectors of 4 / 2 (no form reads single floats)
    if (a->q_dtype == MMVAE_BF16) { if (a->ldq % 8 || ((uintptr_t)a->q & 15)) return NA; qkind = 0; }
    else { qkind = vec_width(a->ldq, a->K, a->q); if (qkind == 1) return NA; }
    // instantiated combinations: an fp32 Q (the input batch of the first encoder layers) with a BatchNorm-corrected bf16 P (the bench
    // widths) or a plain bf16 P (very wide inputs, where the engine applies the correction in a pass of its own: hundreds of K tiles would
    // each redo it).  Plain bf16 x bf16 problems (last decoder layers) were measured on this kernel too (3-stage ring): 57-59 us against
    // 58 us of gemm_tn.hip's 128 x 128 DMA form with two workgroups per CU, plus a larger slab reduce -- they stay there.
    if (qkind == 0) {
        // bf16 x bf16 with a very large output (the decoders' last layers at the scaled widths: 27 000 x 512): 128 x 128 tiles re-ingest
        // P four times and Q 211 times; at the bench widths gemm_tn.hip's form with two workgroups per CU is as fast (above)
        if (pmode || a->M % 32 || (long)a->N * a->K < (4L << 20)) return NA;
    } else if (!pmode && (qkind != 4 || a->M % 32)) return NA;   // plain P: LDS-DMA forms only
    auto padded = [&](int nt_, int kt_) { return (long)((a->N + nt_ - 1) / nt_ * nt_) * ((a->K + kt_ - 1) / kt_ * kt_); };
    const int cfg = qkind == 0 ? 0 : (a->N <= 128 || padded(CfgB::NT, CfgB::KT) < padded(CfgA::NT, CfgA::KT)) ? 1 : 0;       // least padded output
    // 256 x 288 tiles run the LDS-DMA form: whole 32-row steps, 16-byte aligned fp32 rows, d and y with one row stride
    if (pmode && cfg == 0 && (qkind != 4 || a->M % 32 || a->ldp != a->ld_py)) return NA;
    const int NT = cfg == 0 ? CfgA::NT : CfgB::NT, KT = cfg == 0 ? CfgA::KT : CfgB::KT;
    TnwArgs w;
    w.ntk = (a->K + KT - 1) / KT;
    w.ntiles = w.ntk * ((a->N + NT - 1) / NT);
    if (w.ntiles > (pmode ? 32 : 4096)) return NA;         // corrected P: every K tile redoes the correction -- the 128 x 128 kernel's case
    const SplitPlan sp = plan_splits(a->M, 32, 0, w.ntiles, NUM_CU);      // one workgroup per CU
    const int nsplit = sp.nsplit, rps = sp.rps;
    if ((long)nsplit * a->N * a->K > a->slab_elems) return NA;
    if (pmode && nsplit < 2) return NA;
    w.nsplit = nsplit; w.rps = rps; w.linear = nsplit < 8 ? 1 : 0;
    w.p = (const bf16*)a->p; w.ldp = (unsigned)a->ldp; w.py = (const bf16*)a->p_y; w.ldpy = (unsigned)a->ld_py;
    w.bn = BnBwdCols{a->p_mean, a->p_rstd, a->p_coef, a->N, a->p_sum_d, a->p_sum_dx, a->p_gamma, a->p_eval_mode, a->M};
    w.dgamma = a->p_dgamma; w.dbeta = a->p_dbeta;
    w.q = a->q; w.ldq = (unsigned)a->ldq; w.M = a->M; w.N = a->N; w.K = a->K; w.slab = a->slab; w.db = a->db;
    *nsplit_out = nsplit;
    if (qkind == 0) return tnw_dma_launch<CfgA, 0, bf16, 3>(w, st);
    if (!pmode) return cfg == 0 ? tnw_dma_launch<CfgA, 0, float, 3>(w, st) : tnw_dma_launch<CfgB, 0, float, 2>(w, st);
    if (cfg == 0) return tnw_dma_launch<CfgA, 1, float, 2>(w, st);
    // 128 x 448 tiles (EncoderA.L0: K = 782, fp32 rows only 8-byte aligned -- 16-byte LDS-DMA pieces from such rows delivered wrong
    // data): the register form
    return qkind == 4 ? tnw_go<gemm_tnw_kernel<CfgB, 1, float, 4>>(w, CfgB::LDS, st) : tnw_go<gemm_tnw_kernel<CfgB, 1, float, 2>>(w, CfgB::LDS, st);
}

}  // namespace mm
