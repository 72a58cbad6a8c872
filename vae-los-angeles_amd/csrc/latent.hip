// The latent path of the forward in ONE launch (gfx950): mmvae_latent_fwd (include/mmvae_hip.h lists the limits).
//
// Replaces, on the MultiModalVAE path (reference file:line): the fc_mu | fc_logvar heads of EncoderA / EncoderB behind the last
// BatchNorm1d + ReLU + Dropout (src/models/encoders.py:14-19, 36-41), mean fusion and reparameterisation (src/models/vae.py:65-73,
// 11-15) and the first Linear + ReLU of every decoder (src/models/decoders.py:13-14, 27-28, 44-45) -- four launches that each stream a
// few tens of MB, hand their result to the next through HBM and do almost no arithmetic (K = 128 / 256 / 20).
//
// One persistent workgroup of 8 waves per CU.  The three weight operands (heads 48 x K, stems N x 32), the two BatchNorm tables, the
// biases and the EncoderC table stay in LDS for the whole launch.  A wave owns 16-row slabs and carries each from y to h0:
//   * y (+ keep bytes), eps and site of the slab are loaded straight in MFMA fragment layout (lane (li, lg): row li, k = 32 j + 8 lg ..),
//     through SrcBnReluDrop (gemm_src.h): the arithmetic, the table and the folded BatchNorm finalisation of mmvae_gemm_nt's prologue;
//     the NEXT slab's loads are issued as soon as the registers are free (behind the heads' MFMAs), so they fly under the slab's work;
//   * heads: 3 x K / 32 MFMAs per encoder with the operands swapped as in the tile kernels (gemm_nt_epi.h), K ascending, bias in fp32;
//     the encoders' sums go through a wave-private LDS image to the fusion's element order (mu_l and logvar_l of a row meet in a lane);
//   * fusion + reparameterisation (fuse_math.h): mu / logvar leave as contiguous fp32, z as bf16 rows from a wave-private LDS image that
//     is also the stems' MFMA operand (pad columns are zero there and in HBM);
//   * stems: one MFMA per 16 columns (K <= 32), two column blocks of 32 interleaved so that a lane owns 8 consecutive columns, halves
//     swapped between lanes li and li ^ 8 (DPP) so that every store instruction writes whole 128-byte lines.
// No workgroup barrier after the set-up: the waves never wait for each other.
#include "common.h"
#include "mmvae_hip.h"
#include "gemm_src.h"
#include "fuse_math.h"
#include "wave_slab.h"

namespace mm {

constexpr int LAT_WAVES = 8, LAT_THREADS = 64 * LAT_WAVES;
constexpr int LAT_NK = 8;                         // MFMA K steps per encoder: K <= 256
constexpr int LAT_HN = 48;                        // head columns in LDS: three MFMA tiles, 2L <= 48
constexpr int LAT_FU = LAT_HN / 2 * 16 / 64;      // fusion elements per lane and slab: 16 rows x L <= 24
constexpr int LAT_NS = 448;                       // stem columns
constexpr int LAT_MAXTAB = 1024;                  // floats of the EncoderC table
constexpr int LAT_WROW = LAT_NK * 64 + 16;        // heads weight row (K <= 256 bf16) + the pad chunk of every LDS row (wave_slab.h)
constexpr int LAT_SROW = 64 + 16;                 // stem weight row and z row (32 bf16)
constexpr int LAT_SUMLD = 52;                     // floats per row of the heads image
constexpr int LAT_OFF_WS = 2 * LAT_HN * LAT_WROW;
constexpr int LAT_OFF_AUX = LAT_OFF_WS + LAT_NS * LAT_SROW;          // [2][1024] floats: SrcBnReluDrop's tables
constexpr int LAT_OFF_BIAS = LAT_OFF_AUX + 2 * 4096;                 // [2][48] heads + [448] stems
constexpr int LAT_OFF_TAB = LAT_OFF_BIAS + (2 * LAT_HN + LAT_NS) * 4;
constexpr int LAT_OFF_SCR = LAT_OFF_TAB + LAT_MAXTAB * 4;
constexpr int LAT_SCR_Z = 16 * LAT_SUMLD * 4;                        // per wave: heads image, then the z image
constexpr int LAT_SCR = LAT_SCR_Z + 16 * LAT_SROW;
constexpr int LAT_LDS = LAT_OFF_SCR + LAT_WAVES * LAT_SCR;           // 135 KB

struct LatEnc { SrcBnReluDrop<bf16> src; const bf16* w; long ldw; const float* bias; int nk; };      // nk = K / 32; 0: absent
struct LatArgs {
    LatEnc e[2];
    int B, L, n_mod, S;
    const float* table; const long long* site; const float* eps; float* mu; float* logvar;
    bf16* z; long ldz;
    const bf16* ws; long ldws; const float* bs; int ns;
    bf16* h0; long ldh0;
    int nslabs;
};

// DET: the autoencoders' deterministic form (mmvae_ae_latent_fwd) -- ONE head of width L per encoder (the staged head rows >= L are
// zero), the table is [S][L], the fusion is fuse_mean_elem: no eps is read, no logvar written, a.mu receives the latent.
template <bool DET>
__global__ __launch_bounds__(LAT_THREADS) void latent_fwd_kernel(const LatArgs a) {
    typedef SrcBnReluDrop<bf16>::Raw Raw;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    float* const aux = (float*)(smem + LAT_OFF_AUX);
    float* const sbias = (float*)(smem + LAT_OFF_BIAS);
    float* const stab = (float*)(smem + LAT_OFF_TAB);
    unsigned char* const scr = smem + LAT_OFF_SCR + wid * LAT_SCR;
    float* const ssum = (float*)scr;
    unsigned char* const sz = scr + LAT_SCR_Z;
    const int L = a.L, L2 = DET ? a.L : 2 * a.L;
    const bool any_enc = a.e[0].nk + a.e[1].nk > 0;

    // slab-independent lane constants: element lane + 64 i of the slab's [16][L] block is (row fr[i], latent fl[i])
    int fr[LAT_FU], fl[LAT_FU];
#pragma unroll
    for (int i = 0; i < LAT_FU; ++i) { const int x = lane + 64 * i; fr[i] = x / L; fl[i] = x - fr[i] * L; }
    const int zcpr = (int)(a.ldz >> 3), zr = lane / zcpr, zc = lane - zr * zcpr;      // 16-byte pieces of the z rows
    const float inv_n = 1.f / (float)a.n_mod;
    const int total = a.B * L;

    Raw raw[2][LAT_NK];
    float eps_r[LAT_FU] = {};
    long long site_r[LAT_FU] = {};
    auto fetch = [&](int slab) __attribute__((always_inline)) {
        const int row = slab * 16 + li;
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int j = 0; j < LAT_NK; ++j)
                if (j < a.e[e].nk) a.e[e].src.fetch(raw[e][j], row, 32 * j + 8 * lg);
        if constexpr (!DET) {
#pragma unroll
            for (int i = 0; i < LAT_FU; ++i) {
                const int idx = min(slab * 16 * L + lane + 64 * i, total - 1);          // clamped: the loads always issue
                eps_r[i] = a.eps[idx];
            }
        }
        // a kernel-uniform branch around loads only: an else-side that writes the same registers makes the compiler wait for every load
        // in flight right here (gemm_src.h)
        if (a.table) {
#pragma unroll
            for (int i = 0; i < LAT_FU; ++i) site_r[i] = a.site[min(slab * 16 + fr[i], a.B - 1)];
        }
    };

    const int nw = gridDim.x * LAT_WAVES;
    int slab = blockIdx.x * LAT_WAVES + wid;
    if (slab < a.nslabs) fetch(slab);          // the first slab's loads fly under the set-up: they depend on nothing in LDS

    // ---------------------------------------------------------------------------------- once per workgroup
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        if (a.e[e].nk == 0) continue;
        // scale / shift tables (+ the folded finalisation).  SrcBnReluDrop::init strides by NTHREADS and lays its table out as
        // [512] scale | [512] shift: 1024 floats per encoder (LAT_OFF_AUX), and K <= 256 <= NTHREADS is one column per thread
        static_assert(NTHREADS <= LAT_THREADS && 32 * LAT_NK <= 512, "SrcBnReluDrop's table: 512 columns, filled by NTHREADS threads");
        if (tid < NTHREADS) a.e[e].src.init(aux + e * 1024, tid, 0);
        stage_rows<LAT_THREADS>(smem + e * LAT_HN * LAT_WROW, LAT_WROW, a.e[e].w, a.e[e].ldw, LAT_HN, a.e[e].nk * 4, tid, EpiCols<false>::wrow);
        if (tid < LAT_HN) sbias[e * LAT_HN + tid] = (a.e[e].bias && tid < L2) ? a.e[e].bias[tid] : 0.f;
    }
    // every 64-column block of the stem weights in EpiCols<true>'s row order: a lane's 8 accumulators of a tile pair are 8 consecutive columns
    stage_rows<LAT_THREADS>(smem + LAT_OFF_WS, LAT_SROW, a.ws, a.ldws, a.ns, 4, tid, [](int x) { return (x & ~63) + EpiCols<true>::wrow(x & 63); });
    for (int c = tid; c < a.ns; c += LAT_THREADS) sbias[2 * LAT_HN + c] = a.bs ? a.bs[c] : 0.f;
    if (a.table) for (int i = tid; i < a.S * L2; i += LAT_THREADS) stab[i] = a.table[i];
    for (int i = lane; i < 16 * LAT_SROW / 16; i += 64) ((uint4*)sz)[i] = uint4{0u, 0u, 0u, 0u};      // z pads (k >= L) stay zero
    __syncthreads();

    for (; slab < a.nslabs; slab += nw) {
        // ------------------------------------------------------------------------------ heads: operand prologue + MFMAs, K ascending
        f32x4 hs[3];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (a.e[e].nk == 0) continue;
            f32x4 acc[3];
#pragma unroll
            for (int n = 0; n < 3; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < LAT_NK; ++j) {
                if (j >= a.e[e].nk) break;
                Chunk<bf16> o;
                a.e[e].src.finish_fast(raw[e][j], 32 * j + 8 * lg, o, aux + e * 1024);
#pragma unroll
                for (int n = 0; n < 3; ++n) {
                    const bf16x8 wf = *(const bf16x8*)(smem + (e * LAT_HN + 16 * n + li) * LAT_WROW + (4 * j + lg) * 16);
                    Mma<bf16>::mma(acc[n], wf, o.v);                        // swapped operands: the lane holds row li, columns 16 n + 4 lg ..
                }
            }
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const f32x4 h = acc[n] + *(const f32x4*)(sbias + e * LAT_HN + 16 * n + 4 * lg);
                hs[n] = (e == 1 && a.e[0].nk) ? hs[n] + h : h;             // the fusion's order: a, then b
            }
        }
        if (any_enc) {
#pragma unroll
            for (int n = 0; n < 3; ++n) *(f32x4*)(ssum + li * LAT_SUMLD + 16 * n + 4 * lg) = hs[n];
        }
        // the slab's operands are consumed: the next slab's loads fly under the rest of this one
        float ep[LAT_FU];
        long long st[LAT_FU];
#pragma unroll
        for (int i = 0; i < LAT_FU; ++i) { ep[i] = eps_r[i]; st[i] = site_r[i]; }
        if (slab + nw < a.nslabs) fetch(slab + nw);
        wave_lds_sync();

        // ------------------------------------------------------------------------------ mean fusion + reparameterisation
#pragma unroll
        for (int i = 0; i < LAT_FU; ++i) {
            if (lane + 64 * i >= 16 * L) break;
            const int r = fr[i], l = fl[i];
            if constexpr (DET) {
                float sum = 0.f;
                bool first = true;                                          // the first term present is taken as it is (a -0 stays -0)
                if (any_enc) { sum = ssum[r * LAT_SUMLD + l]; first = false; }
                if (a.table) {
                    const long long s = st[i];
                    const bool ok = s >= 0 && s < a.S;
                    const float t = ok ? stab[(int)s * L + l] : __builtin_nanf("");
                    sum = first ? t : sum + t;
                }
                const float m = fuse_mean_elem(sum, a.n_mod, inv_n);
                const int idx = slab * 16 * L + lane + 64 * i;
                if (idx < total) a.mu[idx] = m;
                ((bf16*)sz)[r * (LAT_SROW / 2) + l] = (bf16)m;
                continue;
            }
            float mu = 0.f, lv = 0.f;
            if (any_enc) { mu += ssum[r * LAT_SUMLD + l]; lv += ssum[r * LAT_SUMLD + L + l]; }
            if (a.table) {
                const long long s = st[i];                                  // out of range: the row is poisoned (fuse_fwd_kernel)
                const bool ok = s >= 0 && s < a.S;
                const int sc = ok ? (int)s : 0;
                const float bad = ok ? 0.f : __builtin_nanf("");
                mu += stab[sc * L2 + l] + bad; lv += stab[sc * L2 + L + l] + bad;
            }
            const float zf = fuse_reparam_elem(mu, lv, a.n_mod, inv_n, ep[i]);
            const int idx = slab * 16 * L + lane + 64 * i;
            if (idx < total) { a.mu[idx] = mu; a.logvar[idx] = lv; }
            ((bf16*)sz)[r * (LAT_SROW / 2) + l] = (bf16)zf;
        }
        wave_lds_sync();
        if (lane < 16 * zcpr && slab * 16 + zr < a.B)
            *(uint4*)(a.z + (long)(slab * 16 + zr) * a.ldz + zc * 8) = *(const uint4*)(sz + zr * LAT_SROW + zc * 16);

        // ------------------------------------------------------------------------------ stems
        const bf16x8 zf8 = *(const bf16x8*)(sz + li * LAT_SROW + lg * 16);
        const bool lowl = li < 8;
        const int rbase = slab * 16 + (li & 7);
        bf16* const crow = line_col(a.h0 + (long)rbase * a.ldh0, li, lg);
        const bool ok0 = rbase < a.B, ok1 = rbase + 8 < a.B;
        for (int p = 0; p < (a.ns >> 6); ++p) {
            f32x4 acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bf16x8 wf = *(const bf16x8*)(smem + LAT_OFF_WS + (64 * p + 16 * q + li) * LAT_SROW + lg * 16);
                acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                Mma<bf16>::mma(acc[q], wf, zf8);
            }
            uint32_t pk[2][4];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float* bp = sbias + 2 * LAT_HN + 64 * p + 32 * h + 8 * lg;
                const f32x4 b0 = *(const f32x4*)bp, b1 = *(const f32x4*)(bp + 4);
                const f32x4 x0 = acc[2 * h] + b0, x1 = acc[2 * h + 1] + b1;
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const f32x4 x = qd < 2 ? x0 : x1;
                    const bf16x2 t = {(bf16)fmaxf(x[2 * (qd & 1)], 0.f), (bf16)fmaxf(x[2 * (qd & 1) + 1], 0.f)};
                    pk[h][qd] = __builtin_bit_cast(uint32_t, t);
                }
            }
            SWAP_HALVES(pk, lowl, st0, st1);
            if (ok0) *(uint4*)(crow + 64 * p) = uint4{st0[0], st0[1], st0[2], st0[3]};
            if (ok1) *(uint4*)(crow + 8 * a.ldh0 + 64 * p) = uint4{st1[0], st1[1], st1[2], st1[3]};
        }
        wave_lds_sync();                              // the images are free for the next slab
    }
}

// the operand source of one encoder, or why not
static int lat_enc(const mmvae_latent_enc& e, int B, LatEnc& o) {
    o = LatEnc{};
    if (!e.y) return 0;
    const mmvae_bn_finalize_args* f = (const mmvae_bn_finalize_args*)e.finalize;
    if (e.K < 32 || e.K % 32 || e.K > 32 * LAT_NK || e.ldy % 8 || e.ldy < e.K || ((uintptr_t)e.y & 15)) return MMVAE_ERR_ARG;
    if (!e.w || e.ldw % 64 || e.ldw < e.K || ((uintptr_t)e.w & 15)) return MMVAE_ERR_ARG;
    if (!f && (!e.scale || !e.shift)) return MMVAE_ERR_ARG;
    if (f && (f->N != e.K || f->M != B || B < 2 || !f->sum || !f->sumsq || !f->gamma || !f->beta || !f->mean || !f->rstd || !f->scale || !f->shift))
        return MMVAE_ERR_ARG;
    if (e.mask && (e.ld_mask % 8 || e.ld_mask < e.K || ((uintptr_t)e.mask & 7))) return MMVAE_ERR_ARG;
    const long lim = 1L << 32;                       // 32-bit element offsets in SrcBnReluDrop::fetch
    if ((long)B * e.ldy * 2 >= lim || (e.mask && (long)B * e.ld_mask >= lim)) return MMVAE_ERR_ARG;
    o.src = SrcBnReluDrop<bf16>{(const bf16*)e.y, e.ldy, B, e.K, e.scale, e.shift, e.mask, e.ld_mask, e.inv_keep, bn_fin_from(f)};
    o.w = (const bf16*)e.w; o.ldw = e.ldw; o.bias = e.bias; o.nk = e.K / 32;
    return 0;
}

// What mmvae_latent_fwd (DET = false) and mmvae_ae_latent_fwd (DET = true) refuse alike, the LatArgs fields both fill alike, and the launch.
// own_ok: the entry point's own requirements (its output pointers, the limits that depend on its head count), tested here behind the
// precision so that a wrong precision is MMVAE_ERR_DTYPE whatever else is wrong; k arrives with the entry point's own fields set.
// enc_b: nullptr where the entry point has one encoder.
template <bool DET, typename A>
static int latent_check_launch(const A& a, bool own_ok, const mmvae_latent_enc& enc_a, const mmvae_latent_enc* enc_b, LatArgs& k, void* stream) {
    if (a.prec != MMVAE_PREC_BF16) return MMVAE_ERR_DTYPE;
    if (a.B <= 0 || a.L <= 0 || (long)a.B * a.L >= (1L << 31) || !own_ok) return MMVAE_ERR_ARG;
    if (!a.z || !a.w_stem || !a.h0) return MMVAE_ERR_ARG;
    const int present = (enc_a.y != nullptr) + (enc_b && enc_b->y != nullptr) + (a.table != nullptr);
    if (present == 0 || present != a.n_mod) return MMVAE_ERR_ARG;
    if (a.table && (!a.site || a.S <= 0)) return MMVAE_ERR_ARG;
    if (a.ldz % 8 || a.ldz < a.L || a.ldz > 32 || ((uintptr_t)a.z & 15)) return MMVAE_ERR_ARG;
    if (a.N_stem < 64 || a.N_stem % 64 || a.N_stem > LAT_NS || a.ldw_stem % 64 || a.ldw_stem < 32 || ((uintptr_t)a.w_stem & 15)) return MMVAE_ERR_ARG;
    if (a.ldh0 % 64 || a.ldh0 < a.N_stem || ((uintptr_t)a.h0 & 127) || (long)a.B * a.ldh0 * 2 >= (1L << 32)) return MMVAE_ERR_ARG;
    { const int rc = lat_enc(enc_a, a.B, k.e[0]); if (rc) return rc; }
    if (enc_b) { const int rc = lat_enc(*enc_b, a.B, k.e[1]); if (rc) return rc; }
    k.B = a.B; k.L = a.L; k.n_mod = a.n_mod; k.S = a.S;
    k.table = a.table; k.site = (const long long*)a.site;
    k.z = (bf16*)a.z; k.ldz = a.ldz;
    k.ws = (const bf16*)a.w_stem; k.ldws = a.ldw_stem; k.bs = a.bias_stem; k.ns = a.N_stem;
    k.h0 = (bf16*)a.h0; k.ldh0 = a.ldh0;
    k.nslabs = (a.B + 15) / 16;
    return launch_lds<latent_fwd_kernel<DET>>(dim3(persistent_grid(k.nslabs, LAT_WAVES)), dim3(LAT_THREADS), LAT_LDS, (hipStream_t)stream, k);
}

}  // namespace mm

extern "C" int mmvae_latent_fwd(const mmvae_latent_fwd_args* a, void* stream) {
    using namespace mm;
    if (!a || !g_tuning.latent_on) return MMVAE_ERR_ARG;
    const bool own_ok = 2 * a->L <= LAT_HN && a->eps && a->mu && a->logvar && (!a->table || (long)a->S * 2 * a->L <= LAT_MAXTAB);
    LatArgs k{};
    k.eps = a->eps; k.mu = a->mu; k.logvar = a->logvar;
    return latent_check_launch<false>(*a, own_ok, a->enc_a, &a->enc_b, k, stream);
}

extern "C" int mmvae_ae_latent_fwd(const mmvae_ae_latent_fwd_args* a, void* stream) {
    using namespace mm;
    if (!a || !g_tuning.ae_latent_on) return MMVAE_ERR_ARG;
    const bool own_ok = a->L <= LAT_HN / 2 && a->latent && (!a->table || (long)a->S * a->L <= LAT_MAXTAB);
    LatArgs k{};
    k.mu = a->latent;
    return latent_check_launch<true>(*a, own_ok, a->enc, nullptr, k, stream);
}
