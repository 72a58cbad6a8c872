// NT GEMM whose epilogue reduces every group of G consecutive output rows to a mean and a standard deviation ON CHIP:
//   x[b G + g][j] = act(sum_k a[b G + g][k] w[j][k] + bias[j]),   mean[b][j] = (1/G) sum_g x,   std[b][j] = sqrt(sum_g (x - mean)^2 / (G - 1))
// -- the decoder's last Linear of a multiple-draw / all-site reconstruction (mmvae/reconstruct.py: G = draws x sites rows per
// sample).  The B G x N fp32 output that mmvae_gemm_nt would store, and a reduction would read back, never reaches HBM.
//
// Tiling: a 128-row tile holds GPT = floor(128 / G) WHOLE groups (rows GPT G .. 127 are idle: they are multiplied and never read),
// 128 columns, 256 threads (4 waves, 2 x 2, 64 x 64 each), the register-staged double-buffered K loop of gemm_nt.hip's short-K form
// (K <= 512: at most 8 steps) over the shared operand source (gemm_src.h) with the swapped-operand accumulator layout (wave_slab.h).
// The tile, after bias and activation, goes to LDS as fp32 (over the staging buffers, which are dead by then); thread (column c,
// half h) then walks column c of groups h, h + 2, ... in ascending g, first for the sum, then for the squared deviations from the
// mean: a fixed order, no atomics, and never sum-of-squares minus square-of-sum.
#include "common.h"
#include "mmvae_hip.h"
#include "gemm_src.h"
#include "wave_slab.h"

namespace mm {

constexpr int GM_LDX = TILE + 4;                                   // floats per row of the fp32 tile image: 16-byte rows, and the 16 lanes
                                                                   // of a ds_write_b128 pass (rows li, one column quad) cover all 64 banks
constexpr int GM_STAGE = 2 * 2 * TILE * ROW_BYTES;                 // double-buffered { A [128][128 B] + W [128][128 B] }
constexpr int GM_IMAGE = TILE * GM_LDX * 4;
constexpr int GM_BIAS = GM_IMAGE > GM_STAGE ? GM_IMAGE : GM_STAGE; // the tile's 128 bias values sit behind both
constexpr int GM_LDS = GM_BIAS + TILE * 4;                         // 68 096 bytes: two workgroups per CU

__device__ __forceinline__ int gm_swz(int row, int chunk) { return row * ROW_BYTES + ((chunk ^ (row & 7)) << 4); }

struct GmArgs {
    SrcPlain<bf16, bf16, 8> src;          // a: [B G][lda] bf16, M = B G
    const bf16* w; long ldw;
    const float* bias;
    float* mean; long ld_mean;
    float* std; long ld_std;              // nullptr: no standard deviation
    int B, G, N, K, act, gpt, gx, gy;     // gpt groups per row tile, gx row tiles, gy column tiles
};

template <bool SIGMOID>
__global__ __launch_bounds__(NTHREADS, 2)
void group_moments_kernel(GmArgs p)
{
    constexpr int BK = ROW_BYTES / 2, A_PER = 4;
    typedef Mma<bf16>::frag frag;
    typedef SrcPlain<bf16, bf16, 8> Src;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* xt = (float*)smem;
    float* sbias = (float*)(smem + GM_BIAS);

    // all column tiles of a row tile on one XCD (shared L2) in adjacent dispatch slots, as gemm_nt.hip
    const int Lb = blockIdx.x, slot = Lb >> 3;
    const int ct = slot % p.gy, rt = (slot / p.gy) * 8 + (Lb & 7);
    if (rt >= p.gx) return;
    const int row0 = rt * p.gpt * p.G, col0 = ct * TILE;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
    const int li = lane & 15, lg = lane >> 4;

    if (tid < TILE) sbias[tid] = (p.bias && col0 + tid < p.N) ? p.bias[col0 + tid] : 0.f;     // visible after the K loop's barriers

    f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    Src::Raw ra0[A_PER], ra1[A_PER];
    Chunk<bf16> rb0[4], rb1[4];
    const int nk = p.K / BK;                                      // 1 .. 8

    // rows past B G are clamped into the operand by the source; W has ceil128(N) rows and ldw >= ceil64(K) columns
    auto fetch = [&](Src::Raw (&ra)[A_PER], Chunk<bf16> (&rb)[4], int kt) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int c = tid + NTHREADS * i, r = c >> 3, ch = c & 7;
            p.src.fetch(ra[i], row0 + r, kt * BK + ch * 8);
            rb[i].v = *(const bf16x8*)(p.w + ((unsigned)(col0 + r) * (unsigned)p.ldw + (unsigned)(kt * BK + ch * 8)));
        }
    };
    auto stage = [&](Src::Raw (&ra)[A_PER], Chunk<bf16> (&rb)[4], int kt, int buf) {
        unsigned char* sA = smem + buf * (2 * TILE * ROW_BYTES);
        unsigned char* sB = sA + TILE * ROW_BYTES;
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int c = tid + NTHREADS * i, r = c >> 3, ch = c & 7;
            Chunk<bf16> o;
            p.src.finish_fast(ra[i], kt * BK + ch * 8, o, nullptr);           // K % 64 == 0: no row ends inside a chunk
            *(bf16x8*)(sA + gm_swz(r, ch)) = o.v;
            *(bf16x8*)(sB + gm_swz(r, ch)) = rb[i].v;
        }
    };
    frag fa[4], fb[4];
    auto rd = [&](int buf, int s) {
        const unsigned char* sA = smem + buf * (2 * TILE * ROW_BYTES);
        const unsigned char* sB = sA + TILE * ROW_BYTES;
        const int ch = s * 4 + lg;
#pragma unroll
        for (int m = 0; m < 4; ++m) fa[m] = *(const frag*)(sA + gm_swz(wr * 64 + m * 16 + li, ch));
#pragma unroll
        for (int n = 0; n < 4; ++n) fb[n] = *(const frag*)(sB + gm_swz(wc * 64 + n * 16 + li, ch));
    };
    auto mma = [&]() {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) Mma<bf16>::mma(acc[m][n], fb[n], fa[m]);      // swapped: lane (li, lg) holds row li, columns 4 lg ..
    };
    // tile kt in LDS buffer `buf`; the next one goes from its registers to the other buffer between the two fragment steps
    auto kstep = [&](auto& ra_n, auto& rb_n, int kt, int buf, bool has_next, bool do_fetch) {
        rd(buf, 0);
        mma();
        if (has_next) stage(ra_n, rb_n, kt + 1, buf ^ 1);
        rd(buf, 1);
        mma();
        if (do_fetch) fetch(ra_n, rb_n, kt + 3);
        __syncthreads();
    };
    fetch(ra0, rb0, 0);
    if (nk > 1) fetch(ra1, rb1, 1);
    stage(ra0, rb0, 0, 0);
    if (nk > 2) fetch(ra0, rb0, 2);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
        kstep(ra1, rb1, kt, 0, kt + 1 < nk, kt + 3 < nk);
        if (kt + 1 < nk) kstep(ra0, rb0, kt + 1, 1, kt + 2 < nk, kt + 4 < nk);
    }

    // ---- the tile image: x = act(acc + bias) in fp32, the arithmetic of EpiStore::compute (gemm_nt_epi.h).  The last K step ended
    // with a barrier, so nobody still reads the staging buffers this overwrites.
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int r = 64 * wr + 16 * m + li;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int c = 64 * wc + 16 * n + 4 * lg;
            const f32x4 b = *(const f32x4*)(sbias + c);
            f32x4 v = acc[m][n] + b;
            if constexpr (SIGMOID) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = __builtin_amdgcn_rcpf(1.f + __expf(-v[j]));
            }
            *(f32x4*)(xt + r * GM_LDX + c) = v;
        }
    }
    __syncthreads();

    // ---- group walk: thread = (column c, half h); groups h, h + 2, ... of the tile, members in ascending g
    const int c = tid & (TILE - 1), col = col0 + c;
    if (col >= p.N) return;
    const float fG = (float)p.G, fG1 = (float)(p.G - 1);
    for (int gi = tid >> 7; gi < p.gpt; gi += 2) {
        const int b = rt * p.gpt + gi;
        if (b >= p.B) break;
        const float* x = xt + gi * p.G * GM_LDX + c;
        float s = 0.f;
        for (int g = 0; g < p.G; ++g) s += x[g * GM_LDX];
        const float mu = s / fG;
        p.mean[(long)b * p.ld_mean + col] = mu;
        if (p.std) {
            float ss = 0.f;
            for (int g = 0; g < p.G; ++g) { const float d = x[g * GM_LDX] - mu; ss = fmaf(d, d, ss); }
            p.std[(long)b * p.ld_std + col] = sqrtf(ss / fG1);
        }
    }
}

}  // namespace mm

extern "C" int mmvae_gemm_nt_group_moments_fits(int32_t prec, int32_t B, int32_t G, int32_t N, int32_t K, int32_t act, int32_t with_std,
                                                int64_t lda, int64_t ldw) {
    if (prec == MMVAE_PREC_F32) return MMVAE_ERR_DTYPE;
    if (prec != MMVAE_PREC_BF16) return MMVAE_ERR_ARG;
    if (B < 1 || G < 1 || G > mm::TILE || N < 1) return MMVAE_ERR_ARG;
    if (with_std && G < 2) return MMVAE_ERR_ARG;
    if (K < 64 || K > 512 || K % 64) return MMVAE_ERR_ARG;
    if (act != MMVAE_ACT_NONE && act != MMVAE_ACT_SIGMOID) return MMVAE_ERR_ARG;
    if (lda % 8 || lda < K || ldw % 64 || ldw < K) return MMVAE_ERR_ARG;
    // 32-bit offsets from a scalar base, as the NT kernels: the operands stay below 4 GiB (one launch: there are no row blocks here)
    const long lim = 1L << 32;
    if ((long)B * G * lda * 2 >= lim || ((long)N + 256) * ldw * 4 >= lim) return MMVAE_ERR_ARG;
    return 0;
}

extern "C" int mmvae_gemm_nt_group_moments(const mmvae_group_moments_args* a, void* stream) {
    using namespace mm;
    if (!a) return MMVAE_ERR_ARG;
    { const int rc = mmvae_gemm_nt_group_moments_fits(a->prec, a->B, a->G, a->N, a->K, a->act, a->std != nullptr, a->lda, a->ldw); if (rc) return rc; }
    if (!a->a || !a->w || !a->mean) return MMVAE_ERR_ARG;
    if (((uintptr_t)a->a & 15) || ((uintptr_t)a->w & 15) || ((uintptr_t)a->mean & 3) || ((uintptr_t)a->std & 3)) return MMVAE_ERR_ARG;
    if (a->ld_mean < a->N || (a->std && a->ld_std < a->N)) return MMVAE_ERR_ARG;
    GmArgs k{};
    k.src = SrcPlain<bf16, bf16, 8>{(const bf16*)a->a, a->lda, a->B * a->G, a->K};
    k.w = (const bf16*)a->w; k.ldw = a->ldw; k.bias = a->bias;
    k.mean = a->mean; k.ld_mean = a->ld_mean; k.std = a->std; k.ld_std = a->ld_std;
    k.B = a->B; k.G = a->G; k.N = a->N; k.K = a->K; k.act = a->act;
    k.gpt = TILE / a->G; k.gx = (a->B + k.gpt - 1) / k.gpt; k.gy = (a->N + TILE - 1) / TILE;
    const long grid = (long)((k.gx + 7) / 8) * 8 * k.gy;
    if (grid >= (1L << 31)) return MMVAE_ERR_ARG;
    if (a->act == MMVAE_ACT_SIGMOID)
        return launch_lds<group_moments_kernel<true>>(dim3((unsigned)grid), dim3(NTHREADS), GM_LDS, (hipStream_t)stream, k);
    return launch_lds<group_moments_kernel<false>>(dim3((unsigned)grid), dim3(NTHREADS), GM_LDS, (hipStream_t)stream, k);
}
