// Shared device helpers for the MI355X (gfx950 / CDNA4) MultiModalVAE kernels.
// Wavefront = 64 lanes; MFMA tiles are 16x16 (bf16: K=32, f32: K=4) with f32 accumulate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mmvae_hip.h"

namespace mm {

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;

constexpr int WAVE = 64;
constexpr int TILE = 128;          // output tile edge of both GEMM kernels
constexpr int NTHREADS = 256;      // 4 waves, 2x2, 64x64 each
constexpr int ROW_BYTES = 128;     // bytes of one LDS row in the NT kernel (= one K step)
constexpr int NUM_CU = 256;        // compute units of the MI355X, the only target: persistent kernels launch one workgroup per CU

// ---- MFMA wrappers: one "fragment step" consumes 16 bytes per lane of A and of B ------------
template <typename CT> struct Mma;

template <> struct Mma<bf16> {
    static constexpr int EPC = 8;            // elements per 16-byte chunk
    static constexpr int KSTEP = 32;         // reduction elements per fragment step
    typedef bf16x8 frag;
    static __device__ __forceinline__ void mma(f32x4& acc, const frag& a, const frag& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
};

template <> struct Mma<float> {
    static constexpr int EPC = 4;
    static constexpr int KSTEP = 16;
    typedef f32x4 frag;
    // lane group g = lane>>4 holds reduction indices 4g..4g+3 of the step; MFMA sub-step s
    // multiplies element s of every group (any bijection of k is valid as long as A and B agree).
    static __device__ __forceinline__ void mma(f32x4& acc, const frag& a, const frag& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc, 0, 0, 0);
    }
};

template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16 from_f32<bf16>(float v) { return (bf16)v; }
__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(bf16 v) { return (float)v; }

// 16-byte register image of EPC compute-type elements
template <typename CT> struct Chunk;
template <> struct Chunk<bf16> {
    bf16x8 v;
    __device__ __forceinline__ void set(int i, float x) { v[i] = (bf16)x; }
    __device__ __forceinline__ void zero() { v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; }
};
template <> struct Chunk<float> {
    f32x4 v;
    __device__ __forceinline__ void set(int i, float x) { v[i] = x; }
    __device__ __forceinline__ void zero() { v = f32x4{0.f, 0.f, 0.f, 0.f}; }
};

// Vector load of `VEC` elements of type T into floats (VEC*sizeof(T) <= 16, naturally aligned).
template <typename T, int VEC> struct VLoad;
template <> struct VLoad<float, 1> { static __device__ __forceinline__ void ld(const float* p, float* o) { o[0] = p[0]; } };
template <> struct VLoad<float, 2> { static __device__ __forceinline__ void ld(const float* p, float* o) { f32x2 v = *(const f32x2*)p; o[0] = v[0]; o[1] = v[1]; } };
template <> struct VLoad<float, 4> { static __device__ __forceinline__ void ld(const float* p, float* o) { f32x4 v = *(const f32x4*)p; o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3]; } };
template <> struct VLoad<bf16, 1> { static __device__ __forceinline__ void ld(const bf16* p, float* o) { o[0] = (float)p[0]; } };
template <> struct VLoad<bf16, 2> { static __device__ __forceinline__ void ld(const bf16* p, float* o) { bf16x2 v = *(const bf16x2*)p; o[0] = (float)v[0]; o[1] = (float)v[1]; } };
template <> struct VLoad<bf16, 4> { static __device__ __forceinline__ void ld(const bf16* p, float* o) { bf16x4 v = *(const bf16x4*)p; for (int i = 0; i < 4; ++i) o[i] = (float)v[i]; } };
template <> struct VLoad<bf16, 8> { static __device__ __forceinline__ void ld(const bf16* p, float* o) { bf16x8 v = *(const bf16x8*)p; for (int i = 0; i < 8; ++i) o[i] = (float)v[i]; } };

// One LDS-DMA wave-instruction (64 lanes x 16 bytes -> 1 KB of LDS at `lds_addr`, lane-linear) as inline assembly.  Through
// __builtin_amdgcn_global_load_lds hipcc's wait-count pass treats later LDS reads as possibly reading the DMA's destination and, in
// loops that wait with counted s_waitcnt vmcnt(N) of their own, drains every transfer in flight with an s_waitcnt vmcnt(0) right
// behind the issue or in front of the next one -- the tile's whole trip from HBM then sits inside every step and a ring deeper than
// two slots buys nothing (seen in the ISA of the rings of gemm_tn.hip and gemm_tn_wide.hip, the callers).  Issued from assembly the
// transfers are invisible to that pass; the kernel's own counted waits order them (vmcnt counts them in issue order like any other
// vector-memory operation).  PRECONDITION: m0 is written and not restored (the compiler reserves the register and knows nothing of
// this write: a clobber entry for it is only warned about), so a kernel that uses this helper uses no builtin LDS-DMA and nothing
// else that reads m0.  The form that saves and restores m0 around the transfer (two more scalar moves) was measured in both rings
// and left the parent's spread on the two-wave-group kernels (profiles/tn_single_source_bench.json).
__device__ __forceinline__ void lds_dma16(const void* g, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" :: "s"(lds_addr), "v"(g) : "memory");
}
__device__ __forceinline__ unsigned lds_addr_of(const void* p) {
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}

// Natural logarithm as ONE v_log_f32 (log2, about 1 ulp) and one multiply.  hipcc expands __logf / logf into 13 vector instructions
// (denormal pre-scaling, a compensated multiply by ln 2, an inf / nan select): in the BCE term that was 22 of the 58 instructions per
// element (round 3, read off the ISA).  Differs from logf only in the last bits and for denormal arguments (below 1.18e-38: -inf here,
// i.e. torch's -100 clamp, where torch still has -87.3 .. -103): no sigmoid output of a finite logit above -87 is that small.
__device__ __forceinline__ float fast_ln(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Philox4x32-10 counter-based generator (Salmon et al. 2011); used for dropout masks and eps.
struct Philox {
    static __device__ __forceinline__ void round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
        const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
        // ONE 32 x 32 -> 64-bit multiply-add (v_mad_u64_u32) per product: written as __umulhi + a 32-bit product hipcc emits
        // v_mul_hi_u32 + v_mul_lo_u32 (the noise launch is bound by its multiplies; step -2.6 us)
        const uint64_t p0 = (uint64_t)M0 * (uint64_t)c[0], p1 = (uint64_t)M1 * (uint64_t)c[2];
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    }
    static __device__ __forceinline__ void gen(uint64_t seed, uint64_t ctr_lo, uint64_t ctr_hi, uint32_t (&out)[4]) {
        uint32_t c[4] = {(uint32_t)ctr_lo, (uint32_t)(ctr_lo >> 32), (uint32_t)ctr_hi, (uint32_t)(ctr_hi >> 32)};
        uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
        for (int i = 0; i < 10; ++i) { round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        for (int i = 0; i < 4; ++i) out[i] = c[i];
    }
};

// ------------------------------------------------------------------------------------------
// Cycle stamps: the diagnostic library only (make STAMP=1 -> libmmvae_stamp.so, read with tools/stamp.py KERNEL).  A kernel sums
// cycle deltas per wave in st_acc[] (slot i of st_acc is slot i of its buffer) and a sample of its waves adds them to the buffer
// with stamp_flush; mmvae_debug_stamps(kernel, out, n, reset) copies a buffer out.  In the product build every piece below is empty.
//
// Kernel ids and slot layouts ("phases" are cycles summed over the sampled waves' steps; "steps" the number of such steps):
//   STAMP_NT   gemm_nt_kernel (gemm_nt.hip), every 16th workgroup's wave 0:  0 reads(s1) + mma(s0) issue, 1 stage (vmcnt wait +
//              ds_write + drain), 2 barrier wait, 3 fetch + reads(s0) + mma(s1) issue, 4 K steps, 5 waves, 6 whole kernel,
//              7 of slot 1: wait for the global loads, 8 before the first K step, 9 after the last one
//   STAMP_NT2  gemm_nt2_kernel (gemm_nt2.h), every 16th workgroup's wave 0:  0 wait for the own DMA, 1 barrier wait, 2 DMA issue of
//              the next step, 3 fragment reads + MFMA, 4 K steps, 5 waves, 6 whole kernel, 9 epilogues (7, 8 unused)
//   STAMP_NTP  gemm_ntp_kernel (gemm_ntp.h), every 16th workgroup:  consumer wave 0: 0 barrier wait, 1 fragment reads + MFMA,
//              2 epilogues, 3 K steps, 4 tiles, 5 whole kernel, 6 workgroups; producer wave 0, per K step: 8 barrier wait,
//              9 wait for the set's loads, 10 v_cvt_pk (fp32 -> bf16), 11 ds_write issue, 12 W DMA issue, 13 A load issue,
//              14 wait for W of the next step
//   STAMP_TN   gemm_tn_kernel's body (gemm_tn.hip), every 8th workgroup's wave 0:  0 fragment step 0, 1 stage (vmcnt wait +
//              ds_write), 2 fragment step 1 + fetch issue + drain, 3 barrier wait, 4 batch steps, 5 waves, 6 whole kernel,
//              7 of slot 1: wait for the global loads, 8 before the first batch step, 9 after the last one
//   STAMP_TNW  gemm_tnw_dma_kernel (gemm_tn_wide.hip), every 8th workgroup's wave 0:  0 wait for the own DMA, 1 barrier, 2 DMA
//              issue, 3 fragments + MFMA, 4 batch steps, 5 workgroups, 6 whole kernel, 7 epilogue
// ------------------------------------------------------------------------------------------
enum StampKernel { STAMP_NT = 0, STAMP_NT2 = 1, STAMP_NTP = 2, STAMP_TN = 3, STAMP_TNW = 4 };
constexpr int STAMP_SLOTS = 16;

#ifdef MM_STAMP
#define STAMP_T(x) unsigned long long x = __builtin_readcyclecounter()      // a timestamp
#define STAMP_ADD(i, d) st_acc[i] += (d)                                    // add a delta to slot i
#define STAMP_ONLY(...) __VA_ARGS__                                         // a statement of the stamp build
#define UNSTAMPED(...)                                                      // a statement of the product build
// A kernel's buffer, in the object that holds the kernel, and its host-side reader
#define STAMP_BUFFER(name) \
    __device__ unsigned long long stamps_##name[STAMP_SLOTS]; \
    int stamp_read_##name(uint64_t* out, int n, int reset) { return stamp_copy(HIP_SYMBOL(stamps_##name), out, n, reset); }
// The extern "C" entry point, in one object of the library
#define STAMP_ENTRY() \
    extern "C" int mmvae_debug_stamps(int32_t kernel, uint64_t* out, int32_t n, int32_t reset) { \
        switch (kernel) { \
        case mm::STAMP_NT: return mm::stamp_read_nt(out, n, reset); \
        case mm::STAMP_NT2: return mm::stamp_read_nt2(out, n, reset); \
        case mm::STAMP_NTP: return mm::stamp_read_ntp(out, n, reset); \
        case mm::STAMP_TN: return mm::stamp_read_tn(out, n, reset); \
        case mm::STAMP_TNW: return mm::stamp_read_tnw(out, n, reset); \
        } \
        return MMVAE_ERR_ARG; \
    }

template <int N>
__device__ __forceinline__ void stamp_flush(unsigned long long* slots, const unsigned long long (&acc)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) atomicAdd(&slots[i], acc[i]);
}
// the first n slots of a buffer -> out; then zeroes the buffer if reset
inline int stamp_copy(const void* sym, uint64_t* out, int n, int reset) {
    if (n < 0 || n > STAMP_SLOTS) return MMVAE_ERR_ARG;
    hipError_t e = hipMemcpyFromSymbol(out, sym, n * sizeof(uint64_t));
    if (e != hipSuccess || !reset) return (int)e;
    const uint64_t z[STAMP_SLOTS] = {};
    return (int)hipMemcpyToSymbol(sym, z, sizeof(z));
}
int stamp_read_nt(uint64_t*, int, int);
int stamp_read_nt2(uint64_t*, int, int);
int stamp_read_ntp(uint64_t*, int, int);
int stamp_read_tn(uint64_t*, int, int);
int stamp_read_tnw(uint64_t*, int, int);
#else
#define STAMP_T(x)
#define STAMP_ADD(i, d)
#define STAMP_ONLY(...)
#define UNSTAMPED(...) __VA_ARGS__
#define STAMP_BUFFER(name)
#define STAMP_ENTRY()
#endif

// ------------------------------------------------------------------------------------------
// Host-side dispatch plumbing shared by the GEMM entry points
// ------------------------------------------------------------------------------------------

// Dispatch knobs, set through mmvae_set_tuning (tests flip them inside one process to compare the kernel forms on the same data)
struct Tuning {
    int nt_wide_min_m = NUM_CU * 128;   // key 0: 128x256 NT tiles only when there are >= NUM_CU row tiles
    int nt2_on = 1;                  // key 2: the LDS-DMA NT generation (gemm_nt2.h) against the register-staged one
    long split_bytes = 1L << 32;     // key 3 (log2, 0 = default): operands of at least this many bytes are processed in row blocks
    long block_bytes = 1L << 31;     //   ... of this size; key 3 sets half the threshold
    int tn_wide_on = 1;              // key 4: the wide-tile dW kernels (gemm_tn_wide.hip)
    int bnbwd_stream = 1;            // key 6: BatchNorm-backward NT epilogue through LDS (gemm_nt2.h)
    int relu_stream = 1;             // key 7: ReLU-mask NT epilogue through LDS (gemm_nt2.h)
    int ntp_on = 1;                  // key 8: the wave-specialised NT kernel (gemm_ntp.h)
    int ntp_min_m = 16384;           // key 9: below this a persistent 256-workgroup grid has < 1 tile per CU
    int latent_on = 1;               // key 10: the fused latent launch (latent.hip); off: mmvae_latent_fwd answers MMVAE_ERR_ARG
    int class_tail_on = 1;           // key 12: the fused class-head launch (class_tail.hip); off: mmvae_class_tail answers MMVAE_ERR_ARG
    int step_head_on = 1;            // key 13: the merged head-of-step launch (elementwise.hip); off: mmvae_step_head answers MMVAE_ERR_ARG
    int ae_latent_on = 1;            // key 15: the autoencoders' fused latent launch (latent.hip); off: mmvae_ae_latent_fwd answers MMVAE_ERR_ARG
    int tn_riders_on = 1;            // key 14: riders in the grouped dW launch (gemm_tn.hip); off: mmvae_gemm_tn_group_riders answers MMVAE_ERR_ARG
};
inline Tuning g_tuning;

// Returned by a form's dispatch when the problem is not one of its own: the caller goes on to the next form.  Distinct from every
// launch status (hipError_t > 0) and argument error (MMVAE_ERR_* < 0).
constexpr int NOT_TAKEN = 1 << 30;

// Launches a kernel with more dynamic LDS than the default limit.  The attribute is set once per kernel (Kernel is the template
// parameter, so kernels that share a parameter list keep separate flags) and retried until it succeeds.  Returns the launch status.
template <auto Kernel, typename... Args>
inline int launch_lds(dim3 grid, dim3 block, int lds, hipStream_t st, const Args&... args) {
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        attr_done = true;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return (int)hipGetLastError();
}

// The kernels address their operands with 32-bit offsets from a scalar base.  Operands of 4 GiB or more (the scaled omics widths:
// 65 536 x 27 000 fp32 = 7 GB) are processed in row blocks: M rows whose largest operand row has row_bytes bytes.
inline bool needs_row_blocks(long M, long row_bytes) { return M * row_bytes >= g_tuning.split_bytes; }

// Calls block(r0, rows) for consecutive row blocks of M rows and stops at the first non-zero status.  A block is below the split
// threshold, so an entry point that recurses into itself for a block ends after one level.
template <typename F>
inline int for_row_blocks(long M, long row_bytes, F&& block) {
    long rows = g_tuning.block_bytes / row_bytes;
    if (rows <= 0) return MMVAE_ERR_ARG;                    // before any block is enqueued
    const long nblk = (M + rows - 1) / rows;                // equal blocks (65 536 rows -> 4 x 16 384, not 3 x 19 712 + 6 400: a short
    long even = (M + nblk - 1) / nblk;                      // last block falls below the sizes the wide-tile kernels take)
    if (even >= 256) even = (even + 255) & ~255L;
    if (even <= rows) rows = even;
    else if (rows >= 256) rows &= ~255L;
    for (long r0 = 0; r0 < M; r0 += rows) {
        const int rc = block(r0, (int)(M - r0 < rows ? M - r0 : rows));
        if (rc) return rc;
    }
    return 0;
}

// Batch split of a dW GEMM: the M rows go to nsplit workgroups of rps rows each, a whole number of MT-row batch steps.
// want > 0 asks for about that many splits.  want <= 0 plans ONE resident round of wg_target workgroups over ntiles output tiles,
// in a multiple of 8 splits (split z runs on XCD z % 8: every XCD gets the same share; a 520-block grid costs a whole extra round).
// An automatic count, and an asked one when limit > 0, keeps at least 4 batch steps per split (every split adds its partial tile to
// each output element) and at most `limit` splits.
struct SplitPlan { int nsplit, rps; };
inline SplitPlan plan_splits(int M, int MT, int want, int ntiles, int wg_target, int limit = 0) {
    int nsplit = want;
    if (want <= 0) {
        nsplit = wg_target / ntiles;
        if (nsplit >= 8) nsplit &= ~7;
    }
    if (want <= 0 || limit > 0) {
        const int max_split = (M + 4 * MT - 1) / (4 * MT);
        if (nsplit > max_split) nsplit = max_split;
        if (limit > 0 && nsplit > limit) nsplit = limit;
        if (nsplit < 1) nsplit = 1;
    }
    int rps = (M + nsplit - 1) / nsplit;
    rps = (rps + MT - 1) / MT * MT;
    return {(M + rps - 1) / rps, rps};
}

// Elements per vector load (4, 2 or 1) of an operand whose rows of n elements of esize bytes lie ld elements apart from p: the
// widest that divides ld and n and to which p is aligned.  Used for fp32 operands with whatever alignment the caller's tensor has
// (e.g. (B, 782): 8-byte rows).
inline int vec_width(long ld, long n, const void* p, long esize = 4) {
    const uintptr_t a = (uintptr_t)p;
    if (ld % 4 == 0 && n % 4 == 0 && (a & (4 * esize - 1)) == 0) return 4;
    if (ld % 2 == 0 && n % 2 == 0 && (a & (2 * esize - 1)) == 0) return 2;
    return 1;
}

}  // namespace mm

#define MM_CHECK_LAUNCH() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)
