// What the kernels that stage 128-row operand tiles of fp32 / bf16 row matrices for the exact-f32 MFMA share (knn.hip, silhouette.hip):
// loads of four consecutive columns as wide as base and stride allow, the width the host picks for them, and the streaming squared
// norm of a row.
#pragma once
#include "common.h"

namespace mm {

__device__ __forceinline__ void knn_vld(const float* p, int vec, float (&r)[4]) {
    if (vec >= 4) { const f32x4 v = *(const f32x4*)p; r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3]; }
    else if (vec == 2) { const f32x2 a = *(const f32x2*)p, b = *(const f32x2*)(p + 2); r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1]; }
    else { r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3]; }
}
__device__ __forceinline__ void knn_vld(const bf16* p, int vec, bf16 (&r)[4]) {
    if (vec >= 4) { const bf16x4 v = *(const bf16x4*)p; r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3]; }
    else if (vec == 2) { const bf16x2 a = *(const bf16x2*)p, b = *(const bf16x2*)(p + 2); r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1]; }
    else { r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3]; }
}
// columns c0 .. c0 + 3 (c0 a multiple of 4) of a row, as stored: zeros for a row outside the matrix and for columns >= F, which are
// not read
template <typename T>
__device__ __forceinline__ void knn_ld4(const T* row, bool rowok, int c0, int F, int vec, T (&r)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = (T)0.f;
    if (!rowok || c0 >= F) return;
    if (c0 + 4 <= F) knn_vld(row + c0, vec, r);
    else {
#pragma unroll
        for (int j = 0; j < 3; ++j) if (c0 + j < F) r[j] = row[c0 + j];
    }
}

// |x - c|^2 of the row of F elements at `base` (dt: MMVAE_F32 / MMVAE_BF16), by one wave: a lane sums every 64th column and the
// butterfly adds the lanes -- a function of the row's values alone; every lane returns the sum.
__device__ __forceinline__ float row_sqnorm(const char* base, int dt, int F, const float* shift, int lane) {
    float s = 0.f;
    for (int c = lane; c < F; c += WAVE) {
        const float x = (dt == MMVAE_BF16 ? (float)((const bf16*)base)[c] : ((const float*)base)[c]) - (shift ? shift[c] : 0.f);
        s += x * x;
    }
    return wave_sum(s);
}

// elements per vector load (at most 4) that the base address and the leading dimension allow
static inline int knn_vec(const void* p, long ld, int esize) {
    for (int v = 4; v > 1; v >>= 1)
        if (ld % v == 0 && ((uintptr_t)p % (uintptr_t)(v * esize)) == 0) return v;
    return 1;
}

}  // namespace mm
