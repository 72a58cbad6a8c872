// The one kernel of the row-tile pipeline that is no template: the streaming squared norms (row_tile.h: rt_norms_launch).
#include "row_tile.h"

namespace mm {

// a wave per output: position `row` of s0, or position `row - s0.rows` of s1
__global__ __launch_bounds__(RT_THREADS) void rt_norms_kernel(RtRows s0, RtRows s1, int F, const float* shift, float* out) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (RT_THREADS / WAVE) + (threadIdx.x >> 6);
    if (row >= (long)s0.rows + s1.rows) return;
    const bool first = row < s0.rows;
    const int dt = first ? s0.dt : s1.dt;
    const long r = rt_row(first ? s0.order : s1.order, first ? row : row - s0.rows, first ? s0.rows : s1.rows);
    const char* base = (const char*)(first ? s0.base : s1.base) + r * (first ? s0.ld : s1.ld) * (dt == MMVAE_BF16 ? 2 : 4);
    const float v = row_sqnorm(base, dt, F, shift, lane);
    if (lane == 0) out[row] = v;
}

int rt_norms_launch(const RtRows& s0, const RtRows& s1, int F, const float* shift, float* out, hipStream_t st) {
    const long nrows = (long)s0.rows + s1.rows;
    hipLaunchKernelGGL(rt_norms_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(RT_THREADS), 0, st, s0, s1, F, shift, out);
    return (int)hipGetLastError();
}

}  // namespace mm
