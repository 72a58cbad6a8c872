// The class (weighted cross-entropy, reference src/utils/losses.py:39) and KL (losses.py:42) terms of vae_loss and their gradients,
// per row / per latent element: shared by vae_loss_kernel's row-per-thread class path (elementwise.hip) and the fused class-head
// launch (class_tail.hip) so that both round alike.  Every function is compiled with floating-point contraction off: each
// operation rounds on its own, whatever code surrounds the call, so the two kernels cannot differ by a fused multiply-add.
#pragma once
#include "common.h"

namespace mm {

// What a label means for its row: the class used (0 for a label that is ignored or out of range), the row's weight (0 for
// F.cross_entropy's default ignore_index -100) and whether the label lies outside [0, S) (counted in sums[4], mmvae_hip.h).
struct CeLabel { int y; float w; bool bad; };
__device__ __forceinline__ CeLabel ce_label(long long y, int S, const float* class_weights) {
    const bool ign = y == -100;
    const bool bad = !ign && (y < 0 || y >= S);
    if (bad || ign) y = 0;
    return CeLabel{(int)y, ign ? 0.f : (class_weights ? class_weights[y] : 1.f), bad};
}

// softmax numerator of one logit; m = the row's maximum
__device__ __forceinline__ float ce_exp(float x, float m) {
#pragma clang fp contract(off)
    return expf(x - m);
}

// the row's loss term: w (log sum exp - x_y); se = sum of ce_exp over the row's logits in ascending order
__device__ __forceinline__ float ce_term(float w, float m, float se, float xy) {
#pragma clang fp contract(off)
    return w * (m + logf(se) - xy);
}

// gradient w.r.t. one logit: gw (softmax - onehot), gw = gamma w
__device__ __forceinline__ float ce_grad(float gw, float e, float se, bool hit) {
#pragma clang fp contract(off)
    return gw * (e / se - (hit ? 1.f : 0.f));
}

// one latent element: returns -0.5 (1 + lv - mu^2 - exp(lv)); g_mu = beta mu, g_lv = -0.5 beta (1 - exp(lv))
__device__ __forceinline__ float kl_elem(float mu, float lv, float beta, float& g_mu, float& g_lv) {
#pragma clang fp contract(off)
    const float ex = expf(lv);
    g_mu = beta * mu;
    g_lv = -0.5f * beta * (1.f - ex);
    return -0.5f * (1.f + lv - mu * mu - ex);
}

// f64 sum over the wave's 64 lanes
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace mm
