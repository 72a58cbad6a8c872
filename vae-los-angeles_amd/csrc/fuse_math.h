// The fusion of ONE latent element in its two forms, shared by the stand-alone kernels (elementwise.hip: fuse_fwd_kernel,
// fuse_mean_fwd_kernel, the plain-mean policy of fuse_bwd_kernel) and the fused latent launch (latent.hip) so that all round alike.
// Mean fusion + reparameterisation (reference src/models/vae.py:65-73, 11-15):
#pragma once
#include "common.h"

namespace mm {

// mu / lv: the sums over the modalities present, in the order a, b, table; they leave as the means.  Returns z = mu + eps * std (fp32).
__device__ __forceinline__ float fuse_reparam_elem(float& mu, float& lv, int n_mod, float inv_n, float eps) {
    if (n_mod > 1) { mu *= inv_n; lv *= inv_n; }
    return mu + eps * expf(0.5f * lv);
}

// The autoencoders' fusion (reference src/models/directional_ae.py:58-64): `sum` over the modalities present in the order head, table
// row; it leaves as the mean.  One or two terms: the result is exact after the one addition.
__device__ __forceinline__ float fuse_mean_elem(float sum, int n_mod, float inv_n) { return n_mod > 1 ? sum * inv_n : sum; }

}  // namespace mm
