// Mean fusion + reparameterisation of ONE latent element (reference src/models/vae.py:65-73, 11-15), shared by
// fuse_fwd_kernel (elementwise.hip) and the fused latent launch (latent.hip) so that both round alike.
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
