// Device bodies of the two small launches that end the backward -- EncoderC's backward and the loss finalisation -- shared by their
// stand-alone kernels (elementwise.hip) and the rider workgroups of the grouped dW launch (gemm_tn.hip): one source, the same
// arithmetic in the same order in both places.
#pragma once
#include "common.h"

namespace mm {

struct EmbedBwd {
    int S, E, L, copies;
    const float* emb; const float* w_mu; const float* w_lv; const float* dTc;
    float* d_emb; float* d_w_mu; float* d_b_mu; float* d_w_lv; float* d_b_lv;
};
constexpr size_t EMBED_BWD_LDS_MAX = 64 * 1024;          // the default dynamic-LDS limit (60 KB at latent 128, embed 32, 24 sites); a rider takes no more
// The stand-alone launch's capacity: operands past EMBED_BWD_LDS_MAX run the same kernel with the attribute raised to the CU's whole
// LDS (74.75 KB at latent 100, embed 64, 24 sites -- the corner of the reference's hyperparameter search)
constexpr size_t EMBED_BWD_LDS_BIG = 160 * 1024;
// heads: 2 = EncoderC's (mu | logvar) table, 1 = the autoencoders' one projection (w_lv / d_w_lv / d_b_lv unused, L2 = L below)
static inline size_t embed_bwd_lds(int S, int E, int L, int heads = 2) { return ((size_t)S * heads * L + (size_t)S * E + (size_t)heads * L * E) * sizeof(float); }
static inline int embed_bwd_blocks(int S, int E, int L, int heads = 2) { return (S * E + heads * L * E + heads * L + 255) / 256; }       // one output element per thread

// Workgroup lb of nb (256 threads each).
// All operands are a few KB: every workgroup first copies them into LDS in ONE round of independent loads (the table gradient summed
// over its scatter copies in fixed order, the embedding, both head weights), then every thread forms its output element from LDS.
// (Round 2's form walked w_mu / w_lv / emb in global memory inside the dot products: 20-24 dependent rounds of L2 latency, 22 us for
// a few thousand multiply-adds.)
template <int HEADS = 2>
__device__ __forceinline__ void embed_table_bwd_body(const EmbedBwd& a, int lb, int nb, float* sm) {
    const int S = a.S, E = a.E, L = a.L, copies = a.copies;
    const float* const emb = a.emb; const float* const w_mu = a.w_mu; const float* const w_lv = a.w_lv; const float* const dTc = a.dTc;
    float* const d_emb = a.d_emb; float* const d_w_mu = a.d_w_mu; float* const d_b_mu = a.d_b_mu; float* const d_w_lv = a.d_w_lv;
    float* const d_b_lv = a.d_b_lv;
    const int L2 = HEADS * L;                            // one head: every j below is < L, w_lv and its gradients are never touched
    float* dT = sm;                                      // [S][2L]: the copies of the table gradient summed (fixed order)
    float* sE = dT + S * L2;                             // [S][E]
    float* sW = sE + S * E;                              // [2L][E]: w_mu rows, then w_lv rows
    const int t0 = lb * blockDim.x + threadIdx.x, nt = nb * blockDim.x;
    // one index space [dEmb | dWcat | db]: the three products run side by side
    const int n0 = S * E, n1 = n0 + L2 * E, n2 = n1 + L2;
    auto dst_of = [&](int i) -> float* {
        if (i < n0) return d_emb + i;
        if (i < n1) { const int k = i - n0, j = k / E, e = k - j * E; return j < L ? d_w_mu + (long)j * E + e : d_w_lv + (long)(j - L) * E + e; }
        const int j = i - n1;
        return j < L ? d_b_mu + j : d_b_lv + (j - L);
    };
    // the gradient element this thread adds to is requested together with the operands: behind the products it was one more
    // dependent round trip of a launch that is nothing but round trips
    float* const dst0 = t0 < n2 ? dst_of(t0) : nullptr;
    const float old0 = dst0 ? *dst0 : 0.f;
    for (int i = threadIdx.x; i < S * L2; i += blockDim.x) {
        float c8[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) c8[c] = c < copies ? dTc[(long)c * S * L2 + i] : 0.f;
        float v = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) v += c8[c];
        for (int c = 8; c < copies; ++c) v += dTc[(long)c * S * L2 + i];
        dT[i] = v;
    }
    for (int i = threadIdx.x; i < S * E; i += blockDim.x) sE[i] = emb[i];
    for (int i = threadIdx.x; i < L2 * E; i += blockDim.x) sW[i] = i < L * E ? w_mu[i] : w_lv[i - L * E];
    __syncthreads();
    for (int i = t0; i < n2; i += nt) {
        float acc = 0.f;
        if (i < n0) {                                    // dEmb = dT x Wcat
            const int s = i / E, e = i - s * E;
#pragma unroll 4
            for (int j = 0; j < L2; ++j) acc += dT[s * L2 + j] * sW[j * E + e];
        } else if (i < n1) {                             // dWcat = dT^T x emb
            const int k = i - n0, j = k / E, e = k - j * E;
#pragma unroll 4
            for (int s = 0; s < S; ++s) acc += dT[s * L2 + j] * sE[s * E + e];
        } else {
            const int j = i - n1;
#pragma unroll 4
            for (int s = 0; s < S; ++s) acc += dT[s * L2 + j];
        }
        if (i == t0) *dst0 = old0 + acc;
        else { float* d = dst_of(i); *d += acc; }
    }
}

// out = {total, recon, class, kld, labels out of range} as the reference returns them (losses.py:44,46); one thread
__device__ __forceinline__ void loss_finalize_body(const double* sums, float beta, float gamma, const float* beta_gamma_dev, float* out) {
    if (beta_gamma_dev) { beta = beta_gamma_dev[0]; gamma = beta_gamma_dev[1]; }
    const double recon = sums[0] + sums[1];
    out[0] = (float)(recon + (double)gamma * sums[2] + (double)beta * sums[3]);
    out[1] = (float)recon; out[2] = (float)sums[2]; out[3] = (float)sums[3]; out[4] = (float)sums[4];
}

}  // namespace mm
