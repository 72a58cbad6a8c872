// Dispatch of the wave-specialised NT GEMM (gemm_ntp.h): which mmvae_gemm_nt problems it takes.
#include "common.h"
#include "mmvae_hip.h"
#include "gemm_ntp.h"

namespace mm {

BnFin bn_fin_of(const mmvae_gemm_nt_args* a);               // gemm_nt.hip

// bf16 output through the plain-store epilogue; A of type AT, through the prologue Pro
template <typename AT, typename Pro = NtpProNone>
static int ntp_launch(const mmvae_gemm_nt_args* a, hipStream_t st, const Pro& pro = Pro{}) {
    // whole tiles and whole 128-byte output lines only (the kernel's epilogue has no edge handling; the tile kernels do)
    const bool wide = a->N % 256 == 0;
    if (a->c_dtype != MMVAE_BF16 || a->M % 128 || a->N % (wide ? 256 : 128) || a->ldc % 64 || ((uintptr_t)a->c & 127)) return NOT_TAKEN;
    auto go = [&](auto cfg, const auto& e) {
        return launch_ntp<decltype(cfg), AT>(a->a, a->lda, a->w, a->ldw, a->M, a->N, a->K, e, st, pro);
    };
    if (a->stat1 != nullptr || a->stat2 != nullptr) {
        const auto e = epi_store<bf16, true>(a);
        return wide ? go(NtpCfg<4, 4>{}, e) : go(NtpCfg<4, 2>{}, e);
    }
    const auto e = epi_store<bf16, false>(a);
    return wide ? go(NtpCfg<4, 4>{}, e) : go(NtpCfg<4, 2>{}, e);
}

// NOT_TAKEN: not taken (the caller continues with the tile kernels); anything else is the launch status
int ntp_dispatch(const mmvae_gemm_nt_args* a, hipStream_t st) {
    if (!g_tuning.ntp_on || a->prec != MMVAE_PREC_BF16 || a->epilogue != MMVAE_EPI_STORE || a->accumulate) return NOT_TAKEN;
    if (a->K <= 64 || a->M < g_tuning.ntp_min_m || a->M % 8) return NOT_TAKEN;      // M % 8: see the A producers' row groups
    if (a->prologue == MMVAE_PRO_BN_RELU_DROP) {
        if (a->pro_out && (a->ld_pro_out % 8 || ((uintptr_t)a->pro_out & 15) || a->ld_pro_out < a->K)) return NOT_TAKEN;
        if (a->a_dtype != MMVAE_BF16 || a->K % 64 || a->K > 512 || a->lda % 8 || ((uintptr_t)a->a & 15) || (!a->pro_finalize && (!a->pro_scale || !a->pro_shift))) return NOT_TAKEN;
        if (a->pro_mask) {
            if (a->ld_pro_mask % 8 || ((uintptr_t)a->pro_mask & 7)) return NOT_TAKEN;      // 8 keep bytes per lane and load
            return ntp_launch<bf16>(a, st, NtpProBn<true>{a->pro_scale, a->pro_shift, a->pro_mask, a->ld_pro_mask, a->pro_inv_keep, (bf16*)a->pro_out, a->ld_pro_out, bn_fin_of(a)});
        }
        return ntp_launch<bf16>(a, st, NtpProBn<false>{a->pro_scale, a->pro_shift, nullptr, 0, a->pro_inv_keep, (bf16*)a->pro_out, a->ld_pro_out, bn_fin_of(a)});
    }
    if (a->prologue != MMVAE_PRO_NONE) return NOT_TAKEN;
    if (a->a_dtype == MMVAE_F32) {
        if (a->K < 4 || ((uintptr_t)a->a & 3)) return NOT_TAKEN;
        return ntp_launch<float>(a, st);
    }
    // plain bf16 A (the decoders' hidden Linear + ReLU, decoders.py:29-30): the producers copy 16-byte chunks; 35 -> 31 us at 256 -> 512
    if (a->a_dtype == MMVAE_BF16 && a->lda % 8 == 0 && ((uintptr_t)a->a & 15) == 0) return ntp_launch<bf16>(a, st);
    return NOT_TAKEN;
}

}  // namespace mm
