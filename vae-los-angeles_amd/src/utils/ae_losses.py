"""rna2dna_ae_loss / dna2rna_ae_loss (reference src/utils/ae_losses.py:8-39): the reconstruction term alone -- sum-BCE for DNA
methylation, sum-MSE for RNA expression -- through the fused loss pass, with no KL term."""
from mmvae import functional as F_


def rna2dna_ae_loss(recon_dna, dna):
    """Returns (total_loss Tensor, reconstruction_loss float)."""
    total, out4 = F_.fused_loss({"b": (recon_dna, dna)}, 0.0, 1.0)
    return total, F_.read_losses(out4)[1]


def dna2rna_ae_loss(recon_rna, rna):
    """Returns (total_loss Tensor, reconstruction_loss float)."""
    total, out4 = F_.fused_loss({"a": (recon_rna, rna)}, 0.0, 1.0)
    return total, F_.read_losses(out4)[1]
