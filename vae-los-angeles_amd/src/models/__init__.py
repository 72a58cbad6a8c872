"""Models package (reference src/models/__init__.py:4-17; the kNN comparator lives in mmvae.knn)."""
from .vae import MultiModalVAE, reparameterize
from .encoders import EncoderA, EncoderB, EncoderC
from .decoders import DecoderA, DecoderB, DecoderC
from .directional_vae import RNA2DNAVAE, DNA2RNAVAE
from .directional_ae import RNA2DNAAE, DNA2RNAAE

__all__ = [
    'MultiModalVAE',
    'reparameterize',
    'EncoderA', 'EncoderB', 'EncoderC',
    'DecoderA', 'DecoderB', 'DecoderC',
    'RNA2DNAVAE', 'DNA2RNAVAE',
    'RNA2DNAAE', 'DNA2RNAAE',
    'KINDS', 'make_model', 'forward_loss',
]

KINDS = {           # the trained models: tag = the infix of their checkpoint files
    "multimodal": dict(tag="multivae", title="MultiModalVAE", cls=MultiModalVAE),
    "dna2rna": dict(tag="dna2rna", title="DNA2RNAVAE", cls=DNA2RNAVAE),
    "rna2dna": dict(tag="rna2dna", title="RNA2DNAVAE", cls=RNA2DNAVAE),
}


def make_model(kind, input_dim_a, input_dim_b, n_sites, latent_dim):
    return KINDS[kind]["cls"](input_dim_a, input_dim_b, n_sites, latent_dim)


def forward_loss(kind, model, a, b, s, beta, class_weights):
    """One reference-shaped forward + loss; returns the total loss tensor."""
    from ..config import Config
    from ..utils import vae_loss
    from ..utils.directional_losses import dna2rna_loss, rna2dna_loss
    if kind == "multimodal":
        ra, rb, rc, mu, lv = model(a=a, b=b, site=s)
        return vae_loss(ra, a, rb, b, rc, s, mu, lv, beta=beta, gamma=Config.GAMMA, class_weights=class_weights)[0]
    if kind == "dna2rna":
        rec, mu, lv = model(dna=b, site=s)
        return dna2rna_loss(rec, a, mu, lv, beta=beta)[0]
    rec, mu, lv = model(rna=a, site=s)
    return rna2dna_loss(rec, b, mu, lv, beta=beta)[0]
