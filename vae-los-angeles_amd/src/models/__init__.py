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
]
