"""RNA2DNAAE / DNA2RNAAE (reference src/models/directional_ae.py:10-134): the non-variational baselines of the cross-validation --
an MLP encoder that ends in ONE Linear(hidden, latent), the site through Embedding -> Linear(embed, latent), the plain mean of the
latents present, one decoder.  No eps, no logvar, no KL term: forward returns (reconstruction, latent).  Constructor signatures,
attribute names and state_dict keys are the reference's (encoder_rna.{0,1,4}, encoder_dna.{0,1,4,5,8}, site_embedding,
site_projection, decoder_dna.fc / decoder_rna.fc); the nn.Sequential encoders are parameter containers only, forward never calls
them (engine.AEGraph)."""
import torch.nn as nn

from mmvae import engine, functional as F_
from ._common import HipModule, hidden_stack
from .decoders import DecoderA, DecoderB


def _encoder(widths, latent_dim):
    """nn.Sequential [Linear, BatchNorm1d, ReLU, Dropout(0.1)] per (in, out) pair, then Linear(last, latent): keys 0, 1, 4, 5, ..."""
    return nn.Sequential(*hidden_stack(widths), nn.Linear(widths[-1][1], latent_dim))


def _encoder_block(seq, name):
    n = (len(seq) - 1) // 4
    return engine.EncoderMLP([seq[4 * i] for i in range(n)], [seq[4 * i + 1] for i in range(n)], seq[4 * n], None, name=name)


class _DirectionalAE(HipModule):
    _SLOT = "a"              # the engine slot of the encoder: "a" (RNA) or "b" (DNA)

    def _parts(self):
        raise NotImplementedError

    def _graph(self):
        g = getattr(self, "_g", None)
        if g is None:
            enc, dec = self._parts()
            g = engine.AEGraph(site=engine.EmbedEncoder(self.site_embedding, self.site_projection), decoder=dec._block(),
                               **{"enc_" + self._SLOT: _encoder_block(enc, type(self).__name__ + ".encoder")})
            object.__setattr__(self, "_g", g)
        return g

    def _run(self, x, site):
        if x is None and site is None:
            return None, None
        xa, xb = (x, None) if self._SLOT == "a" else (None, x)
        outs, latent = F_.run_ae_graph(self._graph(), self._prec(), self.training, xa, xb, site)
        return outs[0], latent


class RNA2DNAAE(_DirectionalAE):
    """Encodes RNA + primary site, decodes DNA methylation."""
    _SLOT = "a"

    def __init__(self, rna_dim, dna_dim, n_sites, latent_dim, embed_dim=32):
        super().__init__()
        self.encoder_rna = _encoder([(rna_dim, 128)], latent_dim)
        self.site_embedding = nn.Embedding(n_sites, embed_dim)
        self.site_projection = nn.Linear(embed_dim, latent_dim)
        self.decoder_dna = DecoderB(latent_dim, dna_dim)

    def _parts(self):
        return self.encoder_rna, self.decoder_dna

    def forward(self, rna=None, site=None):
        """Returns (reconstructed_dna, latent); two Nones without inputs."""
        return self._run(rna, site)


class DNA2RNAAE(_DirectionalAE):
    """Encodes DNA methylation + primary site, decodes RNA expression."""
    _SLOT = "b"

    def __init__(self, rna_dim, dna_dim, n_sites, latent_dim, embed_dim=32):
        super().__init__()
        self.encoder_dna = _encoder([(dna_dim, 512), (512, 256)], latent_dim)
        self.site_embedding = nn.Embedding(n_sites, embed_dim)
        self.site_projection = nn.Linear(embed_dim, latent_dim)
        self.decoder_rna = DecoderA(latent_dim, rna_dim)

    def _parts(self):
        return self.encoder_dna, self.decoder_rna

    def forward(self, dna=None, site=None):
        """Returns (reconstructed_rna, latent); two Nones without inputs."""
        return self._run(dna, site)
