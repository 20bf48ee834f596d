"""The paper's baseline networks on the MI355X hot path -- the part of the reference's ``ext_models`` package that needs no graph
library: ``rGANG`` (FC generator), ``rGAND`` (rGAN discriminator), ``PointNetMixD`` (PointNet-Mix discriminator) and
``TreeGCN`` / ``TreeGANG`` (TreeGAN generator), ext_models/ext_models.py:14-72, :160-207, :211-333, and PCGAN's nets
(ext_models/pcgan_model.py: the equivariant layers, the set encoders ``G_inv_Tanh`` / ``G_inv``, the decoder ``G``, ``latent_G`` /
``latent_D``; ``load_pcgan_encoder`` builds the frozen pre-trained encoder).  Same class names, ``args`` attributes / constructor
arguments, ``forward`` signatures and state-dict keys."""
from .ext_models import rGANG, rGAND, PointNetMixD, TreeGCN, TreeGANG  # noqa: F401
from .pcgan_model import (PermEqui1_max, PermEqui2_max, PermEqui2_mean, G_inv_Tanh, G_inv, G, latent_G, latent_D,  # noqa: F401
                          load_pcgan_encoder)
