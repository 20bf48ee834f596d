"""The paper's baseline networks on the MI355X hot path -- the part of the reference's ``ext_models`` package that needs no graph
library: ``rGANG`` (FC generator), ``rGAND`` (rGAN discriminator), ``PointNetMixD`` (PointNet-Mix discriminator) and
``TreeGCN`` / ``TreeGANG`` (TreeGAN generator), ``NNConv`` / ``GraphBatchNorm`` / ``GraphCNNGANG`` (GraphCNN-GAN generator, on
``ops.knn_sets`` and ``ops.nnconv`` instead of PyG and torch_cluster), ext_models/ext_models.py:14-333, and PCGAN's nets
(ext_models/pcgan_model.py: the equivariant layers, the set encoders ``G_inv_Tanh`` / ``G_inv``, the decoder ``G``, ``latent_G`` /
``latent_D``; ``load_pcgan_encoder`` builds the frozen pre-trained encoder).  Same class names, ``args`` attributes / constructor
arguments, ``forward`` signatures and state-dict keys."""
from .ext_models import (rGANG, rGAND, PointNetMixD, TreeGCN, TreeGANG, NNConv, GraphBatchNorm, GraphCNNGANG,  # noqa: F401
                         knn_adjacency)
from .pcgan_model import (PermEqui1_max, PermEqui2_max, PermEqui2_mean, G_inv_Tanh, G_inv, G, latent_G, latent_D,  # noqa: F401
                          load_pcgan_encoder)
