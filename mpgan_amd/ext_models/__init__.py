"""The paper's baseline networks on the MI355X hot path -- the part of the reference's ``ext_models`` package that needs no graph
library: ``rGANG`` (FC generator), ``rGAND`` (rGAN discriminator), ``PointNetMixD`` (PointNet-Mix discriminator) and
``TreeGCN`` / ``TreeGANG`` (TreeGAN generator), ext_models/ext_models.py:14-72, :160-207, :211-333.  Same class names, ``args`` attributes, ``forward`` signatures and state-dict keys."""
from .ext_models import rGANG, rGAND, PointNetMixD, TreeGCN, TreeGANG  # noqa: F401
