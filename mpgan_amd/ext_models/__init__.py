"""The paper's baseline networks on the MI355X hot path -- the part of the reference's ``ext_models`` package that needs no graph
library: ``rGANG`` (FC generator), ``rGAND`` (rGAN discriminator) and ``PointNetMixD`` (PointNet-Mix discriminator),
ext_models/ext_models.py:14-72, :160-207.  Same class names, ``args`` attributes, ``forward`` signatures and state-dict keys."""
from .ext_models import rGANG, rGAND, PointNetMixD  # noqa: F401
