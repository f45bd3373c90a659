from .base import Regressor
from .hip_gp import HipGP
from .hip_gp import HipGP as GP
from .sparse_gp import HipSparseGP
from .sparse_gp import HipSparseGP as SparseGP
from .gpc import HipGPC
from .gpc import HipGPC as GPC

__all__ = ["Regressor", "GP", "HipGP", "SparseGP", "HipSparseGP", "GPC", "HipGPC"]
