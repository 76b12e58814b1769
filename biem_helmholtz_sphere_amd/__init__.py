"""MI355X-native implementation of the biem() dense assembly-and-solve hot path.

Drop-in for the public surface of ``biem_helmholtz_sphere`` (reference ``__init__.py:2-24``) on this path:
``biem``, ``BIEMResultCalculator``, ``plane_wave``, ``point_source``, ``max_memory``, ``max_n_end`` and the
typing helpers, plus the coordinate-tree factory the reference imports from ``ultrasphere``.
"""
__version__ = "0.1.0"

from . import _biem
from ._biem import *  # noqa: F401,F403  (every name of _biem.__all__, the one list of the binding's public names)
from ._coords import SphericalCoordinates, create_from_branching_types

__all__ = [*_biem.__all__, "SphericalCoordinates", "create_from_branching_types"]
