"""sph_raytracer_amd — MI355X-native spherical-grid raytracer (drop-in for Evidlo/sph_raytracer).

    from sph_raytracer_amd import SphericalGrid, ConeRectGeom, Operator
"""
from .raytracer import MatrixFreeOperator, Operator, back_project, line_integrals
from .geometry import *  # noqa: F401,F403
from .geometry import __all__ as _geometry_all
from .retrieval import cg, chambolle_pock, fista, gd, primal_dual

__all__ = ['Operator', 'MatrixFreeOperator', 'back_project', 'line_integrals', 'gd', 'cg',
           'fista', 'primal_dual', 'chambolle_pock'] + list(_geometry_all)
