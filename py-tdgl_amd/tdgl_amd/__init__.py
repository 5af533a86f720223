"""tdgl_amd: MI355X-native TDGL time-stepping core behind py-tdgl's solver API.

Public surface (mirrors `tdgl/__init__.py:1-23` of the reference for the solver path):
``Layer, Polygon, Device, SolverOptions, SolverOptionsError, SparseSolver, solve, TDGLSolver,
Solution`` and the ``geometry`` helpers; beyond it, ``solve_ensemble`` (many replicas of one device at once)
``SolverOptions.vortex_census`` (vortex counts and boundary windings at every step, counted inside the time loop:
``DynamicsData.vortex_counts`` / ``windings``, ``WINDING_UNDEFINED``), ``SolverOptions.vortex_cores`` (the cores themselves at
every step, recorded by the same launch: ``DynamicsData.vortex_cores``, a ``VortexCores`` with ``.tracks()``),
``FieldEvaluator`` (fields of the currents at many points, on the device), ``VortexFinder`` / ``Vortices`` (vortex
cores, charges and boundary windings of saved steps, on the device), ``track_vortices`` / ``VortexTracks`` (those cores
linked into tracks from frame to frame) and ``CurrentSampler`` (sheet currents and psi
between the sites, path currents and moments of saved steps, on the device).
"""

from . import geometry  # noqa: F401
from .device import Device, Layer, Polygon, TerminalInfo  # noqa: F401
from .finite_volume import EdgeMesh, Mesh  # noqa: F401
from .operators import MeshOperators  # noqa: F401
from .parameter import (  # noqa: F401
    CompositeParameter, Constant, ConstantField, CurrentLoop, HotSpot, HotSpotEpsilon, LinearRamp, MovingCurrentLoop, Parameter,
    PiecewiseLinear, Scale, SeparableEpsilon, TabulatedCurrents, TabulatedRamp,
)
from .options import SolverOptions, SolverOptionsError, SparseSolver  # noqa: F401
from .solution import WINDING_UNDEFINED, BiotSavartField, BoundaryPhases, DynamicsData, Fluxoid, Solution, TDGLData  # noqa: F401
from .solver import SolverResult, TDGLSolver, solve  # noqa: F401
from .ensemble import ENSEMBLE_MAX_SITES, solve_ensemble  # noqa: F401
from .fields import FieldEvaluator  # noqa: F401
from .vortices import VortexCores, VortexFinder, VortexTracks, Vortices, track_vortices  # noqa: F401
from .sampling import CurrentSampler  # noqa: F401

__version__ = "0.1.0"
