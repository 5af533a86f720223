"""Fields of the sheet currents at many points, evaluated on the device.

``Solution.field_at_position`` / ``vector_potential_at_position`` are all-pairs sums over (target, site) pairs; their
NumPy form holds several ``[m, n]`` arrays at once.  :class:`FieldEvaluator` keeps the sites, their areas and the
targets on the GPU (`hipcore.FieldPlan`, csrc/fields.inc) and evaluates the same sums for any saved step: per step
only the two site current fields go up (``2 x n x 2`` doubles) and the sums come back.  The ``Solution`` methods with
``backend="hip"`` are one-shot uses of it; argument checks, units and return shapes are the ``Solution`` methods' own.
"""

import numpy as np

from . import _lib
from .hipcore import FieldPlan
from .solution import Solution, TDGLData, positions_and_heights


class FieldEvaluator:
    """``positions``: (m, 2) with ``zs`` a number or an array [m], or (m, 3); in ``device.length_units``, as for
    ``Solution.field_at_position``.  ``field_units`` / ``current_units`` apply to a bare ``TDGLData``; a ``Solution``
    brings its own.  A context manager; the device buffers are freed by :meth:`close` or with the object."""

    def __init__(self, device, positions, zs=None, device_id=0, *, field_units="mT", current_units="uA"):
        self.device = device
        self.positions, self.zs = positions_and_heights(positions, zs)
        if len(self.zs) != len(self.positions):
            raise ValueError(f"Expected {len(self.positions)} heights (got {len(self.zs)}).")
        self.device_id = int(device_id)
        self.field_units, self.current_units = field_units, current_units
        if _lib.device_count() == 0:
            raise RuntimeError('backend="hip" needs a GPU, but tdgl_device_count() == 0: no HIP device is visible. '
                               'Use backend="host" (there is no silent fallback).')
        self.plan = FieldPlan(device.points, device.mesh.areas * device.coherence_length**2, device.layer.z0,
                              np.column_stack([self.positions, self.zs]), device_id=self.device_id)

    def _solution(self, solution_or_data) -> Solution:
        if isinstance(solution_or_data, Solution):
            return solution_or_data
        if not isinstance(solution_or_data, TDGLData):
            raise TypeError(f"Expected a Solution or a TDGLData (got {type(solution_or_data)}).")
        from .options import SolverOptions

        # a saved step on its own: this evaluator's device and units; it knows no applied vector potential off the mesh
        options = SolverOptions(solve_time=1.0, field_units=self.field_units, current_units=self.current_units,
                                device_id=self.device_id)
        return Solution(device=self.device, options=options, saved_steps=[solution_or_data])

    def field(self, solution_or_data, vector: bool = False, return_sum: bool = True, with_units: bool = True):
        """``Solution.field_at_position`` at this evaluator's points for the loaded step of a ``Solution`` or for a
        ``TDGLData``."""
        sol = self._solution(solution_or_data)
        return sol._field_at(self.positions, self.zs, vector, None, with_units, return_sum, "hip", self)

    def vector_potential(self, solution_or_data, return_sum: bool = True, with_units: bool = True):
        """``Solution.vector_potential_at_position`` at this evaluator's points (for a bare ``TDGLData`` the applied
        part is zero)."""
        sol = self._solution(solution_or_data)
        return sol._vector_potential_at(self.positions, self.zs, None, with_units, return_sum, "hip", self)

    def close(self):
        plan = getattr(self, "plan", None)
        if plan is not None:
            plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
