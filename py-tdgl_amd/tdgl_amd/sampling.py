"""Sheet currents and psi between the sites of saved steps, on the GPU.

:class:`CurrentSampler` (`hipcore.SamplePlan`, csrc/sample.inc) keeps the mesh and a fixed set of positions on the device
and serves every saved step of a run in one call: the edge -> site average of ``Mesh.get_quantity_on_site``, the
piecewise-linear interpolant of `tdgl_amd.triinterp` at the positions, the current through the path the positions form
and the dipole moment.  Definitions ("Currents between the sites"; each a fixed sequence of
separately rounded operations, so the kernels agree with the NumPy model of tests/sample_model.py bit for bit):

* site density ``g_i = (sum of F_e d_e over the edges that start at i, ascending, then over those that end at i) /
  count_i / 2`` -- ``np.bincount``'s order in ``get_quantity_on_site``;
* a position belongs to the lowest-numbered triangle whose barycentric coordinates are all >= -1e-12 (triinterp.py's
  formula), found through a uniform grid of cells; in none: NaN (psi) or zero (current densities, like the host method);
* value at a position ``(w0 v0 + w1 v1) + w2 v2``;
* moment ``sum_i 1/2 ((x_i - cx) g_y - (y_i - cy) g_x) a_i`` in a fixed order.

The kernels apply no physical prefactor; K0, xi and the units are applied here.  The sampler's raster lives on the mesh
triangulation: it is the interpolant of ``Solution.interp_current_density``, not ``grid_current_density``'s SciPy
``griddata`` (which triangulates the sites anew and so also fills holes and concave corners).
``Solution.interp_current_density``, ``interp_order_parameter``, ``current_through_path`` and ``magnetic_moment`` use a
sampler with ``backend="hip"``.
"""

import numpy as np

from . import _lib


def trapezoid_path_current(J, path_coords, inside) -> float:
    """The reference's accumulation of ``current_through_path`` (solution.py:623-667) for ``J`` [m, 2] sampled on the
    path's vertices: per-segment means dotted into the segment normals, times the segment lengths, over the segments
    whose centres are ``inside``, then the trapezoid rule over those.  The operations of ``Solution.current_through_path``
    on one frame, so that a frame's current does not depend on how many frames a call holds."""
    from .geometry import path_vectors

    J_edge = (J[:-1] + J[1:]) / 2
    lengths, normals = path_vectors(path_coords)
    J_dot_n = (J_edge * normals).sum(axis=1)
    y = (J_dot_n * lengths)[inside]
    return float(np.sum((y[1:] + y[:-1]) / 2)) if len(y) > 1 else 0.0


class CurrentSampler:
    """Currents and psi of many saved steps at fixed ``positions`` [m, 2] (``device.length_units``; ``None``: site
    quantities and moments only).  ``x`` below is a ``Solution`` (its loaded step), a ``TDGLData``, a list of
    ``TDGLData``, or for the currents ``(supercurrent [F, E], normal_current [F, E])`` and for psi an array [F, n]; one
    frame in gives one frame out, many give a leading axis.  Currents come in ``current_units`` (a ``Solution``'s own,
    else the sampler's attribute, ``"uA"`` unless changed) per ``device.length_units``.  A context manager; the device
    buffers are freed by :meth:`close` or with the object.  The positions are located on the mesh triangulation (not
    SciPy's ``griddata``)."""

    DATASETS = (None, "supercurrent", "normal_current")

    def __init__(self, device, positions=None, device_id=0):
        from .hipcore import SamplePlan

        self.device = device
        self.device_id = int(device_id)
        self.current_units = "uA"
        self.positions = None if positions is None else np.atleast_2d(np.asarray(positions, dtype=float))
        if self.positions is not None and (self.positions.ndim != 2 or self.positions.shape[1] != 2):
            raise ValueError(f"Expected positions [m, 2] (got {self.positions.shape}).")
        if _lib.device_count() == 0:
            raise RuntimeError('backend="hip" needs a GPU, but tdgl_device_count() == 0: no HIP device is visible. '
                               'Use backend="host" (there is no silent fallback).')
        mesh, xi = device.mesh, device.coherence_length
        self.inside = None if self.positions is None else device.contains_points(self.positions)
        # the centre of mass as Solution.magnetic_moment computes it
        com = (mesh.sites * mesh.areas[:, None]).sum(axis=0) / mesh.areas.sum()
        self.plan = SamplePlan(device.points, mesh.edge_mesh.edges, mesh.edge_mesh.normalized_directions, device.triangles,
                               self.positions, weights=mesh.areas, centre=xi * com, device_id=self.device_id)

    # -- inputs -------------------------------------------------------------------------------------------------------
    def _steps(self, x):
        from .solution import Solution, TDGLData

        if isinstance(x, Solution):
            x = x.tdgl_data
        if isinstance(x, TDGLData):
            return [x], True
        if isinstance(x, list) and all(isinstance(step, TDGLData) for step in x):
            if not x:
                raise ValueError("Expected at least one saved step.")
            return x, False
        return None, False

    def _edge_values(self, x, dataset):
        """(edge values [F, n_fields, E], whether ``x`` was a single frame)."""
        if dataset not in self.DATASETS:
            raise ValueError(f"Unexpected dataset: {dataset}.")
        steps, single = self._steps(x)
        if steps is not None:
            js = np.stack([np.asarray(s.supercurrent, dtype=float) for s in steps])
            jn = np.stack([np.asarray(s.normal_current, dtype=float) for s in steps])
        elif isinstance(x, tuple) and len(x) == 2:
            js, jn = (np.asarray(a, dtype=float) for a in x)
            if js.shape != jn.shape or js.ndim not in (1, 2):
                raise TypeError(f"Expected (supercurrent, normal_current) of one shape [E] or [F, E] (got {js.shape}, {jn.shape}).")
            single = js.ndim == 1
            js, jn = np.atleast_2d(js), np.atleast_2d(jn)
        else:
            raise TypeError("Expected a Solution, a TDGLData, a list of TDGLData or (supercurrent, normal_current) "
                            f"(got {type(x)}).")
        fields = {None: (js, jn), "supercurrent": (js,), "normal_current": (jn,)}[dataset]
        return np.stack(fields, axis=1), single

    def _psi(self, x):
        steps, single = self._steps(x)
        if steps is not None:
            return np.stack([np.asarray(s.psi, dtype=complex) for s in steps]), single
        psi = np.asarray(x, dtype=complex)
        if psi.ndim not in (1, 2):
            raise TypeError(f"Expected a Solution, a TDGLData, a list of TDGLData or an array [n] or [F, n] (got {type(x)}).")
        return (psi[None], True) if psi.ndim == 1 else (psi, False)

    def _need_positions(self):
        if self.positions is None:
            raise ValueError("This sampler was opened without positions.")

    def _units_of(self, x) -> str:
        from .solution import Solution

        return x.options.current_units if isinstance(x, Solution) else self.current_units

    def _k0(self, current_units: str) -> float:
        """K0 in ``current_units / length_units``, as ``Solution._k0``."""
        from .device import CURRENT_UNITS, LENGTH_UNITS, _unit

        dev = self.device
        return dev.K0 * LENGTH_UNITS[dev.length_units] / _unit(CURRENT_UNITS, current_units, "current")

    def _density_factor(self, current_units: str, units) -> float:
        """Conversion from ``current_units / length_units`` to ``units``, as ``Solution._density_factor``."""
        from .device import CURRENT_UNITS, LENGTH_UNITS, _unit

        if units is None:
            return 1.0
        parts = [p.strip() for p in units.split("/")]
        if len(parts) != 2:
            raise ValueError(f"Expected current density units like 'uA / um' (got {units!r}).")
        have = CURRENT_UNITS[current_units] / LENGTH_UNITS[self.device.length_units]
        want = _unit(CURRENT_UNITS, parts[0], "current") / _unit(LENGTH_UNITS, parts[1], "length")
        return have / want

    @staticmethod
    def _total(k0, parts):
        """``k0 * part`` summed over the one or two fields [F, n_fields, ...], in the host methods' order."""
        return k0 * parts[:, 0] + k0 * parts[:, 1] if parts.shape[1] == 2 else k0 * parts[:, 0]

    def _point_density(self, values, k0, factor):
        J = self._total(k0, self.plan.eval(values, point_density=True)[1]) * factor
        J[~np.isfinite(J).all(axis=-1)] = 0
        J[:, ~self.inside] = 0
        return J

    # -- results ------------------------------------------------------------------------------------------------------
    def site_current_density(self, x, dataset=None) -> np.ndarray:
        """The sheet current density on the sites, [n, 2] or [F, n, 2], in ``current_units / length_units``:
        ``Solution.current_density`` (``supercurrent_density``, ``normal_current_density``) of every frame, to the bit."""
        values, single = self._edge_values(x, dataset)
        g = self._total(self._k0(self._units_of(x)), self.plan.eval(values, site_density=True)[0])
        return g[0] if single else g

    def current_density(self, x, dataset=None, units=None) -> np.ndarray:
        """The sheet current density at the positions, [m, 2] or [F, m, 2], in ``units`` (default
        ``current_units / length_units``): zero outside the film and in holes, as ``Solution.interp_current_density``."""
        self._need_positions()
        values, single = self._edge_values(x, dataset)
        cu = self._units_of(x)
        J = self._point_density(values, self._k0(cu), self._density_factor(cu, units))
        return J[0] if single else J

    def order_parameter(self, x) -> np.ndarray:
        """psi at the positions, [m] or [F, m]; NaN outside the mesh."""
        self._need_positions()
        psi, single = self._psi(x)
        out = self.plan.eval(psi=psi, point_psi=True)[2]
        return out[0] if single else out

    def magnetic_moment(self, x):
        """The z component of the dipole moment of the total sheet current about the film's centre of mass,
        ``(1/2) sum_i (r_i - r_cm) x K_i a_i`` in ``current_units * length_units**2``: a float or [F]."""
        values, single = self._edge_values(x, None)
        M = self._total(self._k0(self._units_of(x)), self.plan.eval(values, moment=True)[3])
        M = M * self.device.coherence_length**2
        return float(M[0]) if single else M

    def path_current(self, x, dataset=None, units=None):
        """The current through the path the positions form, in ``units`` (default ``current_units``): the reference's
        ``current_through_path`` -- its trapezoid accumulation of the sampled densities, on the host.  A float or [F]."""
        from .device import CURRENT_UNITS, _unit

        self._need_positions()
        values, single = self._edge_values(x, dataset)
        cu = self._units_of(x)
        J = self._point_density(values, self._k0(cu), 1.0)
        centres = (self.positions[:-1] + self.positions[1:]) / 2
        inside = self.device.contains_points(centres)
        total = np.array([trapezoid_path_current(frame, self.positions, inside) for frame in J])
        if units is not None:
            total = total * (CURRENT_UNITS[cu] / _unit(CURRENT_UNITS, units, "current"))
        return float(total[0]) if single else total

    def location(self):
        """``(triangle [m] int32, weights [m, 3])`` of the positions: rows of ``device.triangles``, -1 where a position
        is in no triangle."""
        self._need_positions()
        return self.plan.location()

    def stats(self) -> dict:
        """`hipcore.SamplePlan.stats` of the last call."""
        return self.plan.stats()

    def close(self):
        plan = getattr(self, "plan", None)
        if plan is not None:
            plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
