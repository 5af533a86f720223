"""Where the vortices are: cores, charges and boundary windings of saved order parameters.

The integer answer to "how many vortices, where, with which sign, how much flux in each hole" is the winding of
``arg psi`` around every mesh triangle and around every boundary loop.  Definitions ("Vortex cores
and windings"; every sign decision compares two separately rounded products and never takes the sign of a difference, so
the host functions here and the kernels of csrc/vortices.inc agree bit for bit):

    p(u, v) = u.re v.im,  q(u, v) = u.im v.re,  s(u, v) = +1 if p > q, -1 if p < q, else 0

* triangle ``(i0, i1, i2)`` with values ``(a, b, c)``: ``w = +-1`` when ``s(a, b), s(b, c), s(c, a)`` are all ``+-1``,
  else 0; the charge is ``w * orient`` with ``orient`` the sign of the triangle's signed area.  A vertex that is zero
  or NaN gives 0.
* core position: the zero of the linear interpolant, ``r = (l_a r_a + l_b r_b) + l_c r_c`` with ``l_a = cross(b, c) / S``,
  ``l_b = cross(c, a) / S``, ``l_c = cross(a, b) / S``, ``cross = p - q``, ``S = (c_a + c_b) + c_c``.
* loop winding: the crossing rule around the origin over the closed loop's edges ``u -> v``: +1 for
  ``u.im <= 0 < v.im`` with ``p > q``, -1 for ``v.im <= 0 < u.im`` with ``p < q``; not defined (``None``) when a vertex
  is zero or not finite, or an edge has ``p == q`` with ``u.re v.re < 0`` or ``u.im v.im < 0`` (a segment through the
  origin).

``Solution.vortices`` / ``Solution.boundary_windings`` use the host functions by default and :class:`VortexFinder`
(`hipcore.VortexPlan`) with ``backend="hip"``; a finder kept open serves every saved step of a run in one call.
"""

from typing import NamedTuple

import numpy as np

from . import _lib


class Vortices(NamedTuple):
    """Cores of one frame, in triangle order: ``positions`` [k, 2] in ``device.length_units``, ``charges`` [k] (+1 or
    -1), ``triangles`` [k] (rows of ``device.triangles``)."""

    positions: np.ndarray
    charges: np.ndarray
    triangles: np.ndarray


def _products(u, v):
    return u.real * v.imag, u.imag * v.real


def triangle_orientations(sites, elements) -> np.ndarray:
    """The sign of each triangle's signed area, int8 [t]: two rounded products compared."""
    r0, r1, r2 = (np.asarray(sites, dtype=float)[np.asarray(elements)[:, k]] for k in range(3))
    p = (r1[:, 0] - r0[:, 0]) * (r2[:, 1] - r0[:, 1])
    q = (r2[:, 0] - r0[:, 0]) * (r1[:, 1] - r0[:, 1])
    return (p > q).astype(np.int8) - (p < q).astype(np.int8)


def triangle_charges(psi, elements, orientations) -> np.ndarray:
    """Charges of all triangles for ``psi`` [..., n]: int8 [..., t]."""
    elements = np.asarray(elements)
    a, b, c = (psi[..., elements[:, k]] for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        pairs = [_products(a, b), _products(b, c), _products(c, a)]
        up = np.logical_and.reduce([p > q for p, q in pairs])
        down = np.logical_and.reduce([p < q for p, q in pairs])
    return (up.astype(np.int8) - down.astype(np.int8)) * orientations


def core_positions(psi, sites, elements, triangles) -> np.ndarray:
    """Zeros of the linear interpolant of ``psi`` [n] on the given triangles: [k, 2]."""
    tri = np.asarray(elements)[triangles]
    a, b, c = (psi[tri[:, k]] for k in range(3))
    cross = lambda u, v: np.subtract(*_products(u, v))  # noqa: E731
    ca, cb, cc = cross(b, c), cross(c, a), cross(a, b)
    S = (ca + cb) + cc
    la, lb, lc = ca / S, cb / S, cc / S
    ra, rb, rc = (np.asarray(sites, dtype=float)[tri[:, k]] for k in range(3))
    return (la[:, None] * ra + lb[:, None] * rb) + lc[:, None] * rc


def host_find(psi, sites, elements, orientations=None) -> Vortices:
    """The cores of one frame ``psi`` [n] on the host."""
    psi = np.asarray(psi, dtype=complex)
    if orientations is None:
        orientations = triangle_orientations(sites, elements)
    charges = triangle_charges(psi, elements, orientations)
    triangles = np.flatnonzero(charges)
    return Vortices(core_positions(psi, sites, elements, triangles), charges[triangles].astype(np.int32),
                    triangles.astype(np.int32))


def loop_winding(psi, loop):
    """Winding of ``psi`` [n] around the closed loop of site indices ``loop``, or ``None`` where it is not defined."""
    loop = np.asarray(loop)
    if len(loop) < 3:
        raise ValueError(f"A loop needs at least 3 sites (got {len(loop)}).")
    u = np.asarray(psi, dtype=complex)[loop]
    v = np.roll(u, -1)
    if np.any(u == 0) or not (np.isfinite(u.real).all() and np.isfinite(u.imag).all()):
        return None
    p, q = _products(u, v)
    if np.any((p == q) & ((u.real * v.real < 0) | (u.imag * v.imag < 0))):
        return None
    up = (u.imag <= 0) & (v.imag > 0) & (p > q)
    down = (u.imag > 0) & (v.imag <= 0) & (p < q)
    return int(np.count_nonzero(up)) - int(np.count_nonzero(down))


def boundary_loops(edges, boundary_edge_indices, points) -> list:
    """The closed chains of the mesh's boundary edges as site-index arrays, each counter-clockwise (positive shoelace
    area), starting at its lowest site number and not repeating it."""
    bedges = np.asarray(edges)[np.asarray(boundary_edge_indices)]
    neighbours = {}
    for i, j in bedges.tolist():
        neighbours.setdefault(i, []).append(j)
        neighbours.setdefault(j, []).append(i)
    if any(len(v) != 2 for v in neighbours.values()):
        raise ValueError("The mesh boundary is not a set of simple closed loops (a boundary site with other than two "
                         "boundary edges).")
    loops, unvisited = [], set(neighbours)
    while unvisited:
        start = min(unvisited)
        chain, prev, here = [start], None, start
        while True:
            unvisited.discard(here)
            nxt = [k for k in neighbours[here] if k != prev]
            nxt = nxt[0] if prev is not None or len(nxt) == 1 else min(nxt)
            if nxt == start:
                break
            chain.append(nxt)
            prev, here = here, nxt
        loop = np.array(chain, dtype=np.int64)
        x, y = points[loop, 0], points[loop, 1]
        if np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y) < 0:
            loop = np.concatenate([loop[:1], loop[:0:-1]])
        loops.append(loop)
    return loops


def _distance_to_polygon(points, polygon) -> np.ndarray:
    """Distance of each point to the closed polygon's boundary."""
    a, b = polygon[:-1], polygon[1:]
    ab = b - a
    length2 = np.maximum((ab**2).sum(axis=1), np.finfo(float).tiny)
    t = np.clip(((points[:, None, :] - a[None]) * ab[None]).sum(axis=2) / length2[None], 0.0, 1.0)
    nearest = a[None] + t[:, :, None] * ab[None]
    return np.sqrt(((points[:, None, :] - nearest) ** 2).sum(axis=2)).min(axis=1)


def name_loops(loops, points, polygons) -> dict:
    """``{polygon.name: loop}``: each polygon takes the loop whose sites lie on its boundary (the smallest largest
    distance of a loop's sites to the polygon's outline)."""
    if len(loops) != len(polygons):
        raise ValueError(f"The mesh boundary has {len(loops)} loops, the device {len(polygons)} polygons (film and holes).")
    named, taken = {}, set()
    for polygon in polygons:
        far = [np.inf if k in taken else _distance_to_polygon(points[loop], polygon.points).max()
               for k, loop in enumerate(loops)]
        k = int(np.argmin(far))
        taken.add(k)
        named[polygon.name] = loops[k]
    return named


class VortexFinder:
    """Cores and windings of many saved order parameters on the GPU.  ``loops``: ``{name: site indices}`` of closed
    loops (default: ``device.boundary_sites()``).  A context manager; the device buffers are freed by :meth:`close` or
    with the object."""

    def __init__(self, device, loops=None, device_id=0):
        from .hipcore import VortexPlan

        self.device = device
        self.device_id = int(device_id)
        self.loops = dict(device.boundary_sites() if loops is None else loops)
        if _lib.device_count() == 0:
            raise RuntimeError('backend="hip" needs a GPU, but tdgl_device_count() == 0: no HIP device is visible. '
                               'Use backend="host" (there is no silent fallback).')
        self.plan = VortexPlan(device.points, device.triangles, list(self.loops.values()), device_id=self.device_id)

    def _frames(self, x):
        """(psi [F, n], whether ``x`` was a single frame)."""
        from .solution import Solution, TDGLData

        if isinstance(x, Solution):
            x = x.tdgl_data
        if isinstance(x, TDGLData):
            return np.asarray(x.psi, dtype=complex)[None], True
        if isinstance(x, (list, tuple)) and all(isinstance(step, TDGLData) for step in x):
            if not x:
                raise ValueError("Expected at least one saved step.")
            return np.stack([np.asarray(step.psi, dtype=complex) for step in x]), False
        psi = np.asarray(x, dtype=complex)
        if psi.ndim not in (1, 2):
            raise TypeError(f"Expected a Solution, a TDGLData, a list of TDGLData or an array [n] or [F, n] (got {type(x)}).")
        return (psi[None], True) if psi.ndim == 1 else (psi, False)

    def find(self, x):
        """The cores of a ``Solution``'s loaded step, of a ``TDGLData`` or of ``psi`` [n]: one :class:`Vortices`; of
        ``psi`` [F, n] or of a list of saved steps: a list, one per frame."""
        psi, single = self._frames(x)
        counts, triangles, charges, xy, _ = self.plan.find(psi, windings=False)
        ends = np.cumsum(counts)
        frames = [Vortices(xy[e - c:e], charges[e - c:e], triangles[e - c:e]) for c, e in zip(counts, ends)]
        return frames[0] if single else frames

    def windings(self, x):
        """``{name: int or None}`` of the loops for one frame, a list of such dicts for many."""
        from .hipcore import WINDING_UNDEFINED

        psi, single = self._frames(x)
        wind = self.plan.windings(psi)
        frames = [{name: (None if w == WINDING_UNDEFINED else int(w)) for name, w in zip(self.loops, row)} for row in wind]
        return frames[0] if single else frames

    def stats(self) -> dict:
        """`hipcore.VortexPlan.stats` of the last call."""
        return self.plan.stats()

    def close(self):
        plan = getattr(self, "plan", None)
        if plan is not None:
            plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
