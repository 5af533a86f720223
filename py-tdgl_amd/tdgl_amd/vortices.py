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

Tracks ("Tracks"): :func:`track_vortices` / `VortexFinder.tracks` link the cores of consecutive
frames by mutual nearest neighbour of equal charge within ``max_distance`` and explain every start and end of a track
as a pair event, a passage through a boundary loop, the edge of the call or nothing (:class:`VortexTracks`).
:func:`link_frames` is the rule in NumPy: the host backend, and the model ``tdgl_vortex_plan_link`` equals exactly.
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


class Links(NamedTuple):
    """What linking gives, one entry per core of all frames one after the other (indices count within a frame, -1 is
    "none"): ``next`` / ``prev`` the same vortex in the next / previous frame, ``end_partner`` / ``start_partner`` the
    core of the same frame it annihilated with / was nucleated with, ``near`` the position of the nearest loop site
    among the concatenated loops and ``near_d2`` its squared distance."""

    next: np.ndarray
    prev: np.ndarray
    end_partner: np.ndarray
    start_partner: np.ndarray
    near: np.ndarray
    near_d2: np.ndarray


LINK_BLOCK = 2048  # sources per block of `keyed_nearest` at the most, and
LINK_ENTRIES = 1 << 22  # entries of a block's distance matrix at the most (32 MiB): never a k x k matrix of a large frame


def keyed_nearest(src_xy, src_key, tgt_xy, tgt_key, r2):
    """For every source the lowest index among the targets whose key equals its own, with ``d2 <= r2`` and ``d2``
    minimal, and that ``d2``; -1 and inf where there is none.  ``d2 = (dx * dx) + (dy * dy)`` with ``dx = b.x - a.x``,
    every operation rounded on its own; a ``d2`` that is NaN or inf is never taken."""
    index = np.full(len(src_xy), -1, dtype=np.int32)
    best = np.full(len(src_xy), np.inf)
    if len(tgt_xy) == 0:
        return index, best
    rows = max(1, min(LINK_BLOCK, LINK_ENTRIES // len(tgt_xy)))
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, len(src_xy), rows):
            a, want = src_xy[lo:lo + rows], src_key[lo:lo + rows]
            dx = tgt_xy[None, :, 0] - a[:, None, 0]
            dy = tgt_xy[None, :, 1] - a[:, None, 1]
            d2 = (dx * dx) + (dy * dy)
            ok = (tgt_key[None, :] == want[:, None]) & (d2 <= r2) & (d2 < np.inf)
            d2 = np.where(ok, d2, np.inf)
            arg = d2.argmin(axis=1)  # (the first of equal minima)
            low = d2[np.arange(len(a)), arg]
            found = low < np.inf
            index[lo:lo + rows] = np.where(found, arg, -1)
            best[lo:lo + rows] = low
    return index, best


def _mutual(mine, theirs):
    """``mine[i]`` where ``theirs[mine[i]] == i``, else -1."""
    out = np.full(len(mine), -1, dtype=np.int32)
    has = np.flatnonzero(mine >= 0)
    back = has[theirs[mine[has]] == has]
    out[back] = mine[back]
    return out


def _frame_arrays(frames):
    """[(positions [k, 2] float, charges [k] int32)] of a list of `Vortices` or of (positions, charges) pairs."""
    out = []
    for frame in frames:
        positions, charges = (frame.positions, frame.charges) if isinstance(frame, Vortices) else frame[:2]
        positions = np.asarray(positions, dtype=float).reshape(-1, 2)
        charges = np.asarray(charges).reshape(-1).astype(np.int32)
        if len(positions) != len(charges):
            raise ValueError(f"A frame has {len(positions)} positions and {len(charges)} charges.")
        if np.any(np.abs(charges) != 1):
            raise ValueError("Charges must be +1 or -1.")
        out.append((positions, charges))
    if not out:
        raise ValueError("Expected at least one frame.")
    return out


def _check_max_distance(max_distance) -> float:
    r = float(max_distance)
    if not (r >= 0.0 and np.isfinite(r)):
        raise ValueError(f"max_distance must be finite and >= 0 (got {max_distance}).")
    return r


def link_frames(frames, max_distance, loop_sites_xy=None) -> Links:
    """Link the cores of consecutive frames on the host: the rule of DESIGN.md section 3, "Tracks", in NumPy, and the
    model ``tdgl_vortex_plan_link`` is held to (equal, not close: every decision compares identically rounded doubles).

    ``frames``: a list of :class:`Vortices` or of ``(positions, charges)``; ``loop_sites_xy`` [q, 2]: the coordinates
    of the boundary loops' sites one loop after the other (``None``: no loops, ``near`` = -1, ``near_d2`` = inf).

    * ``next[i] = j`` and ``prev[j] = i`` where j is i's nearest core of equal charge in the next frame within
      ``max_distance`` (ties to the lower index) and i is j's in the frame before: mutual nearest neighbour, one-to-one,
      no gap closing and not the optimal assignment.
    * ends (``next == -1``, not in the last frame) pair with their mutually nearest end of opposite charge in the same
      frame: ``end_partner``; likewise starts (``prev == -1``, not in the first frame): ``start_partner``.
    * ``near`` / ``near_d2``: the nearest loop site of every core, no radius."""
    frames = _frame_arrays(frames)
    r = _check_max_distance(max_distance)
    r2 = r * r
    nxt = [np.full(len(c), -1, dtype=np.int32) for _, c in frames]
    prv = [np.full(len(c), -1, dtype=np.int32) for _, c in frames]
    for f in range(len(frames) - 1):
        (a, ka), (b, kb) = frames[f], frames[f + 1]
        fwd, bwd = keyed_nearest(a, ka, b, kb, r2)[0], keyed_nearest(b, kb, a, ka, r2)[0]
        nxt[f], prv[f + 1] = _mutual(fwd, bwd), _mutual(bwd, fwd)
    partners = []
    for link, frames_with in ((nxt, range(len(frames) - 1)), (prv, range(1, len(frames)))):
        partner = [np.full(len(c), -1, dtype=np.int32) for _, c in frames]
        for f in frames_with:
            xy, charge = frames[f]
            loose = link[f] < 0
            choice = keyed_nearest(xy, np.where(loose, -charge, 2), xy, np.where(loose, charge, 0), r2)[0]
            partner[f] = _mutual(choice, choice)
        partners.append(partner)
    every = np.concatenate([xy for xy, _ in frames])
    if loop_sites_xy is None or len(loop_sites_xy) == 0:
        near, near_d2 = np.full(len(every), -1, dtype=np.int32), np.full(len(every), np.inf)
    else:
        targets = np.asarray(loop_sites_xy, dtype=float).reshape(-1, 2)
        zeros = np.zeros(max(len(every), len(targets)), dtype=np.int32)
        near, near_d2 = keyed_nearest(every, zeros[:len(every)], targets, zeros[:len(targets)], np.inf)
    return Links(np.concatenate(nxt), np.concatenate(prv), np.concatenate(partners[0]), np.concatenate(partners[1]),
                 near, near_d2)


class Event(NamedTuple):
    """How a track starts or ends.  ``kind``: ``"open"`` (the first / last frame of the call), ``"pair"`` (nucleated /
    annihilated with the track ``partner``), ``"boundary"`` (not a pair and within ``max_distance`` of a site of the
    loop named ``loop``: entered / left there) or ``"unexplained"``.  ``distance``: to the partner's core for a pair,
    to the nearest loop site for ``"boundary"`` and ``"unexplained"`` (inf without loops), ``None`` for ``"open"``."""

    kind: str
    partner: object
    loop: object
    distance: object


class Track(NamedTuple):
    """One vortex followed through consecutive frames: ``charge``, ``frame_indices`` [L], ``core_indices`` [L] (index in
    the frame's `Vortices`), ``positions`` [L, 2], ``triangles`` [L], ``times`` [L] (empty when none were given),
    ``velocities`` [L - 1, 2] = delta r / delta t (empty without times), ``rim_distance`` [L] to the nearest loop site,
    ``start`` and ``end`` (:class:`Event`)."""

    charge: int
    frame_indices: np.ndarray
    core_indices: np.ndarray
    positions: np.ndarray
    triangles: np.ndarray
    times: np.ndarray
    velocities: np.ndarray
    rim_distance: np.ndarray
    start: Event
    end: Event


class VortexTracks:
    """The cores of a sequence of frames linked into tracks.  ``frames``: the list of :class:`Vortices`; ``times`` [F]
    or ``None``; ``next`` / ``prev``: per frame, the index of the same vortex in the next / previous frame or -1;
    ``links``: the raw :class:`Links`; ``tracks``: the list of :class:`Track`, numbered by (first frame, index in it) of
    their first core; ``track_of``: per frame, the track number of every core.  ``loops``: ``{name: site indices}`` the
    positions ``links.near`` count through, for the events' loop names."""

    def __init__(self, frames, links, max_distance, times=None, loops=None):
        self.frames = list(frames)
        self.links = links
        self.max_distance = _check_max_distance(max_distance)
        counts = np.array([len(v.charges) for v in self.frames], dtype=np.int64)
        offset = np.concatenate([[0], np.cumsum(counts)])
        total = int(offset[-1])
        if any(len(a) != total for a in links):
            raise ValueError(f"The links are not those of these frames ({total} cores).")
        if times is not None:
            times = np.asarray(times, dtype=float).reshape(-1)
            if len(times) != len(self.frames):
                raise ValueError(f"Expected one time per frame ({len(self.frames)}; got {len(times)}).")
        self.times = times
        split = lambda a: [a[offset[f]:offset[f + 1]] for f in range(len(counts))]  # noqa: E731
        self.next, self.prev = split(links.next), split(links.prev)
        loop_names = list(loops) if loops else []
        loop_ends = np.cumsum([len(loops[name]) for name in loop_names]) if loop_names else np.zeros(0, dtype=np.int64)
        frame_of = np.repeat(np.arange(len(counts)), counts)
        # chains: every core without a predecessor begins one, in (frame, index) order
        track_of = np.full(total, -1, dtype=np.int64)
        chains = []
        for g in np.flatnonzero(links.prev < 0):
            chain = [int(g)]
            while links.next[chain[-1]] >= 0:
                here = chain[-1]
                chain.append(int(offset[frame_of[here] + 1] + links.next[here]))
            track_of[chain] = len(chains)
            chains.append(np.array(chain, dtype=np.int64))
        self.track_of = split(track_of)
        xy = np.concatenate([np.asarray(v.positions, dtype=float).reshape(-1, 2) for v in self.frames])
        charges = np.concatenate([np.asarray(v.charges) for v in self.frames])
        triangles = np.concatenate([np.asarray(v.triangles) for v in self.frames])
        rim = np.sqrt(links.near_d2)
        r2 = self.max_distance * self.max_distance

        def event(g, partner, edge_frame):
            f = frame_of[g]
            if f == edge_frame:
                return Event("open", None, None, None)
            if partner[g] >= 0:
                other = offset[f] + partner[g]
                return Event("pair", int(track_of[other]), None, float(np.hypot(*(xy[other] - xy[g]))))
            if links.near_d2[g] <= r2:
                return Event("boundary", None, loop_names[int(np.searchsorted(loop_ends, links.near[g], side="right"))],
                             float(rim[g]))
            return Event("unexplained", None, None, float(rim[g]))

        self.tracks = []
        for chain in chains:
            frame_indices = frame_of[chain]
            t = self.times[frame_indices] if self.times is not None else np.zeros(0)
            positions = xy[chain]
            velocities = (np.diff(positions, axis=0) / np.diff(t)[:, None]) if self.times is not None else np.zeros((0, 2))
            self.tracks.append(Track(
                charge=int(charges[chain[0]]), frame_indices=frame_indices, core_indices=chain - offset[frame_indices],
                positions=positions, triangles=triangles[chain], times=t, velocities=velocities, rim_distance=rim[chain],
                start=event(chain[0], links.start_partner, 0), end=event(chain[-1], links.end_partner, len(counts) - 1)))

    def __len__(self):
        return len(self.tracks)

    def __iter__(self):
        return iter(self.tracks)

    def __getitem__(self, k):
        return self.tracks[k]


def _psi_frames(x):
    """(psi [F, n], whether ``x`` was a single frame) of a ``Solution`` (its loaded step), a ``TDGLData``, a list of
    ``TDGLData`` or an array [n] or [F, n]."""
    from .solution import Solution, TDGLData

    if isinstance(x, Solution):
        x = x.tdgl_data
    if isinstance(x, TDGLData):
        return np.asarray(x.psi, dtype=complex)[None], True
    if isinstance(x, (list, tuple)) and all(isinstance(step, TDGLData) for step in x):
        if not x:
            raise ValueError("Expected at least one saved step.")
        x = [np.asarray(step.psi, dtype=complex) for step in x]
    if isinstance(x, (list, tuple)) and len({np.shape(frame) for frame in x}) > 1:
        raise ValueError(f"The frames have unequal site counts: {sorted({np.shape(frame) for frame in x})}.")
    psi = np.asarray(x, dtype=complex)
    if psi.ndim not in (1, 2):
        raise TypeError(f"Expected a Solution, a TDGLData, a list of TDGLData or an array [n] or [F, n] (got {type(x)}).")
    return (psi[None], True) if psi.ndim == 1 else (psi, False)


def _track_input(x, times):
    """(psi [F, n], times [F] or None) for tracking: a ``Solution`` stands for all its saved steps; ``times`` defaults to
    the saved steps' where ``x`` carries them."""
    from .solution import Solution, TDGLData

    if isinstance(x, Solution):
        x = list(x.saved_steps)
    if times is None and isinstance(x, (list, tuple)) and x and all(isinstance(step, TDGLData) for step in x):
        times = [step.time for step in x]
    return _psi_frames(x)[0], times


def track_vortices(device, x, max_distance, times=None, backend="host", device_id=0) -> VortexTracks:
    """The vortex cores of every frame of ``x`` (a ``Solution``: all its saved steps; a list of ``TDGLData``; ``psi``
    [F, n]) linked into tracks: see :func:`link_frames` for the rule and :class:`VortexTracks` for what comes back.
    ``max_distance`` (in ``device.length_units``) is how far a vortex may move between two frames; it has no default.
    ``backend``: ``"host"`` (:func:`host_find` per frame and :func:`link_frames`) or ``"hip"`` (:class:`VortexFinder`;
    needs a GPU, never falls back).  Both give the same links."""
    if backend not in ("host", "hip"):
        raise ValueError(f'backend must be "host" or "hip" (got {backend!r}).')
    _check_max_distance(max_distance)
    if backend == "hip":
        with VortexFinder(device, device_id=device_id) as finder:
            return finder.tracks(x, max_distance, times=times)
    psi, times = _track_input(x, times)
    sites, elements = device.points, device.triangles
    if psi.shape[1] != len(sites):
        raise ValueError(f"Expected frames of {len(sites)} sites (got {psi.shape[1]}).")
    loops = dict(device.boundary_sites() or {})
    orientations = triangle_orientations(sites, elements)
    frames = [host_find(frame, sites, elements, orientations) for frame in psi]
    loop_xy = np.asarray(sites, dtype=float)[np.concatenate([np.asarray(l) for l in loops.values()])] if loops else None
    return VortexTracks(frames, link_frames(frames, max_distance, loop_xy), max_distance, times=times, loops=loops)


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
        return _psi_frames(x)

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

    def tracks(self, x, max_distance, times=None) -> VortexTracks:
        """The cores of every frame of ``x`` (a ``Solution``: all its saved steps; a list of ``TDGLData``; ``psi``
        [F, n]) found and linked into tracks on the device: :meth:`find`, then `hipcore.VortexPlan.link`.
        ``max_distance``: how far a vortex may move between two frames (no default).  ``times`` [F] defaults to the
        saved steps' where ``x`` carries them; without times the tracks have no velocities."""
        r = _check_max_distance(max_distance)
        psi, times = _track_input(x, times)
        frames = self.find(psi)
        links = Links(*self.plan.link([len(v.charges) for v in frames], np.concatenate([v.positions for v in frames]),
                                      np.concatenate([v.charges for v in frames]), r))
        return VortexTracks(frames, links, r, times=times, loops=self.loops)

    def stats(self) -> dict:
        """`hipcore.VortexPlan.stats` of the last call."""
        return self.plan.stats()

    def link_stats(self) -> dict:
        """`hipcore.VortexPlan.link_stats` of the last :meth:`tracks`."""
        return self.plan.link_stats()

    def close(self):
        plan = getattr(self, "plan", None)
        if plan is not None:
            plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class VortexCores:
    """The vortex cores recorded inside the time loop (``SolverOptions.vortex_cores``): for every recorded step what
    :func:`host_find` / ``Solution.vortices()`` give for psi after that step, without psi having been saved.

    ``steps`` [F]: the recorded steps as row indices into ``dynamics.time``; ``times`` [F]: when psi was what the frame
    holds, after the step, ``dynamics.time[steps] + dynamics.dt[steps]``; ``counts`` [F]: records
    held per step; ``complete`` [F]: False for a step whose records did not fit ``vortex_cores_capacity`` between two
    flushes of the loop (it holds none; ``dynamics.vortex_counts`` still has its exact numbers); ``offsets`` [F + 1]:
    frame k's records are ``offsets[k]:offsets[k + 1]`` of ``positions`` [N, 2] (the units of ``device.points``),
    ``charges`` [N] and ``triangles`` [N] (rows of ``device.triangles``, ascending within a step).  ``len()``: F;
    iteration and :meth:`frame` give :class:`Vortices`.  Not written to HDF5."""

    def __init__(self, steps, times, counts, complete, positions, charges, triangles, device=None):
        self.steps = np.asarray(steps, dtype=np.int64).reshape(-1)
        self.times = np.asarray(times, dtype=float).reshape(-1)
        self.counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        self.complete = np.asarray(complete, dtype=bool).reshape(-1)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.positions = np.asarray(positions, dtype=float).reshape(-1, 2)
        self.charges = np.asarray(charges, dtype=np.int32).reshape(-1)
        self.triangles = np.asarray(triangles, dtype=np.int32).reshape(-1)
        self.device = device
        if not (len(self.steps) == len(self.times) == len(self.counts) == len(self.complete)):
            raise ValueError("steps, times, counts and complete must have one entry per recorded step.")
        if not (self.offsets[-1] == len(self.positions) == len(self.charges) == len(self.triangles)):
            raise ValueError(f"The counts add up to {self.offsets[-1]} records; got {len(self.positions)} positions, "
                             f"{len(self.charges)} charges, {len(self.triangles)} triangles.")

    def __len__(self):
        return len(self.steps)

    def frame(self, k) -> Vortices:
        """The cores of recorded step ``k`` (negative: from the end)."""
        k = int(k)
        if not -len(self) <= k < len(self):
            raise IndexError(f"frame {k} of {len(self)} recorded steps")
        k %= len(self)
        lo, hi = self.offsets[k], self.offsets[k + 1]
        return Vortices(self.positions[lo:hi], self.charges[lo:hi], self.triangles[lo:hi])

    def __iter__(self):
        return (self.frame(k) for k in range(len(self)))

    def tracks(self, max_distance, backend="host", first=0, last=None, device_id=0) -> VortexTracks:
        """The recorded frames ``first`` .. ``last`` (inclusive; default: all) linked into tracks with their times, by
        :func:`link_frames` (``backend="host"``) or `hipcore.VortexPlan.link` (``"hip"``; needs a GPU, never falls
        back), with the device's boundary loops: what :func:`track_vortices` gives for the same steps had they been
        saved, and psi is never uploaded.  Raises ``ValueError`` when a frame in the range is incomplete."""
        if backend not in ("host", "hip"):
            raise ValueError(f'backend must be "host" or "hip" (got {backend!r}).')
        r = _check_max_distance(max_distance)
        last = len(self) - 1 if last is None else int(last)
        first = int(first)
        if not 0 <= first <= last < len(self):
            raise ValueError(f"Expected 0 <= first <= last < {len(self)} (got {first}, {last}).")
        bad = np.flatnonzero(~self.complete[first:last + 1])
        if len(bad):
            raise ValueError(f"{len(bad)} of the recorded steps {first} .. {last} are incomplete (the first: {first + bad[0]}): "
                             "their cores did not fit vortex_cores_capacity records between two flushes of the time loop.")
        if self.device is None:
            raise ValueError("These records carry no device (its boundary loops are needed).")
        frames = [self.frame(k) for k in range(first, last + 1)]
        times = self.times[first:last + 1]
        loops = dict(self.device.boundary_sites() or {})
        if backend == "hip":
            with VortexFinder(self.device, loops=loops, device_id=device_id) as finder:
                links = Links(*finder.plan.link([len(v.charges) for v in frames], np.concatenate([v.positions for v in frames]),
                                                np.concatenate([v.charges for v in frames]), r))
        else:
            sites = np.asarray(self.device.points, dtype=float)
            loop_xy = sites[np.concatenate([np.asarray(l) for l in loops.values()])] if loops else None
            links = link_frames(frames, r, loop_xy)
        return VortexTracks(frames, links, r, times=times, loops=loops)
