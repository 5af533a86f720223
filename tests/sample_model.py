"""NumPy model of csrc/sample.inc ("Currents between the sites"): every result as the fixed
sequence of separately rounded operations the kernels perform, so that model and device agree bit for bit.

* edge -> site: per site one running sum over the edges that start there (ascending), then over those that end there
  (ascending), of ``F_e d_e``; divided by the number of incident edges, then by 2.  An explicit ordered loop.
* location: the lowest-numbered triangle whose barycentric coordinates ``l1 = inv0 dx + inv1 dy``,
  ``l2 = inv2 dx + inv3 dy``, ``l0 = (1 - l1) - l2`` are all >= -1e-12, searched over ALL triangles; a triangle with zero
  determinant is never chosen; -1 and zero weights where there is none.
* sampling: ``(w0 v0 + w1 v1) + w2 v2`` per component; NaN where the triangle is -1.
* moment: ``math.fsum`` of the per-site terms ``0.5 ((x - cx) g_y - (y - cy) g_x) weight``; the device adds the same
  terms in another order, within ``n 2^-53 sum |term|``.
"""

import math

import numpy as np

TOL = 1e-12
U = 2.0 ** -53


def edges_of(elements):
    """The unique edges of a triangulation, [e, 2] int32 with the lower site first, sorted."""
    elements = np.asarray(elements).reshape(-1, 3)
    pairs = np.concatenate([elements[:, [0, 1]], elements[:, [1, 2]], elements[:, [2, 0]]])
    return np.unique(np.sort(pairs, axis=1), axis=0).astype(np.int32)


def directions(sites, edges):
    """Unit directions of the edges [e, 2] (a zero-length edge gets (1, 0))."""
    d = sites[edges[:, 1]] - sites[edges[:, 0]]
    length = np.hypot(d[:, 0], d[:, 1])
    out = d / np.where(length > 0, length, 1.0)[:, None]
    out[length == 0] = (1.0, 0.0)
    return out


def incidence_rows(n_sites, edges):
    """Per site the list of edge numbers in summation order."""
    rows = [[] for _ in range(n_sites)]
    for e, (i, _) in enumerate(edges.tolist()):
        rows[i].append(e)
    for e, (_, j) in enumerate(edges.tolist()):
        rows[j].append(e)
    return rows


def site_density(n_sites, edges, edge_dir, values, rows=None):
    """``values`` [..., n_edges] -> g [..., n_sites, 2]: the ordered loop."""
    values = np.asarray(values, dtype=float)
    rows = incidence_rows(n_sites, edges) if rows is None else rows
    lead = values.shape[:-1]
    flat = values.reshape(-1, values.shape[-1])
    out = np.empty((len(flat), n_sites, 2))
    for i, row in enumerate(rows):
        sx = np.zeros(len(flat))
        sy = np.zeros(len(flat))
        for e in row:
            sx = sx + flat[:, e] * edge_dir[e, 0]
            sy = sy + flat[:, e] * edge_dir[e, 1]
        count = float(len(row))
        out[:, i, 0] = sx / count / 2.0
        out[:, i, 1] = sy / count / 2.0
    return out.reshape(lead + (n_sites, 2))


def triangle_geometry(sites, elements):
    """(a [t, 2], inv [t, 4], usable [t]) as triinterp.py forms them."""
    tri = np.asarray(sites, dtype=float)[np.asarray(elements).reshape(-1, 3)]
    a = tri[:, 0]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.stack([e2[:, 1], -e2[:, 0], -e1[:, 1], e1[:, 0]], axis=1) / det[:, None]
    usable = (det != 0) & np.isfinite(inv).all(axis=1)
    return a, inv, usable


def _locate_block(p, a, inv, usable, chunk):
    """The points ``p`` [b, 2] against every triangle, in ascending chunks of triangles; a point leaves once it has its
    triangle (every lower-numbered one has been tested by then)."""
    triangle = np.full(len(p), -1, dtype=np.int32)
    weights = np.zeros((len(p), 3))
    left = np.arange(len(p))
    for t0 in range(0, len(a), chunk):
        t1 = min(t0 + chunk, len(a))
        with np.errstate(invalid="ignore", over="ignore"):
            dx = p[left, None, 0] - a[None, t0:t1, 0]
            dy = p[left, None, 1] - a[None, t0:t1, 1]
            l1 = inv[None, t0:t1, 0] * dx + inv[None, t0:t1, 1] * dy
            l2 = inv[None, t0:t1, 2] * dx + inv[None, t0:t1, 3] * dy
            l0 = 1.0 - l1 - l2
            ok = (l0 >= -TOL) & (l1 >= -TOL) & (l2 >= -TOL) & usable[None, t0:t1]
        hit = ok.any(axis=1)
        if hit.any():
            rows = np.flatnonzero(hit)
            first = ok[rows].argmax(axis=1)
            triangle[left[rows]] = t0 + first
            weights[left[rows]] = np.stack([l0[rows, first], l1[rows, first], l2[rows, first]], axis=1)
            left = left[~hit]
            if len(left) == 0:
                break
    return triangle, weights


def locate(sites, elements, points, block=32, chunk=4096):
    """Exhaustive search: ``(triangle [m] int32, weights [m, 3])``.  Every point is tested against every triangle up
    to and including the one it belongs to (all of them when it belongs to none); blocks of points run on a few
    threads (NumPy releases the interpreter lock), which changes no result."""
    from concurrent.futures import ThreadPoolExecutor

    points = np.asarray(points, dtype=float).reshape(-1, 2)
    m = len(points)
    triangle = np.full(m, -1, dtype=np.int32)
    weights = np.zeros((m, 3))
    a, inv, usable = triangle_geometry(sites, elements)
    if len(a) == 0 or m == 0:
        return triangle, weights
    starts = range(0, m, block)
    work = lambda lo: _locate_block(points[lo:lo + block], a, inv, usable, chunk)  # noqa: E731
    if m * len(a) < 10_000_000:
        results = [work(lo) for lo in starts]
    else:
        with ThreadPoolExecutor(max_workers=8) as pool:
            results = list(pool.map(work, starts))
    for lo, (t, w) in zip(starts, results):
        triangle[lo:lo + block] = t
        weights[lo:lo + block] = w
    return triangle, weights


def sample(values, elements, triangle, weights):
    """``values`` [..., n_sites] complex or [..., n_sites, 2] -> [..., m] / [..., m, 2]."""
    values = np.asarray(values)
    vector = not np.iscomplexobj(values)
    if not vector:
        values = np.stack([values.real, values.imag], axis=-1)
    elements = np.asarray(elements).reshape(-1, 3)
    corners = elements[np.maximum(triangle, 0)] if len(elements) else np.zeros((len(triangle), 3), dtype=int)
    v0, v1, v2 = (values[..., corners[:, k], :] for k in range(3))
    w0, w1, w2 = (weights[:, k, None] for k in range(3))
    out = (w0 * v0 + w1 * v1) + w2 * v2
    out[..., triangle < 0, :] = np.nan
    return out if vector else out[..., 0] + 1j * out[..., 1]


def moment_terms(sites, weight, centre, g):
    """Per-site terms [..., n_sites] of the moment of g [..., n_sites, 2]."""
    rx, ry = sites[:, 0] - centre[0], sites[:, 1] - centre[1]
    return 0.5 * (rx * g[..., 1] - ry * g[..., 0]) * weight


def moment(sites, weight, centre, g):
    """``(M [...], bound [...])``: the exact sum of the terms, rounded once, and the summation-order bound."""
    terms = moment_terms(sites, weight, centre, g)
    lead = terms.shape[:-1]
    flat = terms.reshape(-1, terms.shape[-1])
    total = np.array([math.fsum(row) for row in flat]).reshape(lead)
    bound = (terms.shape[-1] * U * np.abs(flat).sum(axis=1)).reshape(lead)
    return total, bound
