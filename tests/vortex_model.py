"""The NumPy model of the vortex finder (csrc/vortices.inc, `tdgl_amd.vortices`), operation for operation as DESIGN.md
section 3 "Vortex cores and windings" defines it, for tests/test_vortices_host.py and tests/test_hip_vortices.py.

Sign decisions compare two separately rounded products ``p = u.re v.im`` and ``q = u.im v.re``; NumPy rounds each
product on its own, and so does any compiler (a comparison offers nothing to contract), so charges, triangle numbers,
record order and windings are compared for EQUALITY.  Core positions use ``p - q``, which a compiler may fuse; they are
compared within `position_bound`:

    each cross carries at most 2u(|p| + |q|); S = (c_a + c_b) + c_c carries the sum of those plus 2u sum|c_k|; the
    three-term position sum carries 3u.  Together at most (4 kappa + 6) u r_max with
    kappa = sum_k (|p_k| + |q_k|) / |S|, u = 2^-53 and r_max the largest |coordinate| of the three sites.

The bound asserted is 8 u (kappa + 1) r_max.  Also here: the wrapped-phase form of both windings (what one would write
with np.angle) and the core position in exact rational arithmetic, as independent references for the model itself.
"""

from fractions import Fraction

import numpy as np

U = 2.0 ** -53
WINDING_UNDEFINED = -(2 ** 31)  # TDGL_WINDING_UNDEFINED


def products(u, v):
    return u.real * v.imag, u.imag * v.real


def orientations(sites, elements):
    r0, r1, r2 = sites[elements[:, 0]], sites[elements[:, 1]], sites[elements[:, 2]]
    p = (r1[:, 0] - r0[:, 0]) * (r2[:, 1] - r0[:, 1])
    q = (r2[:, 0] - r0[:, 0]) * (r1[:, 1] - r0[:, 1])
    return np.where(p > q, 1, np.where(p < q, -1, 0)).astype(np.int8)


def charges(psi, elements, orient):
    """psi: [F, n] -> int32 [F, t]."""
    a, b, c = psi[:, elements[:, 0]], psi[:, elements[:, 1]], psi[:, elements[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        s = []
        for u, v in ((a, b), (b, c), (c, a)):
            p, q = products(u, v)
            s.append(np.where(p > q, 1, np.where(p < q, -1, 0)))
    w = np.where((s[0] > 0) & (s[1] > 0) & (s[2] > 0), 1, np.where((s[0] < 0) & (s[1] < 0) & (s[2] < 0), -1, 0))
    return (w * orient[None, :].astype(np.int64)).astype(np.int32)


def find(psi, sites, elements, orient=None):
    """All records of psi [F, n] in (frame, triangle) order: dict with counts [F], frame [k], triangle [k],
    charge [k], xy [k, 2] and the yardstick's bound [k]."""
    psi = np.atleast_2d(np.asarray(psi, dtype=complex))
    if orient is None:
        orient = orientations(sites, elements)
    ch = charges(psi, elements, orient)
    frame, tri = np.nonzero(ch)  # row-major: (frame, triangle) order
    el = elements[tri]
    a, b, c = psi[frame, el[:, 0]], psi[frame, el[:, 1]], psi[frame, el[:, 2]]
    pq = [products(b, c), products(c, a), products(a, b)]
    ca, cb, cc = (p - q for p, q in pq)
    S = (ca + cb) + cc
    la, lb, lc = ca / S, cb / S, cc / S
    ra, rb, rc = sites[el[:, 0]], sites[el[:, 1]], sites[el[:, 2]]
    xy = (la[:, None] * ra + lb[:, None] * rb) + lc[:, None] * rc
    kappa = sum(np.abs(p) + np.abs(q) for p, q in pq) / np.abs(S)
    r_max = np.abs(np.concatenate([ra, rb, rc], axis=1)).max(axis=1) if len(tri) else np.zeros(0)
    return dict(counts=np.count_nonzero(ch, axis=1).astype(np.int64), frame=frame, triangle=tri.astype(np.int32),
                charge=ch[frame, tri], xy=xy, bound=8 * U * (kappa + 1) * r_max)


def position_bound(psi_frame, sites, elements, triangles):
    """8 u (kappa + 1) r_max for the given triangles of one frame."""
    el = elements[triangles]
    a, b, c = psi_frame[el[:, 0]], psi_frame[el[:, 1]], psi_frame[el[:, 2]]
    pq = [products(b, c), products(c, a), products(a, b)]
    S = ((pq[0][0] - pq[0][1]) + (pq[1][0] - pq[1][1])) + (pq[2][0] - pq[2][1])
    kappa = sum(np.abs(p) + np.abs(q) for p, q in pq) / np.abs(S)
    r_max = np.abs(sites[el].reshape(len(el), 6)).max(axis=1)
    return 8 * U * (kappa + 1) * r_max


def winding(psi_frame, loop):
    """The crossing rule around the origin; WINDING_UNDEFINED where it is not defined."""
    u = psi_frame[np.asarray(loop)]
    v = np.roll(u, -1)
    if np.any((u.real == 0) & (u.imag == 0)) or not np.all(np.isfinite(u.real) & np.isfinite(u.imag)):
        return WINDING_UNDEFINED
    p, q = products(u, v)
    if np.any((p == q) & ((u.real * v.real < 0) | (u.imag * v.imag < 0))):
        return WINDING_UNDEFINED
    up = (u.imag <= 0) & (v.imag > 0) & (p > q)
    down = (u.imag > 0) & (v.imag <= 0) & (p < q)
    return int(up.sum()) - int(down.sum())


def windings(psi, loops):
    """int32 [F, n_loops]."""
    psi = np.atleast_2d(np.asarray(psi, dtype=complex))
    return np.array([[winding(frame, loop) for loop in loops] for frame in psi], dtype=np.int32).reshape(len(psi), len(loops))


# ---------------------------------------------------------------- independent references for the model
def wrap(d):
    """Phase differences wrapped into [-pi, pi)."""
    return (d + np.pi) % (2 * np.pi) - np.pi


def wrapped_phase_charges(psi_frame, elements, orient):
    """The rounded sum of the wrapped phase differences around each triangle over 2 pi, times the orientation."""
    th = np.angle(psi_frame)
    t0, t1, t2 = th[elements[:, 0]], th[elements[:, 1]], th[elements[:, 2]]
    total = wrap(t1 - t0) + wrap(t2 - t1) + wrap(t0 - t2)
    return np.rint(total / (2 * np.pi)).astype(np.int32) * orient


def wrapped_phase_winding(psi_frame, loop):
    th = np.angle(psi_frame[np.asarray(loop)])
    return int(np.rint(wrap(np.roll(th, -1) - th).sum() / (2 * np.pi)))


def exact_position(a, b, c, ra, rb, rc):
    """The zero of the linear interpolant in exact rational arithmetic, rounded once at the end: (x, y)."""
    F = Fraction
    ar, ai, br, bi, cr, ci = (F(float(v)) for v in (a.real, a.imag, b.real, b.imag, c.real, c.imag))
    ca, cb, cc = br * ci - bi * cr, cr * ai - ci * ar, ar * bi - ai * br
    S = ca + cb + cc
    return tuple(float((ca * F(float(ra[k])) + cb * F(float(rb[k])) + cc * F(float(rc[k]))) / S) for k in range(2))


def shoelace(points):
    x, y = points[:, 0], points[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
