"""The linking rule of DESIGN.md section 3, "Tracks", in plain loops over Python floats (IEEE doubles, every operation
rounded on its own), written without a look at `tdgl_amd.vortices.link_frames`: the model both that function and
``tdgl_vortex_plan_link`` are compared with, for equality.

    d2(a, b) = (dx * dx) + (dy * dy),  dx = b.x - a.x,  dy = b.y - a.y
    nearest(a; B, accept): the lowest j with accept(j), d2(a, B[j]) <= r2 and d2 minimal, else -1
                           (a scan in index order with a strict <, from +inf)
"""

import math

import numpy as np


def d2(a, b):
    dx = b[0] - a[0]
    dy = b[1] - a[1]
    return (dx * dx) + (dy * dy)


def nearest(a, targets, accept, r2, tally=None):
    """(index, d2) of the keyed nearest target, (-1, inf) without one.  ``tally``: a dict that counts the accepted
    targets at exactly the minimum beyond the first (``ties``) and those at exactly ``r2`` (``at_radius``)."""
    best, arg, equal = math.inf, -1, 0
    for j, b in enumerate(targets):
        if not accept(j):
            continue
        d = d2(a, b)
        if tally is not None and d == r2:
            tally["at_radius"] += 1
        if d <= r2 and d < best:
            best, arg, equal = d, j, 0
        elif d <= r2 and d == best:
            equal += 1
    if tally is not None:
        tally["ties"] += equal
    return arg, best


def link(counts, xy, charges, max_distance, loop_xy=None):
    """dict of ``next, prev, end_partner, start_partner, near`` (int32 [total]) and ``near_d2`` (float [total]) for
    frames of ``counts[f]`` cores, ``xy`` [total, 2] and ``charges`` [total] one frame after the other; and, about the
    case, ``links``, ``ties``, ``at_radius`` and ``non_mutual`` (forward choices that were not returned)."""
    counts = [int(c) for c in counts]
    xy = [(float(x), float(y)) for x, y in np.asarray(xy, dtype=float).reshape(-1, 2)]
    charges = [int(c) for c in np.asarray(charges).reshape(-1)]
    r2 = float(max_distance) * float(max_distance)
    F, total = len(counts), sum(counts)
    start = [sum(counts[:f]) for f in range(F + 1)]
    frame = [range(start[f], start[f + 1]) for f in range(F)]
    nxt, prv, endp, startp = ([-1] * total for _ in range(4))
    tally = dict(ties=0, at_radius=0)
    non_mutual = 0
    for f in range(F - 1):
        here, there = [xy[g] for g in frame[f]], [xy[g] for g in frame[f + 1]]
        qa, qb = [charges[g] for g in frame[f]], [charges[g] for g in frame[f + 1]]
        fwd = [nearest(here[i], there, lambda j: qb[j] == qa[i], r2, tally)[0] for i in range(len(here))]
        bwd = [nearest(there[j], here, lambda i: qa[i] == qb[j], r2)[0] for j in range(len(there))]
        for i, j in enumerate(fwd):
            if j >= 0 and bwd[j] == i:
                nxt[start[f] + i] = j
                prv[start[f + 1] + j] = i
            elif j >= 0:
                non_mutual += 1
    for link_, out, frames in ((nxt, endp, range(F - 1)), (prv, startp, range(1, F))):
        for f in frames:
            here = [xy[g] for g in frame[f]]
            q = [charges[g] for g in frame[f]]
            loose = [link_[g] == -1 for g in frame[f]]
            p = [nearest(here[i], here, lambda j: loose[j] and q[j] == -q[i], r2)[0] if loose[i] else -1
                 for i in range(len(here))]
            for i, j in enumerate(p):
                if j >= 0 and p[j] == i:
                    out[start[f] + i] = j
    near, near_d2 = [-1] * total, [math.inf] * total
    if loop_xy is not None and len(loop_xy):
        targets = [(float(x), float(y)) for x, y in np.asarray(loop_xy, dtype=float).reshape(-1, 2)]
        for g in range(total):
            near[g], near_d2[g] = nearest(xy[g], targets, lambda j: True, math.inf)
    i32 = lambda a: np.array(a, dtype=np.int32).reshape(-1)  # noqa: E731
    return dict(next=i32(nxt), prev=i32(prv), end_partner=i32(endp), start_partner=i32(startp), near=i32(near),
                near_d2=np.array(near_d2, dtype=float).reshape(-1), links=sum(j >= 0 for j in nxt), ties=tally["ties"],
                at_radius=tally["at_radius"], non_mutual=non_mutual)


COUNT_SEQUENCES = ([0, 1, 2, 63], [64, 65, 0, 255], [256, 257, 600], [5])


def random_case(counts, seed, floats=False):
    """(xy [total, 2], charges [total]): integer coordinates from [0, 24)^2 (exact ties and pairs at exactly d2 = 25
    abound) or, with ``floats``, a uniform cloud over the same square; charges +-1 at random."""
    rng = np.random.default_rng(seed)
    total = int(sum(counts))
    xy = rng.uniform(0, 24, size=(total, 2)) if floats else rng.integers(0, 24, size=(total, 2)).astype(float)
    return xy, rng.choice([-1, 1], size=total).astype(np.int32)


SCENARIO_FRAMES, SCENARIO_R = 12, 2.4
SCENARIO_COUNTS = [4, 4, 4, 4, 4, 4, 2, 2, 2, 1, 1, 1]


def scenario_psi(sites):
    """psi [12, n] = prod (z - a_k) / |z - a_k| (conjugated for antivortices) on ``sites``, s = f / 11: C (+) fixed at
    (-6, -6); A (+) at (1 + 12 s, 5), which leaves a film [-10, 10]^2 through its rim; B+- at (+-sep / 2, -2) with
    sep = 6 (1 - 1.6 s) while sep > 0, which annihilate."""
    z = sites[:, 0] + 1j * sites[:, 1]
    frames = []
    for f in range(SCENARIO_FRAMES):
        s = f / 11
        cores = [(-6.0, -6.0, 1), (1 + 12 * s, 5.0, 1)]
        sep = 6 * (1 - 1.6 * s)
        if sep > 0:
            cores += [(sep / 2, -2.0, 1), (-sep / 2, -2.0, -1)]
        psi = np.ones(len(z), dtype=complex)
        for x0, y0, q in cores:
            w = z - complex(x0, y0)
            w = w / np.abs(w)
            psi = psi * (w if q > 0 else w.conj())
        frames.append(psi)
    return np.stack(frames)


def assert_scenario(tracks):
    """The numbers of the scenario, asserted on a `VortexTracks` of `scenario_psi` with r = 2.4."""
    assert [len(v.charges) for v in tracks.frames] == SCENARIO_COUNTS
    assert len(tracks.tracks) == 4
    by_length = sorted(tracks.tracks, key=lambda t: -len(t.frame_indices))
    c, a, b1, b2 = by_length
    assert [len(t.frame_indices) for t in by_length] == [12, 9, 6, 6]
    assert c.charge == 1 and np.abs(c.positions - (-6, -6)).max() < 1.0
    assert a.charge == 1 and a.frame_indices.tolist() == list(range(9))
    assert a.end.kind == "boundary" and a.end.loop == "film" and a.end.partner is None
    assert abs(a.end.distance - 0.42) < 0.05 and a.end.distance == a.rim_distance[-1]
    assert {b1.charge, b2.charge} == {1, -1}
    for b, other in ((b1, b2), (b2, b1)):
        assert b.frame_indices.tolist() == list(range(6))
        assert b.end.kind == "pair" and tracks.tracks[b.end.partner] is other and b.end.loop is None
        assert b.end.distance <= SCENARIO_R
    kinds = [(t.start.kind, t.end.kind) for t in (c, a, b1, b2)]
    assert kinds == [("open", "open"), ("open", "boundary"), ("open", "pair"), ("open", "pair")]
    seen = np.concatenate([np.stack([t.frame_indices, t.core_indices], axis=1) for t in tracks.tracks])
    assert len(seen) == sum(SCENARIO_COUNTS) == len({tuple(row) for row in seen.tolist()})  # every core in one track
    for k, t in enumerate(tracks.tracks):
        assert all(tracks.frames[f].charges[i] == t.charge for f, i in zip(t.frame_indices, t.core_indices))
        assert all(tracks.track_of[f][i] == k for f, i in zip(t.frame_indices, t.core_indices))
        assert np.array_equal(t.positions, np.stack([tracks.frames[f].positions[i] for f, i in zip(t.frame_indices, t.core_indices)]))
        assert t.velocities.shape == (len(t.frame_indices) - 1, 2) and t.times.shape == t.frame_indices.shape
    # tracks are numbered by (first frame, index in it) of their first core
    firsts = [(int(t.frame_indices[0]), int(t.core_indices[0])) for t in tracks.tracks]
    assert firsts == sorted(firsts)


FIELDS = ("next", "prev","end_partner", "start_partner", "near", "near_d2")


def assert_equal(got, want):
    """The six arrays of a `Links` / a tuple in the order of ``FIELDS`` equal the model's, dtype and bytes."""
    for name, a in zip(FIELDS, got):
        b = want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert a.tobytes() == b.tobytes(), (name, np.flatnonzero(a != b)[:10])
