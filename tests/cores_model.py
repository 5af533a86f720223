"""Model of the core records taken inside the time loops (tests/test_cores_host.py on the CPU, tests/test_hip_cores.py on
the GPU).  Nothing here is new arithmetic: the cores of a state are `tdgl_amd.vortices.host_find` on it, and the way a
flush puts the device's pool together (csrc/core_records.h) is restated as a plain loop.

Inputs: tests/census_model.py (A, B, A12).  The dense state of the GPU tests: on the mesh of input B, psi_0 of seeded
random complex values of modulus <= 1.
"""

import numpy as np

import census_model as M
from tdgl_amd.vortices import Vortices, host_find, triangle_orientations


def cores_of_states(psis, mesh):
    """`host_find` on every state: a list of `Vortices` (triangles ascending)."""
    orient = triangle_orientations(mesh.sites, mesh.elements)
    return [host_find(psi, mesh.sites, mesh.elements, orient) for psi in psis]


def dense_psi0(mesh, seed=7):
    """Random complex values of modulus <= 1: charged triangles everywhere."""
    rng = np.random.default_rng(seed)
    n = len(mesh.sites)
    return np.sqrt(rng.uniform(0.0, 1.0, n)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, n))


def assemble(rows, recorded, pool_triangles, pool_charges, pool_xy, capacity):
    """The rule of csrc/core_records.h as a loop.  ``rows`` [n, ncol] census rows of a flush window, ``recorded`` [n];
    the pool: the device's records in the order they were reserved.  Returns ``(row, offset, complete, triangles,
    charges, xy)`` over the recorded steps: a step whose segment ends within ``capacity`` keeps its records sorted by
    triangle; one whose segment reaches beyond it keeps none and is incomplete, like every recorded step after it."""
    row, offset, complete, tri, chg, xy = [], [0], [], [], [], []
    begin, overflowed = 0, False
    for r in range(len(rows)):
        if not recorded[r]:
            continue
        count = int(rows[r][0]) + int(rows[r][1])
        if begin + count > capacity:
            overflowed = True
        row.append(r)
        complete.append(not overflowed)
        if not overflowed:
            segment = sorted(range(begin, begin + count), key=lambda g: pool_triangles[g])
            tri += [pool_triangles[g] for g in segment]
            chg += [pool_charges[g] for g in segment]
            xy += [tuple(pool_xy[g]) for g in segment]
        begin += count
        offset.append(len(tri))
    return (np.array(row, dtype=np.int64), np.array(offset, dtype=np.int64), np.array(complete, dtype=bool),
            np.array(tri, dtype=np.int32), np.array(chg, dtype=np.int32), np.array(xy, dtype=float).reshape(-1, 2))


def frames_of(cores):
    """The `Vortices` of every recorded step of a ``run``'s ``cores`` dict."""
    ends = np.cumsum(cores["counts"])
    return [Vortices(cores["positions"][e - c:e], cores["charges"][e - c:e], cores["triangles"][e - c:e])
            for c, e in zip(cores["counts"], ends)]


def records_bytes(cores):
    """Everything a ``cores`` dict holds as bytes: two runs that agree give the same."""
    return b"".join(np.ascontiguousarray(cores[k]).tobytes() for k in ("steps", "counts", "complete", "triangles", "charges", "positions"))


problem = M.problem
