"""Inputs, NumPy model and oracle record of the census tests (tests/test_census_host.py on the CPU,
tests/test_hip_census.py on the GPU).

The census of an order parameter is one int32 row ``(n_plus, n_minus, w_0 .. w_{L-1})``: the number of mesh triangles
of charge +1 / -1 (`tdgl_amd.vortices.triangle_charges`) and the winding around every loop
(`tdgl_amd.vortices.loop_winding`, `WINDING_UNDEFINED` where it is None).  The oracle's census is that of its psi
after every `OracleSolver.update` with dt_init 1e-3, dt_max 0.1, adaptive, epsilon = 1, u and gamma the defaults, no
terminals.

Input A   `synthetic_mesh(8)`: 95 sites, 153 triangles, one rim of 35 sites, zero field; psi_0 the product of three
          vortex factors z / |z| tanh|z|, z = (x - x0) + i q (y - y0), at (-0.21, +0.07), (+0.13, -0.11), (+0.33, +0.29)
          of the bounding box's span from the mean of the sites with q = +1, -1, +1.
Input A12 `synthetic_mesh(12)`: 189 sites, the same psi_0 recipe, uniform field b = 0.35: a vortex that stays.
Input B   tests/golden/mesh_polygon.npz: 1,002 sites, rim and two holes of 40 and 30 sites, zero field; psi_0 a pure
          phase winding +1 around the centre of the first hole times one vortex factor with xi = 0.5, placed 0.6
          outside the second hole's edge on the line towards the first.
"""

import functools
import os
from types import SimpleNamespace

import numpy as np

from helpers import GAMMA_DEFAULT, U_DEFAULT, mesh_from_golden, synthetic_mesh, uniform_field_A
from tdgl_amd.vortices import boundary_loops, loop_winding, triangle_charges, triangle_orientations

WINDING_UNDEFINED = -(2 ** 31)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CORES = ((-0.21, 0.07, 1), (0.13, -0.11, -1), (0.33, 0.29, 1))
FIELD_A12 = 0.35


def options(**kw):
    d = dict(solve_time=1e9, skip_time=0.0, dt_init=1e-3, dt_max=0.1, adaptive=True, adaptive_window=10,
             max_solve_retries=10, adaptive_time_step_multiplier=0.25, save_every=10**9, terminal_psi=None)
    d.update(kw)
    return SimpleNamespace(**d)


def loops_of(mesh):
    """The closed chains of the mesh's boundary edges, the longest (the rim) first."""
    em = mesh.edge_mesh
    loops = boundary_loops(em.edges, em.boundary_edge_indices, mesh.sites)
    return sorted(loops, key=len, reverse=True)


def census_row(psi, mesh, loops, orient=None):
    """The model: one row for ``psi`` [n]."""
    if orient is None:
        orient = triangle_orientations(mesh.sites, mesh.elements)
    q = triangle_charges(np.asarray(psi, dtype=complex), mesh.elements, orient)
    w = [loop_winding(psi, loop) for loop in loops]
    return np.array([np.count_nonzero(q > 0), np.count_nonzero(q < 0)] + [WINDING_UNDEFINED if v is None else v for v in w],
                    dtype=np.int32)


def census_rows(psis, mesh, loops):
    orient = triangle_orientations(mesh.sites, mesh.elements)
    return np.array([census_row(p, mesh, loops, orient) for p in psis], dtype=np.int32).reshape(len(psis), 2 + len(loops))


def vortex_factor(sites, x0, y0, q, xi=1.0):
    z = (sites[:, 0] - x0) + 1j * q * (sites[:, 1] - y0)
    r = np.abs(z)
    return np.where(r > 0, z / np.where(r > 0, r, 1.0), 0.0) * np.tanh(r / xi)


def psi0_three(mesh, reverse=False):
    """Input A's start; ``reverse``: every charge reversed."""
    s = mesh.sites
    c, span = s.mean(axis=0), s.max(axis=0) - s.min(axis=0)  # the centre: the mean of the sites
    psi = np.ones(len(s), dtype=complex)
    for fx, fy, q in CORES:
        psi = psi * vortex_factor(s, c[0] + fx * span[0], c[1] + fy * span[1], -q if reverse else q)
    return psi


def psi0_hole_and_vortex(mesh, loops):
    """Input B's start."""
    s = mesh.sites
    c1, c2 = s[loops[1]].mean(axis=0), s[loops[2]].mean(axis=0)
    z = (s[:, 0] - c1[0]) + 1j * (s[:, 1] - c1[1])
    d = (c1 - c2) / np.linalg.norm(c1 - c2)
    edge = float(np.linalg.norm(s[loops[2]] - c2, axis=1).mean())  # the (round) hole's radius
    at = c2 + (edge + 0.6) * d
    return z / np.abs(z) * vortex_factor(s, at[0], at[1], 1, xi=0.5)


@functools.lru_cache(maxsize=None)
def problem(name):
    """``dict(mesh, loops, A, psi0, mu0, options)`` of input "A", "A_reversed", "A_uniform", "A12" or "B"."""
    if name in ("A", "A_reversed", "A_uniform"):
        mesh = synthetic_mesh(8)
        loops = loops_of(mesh)
        psi0 = np.ones(len(mesh.sites), dtype=complex) if name == "A_uniform" else psi0_three(mesh, name == "A_reversed")
        A = uniform_field_A(mesh, 0.0)
    elif name == "A12":
        mesh = synthetic_mesh(12)
        loops = loops_of(mesh)
        psi0, A = psi0_three(mesh), uniform_field_A(mesh, FIELD_A12)
    elif name == "B":
        mesh = mesh_from_golden(np.load(os.path.join(GOLDEN, "mesh_polygon.npz")))
        loops = loops_of(mesh)
        psi0, A = psi0_hole_and_vortex(mesh, loops), uniform_field_A(mesh, 0.0)
    else:
        raise KeyError(name)
    return dict(name=name, mesh=mesh, loops=loops, A=A, psi0=psi0, mu0=np.zeros(len(mesh.sites)), options=options(),
                u=U_DEFAULT, gamma=GAMMA_DEFAULT)


@functools.lru_cache(maxsize=None)
def oracle_census(name, n_steps):
    """``(rows [n_steps, 2 + L], dt [n_steps], psi after the last step)`` of the CPU oracle on input ``name``.  Computed
    once per process and shared; callers must not write into it."""
    from oracle import OracleSolver

    p = problem(name)
    mesh = p["mesh"]
    solver = OracleSolver(mesh, p["A"], 1.0, p["u"], p["gamma"], options())
    orient = triangle_orientations(mesh.sites, mesh.elements)
    psi, mu = p["psi0"].copy(), p["mu0"].copy()
    t, dt = 0.0, p["options"].dt_init
    rows, dts = [], []
    for k in range(n_steps):
        dt, psi, mu, _, _ = solver.update({"step": k, "time": t, "dt": dt}, None, dt, psi=psi, mu=mu)
        t += dt
        rows.append(census_row(psi, mesh, p["loops"], orient))
        dts.append(dt)
    rows = np.array(rows, dtype=np.int32)
    rows.setflags(write=False)
    return rows, np.array(dts), psi


@functools.lru_cache(maxsize=None)
def oracle_states(name, n_steps, seed=None):
    """psi after every update of the oracle on input ``name``, [n_steps, n]; with ``seed`` the start is psi_0 (1 + 1e-15 g),
    g standard normal from that seed: a change of rounding size."""
    from oracle import OracleSolver

    p = problem(name)
    solver = OracleSolver(p["mesh"], p["A"], 1.0, p["u"], p["gamma"], options())
    psi, mu = p["psi0"].copy(), p["mu0"].copy()
    if seed is not None:
        psi = psi * (1.0 + 1e-15 * np.random.default_rng(seed).standard_normal(len(psi)))
    t, dt = 0.0, p["options"].dt_init
    out = []
    for k in range(n_steps):
        dt, psi, mu, _, _ = solver.update({"step": k, "time": t, "dt": dt}, None, dt, psi=psi, mu=mu)
        t += dt
        out.append(psi)
    out = np.array(out)
    out.setflags(write=False)
    return out


def deviation(psi, ref):
    """max |psi - ref| after the global phase that the gauge of mu leaves open has been taken out (helpers.align_phase)."""
    ov = np.vdot(psi, ref)
    if abs(ov) > 0:
        psi = psi * (ov / abs(ov))
    return float(np.max(np.abs(psi - ref)))


SENSITIVITY_SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def oracle_sensitivity(name, n_steps):
    """E[k]: how far the oracle's own psi after update k + 1 moves when its start changes by one rounding (the largest
    deviation so far over `SENSITIVITY_SEEDS`, so E does not decrease).  On inputs A and B the vortices' motion makes
    the trajectory unstable: E grows from 1e-12 after the first update by eight orders of magnitude in 80 updates."""
    ref = oracle_states(name, n_steps)
    worst = np.zeros(n_steps)
    for seed in SENSITIVITY_SEEDS:
        twin = oracle_states(name, n_steps, seed)
        worst = np.maximum(worst, [deviation(twin[k], ref[k]) for k in range(n_steps)])
    return np.maximum.accumulate(worst)


ONE_UPDATE = 5e-12  # what one update of the device may differ from the oracle's by (tests/test_hip_local_failure.py,
#                     test_single_psi_update_call: the tolerance of one psi update against the oracle)


def deviation_bound(name, n_steps):
    """What the device's psi may differ from the oracle's by after update k + 1: (k + 1) `ONE_UPDATE` E[k] / E[0].
    The device rounds the operations of every update differently from the oracle, so each of the k + 1 updates so far
    has put in a difference of at most `ONE_UPDATE`, and none of them has grown by more than a difference present after
    the first update grows in the oracle itself, which is E[k] / E[0]."""
    E = oracle_sensitivity(name, n_steps)
    return (np.arange(n_steps) + 1.0) * ONE_UPDATE * E / E[0]


def transitions(rows):
    """``[(k, row)]``: row 0 and every row that differs from the one before it (k: its index; "after update k + 1")."""
    rows = np.asarray(rows)
    keep = [0] + [k for k in range(1, len(rows)) if not np.array_equal(rows[k], rows[k - 1])]
    return [(k, tuple(int(v) for v in rows[k])) for k in keep]
