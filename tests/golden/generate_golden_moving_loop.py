"""Generate `traj_moving_loop_small.npz` by running the REFERENCE itself (build container only).

    python tests/golden/generate_golden_moving_loop.py [--out DIR]

A uniform bias field plus one current loop scanned across mesh_small, A(r, t) = A_0(r) + I(t) A_loop(r - c(t); a), given to
the reference's `TDGLSolver.update` as one time-dependent `applied_vector_potential` that calls the reference's own
`em.current_loop_vector_potential` at c(t) (as `generate_golden_field_terms` does for a sum of terms):

    A_0   a uniform field b = 0.1,
    loop  radius 2, one length unit above the film; its centre moves (-4, -1) -> (4, 2) over t in [0.3, 2.0], rests, then
          moves in y only until t = 3.0; its current goes up, holds, and comes down through zero.

Centre and current are piecewise linear on ONE list of nodes (the union of the path's and the waveform's, which differ); the
last node lies before the end of the run.  The script asserts that the run holds every kind of step the step rule tells
apart.  The file stores the bias, the nodes, what `run_reference` returns and the loop's values at every call.  Data only
(no reference source text).
"""

import numpy as np

import generate_golden as gg
from generate_golden_field_terms import longest_run
from generate_golden_loop import _Units
from tdgl import em

B0 = 0.1
RADIUS, HEIGHT = 2.0, 1.0
PATH_T = [0.3, 2.0, 2.4, 3.0]
PATH_XY = [(-4.0, -1.0), (4.0, 2.0), (4.0, 2.0), (4.0, -1.0)]
WAVE_T = [0.1, 0.7, 2.3, 3.3]           # up, a hold that outlasts the path's rest by 0.1 on the left, down through zero
WAVE_I = [0.0, 1.5, 1.5, -0.6]          # (dimensionless: mu_0, the units and the field scale folded in; peak field ~ 0.27)
SOLVE_TIME = 4.0


def nodes():
    """times, centers [n, 3], currents [n]: both piecewise-linear functions on the union of their nodes."""
    t = np.array(sorted(set(PATH_T) | set(WAVE_T)))
    xy = np.array(PATH_XY)
    centers = np.column_stack([np.interp(t, PATH_T, xy[:, 0]), np.interp(t, PATH_T, xy[:, 1]), HEIGHT * np.ones(len(t))])
    return t, centers, np.interp(t, WAVE_T, WAVE_I)


def main():
    em.ureg = _Units()
    small = gg.make_ref_mesh(20, 20)  # mesh_small
    # (dt_max = 0.05: see generate_golden_field_terms)
    o = gg.SolverOptions(solve_time=SOLVE_TIME, dt_init=1e-3, dt_max=0.05, save_every=50)
    probes = [small.closest_site((-5, 0)), small.closest_site((5, 0))]
    A0 = gg.uniform_field_A(small, B0)
    times, centers, currents = nodes()
    pos = np.column_stack([small.edge_mesh.centers, np.zeros(len(A0))])
    calls = []

    def values(t):
        return [float(np.interp(t, times, centers[:, j])) for j in range(3)] + [float(np.interp(t, times, currents))]

    def field(x, y, z, *, t=0):
        cx, cy, cz, cur = values(t)
        calls.append((t, cx, cy, cz, cur))
        # the reference's loop for 1 uA, lengths in um, in T m: mu_0 (1e-6 A) G; the run's current is dimensionless
        unit = np.asarray(em.current_loop_vector_potential(pos, loop_center=(cx, cy, cz), loop_radius=RADIUS, current=1.0,
                                                           length_units="um", current_units="uA"))
        a2 = A0 + cur * (unit[:, :2] / (em.mu_0 * 1e-6))
        return np.column_stack([a2, np.zeros(len(a2))])

    s, psi0, _ = gg.make_ref_solver(small, field(None, None, None, t=0)[:, :2], o, probe_points=probes)
    s.dynamic_vector_potential = True
    s.applied_vector_potential = field
    s.A_scale = 1.0
    s.edge_centers = small.edge_mesh.centers
    s.z0 = np.zeros(len(s.edge_centers))
    s.current_A_applied = field(None, None, None, t=0)[:, :2]
    assert np.all(np.isfinite(s.current_A_applied))
    s.operators.set_link_exponents(s.current_A_applied)
    del calls[:]
    out = gg.run_reference(s, psi0, o)
    c = np.array(calls)
    t = c[:, 0]
    assert len(t) == len(out["call_dt"]) and np.array_equal(t, out["call_time"])  # one evaluation per call of update()

    # ---- the run holds every kind of step ----------------------------------------------------------------------------
    moved = np.any(np.diff(np.vstack([values(0.0), c[:, 1:]]), axis=0) != 0, axis=1)
    hold = ~moved & (t > PATH_T[1]) & (t < WAVE_T[2])  # (path at rest, current on its plateau; both move again after)
    settled = ~moved & (t >= times[-1])
    counts = dict(moving=int(moved.sum()), joint_hold_longest_run=longest_run(hold), after_settling=int(settled.sum()))
    print("moving-loop calls:", len(t), counts, "max |J_s|", np.abs(out["final_supercurrent"]).max())
    assert counts["moving"] >= 10 and counts["joint_hold_longest_run"] >= 3 and counts["after_settling"] >= 3
    assert times[-1] < t[-1] and not np.any(np.isin(times, t))  # (the last node before the end; no step landed on a node)

    gg.save("traj_moving_loop_small", probe_points=np.array(probes), A0=A0, b0=B0, loop_times=times, loop_centers=centers,
            loop_currents=currents, loop_radius=RADIUS, call_loop_values=c[:, 1:], **gg.options_arrays(o), **out)


if __name__ == "__main__":
    main()
