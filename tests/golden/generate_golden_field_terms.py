"""Generate `traj_field_terms_small.npz` by running the REFERENCE itself (build container only).

    python tests/golden/generate_golden_field_terms.py [--out DIR]

A sum of a static field and two time-scaled ones on mesh_small, A(t) = A_0 + f_1(t) A_1 + f_2(t) A_2, given to the
reference's `TDGLSolver.update` as one time-dependent `applied_vector_potential` (as `generate_golden.gen_dynamic_lag`
does for a single ramp):

    A_0  a uniform field,
    A_1  a uniform field of another strength, f_1 a two-node ramp,
    A_2  the vector potential of a Gaussian flux spot off centre, A_phi = Phi / (2 pi r) (1 - exp(-r^2 / 2 sigma^2)),
         f_2 a table: up, a hold longer than three steps at dt_max, down through zero.

The nodes are chosen so that the two factors stop moving at different times and both before the run ends, and the script
asserts that the run holds every kind of step the sum's step rule tells apart.  The file stores the bases, the nodes,
what `run_reference` returns and the factors of every call.  Data only (no reference source text).
"""

import numpy as np

import generate_golden as gg

B0, B1 = 0.1, 0.15                      # A_0, A_1: uniform fields
RAMP = dict(tmin=0.21, tmax=1.0, initial=0.0, final=1.0)
SPOT = dict(x=3.0, y=-2.0, sigma=2.0, flux=5.0)  # (peak field flux / (2 pi sigma^2) = 0.2)
TIMES = [0.6, 1.3, 2.2, 3.1]            # f_2: up while f_1 still ramps, hold 0.9 (eighteen steps of dt_max), down through zero
VALUES = [0.0, 1.0, 1.0, -0.6]
SOLVE_TIME = 4.0


def flux_spot_A(mesh, x, y, sigma, flux):
    c = mesh.edge_mesh.centers
    dx, dy = c[:, 0] - x, c[:, 1] - y
    r2 = dx * dx + dy * dy
    # A_phi / r (-> flux / (4 pi sigma^2) at the centre)
    g = np.where(r2 > 1e-24, flux / (2 * np.pi * np.maximum(r2, 1e-24)) * -np.expm1(-r2 / (2 * sigma**2)), flux / (4 * np.pi * sigma**2))
    return np.column_stack([-g * dy, g * dx])


def ramp_value(t):
    if t < RAMP["tmin"]:
        return RAMP["initial"]
    if t < RAMP["tmax"]:
        return RAMP["initial"] + (RAMP["final"] - RAMP["initial"]) * (t - RAMP["tmin"]) / (RAMP["tmax"] - RAMP["tmin"])
    return RAMP["final"]


def table_value(t):
    return float(np.interp(t, TIMES, VALUES))


def longest_run(mask):
    best = run = 0
    for v in mask:
        run = run + 1 if v else 0
        best = max(best, run)
    return best


def main():
    small = gg.make_ref_mesh(20, 20)  # mesh_small
    # dt_max = 0.05: with adaptive steps up to 0.1 this run amplifies a 1e-14 perturbation of psi_0 to 7e-8 in J_s and J_n
    # (the CPU oracle against itself, 67 steps) and no second implementation can be held to 1e-8; up to 0.05 it moves by
    # 2e-11 (93 steps), as it does at 0.02, 0.01 and with a fixed step of 0.01
    o = gg.SolverOptions(solve_time=SOLVE_TIME, dt_init=1e-3, dt_max=0.05, save_every=50)
    probes = [small.closest_site((-5, 0)), small.closest_site((5, 0))]
    A0, A1 = gg.uniform_field_A(small, B0), gg.uniform_field_A(small, B1)
    A2 = flux_spot_A(small, **SPOT)
    factors = []

    def field(x, y, z, *, t=0):
        f1, f2 = ramp_value(t), table_value(t)
        factors.append((t, f1, f2))
        a2 = A0 + f1 * A1 + f2 * A2
        return np.column_stack([a2, np.zeros(len(a2))])

    s, psi0, _ = gg.make_ref_solver(small, field(None, None, None, t=0)[:, :2], o, probe_points=probes)
    s.dynamic_vector_potential = True
    s.applied_vector_potential = field
    s.A_scale = 1.0
    s.edge_centers = small.edge_mesh.centers
    s.z0 = np.zeros(len(s.edge_centers))
    s.current_A_applied = field(None, None, None, t=0)[:, :2]
    s.operators.set_link_exponents(s.current_A_applied)
    del factors[:]
    out = gg.run_reference(s, psi0, o)
    t, f1, f2 = (np.array(c) for c in zip(*factors))
    assert len(t) == len(out["call_dt"]) and np.array_equal(t, out["call_time"])  # one evaluation per call of update()

    # ---- the run holds every kind of step ----------------------------------------------------------------------------
    m1 = np.diff(np.concatenate([[ramp_value(0.0)], f1])) != 0
    m2 = np.diff(np.concatenate([[table_value(0.0)], f2])) != 0
    t_end = max(RAMP["tmax"], TIMES[-1])
    assert RAMP["tmax"] != TIMES[-1] and t_end < t[-1]
    only1, only2, both, neither = m1 & ~m2, ~m1 & m2, m1 & m2, ~m1 & ~m2
    joint_hold = neither & (t > RAMP["tmax"]) & (t < TIMES[2])  # (both have moved before, the table moves again after)
    settled = neither & (t >= t_end)
    counts = dict(only_term_1=int(only1.sum()), only_term_2=int(only2.sum()), both=int(both.sum()),
                  joint_hold_longest_run=longest_run(joint_hold), after_settling=int(settled.sum()))
    print("field-terms calls:", len(t), counts, "max |J_s|", np.abs(out["final_supercurrent"]).max())
    assert counts["only_term_1"] > 0 and counts["only_term_2"] > 0 and counts["both"] > 0
    assert counts["joint_hold_longest_run"] >= 3
    assert counts["after_settling"] >= 3  # (two evaluations at the end values, then settled steps)
    assert not np.any(np.isin(TIMES + [RAMP["tmin"], RAMP["tmax"]], t))  # (no step landed on a node)

    gg.save("traj_field_terms_small", probe_points=np.array(probes), A0=A0, A1=A1, A2=A2, b0=B0, b1=B1,
            **{"ramp_" + k: v for k, v in RAMP.items()}, **{"spot_" + k: v for k, v in SPOT.items()},
            table_times=np.array(TIMES), table_values=np.array(VALUES), call_f1=f1, call_f2=f2,
            **gg.options_arrays(o), **out)


if __name__ == "__main__":
    main()
