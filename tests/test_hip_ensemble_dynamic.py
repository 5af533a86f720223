"""solve_ensemble with time-dependent replicas on the GPU: field ramps (LinearRamp x static A), tabulated terminal
currents (TabulatedCurrents) and separable disorder (SeparableEpsilon), each replica with its own parameters and all
evaluated on the device.  One replica reproduces a reference fixture at the tolerance of its single-run test
(tests/test_hip_parity.py); the others match tdgl.solve (TDGLSolver.from_dimensionless) of that replica alone; a
replica of a mixed ensemble of 33 is bit for bit what an ensemble of one computes for it."""

import numpy as np
import pytest

from conftest import load_golden
from helpers import (
    GAMMA_DEFAULT,
    U_DEFAULT,
    align_phase,
    edge_terminal,
    max_abs,
    options_from_golden,
    reference_mesh,
    remove_mean,
    uniform_field_A,
)

pytestmark = pytest.mark.gpu


def _options(g, **override):
    from tdgl_amd import SolverOptions

    pcg_rtol = override.pop("pcg_rtol", 1e-11)
    o = options_from_golden(g, **override)
    return SolverOptions(
        solve_time=o.solve_time, skip_time=o.skip_time, dt_init=o.dt_init, dt_max=o.dt_max,
        adaptive=o.adaptive, adaptive_window=o.adaptive_window, max_solve_retries=o.max_solve_retries,
        adaptive_time_step_multiplier=o.adaptive_time_step_multiplier, save_every=o.save_every,
        terminal_psi=o.terminal_psi, pcg_rtol=pcg_rtol,
    )


def _probes(g):
    return [int(p) for p in g["probe_points"]] if "probe_points" in g else None


def _ramp_value(ramp, t):
    from tdgl_amd import LinearRamp

    return LinearRamp(**ramp).scalar(t)


def _assert_like_fixture(g, sol, tol, n_sim=None):
    """tests/test_hip_parity.py::_assert_hip_trajectory"""
    dyn = sol.dynamics
    want_dt = g["call_dt"] if n_sim is None else g["call_dt"][n_sim:]
    assert len(dyn.dt) == len(want_dt)
    assert max_abs(dyn.dt, want_dt) <= tol * want_dt.max()
    last = sol.tdgl_data
    assert max_abs(np.abs(last.psi) ** 2, np.abs(g["final_psi"]) ** 2) < tol
    assert max_abs(last.supercurrent, g["final_supercurrent"]) < tol
    assert max_abs(last.normal_current, g["final_normal_current"]) < tol
    scale = max(1.0, np.abs(remove_mean(g["final_mu"])).max())
    assert max_abs(remove_mean(last.mu), remove_mean(g["final_mu"])) < tol * scale
    assert max_abs(align_phase(last.psi, g["final_psi"]), g["final_psi"]) < tol
    if "call_mu_probe" in g and dyn.mu is not None and dyn.mu.shape[0] > 1:
        want_mu = g["call_mu_probe"] if n_sim is None else g["call_mu_probe"][n_sim:]
        assert max_abs(dyn.mu[0] - dyn.mu[1], want_mu[:, 0] - want_mu[:, 1]) < tol * scale
        want_th = g["call_theta_probe"] if n_sim is None else g["call_theta_probe"][n_sim:]
        assert max_abs(np.exp(1j * (dyn.theta[0] - dyn.theta[1])), np.exp(1j * (want_th[:, 0] - want_th[:, 1]))) < tol
    assert [s.step for s in sol.saved_steps] == list(g["save_step"])
    assert max_abs([s.time for s in sol.saved_steps], g["save_time"]) <= tol * max(1.0, g["save_time"].max())


def _assert_like_single(ens, one, tol, dt_tol=None):
    """A replica of an ensemble against tdgl.solve of that replica alone."""
    dt_tol = tol if dt_tol is None else dt_tol
    assert ens.stats["mu_solver"] == "dense_ensemble"
    assert ens.stats["steps_thermalizing"] == one.stats["steps_thermalizing"]
    assert ens.stats["steps_simulating"] == one.stats["steps_simulating"]
    assert ens.dynamic_vector_potential == one.dynamic_vector_potential
    assert ens.dynamic_epsilon == one.dynamic_epsilon
    a, b = ens.dynamics, one.dynamics
    assert len(a.dt) == len(b.dt)
    assert max_abs(a.dt, b.dt) <= dt_tol * b.dt.max()
    assert max_abs(a.time, b.time) <= dt_tol * max(1.0, b.time.max())
    assert [s.step for s in ens.saved_steps] == [s.step for s in one.saved_steps]
    assert max_abs([s.time for s in ens.saved_steps], [s.time for s in one.saved_steps]) <= dt_tol * max(1.0, one.saved_steps[-1].time)
    x, y = ens.tdgl_data, one.tdgl_data
    scale = max(1.0, np.abs(remove_mean(y.mu)).max())
    assert max_abs(np.abs(x.psi) ** 2, np.abs(y.psi) ** 2) < tol
    assert max_abs(remove_mean(x.mu), remove_mean(y.mu)) < tol * scale
    assert max_abs(x.supercurrent, y.supercurrent) < tol * max(1.0, np.abs(y.supercurrent).max())
    assert max_abs(x.normal_current, y.normal_current) < tol * max(1.0, np.abs(y.normal_current).max())
    if b.mu is not None and b.mu.shape[0] > 1:
        # (relative to the probe voltage itself: while a field ramps it is far larger than the final mu)
        assert max_abs(a.mu[0] - a.mu[1], b.mu[0] - b.mu[1]) < tol * max(scale, np.abs(b.mu[0] - b.mu[1]).max())
        assert max_abs(np.exp(1j * (a.theta[0] - a.theta[1])), np.exp(1j * (b.theta[0] - b.theta[1]))) < tol
    # (saved A and epsilon are those at the time of the last step taken, which agree to dt_tol)
    for s, t in zip(ens.saved_steps, one.saved_steps):
        assert max_abs(s.applied_vector_potential, t.applied_vector_potential) < dt_tol * max(1.0, np.abs(t.applied_vector_potential).max())
        assert max_abs(s.epsilon, t.epsilon) < dt_tol


def test_field_ramps_with_lagging_links(direct_solve):
    """traj_dynamic_lag (A moves by less than np.allclose's tolerance per step: dA/dt follows, the links lag) as
    replica 0 at its single-run tolerance (1e-8); other end fields and ramp times, one ramp that settles a quarter of
    the way through the run, and a static replica, each against TDGLSolver.from_dimensionless with the same ramp."""
    from tdgl_amd import TDGLSolver
    from tdgl_amd.ensemble import solve_ensemble_dimensionless

    g = load_golden("traj_dynamic_lag")
    mesh = reference_mesh(load_golden("mesh_small"))
    opts = _options(g, adaptive=False, pcg_rtol=1e-12)
    A_base = g["A_base"]
    ramp = {k: float(g["ramp_" + k]) for k in ("tmin", "tmax", "initial", "final")}
    ramps = [ramp, dict(ramp, final=32.0), dict(ramp, tmax=0.5), dict(ramp, tmax=1.0, final=30.5), None]
    assert ramps[2]["tmax"] < opts.solve_time / 2
    As = [None, None, None, None, 30.0 * A_base]
    vpr = [None if r is None else (A_base, r) for r in ramps]
    sols = solve_ensemble_dimensionless(mesh, opts, As, 1.0, U_DEFAULT, GAMMA_DEFAULT, probe_points=_probes(g),
                                        vector_potential_ramp=vpr)
    _assert_like_fixture(g, sols[0], 1e-8)
    assert max_abs(sols[0].tdgl_data.applied_vector_potential, _ramp_value(ramp, float(g["call_time"][-1])) * A_base) < 1e-12
    for r in range(len(ramps)):
        sol = sols[r]
        assert sol.dynamic_vector_potential == (ramps[r] is not None)
        if ramps[r] is not None:
            t_last = float(sol.dynamics.time[-1])
            assert max_abs(sol.tdgl_data.applied_vector_potential, _ramp_value(ramps[r], t_last) * A_base) < 1e-12
        A0 = 30.0 * A_base if ramps[r] is None else _ramp_value(ramps[r], 0.0) * A_base
        one = TDGLSolver.from_dimensionless(mesh, opts, A0, 1.0, U_DEFAULT, GAMMA_DEFAULT, probe_points=_probes(g),
                                            vector_potential_ramp=vpr[r]).solve()
        _assert_like_single(sol, one, 1e-8)
    # the settled ramp holds its end value
    assert max_abs(sols[2].tdgl_data.applied_vector_potential, 31.0 * A_base) == 0.0


def test_tabulated_currents_per_replica(direct_solve):
    """traj_transport_ramp driven by TabulatedCurrents as replica 0 (first 65 dt at 1e-6 and the saved steps, as
    test_tabulated_currents_and_epsilon_run_inside_the_time_loop: the run sits at the stability edge of the scheme);
    other slopes and a rising-then-falling table against the single run of the same table."""
    from tdgl_amd import TDGLSolver
    from tdgl_amd.ensemble import solve_ensemble_dimensionless
    from tdgl_amd.parameter import TabulatedCurrents

    g = load_golden("traj_transport_ramp")
    mesh = reference_mesh(load_golden("mesh_strip"))
    terms = [edge_terminal(mesh, "source", -30.0), edge_terminal(mesh, "drain", 30.0)]
    opts = _options(g)
    A = uniform_field_A(mesh, 0.0)

    def table(times, values):
        return TabulatedCurrents(times, dict(source=list(values), drain=[-v for v in values]))

    tables = [
        table([0.0, 8.0, 1e9], [0.0, 4.0, 4.0]),
        table([0.0, 8.0, 1e9], [0.0, 1.0, 1.0]),
        table([0.0, 6.0], [0.0, 2.0]),
        table([0.0, 3.0, 6.0, 9.0], [0.0, 1.5, 0.5, 0.0]),  # rising, then falling
    ]
    sols = solve_ensemble_dimensionless(mesh, opts, A, 1.0, U_DEFAULT, GAMMA_DEFAULT, terminal_info=terms,
                                        currents=tables, probe_points=_probes(g))
    s0 = sols[0]
    assert max_abs(s0.dynamics.dt[:65], g["call_dt"][:65]) <= 1e-6 * g["call_dt"].max()
    assert [s.step for s in s0.saved_steps] == list(g["save_step"])
    # Tolerances: the measured agreement of tdgl.solve's own direct and iterative mu solves on these tables, which is
    # looser than 1e-9.  Both pairs first differ at step 38 - 41 and then part at the same rate: max |dt| / dt_max
    # 1.7e-4 / 2.4e-5 / 4.1e-3 (direct vs iterative) and 1.0e-4 / 1.6e-4 / 3.6e-3 (ensemble vs direct) for
    # replicas 1 / 2 / 3, final |psi|^2 up to 4e-5 in both; over the first 65 steps both stay below 1e-8.
    for r in (1, 2, 3):
        one = TDGLSolver.from_dimensionless(mesh, opts, A, 1.0, U_DEFAULT, GAMMA_DEFAULT, terminal_info=terms,
                                            current_func=tables[r], probe_points=_probes(g)).solve()
        a, b = sols[r], one
        assert a.stats["steps_simulating"] == b.stats["steps_simulating"]
        assert [s.step for s in a.saved_steps] == [s.step for s in b.saved_steps]
        assert max_abs(a.dynamics.dt[:65], b.dynamics.dt[:65]) <= 2e-8 * b.dynamics.dt.max()
        assert max_abs(a.dynamics.dt, b.dynamics.dt) <= 1e-2 * b.dynamics.dt.max()
        assert max_abs(np.abs(a.tdgl_data.psi) ** 2, np.abs(b.tdgl_data.psi) ** 2) < 1e-4
    assert sols[3].dynamics.mean_voltage() != sols[1].dynamics.mean_voltage()


def test_separable_epsilon_per_replica(direct_solve):
    """The hot stripe of the parity test switched by three different factor tables, one per replica."""
    from tdgl_amd import SolverOptions, TDGLSolver
    from tdgl_amd.ensemble import solve_ensemble_dimensionless
    from tdgl_amd.parameter import PiecewiseLinear

    small = reference_mesh(load_golden("mesh_small"))
    static = np.where(np.abs(small.sites[:, 0]) < 2.0, 1.0, 0.4)
    factors = [([0.0, 1.0, 2.0], [1.0, 0.2, 0.9]), ([0.0, 1.0, 2.0], [1.0, 0.6, 1.0]), ([0.0, 0.5, 2.5], [0.7, 1.0, 0.3])]
    opts = SolverOptions(solve_time=3.0, dt_init=1e-3, save_every=50, pcg_rtol=1e-11)
    A = uniform_field_A(small, 0.3)
    sols = solve_ensemble_dimensionless(small, opts, A, 1.0, U_DEFAULT, GAMMA_DEFAULT,
                                        epsilon_table=[(static, t, f) for t, f in factors])
    for r, (times, values) in enumerate(factors):
        f = PiecewiseLinear(times, values)
        one = TDGLSolver.from_dimensionless(small, opts, A, static * f(0.0))
        one._eps_table = (static, f.times, f.values)  # (as the parity test sets the single run up)
        one.epsilon_func, one.dynamic_epsilon = (lambda t, f=f: f(t) * static), True
        one.ctx.set_epsilon_table(static, f.times, f.values)
        one._epsilon_on_device = True
        b = one.solve()
        a = sols[r]
        assert a.dynamic_epsilon
        assert len(a.dynamics.dt) == len(b.dynamics.dt)
        dev = (max_abs(a.dynamics.dt, b.dynamics.dt) / b.dynamics.dt.max(), max_abs(np.abs(a.tdgl_data.psi) ** 2, np.abs(b.tdgl_data.psi) ** 2))
        print(f"separable epsilon, replica {r}: dt {dev[0]:.2e}, |psi|^2 {dev[1]:.2e}")
        # (dt: measured 9e-11 / 9e-11 / 2.3e-9, |psi|^2 2e-10 / 7e-11 / 1.6e-9 for replicas 0 / 1 / 2: the dense product's
        # different order of sums, grown over the adaptive run)
        assert dev[0] <= 1e-8
        assert dev[1] < 1e-8
        assert [s.step for s in a.saved_steps] == [s.step for s in b.saved_steps]
        # the saved epsilon is the factor at the replica's own time of the last step taken ...
        last = a.saved_steps[-1]
        assert max_abs(last.epsilon, f(last.time) * static) < 1e-12
        # ... and that time agrees with the single run's to the dt tolerance
        for x, y in zip(a.saved_steps, b.saved_steps):
            assert max_abs(x.epsilon, y.epsilon) < 1e-8
    assert max_abs(sols[0].tdgl_data.epsilon, sols[2].tdgl_data.epsilon) > 0.1


def test_mixed_ensemble_of_33_is_bit_identical_to_ensembles_of_one(direct_solve):
    """Static, ramped, tabulated, separable-epsilon and tabulated + separable-epsilon replicas in one ensemble that
    crosses the 16-replica workgroup of the dense product, with a thermalisation stage (the ramps start again at the
    simulation stage).  Replicas 16 .. 20, one of each kind, are bit for bit what an ensemble of one computes."""
    from tdgl_amd.ensemble import solve_ensemble_dimensionless
    from tdgl_amd.parameter import TabulatedCurrents

    g = load_golden("traj_transport_strip")
    mesh = reference_mesh(load_golden("mesh_strip"))
    terms = [edge_terminal(mesh, "source", -30.0), edge_terminal(mesh, "drain", 30.0)]
    opts = _options(g, solve_time=6.0, skip_time=1.0)
    cur = float(g["current"])
    A_base = uniform_field_A(mesh, 0.05)
    x = mesh.sites[:, 0]
    R = 33
    As, ramps, currents, eps_tables = [], [], [], []
    for r in range(R):
        k, s = r % 5, 0.5 + r / R
        As.append(A_base if k != 1 else None)
        ramps.append((A_base, dict(tmin=0.0, tmax=2.0 * s, initial=0.0, final=2.0 * s)) if k == 1 else None)
        if k in (2, 4):
            currents.append(TabulatedCurrents([0.0, 3.0 * s, 1e9], dict(source=[0.0, s * cur, s * cur], drain=[0.0, -s * cur, -s * cur])))
        else:
            currents.append({"source": s * cur, "drain": -s * cur})
        eps_tables.append((1.0 - 0.3 * (x > 0), [0.0, 2.0 * s], [1.0, 0.6]) if k in (3, 4) else None)

    def run(idx):
        return solve_ensemble_dimensionless(mesh, opts, [As[i] for i in idx], 1.0, U_DEFAULT, GAMMA_DEFAULT,
                                            terminal_info=terms, currents=[currents[i] for i in idx],
                                            probe_points=_probes(g), vector_potential_ramp=[ramps[i] for i in idx],
                                            epsilon_table=[eps_tables[i] for i in idx])

    sols = run(range(R))
    assert len(sols) == R
    assert len({len(s.dynamics.dt) for s in sols}) > 1
    for r in (16, 17, 18, 19, 20):
        alone = run([r])[0]
        a, b = alone, sols[r]
        assert np.array_equal(a.dynamics.dt, b.dynamics.dt)
        assert np.array_equal(a.tdgl_data.psi, b.tdgl_data.psi)
        assert np.array_equal(a.tdgl_data.mu, b.tdgl_data.mu)
        assert np.array_equal(a.tdgl_data.normal_current, b.tdgl_data.normal_current)
        assert np.array_equal(a.tdgl_data.applied_vector_potential, b.tdgl_data.applied_vector_potential)
        assert np.array_equal(a.tdgl_data.epsilon, b.tdgl_data.epsilon)


def _strip_device():
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box

    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    film = tdgl.Polygon("film", points=box(4, 2))
    source = tdgl.Polygon("source", points=box(0.02, 2, center=(-2, 0)))
    drain = tdgl.Polygon("drain", points=box(0.02, 2, center=(2, 0)))
    device = tdgl.Device("strip", layer=layer, film=film, terminals=[source, drain], probe_points=[(-1.5, 0), (1.5, 0)],
                         length_units="um")
    device.make_mesh(max_edge_length=0.15)
    return device


def test_public_interface_field_ramps_and_current_tables(direct_solve):
    """tdgl.solve_ensemble on a Device with LinearRamp x ConstantField fields and TabulatedCurrents, against
    tdgl.solve per replica."""
    import tdgl_amd as tdgl
    from tdgl_amd.parameter import TabulatedCurrents

    device = _strip_device()
    opts = tdgl.SolverOptions(solve_time=8, skip_time=1, field_units="mT", current_units="uA", save_every=50)
    fields = [tdgl.LinearRamp(tmin=0, tmax=4) * tdgl.ConstantField(b, field_units="mT", length_units="um") for b in (0.5, 2.0, 5.0)]
    sols = tdgl.solve_ensemble(device, opts, applied_vector_potential=fields + [0.5])
    assert len(sols) == 4
    for r in range(4):
        one = tdgl.solve(device, opts, applied_vector_potential=(fields + [0.5])[r])
        _assert_like_single(sols[r], one, 1e-9)
        assert sols[r].dynamic_vector_potential == (r < 3)
    assert max_abs(sols[2].tdgl_data.applied_vector_potential, 0.0) > 0.0
    tables = [TabulatedCurrents([0.0, 4.0, 1e9], dict(source=[0.0, i, i], drain=[0.0, -i, -i])) for i in (1.0, 3.0)]
    tables.append(TabulatedCurrents([0.0, 2.0, 4.0, 6.0], dict(source=[0.0, 3.0, 1.0, 0.0], drain=[0.0, -3.0, -1.0, 0.0])))
    sols = tdgl.solve_ensemble(device, opts, terminal_currents=tables)
    for r in range(3):
        one = tdgl.solve(device, opts, terminal_currents=tables[r])
        _assert_like_single(sols[r], one, 1e-9)
        assert np.isfinite(sols[r].dynamics.mean_voltage())
