"""solve_ensemble on the GPU: one replica of an ensemble reproduces each reference fixture at the tolerance of its
single-run test (tests/test_hip_parity.py), and every other replica -- other currents, fields, disorder, seeds --
matches ``tdgl.solve`` of that replica alone.  The single runs use the product's direct mu solve (the
``direct_solve`` fixture).  The replicas' inputs are chosen where tdgl.solve agrees with itself: on some weak-field
runs of these meshes (b = 0.05 - 0.1 on mesh_small, 0.005 - 0.02 on the 5k film) the direct and the iterative mu
solves of tdgl.solve already part after ~20 steps (different step counts), and so does the ensemble."""

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
    synthetic_mesh,
    uniform_field_A,
)

pytestmark = pytest.mark.gpu


def _options(g, **override):
    from tdgl_amd import SolverOptions

    o = options_from_golden(g, **override)
    return SolverOptions(
        solve_time=o.solve_time, skip_time=o.skip_time, dt_init=o.dt_init, dt_max=o.dt_max,
        adaptive=o.adaptive, adaptive_window=o.adaptive_window, max_solve_retries=o.max_solve_retries,
        adaptive_time_step_multiplier=o.adaptive_time_step_multiplier, save_every=o.save_every,
        terminal_psi=o.terminal_psi, pcg_rtol=1e-11,
    )


def _probes(g):
    return [int(p) for p in g["probe_points"]] if "probe_points" in g else None


def _single(g, mesh, A, eps=1.0, terminals=(), currents=None, **override):
    from tdgl_amd import TDGLSolver

    return TDGLSolver.from_dimensionless(mesh, _options(g, **override), A, eps, U_DEFAULT, GAMMA_DEFAULT,
                                         terminal_info=terminals, current_func=currents, probe_points=_probes(g)).solve()


def _ensemble(g, mesh, As, eps=1.0, terminals=(), currents=None, **override):
    from tdgl_amd.ensemble import solve_ensemble_dimensionless

    return solve_ensemble_dimensionless(mesh, _options(g, **override), As, eps, U_DEFAULT, GAMMA_DEFAULT,
                                        terminal_info=terminals, currents=currents, probe_points=_probes(g))


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


def _assert_like_single(ens, one, tol):
    """A replica of an ensemble against tdgl.solve of that replica alone."""
    assert ens.stats["mu_solver"] == "dense_ensemble"
    assert ens.stats["steps_thermalizing"] == one.stats["steps_thermalizing"]
    assert ens.stats["steps_simulating"] == one.stats["steps_simulating"]
    a, b = ens.dynamics, one.dynamics
    assert len(a.dt) == len(b.dt)
    assert max_abs(a.dt, b.dt) <= tol * b.dt.max()
    assert max_abs(a.time, b.time) <= tol * max(1.0, b.time.max())
    assert [s.step for s in ens.saved_steps] == [s.step for s in one.saved_steps]
    assert max_abs([s.time for s in ens.saved_steps], [s.time for s in one.saved_steps]) <= tol * max(1.0, one.saved_steps[-1].time)
    x, y = ens.tdgl_data, one.tdgl_data
    scale = max(1.0, np.abs(remove_mean(y.mu)).max())
    assert max_abs(np.abs(x.psi) ** 2, np.abs(y.psi) ** 2) < tol
    assert max_abs(remove_mean(x.mu), remove_mean(y.mu)) < tol * scale
    assert max_abs(x.supercurrent, y.supercurrent) < tol * max(1.0, np.abs(y.supercurrent).max())
    assert max_abs(x.normal_current, y.normal_current) < tol * max(1.0, np.abs(y.normal_current).max())
    if b.mu is not None and b.mu.shape[0] > 1:
        assert max_abs(a.mu[0] - a.mu[1], b.mu[0] - b.mu[1]) < tol * scale
        assert max_abs(np.exp(1j * (a.theta[0] - a.theta[1])), np.exp(1j * (b.theta[0] - b.theta[1]))) < tol


def test_transport_strip_currents_with_thermalisation(direct_solve):
    """traj_transport_strip (1e-9) as replica 0; zero current, half the current and one far above the depairing
    current (phase slips, a psi-update retry every few steps) as the others."""
    g = load_golden("traj_transport_strip")
    mesh = reference_mesh(load_golden("mesh_strip"))
    terms = [edge_terminal(mesh, "source", -30.0), edge_terminal(mesh, "drain", 30.0)]
    A = uniform_field_A(mesh, float(g["b"]))
    cur = float(g["current"])
    currents = [cur, 0.0, 0.5 * cur, 8 * cur]
    sols = _ensemble(g, mesh, A, terminals=terms, currents=[{"source": c, "drain": -c} for c in currents])
    n_sim = int((g["call_time"] == 0).nonzero()[0][-1])
    assert sols[0].stats["steps_thermalizing"] == n_sim
    _assert_like_fixture(g, sols[0], 1e-9, n_sim=n_sim)
    assert np.all(sols[0].tdgl_data.psi[g["fixed_sites"]] == 0)
    # (8x, phase slips: tdgl.solve itself moves by 3e-7 in dt between its direct and its iterative mu solve on this
    # run, and the probes' phase difference, which jumps by 2 pi at every slip, by more)
    for r, tol in ((1, 1e-9), (2, 1e-9), (3, 1e-4)):
        c = currents[r]
        one = _single(g, mesh, A, terminals=terms, currents={"source": c, "drain": -c})
        _assert_like_single(sols[r], one, tol)
    # the replicas took different numbers of steps
    steps = [s.stats["steps_thermalizing"] + s.stats["steps_simulating"] for s in sols]
    assert len(set(steps)) > 1


def test_field_small_fields_and_disorder(direct_solve):
    """traj_field_small (vortex entry, 5e-8) as replica 0; other fields and a position-dependent epsilon."""
    g = load_golden("traj_field_small")
    mesh = reference_mesh(load_golden("mesh_small"))
    b = float(g["b"])
    x = mesh.sites[:, 0]
    eps_dis = 1.0 - 0.3 * (x > np.median(x))
    fields = [b, 0.0, 0.35, 0.8, b]
    As = [uniform_field_A(mesh, f) for f in fields]
    eps = [1.0, 1.0, 1.0, 1.0, eps_dis]
    sols = _ensemble(g, mesh, As, eps)
    _assert_like_fixture(g, sols[0], 5e-8)
    for r in (1, 2, 3, 4):
        _assert_like_single(sols[r], _single(g, mesh, As[r], eps[r]), 5e-8)


def test_zero_field_5k_in_an_ensemble_of_eight(direct_solve):
    """traj_zero_field_5k (1e-12) as replicas 0 and 4 of eight; fields and a disordered epsilon in the others."""
    g = load_golden("traj_zero_field_5k")
    mesh = synthetic_mesh(70)
    fields = [0.0, 0.1, 0.2, 0.3, 0.0, 0.4, 0.5, 0.0]
    x = mesh.sites[:, 0]
    eps = [1.0] * 7 + [0.8 + 0.2 * np.cos(x / 7.0) ** 2]
    sols = _ensemble(g, mesh, [uniform_field_A(mesh, b) for b in fields], eps)
    assert len(sols) == 8
    _assert_like_fixture(g, sols[0], 1e-12)
    _assert_like_fixture(g, sols[4], 1e-12)
    # (disordered epsilon: tdgl.solve's direct and iterative mu solves differ by 1.4e-11 in |psi|^2 on this run)
    _assert_like_single(sols[7], _single(g, mesh, uniform_field_A(mesh, 0.0), eps[7]), 1e-10)


@pytest.mark.parametrize("R", [1, 33])
def test_replica_counts_off_the_tile_sizes(R, direct_solve):
    """R = 1 and R = 33 (not a multiple of the 16 replicas of a workgroup of the dense product).  Replica 16 sits in
    the second workgroup; it is bit for bit what an ensemble of one computes for it."""
    g = load_golden("traj_field_small")
    mesh = reference_mesh(load_golden("mesh_small"))
    fields = [0.35 + 0.45 * k / max(R - 1, 1) for k in range(R)]
    sols = _ensemble(g, mesh, [uniform_field_A(mesh, f) for f in fields])
    assert len(sols) == R
    for r in sorted({0, R - 1}):
        _assert_like_single(sols[r], _single(g, mesh, uniform_field_A(mesh, fields[r])), 5e-8)
    if R > 1:
        assert len({len(s.dynamics.dt) for s in sols}) > 1
        alone = _ensemble(g, mesh, uniform_field_A(mesh, fields[16]))[0]
        assert np.array_equal(alone.dynamics.dt, sols[16].dynamics.dt)
        assert np.array_equal(alone.tdgl_data.psi, sols[16].tdgl_data.psi)
        assert np.array_equal(alone.tdgl_data.mu, sols[16].tdgl_data.mu)


def test_public_interface_with_seed_solutions(direct_solve):
    """tdgl.solve_ensemble on a Device: a current sweep seeded per replica from the solutions of a first ensemble,
    against tdgl.solve with the same seed."""
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box

    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    film = tdgl.Polygon("film", points=box(4, 2))
    source = tdgl.Polygon("source", points=box(0.02, 2, center=(-2, 0)))
    drain = tdgl.Polygon("drain", points=box(0.02, 2, center=(2, 0)))
    device = tdgl.Device("strip", layer=layer, film=film, terminals=[source, drain], probe_points=[(-1.5, 0), (1.5, 0)],
                         length_units="um")
    device.make_mesh(max_edge_length=0.15)
    opts = tdgl.SolverOptions(solve_time=8, skip_time=2, field_units="mT", current_units="uA", save_every=50)
    currents = [dict(source=i, drain=-i) for i in (0.0, 2.0, 4.0)]
    first = tdgl.solve_ensemble(device, opts, terminal_currents=currents)
    assert len(first) == 3
    second = tdgl.solve_ensemble(device, opts, terminal_currents=currents, seed_solutions=first)
    for r in range(3):
        one = tdgl.solve(device, opts, terminal_currents=currents[r], seed_solution=first[r])
        _assert_like_single(second[r], one, 1e-9)
        assert np.isfinite(second[r].dynamics.mean_voltage())
    assert second[2].dynamics.mean_voltage() != second[0].dynamics.mean_voltage()


def test_retry_budget_exhaustion_raises_with_the_replica_index():
    g = load_golden("traj_retry_small")
    mesh = reference_mesh(load_golden("mesh_small"))
    A = uniform_field_A(mesh, float(g["b"]))
    with pytest.raises(RuntimeError, match=r"replica 0: Solver failed to converge in 10 retries at step 0 with dt = 2.00e\+00"):
        _ensemble(g, mesh, [A, A], adaptive=False)
