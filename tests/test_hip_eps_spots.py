"""Gaussian hot spots in epsilon(r, t) evaluated on the device (tdgl_set_epsilon_spots, k_eps_spots), on mesh_small: 516
sites -- three workgroups, the last one holding four lanes -- with the direct mu solve.  The values against the NumPy model
(tests/eps_spots_model.py) at a derived bound, the reference's moving-spot fixture in both time loops and their agreement to
the last bit, the device path against the per-step callable, the setters and getters, a mixed ensemble, and the example."""

import os
import subprocess
import sys

import numpy as np
import pytest

import eps_spots_model as model
from conftest import load_golden
from helpers import GAMMA_DEFAULT, U_DEFAULT, max_abs, options_from_golden, reference_mesh, uniform_field_A
from test_hip_parity import _assert_hip_trajectory

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the fixture's spot: epsilon = 1 - 0.6 exp(-|r - c(t)|^2 / 4), c(t) = (-6 + 1.5 t, 1); the nodes reach past its last call
FIXTURE_SPOT = dict(times=[0.0, 16.0], centers=[[-6.0, 1.0], [18.0, 1.0]], amplitudes=0.6, sigmas=np.sqrt(2.0))
RAMP = dict(tmin=0.0, tmax=5.0, initial=0.0, final=1.0)  # min(t / 5, 1), the fixture's field ramp


def _small():
    return reference_mesh(load_golden("mesh_small"))


def _static_solver(mesh, eps=1.0, **kw):
    from tdgl_amd import SolverOptions, TDGLSolver

    opts = SolverOptions(solve_time=1e9, dt_init=1e-3, dt_max=0.1, save_every=10**6, pcg_rtol=1e-11)
    return TDGLSolver.from_dimensionless(mesh, opts, uniform_field_A(mesh, 0.3), eps, U_DEFAULT, GAMMA_DEFAULT, **kw)


def _spot(k):
    """K placeholder spots to be moved by update_epsilon_spots."""
    return [dict(times=[0.0], centers=[[0.0, 0.0]], amplitudes=0.0, sigmas=1.0)] * k


def test_values_against_the_model(direct_solve):
    """update_epsilon_spots at eleven value sets with K = 1, 2 and 4, read back with tdgl_get_epsilon.  Per site
    |eps_dev - eps_model| <= 8 * 2^-52 * (1 + sum a_k) -- derived, not measured (eps_spots_model.value_bound: 3 ulp of the
    device's exp, as many for NumPy's, the products' and the K subtractions' roundings); epsilon is exactly eps0 wherever
    every a_k = 0.  cx != cy in every set and eps0 varies from site to site, so a swap of x and y or a missing site permutation
    moves epsilon by far more than the bound (checked on the model below).  Measured worst: see the printed line
    (DESIGN.md section 3 quotes it)."""
    mesh = _small()
    sites = mesh.sites
    n = len(sites)
    assert n == 516
    eps0 = 0.3 + 0.7 * np.cos(0.37 * np.arange(n)) ** 2  # in [0.3, 1], different at every site
    on_site = sites[333]
    sets = {
        1: [[[3.0, -4.5, 0.6, 1.5]],                      # inside the mesh
            [[14.0, -12.5, 0.9, 3.0]],                    # outside it
            [[on_site[0], on_site[1], 0.35, 0.8]],        # exactly on a site: d2 = 0 there
            [[-2.25, 6.5, 0.0, 1.0]],                     # a = 0
            [[1.5, -7.0, 0.002, 0.05]]],                  # a and sigma three decades down: narrower than the mesh spacing
        2: [[[3.0, -4.5, 0.6, 1.5], [-6.0, 2.0, 0.004, 12.0]],
            [[on_site[0], on_site[1], 1.0, 0.03], [25.0, -1.0, 0.5, 30.0]],
            [[-2.25, 6.5, 0.0, 1.0], [4.0, 8.5, 0.0, 0.01]]],      # every a = 0
        4: [[[3.0, -4.5, 0.6, 1.5], [-6.0, 2.0, 0.004, 12.0], [7.5, 7.0, 0.05, 0.4], [-8.0, -9.5, 0.3, 2.5]],
            [[0.5, -0.25, 1.0, 20.0], [-11.0, 3.0, 0.001, 0.02], [on_site[0], on_site[1], 0.0, 0.5], [9.0, -9.5, 0.07, 5.0]],
            [[1.0, -2.0, 0.0, 1.0], [2.0, -3.0, 0.0, 2.0], [3.0, -4.0, 0.0, 3.0], [4.0, -5.0, 0.0, 4.0]]],
    }
    worst = (0.0, 0.0)
    for K, value_sets in sets.items():
        solver = _static_solver(mesh, epsilon_spots=(eps0, _spot(K)))
        ctx = solver.ctx
        assert not np.array_equal(ctx.perm, np.arange(n))  # (the context reorders the sites)
        assert np.array_equal(ctx.epsilon(), eps0)  # a = 0 at t = 0
        for values in value_sets:
            v = np.array(values)
            assert np.all(v[:, 0] != v[:, 1])
            ctx.update_epsilon_spots(v)
            assert np.array_equal(ctx.epsilon_spot_values(), v)
            got, want = ctx.epsilon(), model.epsilon(sites, eps0, v)
            err, bound = float(np.abs(got - want).max()), float(model.value_bound(v))
            worst = max(worst, (err / bound, err))
            print(f"K = {K}, sum a = {v[:, 2].sum():.3f}: max |eps_dev - eps_model| = {err:.3e}, bound {bound:.3e}")
            assert np.all(np.abs(got - want) <= bound)
            if np.all(v[:, 2] == 0):
                assert np.array_equal(got, eps0)
            elif v[:, 2].max() * np.exp(-0.5 * (3.0 / v[:, 3].min()) ** 2) > 1e-6:  # (a spot wider than a needle)
                # what a swap of x and y, or sites and eps0 left in the caller's order, would give: far from the model
                perm = ctx.perm
                assert np.abs(model.epsilon(sites[:, ::-1], eps0, v) - want).max() > 1e3 * bound
                assert np.abs(model.epsilon(sites[perm], eps0[perm], v) - want).max() > 1e3 * bound
        ctx.close()
    print(f"worst over all value sets: {worst[1]:.3e} ({worst[0]:.3f} of the bound)")


_RUNS = {}


def _fixture_runs():
    """traj_dynamic_small with the ramp as vector_potential_ramp and the spot as epsilon_spots, once per loop, and the same
    HotSpotEpsilon down the per-step callable path; computed once and shared by the tests below (which leave it unchanged)."""
    if _RUNS:
        return _RUNS
    from tdgl_amd import HotSpot, HotSpotEpsilon, SolverOptions, TDGLSolver

    g = load_golden("traj_dynamic_small")
    mesh = _small()
    o = options_from_golden(g)
    opts = SolverOptions(solve_time=o.solve_time, dt_init=o.dt_init, dt_max=o.dt_max, save_every=o.save_every, pcg_rtol=1e-11)
    A_full = g["A_full"]
    kw = dict(probe_points=[int(p) for p in g["probe_points"]], vector_potential_ramp=(A_full, RAMP))
    source = HotSpotEpsilon(1.0, [HotSpot(**FIXTURE_SPOT)])
    saved = os.environ.pop("TDGL_NO_RUN_AHEAD", None)
    try:
        for mode in ("run_ahead", "classic", "callable"):
            if mode == "classic":
                os.environ["TDGL_NO_RUN_AHEAD"] = "1"
            else:
                os.environ.pop("TDGL_NO_RUN_AHEAD", None)
            if mode == "callable":
                solver = TDGLSolver.from_dimensionless(mesh, opts, 0.0 * A_full, source(mesh.sites, t=0.0), U_DEFAULT, GAMMA_DEFAULT,
                                                       epsilon_func=lambda t: source(mesh.sites, t=t), **kw)
                assert not solver.device_evaluates_epsilon()
            else:
                solver = TDGLSolver.from_dimensionless(mesh, opts, 0.0 * A_full, 1.0, U_DEFAULT, GAMMA_DEFAULT,
                                                       epsilon_spots=(1.0, [FIXTURE_SPOT]), **kw)
                assert solver.device_evaluates_epsilon() and solver.device_evaluates_field()
            assert solver.ctx.dense_direct
            solver.ctx.step_stats(reset=True)
            sol = solver.solve()
            _RUNS[mode] = dict(sol=sol, stats=solver.ctx.step_stats(), state=solver.ctx.get_state(), eps=solver.ctx.epsilon(),
                               values=solver.ctx.epsilon_spot_values(), loop=solver.ctx.loop_state())
            solver.ctx.close()
    finally:
        os.environ.pop("TDGL_NO_RUN_AHEAD", None)
        if saved is not None:
            os.environ["TDGL_NO_RUN_AHEAD"] = saved
    _RUNS["g"] = g
    return _RUNS


@pytest.mark.parametrize("mode", ["run_ahead", "classic"])
def test_fixture_in_both_loops(direct_solve, mode):
    """The reference's trajectory with a ramped field and a moving hot spot (265 steps), the spot evaluated on the device:
    the assertions and the tolerance of test_hip_parity.py::test_trajectory_time_dependent_field_and_epsilon."""
    runs = _fixture_runs()
    g, run = runs["g"], runs[mode]
    _assert_hip_trajectory(g, run["sol"], 1e-7)
    steps = len(g["call_dt"])
    per_step = run["stats"]["host_syncs"] / steps
    print(f"{mode}: {run['stats']['host_syncs']} host synchronisations in {steps} steps ({per_step:.3f} per step)")
    if mode == "run_ahead":
        assert per_step < 0.05
    else:
        assert per_step >= 1.0
    # the epsilon in force is the model's at the time of the last step taken, and so is the host's copy in the saved step
    t_last = float(run["sol"].dynamics.time[-1])
    # (the recorded times are sums of the 265 dt, the loop's own time another sum of them: 265 roundings of half an ulp of 8,
    # 2.4e-13, times the centre's speed 1.5)
    v = run["values"]
    assert max_abs(v, model.spot_values([FIXTURE_SPOT], t_last)) < 1e-12
    assert np.all(np.abs(run["eps"] - model.epsilon(_small().sites, 1.0, v)) <= model.value_bound(v))
    assert max_abs(run["sol"].tdgl_data.epsilon, run["eps"]) < 1e-12


def test_the_two_loops_are_bit_identical(direct_solve):
    runs = _fixture_runs()
    ra, cl = runs["run_ahead"], runs["classic"]
    assert np.array_equal(ra["sol"].dynamics.dt, cl["sol"].dynamics.dt)
    for key in ("psi", "mu", "supercurrent", "normal_current"):
        assert np.array_equal(ra["state"][key], cl["state"][key]), key
    assert np.array_equal(ra["eps"], cl["eps"]) and np.array_equal(ra["values"], cl["values"])
    assert ra["loop"] == cl["loop"]
    assert ra["stats"]["host_syncs"] < 0.05 * cl["stats"]["host_syncs"]
    assert ra["eps"].min() < 0.5  # the spot is in the film


def test_device_path_against_the_callable_path(direct_solve):
    """The same HotSpotEpsilon forced down the per-step callable path (one Python call and one upload per step): the
    project's 1e-8."""
    runs = _fixture_runs()
    a, b = runs["run_ahead"], runs["callable"]
    assert b["stats"]["host_syncs"] >= len(b["sol"].dynamics.dt) and len(b["values"]) == 0
    da, db = a["sol"].dynamics, b["sol"].dynamics
    assert len(da.dt) == len(db.dt)
    dev = dict(dt=max_abs(da.dt, db.dt) / db.dt.max(),
               psi2=max_abs(np.abs(a["state"]["psi"]) ** 2, np.abs(b["state"]["psi"]) ** 2),
               mu=max_abs(a["state"]["mu"] - a["state"]["mu"].mean(), b["state"]["mu"] - b["state"]["mu"].mean()),
               js=max_abs(a["state"]["supercurrent"], b["state"]["supercurrent"]),
               jn=max_abs(a["state"]["normal_current"], b["state"]["normal_current"]),
               eps=max_abs(a["eps"], b["eps"]))
    print("device path vs per-step callable:", {k: f"{v:.2e}" for k, v in dev.items()})
    for k, v in dev.items():
        assert v < 1e-8, (k, v)


def _raw_set_spots(ctx, sites, eps0, off, times, cx, cy, amp, sigma):
    from tdgl_amd._lib import f64, i32, p_f64, p_i32

    arrs = [f64(sites), f64(eps0), i32(off), f64(times), f64(cx), f64(cy), f64(amp), f64(sigma)]
    ctx._chk(ctx._lib.tdgl_set_epsilon_spots(ctx._ctx, p_f64(arrs[0]), p_f64(arrs[1]), len(off) - 1, p_i32(arrs[2]),
                                             *[p_f64(a) for a in arrs[3:]]))


def test_setters_and_getters(direct_solve):
    """Spots, then set_epsilon_table, then set_epsilon, each replacing the other; a refused set_epsilon_spots (one per rule)
    leaves epsilon and the run unchanged; n_spots = 0 switches the spots off and leaves epsilon as last written."""
    mesh = _small()
    sites, n = mesh.sites, len(mesh.sites)
    e_plain = 0.5 + 0.5 * np.sin(0.11 * np.arange(n)) ** 2
    spots = [dict(times=[0.0, 0.5, 2.0], centers=[[-3.0, 1.0], [0.0, 2.0], [4.0, -1.0]], amplitudes=[0.2, 0.7, 0.1], sigmas=[1.0, 2.0, 1.5]),
             dict(times=[0.1, 1.0], centers=[[5.0, -6.0], [5.0, 6.0]], amplitudes=0.4, sigmas=[0.5, 3.0])]
    eps0 = np.linspace(0.6, 1.0, n)

    def start(ctx, solver):
        ctx.set_state(solver.psi_init, solver.mu_init)
        ctx.set_controller_state(solver.options.dt_init)
        ctx.set_loop_state(0, 0.0, solver.options.dt_init)
        ctx.begin_stage()

    ref = _static_solver(mesh, e_plain)
    start(ref.ctx, ref)
    want = ref.ctx.run(12)["dt"], ref.ctx.get_state()["psi"]
    ref.ctx.close()

    solver = _static_solver(mesh, e_plain)
    ctx = solver.ctx
    assert np.array_equal(ctx.epsilon(), e_plain) and ctx.epsilon_spot_values().shape == (0, 4)
    # spots: epsilon = epsilon(r, 0), and the run moves it
    ctx.set_epsilon_spots(sites, eps0, spots)
    v0 = model.spot_values(spots, 0.0)
    assert np.array_equal(ctx.epsilon_spot_values(), v0)
    assert np.all(np.abs(ctx.epsilon() - model.epsilon(sites, eps0, v0)) <= model.value_bound(v0))
    start(ctx, solver)
    ctx.run(5, end_time=0.3)
    t_step = ctx.loop_state()["time"] - ctx.loop_state()["dt"]
    v = ctx.epsilon_spot_values()
    assert max_abs(v, model.spot_values(spots, t_step)) < 1e-12 and not np.array_equal(v, v0)
    assert np.all(np.abs(ctx.epsilon() - model.epsilon(sites, eps0, v)) <= model.value_bound(v))
    # ... the table replaces them ...
    static = np.linspace(1.0, 0.5, n)
    ctx.set_epsilon_table(static, [0.0, 10.0], [0.9, 0.9])
    assert ctx.epsilon_spot_values().shape == (0, 4)
    ctx.run(3)
    assert max_abs(ctx.epsilon(), 0.9 * static) == 0.0
    # ... spots replace the table ...
    ctx.set_epsilon_spots(sites, eps0, spots[:1])
    ctx.run(3)
    v = ctx.epsilon_spot_values()
    assert v.shape == (1, 4) and np.all(np.abs(ctx.epsilon() - model.epsilon(sites, eps0, v)) <= model.value_bound(v))
    # ... and plain values replace either: they stay through a run
    ctx.set_epsilon_table(static, [0.0, 10.0], [0.9, 0.9])
    ctx.set_epsilon(e_plain)
    ctx.run(3)
    assert np.array_equal(ctx.epsilon(), e_plain)
    ctx.set_epsilon_spots(sites, eps0, spots)
    ctx.set_epsilon(e_plain)
    assert ctx.epsilon_spot_values().shape == (0, 4)
    ctx.run(3)
    assert np.array_equal(ctx.epsilon(), e_plain)

    # one refusal per rule, on plain values and with spots in force: epsilon, the spots and the run stay as they were
    t, cx, cy, a, s = [0.0, 1.0], [0.0, 1.0], [0.5, 0.5], [0.1, 0.2], [1.0, 2.0]
    five = ([0, 1, 2, 3, 4, 5], [0.0] * 5, [0.0] * 5, [1.0] * 5, [0.1] * 5, [1.0] * 5)
    bad_sites = sites.copy()
    bad_sites[77, 1] = np.inf
    refusals = [
        ("n_spots", lambda: _raw_set_spots(ctx, sites, eps0, *five)),
        ("sites", lambda: _raw_set_spots(ctx, bad_sites, eps0, [0, 2], t, cx, cy, a, s)),
        ("eps0", lambda: _raw_set_spots(ctx, sites, np.where(np.arange(n) == 5, 1.0 + 1e-9, eps0), [0, 2], t, cx, cy, a, s)),
        ("eps0", lambda: _raw_set_spots(ctx, sites, np.where(np.arange(n) == 5, np.nan, eps0), [0, 2], t, cx, cy, a, s)),
        ("tab_times", lambda: _raw_set_spots(ctx, sites, eps0, [0, 2], [1.0, 1.0], cx, cy, a, s)),
        ("tab_times", lambda: _raw_set_spots(ctx, sites, eps0, [0, 2], [0.0, np.nan], cx, cy, a, s)),
        ("tab_cx", lambda: _raw_set_spots(ctx, sites, eps0, [0, 2], t, [0.0, np.inf], cy, a, s)),
        ("tab_cy", lambda: _raw_set_spots(ctx, sites, eps0, [0, 2], t, cx, [np.nan, 0.5], a, s)),
        ("tab_amp", lambda: _raw_set_spots(ctx, sites, eps0, [0, 2], t, cx, cy, [0.1, -1e-300], s)),
        ("tab_sigma", lambda: _raw_set_spots(ctx, sites, eps0, [0, 2], t, cx, cy, a, [1.0, 0.0])),
        ("tab_sigma", lambda: _raw_set_spots(ctx, sites, eps0, [0, 2], t, cx, cy, a, [1.0, 1e-170])),  # sigma^2 underflows
        ("tab_off", lambda: _raw_set_spots(ctx, sites, eps0, [0, 0], t, cx, cy, a, s)),
    ]
    for in_force in (False, True):
        if in_force:
            ctx.set_epsilon_spots(sites, eps0, spots)
        before, values = ctx.epsilon(), ctx.epsilon_spot_values()
        for name, call in refusals:
            with pytest.raises(ValueError, match=name):
                call()
            assert np.array_equal(ctx.epsilon(), before) and np.array_equal(ctx.epsilon_spot_values(), values), name
        for name, bad in (("centre", [np.nan, 0.0, 0.1, 1.0]), ("amplitude", [0.0, 1.0, -0.1, 1.0]), ("sigma", [0.0, 1.0, 0.1, 0.0]),
                          ("sigma", [0.0, 1.0, 0.1, 1e-170])):
            from tdgl_amd._lib import f64, p_f64

            with pytest.raises(ValueError if in_force else RuntimeError, match=name if in_force else "call tdgl_set_epsilon_spots first"):
                ctx._chk(ctx._lib.tdgl_update_epsilon_spots(ctx._ctx, p_f64(f64([bad, bad]))))
            assert np.array_equal(ctx.epsilon(), before) and np.array_equal(ctx.epsilon_spot_values(), values), name
        if not in_force:  # the run on plain values is the run of a context that never heard of spots
            start(ctx, solver)
            assert np.array_equal(ctx.run(12)["dt"], want[0]) and np.array_equal(ctx.get_state()["psi"], want[1])

    # n_spots = 0: off, epsilon as last written -- also through further steps
    start(ctx, solver)
    ctx.run(4)
    last = ctx.epsilon()
    assert not np.array_equal(last, before)
    ctx.set_epsilon_spots(None, None, None)
    assert ctx.epsilon_spot_values().shape == (0, 4) and np.array_equal(ctx.epsilon(), last)
    ctx.run(4)
    assert np.array_equal(ctx.epsilon(), last)
    ctx.close()


def test_mixed_ensemble(direct_solve):
    """R = 5 replicas: static epsilon, a table, one spot, four spots and a spot with a = 0 throughout.  The ensemble is bit
    for bit five ensembles of one; the spot replicas agree with TDGLSolver runs of the same spots within the tolerances of
    test_separable_epsilon_per_replica (1e-8 on dt / dt_max and on |psi|^2); the a = 0 replica is the static one to the
    last bit."""
    from tdgl_amd import SolverOptions, TDGLSolver
    from tdgl_amd.ensemble import solve_ensemble_dimensionless

    mesh = _small()
    n = len(mesh.sites)
    e_static = np.where(np.abs(mesh.sites[:, 0]) < 2.0, 1.0, 0.4)
    one_spot = [dict(times=[0.0, 0.3, 1.5], centers=[[-4.0, 1.0], [-2.0, 1.5], [3.0, -2.0]], amplitudes=[0.0, 0.6, 0.2], sigmas=[0.8, 1.5, 3.0])]
    four = one_spot + [dict(times=[0.0, 1.5], centers=[[6.0, 6.0], [-6.0, 5.0]], amplitudes=0.3, sigmas=1.0),
                       dict(times=[0.5], centers=[[0.0, -7.0]], amplitudes=0.25, sigmas=2.0),
                       dict(times=[0.2, 0.4, 0.6, 1.0], centers=[[7.0, -7.0]] * 4, amplitudes=[0.0, 0.5, 0.5, 0.0], sigmas=[0.5, 0.5, 1.0, 1.0])]
    zero = [dict(times=[0.0, 1.0], centers=[[-3.0, 0.5], [3.0, 0.7]], amplitudes=0.0, sigmas=[1.0, 2.0])]
    eps = [e_static, e_static, 1.0, 1.0, e_static]
    tables = [None, (e_static, [0.0, 0.7, 1.5], [1.0, 0.4, 0.9]), None, None, None]
    spots = [None, None, (e_static, one_spot), (1.0, four), (e_static, zero)]
    opts = SolverOptions(solve_time=1.5, dt_init=1e-3, save_every=50, pcg_rtol=1e-11)
    A = uniform_field_A(mesh, 0.3)

    def ensemble(idx):
        return solve_ensemble_dimensionless(mesh, opts, A, [eps[i] for i in idx], U_DEFAULT, GAMMA_DEFAULT,
                                            epsilon_table=[tables[i] for i in idx], epsilon_spots=[spots[i] for i in idx])

    sols = ensemble(range(5))
    assert [s.dynamic_epsilon for s in sols] == [False, True, True, True, True]
    for r in range(5):
        (alone,) = ensemble([r])
        assert np.array_equal(sols[r].dynamics.dt, alone.dynamics.dt), r
        for x, y in zip(sols[r].saved_steps, alone.saved_steps):
            assert x.step == y.step and x.time == y.time
        a, b = sols[r].tdgl_data, alone.tdgl_data
        for key in ("psi", "mu", "supercurrent", "normal_current", "epsilon"):
            assert np.array_equal(getattr(a, key), getattr(b, key)), (r, key)
    # a = 0 throughout: the static replica, to the last bit
    assert np.array_equal(sols[4].dynamics.dt, sols[0].dynamics.dt)
    for key in ("psi", "mu", "supercurrent", "normal_current"):
        assert np.array_equal(getattr(sols[4].tdgl_data, key), getattr(sols[0].tdgl_data, key)), key
    assert np.array_equal(sols[4].tdgl_data.epsilon, e_static)
    # the spots did act
    assert max_abs(np.abs(sols[2].tdgl_data.psi) ** 2, np.abs(sols[0].tdgl_data.psi) ** 2) > 1e-3
    for r in (2, 3):
        e0, sp = spots[r]
        one = TDGLSolver.from_dimensionless(mesh, opts, A, 1.0, U_DEFAULT, GAMMA_DEFAULT, epsilon_spots=(e0, sp))
        b = one.solve()
        one.ctx.close()
        a = sols[r]
        assert len(a.dynamics.dt) == len(b.dynamics.dt)
        dev = (max_abs(a.dynamics.dt, b.dynamics.dt) / b.dynamics.dt.max(), max_abs(np.abs(a.tdgl_data.psi) ** 2, np.abs(b.tdgl_data.psi) ** 2))
        print(f"hot spots, replica {r}: dt {dev[0]:.2e}, |psi|^2 {dev[1]:.2e}")
        assert dev[0] <= 1e-8
        assert dev[1] < 1e-8
        assert [s.step for s in a.saved_steps] == [s.step for s in b.saved_steps]
        last = a.saved_steps[-1]
        assert max_abs(last.epsilon, model.epsilon(mesh.sites, e0, model.spot_values(sp, last.time))) < 1e-12
        for x, y in zip(a.saved_steps, b.saved_steps):
            assert max_abs(x.epsilon, y.epsilon) < 1e-8


def test_ensemble_setter_refuses_like_the_contexts(direct_solve):
    """tdgl_ensemble_set_epsilon_spots: the context's rules under its own name; a refused call leaves the replica's epsilon;
    spots, a table and plain values replace each other; tdgl_ensemble_get_epsilon reads what is in force."""
    from tdgl_amd.ensemble import EnsembleContext

    mesh = _small()
    sites, n = mesh.sites, len(mesh.sites)
    solver = _static_solver(mesh, 1.0)
    ens = EnsembleContext(solver.ctx, 2)
    e_plain = np.linspace(0.2, 0.9, n)
    for r in range(2):
        ens.set_epsilon(r, e_plain)
    spot = dict(times=[0.0, 1.0], centers=[[-3.0, 1.0], [2.0, 1.5]], amplitudes=[0.4, 0.6], sigmas=1.3)
    eps0 = np.linspace(1.0, 0.7, n)
    ens.set_epsilon_spots(1, sites, eps0, [spot])
    v0 = model.spot_values([spot], 0.0)
    assert np.array_equal(ens.epsilon(0), e_plain)
    assert np.all(np.abs(ens.epsilon(1) - model.epsilon(sites, eps0, v0)) <= model.value_bound(v0))
    before = ens.epsilon(1)
    with pytest.raises(ValueError, match="tdgl_ensemble_set_epsilon_spots: spot 0: tab_sigma"):
        ens.set_epsilon_spots(1, sites, eps0, [_bare(spot, sigmas=[1.0, -1.0])])
    with pytest.raises(ValueError, match="tdgl_ensemble_set_epsilon_spots: spot 1: tab_times"):
        ens.set_epsilon_spots(1, sites, eps0, [spot, _bare(spot, times=[1.0, 1.0])])
    with pytest.raises(ValueError, match="tdgl_ensemble_set_epsilon_spots: spot 0: tab_amp"):
        ens.set_epsilon_spots(1, sites, eps0, [_bare(spot, amplitudes=[0.4, -0.1])])
    assert np.array_equal(ens.epsilon(1), before)
    ens.set_epsilon(1, e_plain)
    assert np.array_equal(ens.epsilon(1), e_plain)
    ens.close()
    solver.ctx.close()


def _bare(spot, **override):
    """A HotSpot that skipped its own checks, so that the library's are reached."""
    from tdgl_amd import HotSpot

    d = dict(spot, **override)
    n = len(d["times"])
    s = object.__new__(HotSpot)
    s.times = np.asarray(d["times"], dtype=float)
    s.centers = np.asarray(d["centers"], dtype=float)
    s.amplitudes = np.asarray(d["amplitudes"], dtype=float) * np.ones(n)
    s.sigmas = np.asarray(d["sigmas"], dtype=float) * np.ones(n)
    return s


def test_example_runs_at_a_reduced_size():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "hot_spot.py"), "--small"], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("bias ")]
    assert len(lines) >= 3 and all(("pulse" in ln) or ("no pulse" in ln) for ln in lines)
    assert "host synchronisations" in out.stdout
