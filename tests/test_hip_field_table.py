"""The tabulated field waveform A(t) = TabulatedRamp(times, values)(t) * A_base on the GPU (tdgl_set_link_table,
tdgl_ensemble_set_link_table): against a reference fixture, against the same waveform evaluated in Python once per step,
the run-ahead loop against the loop with one synchronisation per step, and as replicas of an ensemble.

Everything runs on fixture mesh_small (516 sites) with the direct mu solve.  The runs several tests look at are made once
(`_run`) and only read afterwards."""

import numpy as np
import pytest

from conftest import load_golden
from helpers import (
    GAMMA_DEFAULT,
    U_DEFAULT,
    align_phase,
    max_abs,
    options_from_golden,
    reference_mesh,
    remove_mean,
    uniform_field_A,
)

pytestmark = pytest.mark.gpu

# first node after t = 0 (the hold rule in front), up, a hold of 0.77 (dt <= 0.1: more than three steps), down through zero
# to a negative value, last node well before the end of the run; no node but a step's luck would land on these times
TIMES = [0.37, 1.13, 1.9, 3.05]
VALUES = [0.0, 1.0, 1.0, -0.6]
SOLVE_TIME = 4.0
B_PEAK = 0.2
TOL = 1e-8  # the native-ramp-against-callable comparisons of tests/test_hip_parity.py

_cache = {}


def _mesh():
    if "mesh" not in _cache:
        _cache["mesh"] = reference_mesh(load_golden("mesh_small"))
    return _cache["mesh"]


def _A_base():
    return uniform_field_A(_mesh(), B_PEAK)


def _options():
    from tdgl_amd import SolverOptions

    return SolverOptions(solve_time=SOLVE_TIME, dt_init=1e-3, dt_max=0.1, save_every=50, pcg_rtol=1e-12)


def _factor(times=TIMES, values=VALUES):
    from tdgl_amd.parameter import PiecewiseLinear

    return PiecewiseLinear(times, values)


def _solve(monkeypatch, run_ahead=True, **kw):
    """One `TDGLSolver.from_dimensionless(...).solve()` on mesh_small; returns what the tests read."""
    from tdgl_amd import TDGLSolver

    if run_ahead:
        monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    else:
        monkeypatch.setenv("TDGL_NO_RUN_AHEAD", "1")  # (read when the context is created)
    A0 = kw.pop("A0")
    solver = TDGLSolver.from_dimensionless(_mesh(), kw.pop("options", None) or _options(), A0, 1.0, U_DEFAULT, GAMMA_DEFAULT,
                                           probe_points=[263, 273], **kw)
    assert solver.ctx.dense_direct
    solver.ctx.step_stats(reset=True)
    sol = solver.solve()
    out = dict(sol=sol, stats=solver.ctx.step_stats(), link_scale=solver.ctx.link_scale())
    solver.ctx.close()
    return out


def _run(name, monkeypatch):
    """The shared runs, each made once: the waveform as a table in the run-ahead loop ("table") and in the loop with one
    synchronisation per step ("table_classic"), and as a Python callable evaluated before every step ("callable")."""
    if name not in _cache:
        A_base, f = _A_base(), _factor()
        if name == "callable":
            kw = dict(vector_potential_func=lambda t: f(t) * A_base)
        else:
            kw = dict(vector_potential_table=(A_base, TIMES, VALUES))
        _cache[name] = _solve(monkeypatch, run_ahead=name != "table_classic", A0=f(0.0) * A_base, **kw)
    return _cache[name]


def _assert_fields_agree(a, b, tol):
    """dt, |psi|^2, mu - <mu>, J_s and J_n of two solutions."""
    assert len(a.dynamics.dt) == len(b.dynamics.dt)
    dev = dict(
        dt=max_abs(a.dynamics.dt, b.dynamics.dt) / b.dynamics.dt.max(),
        psi2=max_abs(np.abs(a.tdgl_data.psi) ** 2, np.abs(b.tdgl_data.psi) ** 2),
        mu=max_abs(remove_mean(a.tdgl_data.mu), remove_mean(b.tdgl_data.mu)) / max(1.0, np.abs(remove_mean(b.tdgl_data.mu)).max()),
        js=max_abs(a.tdgl_data.supercurrent, b.tdgl_data.supercurrent),
        jn=max_abs(a.tdgl_data.normal_current, b.tdgl_data.normal_current),
    )
    print("deviations:", {k: float(v) for k, v in dev.items()})
    assert dev["dt"] <= tol
    for k in ("psi2", "mu", "js", "jn"):
        assert dev[k] < tol, (k, dev)


def test_two_node_table_reproduces_the_reference_ramp(direct_solve, monkeypatch):
    """traj_dynamic_lag (the reference's LinearRamp moving A by less than np.allclose's tolerance per step: dA/dt follows,
    the links lag) with the ramp given as the table [(tmin, initial), (tmax, final)]: the checks of
    tests/test_hip_parity.py::_assert_hip_trajectory at the fixture's own tolerance, 1e-8."""
    from tdgl_amd import SolverOptions

    g = load_golden("traj_dynamic_lag")
    o = options_from_golden(g)
    opts = SolverOptions(solve_time=o.solve_time, dt_init=o.dt_init, dt_max=o.dt_max, adaptive=False, save_every=o.save_every,
                         pcg_rtol=1e-12)
    A_base = g["A_base"]
    tmin, tmax, initial, final = (float(g["ramp_" + k]) for k in ("tmin", "tmax", "initial", "final"))
    f = _factor([tmin, tmax], [initial, final])
    run = _solve(monkeypatch, A0=f(0.0) * A_base, options=opts, vector_potential_table=(A_base, [tmin, tmax], [initial, final]))
    sol, tol = run["sol"], 1e-8
    dyn, last = sol.dynamics, sol.tdgl_data
    want_dt = g["call_dt"]
    assert len(dyn.dt) == len(want_dt)
    assert max_abs(dyn.dt, want_dt) <= tol * want_dt.max()
    assert max_abs(np.abs(last.psi) ** 2, np.abs(g["final_psi"]) ** 2) < tol
    assert max_abs(last.supercurrent, g["final_supercurrent"]) < tol
    assert max_abs(last.normal_current, g["final_normal_current"]) < tol
    scale = max(1.0, np.abs(remove_mean(g["final_mu"])).max())
    assert max_abs(remove_mean(last.mu), remove_mean(g["final_mu"])) < tol * scale
    assert max_abs(align_phase(last.psi, g["final_psi"]), g["final_psi"]) < tol
    assert max_abs(dyn.mu[0] - dyn.mu[1], g["call_mu_probe"][:, 0] - g["call_mu_probe"][:, 1]) < tol * scale
    d1 = np.exp(1j * (dyn.theta[0] - dyn.theta[1]))
    d2 = np.exp(1j * (g["call_theta_probe"][:, 0] - g["call_theta_probe"][:, 1]))
    assert max_abs(d1, d2) < tol
    assert [s.step for s in sol.saved_steps] == list(g["save_step"])
    assert max_abs([s.time for s in sol.saved_steps], g["save_time"]) <= tol * max(1.0, g["save_time"].max())
    assert sol.stats["steps_simulating"] == len(g["call_dt"])
    # the saved A_applied follows the table (its value at the last step taken) although the links lag
    assert max_abs(last.applied_vector_potential, f(float(g["call_time"][-1])) * A_base) < 1e-12
    # the device evaluated it: far fewer synchronisations than steps
    assert run["stats"]["host_syncs"] < 0.2 * run["stats"]["steps"]


def test_waveform_matches_the_callable_evaluated_on_the_host(direct_solve, monkeypatch):
    """Up, hold, down through zero, hold: the table the device evaluates against the same waveform as a Python callable,
    evaluated and uploaded before every step."""
    tab, ref = _run("table", monkeypatch), _run("callable", monkeypatch)
    a, b = tab["sol"], ref["sol"]
    assert a.dynamic_vector_potential and b.dynamic_vector_potential
    assert a.stats["steps_simulating"] == b.stats["steps_simulating"]
    _assert_fields_agree(a, b, TOL)
    # the waveform did act, and the run went through every piece of it
    t = a.dynamics.time
    assert t[-1] > TIMES[-1] and np.abs(a.tdgl_data.supercurrent).max() > 1e-3
    assert not np.any(np.isin(TIMES, t))  # (no step landed on a node)
    assert np.sum((t > TIMES[1]) & (t < TIMES[2])) > 3  # (the hold)
    # the saved A_applied is the last node's from there on, exactly
    A_end = VALUES[-1] * _A_base()
    assert np.array_equal(a.tdgl_data.applied_vector_potential, A_end)
    assert max_abs(b.tdgl_data.applied_vector_potential, A_end) < 1e-12
    assert tab["link_scale"] == VALUES[-1]


def test_run_ahead_loop_and_classic_loop_agree_to_the_last_bit(direct_solve, monkeypatch):
    """table_value on the device against table_value on the host (TDGL_NO_RUN_AHEAD=1), operation for operation."""
    ra, cl = _run("table", monkeypatch), _run("table_classic", monkeypatch)
    a, b = ra["sol"], cl["sol"]
    assert np.array_equal(a.dynamics.dt, b.dynamics.dt)
    assert np.array_equal(a.tdgl_data.psi, b.tdgl_data.psi)
    assert np.array_equal(a.tdgl_data.mu, b.tdgl_data.mu)
    assert np.array_equal(a.tdgl_data.supercurrent, b.tdgl_data.supercurrent)
    assert np.array_equal(a.tdgl_data.normal_current, b.tdgl_data.normal_current)
    assert ra["link_scale"] == cl["link_scale"]
    assert ra["stats"]["host_syncs"] < cl["stats"]["host_syncs"]


def test_the_table_runs_in_the_run_ahead_loop(direct_solve, monkeypatch):
    """Host synchronisations per accepted step: below one for the table, at least one for the callable."""
    tab, ref = _run("table", monkeypatch)["stats"], _run("callable", monkeypatch)["stats"]
    assert tab["steps"] == ref["steps"] > 0
    print("host syncs per step: table", tab["host_syncs"] / tab["steps"], "callable", ref["host_syncs"] / ref["steps"])
    assert tab["host_syncs"] / tab["steps"] < 1.0
    assert ref["host_syncs"] / ref["steps"] >= 1.0


def test_one_node_table_is_the_static_field(direct_solve, monkeypatch):
    from tdgl_amd import SolverOptions

    A_base = _A_base()
    opts = SolverOptions(solve_time=1.0, dt_init=1e-3, dt_max=0.1, save_every=50, pcg_rtol=1e-12)
    one = _solve(monkeypatch, A0=0.7 * A_base, options=opts, vector_potential_table=(A_base, [0.4], [0.7]))
    static = _solve(monkeypatch, A0=0.7 * A_base, options=opts)
    a, b = one["sol"], static["sol"]
    assert len(a.dynamics.dt) > 10 and np.array_equal(a.dynamics.dt, b.dynamics.dt)
    assert max_abs(np.abs(a.tdgl_data.psi) ** 2, np.abs(b.tdgl_data.psi) ** 2) < 1e-12
    assert one["link_scale"] == 0.7
    assert np.array_equal(a.tdgl_data.applied_vector_potential, 0.7 * A_base)


def test_table_that_ends_before_the_run_holds_its_last_value(direct_solve, monkeypatch):
    from tdgl_amd import TDGLSolver

    monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    A_base = _A_base()
    times, values = [0.0, 0.05], [0.2, 0.45]
    solver = TDGLSolver.from_dimensionless(_mesh(), _options(), 0.2 * A_base, 1.0, U_DEFAULT, GAMMA_DEFAULT,
                                           vector_potential_table=(A_base, times, values))
    ctx = solver.ctx
    ctx.set_state(solver.psi_init, solver.mu_init)
    ctx.begin_stage()
    inside = ctx.run(10)  # dt_init = 1e-3: still on the slope
    t_in = ctx.loop_state()["time"]
    assert len(inside["dt"]) == 10 and t_in < times[-1]
    assert values[0] < ctx.link_scale() < values[-1]
    assert abs(ctx.link_scale() - _factor(times, values)(t_in - inside["dt"][-1])) < 1e-12
    res = ctx.run(10**4, end_time=0.3)
    assert res["reached_end"] and ctx.loop_state()["time"] >= 0.3
    assert ctx.link_scale() == values[-1]
    # settled: the field is static from here on and the run goes on in batches
    ctx.step_stats(reset=True)
    more = ctx.run(64)
    st = ctx.step_stats()
    assert len(more["dt"]) == 64 and st["host_syncs"] < 0.2 * st["steps"] and ctx.link_scale() == values[-1]
    ctx.close()


def _assert_like_single(ens, one, tol):
    """A replica of an ensemble against tdgl.solve of that replica alone
    (tests/test_hip_ensemble_dynamic.py::_assert_like_single)."""
    assert ens.stats["mu_solver"] == "dense_ensemble"
    assert ens.stats["steps_thermalizing"] == one.stats["steps_thermalizing"]
    assert ens.stats["steps_simulating"] == one.stats["steps_simulating"]
    assert ens.dynamic_vector_potential == one.dynamic_vector_potential
    assert ens.dynamic_epsilon == one.dynamic_epsilon
    a, b = ens.dynamics, one.dynamics
    assert len(a.dt) == len(b.dt)
    assert max_abs(a.dt, b.dt) <= tol * b.dt.max()
    assert max_abs(a.time, b.time) <= tol * max(1.0, b.time.max())
    assert [s.step for s in ens.saved_steps] == [s.step for s in one.saved_steps]
    assert max_abs([s.time for s in ens.saved_steps], [s.time for s in one.saved_steps]) <= tol * max(1.0, one.saved_steps[-1].time)
    x, y = ens.tdgl_data, one.tdgl_data
    scale = max(1.0, np.abs(remove_mean(y.mu)).max())
    print("ensemble against single: dt", float(max_abs(a.dt, b.dt) / b.dt.max()), "|psi|^2", float(max_abs(np.abs(x.psi) ** 2, np.abs(y.psi) ** 2)),
          "mu", float(max_abs(remove_mean(x.mu), remove_mean(y.mu)) / scale), "J_s", float(max_abs(x.supercurrent, y.supercurrent)),
          "J_n", float(max_abs(x.normal_current, y.normal_current)))
    assert max_abs(np.abs(x.psi) ** 2, np.abs(y.psi) ** 2) < tol
    assert max_abs(remove_mean(x.mu), remove_mean(y.mu)) < tol * scale
    assert max_abs(x.supercurrent, y.supercurrent) < tol * max(1.0, np.abs(y.supercurrent).max())
    assert max_abs(x.normal_current, y.normal_current) < tol * max(1.0, np.abs(y.normal_current).max())
    if b.mu is not None and b.mu.shape[0] > 1:
        assert max_abs(a.mu[0] - a.mu[1], b.mu[0] - b.mu[1]) < tol * max(scale, np.abs(b.mu[0] - b.mu[1]).max())
        assert max_abs(np.exp(1j * (a.theta[0] - a.theta[1])), np.exp(1j * (b.theta[0] - b.theta[1]))) < tol
    for s, t in zip(ens.saved_steps, one.saved_steps):
        assert max_abs(s.applied_vector_potential, t.applied_vector_potential) < tol * max(1.0, np.abs(t.applied_vector_potential).max())
        assert max_abs(s.epsilon, t.epsilon) < tol


def test_ensemble_of_tables_a_ramp_and_a_static_field(direct_solve, monkeypatch):
    """The waveform, a second table of another length that is still on a slope when the run ends, a LinearRamp and a static
    field in one ensemble: each replica against the single run of the same input, with the checks, the tolerance (1e-8) and
    the options of tests/test_hip_ensemble_dynamic.py::test_field_ramps_with_lagging_links: fixed dt = 1e-3, pcg_rtol 1e-12.
    The tolerance belongs to those options.  The CPU oracle run twice on these inputs, psi_0 perturbed by 1e-14, moves by
    1.5e-10 in |psi|^2 over the 4,002 fixed steps -- and by 7.5e-8 with adaptive dt up to 0.1 (68 steps, the static replica
    as much as the tabulated ones), where no two orders of summation can be held to 1e-8."""
    from tdgl_amd import SolverOptions
    from tdgl_amd.ensemble import EnsembleContext, ensemble_dimensionless

    opts = SolverOptions(solve_time=SOLVE_TIME, dt_init=1e-3, dt_max=1e-3, adaptive=False, save_every=1000, pcg_rtol=1e-12)

    monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    A_base = _A_base()
    second = ([0.5, 2.0, 9.0], [0.2, 0.8, 0.0])
    ramp = dict(tmin=0.0, tmax=1.5, initial=0.0, final=0.7)
    tables = [(A_base, TIMES, VALUES), (A_base, *second), None, None]
    ramps = [None, None, (A_base, ramp), None]
    A0 = [None, None, None, 0.4 * A_base]
    scales = {}
    close = EnsembleContext.close

    def close_after_reading_the_link_scales(self):
        if self._ens:
            scales.update({r: self.link_scale(r) for r in range(self.R)})
        close(self)

    monkeypatch.setattr(EnsembleContext, "close", close_after_reading_the_link_scales)
    sols = ensemble_dimensionless(_mesh(), opts, A0, 1.0, U_DEFAULT, GAMMA_DEFAULT, probe_points=[263, 273],
                                  vector_potential_ramp=ramps, vector_potential_table=tables).solve()
    assert len(sols) == 4 and sorted(scales) == [0, 1, 2, 3]
    singles = [
        _solve(monkeypatch, A0=VALUES[0] * A_base, options=opts, vector_potential_table=tables[0])["sol"],
        _solve(monkeypatch, A0=second[1][0] * A_base, options=opts, vector_potential_table=tables[1])["sol"],
        _solve(monkeypatch, A0=0.0 * A_base, options=opts, vector_potential_ramp=ramps[2])["sol"],
        _solve(monkeypatch, A0=A0[3], options=opts)["sol"],
    ]
    for r in range(4):
        _assert_like_single(sols[r], singles[r], 1e-8)
    # the factor of the last step taken is the table's value at that step's time
    assert scales[0] == VALUES[-1]
    t_last = float(sols[1].dynamics.time[-1])
    assert second[0][1] < t_last < second[0][2]
    assert abs(scales[1] - _factor(*second)(t_last)) < 1e-12
    assert max_abs(sols[1].tdgl_data.applied_vector_potential, _factor(*second)(t_last) * A_base) < 1e-12
    assert scales[2] == ramp["final"]
