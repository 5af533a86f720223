"""Sums of a static and time-scaled field terms A(t) = A_0 + f_1(t) A_1 + ... + f_K(t) A_K on the GPU (tdgl_set_link_terms,
tdgl_update_link_terms, tdgl_ensemble_set_link_terms): against the reference fixture traj_field_terms_small, the run-ahead
loop against the loop with one synchronisation per step, against the same field evaluated in Python once per step, the
lag rule of traj_dynamic_lag with its ramp split into a sum, the step rule's skipped edge passes, edge cases, replicas of
an ensemble and the entry points' refusals.

Everything runs on fixture mesh_small (516 sites) with the direct mu solve and pcg_rtol = 1e-12.  The runs several tests
look at are made once (`_run`) and only read afterwards."""

import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from field_terms_model import StepRule, factor_value, fixture_terms, flux_spot_A, terms_sum
from helpers import GAMMA_DEFAULT, U_DEFAULT, align_phase, max_abs, options_from_golden, reference_mesh, remove_mean, uniform_field_A

pytestmark = pytest.mark.gpu

TOL = 1e-8  # the fixture tolerance of the time-dependent fields (traj_dynamic_lag in tests/test_hip_field_table.py)
PROBES = [263, 273]

_cache = {}


def _mesh():
    if "mesh" not in _cache:
        _cache["mesh"] = reference_mesh(load_golden("mesh_small"))
    return _cache["mesh"]


def _golden():
    if "g" not in _cache:
        _cache["g"] = load_golden("traj_field_terms_small")
    return _cache["g"]


def _options(g=None, **kw):
    from tdgl_amd import SolverOptions

    if g is None:
        base = dict(solve_time=1.0, dt_init=1e-3, dt_max=0.05, save_every=50)  # (dt_max: see the fixture's generator)
    else:
        o = options_from_golden(g)
        base = dict(solve_time=o.solve_time, dt_init=o.dt_init, dt_max=o.dt_max, adaptive=o.adaptive, save_every=o.save_every)
    base.update(kw)
    return SolverOptions(pcg_rtol=1e-12, **base)


def _solve(monkeypatch, options, run_ahead=True, A=None, probe_points=PROBES, **kw):
    """One `TDGLSolver.from_dimensionless(...).solve()` on mesh_small; returns what the tests read."""
    from tdgl_amd import TDGLSolver

    if run_ahead:
        monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    else:
        monkeypatch.setenv("TDGL_NO_RUN_AHEAD", "1")  # (read when the context is created)
    terms = kw.get("vector_potential_terms")
    if A is None:
        A0, products = terms
        A = terms_sum(A0, [b for b, _ in products], [factor_value(s, 0.0) for _, s in products])
    solver = TDGLSolver.from_dimensionless(_mesh(), options, A, 1.0, U_DEFAULT, GAMMA_DEFAULT, probe_points=probe_points, **kw)
    assert solver.ctx.dense_direct
    solver.ctx.step_stats(reset=True)
    sol = solver.solve()
    out = dict(sol=sol, stats=solver.ctx.step_stats(), scales=solver.ctx.link_term_scales(), moves=solver.ctx.link_term_moves(),
               link_scale=solver.ctx.link_scale(), device_evaluates=solver.device_evaluates_field())
    solver.ctx.close()
    return out


def _run(name, monkeypatch):
    """The shared runs of the fixture's field, each made once: as terms in the run-ahead loop ("terms") and in the loop with
    one synchronisation per step ("terms_classic"), and as a Python callable evaluated before every step ("callable")."""
    if name not in _cache:
        g = _golden()
        A0, products = fixture_terms(g)
        bases, specs = [b for b, _ in products], [s for _, s in products]
        if name == "callable":
            kw = dict(vector_potential_func=lambda t: terms_sum(A0, bases, [factor_value(s, t) for s in specs]),
                      A=terms_sum(A0, bases, [factor_value(s, 0.0) for s in specs]))
        else:
            kw = dict(vector_potential_terms=(A0, products))
        _cache[name] = _solve(monkeypatch, _options(g), run_ahead=name != "terms_classic", **kw)
    return _cache[name]


def _assert_like_fixture(g, sol, tol):
    """tests/test_hip_parity.py::_assert_hip_trajectory."""
    dyn, last = sol.dynamics, sol.tdgl_data
    want_dt = g["call_dt"]
    assert len(dyn.dt) == len(want_dt)
    scale = max(1.0, np.abs(remove_mean(g["final_mu"])).max())
    print("against the fixture: dt", float(max_abs(dyn.dt, want_dt) / want_dt.max()),
          "|psi|^2", float(max_abs(np.abs(last.psi) ** 2, np.abs(g["final_psi"]) ** 2)),
          "J_s", float(max_abs(last.supercurrent, g["final_supercurrent"])), "J_n", float(max_abs(last.normal_current, g["final_normal_current"])),
          "mu", float(max_abs(remove_mean(last.mu), remove_mean(g["final_mu"])) / scale))
    assert max_abs(dyn.dt, want_dt) <= tol * want_dt.max()
    assert max_abs(np.abs(last.psi) ** 2, np.abs(g["final_psi"]) ** 2) < tol
    assert max_abs(last.supercurrent, g["final_supercurrent"]) < tol
    assert max_abs(last.normal_current, g["final_normal_current"]) < tol
    assert max_abs(remove_mean(last.mu), remove_mean(g["final_mu"])) < tol * scale
    assert max_abs(align_phase(last.psi, g["final_psi"]), g["final_psi"]) < tol
    assert max_abs(dyn.mu[0] - dyn.mu[1], g["call_mu_probe"][:, 0] - g["call_mu_probe"][:, 1]) < tol * scale
    d1 = np.exp(1j * (dyn.theta[0] - dyn.theta[1]))
    d2 = np.exp(1j * (g["call_theta_probe"][:, 0] - g["call_theta_probe"][:, 1]))
    assert max_abs(d1, d2) < tol
    assert [s.step for s in sol.saved_steps] == list(g["save_step"])
    assert max_abs([s.time for s in sol.saved_steps], g["save_time"]) <= tol * max(1.0, g["save_time"].max())
    assert sol.stats["steps_simulating"] == len(g["call_dt"])


@pytest.mark.parametrize("name", ["terms", "terms_classic"])
def test_fixture_through_vector_potential_terms(direct_solve, monkeypatch, name):
    """traj_field_terms_small (a uniform bias, a ramped uniform field, a flux spot driven up, held and down through zero)
    in the run-ahead loop and in the loop with one synchronisation per step."""
    g = _golden()
    assert list(g["probe_points"]) == PROBES
    run = _run(name, monkeypatch)
    assert run["device_evaluates"]
    _assert_like_fixture(g, run["sol"], TOL)


def test_run_ahead_loop_and_classic_loop_agree_to_the_last_bit(direct_solve, monkeypatch):
    """One links kernel and one step rule behind both loops, the factors from linear_ramp_value and table_value on
    the host and on the device: nothing may differ."""
    ra, cl = _run("terms", monkeypatch), _run("terms_classic", monkeypatch)
    a, b = ra["sol"], cl["sol"]
    assert np.array_equal(a.dynamics.dt, b.dynamics.dt)
    assert np.array_equal(a.tdgl_data.psi, b.tdgl_data.psi)
    assert np.array_equal(a.tdgl_data.mu, b.tdgl_data.mu)
    assert np.array_equal(a.tdgl_data.supercurrent, b.tdgl_data.supercurrent)
    assert np.array_equal(a.tdgl_data.normal_current, b.tdgl_data.normal_current)
    assert np.array_equal(ra["scales"], cl["scales"]) and ra["moves"] == cl["moves"]
    for s, t in zip(a.saved_steps, b.saved_steps):
        assert np.array_equal(s.applied_vector_potential, t.applied_vector_potential)


def test_terms_match_the_callable_evaluated_on_the_host(direct_solve, monkeypatch):
    """The same field as a Python callable, evaluated and uploaded before every step; the saved A_applied of the terms is
    the NumPy expression ((A_0 + s_1 A_1) + s_2 A_2) with the factors of the last step taken, bit for bit."""
    g = _golden()
    tm, ref = _run("terms", monkeypatch), _run("callable", monkeypatch)
    a, b = tm["sol"], ref["sol"]
    assert a.dynamic_vector_potential and b.dynamic_vector_potential
    assert len(a.dynamics.dt) == len(b.dynamics.dt)
    assert max_abs(a.dynamics.dt, b.dynamics.dt) <= TOL * b.dynamics.dt.max()
    x, y = a.tdgl_data, b.tdgl_data
    assert max_abs(np.abs(x.psi) ** 2, np.abs(y.psi) ** 2) < TOL
    assert max_abs(remove_mean(x.mu), remove_mean(y.mu)) < TOL * max(1.0, np.abs(remove_mean(y.mu)).max())
    assert max_abs(x.supercurrent, y.supercurrent) < TOL
    assert max_abs(x.normal_current, y.normal_current) < TOL
    A0, products = fixture_terms(g)
    bases, specs = [p[0] for p in products], [p[1] for p in products]
    saved = a.saved_steps
    assert len(saved) >= 3
    t_begin = np.concatenate([[0.0], a.dynamics.time[:-1]])
    for k, s in enumerate(saved):
        # (the factors of the last step taken, evaluated at the time that step began)
        t_eval = 0.0 if s.step == 0 else float(t_begin[min(s.step, len(t_begin)) - 1])
        want = terms_sum(A0, bases, [factor_value(spec, t_eval) for spec in specs])
        assert np.array_equal(s.applied_vector_potential, want), (k, s.step)
    assert list(tm["scales"]) == [float(g["ramp_final"]), float(g["table_values"][-1])]
    assert max_abs(y.applied_vector_potential, x.applied_vector_potential) < 1e-12


def test_the_lag_rule_survives_the_sum(direct_solve, monkeypatch):
    """traj_dynamic_lag (the reference's ramp 30 -> 31 moving A by less than np.allclose's tolerance per step: dA/dt
    follows, the links stay put) with the ramp split as 30 A_base + ramp(0 -> 1) A_base: that fixture's checks at 1e-8."""
    g = load_golden("traj_dynamic_lag")
    o = options_from_golden(g)
    opts = _options(solve_time=o.solve_time, dt_init=o.dt_init, dt_max=o.dt_max, adaptive=False, save_every=o.save_every)
    A_base = g["A_base"]
    tmin, tmax, initial, final = (float(g["ramp_" + k]) for k in ("tmin", "tmax", "initial", "final"))
    ramp = dict(tmin=tmin, tmax=tmax, initial=0.0, final=final - initial)
    run = _solve(monkeypatch, opts, vector_potential_terms=(initial * A_base, [(A_base, ramp)]))
    _assert_like_fixture(g, run["sol"], 1e-8)
    t_last = float(g["call_time"][-1])
    want = initial * A_base + factor_value(ramp, t_last) * A_base
    assert np.array_equal(run["sol"].tdgl_data.applied_vector_potential, want)
    assert run["stats"]["host_syncs"] < 0.2 * run["stats"]["steps"]


def test_the_device_evaluates_the_terms_and_skips_what_does_not_move(direct_solve, monkeypatch):
    """Far fewer synchronisations than steps (the threshold of tests/test_hip_field_table.py), and the edge pass runs
    exactly in the steps the step rule says: not during the joint hold, not after both terms have settled."""
    g = _golden()
    tm, cl, ref = _run("terms", monkeypatch), _run("terms_classic", monkeypatch), _run("callable", monkeypatch)
    st = tm["stats"]
    assert st["steps"] == ref["stats"]["steps"] == len(g["call_dt"])
    print("host syncs per step: terms", st["host_syncs"] / st["steps"], "callable", ref["stats"]["host_syncs"] / ref["stats"]["steps"])
    assert st["host_syncs"] / st["steps"] < 1.0
    assert st["host_syncs"] < 0.2 * st["steps"]
    assert ref["stats"]["host_syncs"] / ref["stats"]["steps"] >= 1.0
    rule = StepRule([spec for _, spec in fixture_terms(g)[1]])
    t = np.concatenate([[0.0], tm["sol"].dynamics.time[:-1]])  # the time every step began at
    kinds = [rule.begin_step(float(x)) for x in t]
    hold = [k for k, x in zip(kinds, t) if float(g["ramp_tmax"]) < x < float(g["table_times"][2])]
    assert hold.count("skip") >= 3 and kinds.count("settled") >= 3 and kinds.count("move") < len(kinds) - 6
    assert tm["moves"] == cl["moves"] == rule.moves == kinds.count("move")


def _short(monkeypatch, terms, **kw):
    return _solve(monkeypatch, _options(**kw), vector_potential_terms=terms)


def test_one_term_with_a_static_part(direct_solve, monkeypatch):
    mesh = _mesh()
    A0, A1 = uniform_field_A(mesh, 0.1), uniform_field_A(mesh, 0.2)
    ramp = dict(tmin=0.1, tmax=0.6, initial=0.25, final=1.0)
    run = _short(monkeypatch, (A0, [(A1, ramp)]))
    want = _solve(monkeypatch, _options(), A=A0 + 0.25 * A1, vector_potential_func=lambda t: A0 + factor_value(ramp, t) * A1)
    a, b = run["sol"], want["sol"]
    assert len(a.dynamics.dt) == len(b.dynamics.dt) > 10
    assert max_abs(a.dynamics.dt, b.dynamics.dt) <= TOL * b.dynamics.dt.max()
    assert max_abs(np.abs(a.tdgl_data.psi) ** 2, np.abs(b.tdgl_data.psi) ** 2) < TOL
    assert max_abs(a.tdgl_data.supercurrent, b.tdgl_data.supercurrent) < TOL
    assert np.array_equal(a.tdgl_data.applied_vector_potential, A0 + 1.0 * A1)
    assert list(run["scales"]) == [1.0]


def test_four_terms(direct_solve, monkeypatch):
    """K = FIELD_TERMS_MAX: two ramps and two tables over four different bases, one factor falling, with a static part."""
    mesh = _mesh()
    A0 = uniform_field_A(mesh, 0.05)
    bases = [uniform_field_A(mesh, 0.1), flux_spot_A(mesh, -4.0, 3.0, 1.5, 2.0), uniform_field_A(mesh, -0.08),
             flux_spot_A(mesh, 2.0, 2.0, 2.5, -3.0)]
    specs = [dict(tmin=0.05, tmax=0.5, initial=0.0, final=1.0), ([0.1, 0.3, 0.45, 0.7], [0.0, 1.0, 1.0, 0.2]),
             dict(tmin=0.2, tmax=0.9, initial=1.0, final=-0.5), ([0.0, 0.8], [0.3, 1.0])]
    run = _short(monkeypatch, (A0, list(zip(bases, specs))))
    want = _solve(monkeypatch, _options(), A=terms_sum(A0, bases, [factor_value(s, 0.0) for s in specs]),
                  vector_potential_func=lambda t: terms_sum(A0, bases, [factor_value(s, t) for s in specs]))
    a, b = run["sol"], want["sol"]
    assert len(a.dynamics.dt) == len(b.dynamics.dt) > 10
    assert max_abs(a.dynamics.dt, b.dynamics.dt) <= TOL * b.dynamics.dt.max()
    assert max_abs(np.abs(a.tdgl_data.psi) ** 2, np.abs(b.tdgl_data.psi) ** 2) < TOL
    assert max_abs(a.tdgl_data.supercurrent, b.tdgl_data.supercurrent) < TOL
    assert max_abs(a.tdgl_data.normal_current, b.tdgl_data.normal_current) < TOL
    assert np.array_equal(a.saved_steps[0].applied_vector_potential, terms_sum(A0, bases, [factor_value(s, 0.0) for s in specs]))
    assert np.array_equal(a.tdgl_data.applied_vector_potential, terms_sum(A0, bases, [1.0, 0.2, -0.5, 1.0]))
    assert list(run["scales"]) == [1.0, 0.2, -0.5, 1.0]
    assert 0 < run["moves"] < run["stats"]["steps"]


def test_two_terms_without_a_static_part_and_a_factor_that_starts_at_zero(direct_solve, monkeypatch):
    mesh = _mesh()
    A1, A2 = uniform_field_A(mesh, 0.15), uniform_field_A(mesh, -0.05)
    specs = [([0.2, 0.5], [0.0, 1.0]), dict(tmin=0.0, tmax=0.4, initial=1.0, final=0.5)]
    run = _short(monkeypatch, (None, [(A1, specs[0]), (A2, specs[1])]))
    want = _solve(monkeypatch, _options(), A=0.0 * A1 + 1.0 * A2,
                  vector_potential_func=lambda t: factor_value(specs[0], t) * A1 + factor_value(specs[1], t) * A2)
    a, b = run["sol"], want["sol"]
    assert len(a.dynamics.dt) == len(b.dynamics.dt) > 10
    assert max_abs(a.dynamics.dt, b.dynamics.dt) <= TOL * b.dynamics.dt.max()
    assert max_abs(np.abs(a.tdgl_data.psi) ** 2, np.abs(b.tdgl_data.psi) ** 2) < TOL
    assert max_abs(a.tdgl_data.supercurrent, b.tdgl_data.supercurrent) < TOL
    # the first saved step is the field at t = 0, where the first factor is 0: the sum starts from the first product
    assert np.array_equal(a.saved_steps[0].applied_vector_potential, 0.0 * A1 + 1.0 * A2)
    assert np.array_equal(a.tdgl_data.applied_vector_potential, 1.0 * A1 + 0.5 * A2)
    assert list(run["scales"]) == [1.0, 0.5]


# one factor two ways: a LinearRamp, and a three-node table that holds its first value (the step rule skips there) and then rises
ONE_FACTOR = {"ramp": dict(tmin=0.1, tmax=0.6, initial=0.25, final=1.0), "table": ([0.05, 0.35, 0.7], [0.4, 0.4, 1.0])}


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "classic"])
@pytest.mark.parametrize("form", ["ramp", "table"])
def test_a_single_product_and_a_sum_of_one_term_are_one_field(direct_solve, monkeypatch, form, run_ahead):
    """A(t) = f(t) A_1 described through the single product's entry points (`vector_potential_ramp` /
    `vector_potential_table`) and as `vector_potential_terms=(None, [(A_1, spec)])`: one drive, one step rule and one links
    kernel behind both, so nothing may differ -- in the run-ahead loop and in the loop with one synchronisation per step."""
    A1 = uniform_field_A(_mesh(), 0.2)
    spec = ONE_FACTOR[form]
    single_kw = dict(vector_potential_ramp=(A1, spec)) if form == "ramp" else dict(vector_potential_table=(A1, *spec))
    one = _solve(monkeypatch, _options(), run_ahead=run_ahead, A=factor_value(spec, 0.0) * A1, **single_kw)
    summed = _solve(monkeypatch, _options(), run_ahead=run_ahead, vector_potential_terms=(None, [(A1, spec)]))
    a, b = one["sol"], summed["sol"]
    assert len(a.dynamics.dt) > 10 and one["device_evaluates"] and summed["device_evaluates"]
    assert np.array_equal(a.dynamics.dt, b.dynamics.dt)
    assert np.array_equal(a.tdgl_data.psi, b.tdgl_data.psi)
    assert np.array_equal(a.tdgl_data.mu, b.tdgl_data.mu)
    assert np.array_equal(a.tdgl_data.supercurrent, b.tdgl_data.supercurrent)
    assert np.array_equal(a.tdgl_data.normal_current, b.tdgl_data.normal_current)
    assert len(a.saved_steps) == len(b.saved_steps) >= 2
    for s, t in zip(a.saved_steps, b.saved_steps):
        assert np.array_equal(s.applied_vector_potential, t.applied_vector_potential)
    assert len(one["scales"]) == 0 and list(summed["scales"]) == [one["link_scale"]] == [1.0]


def test_a_single_product_keeps_its_own_entry_points(direct_solve, monkeypatch):
    """TabulatedRamp * <static field> with no static part still goes through tdgl_set_link_exponents_base and
    tdgl_set_link_table, and a sum goes through tdgl_set_link_terms: seen by spying on the context's methods."""
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box
    from tdgl_amd.hipcore import TDGLContext

    calls = []
    for name in ("set_link_exponents_base", "set_link_table", "set_link_ramp", "set_link_terms", "set_link_exponents"):
        def spy(self, *a, _name=name, _real=getattr(TDGLContext, name), **k):
            calls.append(_name)
            return _real(self, *a, **k)

        monkeypatch.setattr(TDGLContext, name, spy)
    monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    dev = tdgl.Device("film", layer=layer, film=tdgl.Polygon("film", points=box(4, 3)), length_units="um")
    dev.make_mesh(max_edge_length=0.3)
    opts = tdgl.SolverOptions(solve_time=0.5, dt_init=1e-4, field_units="mT", current_units="uA", pcg_rtol=1e-12)
    field = tdgl.ConstantField(1.0, field_units="mT", length_units="um")
    wave = tdgl.TabulatedRamp([0.1, 0.3], [0.0, 1.0])
    single = tdgl.TDGLSolver(dev, opts, applied_vector_potential=wave * field)
    assert calls == ["set_link_exponents_base", "set_link_table"] and single.field.kind == "table"
    single.ctx.close()
    del calls[:]
    summed = tdgl.TDGLSolver(dev, opts, applied_vector_potential=tdgl.ConstantField(0.5) + wave * field)
    assert calls == ["set_link_terms"] and summed.field.kind == "terms" and summed.device_evaluates_field()
    sol = summed.solve()
    ex, ey = summed.edge_centers[:, 0], summed.edge_centers[:, 1]
    want = summed.A_scale * (np.asarray(tdgl.ConstantField(0.5)(ex, ey, summed.z0))[:, :2] + np.asarray(field(ex, ey, summed.z0))[:, :2])
    assert max_abs(sol.tdgl_data.applied_vector_potential, want) < 1e-12 * np.abs(want).max()
    assert list(summed.ctx.link_term_scales()) == [1.0]
    summed.ctx.close()


def _assert_like_single(ens, one, tol):
    """A replica of an ensemble against tdgl.solve of that replica alone
    (tests/test_hip_ensemble_dynamic.py::_assert_like_single)."""
    assert ens.stats["mu_solver"] == "dense_ensemble"
    assert ens.stats["steps_simulating"] == one.stats["steps_simulating"]
    assert ens.dynamic_vector_potential == one.dynamic_vector_potential
    a, b = ens.dynamics, one.dynamics
    assert len(a.dt) == len(b.dt)
    assert max_abs(a.dt, b.dt) <= tol * b.dt.max()
    assert max_abs(a.time, b.time) <= tol * max(1.0, b.time.max())
    assert [s.step for s in ens.saved_steps] == [s.step for s in one.saved_steps]
    x, y = ens.tdgl_data, one.tdgl_data
    scale = max(1.0, np.abs(remove_mean(y.mu)).max())
    print("ensemble against single: |psi|^2", float(max_abs(np.abs(x.psi) ** 2, np.abs(y.psi) ** 2)),
          "mu", float(max_abs(remove_mean(x.mu), remove_mean(y.mu)) / scale), "J_s", float(max_abs(x.supercurrent, y.supercurrent)),
          "J_n", float(max_abs(x.normal_current, y.normal_current)))
    assert max_abs(np.abs(x.psi) ** 2, np.abs(y.psi) ** 2) < tol
    assert max_abs(remove_mean(x.mu), remove_mean(y.mu)) < tol * scale
    assert max_abs(x.supercurrent, y.supercurrent) < tol * max(1.0, np.abs(y.supercurrent).max())
    assert max_abs(x.normal_current, y.normal_current) < tol * max(1.0, np.abs(y.normal_current).max())
    assert max_abs(a.mu[0] - a.mu[1], b.mu[0] - b.mu[1]) < tol * max(scale, np.abs(b.mu[0] - b.mu[1]).max())
    assert max_abs(np.exp(1j * (a.theta[0] - a.theta[1])), np.exp(1j * (b.theta[0] - b.theta[1]))) < tol
    for s, t in zip(ens.saved_steps, one.saved_steps):
        assert max_abs(s.applied_vector_potential, t.applied_vector_potential) < tol * max(1.0, np.abs(t.applied_vector_potential).max())


def test_ensemble_of_a_static_a_tabulated_and_a_two_term_replica(direct_solve, monkeypatch):
    """R = 4: a static field, a single table, the fixture's two-term sum and a single LinearRamp product in one ensemble
    (every kind of replica behind the one pair of field launches), each replica against the
    single run of the same input with the checks, the tolerance (1e-8) and the options of
    tests/test_hip_ensemble_dynamic.py::test_field_ramps_with_lagging_links: fixed dt = 1e-3, pcg_rtol 1e-12."""
    from tdgl_amd.ensemble import ensemble_dimensionless

    g = _golden()
    opts = _options(solve_time=3.3, dt_init=1e-3, dt_max=1e-3, adaptive=False, save_every=1000)
    monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    terms = fixture_terms(g)
    table = (g["A1"], [0.3, 1.1, 2.0], [0.2, 1.0, -0.4])
    static = 0.8 * g["A1"]
    ramp = (g["A1"], dict(tmin=0.4, tmax=2.5, initial=0.1, final=0.9))
    sols = ensemble_dimensionless(_mesh(), opts, [static, None, None, None], 1.0, U_DEFAULT, GAMMA_DEFAULT, probe_points=PROBES,
                                  vector_potential_table=[None, table, None, None], vector_potential_terms=[None, None, terms, None],
                                  vector_potential_ramp=[None, None, None, ramp]).solve()
    assert len(sols) == 4
    singles = [
        _solve(monkeypatch, opts, A=static)["sol"],
        _solve(monkeypatch, opts, A=0.2 * g["A1"], vector_potential_table=table)["sol"],
        _solve(monkeypatch, opts, vector_potential_terms=terms)["sol"],
        _solve(monkeypatch, opts, A=0.1 * g["A1"], vector_potential_ramp=ramp)["sol"],
    ]
    for r in range(4):
        _assert_like_single(sols[r], singles[r], 1e-8)
    # the two-term replica ended settled, its saved A the sum at the end values, exactly as the single run's
    assert np.array_equal(sols[2].tdgl_data.applied_vector_potential, singles[2].tdgl_data.applied_vector_potential)
    want = terms_sum(terms[0], [g["A1"], g["A2"]], [float(g["ramp_final"]), float(g["table_values"][-1])])
    assert np.array_equal(sols[2].tdgl_data.applied_vector_potential, want)


def _terms_c_args(m, A0, terms):
    from tdgl_amd.hipcore import link_terms_args

    return link_terms_args(m, A0, terms)


def test_refused_terms_leave_a_working_field_in_force(direct_solve, monkeypatch):
    """tdgl_set_link_terms, tdgl_update_link_terms and tdgl_ensemble_set_link_terms return TDGL_ERR_ARG for a null base,
    n_terms of 0 or 5, non-increasing times, a non-finite value and tmax <= tmin -- and the field set before still runs."""
    from tdgl_amd import TDGLSolver, _lib
    from tdgl_amd.ensemble import EnsembleContext

    monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    mesh = _mesh()
    m = len(mesh.edge_mesh.edges)
    A0, A1 = uniform_field_A(mesh, 0.1), uniform_field_A(mesh, 0.2)
    ramp = dict(tmin=0.0, tmax=0.5, initial=0.0, final=1.0)
    good = (A0, [(A1, ramp), (A1, ([0.1, 0.4], [0.0, 0.5]))])
    solver = TDGLSolver.from_dimensionless(mesh, _options(), terms_sum(A0, [A1, A1], [0.0, 0.0]), 1.0, U_DEFAULT, GAMMA_DEFAULT,
                                           vector_potential_terms=good)
    ctx, lib = solver.ctx, _lib.load()
    ERR_ARG = _lib.TDGL_ERR_ARG
    bad_ramp = dict(ramp, tmax=0.0)
    cases = {
        "n_terms = 5": (A0, [(A1, ramp)] * 5),
        "non-increasing times": (A0, [(A1, ([0.1, 0.1], [0.0, 1.0]))]),
        "a non-finite value": (A0, [(A1, ([0.1, 0.2], [0.0, np.inf]))]),
        "a non-finite ramp": (A0, [(A1, dict(ramp, final=np.nan))]),
        "tmax <= tmin": (A0, [(A1, bad_ramp)]),
    }

    def refused_by(call):
        for name, (a0, terms) in cases.items():
            assert call(*_terms_c_args(m, a0, terms)) == ERR_ARG, name
        args = list(_terms_c_args(m, A0, [(A1, ramp)]))
        assert call(*(args[:1] + [0] + args[2:])) == ERR_ARG, "n_terms = 0"
        assert call(*(args[:2] + [None] + args[3:])) == ERR_ARG, "null base"

    def still_works():
        ctx.set_state(solver.psi_init, solver.mu_init)
        ctx.begin_stage()
        res = ctx.run(40)
        assert len(res["dt"]) == 40 and 0.0 < ctx.link_term_scales()[0] <= 1.0 and len(ctx.link_term_scales()) == 2

    refused_by(lambda *a: lib.tdgl_set_link_terms(ctx._ctx, *a))
    still_works()
    # tdgl_update_link_terms: null factors, a non-finite factor, dt_prev <= 0
    two = np.array([0.5, 0.25])
    ptr = two.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.tdgl_update_link_terms(ctx._ctx, None, 1e-3) == ERR_ARG
    assert lib.tdgl_update_link_terms(ctx._ctx, np.array([0.5, np.nan]).ctypes.data_as(C.POINTER(C.c_double)), 1e-3) == ERR_ARG
    assert lib.tdgl_update_link_terms(ctx._ctx, ptr, 0.0) == ERR_ARG
    still_works()
    ctx.update_link_terms(two, 1e-3)
    assert list(ctx.link_term_scales()) == [0.5, 0.25]
    # the ensemble twin: a refused argument leaves the replica's field as it was
    ens = EnsembleContext(ctx, 2)
    try:
        ens.set_link_terms(1, *good)
        refused_by(lambda *a: lib.tdgl_ensemble_set_link_terms(ens._ens, 1, *a))
        assert list(ens.link_term_scales(1)) == [0.0, 0.0] and len(ens.link_term_scales(0)) == 0
    finally:
        ens.close()
    ctx.close()
