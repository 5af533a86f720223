"""Moving current loops as applied-field sources on the GPU (tdgl_set_link_loops, tdgl_update_link_loops,
tdgl_get_link_loop_params, tdgl_get_link_exponents): the loop's potential against 40-digit values and the reference's own,
the reference fixture traj_moving_loop_small in both time loops, the two loops against each other bit for bit, against the
same field evaluated in Python once per step, the step rule's skipped edge passes, compositions with terms, the entry
points' refusals and a user-level script.

Everything but the last test runs on fixture mesh_small (516 sites, 1,458 edges: six workgroups of edges, the last one
ragged) with the direct mu solve and pcg_rtol = 1e-12.  The runs several tests look at are made once (`_run`)."""

import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from field_terms_model import factor_value, flux_spot_A, terms_sum
from helpers import GAMMA_DEFAULT, U_DEFAULT, max_abs, reference_mesh, remove_mean, uniform_field_A
from loop_field_model import StepRule, fixture_loop, loop_values, loops_field
from test_hip_field_terms import _assert_like_fixture, _options

pytestmark = pytest.mark.gpu

TOL = 1e-8  # the project's tolerance for time-dependent fields
PROBES = [263, 273]

_cache = {}


def _mesh():
    if "mesh" not in _cache:
        _cache["mesh"] = reference_mesh(load_golden("mesh_small"))
    return _cache["mesh"]


def _golden():
    if "g" not in _cache:
        _cache["g"] = load_golden("traj_moving_loop_small")
    return _cache["g"]


def _solver(monkeypatch, options, A, run_ahead=True, **kw):
    from tdgl_amd import TDGLSolver

    if run_ahead:
        monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    else:
        monkeypatch.setenv("TDGL_NO_RUN_AHEAD", "1")  # (read when the context is created)
    solver = TDGLSolver.from_dimensionless(_mesh(), options, A, 1.0, U_DEFAULT, GAMMA_DEFAULT, probe_points=PROBES, **kw)
    assert solver.ctx.dense_direct
    return solver


def _solve(monkeypatch, options, A, run_ahead=True, **kw):
    solver = _solver(monkeypatch, options, A, run_ahead, **kw)
    solver.ctx.step_stats(reset=True)
    sol = solver.solve()
    out = dict(sol=sol, stats=solver.ctx.step_stats(), params=solver.ctx.link_loop_params(), moves=solver.ctx.link_term_moves(),
               device_evaluates=solver.device_evaluates_field())
    solver.ctx.close()
    return out


def _run(name, monkeypatch):
    """The shared runs of the fixture's field, each made once: on the device in the run-ahead loop ("loops") and in the loop
    with one synchronisation per step ("loops_classic"), and as a Python callable evaluated before every step ("callable")."""
    if name not in _cache:
        g = _golden()
        loop, centres = fixture_loop(g), _mesh().edge_mesh.centers
        if name == "callable":
            _cache[name] = _solve(monkeypatch, _options(g), loops_field(centres, 0.0, [loop], 0.0, g["A0"]),
                                  vector_potential_func=lambda t: loops_field(centres, 0.0, [loop], t, g["A0"]))
        else:
            _cache[name] = _solve(monkeypatch, _options(g), g["A0"], run_ahead=name != "loops_classic", vector_potential_loops=[loop])
    return _cache[name]


# ---- 1. values -------------------------------------------------------------------------------------------------------
def test_loop_potential_against_exact_values_and_the_reference(direct_solve, monkeypatch):
    """The fixture's points as "edge centres", one loop per geometry moved to its place by tdgl_update_link_loops, A read back
    by tdgl_get_link_exponents: |G_dev - G_exact| <= 8 model_worst_rel G_exact everywhere (8: another, still correctly
    rounded order of operations), exactly 0 on the axis, perpendicular to (dx, dy) to 4 ulp, and within 2e-10 G_exact of the
    reference where the reference itself is within 1e-10."""
    f = load_golden("loop_potential_reference")
    bound = 8.0 * float(f["model_worst_rel"])
    assert bound <= 1e-13
    solver = _solver(monkeypatch, _options(), np.zeros((1458, 2)))
    ctx = solver.ctx
    for g, (a, cx, cy, cz) in enumerate(f["geometries"]):
        pts = f["points"][g]
        assert pts.shape == (ctx.m, 2)
        # (set somewhere else with another current, so that the update has something to move)
        ctx.set_link_loops(pts, 0.0, [dict(times=[0.0, 1.0], centers=[[cx + 0.5, cy - 0.25, 2 * cz]] * 2, currents=[0.5, 0.5], radius=a)])
        ctx.update_link_loops(None, [[cx, cy, cz, 1.0]], 1e-3)
        assert np.array_equal(ctx.link_loop_params(), [[cx, cy, cz, 1.0]])
        A = ctx.link_exponents()
        dx, dy = pts[:, 0] - cx, pts[:, 1] - cy
        rho, G_exact = np.hypot(dx, dy), f["G_exact"][g]
        assert rho[0] == 0.0 and A[0, 0] == 0.0 and A[0, 1] == 0.0 and np.all(np.isfinite(A))
        G_dev = np.hypot(A[:, 0], A[:, 1])
        assert np.all((-dy * A[:, 0] + dx * A[:, 1])[1:] > 0)  # (the sense of the current)
        err = np.abs(G_dev - G_exact)
        print("geometry", g, "worst |G_dev - G_exact| / G_exact", float(np.max(err[1:] / G_exact[1:])), "bound", bound)
        assert np.all(err <= bound * G_exact)
        assert np.all(np.abs(A[:, 0] * dx + A[:, 1] * dy) <= 4 * np.spacing(np.abs(A[:, 0] * dx)))
        ok = f["reference_ok"][g]
        ref = f["A_reference"][g] / (float(f["mu_0"]) * float(f["current_uA"]) * 1e-6)
        G_ref = np.hypot(ref[ok, 0], ref[ok, 1])
        print("geometry", g, "worst |G_dev - G_ref| / G_exact on the mask", float(np.max(np.abs(G_dev[ok] - G_ref) / G_exact[ok])))
        assert ok.sum() > 800 and np.all(np.abs(G_dev[ok] - G_ref) <= 2e-10 * G_exact[ok])
    ctx.close()


# ---- 2. the trajectory fixture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["loops", "loops_classic"])
def test_fixture_through_vector_potential_loops(direct_solve, monkeypatch, name):
    """traj_moving_loop_small (a uniform bias and a loop scanned across the film, its current up, held and down through
    zero; the reference evaluated its own loop formula per step) in the run-ahead loop and in the classic loop."""
    g = _golden()
    assert list(g["probe_points"]) == PROBES
    run = _run(name, monkeypatch)
    assert run["device_evaluates"]
    _assert_like_fixture(g, run["sol"], TOL)


# ---- 3. both loops, bit for bit --------------------------------------------------------------------------------------
def test_run_ahead_loop_and_classic_loop_agree_to_the_last_bit(direct_solve, monkeypatch):
    ra, cl = _run("loops", monkeypatch), _run("loops_classic", monkeypatch)
    a, b = ra["sol"], cl["sol"]
    assert np.array_equal(a.dynamics.dt, b.dynamics.dt)
    for name in ("psi", "mu", "supercurrent", "normal_current"):
        assert np.array_equal(getattr(a.tdgl_data, name), getattr(b.tdgl_data, name)), name
    assert len(a.saved_steps) == len(b.saved_steps) >= 3
    for s, t in zip(a.saved_steps, b.saved_steps):
        assert np.array_equal(s.applied_vector_potential, t.applied_vector_potential)
    assert np.array_equal(ra["params"], cl["params"]) and ra["moves"] == cl["moves"]
    g = _golden()
    assert np.array_equal(ra["params"], [list(g["loop_centers"][-1]) + [float(g["loop_currents"][-1])]])


# ---- 4. against the callable -------------------------------------------------------------------------------------------
def test_loops_match_the_callable_evaluated_on_the_host(direct_solve, monkeypatch):
    dev, ref = _run("loops", monkeypatch), _run("callable", monkeypatch)
    a, b = dev["sol"], ref["sol"]
    assert len(a.dynamics.dt) == len(b.dynamics.dt)
    assert max_abs(a.dynamics.dt, b.dynamics.dt) <= TOL * b.dynamics.dt.max()
    x, y = a.tdgl_data, b.tdgl_data
    assert max_abs(np.abs(x.psi) ** 2, np.abs(y.psi) ** 2) < TOL
    assert max_abs(remove_mean(x.mu), remove_mean(y.mu)) < TOL * max(1.0, np.abs(remove_mean(y.mu)).max())
    assert max_abs(x.supercurrent, y.supercurrent) < TOL
    assert max_abs(x.normal_current, y.normal_current) < TOL
    # what is saved is what was applied: the device's A of every saved step against the host's formula
    for s, t in zip(a.saved_steps, b.saved_steps):
        assert max_abs(s.applied_vector_potential, t.applied_vector_potential) < 1e-12


# ---- 5. synchronisations and the step rule ---------------------------------------------------------------------------------
def test_the_device_evaluates_the_loop_and_skips_what_does_not_move(direct_solve, monkeypatch):
    g = _golden()
    dev, cl, ref = _run("loops", monkeypatch), _run("loops_classic", monkeypatch), _run("callable", monkeypatch)
    st = dev["stats"]
    assert st["steps"] == ref["stats"]["steps"] == len(g["call_dt"])
    print("host syncs per step: device", st["host_syncs"] / st["steps"], "callable", ref["stats"]["host_syncs"] / ref["stats"]["steps"])
    assert st["host_syncs"] < 0.2 * st["steps"]
    assert ref["stats"]["host_syncs"] / ref["stats"]["steps"] >= 1.0
    loop = fixture_loop(g)
    rule = StepRule([], [loop])
    t = np.concatenate([[0.0], dev["sol"].dynamics.time[:-1]])  # the time every step began at
    kinds = [rule.begin_step(float(x)) for x in t]
    hold = [k for k, x in zip(kinds, t) if 2.0 < x < 2.3]  # (the path rests from 2.0 to 2.4, the current holds until 2.3)
    assert hold.count("skip") >= 3 and "move" not in hold[2:]
    assert kinds.count("settled") >= 3 and "move" not in kinds[-3:]
    assert dev["moves"] == cl["moves"] == rule.moves == kinds.count("move") < len(kinds) - 6


# ---- 6. composition ---------------------------------------------------------------------------------------------------------
def test_two_loops_two_products_and_a_static_part(direct_solve, monkeypatch):
    mesh = _mesh()
    centres = mesh.edge_mesh.centers
    A0 = uniform_field_A(mesh, 0.05)
    bases = [uniform_field_A(mesh, 0.1), flux_spot_A(mesh, -4.0, 3.0, 1.5, 2.0)]
    specs = [dict(tmin=0.05, tmax=0.5, initial=0.0, final=1.0), ([0.1, 0.3, 0.45, 0.7], [0.0, 1.0, 1.0, 0.2])]
    loops = [dict(times=[0.1, 0.6], centers=[[-3.0, 2.0, 0.8], [2.0, -1.0, 1.2]], currents=[0.0, 1.2], radius=1.5),
             dict(times=[0.0, 0.3, 0.8], centers=[[4.0, 4.0, -0.5]] * 3, currents=[0.5, -0.7, 0.4], radius=0.75)]

    def field(t):
        return loops_field(centres, 0.0, loops, t, terms_sum(A0, bases, [factor_value(s, t) for s in specs]))

    run = _solve(monkeypatch, _options(), None, vector_potential_terms=(A0, list(zip(bases, specs))), vector_potential_loops=loops)
    want = _solve(monkeypatch, _options(), field(0.0), vector_potential_func=field)
    a, b = run["sol"], want["sol"]
    assert run["device_evaluates"] and run["stats"]["host_syncs"] < 0.2 * run["stats"]["steps"]
    assert len(a.dynamics.dt) == len(b.dynamics.dt) > 10
    assert max_abs(a.dynamics.dt, b.dynamics.dt) <= TOL * b.dynamics.dt.max()
    assert max_abs(np.abs(a.tdgl_data.psi) ** 2, np.abs(b.tdgl_data.psi) ** 2) < TOL
    assert max_abs(a.tdgl_data.supercurrent, b.tdgl_data.supercurrent) < TOL
    assert max_abs(a.tdgl_data.normal_current, b.tdgl_data.normal_current) < TOL
    assert max_abs(a.saved_steps[0].applied_vector_potential, field(0.0)) < 1e-12
    assert max_abs(a.tdgl_data.applied_vector_potential, field(1.0)) < 1e-12
    assert np.array_equal(run["params"], [loop_values(lp, 1.0) for lp in loops])
    assert 0 < run["moves"] < run["stats"]["steps"]


def _forty_steps(solver):
    ctx = solver.ctx
    ctx.set_state(solver.psi_init, solver.mu_init)
    ctx.set_controller_state(solver.options.dt_init)
    ctx.set_loop_state(0, 0.0, solver.options.dt_init)
    ctx.begin_stage()
    res = ctx.run(40)
    st = ctx.get_state()
    return res["dt"], st["psi"], st["mu"], ctx.link_exponents()


def _same_runs(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def test_removing_the_loops_restores_the_field_they_were_added_to(direct_solve, monkeypatch):
    """n_loops = 0 after loops on terms: bit for bit the run that never had loops; after loops on a static A: that A."""
    mesh = _mesh()
    centres = mesh.edge_mesh.centers
    A0, A1 = uniform_field_A(mesh, 0.1), uniform_field_A(mesh, 0.2)
    terms = (A0, [(A1, dict(tmin=0.0, tmax=0.5, initial=0.2, final=1.0))])
    loop = dict(times=[0.0, 0.5], centers=[[-2.0, 0.0, 1.0], [2.0, 0.0, 1.0]], currents=[1.0, 1.0], radius=2.0)
    plain = _solver(monkeypatch, _options(), A0 + 0.2 * A1, vector_potential_terms=terms)
    want = _forty_steps(plain)
    plain.ctx.close()
    solver = _solver(monkeypatch, _options(), None, vector_potential_terms=terms, vector_potential_loops=[loop])
    with_loops = _forty_steps(solver)
    assert not np.array_equal(with_loops[1], want[1])
    solver.ctx.set_link_loops(None, 0.0, None)
    assert len(solver.ctx.link_loop_params()) == 0 and len(solver.ctx.link_term_scales()) == 1
    # (the terms stay at the factors in force; a fresh set of terms starts them over, as the undisturbed run did)
    assert np.array_equal(solver.ctx.link_exponents(), A0 + solver.ctx.link_term_scales()[0] * A1)
    solver.ctx.set_link_terms(*terms)
    solver.ctx.set_link_loops(centres, 0.0, [loop])
    solver.ctx.set_link_loops(None, 0.0, None)
    assert _same_runs(_forty_steps(solver), want)
    # another link setter removes the loops too
    solver.ctx.set_link_loops(centres, 0.0, [loop])
    solver.ctx.set_link_exponents(A0)
    assert len(solver.ctx.link_loop_params()) == 0 and np.array_equal(solver.ctx.link_exponents(), A0)
    solver.ctx.set_link_loops(centres, 0.0, [loop])
    assert max_abs(solver.ctx.link_exponents(), loops_field(centres, 0.0, [loop], 0.0, A0)) < 1e-13
    solver.ctx.set_link_loops(None, 0.0, None)
    assert np.array_equal(solver.ctx.link_exponents(), A0)
    solver.ctx.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def _raw_args(m, centres, z_film, loops):
    """tdgl_set_link_loops's arguments without any check on this side."""
    from tdgl_amd._lib import f64, p_f64, p_i32

    off = np.cumsum([0] + [len(lp["times"]) for lp in loops]).astype(np.int32)
    cat = lambda key, j=None: f64(np.concatenate([np.asarray(lp[key], dtype=float) if j is None else np.asarray(lp[key], dtype=float)[:, j]  # noqa: E731
                                                  for lp in loops]))
    return (len(loops), p_f64(f64(centres)), float(z_film), p_f64(f64([lp["radius"] for lp in loops])), p_i32(off), p_f64(cat("times")),
            p_f64(cat("centers", 0)), p_f64(cat("centers", 1)), p_f64(cat("centers", 2)), p_f64(cat("currents")))


def test_refused_loops_leave_a_working_field_in_force(direct_solve, monkeypatch):
    from tdgl_amd import _lib

    mesh = _mesh()
    centres, m = mesh.edge_mesh.centers, len(mesh.edge_mesh.edges)
    A0 = uniform_field_A(mesh, 0.1)
    good = dict(times=[0.0, 0.5], centers=[[-2.0, 0.0, 1.0], [2.0, 0.0, 1.0]], currents=[0.5, 1.0], radius=2.0)
    undisturbed = _solver(monkeypatch, _options(), A0, vector_potential_loops=[good])
    want = _forty_steps(undisturbed)
    undisturbed.ctx.close()
    solver = _solver(monkeypatch, _options(), A0, vector_potential_loops=[good])
    ctx, lib, ERR_ARG = solver.ctx, _lib.load(), _lib.TDGL_ERR_ARG
    bad_centres = centres.copy()
    bad_centres[7, 1] = np.nan
    cases = {
        "three loops": (centres, 0.0, [good] * 3),
        "decreasing times": (centres, 0.0, [dict(good, times=[0.5, 0.0])]),
        "equal times": (centres, 0.0, [dict(good, times=[0.5, 0.5])]),
        "radius 0": (centres, 0.0, [dict(good, radius=0.0)]),
        "a negative radius": (centres, 0.0, [good, dict(good, radius=-1.0)]),
        "a non-finite current": (centres, 0.0, [dict(good, currents=[0.5, np.inf])]),
        "a non-finite centre": (centres, 0.0, [dict(good, centers=[[-2.0, np.nan, 1.0], [2.0, 0.0, 1.0]])]),
        "a non-finite edge centre": (bad_centres, 0.0, [good]),
        "cz == z_film at a node": (centres, 1.0, [good]),
        "cz == z_film at one node": (centres, 0.0, [dict(good, centers=[[-2.0, 0.0, 1.0], [2.0, 0.0, 0.0]])]),
        "the loop's plane crosses the film's": (centres, 0.0, [dict(good, centers=[[-2.0, 0.0, 1.0], [2.0, 0.0, -1.0]])]),
        "a non-finite z_film": (centres, np.nan, [good]),
    }
    for name, (c, z, loops) in cases.items():
        assert lib.tdgl_set_link_loops(ctx._ctx, *_raw_args(m, c, z, loops)) == ERR_ARG, name
    args = list(_raw_args(m, centres, 0.0, [good]))
    assert lib.tdgl_set_link_loops(ctx._ctx, -1, *args[1:]) == ERR_ARG
    for k in (1, 3, 4, 5, 6, 9):
        assert lib.tdgl_set_link_loops(ctx._ctx, *(args[:k] + [None] + args[k + 1:])) == ERR_ARG, f"null argument {k}"
    # tdgl_update_link_loops: null values, a non-finite value, the film's plane, dt_prev <= 0
    ptr = lambda v: np.asarray(v, dtype=float).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    assert lib.tdgl_update_link_loops(ctx._ctx, None, None, 1e-3) == ERR_ARG
    assert lib.tdgl_update_link_loops(ctx._ctx, None, ptr([0.0, np.nan, 1.0, 1.0]), 1e-3) == ERR_ARG
    assert lib.tdgl_update_link_loops(ctx._ctx, None, ptr([0.0, 0.0, 0.0, 1.0]), 1e-3) == ERR_ARG
    assert lib.tdgl_update_link_loops(ctx._ctx, None, ptr([0.0, 0.0, 1.0, 1.0]), 0.0) == ERR_ARG
    assert np.array_equal(ctx.link_loop_params(), [[-2.0, 0.0, 1.0, 0.5]])
    assert _same_runs(_forty_steps(solver), want)
    # the same refusals one level up, as ValueError before anything reaches the library
    for name in ("three loops", "decreasing times", "radius 0", "cz == z_film at a node", "the loop's plane crosses the film's"):
        with pytest.raises(ValueError):
            ctx.set_link_loops(*cases[name])
    # a single ramped product in force: loops are refused, the ramp stays
    ctx.set_link_exponents_base(A0, 0.0)
    ctx.set_link_ramp(tmin=0.0, tmax=1.0, initial=0.0, final=1.0)
    assert lib.tdgl_set_link_loops(ctx._ctx, *args) == ERR_ARG
    assert len(_forty_steps(solver)[0]) == 40 and ctx.link_scale() > 0.0
    ctx.close()


# ---- 8. user level ----------------------------------------------------------------------------------------------------------
def test_user_script_with_a_moving_current_loop(direct_solve, monkeypatch):
    """tdgl.solve with ConstantField + MovingCurrentLoop: evaluated on the device; the same loop hidden in a plain
    time-dependent Parameter (evaluated and uploaded before every step) gives the same run."""
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box

    monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    dev = tdgl.Device("film", layer=layer, film=tdgl.Polygon("film", points=box(4, 3)), length_units="um")
    dev.make_mesh(max_edge_length=0.3)
    opts = tdgl.SolverOptions(solve_time=1.0, dt_init=1e-4, dt_max=0.05, field_units="mT", current_units="mA", pcg_rtol=1e-12,
                              save_every=50)
    loop = tdgl.MovingCurrentLoop([0.1, 0.8], [[-1.5, -0.5, 0.4], [1.5, 0.5, 0.4]], radius=0.6, current=[0.0, 2.0], current_units="mA")
    bias = tdgl.ConstantField(0.3, field_units="mT", length_units="um")
    solver = tdgl.TDGLSolver(dev, opts, applied_vector_potential=bias + loop)
    assert solver.device_evaluates_field() and solver.field.kind == "loops"
    solver.ctx.step_stats(reset=True)
    a = solver.solve()
    st = solver.ctx.step_stats()
    assert st["host_syncs"] < 0.2 * st["steps"]
    solver.ctx.close()

    def hidden(x, y, z, *, t):
        return loop(x, y, z, t=t)

    per_step = tdgl.TDGLSolver(dev, opts, applied_vector_potential=bias + tdgl.Parameter(hidden, time_dependent=True))
    assert not per_step.device_evaluates_field()
    b = per_step.solve()
    per_step.ctx.close()
    assert len(a.dynamics.dt) == len(b.dynamics.dt) > 20
    assert max_abs(a.dynamics.dt, b.dynamics.dt) <= TOL * b.dynamics.dt.max()
    assert max_abs(np.abs(a.tdgl_data.psi) ** 2, np.abs(b.tdgl_data.psi) ** 2) < TOL
    assert max_abs(a.tdgl_data.supercurrent, b.tdgl_data.supercurrent) < TOL * max(1.0, np.abs(b.tdgl_data.supercurrent).max())
    assert np.abs(a.tdgl_data.applied_vector_potential).max() > 0
    assert max_abs(a.tdgl_data.applied_vector_potential, b.tdgl_data.applied_vector_potential) < 1e-12 * np.abs(b.tdgl_data.applied_vector_potential).max()
