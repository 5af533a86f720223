"""What the ledger of the edge currents (loop.inc: EdgeCurrents) calls formed IS formed: after every return of the time
loop, J_s and J_n as the loop's schedule left them are compared with `==` against the currents a second context of the
same solver forms on request from the same psi and mu (tdgl_set_state + tdgl_get_state: the stand-alone
k_edge_currents).  The bit-identity tests of the schedules (tests/test_hip_sync_shadow.py, the run-ahead tests of
tests/test_hip_direct.py) compare one schedule with another and would not see a mistake both share; this one compares
every schedule -- one case per plan value (tdgl_currents_plan), the run-ahead loop included -- with no schedule at all."""
import numpy as np
import pytest

from helpers import GAMMA_DEFAULT, U_DEFAULT, edge_terminal, synthetic_mesh, uniform_field_A

RAMP = dict(tmin=0.0, tmax=3.0, initial=0.0, final=1.0)

# case -> (mesh, direct solve, field ramp, environment switches, currents every step)
CASES = {
    "dense_run_ahead": ("strip", True, False, (), True),                       # owed, taken by the next attempt of a batch
    "dense_with_next_psi": ("strip", True, False, ("TDGL_NO_RUN_AHEAD",), True),
    "dense_ramp_run_ahead": ("strip", True, True, (), True),                   # k_ra_edge_currents in front of the ramp's move
    "dense_ramp_speculative": ("strip", True, True, ("TDGL_NO_RUN_AHEAD",), True),
    "iterative_behind_next_look": ("square", False, False, (), True),
    "iterative_now": ("square", False, False, ("TDGL_NO_SYNC_SHADOW",), True),
    "on_request": ("strip", True, False, (), False),
}


def _solver(mesh_name, ramp, every_step):
    from tdgl_amd import SolverOptions, TDGLSolver

    kw = {}
    if mesh_name == "strip":  # the strip with terminals of the run-ahead tests
        mesh = synthetic_mesh(60, 24)
        kw.update(terminal_info=[edge_terminal(mesh, "source", -30.0), edge_terminal(mesh, "drain", 30.0)],
                  current_func={"source": 9.0, "drain": -9.0})
        field = 0.25
    else:  # the square of the sync-shadow tests
        mesh = synthetic_mesh(64, 64)
        field = 0.4
    A = uniform_field_A(mesh, field)
    if ramp:
        kw["vector_potential_ramp"] = (A, RAMP)
        A = 0.0 * A
    opts = SolverOptions(solve_time=1e9, dt_init=1e-3, dt_max=0.1, save_every=10 ** 6)
    solver = TDGLSolver.from_dimensionless(mesh, opts, A, 1.0, U_DEFAULT, GAMMA_DEFAULT, **kw)
    ctx = solver.ctx
    if not every_step:
        ctx.set_poisson_options(edge_currents_every_step=False)
    ctx.set_state(solver.psi_init, solver.mu_init)
    ctx.begin_stage()
    solver.update_mu_boundary(0.0)
    return solver, ctx, opts


def _ramp_value(t):
    """LinearRamp (tdgl/sources/scaling.py:4-14) in the library's order of operations (kernels.inc: linear_ramp_value)."""
    if t < RAMP["tmin"]:
        return RAMP["initial"]
    if t < RAMP["tmax"]:
        return RAMP["initial"] + (RAMP["final"] - RAMP["initial"]) * (t - RAMP["tmin"]) / (RAMP["tmax"] - RAMP["tmin"])
    return RAMP["final"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_currents_the_loop_left_are_those_formed_on_request(case, request, monkeypatch):
    mesh_name, direct, ramp, switches, every_step = CASES[case]
    if direct:
        request.getfixturevalue("direct_solve")
    for name in ("TDGL_NO_RUN_AHEAD", "TDGL_NO_SYNC_SHADOW"):
        monkeypatch.delenv(name, raising=False)
    for name in switches:  # (read when a context is created)
        monkeypatch.setenv(name, "1")
    _, ctx, opts = _solver(mesh_name, ramp, every_step)
    _, other, _ = _solver(mesh_name, ramp, every_step)
    assert ctx.dense_direct == direct and other.dense_direct == direct
    ctx.step_stats(reset=True)
    time, runner_dt, steps = 0.0, opts.dt_init, 0
    for n in (1, 7, 20):
        res = ctx.run(n)
        assert len(res["dt"]) == n
        steps += n
        got = ctx.get_state()
        for dt in res["dt"]:  # the second context's links follow the ramp: one update in front of every step
            if ramp:
                other.update_link_scale(_ramp_value(time), runner_dt)
            runner_dt = float(dt)
            time += runner_dt
        if ramp:
            assert time < RAMP["tmax"] and ctx.link_scale() == other.link_scale()
        other.set_state(got["psi"], got["mu"])
        want = other.get_state()
        assert np.array_equal(want["psi"], got["psi"]) and np.array_equal(want["mu"], got["mu"])
        for key in ("supercurrent", "normal_current"):
            assert steps < 28 or np.abs(want[key]).max() > 0  # (a ramp starts from no field: no supercurrent at first)
            assert np.array_equal(got[key], want[key]), (case, steps, key, np.abs(got[key] - want[key]).max())
    assert not ramp or ctx.link_scale() > 0.0
    stats = ctx.step_stats()
    print(case, stats)
    assert stats["steps"] == steps == 28
    if not every_step:
        assert stats["edge_current_launches"] == 3  # the three reads
    elif "run_ahead" in case:
        assert stats["host_syncs"] < steps  # (batches; their predicated formations are not counted)
    elif stats["psi_retries"] == 0:  # (a failed attempt of the direct solve has queued them in vain)
        assert stats["edge_current_launches"] == steps
    ctx.close()
    other.close()
