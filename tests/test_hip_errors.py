"""GPU tests of the C ABI's error behaviour and of degenerate inputs: every failure comes back
as a status + message (ValueError for bad arguments / call order, RuntimeError otherwise), never
as a crash, and the smallest possible meshes run."""

import copy

import numpy as np
import pytest

from conftest import load_golden
from helpers import (GAMMA_DEFAULT, U_DEFAULT, edge_terminal, max_abs, reference_mesh, remove_mean, synthetic_mesh,
                     uniform_field_A)

pytestmark = pytest.mark.gpu


def _ctx(mesh, **kw):
    from tdgl_amd.hipcore import TDGLContext

    return TDGLContext(mesh, **kw)


def test_invalid_meshes_are_rejected_with_a_message():
    mesh = synthetic_mesh(6)
    bad = copy.deepcopy(mesh)
    bad.edge_mesh.edges = bad.edge_mesh.edges.copy()
    bad.edge_mesh.edges[3, 1] = len(mesh.sites) + 5
    with pytest.raises(ValueError, match=r"edge 3 has invalid sites"):
        _ctx(bad, reorder="none")  # (the RCM ordering of the host layer would already choke on it)
    bad = copy.deepcopy(mesh)
    bad.edge_mesh.edge_lengths = bad.edge_mesh.edge_lengths.copy()
    bad.edge_mesh.edge_lengths[0] = 0.0
    with pytest.raises(ValueError, match="non-positive length"):
        _ctx(bad)
    with pytest.raises(ValueError):
        _ctx(mesh, fixed_sites=[len(mesh.sites) + 1])


def test_call_order_and_shapes():
    mesh = synthetic_mesh(8)
    ctx = _ctx(mesh)
    n, m = ctx.n, ctx.m
    with pytest.raises(RuntimeError, match="no AMG hierarchy"):
        ctx.poisson_solve(np.zeros(n))
    ctx.build_poisson()
    ctx.set_state(np.ones(n, dtype=complex), np.zeros(n))
    with pytest.raises(RuntimeError, match="set link exponents, epsilon and state first"):
        ctx.run(1)
    with pytest.raises(ValueError, match="Unexpected shape for vector_potential"):
        ctx.set_link_exponents(np.zeros((m + 1, 2)))
    with pytest.raises(RuntimeError, match="call tdgl_set_link_exponents first"):
        ctx.update_link_exponents(np.zeros((m, 2)), 1e-3)
    ctx.set_link_exponents(np.zeros((m, 2)))
    with pytest.raises(ValueError, match="dt_prev must be > 0"):
        ctx.update_link_exponents(np.zeros((m, 2)), 0.0)
    with pytest.raises(RuntimeError, match="screening is not enabled"):
        ctx.set_induced_vector_potential(np.zeros((m, 2)))
    with pytest.raises(ValueError, match="has no coarse-level transfer"):
        ctx._chk(ctx._lib.tdgl_poisson_set_fused_level(ctx._ctx, 0, None, None, None, None, None, None, None))
    with pytest.raises(ValueError, match="screening_step_drag must be in"):
        ctx.set_screening(mesh.sites, mesh.edge_mesh.centers, mesh.areas, step_drag=0.0)
    ctx.close()


def test_poisson_iteration_budget_is_reported():
    mesh = synthetic_mesh(40)
    ctx = _ctx(mesh)
    ctx.build_poisson(rtol=1e-13, max_iter=2)
    rhs = np.random.default_rng(0).normal(size=ctx.n)
    rhs -= (rhs * mesh.areas).sum() / mesh.areas.sum()
    # (2 iterations with the fp32-stored level-0 operators + the fp64 restart's 2)
    with pytest.raises(RuntimeError, match=r"Poisson solve did not converge: relative residual .* after 4 iterations"):
        ctx.poisson_solve(rhs)
    ctx.set_poisson_options(rtol=1e-13, max_iter=2, precond_fp32=False)
    with pytest.raises(RuntimeError, match=r"Poisson solve did not converge: relative residual .* after 2 iterations"):
        ctx.poisson_solve(rhs)
    ctx.set_poisson_options(rtol=1e-10, max_iter=200)
    mu, iters, relres = ctx.poisson_solve(rhs)
    assert relres <= 1e-10 and iters > 4
    # safety net: a budget just short of what the fp32-stored preconditioner needs is followed by
    # a restart with the fp64 operators from the current iterate, which then converges
    ctx.set_poisson_options(rtol=1e-10, max_iter=iters - 2)
    mu2, iters2, relres2 = ctx.poisson_solve(rhs)
    assert relres2 <= 1e-10 and iters - 2 < iters2 <= 2 * (iters - 2)
    assert max_abs(mu2, mu) < 1e-8 * np.abs(mu).max()
    ctx.close()


def test_inconsistent_halo_plan_is_rejected():
    from tdgl_amd.partition import build_local_problem, rcb_partition

    mesh = synthetic_mesh(20)
    part = rcb_partition(mesh.sites, 2)
    lp = build_local_problem(mesh, part, 0)
    ctx = _ctx(lp.mesh, n_owned=lp.n_own)
    wrong = copy.deepcopy(lp)
    nb = wrong.neighbors[0]
    a, b = wrong.recv_range[nb]
    wrong.recv_range[nb] = (a, b - 1)  # one ghost short
    with pytest.raises(ValueError, match="ghost sites"):
        ctx.set_halo_plan(wrong)
    ctx.set_halo_plan(lp)
    assert ctx.comm_overlap()[1] % 256 == 0
    ctx.close()


def test_vcycle_stored_is_refused_where_the_cg_applies_the_fp64_cycle():
    """`tdgl_vcycle_stored` answers for the cycle in reduced storage alone: every state in which the CG would apply the
    fp64 one (`tdgl_vcycle`) is a refusal with its reason, and so is a rank of a decomposed run."""
    from tdgl_amd.partition import build_local_problem, rcb_partition

    mesh = synthetic_mesh(40)
    ctx = _ctx(mesh)
    r = np.zeros(ctx.n)
    with pytest.raises(RuntimeError, match="tdgl_vcycle_stored: no AMG hierarchy"):
        ctx.vcycle_stored(r)
    assert ctx.index_forms()["levels"] == 0 and ctx.index_forms()["A16"] is None
    h = ctx.build_poisson()
    assert len(h.levels) >= 2
    ctx.set_poisson_options(precond_fp32=False)
    with pytest.raises(RuntimeError, match=r"stored in fp64 \(precond_fp32 = 0\)"):
        ctx.vcycle_stored(r)
    ctx.set_poisson_options(nu_fine=2)
    with pytest.raises(RuntimeError, match="level-0 smoother has a degree other than 1"):
        ctx.vcycle_stored(r, r)
    ctx.set_poisson_options(fused_restriction=False)
    with pytest.raises(RuntimeError, match="no fused restriction for the level-0 coefficient in use"):
        ctx.vcycle_stored(r)
    ctx.set_poisson_options()
    z, rz, qz = ctx.vcycle_stored(r, r)  # (and the defaults are served: zero in, zero out)
    assert not z.any() and rz == 0.0 and qz == 0.0 and ctx.precond_storage() == 2
    ctx.close()
    ctx = _ctx(synthetic_mesh(8))
    h = ctx.build_poisson()
    assert len(h.levels) == 1
    with pytest.raises(RuntimeError, match="the hierarchy has a single level"):
        ctx.vcycle_stored(np.zeros(ctx.n))
    ctx.close()
    lp = build_local_problem(mesh, rcb_partition(mesh.sites, 2), 0)
    ctx = _ctx(lp.mesh, n_owned=lp.n_own)
    with pytest.raises(RuntimeError, match="tdgl_vcycle_stored: single-GPU contexts only"):
        ctx.vcycle_stored(np.zeros(ctx.n))
    ctx.close()


@pytest.mark.parametrize("shape", ["two_triangles", "one_triangle"])
def test_smallest_meshes_run(shape):
    """4 sites / 5 edges and 3 sites / 3 edges: every site on the boundary, single-level
    hierarchy (dense coarse solve only), one SELL slice with 60 padded lanes.  The reference
    cannot serve as the checker here (SuperLU reports "Factor is exactly singular" for the
    pure-Neumann matrix at this size), so the step is checked through its defining equations,
    built from the oracle's operator matrices."""
    from oracle.fv_operators import divergence_matrix, gradient_matrix, laplacian_matrix
    from tdgl_amd import SolverOptions, TDGLSolver
    from tdgl_amd.finite_volume import Mesh

    if shape == "two_triangles":
        pts = np.array([[0.0, 0.0], [1.0, 0.05], [0.55, 0.8], [1.5, 0.9]])
        tri = np.array([[0, 1, 2], [1, 3, 2]])
    else:
        pts = np.array([[0.0, 0.0], [1.0, 0.0], [0.45, 0.75]])
        tri = np.array([[0, 1, 2]])
    mesh = Mesh.from_triangulation(pts, tri)
    assert mesh.edge_mesh.dual_edge_lengths.min() > 0
    opts = SolverOptions(solve_time=1e9, dt_init=1e-3, dt_max=1e-1, save_every=10**9, pcg_rtol=1e-13)
    solver = TDGLSolver.from_dimensionless(mesh, opts, uniform_field_A(mesh, 0.7), 0.8, U_DEFAULT, GAMMA_DEFAULT)
    ctx = solver.ctx
    ctx.set_state(solver.psi_init, solver.mu_init)
    ctx.begin_stage()
    res = ctx.run(30)
    got = ctx.get_state()
    assert len(res["dt"]) == 30 and np.all(res["pcg_iters"] <= 2)
    assert np.all(np.isfinite(got["psi"])) and 0.5 < np.abs(got["psi"]).min() <= np.abs(got["psi"]).max() <= 1.0
    # mu solves L mu = div J_s (solver.py:507-516) and J_n = -grad mu (solver.py:519)
    lap, _ = laplacian_matrix(mesh)
    rhs = divergence_matrix(mesh) @ got["supercurrent"]
    assert max_abs(lap @ got["mu"], rhs) < 1e-10 * max(1.0, np.abs(rhs).max())
    assert max_abs(got["normal_current"], -(gradient_matrix(mesh) @ got["mu"])) < 1e-12
    assert abs(got["mu"].mean()) < 1e-12
    # total current is divergence free
    assert max_abs(divergence_matrix(mesh) @ (got["supercurrent"] + got["normal_current"]), 0 * rhs) < 1e-9


def _small_transport_solver(probes=True):
    from helpers import edge_terminal
    from tdgl_amd import SolverOptions, TDGLSolver

    mesh = synthetic_mesh(40, 12)
    terms = [edge_terminal(mesh, "source", -20.0), edge_terminal(mesh, "drain", 20.0)]
    opts = SolverOptions(solve_time=1e9, dt_init=1e-4, save_every=10**9)
    solver = TDGLSolver.from_dimensionless(
        mesh, opts, uniform_field_A(mesh, 0.02), 1.0, U_DEFAULT, GAMMA_DEFAULT, terminal_info=terms,
        current_func={"source": 3.0, "drain": -3.0},
        probe_points=[mesh.closest_site((-10, 0)), mesh.closest_site((10, 0))] if probes else None,
    )
    solver.ctx.set_state(solver.psi_init, solver.mu_init)
    solver.ctx.begin_stage()
    solver.update_mu_boundary(0.0)
    return mesh, solver


def test_probe_ring_buffer_wraps_and_matches_short_batches():
    """Probe read-outs (running state "mu" / "theta", solver.py:690-694) live in a device ring buffer of
    1024 steps that `tdgl_run` flushes when it fills and when the batch ends: one call of 2,500 steps
    must return the very trace that 25 calls of 100 steps return, and probes must not change a step."""
    n_steps = 2500
    mesh, one = _small_transport_solver()
    a = one.ctx.run(n_steps)
    assert a["mu"].shape == (n_steps, 2) and np.all(np.isfinite(a["mu"])) and np.all(np.isfinite(a["theta"]))
    assert one.ctx.step_stats()["host_syncs"] <= 2 * n_steps + 3 + a["pcg_iters"].sum()  # flushes: 3, not 2,500
    _, many = _small_transport_solver()
    parts = [many.ctx.run(100) for _ in range(n_steps // 100)]
    for key in ("dt", "mu", "theta"):
        assert np.array_equal(a[key], np.concatenate([p[key] for p in parts])), key
    st = one.ctx.get_state()
    probes = [mesh.closest_site((-10, 0)), mesh.closest_site((10, 0))]
    assert np.array_equal(a["mu"][-1], st["mu"][probes])
    _, bare = _small_transport_solver(probes=False)
    b = bare.ctx.run(n_steps)
    assert b["mu"] is None and np.array_equal(b["dt"], a["dt"])
    assert np.array_equal(bare.ctx.get_state()["psi"], st["psi"])


def test_run_restarts_from_recorded_controller_state():
    """`tdgl_get/set_controller_state` + `tdgl_set_loop_state` + `tdgl_set_state`: a run restarted from a
    recorded point takes the dt sequence the uninterrupted run took (the list d_psi_sq_vals persists
    in the reference, solver.py:318, 698-707)."""
    _, s = _small_transport_solver()
    ctx = s.ctx
    ctx.run(137)
    st, ls, cs = ctx.get_state(), ctx.loop_state(), ctx.controller_state()
    assert len(cs["history"]) >= 10 and cs["tentative_dt"] == ls["tentative_dt"]
    cont = ctx.run(60)
    end = ctx.get_state()
    _, t = _small_transport_solver()
    t.ctx.set_state(st["psi"], st["mu"])
    t.ctx.set_loop_state(ls["step"], ls["time"], ls["dt"])
    t.ctx.set_controller_state(cs["tentative_dt"], cs["history"])
    again = t.ctx.run(60)
    assert max_abs(again["dt"], cont["dt"]) <= 1e-9 * cont["dt"].max()
    got = t.ctx.get_state()
    assert max_abs(np.abs(got["psi"]) ** 2, np.abs(end["psi"]) ** 2) < 1e-8
    assert max_abs(remove_mean(got["mu"]), remove_mean(end["mu"])) < 1e-8 * max(1.0, np.abs(end["mu"]).max())
    with pytest.raises(ValueError, match="tentative_dt must be positive"):
        t.ctx.set_controller_state(0.0, [])


def _golden_transport_solver():
    from tdgl_amd import SolverOptions, TDGLSolver

    mesh = reference_mesh(load_golden("mesh_small"))
    terms = [edge_terminal(mesh, "source", -10.0), edge_terminal(mesh, "drain", 10.0)]
    opts = SolverOptions(solve_time=1e9, dt_init=1e-4, save_every=10**9)
    solver = TDGLSolver.from_dimensionless(mesh, opts, uniform_field_A(mesh, 0.1), 1.0, U_DEFAULT, GAMMA_DEFAULT,
                                           terminal_info=terms, current_func={"source": 2.0, "drain": -2.0})
    solver.ctx.set_state(solver.psi_init, solver.mu_init)
    solver.ctx.begin_stage()
    solver.update_mu_boundary(0.0)
    return solver, [np.asarray(t["boundary_edge_indices"], dtype=np.int32) for t in terms]


@pytest.fixture(scope="module")
def run_without_tables():
    """8 steps of the small transport run with no table installed: what a refused table must leave behind."""
    solver, _ = _golden_transport_solver()
    res = solver.ctx.run(8)
    return res["dt"], solver.ctx.get_state()["psi"]


@pytest.mark.parametrize("flaw", ["group_ptr[0] != 0", "group_ptr decreases", "NaN density", "NaN epsilon factor"])
def test_malformed_time_tables_are_refused_and_leave_no_table(flaw, run_without_tables):
    """tdgl_set_mu_boundary_table walks group_pos up to group_ptr[n_groups] and keeps group_ptr for the time loop to
    walk: a group_ptr that does not start at 0 or decreases, a non-finite density and a non-finite epsilon factor
    are TDGL_ERR_ARG (the ensemble's setters always said so), and the run that follows is the run without a table."""
    from tdgl_amd._lib import f64, i32, p_f64, p_i32

    solver, groups = _golden_transport_solver()
    ctx = solver.ctx
    times = f64([0.0, 1e-3, 1.0])
    ptr = i32([0, len(groups[0]), len(groups[0]) + len(groups[1])])
    pos = i32(np.concatenate(groups))
    dens = f64([[0.0, 5.0, 9.0], [0.0, -5.0, -9.0]])  # (installed, it would change the run from the second step on)
    eps0, factor = f64(np.full(ctx.n, 0.8)), f64([1.0, 0.5, 0.2])
    message = flaw
    if flaw == "group_ptr[0] != 0":
        ptr[0], message = 1, "group_ptr must start at 0"
    elif flaw == "group_ptr decreases":
        ptr[1] = ptr[2] + 1
    elif flaw == "NaN density":
        dens[1, 2], message = np.nan, "non-finite density"
    else:
        factor[1], message = np.nan, "non-finite factor"
    with pytest.raises(ValueError, match=message):
        if flaw == "NaN epsilon factor":
            ctx._chk(ctx._lib.tdgl_set_epsilon_table(ctx._ctx, p_f64(eps0), len(times), p_f64(times), p_f64(factor)))
        else:
            ctx._chk(ctx._lib.tdgl_set_mu_boundary_table(ctx._ctx, len(times), p_f64(times), 2, p_i32(ptr), p_i32(pos), p_f64(dens)))
    res = ctx.run(8)
    want_dt, want_psi = run_without_tables
    assert np.array_equal(res["dt"], want_dt)
    assert np.array_equal(ctx.get_state()["psi"], want_psi)
