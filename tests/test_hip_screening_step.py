"""The screened time step (`step_screening`, csrc/run.inc; k_site_average, k_induced_vector_potential, k_polyak,
csrc/screening.inc) against the float64 oracle, teacher-forced: the device starts a step from the oracle's recorded
state -- psi, mu, A_induced, the boundary values of mu, the controller's tentative dt -- and is compared one step later,
at sizes where the path runs in more than its smallest configuration (tests/screening_step_model.py: several site
chunks with a partial last tile, several edge blocks, many workgroups behind the error's atomic maximum).

  A  one screening iteration (tolerance 1e300 on both sides: the count cannot differ): every entry of dt, psi (|psi|^2 and
     phase-aligned), mu without its mean, J_s, J_n and A_induced = A0 + alpha (A_new - A0) within 1e-9, the bound of
     `test_teacher_forced_steps` (mu relative to max(1, max |mu - mean|), A_induced to max(1, max |A|)).
  B  the whole step with the configuration's tolerance 1e-3: the same number of screening iterations and the same dt
     as the oracle -- tests/test_screening_step_host.py shows that no decision of the oracle is near a tie at the steps
     used -- and the same quantities within `BOUND_B`, ten times the worst deviation measured on an MI355X and in no
     case above 1e-7.

Configurations: C1 the strip with terminals and a transport current (5 chunks, 7 edge blocks; steps of 304, 14, 1, 51
and 6 iterations); C2 the same from dt = 2: psi updates fail inside the screening loop and dt stays shrunk; C3 field
only, no terminals (3 chunks); C4 = C1 on the AMG-PCG solve with the projection guess; C5 = C1 under a field ramp
scaled on the device, so that dA/dt enters the right-hand side while A_induced moves (a fixed dt = 1e-5 and a ramp
over t = 1: the oracle converges in 19, 17, 4, 1, ... iterations and meets the margin conditions; with dt = 1e-3 it does
not converge); C7 = C2 with a retry budget that a step exceeds as a whole but no screening iteration does.  All but C4
run on the product's dense direct mu solve.

Measured on an MI355X (worst deviation over the steps of a configuration and all quantities; |psi|^2 leads each):
     A: C1 2.8e-12, C2 2.5e-12, C3 3.0e-12, C4 2.8e-12, C5 2.8e-12, C7 2.5e-12   (A_induced alone: <= 8.5e-15)
     B: C1 3.0e-12, C2 2.8e-12, C3 3.0e-12, C4 3.1e-12, C5 2.9e-12, C7 2.7e-12   (A_induced alone: <= 2.0e-14)
A step of 304 iterations deviates no more than one of a single iteration: the loop converges to a fixed point and
does not amplify.  The same run with a library in which k_polyak strides the chunks by m instead of m_pad, the
velocity is not zeroed per step, the update formula takes |psi|^2 of the current iterate, or the retry budget is not
restored per iteration fails 13, 12, 6 and 1 (C7) of the 14 tests.

C6: chunks of several tiles (`tiles_per_chunk` = 2 from about 12k sites on, where an oracle matrix no longer fits):
one iteration on a 12k-site mesh, A_induced compared with A0 + alpha (A_new - A0), A_new from
`evaluate_induced_vector_potential` of the currents the step left (the kernel that
`test_induced_vector_potential_kernel_matches_direct_sum` holds to a float64 direct sum; its host-side sum over the
chunks runs in k_polyak's order).  Expected bit-equal; seen on an MI355X: all 69776 entries equal (23 chunks of 2).

Not covered: the one-process-per-GPU form, the treecode inside the step, `tiles_per_chunk` > 1 against the oracle.
"""
import numpy as np
import pytest

import screening_step_model as M
from helpers import GAMMA_DEFAULT, U_DEFAULT, align_phase, max_abs, remove_mean, synthetic_mesh, uniform_field_A

pytestmark = pytest.mark.gpu

CASES = {"C1": "C1", "C2": "C2", "C3": "C3", "C4": "C1", "C5": "C5", "C7": "C7"}  # case -> configuration of the model
BOUND_A = 1e-9
BOUND_B = {"C1": 3.0e-11, "C2": 2.9e-11, "C3": 3.1e-11, "C4": 3.1e-11, "C5": 3.0e-11, "C7": 2.7e-11}


def _device_solver(case, p, tolerance, request, monkeypatch):
    from tdgl_amd import SolverOptions, TDGLSolver
    from tdgl_amd.hipcore import TDGLContext

    if case == "C4":  # no direct solve, no factor preconditioner: AMG-PCG (as tests/test_hip_vcycle_stored.py does)
        for attr, value in (("DENSE_MAX_SITES", 0), ("SUB_MAX_SITES", 0), ("SUB2_MAX_SITES", 0), ("PD_CHOICE", 2)):
            monkeypatch.setattr(TDGLContext, attr, value)
    else:
        request.getfixturevalue("direct_solve")
    o, s = p.options, p.screening
    opts = SolverOptions(solve_time=1e9, dt_init=o.dt_init, dt_max=o.dt_max, adaptive=o.adaptive, save_every=10**9,
                         max_solve_retries=o.max_solve_retries,
                         adaptive_time_step_multiplier=o.adaptive_time_step_multiplier, pcg_rtol=1e-12,
                         include_screening=True, screening_tolerance=tolerance,
                         max_iterations_per_step=s["max_iterations"], screening_step_size=s["step_size"],
                         screening_step_drag=s["step_drag"])
    A0 = p.A if p.field is None else p.field(0.0)
    solver = TDGLSolver.from_dimensionless(
        p.mesh, opts, A0, 1.0, U_DEFAULT, GAMMA_DEFAULT, terminal_info=p.terminals, current_func=p.current,
        screening=dict(sites=s["sites"], edge_centers=s["edge_centers"], areas=s["areas"]))
    ctx = solver.ctx
    if case == "C4":
        assert ctx.mu.form == "amg" and not ctx.dense_direct and not ctx.precond_direct
    else:
        assert ctx.mu.form == "dense" and ctx.dense_direct
    return solver


def _teacher_forced_step(solver, p, before, want):
    """One device step from the oracle's state ``before``; the deviations from the oracle's step ``want``."""
    ctx, o = solver.ctx, solver.options
    ctx.set_state(before["psi"], before["mu"])
    if p.scale is not None:  # A and dA/dt as the loop with one look per step leaves them before step k
        ctx.set_link_exponents_base(p.A, p.scale(before["time_prev"]))
        if before["time"] > before["time_prev"]:
            ctx.update_link_scale(p.scale(before["time"]), before["dt_prev"])
    ctx.set_induced_vector_potential(before["A_induced"])
    ctx.set_mu_boundary(want["mu_boundary"])
    td = before["tentative_dt"]
    ctx.set_controller(td, max(td, o.dt_max), o.adaptive, 10**6, o.max_solve_retries, o.adaptive_time_step_multiplier)
    ctx.begin_stage()
    res = ctx.run(1)
    got = ctx.get_state()
    A = ctx.induced_vector_potential()
    mu_scale = max(1.0, np.abs(remove_mean(want["mu"])).max())
    dev = {
        "|psi|^2": max_abs(np.abs(got["psi"]) ** 2, np.abs(want["psi"]) ** 2),
        "psi": max_abs(align_phase(got["psi"], want["psi"]), want["psi"]),
        "mu": max_abs(remove_mean(got["mu"]), remove_mean(want["mu"])) / mu_scale,
        "J_s": max_abs(got["supercurrent"], want["js"]),
        "J_n": max_abs(got["normal_current"], want["jn"]),
        "A_induced": max_abs(A, want["A_induced"]) / max(1.0, np.abs(want["A_induced"]).max()),
    }
    return res, dev


def _run_case(case, take, tolerance, bound, request, monkeypatch):
    p, rec, _ = M.record(CASES[case])
    solver = _device_solver(case, p, tolerance, request, monkeypatch)
    ctx = solver.ctx
    ctx.step_stats(reset=True)
    worst, counts, retries = {}, [], 0
    for k in p.steps:
        before, want = rec[k]["before"], rec[k][take]
        res, dev = _teacher_forced_step(solver, p, before, want)
        counts.append(int(res["screening_iterations"][0]))
        print(f"{case} {take} step {k}: iterations {counts[-1]} (oracle {want['iterations']}), dt {res['dt'][0]:.6g},"
              f" deviations " + ", ".join(f"{q} {v:.1e}" for q, v in dev.items()))
        assert counts[-1] == want["iterations"], (case, k)
        assert res["dt"][0] == want["dt"], (case, k)  # the same retry decisions from the same state
        failed = sum(a["failed"] for a in want["attempts"])
        stats = ctx.step_stats()
        assert stats["psi_retries"] - retries == failed, (case, k)
        retries = stats["psi_retries"]
        for q, v in dev.items():
            worst[q] = max(worst.get(q, 0.0), v)
            assert v < bound, (case, k, q, v)
    stats = ctx.step_stats()
    if case in ("C2", "C7"):
        assert stats["psi_retries"] > 0
    if case == "C4":  # PCG iterations were spent, from the projection guess (`extrapolate` = 3, the default)
        assert stats["pcg_iterations"] > 0
        if take == "whole":  # (a single iteration is the first solve after tdgl_set_state: nothing to project onto yet)
            assert ctx.guess_stats()["vectors"] > 0
    else:
        assert stats["pcg_iterations"] == 0
    print(f"{case} {take}: steps {list(p.steps)}, screening iterations {counts}, worst deviation"
          f" {max(worst.values()):.2e} (" + ", ".join(f"{q} {v:.1e}" for q, v in worst.items()) + ")")
    ctx.close()


@pytest.mark.parametrize("case", list(CASES))
def test_one_screening_iteration_entry_by_entry(case, request, monkeypatch):
    p, rec, _ = M.record(CASES[case])
    assert all(rec[k]["single"]["iterations"] == 1 for k in p.steps)  # ... on the oracle's side
    _run_case(case, "single", M.ONE_ITERATION, BOUND_A, request, monkeypatch)


@pytest.mark.parametrize("case", list(CASES))
def test_whole_screened_steps(case, request, monkeypatch):
    assert BOUND_B[case] <= 1e-7
    _run_case(case, "whole", M.TOLERANCE, BOUND_B[case], request, monkeypatch)


def test_induced_vector_potential_round_trip(request, monkeypatch):
    """`set_induced_vector_potential` then `induced_vector_potential`: the edge permutation there and back."""
    p = M.record("C1")[0]
    solver = _device_solver("C1", p, M.TOLERANCE, request, monkeypatch)
    ctx = solver.ctx
    rng = np.random.default_rng(11)
    A = rng.standard_normal((ctx.m, 2))
    ctx.set_induced_vector_potential(A)
    assert np.array_equal(ctx.induced_vector_potential(), A)
    ctx.close()


def test_chunks_of_several_tiles():
    """C6 (module docstring): k_polyak's sum over chunks of two tiles each, inside the step."""
    from tdgl_amd import SolverOptions, TDGLSolver

    mesh = synthetic_mesh(100)
    em = mesh.edge_mesh
    n, m = len(mesh.sites), len(em.edges)
    # set_screening_impl: tiles of 256 sites, at most max(1, 2048 / edge blocks) chunks
    tiles, eblocks = -(-n // 256), -(-m // 512)
    chunks = min(tiles, 64, max(1, 2048 // eblocks))
    tiles_per_chunk = -(-tiles // chunks)
    assert tiles_per_chunk == 2 and -(-tiles // tiles_per_chunk) > 20
    alpha, beta = 0.1, 0.5
    opts = SolverOptions(solve_time=1e9, dt_init=1e-3, dt_max=0.1, save_every=10**9, pcg_rtol=1e-11,
                         include_screening=True, screening_tolerance=M.ONE_ITERATION, max_iterations_per_step=400,
                         screening_step_size=alpha, screening_step_drag=beta)
    A_applied = uniform_field_A(mesh, 0.1)
    geometry = dict(sites=mesh.sites, edge_centers=em.centers, areas=0.01 * mesh.areas)
    solver = TDGLSolver.from_dimensionless(mesh, opts, A_applied, 1.0, U_DEFAULT, GAMMA_DEFAULT, screening=geometry)
    ctx = solver.ctx
    # a relaxed state: twenty steps of the device without screening
    ctx.set_screening(None, None, None)
    ctx.set_state(solver.psi_init, solver.mu_init)
    ctx.begin_stage()
    ctx.run(20)
    state = ctx.get_state()
    ctx.set_screening(geometry["sites"], geometry["edge_centers"], geometry["areas"], max_iterations=400,
                      tolerance=M.ONE_ITERATION, step_size=alpha, step_drag=beta)
    A0 = -0.05 * A_applied  # smooth, non-zero, of the induced field's sense
    ctx.set_state(state["psi"], state["mu"])
    ctx.set_induced_vector_potential(A0)
    ctx.begin_stage()
    res = ctx.run(1)
    assert res["screening_iterations"][0] == 1
    A = ctx.induced_vector_potential()
    # (the ledger of the currents is FORMED after a screened step -- `currents.screening_done()` --, so get_state returns
    # J_s and J_n as the last iteration formed and used them)
    got = ctx.get_state()
    A_new = ctx.evaluate_induced_vector_potential(got["supercurrent"] + got["normal_current"])
    want = A0 + alpha * (A_new - A0)
    excess = np.abs(A - want) - 4 * 2.0**-53 * (np.abs(A0) + np.abs(A_new))
    print(f"C6: {n} sites, {m} edges, {-(-tiles // tiles_per_chunk)} chunks of {tiles_per_chunk} tiles: max |A - want| ="
          f" {np.abs(A - want).max():.1e}, entries that differ: {int(np.count_nonzero(A != want))} of {A.size};"
          f" max |A_new - A0| = {np.abs(A_new - A0).max():.1e}")
    assert np.abs(A_new - A0).max() > 1e-3  # the update moved A_induced
    assert excess.max() <= 0.0
    ctx.close()
