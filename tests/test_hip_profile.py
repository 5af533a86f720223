"""The in-run timers (`profile_enable`, `profile_read`, `profile_read_pcg`, `profile_read_direct`): which launches of
`run` each of the three read-outs counts, in the loop with one synchronisation per step and in the run-ahead loop, and
what enabling, re-enabling, disabling and reading twice do to the counters.  Only the counts are pinned -- the times
are the device's business; they are positive where a pair was recorded and zero where none was.

What each read-out counts, on one GPU (csrc/tdgl_internal.h: Profile):
  profile_read         K1 (L psi' and the right-hand side): every attempt of the classic loop, once per run-ahead batch;
  profile_read_pcg     the CG's fused A p: every 8th launch since `profile_enable`, 64 samples at most -- with `queued`
                       iterations launched (`pcg_prediction_stats`, one A p each) that is min(64, ceil(queued / 8));
  profile_read_direct  the direct solve's launch sequence once per run-ahead batch (as often as K1 there), or every
                       application of the factors as the CG's preconditioner (one per iteration) up to 64: min(64, queued).
A fresh context's run-ahead loop queues batches of 4, 8, 16, ... attempts: 24 steps that all succeed are batches of
4, 8 and the remaining 12."""

import numpy as np
import pytest

from conftest import load_golden
from helpers import GAMMA_DEFAULT, U_DEFAULT, reference_mesh, uniform_field_A

pytestmark = pytest.mark.gpu

STEPS = 24
DT = 1e-3
ZERO = ((0, 0.0), (0, 0.0), (0, 0.0))


def _context(steps_rtol=1e-10):
    """mesh_small in a field, fixed dt, a state set and a stage begun; the mu solver is whatever the class limits say."""
    from tdgl_amd import SolverOptions, TDGLSolver

    mesh = reference_mesh(load_golden("mesh_small"))
    opts = SolverOptions(solve_time=1e9, dt_init=DT, dt_max=DT, adaptive=False, save_every=10 ** 9, pcg_rtol=steps_rtol)
    solver = TDGLSolver.from_dimensionless(mesh, opts, uniform_field_A(mesh, 0.4), 1.0, U_DEFAULT, GAMMA_DEFAULT)
    ctx = solver.ctx
    ctx.set_state(solver.psi_init, solver.mu_init)
    ctx.begin_stage()
    solver.update_mu_boundary(0.0)
    return ctx


def _read(ctx):
    return ctx.profile_read(), ctx.profile_read_pcg(), ctx.profile_read_direct()


def _run(ctx, steps=STEPS):
    """`steps` steps of the fixed dt, none of them repeated; returns the iterations launched meanwhile."""
    before = ctx.pcg_prediction_stats()["queued"]
    ctx.step_stats(reset=True)
    res = ctx.run(steps)
    st = ctx.step_stats()
    assert len(res["dt"]) == steps and np.all(res["dt"] == DT)
    assert st["steps"] == steps and st["psi_retries"] == 0
    return ctx.pcg_prediction_stats()["queued"] - before


def test_classic_loop_with_the_iterative_solve(monkeypatch):
    monkeypatch.setenv("TDGL_NO_RUN_AHEAD", "1")  # (read when the context is created)
    ctx = _context()
    try:
        assert not ctx.dense_direct
        assert _read(ctx) == ZERO  # nothing is timed before it is asked for
        _run(ctx, 3)
        assert _read(ctx) == ZERO
        ctx.profile_enable(True)
        queued = _run(ctx)
        st = ctx.step_stats()
        (k1, k1_ms), (axp, axp_ms), direct = first = _read(ctx)
        print(f"classic, AMG-PCG: K1 {k1} launches {k1_ms:.3f} ms; A p {axp} samples of {queued} launches {axp_ms:.3f} ms; direct {direct}")
        assert k1 == st["steps"] + st["psi_retries"] == STEPS and k1_ms > 0.0
        assert queued >= 1 and 1 <= axp <= 64 and axp == min(64, -(-queued // 8)) and axp_ms > 0.0
        assert direct == (0, 0.0)
        assert _read(ctx) == first  # a second read finds nothing new
        # enabled again: every counter starts over, and so does the count to every 8th launch
        ctx.profile_enable(True)
        assert _read(ctx) == ZERO
        queued = _run(ctx, 5)
        (k1, _), (axp, _), direct = _read(ctx)
        assert k1 == 5 and axp == min(64, -(-queued // 8)) and direct == (0, 0.0)
        # disabled: zero, and it stays there
        ctx.profile_enable(False)
        assert _read(ctx) == ZERO
        _run(ctx, 5)
        assert _read(ctx) == ZERO
    finally:
        ctx.close()


def test_run_ahead_loop_with_the_dense_inverse(monkeypatch, direct_solve):
    monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    ctx = _context()
    try:
        assert ctx.dense_direct
        ctx.profile_enable(True)
        queued = _run(ctx)
        (k1, k1_ms), axp, (solves, solves_ms) = first = _read(ctx)
        print(f"run-ahead, dense inverse: K1 {k1} launches {k1_ms:.3f} ms; direct {solves} solves {solves_ms:.3f} ms; A p {axp}")
        assert queued == 0 and axp == (0, 0.0)
        assert k1 == solves and 1 <= k1 <= STEPS and k1_ms > 0.0 and solves_ms > 0.0
        assert k1 == 3  # batches of 4, 8 and 12 attempts: one pair each
        assert _read(ctx) == first
        ctx.profile_enable(True)
        assert _read(ctx) == ZERO
        ctx.profile_enable(False)
        _run(ctx)
        assert _read(ctx) == ZERO
    finally:
        ctx.close()


def test_factors_as_the_preconditioner_are_timed_64_times(monkeypatch):
    """The three-level factors precondition the CG from 200 sites up (the class limits of the `precond_direct_solve`
    fixture): one application per iteration, the first 64 of them timed."""
    from tdgl_amd.hipcore import TDGLContext

    monkeypatch.setenv("TDGL_NO_RUN_AHEAD", "1")
    for name, value in dict(DENSE_MAX_SITES=199, SUB_MAX_SITES=199, SUB2_MAX_SITES=199, SUB2_BLOCK=60, SUB2_SUPER=500,
                            SUB3_MIN_SITES=200, SUB3_BIG=3000, PD_MAX_SITES=10 ** 9, PD_CHOICE=1).items():
        monkeypatch.setattr(TDGLContext, name, value)
    ctx = _context(steps_rtol=1e-13)
    try:
        if ctx.dense_direct or ctx.mu.form != "precond":
            pytest.skip(f"mesh_small does not take the factors as the preconditioner (mu solve: {ctx.mu.form})")
        ctx.profile_enable(True)
        queued = _run(ctx, 8)
        (k1, _), (axp, _), (applied, applied_ms) = _read(ctx)
        print(f"factors preconditioning: {queued} iterations in 8 steps; K1 {k1}, A p {axp} samples, {applied} applications {applied_ms:.3f} ms")
        assert k1 == 8 and axp == min(64, -(-queued // 8))
        assert applied == min(64, queued) and (applied_ms > 0.0) == (applied > 0)
        queued += _run(ctx, 120)
        (k1, _), (axp, _), (applied, applied_ms) = first = _read(ctx)
        print(f"... {queued} iterations in 128 steps; K1 {k1}, A p {axp} samples, {applied} applications {applied_ms:.3f} ms")
        assert queued > 64, "the case needs more than 64 applications"
        assert k1 == 128 and axp == min(64, -(-queued // 8)) and applied == 64 and applied_ms > 0.0
        assert _read(ctx) == first
    finally:
        ctx.close()
