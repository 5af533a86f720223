"""The factor preconditioner's folded application against the two-pass order it replaces.

By default the first level's way down reads the residual through the dissection's map and its way up stores z through
it (`k_sub_down_sym` / `k_sub_down_lanes` / `k_sub_up` in their mapped form), and r . z is formed by `k_sell_axp` on the
first iteration of a run, by `k_dot_partial` on a later one.  `TDGL_PD_TWO_PASS`, read when the context is created,
restores `k_pd_gather`, the sequence on vectors in the dissection's order, `k_pd_scatter`.  The sweeps do the same
arithmetic on the same values in the same order either way, so z of one application is the same BIT FOR BIT; r . z
changes its summation order, and with it the CG's alpha in the last bits.

Every test builds both contexts on a prescribed layout (tests/prescribed_dissection.py: parts on both sides of every
size the kernels branch on).  The single-GPU preconditioner is always cut to three levels (`TDGLContext.mu_plan`), so
the time loop of test 3 runs on the three-level `mixed` layout: a two-level preconditioner cannot be built."""

import functools

import numpy as np
import pytest

import dense_reference as D
import prescribed_dissection as P
from helpers import uniform_field_A

pytestmark = pytest.mark.gpu

PARITY_TOL = 1e-8  # (bench.py's)
SETTINGS = (("DENSE_MAX_SITES", 199), ("SUB_MAX_SITES", 199), ("SUB2_MAX_SITES", 199), ("SUB3_MIN_SITES", 200),
            ("SUB3_BIG", 6000), ("PD_MAX_SITES", 10 ** 9), ("PD_CHOICE", 1))


@functools.lru_cache(maxsize=None)
def _layout(name):
    return P.build_layout(name, 3)


@functools.lru_cache(maxsize=None)
def _kappa(lx):
    from helpers import synthetic_mesh

    A = D.poisson_matrix_of(synthetic_mesh(lx))
    return D.condition_number(A, D.pinv_reference(A))


def teardown_module(module):
    for f in (_layout, _kappa):
        f.cache_clear()


def _settings(name, monkeypatch, sym, two_pass):
    """The factors as preconditioner on every solve, at the prescribed part sizes (what `_precond_ctx` of
    tests/test_hip_sub_prescribed.py sets), and the order of the application."""
    from tdgl_amd import substructure
    from tdgl_amd.hipcore import TDGLContext

    lay = _layout(name)
    for attr, value in SETTINGS:
        monkeypatch.setattr(TDGLContext, attr, value)
    monkeypatch.setenv("TDGL_PD_BLR", "0")
    if sym:
        monkeypatch.setenv("TDGL_PD_SYM", "2")
    else:
        monkeypatch.delenv("TDGL_PD_SYM", raising=False)
    monkeypatch.delenv("TDGL_UP_PARTS", raising=False)
    if two_pass:
        monkeypatch.setenv("TDGL_PD_TWO_PASS", "1")
    else:
        monkeypatch.delenv("TDGL_PD_TWO_PASS", raising=False)
    for k, fn in enumerate(("substructure_order", "substructure_order2", "substructure_order3")):
        monkeypatch.setattr(substructure, fn, P.order_function(lay.lists[:k + 1]))
    return lay


def _ctx(name, monkeypatch, sym, two_pass, rtol=1e-10):
    from tdgl_amd.hipcore import TDGLContext

    lay = _settings(name, monkeypatch, sym, two_pass)
    ctx = TDGLContext(lay.mesh)
    ctx.build_poisson(rtol=rtol)
    assert ctx.precond_direct and not ctx.dense_direct, ctx.setup_times
    assert np.array_equal(ctx._pd_order[0], lay.perm)
    return ctx, lay


def _both(name, monkeypatch, sym, rtol=1e-10):
    folded, lay = _ctx(name, monkeypatch, sym, False, rtol)
    try:
        two_pass, _ = _ctx(name, monkeypatch, sym, True, rtol)
    except BaseException:
        folded.close()
        raise
    return folded, two_pass, lay


def _took(ctx):
    """'folded' / 'two_pass': the order EVERY application of the context took so far (at least one)."""
    st = ctx.precond_apply_stats()
    assert st["folded"] + st["two_pass"] > 0 and min(st["folded"], st["two_pass"]) == 0, st
    return "folded" if st["folded"] else "two_pass"


SYM = {"mixed": False, "tiles256": True, "tiles64": True, "lanes2048": False}


@pytest.mark.parametrize("name", ["mixed", "tiles256", "tiles64", "lanes2048"])
def test_one_application_is_the_two_pass_one_bit_for_bit(name, monkeypatch):
    """The layout's probe columns and four seeded random vectors: z identical, r . z of both within n u sum |r z| of r @ z."""
    folded, two_pass, lay = _both(name, monkeypatch, SYM[name])
    try:
        assert folded.precond_direct_layout() == two_pass.precond_direct_layout()
        assert (folded.precond_direct_layout()[0] > 0) == SYM[name]
        B = P.probe_columns(lay.ptrs, lay.n)[lay.iperm]  # (site order: r[perm[i]] = B[i])
        B = np.column_stack([B, np.random.default_rng(20).standard_normal((lay.n, 4))])
        worst = 0.0
        for j in range(B.shape[1]):
            r = np.ascontiguousarray(B[:, j])
            z_f, rz_f = folded.precond_apply(r)
            z_t, rz_t = two_pass.precond_apply(r)
            assert np.array_equal(z_f, z_t), (j, np.abs(z_f - z_t).max(), np.abs(z_t).max())
            bound = lay.n * D.U * np.abs(r * z_t).sum()
            for rz in (rz_f, rz_t):
                worst = max(worst, abs(rz - r @ z_t) / bound)
                assert abs(rz - r @ z_t) <= bound, (j, rz, r @ z_t)
        print(f"{name}: {B.shape[1]} columns, z identical; largest |rz - r @ z| / (n u sum |r z|) = {worst:.3g}")
        assert _took(folded) == "folded" and _took(two_pass) == "two_pass"
    finally:
        folded.close()
        two_pass.close()


@pytest.mark.parametrize("name", ["mixed", "tiles256"])
def test_two_iterations_with_the_factors(name, monkeypatch):
    """rtol 1e-10 from a zero guess: fp32-stored factors need a second application, whose r . z comes from
    `k_dot_partial` on the folded path.  The same iteration count, both converged, the solutions within the suite's
    floor C_TOL kappa u of each other."""
    rtol = 1e-10
    folded, two_pass, lay = _both(name, monkeypatch, SYM[name], rtol)
    try:
        rhs = np.random.default_rng(21).standard_normal(lay.n)
        out = {}
        for key, ctx in (("folded", folded), ("two_pass", two_pass)):
            ctx.precond_direct_stats(reset=True)
            out[key] = ctx.poisson_solve(rhs)
            st = ctx.precond_direct_stats()
            assert st["solves_factors"] == 1 and st["solves_vcycle"] == 0 and st["handovers"] == 0, (key, st)
            assert _took(ctx) == key
        (x_f, it_f, rel_f), (x_t, it_t, rel_t) = out["folded"], out["two_pass"]
        kappa = _kappa(P.LAYOUTS[name][0])
        diff = np.abs(x_f - x_t).max() / np.abs(x_t).max()
        print(f"{name}: iterations {it_f} / {it_t}, relres {rel_f:.3g} / {rel_t:.3g}, max |x_f - x_t| / max |x| = {diff:.3g} "
              f"(floor {D.C_TOL * kappa * D.U:.3g})")
        assert it_f >= 2 and it_t >= 2  # (the test's own precondition)
        assert it_f == it_t
        assert rel_f <= rtol and rel_t <= rtol
        assert diff <= D.C_TOL * kappa * D.U
    finally:
        folded.close()
        two_pass.close()


def test_twenty_steps_of_the_time_loop(monkeypatch):
    """20 steps of the classic loop with the factors on every solve: the same accepted steps and retries, dt and the
    fields of the two paths within bench.py's PARITY_TOL (normalised as its parity_block does)."""
    from tdgl_amd import SolverOptions, TDGLSolver

    runs = {}
    for key in ("folded", "two_pass"):
        lay = _settings("mixed", monkeypatch, False, key == "two_pass")
        s = TDGLSolver.from_dimensionless(lay.mesh, SolverOptions(solve_time=1e9, dt_init=1e-4, save_every=10 ** 9),
                                          uniform_field_A(lay.mesh, 0.3), 1.0)
        ctx = s.ctx
        try:
            assert ctx.precond_direct and not ctx.dense_direct and np.array_equal(ctx._pd_order[0], lay.perm), ctx.setup_times
            ctx.set_state(s.psi_init, s.mu_init)
            ctx.begin_stage()
            ctx.step_stats(reset=True)
            ctx.precond_direct_stats(reset=True)
            res = ctx.run(20)
            pd = ctx.precond_direct_stats()
            assert pd["solves_factors"] >= 20 and pd["solves_vcycle"] == 0, pd
            assert _took(ctx) == key
            runs[key] = (np.array(res["dt"], dtype=float), ctx.get_state(), ctx.step_stats())
        finally:
            ctx.close()
    (dt_f, st_f, n_f), (dt_t, st_t, n_t) = runs["folded"], runs["two_pass"]
    assert len(dt_f) == len(dt_t) == 20
    assert (n_f["steps"], n_f["psi_retries"]) == (n_t["steps"], n_t["psi_retries"]), (n_f, n_t)

    def dev(a, b):
        return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))

    got = dict(dt=float(np.max(np.abs(dt_f - dt_t)) / np.max(dt_t)),
               abs_sq_psi=dev(np.abs(st_f["psi"]) ** 2, np.abs(st_t["psi"]) ** 2),
               mu_zero_mean=dev(st_f["mu"] - st_f["mu"].mean(), st_t["mu"] - st_t["mu"].mean()),
               J_s=dev(st_f["supercurrent"], st_t["supercurrent"]),
               J_n=dev(st_f["normal_current"], st_t["normal_current"]))
    print("folded against two-pass after 20 steps:", got, "steps / retries", n_f["steps"], n_f["psi_retries"])
    assert all(v <= PARITY_TOL for v in got.values()), got


def test_the_switch_is_honoured(monkeypatch):
    """`precond_apply_stats` counts the applications by the order they took: the set-up's (calibration and check) and every
    later one go to the counter the switch selects, the other one stays at zero."""
    folded, two_pass, lay = _both("tiles64", monkeypatch, True)
    try:
        r = np.random.default_rng(22).standard_normal(lay.n)
        for ctx, mine, other in ((folded, "folded", "two_pass"), (two_pass, "two_pass", "folded")):
            before = ctx.precond_apply_stats()
            assert before[mine] > 0 and before[other] == 0, before
            ctx.precond_apply(r)
            after = ctx.precond_apply_stats()
            assert after[mine] == before[mine] + 1 and after[other] == 0, (before, after)
            _, iters, _ = ctx.poisson_solve(r)
            assert iters >= 1
            last = ctx.precond_apply_stats()
            # (a batch may launch more iterations than the solve then reports as needed)
            assert last[mine] >= after[mine] + iters and last[other] == 0, (after, last, iters)
    finally:
        folded.close()
        two_pass.close()
