"""The work queued behind the status copies of the iterative step (poisson.inc: sync_status with a shadow) changes
no result: the previous step's edge currents behind the first look of the mu solve, the guarded end of the solve
(k_finish_solution) behind the look that follows a batch of iterations.  Every case runs twice in fresh child
processes -- with the shadows and with `TDGL_NO_SYNC_SHADOW`, which restores the order without them -- and psi, mu,
J_s, J_n, the dt sequence, the PCG iteration counts and the probe read-outs are compared with `==`.

The children are this file run as a script: ``python tests/test_hip_sync_shadow.py CASE OUT.npz``."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mu solver of the child's contexts: the limits of the direct solves below every mesh, so that the iterative path with
# the projection guess runs -- on the V-cycle alone, or with the three-level factors as the CG's preconditioner
# (what the 1M-site benchmark step does; the class limits `bench.py --sub-limits` sets, parts of ~60 sites)
LIMITS = dict(
    vcycle=dict(DENSE_MAX_SITES=0, SUB_MAX_SITES=0, SUB2_MAX_SITES=0),
    factors=dict(DENSE_MAX_SITES=199, SUB_MAX_SITES=199, SUB2_MAX_SITES=199, SUB2_BLOCK=60, SUB2_SUPER=500,
                 SUB3_MIN_SITES=200, SUB3_BIG=3000, PD_MAX_SITES=10 ** 9, PD_CHOICE=1),
)
ENV_LIMITS = dict(TDGL_DENSE_MAX_SITES="0", TDGL_SUB_MAX_SITES="0", TDGL_SUB_BLOCK="0")


def _fields(out, tag, ctx):
    st = ctx.get_state()
    for key in ("psi", "mu", "supercurrent", "normal_current"):
        out[f"{tag}_{key}"] = st[key]


def _run(out, tag, ctx, steps):
    res = ctx.run(steps)
    out[f"{tag}_dt"] = res["dt"]
    out[f"{tag}_pcg_iters"] = res["pcg_iters"]
    if res["mu"] is not None:
        out[f"{tag}_probe_mu"] = res["mu"]
        out[f"{tag}_probe_theta"] = res["theta"]
    return res


def _solver(mesh, precond, opts_kw, field, **kw):
    from helpers import GAMMA_DEFAULT, U_DEFAULT, uniform_field_A
    from tdgl_amd import SolverOptions, TDGLSolver
    from tdgl_amd.hipcore import TDGLContext

    for name, value in LIMITS[precond].items():
        setattr(TDGLContext, name, value)
    opts = SolverOptions(solve_time=1e9, save_every=10 ** 6, **opts_kw)
    A = uniform_field_A(mesh, field)
    if "vector_potential_ramp" in kw:
        kw["vector_potential_ramp"] = (A, kw["vector_potential_ramp"])
        A = 0.0 * A
    solver = TDGLSolver.from_dimensionless(mesh, opts, A, 1.0, U_DEFAULT, GAMMA_DEFAULT, **kw)
    ctx = solver.ctx
    assert not ctx.dense_direct, "the iterative mu solve is what these cases are about"
    if precond == "factors":
        assert ctx.mu.form == "precond"
    ctx.set_state(solver.psi_init, solver.mu_init)
    ctx.begin_stage()
    solver.update_mu_boundary(0.0)
    return solver, ctx


def _stats(out, ctx):
    st = ctx.step_stats()
    for key in ("steps", "psi_retries", "pcg_iterations", "host_syncs", "edge_current_launches"):
        out[f"stat_{key}"] = np.int64(st[key])
    out["stat_extra_looks"] = np.int64(ctx.pcg_prediction_stats()["extra_looks"])


def case_square(out):
    """60 steps of a square film in a field, the factors preconditioning; the state read after run(1), run(7) and the
    rest: the owed currents are flushed at a return each time."""
    from helpers import synthetic_mesh

    _, ctx = _solver(synthetic_mesh(64, 64), "factors", dict(dt_init=1e-3, dt_max=0.1), 0.4)
    for tag, steps in (("a", 1), ("b", 7), ("c", 52)):
        _run(out, tag, ctx, steps)
        _fields(out, tag, ctx)
    _stats(out, ctx)


def case_retries(out):
    """dt_init far too large: psi retries re-enter the solve for the same step."""
    mesh, kw = _strip()
    _, ctx = _solver(mesh, "vcycle", dict(dt_init=0.5, dt_max=2.0, max_solve_retries=12), 0.25, **kw)
    _run(out, "a", ctx, 40)
    _fields(out, "a", ctx)
    _stats(out, ctx)


def case_holds_back(out):
    """Solves that do not converge in their first batch: the host looks after every V-cycle iteration (check_every=1),
    a window of one vector from a cold start.  The guarded finish holds back at every look but the last; the next 10
    steps' iteration counts show that the window holds the same vectors."""
    from helpers import synthetic_mesh

    _, ctx = _solver(synthetic_mesh(64, 64), "vcycle", dict(dt_init=1e-3, dt_max=0.1), 0.4)
    ctx.set_poisson_options(rtol=1e-10, check_every=1, guess_window=1)
    _run(out, "a", ctx, 30)
    _fields(out, "a", ctx)
    _run(out, "b", ctx, 10)
    _fields(out, "b", ctx)
    _stats(out, ctx)


def _strip():
    from helpers import edge_terminal, synthetic_mesh

    mesh = synthetic_mesh(120, 30)
    terms = [edge_terminal(mesh, "source", -60.0), edge_terminal(mesh, "drain", 60.0)]
    probes = [mesh.closest_site((-25, 0)), mesh.closest_site((25, 0))]
    return mesh, dict(terminal_info=terms, current_func={"source": 9.0, "drain": -9.0}, probe_points=probes)


def case_strip(out):
    """A strip with terminals and two probes, the factors preconditioning."""
    mesh, kw = _strip()
    _, ctx = _solver(mesh, "factors", dict(dt_init=1e-3, dt_max=0.1), 0.2, **kw)
    _run(out, "a", ctx, 40)
    _fields(out, "a", ctx)
    _stats(out, ctx)


def case_ramp(out):
    """Fall-back: a field ramp (the links change at step begin) keeps the old order."""
    from helpers import synthetic_mesh

    _, ctx = _solver(synthetic_mesh(64, 64), "vcycle", dict(dt_init=1e-3, dt_max=0.1), 0.6,
                     vector_potential_ramp=dict(tmin=0.0, tmax=3.0, initial=0.0, final=1.0))
    ctx.step_stats(reset=True)
    _run(out, "a", ctx, 40)
    _stats(out, ctx)
    _fields(out, "a", ctx)


def case_extrapolate(out):
    """Fall-back: an extrapolated guess (k_extrapolate writes mu before the first look) keeps the old order."""
    from helpers import synthetic_mesh

    _, ctx = _solver(synthetic_mesh(64, 64), "vcycle", dict(dt_init=1e-3, dt_max=0.1), 0.4)
    ctx.set_poisson_options(rtol=1e-10, extrapolate=1)
    ctx.step_stats(reset=True)
    _run(out, "a", ctx, 40)
    _stats(out, ctx)
    _fields(out, "a", ctx)


def case_set_state(out):
    """set_state between two runs, and the currents read directly after set_state."""
    mesh, kw = _strip()
    solver, ctx = _solver(mesh, "vcycle", dict(dt_init=1e-3, dt_max=0.1), 0.2, **kw)
    _run(out, "a", ctx, 12)
    st = ctx.get_state()
    rng = np.random.default_rng(5)
    psi = st["psi"] * (1.0 + 0.01 * rng.standard_normal(ctx.n))
    psi[solver.fixed_sites] = 0.0
    ctx.set_state(psi, 0.5 * st["mu"])
    _fields(out, "set", ctx)  # (supercurrent=True: formed on request from the state just set)
    _run(out, "b", ctx, 12)
    _fields(out, "b", ctx)
    _stats(out, ctx)


CASES = dict(square=case_square, retries=case_retries, holds_back=case_holds_back, strip=case_strip, ramp=case_ramp,
             extrapolate=case_extrapolate, set_state=case_set_state)


def _children(case, tmp_path):
    """Both runs of a case, side by side in fresh processes: (with the shadows, reference with the switch set)."""
    procs, paths = [], []
    for switch in (False, True):
        env = {k: v for k, v in os.environ.items() if k != "TDGL_NO_SYNC_SHADOW"}
        env.update(ENV_LIMITS)
        if switch:
            env["TDGL_NO_SYNC_SHADOW"] = "1"
        paths.append(str(tmp_path / f"{case}_{int(switch)}.npz"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), case, paths[-1]], cwd=ROOT, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, text in zip(procs, outs):
        assert p.returncode == 0, text[-4000:]
    loaded = []
    for path in paths:
        with np.load(path) as f:
            loaded.append({k: f[k] for k in f.files})
    return loaded


def _assert_equal(new, ref):
    assert sorted(new) == sorted(ref)
    for key in ref:
        assert new[key].shape == ref[key].shape and np.array_equal(new[key], ref[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_sync_shadow_changes_no_result(case, tmp_path):
    new, ref = _children(case, tmp_path)
    # what the case is there for, asserted on the reference side
    assert np.all(np.isfinite(ref["a_dt"])) and ref["stat_steps"] > 0
    if case == "square":
        assert ref["stat_steps"] == 60 and ref["stat_edge_current_launches"] == 60 and np.abs(ref["c_supercurrent"]).max() > 0
    elif case == "retries":
        assert ref["stat_psi_retries"] >= 3
    elif case == "holds_back":
        assert np.count_nonzero(ref["a_pcg_iters"] >= 2) >= 5 and ref["stat_extra_looks"] >= 5
        assert np.array_equal(new["b_pcg_iters"], ref["b_pcg_iters"])
    elif case == "strip":
        assert ref["a_probe_mu"].shape == (40, 2) and np.abs(ref["a_probe_mu"]).max() > 0
    elif case in ("ramp", "extrapolate"):
        for side in (new, ref):
            assert side["stat_edge_current_launches"] == side["stat_steps"] == 40
    elif case == "set_state":
        assert np.abs(ref["set_supercurrent"]).max() > 0
    _assert_equal(new, ref)


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "py-tdgl_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    results = {}
    CASES[sys.argv[1]](results)
    np.savez(sys.argv[2], **results)
