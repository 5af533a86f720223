"""Every time loop when the psi update fails at a SINGLE site (tests/local_failure.py).

`psi_update_body` reports one failure flag and one max d|psi|^2 per workgroup of 256 rows.  Their readers --
`reduce_psi_status` in `k_publish_status`, `k_status_pack`, `dense_finish_tail` and `k_ens_sub_control`; the
mu-writing guards of `dense_sym_finish_body`, `k_blr_finish`, `k_sub_up`, `k_ens_finish` and `k_ens_sub_up` -- and the
host paths around them (the roll-backs of mu, the L psi cache, the currents ledger, the run-ahead controller) are run
here with exactly one failing site, placed through `ctx.perm` in workgroup 0, a middle one and the last, partially
filled one at its last valid lane.  A reader that looks at the first entries only, at the wrong replica's row or at a
stale entry overwrites mu^n with the solve for the rejected psi' (a wrong phase factor in the retry) or feeds the
adaptive-dt controller a wrong maximum.

Reference: `OracleSolver` (three steps from a random state; `local_failure.oracle_steps` asserts that every failing
attempt fails at the spiked site alone, that no discriminant is within 1 of zero and that the largest d|psi|^2 sits at
the spiked site).  Tolerances: dt and the retry count exactly; |psi|^2, phase-aligned psi, mean-free mu, J_s, J_n
within 1e-9 (the expressions of `test_teacher_forced_steps`); the controller's last three history entries within
1e-11 max(1, value) -- the oracle's own fp64 value of that entry is within 3e-15 of an `np.longdouble` evaluation of
the same formula (tests/test_local_failure_host.py), so nothing wider is needed.
"""

import os
import sys

import numpy as np
import pytest

import local_failure as LF
from conftest import ROOT
from helpers import GAMMA_DEFAULT, U_DEFAULT, align_phase, max_abs, remove_mean, uniform_field_A

pytestmark = pytest.mark.gpu

POSITIONS = ("first", "middle", "last")


# ------------------------------------------------------------------ plumbing
def _solver(mesh, iterative=False, retries=10):
    from tdgl_amd import SolverOptions, TDGLSolver

    opts = SolverOptions(solve_time=1e9, dt_init=LF.DT_INIT, dt_max=0.1, save_every=10**9, pcg_rtol=1e-12,
                         max_solve_retries=retries, adaptive_time_step_multiplier=LF.MULTIPLIER,
                         **(dict(sparse_solver="amg_pcg") if iterative else {}))
    return TDGLSolver.from_dimensionless(mesh, opts, uniform_field_A(mesh, LF.FIELD), 1.0, U_DEFAULT, GAMMA_DEFAULT)


def _sites(ctx):
    """The three spiked sites of this context: ``{position: (workgroup, site)}``; the CPU test checked the same ones
    (`LF.host_order`)."""
    sites = LF.spike_sites(ctx.perm, ctx._sub_ptrs)
    nw = LF.workgroups(ctx)
    assert sites["first"][1] == LF.site_in_workgroup(ctx, 0, 0)
    assert sites["middle"][1] == LF.site_in_workgroup(ctx, nw // 2, 0)
    assert sites["last"][1] == LF.site_in_workgroup(ctx, -1, None) and sites["last"][0] == nw - 1
    return sites


def _begin(ctx, problem, spiked=True, retries=10):
    o = problem["options"]
    ctx.set_epsilon(problem["epsilon"] if spiked else 1.0)
    ctx.set_state(problem["psi0"], problem["mu0"])
    ctx.set_controller(o.dt_init, o.dt_max, True, o.adaptive_window, retries, o.adaptive_time_step_multiplier)
    ctx.begin_stage()
    ctx.step_stats(reset=True)


def _field_deviation(got, want):
    """The expressions of test_hip_parity.py::test_teacher_forced_steps."""
    return max(
        max_abs(np.abs(got["psi"]) ** 2, np.abs(want["psi"]) ** 2),
        max_abs(align_phase(got["psi"], want["psi"]), want["psi"]),
        max_abs(remove_mean(got["mu"]), remove_mean(want["mu"])) / max(1.0, np.abs(remove_mean(want["mu"])).max()),
        max_abs(got["supercurrent"], want["js"]),
        max_abs(got["normal_current"], want["jn"]),
    )


def _run_steps(ctx, problem, want, label, warm=0, n_steps=LF.N_STEPS):
    """``warm`` spike-free steps, then the spiked ones; every assertion of a time-loop case.  Returns what the
    bit-for-bit comparisons between two loops need."""
    _begin(ctx, problem, spiked=not warm)
    if warm:
        first = ctx.run(warm)
        assert np.array_equal(first["dt"], [s["dt"] for s in want["warm"]]) and ctx.step_stats()["psi_retries"] == 0
        ctx.set_epsilon(problem["epsilon"])
        ctx.step_stats(reset=True)
    res = ctx.run(n_steps)
    got = ctx.get_state()
    retries = ctx.step_stats()["psi_retries"]
    hist = ctx.controller_state()["history"]
    dev = _field_deviation(got, want["steps"][-1])
    want_dmax = np.array([s["dmax"] for s in want["steps"]])
    dmax_dev = float(np.max(np.abs(hist[-n_steps:] - want_dmax) / np.maximum(1.0, want_dmax))) if len(hist) >= n_steps else np.inf
    print(f"{label}: site {problem['site']}, retries {retries} (oracle {want['retries']}), dt {res['dt']}, "
          f"worst field deviation {dev:.2e}, dmax deviation {dmax_dev:.2e}")
    assert np.array_equal(res["dt"], want["dts"]), (label, res["dt"], want["dts"])
    assert retries == want["retries"], (label, retries, want["retries"])
    assert dev < 1e-9, (label, dev)
    assert len(hist) == warm + n_steps and dmax_dev <= 1e-11, (label, hist, want_dmax)
    return dict(dt=res["dt"], psi=got["psi"], mu=got["mu"])


def _all_positions(ctx, mesh, label, warm=0, positions=POSITIONS, n_steps=LF.N_STEPS, eps=LF.EPS_ONE_RETRY):
    out = {}
    for pos, (w, site) in _sites(ctx).items():
        if pos not in positions:
            continue
        problem = LF.spiked_problem(mesh, site, eps)
        want = LF.oracle_steps(problem, n_steps=n_steps, warm_steps=warm)
        assert want["retries"] >= n_steps  # (every spiked step retries at least once)
        out[pos] = _run_steps(ctx, problem, want, f"{label}, workgroup {w} of {LF.workgroups(ctx)} ({pos})", warm, n_steps)
    return out


def _both_loops(monkeypatch, mesh, label, check=None, **kw):
    """A direct-solve case in the run-ahead and in the classic loop: each against the oracle, and bit for bit against
    each other in dt, psi and mu."""
    out = {}
    for loop in ("run_ahead", "classic"):
        if loop == "classic":
            monkeypatch.setenv("TDGL_NO_RUN_AHEAD", "1")
        else:
            monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
        ctx = _solver(mesh).ctx
        try:
            assert ctx.dense_direct
            if check is not None:
                check(ctx)
            out[loop] = _all_positions(ctx, mesh, f"{label} [{loop}]", **kw)
            syncs = ctx.step_stats()["host_syncs"]
        finally:
            ctx.close()
        out[loop + "_syncs"] = syncs
    for pos, ra in out["run_ahead"].items():
        for key in ("dt", "psi", "mu"):
            assert np.array_equal(ra[key], out["classic"][pos][key]), (label, pos, key)
    return out


# ------------------------------------------------------------------ (a) the single call
@pytest.mark.parametrize("mesh_of", [LF.mesh_small, LF.mesh_17_workgroups], ids=["1452", "4099"])
def test_single_psi_update_call(mesh_of):
    """`ctx.psi_update` (k_psi_update + k_publish_status): None exactly when the oracle's psi_update is None, for
    dt = 1e-3 (fails at the spiked site) and dt / 4 (succeeds); psi' and |psi'|^2 within 5e-12 (the tolerance of
    test_psi_update_matches_reference_including_failures), at the spiked site within 5e-12 max(1, |psi'_s|^2)."""
    from oracle import psi_update
    from tdgl_amd.hipcore import TDGLContext

    mesh = mesh_of()
    ctx = TDGLContext(mesh, u=U_DEFAULT, gamma=GAMMA_DEFAULT)
    try:
        for pos, (w, site) in _sites(ctx).items():
            problem = LF.spiked_problem(mesh, site, LF.EPS_ONE_RETRY)
            lap = LF.oracle_solver(problem).operators.psi_laplacian
            ctx.set_link_exponents(problem["A"])
            ctx.set_epsilon(problem["epsilon"])
            psi, mu = problem["psi0"], problem["mu0"]
            outcomes = []
            for dt in (LF.DT_INIT, LF.DT_INIT * LF.MULTIPLIER):
                want = psi_update(psi, np.abs(psi) ** 2, mu, problem["epsilon"], GAMMA_DEFAULT, U_DEFAULT, dt, lap)
                got = ctx.psi_update(psi, mu, dt)
                outcomes.append(want is None)
                assert (got is None) == (want is None), (pos, dt)
                if got is None:
                    continue
                rest = np.arange(len(psi)) != site
                scale = max(1.0, float(want[1][site]))
                at_site = max(abs(got[0][site] - want[0][site]), abs(got[1][site] - want[1][site]))
                print(f"single call, n = {len(psi)}, workgroup {w} ({pos}), site {site}, dt {dt:g}: |psi'_s|^2 = "
                      f"{want[1][site]:.4g}, deviation there {at_site:.2e}, elsewhere "
                      f"{max(max_abs(got[0][rest], want[0][rest]), max_abs(got[1][rest], want[1][rest])):.2e}")
                assert max_abs(got[0][rest], want[0][rest]) < 5e-12 and max_abs(got[1][rest], want[1][rest]) < 5e-12
                assert at_site < 5e-12 * scale, (pos, at_site, scale)
            assert outcomes == [True, False]
    finally:
        ctx.close()


# ------------------------------------------------------------------ (b) classic loop, iterative solve
@pytest.mark.parametrize("extrapolate", [3, 1, 2])
def test_classic_loop_with_the_iterative_solve(extrapolate):
    """AMG-PCG with the projection guess (3: rolled back through `guess.newest_x()` or the copy made before the first
    solve) and with the extrapolated guesses (1, 2: `mu_prev`, `k_extrapolate`), the latter after two spike-free
    accepted steps so that the history exists."""
    mesh = LF.mesh_small()
    ctx = _solver(mesh, iterative=True).ctx
    try:
        assert not ctx.dense_direct
        o = ctx.poisson_options
        ctx.set_poisson_options(rtol=o["rtol"], max_iter=o["max_iter"], nu=o["nu"], check_every=o["check_every"],
                                smoother=o["smoother"], cheb_lo=o["cheb_lo"], nu_fine=o["nu_fine"], extrapolate=extrapolate)
        _all_positions(ctx, mesh, f"AMG-PCG, extrapolate {extrapolate}", warm=0 if extrapolate == 3 else 2)
        assert ctx.step_stats()["pcg_iterations"] > 0
    finally:
        ctx.close()


def test_classic_loop_with_the_factors_as_preconditioner(precond_direct_solve):
    """CG preconditioned by the fp32-stored three-level factors on every solve (`PD_CHOICE` 1): their top separator's
    finish (`k_blr_finish` or `k_dense_sym_finish`) runs inside the step and is handed the flags."""
    mesh = LF.mesh_small()
    ctx = _solver(mesh).ctx
    try:
        assert ctx.precond_direct is not None and not ctx.dense_direct
        blr = ctx.precond_direct_blr()
        _all_positions(ctx, mesh, f"factors as preconditioner ({precond_direct_solve}, top separator: {blr})")
        stats = ctx.precond_direct_stats()
        assert stats["solves_factors"] > 0 and stats["solves_vcycle"] == 0, stats
    finally:
        ctx.close()


# ------------------------------------------------------------------ (c) direct solves, run-ahead and classic loop
@pytest.mark.parametrize("mesh_of", [LF.mesh_small, LF.mesh_17_workgroups], ids=["1452", "4099"])
def test_dense_inverse_in_both_loops(mesh_of, direct_solve, monkeypatch):
    def check(ctx):
        assert ctx.substructure is None

    out = _both_loops(monkeypatch, mesh_of(), "dense inverse", check=check)
    assert out["run_ahead_syncs"] < out["classic_syncs"]


def _levels(k):
    def check(ctx):
        assert ctx.substructure is not None and ctx.substructure.get("levels", 1) == k, ctx.substructure

    return check


def test_one_level_in_both_loops(substructured_solve, monkeypatch):
    """(`spike_sites` asserts: "first" is a row of a part interior, "last" one of the separator -- different branches
    of `k_sub_up`.)"""
    _both_loops(monkeypatch, LF.mesh_small(), "one level", check=_levels(1))


def test_two_levels_in_both_loops(two_level_solve, monkeypatch):
    _both_loops(monkeypatch, LF.mesh_small(), f"two levels ({two_level_solve})", check=_levels(2))


def test_three_levels_in_both_loops(three_level_solve, monkeypatch):
    _both_loops(monkeypatch, LF.mesh_17_workgroups(), f"three levels ({three_level_solve})", check=_levels(3))


# ------------------------------------------------------------------ (d) ensemble
def _ensemble_options(retries=10):
    from tdgl_amd import SolverOptions

    return SolverOptions(solve_time=1e9, dt_init=LF.DT_INIT, dt_max=0.1, save_every=10**9, pcg_rtol=1e-12,
                         max_solve_retries=retries, adaptive_time_step_multiplier=LF.MULTIPLIER)


def _ensemble_load(ens, ctx, problems, opts):
    for r, p in enumerate(problems):
        ens.set_link_exponents(r, p["A"])
        ens.set_mu_boundary(r, np.zeros(ctx.n_boundary))
        ens.set_epsilon(r, p["epsilon"])
        ens.set_state(r, p["psi0"], p["mu0"])
        ens.set_controller(r, opts)
        ens.begin_stage(r)


@pytest.fixture(params=["dense", "one_level"])
def ensemble_path(request, monkeypatch):
    if request.param == "one_level":
        from tdgl_amd import ensemble
        from tdgl_amd.hipcore import TDGLContext

        monkeypatch.setattr(TDGLContext, "DENSE_MAX_SITES", 199)
        monkeypatch.setattr(TDGLContext, "SUB_MAX_SITES", 10 ** 9)
        monkeypatch.setattr(TDGLContext, "SUB_BLOCK", 150)
        monkeypatch.setattr(ensemble, "ENSEMBLE_DENSE_MAX_SITES", 199)
    return request.param


def test_ensemble_with_two_spiked_replicas(ensemble_path):
    """R = 17: replica 9 spiked in its last workgroup, replica 16 (alone in the third group of 8 of the substructured
    path) in workgroup 0, every other replica spike-free with the same psi_0 -- `k_ens_finish` / `k_ens_sub_up`
    (``fail_part[(g0 + q) * nfail + f % nfail]``) and `k_ens_sub_control` read each replica's own row.  (An ensemble
    reports neither a retry count nor the controller's history per replica: the retries show in the exact dts, the
    history is out of reach here.)"""
    from tdgl_amd.ensemble import EnsembleContext, build_context

    mesh = LF.mesh_small()
    opts = _ensemble_options()
    ctx = build_context(mesh, opts, None, U_DEFAULT, GAMMA_DEFAULT)
    ens = None
    try:
        sites = _sites(ctx)
        R = 17
        spiked = {9: sites["last"], 16: sites["first"]}
        problems = [LF.spiked_problem(mesh, spiked[r][1] if r in spiked else None, LF.EPS_ONE_RETRY) for r in range(R)]
        ens = EnsembleContext(ctx, R)
        assert ens.mu_path()[0] == (0 if ensemble_path == "dense" else 1)
        _ensemble_load(ens, ctx, problems, opts)
        res = ens.run(np.full(R, LF.N_STEPS), np.full(R, np.inf))
        states = [ens.get_state(r) for r in range(R)]
        plain = LF.oracle_steps(problems[0])
        assert plain["retries"] == 0 and np.array_equal(plain["dts"], [LF.DT_INIT] * LF.N_STEPS)
        for r in range(R):
            want = LF.oracle_steps(problems[r]) if r in spiked else plain
            dev = _field_deviation(states[r], want["steps"][-1])
            if r in spiked or r == 0:
                print(f"ensemble ({ensemble_path}), replica {r}: " +
                      (f"workgroup {spiked[r][0]}, site {spiked[r][1]}, " if r in spiked else "no spike, ") +
                      f"oracle retries {want['retries']}, dt {res[r]['dt']}, worst field deviation {dev:.2e}")
            assert np.array_equal(res[r]["dt"], want["dts"]), (r, res[r]["dt"], want["dts"])
            assert dev < 1e-9, (r, dev)
        for r in range(1, R):  # equal inputs: bit-identical
            if r not in spiked:
                for key in ("psi", "mu", "supercurrent", "normal_current"):
                    assert np.array_equal(states[r][key], states[0][key]), (r, key)
    finally:
        if ens is not None:
            ens.close()
        ctx.close()


# ------------------------------------------------------------------ (e) more than 256 psi workgroups
@pytest.mark.parametrize("solve", ["amg_pcg", "direct"])
def test_more_than_256_workgroups(solve, request):
    """65,862 sites, 258 workgroups: the spike in workgroup 0, in workgroup 256 (the first entry of the second trip of
    the readers' loops over the flags) and in the last one; one step each, with AMG-PCG and with the product's
    direct solve at this size (two levels)."""
    if solve == "direct":
        request.getfixturevalue("direct_solve")
    mesh = LF.mesh_258_workgroups()
    ctx = _solver(mesh, iterative=solve == "amg_pcg").ctx
    try:
        nw = LF.workgroups(ctx)
        assert len(mesh.sites) == 65862 and nw == 258
        assert ctx.dense_direct == (solve == "direct") and (solve != "direct" or ctx.substructure["levels"] == 2)
        rows = {"workgroup 0": 0, "workgroup 256": 256 * LF.WORKGROUP, "last workgroup": len(mesh.sites) - 1}
        for name, row in rows.items():
            site = LF.site_in_workgroup(ctx, row // LF.WORKGROUP, row % LF.WORKGROUP)
            problem = LF.spiked_problem(mesh, site, LF.EPS_ONE_RETRY)
            want = LF.oracle_steps(problem, n_steps=1)
            assert want["retries"] == 1
            _run_steps(ctx, problem, want, f"n = 65,862 [{solve}], {name} of {nw}", n_steps=1)
    finally:
        ctx.close()


# ------------------------------------------------------------------ (f) budget spent
def _budget_spent(ctx, mesh, label, after_set_state=False):
    """Two accepted steps with a budget of 10, then a budget of 1 (epsilon_s = -1e6 needs three shrinks): the run raises
    the oracle's text, and the accepted state is still there, bit for bit."""
    w, site = LF.last_workgroup_site(mesh, ctx.perm, LF.EPS_THREE_SHRINKS, max_solve_retries=[10, 10, 1])
    problem = LF.spiked_problem(mesh, site, LF.EPS_THREE_SHRINKS)
    want = LF.oracle_steps(problem, max_solve_retries=[10, 10, 1])
    assert want["error"] is not None and len(want["steps"]) == 2 and len(want["attempts"][2]) == 3
    o = problem["options"]
    _begin(ctx, problem)
    res = ctx.run(2)
    assert np.array_equal(res["dt"], want["dts"]) and ctx.step_stats()["psi_retries"] == want["retries"]
    before = ctx.get_state()
    assert _field_deviation(before, want["steps"][-1]) < 1e-9
    if after_set_state:  # (a new state: the projection guess has no basis vector yet)
        ctx.set_state(before["psi"], before["mu"])
        before = ctx.get_state()
    loop, ctl = ctx.loop_state(), ctx.controller_state()
    ctx.set_controller(o.dt_init, o.dt_max, True, o.adaptive_window, 1, o.adaptive_time_step_multiplier)
    ctx.set_loop_state(loop["step"], loop["time"], loop["dt"])  # (a new controller begins a new stage: carry on at step 2)
    ctx.set_controller_state(ctl["tentative_dt"], ctl["history"])
    with pytest.raises(RuntimeError) as exc:
        ctx.run(1)
    assert want["error"] in str(exc.value) and "at step 2 with dt = 6.25e-05" in want["error"], (str(exc.value), want["error"])
    after = ctx.get_state()
    print(f"budget spent, {label}: workgroup {w}, site {site}, retries before {want['retries']}, message {want['error']!r}")
    for key in ("psi", "mu", "supercurrent", "normal_current"):
        assert np.array_equal(after[key], before[key]), (label, key, max_abs(after[key], before[key]))


@pytest.mark.parametrize("extrapolate, after_set_state", [(1, False), (2, False), (3, False), (3, True)])
def test_budget_spent_with_the_iterative_solve(extrapolate, after_set_state):
    mesh = LF.mesh_small()
    ctx = _solver(mesh, iterative=True).ctx
    try:
        o = ctx.poisson_options
        ctx.set_poisson_options(rtol=o["rtol"], max_iter=o["max_iter"], nu=o["nu"], check_every=o["check_every"],
                                smoother=o["smoother"], cheb_lo=o["cheb_lo"], nu_fine=o["nu_fine"], extrapolate=extrapolate)
        _budget_spent(ctx, mesh, f"AMG-PCG, extrapolate {extrapolate}" + (", after set_state" if after_set_state else ""),
                      after_set_state)
    finally:
        ctx.close()


@pytest.mark.parametrize("loop", ["run_ahead", "classic"])
def test_budget_spent_with_the_dense_inverse(loop, direct_solve, monkeypatch):
    if loop == "classic":
        monkeypatch.setenv("TDGL_NO_RUN_AHEAD", "1")
    else:
        monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    mesh = LF.mesh_small()
    ctx = _solver(mesh).ctx
    try:
        assert ctx.dense_direct and ctx.substructure is None
        _budget_spent(ctx, mesh, f"dense inverse [{loop}]")
    finally:
        ctx.close()


def test_budget_spent_with_two_levels(two_level_solve, monkeypatch):
    monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    mesh = LF.mesh_small()
    ctx = _solver(mesh).ctx
    try:
        _levels(2)(ctx)
        _budget_spent(ctx, mesh, f"two levels ({two_level_solve}) [run_ahead]")
    finally:
        ctx.close()


def test_budget_spent_in_one_replica_of_an_ensemble():
    """The spiked replica's message carries its index (test_retry_budget_exhaustion_raises_with_the_replica_index:
    `tdgl_ensemble_run` fails as a whole, so no replica's results are delivered); its accepted state survives bit for
    bit, and the spike-free replicas, equal in their inputs, are left equal to each other.  (A new controller begins a
    new stage of its replica: the message counts its steps from 0.)"""
    from tdgl_amd.ensemble import EnsembleContext, build_context

    mesh = LF.mesh_small()
    opts = _ensemble_options()
    ctx = build_context(mesh, opts, None, U_DEFAULT, GAMMA_DEFAULT)
    ens = None
    try:
        R, r_bad = 17, 9
        w, site = LF.last_workgroup_site(mesh, ctx.perm, LF.EPS_THREE_SHRINKS, max_solve_retries=[10, 10, 1])
        problems = [LF.spiked_problem(mesh, site if r == r_bad else None, LF.EPS_THREE_SHRINKS) for r in range(R)]
        want = LF.oracle_steps(problems[r_bad], max_solve_retries=[10, 10, 1])
        assert want["error"] is not None and len(want["steps"]) == 2
        ens = EnsembleContext(ctx, R)
        _ensemble_load(ens, ctx, problems, opts)
        res = ens.run(np.full(R, 2), np.full(R, np.inf))
        assert np.array_equal(res[r_bad]["dt"], want["dts"])
        before = ens.get_state(r_bad)
        assert _field_deviation(before, want["steps"][-1]) < 1e-9
        ens.set_controller(r_bad, _ensemble_options(retries=1))
        text = "replica 9: " + want["error"].replace("at step 2", "at step 0")
        with pytest.raises(RuntimeError) as exc:
            ens.run(np.full(R, 1), np.full(R, np.inf))
        assert text in str(exc.value), (str(exc.value), text)
        after = ens.get_state(r_bad)
        print(f"budget spent, ensemble replica {r_bad}: workgroup {w}, site {site}, message {text!r}")
        for key in ("psi", "mu", "supercurrent", "normal_current"):
            assert np.array_equal(after[key], before[key]), key
        others = [ens.get_state(r) for r in range(R) if r != r_bad]
        for st in others[1:]:
            for key in ("psi", "mu", "supercurrent", "normal_current"):
                assert np.array_equal(st[key], others[0][key]) and np.all(np.isfinite(st[key])), key
    finally:
        if ens is not None:
            ens.close()
        ctx.close()


# ------------------------------------------------------------------ (g) two ranks
def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank1_site(mesh):
    """A site that rank 1 of two owns and rank 0 does not hold as a ghost, in rank 1's last psi workgroup: the highest
    of its owned rows without a neighbour on the other rank (`LocalProblem.n_interior`), through the local-to-global
    map of its owned rows."""
    from tdgl_amd.partition import build_local_problem, rcb_partition

    part = rcb_partition(mesh.sites, 2)
    lp0, lp1 = build_local_problem(mesh, part, 0), build_local_problem(mesh, part, 1)
    row = lp1.n_interior - 1
    assert row // LF.WORKGROUP == (lp1.n_own - 1) // LF.WORKGROUP >= 1
    site = int(lp1.local_to_global[:lp1.n_own][row])
    assert part[site] == 1 and site not in set(lp0.local_to_global.tolist())
    return row // LF.WORKGROUP, site


def _rank_worker(rank, world, port, out_dir, site):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for p in (ROOT, os.path.join(ROOT, "py-tdgl_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from tdgl_amd import _lib  # noqa: F401  (load libtdgl_hip and its ROCm runtime before torch)

    _lib.load()
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tdgl_amd.distributed import DistributedTDGL

        mesh = LF.mesh_small()
        problem = LF.spiked_problem(mesh, site, LF.EPS_ONE_RETRY)
        run = DistributedTDGL(mesh, _ensemble_options(), problem["A"], problem["epsilon"], U_DEFAULT, GAMMA_DEFAULT,
                              rank=rank, world=world, transport="gloo", device_id=0)
        assert site in set(run.lp.local_to_global[:run.lp.n_own].tolist()) if rank == 1 else \
            site not in set(run.lp.local_to_global.tolist())
        if rank == 1:
            row = int(np.flatnonzero(run.lp.local_to_global[:run.lp.n_own] == site)[0])
            assert LF.site_in_workgroup(run.ctx, row // LF.WORKGROUP, row % LF.WORKGROUP, run.lp.local_to_global[:run.lp.n_own]) == site
        run.set_state(problem["psi0"], problem["mu0"])
        run.begin_stage()
        run.ctx.step_stats(reset=True)
        res = run.run(LF.N_STEPS)
        fields = run.gather_state()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), dt=res["dt"], retries=run.ctx.step_stats()["psi_retries"],
                 history=run.ctx.controller_state()["history"], **(fields if rank == 0 else {}))
        run.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_a_failure_only_one_of_them_sees(tmp_path):
    """`k_status_pack` and the status reduction across ranks: the spike sits at a site of rank 1 that rank 0 does not
    even hold as a ghost, and both ranks must retry."""
    import torch.multiprocessing as mp

    mesh = LF.mesh_small()
    w, site = _rank1_site(mesh)
    problem = LF.spiked_problem(mesh, site, LF.EPS_ONE_RETRY)
    want = LF.oracle_steps(problem)
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path), site), nprocs=2, join=True)
    got = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2)]
    want_dmax = np.array([s["dmax"] for s in want["steps"]])
    fields = {k: got[0][k] for k in ("psi", "mu", "supercurrent", "normal_current")}
    dev = _field_deviation(fields, want["steps"][-1])
    dmax_dev = [float(np.max(np.abs(g["history"][-LF.N_STEPS:] - want_dmax) / np.maximum(1.0, want_dmax))) for g in got]
    print(f"two ranks: rank 1's workgroup {w}, site {site}, retries {[int(g['retries']) for g in got]} (oracle "
          f"{want['retries']}), dt {got[0]['dt']}, worst field deviation {dev:.2e}, dmax deviation {max(dmax_dev):.2e}")
    for r in range(2):
        assert np.array_equal(got[r]["dt"], want["dts"]), (r, got[r]["dt"], want["dts"])
        assert int(got[r]["retries"]) == want["retries"], (r, got[r]["retries"])
        assert len(got[r]["history"]) == LF.N_STEPS and dmax_dev[r] <= 1e-11, (r, got[r]["history"], want_dmax)
    assert dev < 1e-9, dev
