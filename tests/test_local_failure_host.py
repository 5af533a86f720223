"""The one-site failure input of tests/test_hip_local_failure.py, checked on the CPU (tests/local_failure.py).

For every (mesh, site order, spiked site, epsilon_s) the GPU tests use, `oracle_steps` runs `OracleSolver` and asserts
the helper's three conditions: every failing attempt fails at exactly the spiked site, min |disc| >= 1 on every attempt
of every step used, and the argmax of d|psi|^2 is the spiked site.  The site orders are those a `TDGLContext` has
under the same fixtures (`host_order`: the lines of its constructor that choose the order, which need no GPU; the GPU
tests go through ``ctx.perm`` and `spike_sites` in the same way).  The largest mesh (65,862 sites) gets the full
oracle run of its one step per position too: it takes about two seconds.
"""

import numpy as np
import pytest

import local_failure as LF


def _check_positions(mesh, perm, ptrs=(), warm=0, n_steps=LF.N_STEPS, positions=("first", "middle", "last")):
    sites = LF.spike_sites(perm, ptrs)
    for pos in positions:
        w, site = sites[pos]
        problem = LF.spiked_problem(mesh, site, LF.EPS_ONE_RETRY)
        out = LF.oracle_steps(problem, n_steps=n_steps, warm_steps=warm)  # (asserts the three conditions)
        assert out["error"] is None and len(out["steps"]) == n_steps
        # one retry per step: dt = 1e-3 fails at the spiked site, dt / 4 succeeds
        assert np.array_equal(out["dts"], [LF.DT_INIT * LF.MULTIPLIER] * n_steps) and out["retries"] == n_steps
        for attempts in out["attempts"]:
            assert [a["failed"] for a in attempts] == [True, False]
            assert list(attempts[0]["bad_sites"]) == [site]
    return sites


def test_recording_solver_is_the_oracle():
    """The helper's solver records every attempt; its steps are `OracleSolver`'s, bit for bit."""
    from oracle import OracleSolver

    mesh = LF.mesh_small()
    problem = LF.spiked_problem(mesh, 700, LF.EPS_THREE_SHRINKS)
    got = LF.oracle_steps(problem)
    plain = OracleSolver(mesh, problem["A"], problem["epsilon"], problem["u"], problem["gamma"], problem["options"])
    psi, mu, t, dt = problem["psi0"], problem["mu0"], 0.0, LF.DT_INIT
    for k in range(LF.N_STEPS):
        dt, psi, mu, js, jn = plain.update({"step": k, "time": t, "dt": dt}, None, dt, psi=psi, mu=mu)
        t += dt
        rec = got["steps"][k]
        assert dt == rec["dt"] and np.array_equal(psi, rec["psi"]) and np.array_equal(mu, rec["mu"])
        assert np.array_equal(js, rec["js"]) and np.array_equal(jn, rec["jn"]) and plain.d_psi_sq_vals[k] == rec["dmax"]
    assert got["dts"][0] == LF.DT_INIT * LF.MULTIPLIER ** 3 and got["retries"] >= 9  # three shrinks at least


def test_permutation_direction_and_workgroup_rows():
    """``perm[internal] = external``: `site_in_workgroup` on a stand-in with a context's three attributes, also for a
    rank of a decomposition (owned rows first, a local-to-global map)."""
    from types import SimpleNamespace

    mesh = LF.mesh_small()
    perm, _ = LF.host_order(mesh, direct_solve=False)
    n = len(perm)
    iperm = np.empty(n, dtype=np.int64)
    iperm[perm] = np.arange(n)
    ctx = SimpleNamespace(perm=perm, iperm=iperm, n_owned=n)
    assert LF.workgroups(ctx) == 6 and n % LF.WORKGROUP == 172
    assert LF.site_in_workgroup(ctx, 0, 0) == perm[0] and LF.site_in_workgroup(ctx, 3, 5) == perm[3 * 256 + 5]
    assert LF.site_in_workgroup(ctx, -1, None) == perm[n - 1] == LF.spike_sites(perm)["last"][1]
    with pytest.raises(AssertionError):
        LF.site_in_workgroup(ctx, 5, 172)  # (past the last valid lane)
    with pytest.raises(AssertionError):
        LF.site_in_workgroup(SimpleNamespace(perm=perm, iperm=perm, n_owned=n), 1, 0)  # (the other direction)
    rank = SimpleNamespace(perm=np.arange(900), iperm=np.arange(900), n_owned=700)
    own = np.arange(700) * 2 + 1
    assert LF.workgroups(rank) == 3 and LF.site_in_workgroup(rank, -1, None, own) == own[699]


def test_conditions_on_the_iterative_order():
    """(a), (b), (d, dense), (f): reverse Cuthill-McKee order, 1,452 and 4,099 sites; with and without the two warm
    steps of the extrapolated guesses."""
    for mesh in (LF.mesh_small(), LF.mesh_17_workgroups()):
        perm, ptrs = LF.host_order(mesh, direct_solve=False)
        assert not ptrs
        _check_positions(mesh, perm)
    _check_positions(LF.mesh_small(), LF.host_order(LF.mesh_small(), direct_solve=False)[0], warm=2)


def test_conditions_on_the_one_level_order(substructured_solve):
    mesh = LF.mesh_small()
    perm, ptrs = LF.host_order(mesh)
    assert len(ptrs) == 1
    _check_positions(mesh, perm, ptrs)


def test_conditions_on_the_two_level_order(two_level_solve):
    mesh = LF.mesh_small()
    perm, ptrs = LF.host_order(mesh)
    assert len(ptrs) == 2
    _check_positions(mesh, perm, ptrs)


def test_conditions_on_the_three_level_order(three_level_solve):
    mesh = LF.mesh_17_workgroups()
    perm, ptrs = LF.host_order(mesh)
    assert len(ptrs) == 3
    _check_positions(mesh, perm, ptrs)


def test_conditions_with_the_factors_as_preconditioner(precond_direct_solve):
    """(the context keeps the reverse Cuthill-McKee order there)"""
    mesh = LF.mesh_small()
    perm, ptrs = LF.host_order(mesh)
    assert not ptrs and np.array_equal(perm, LF.host_order(mesh, direct_solve=False)[0])


@pytest.mark.parametrize("direct", [False, True])
def test_conditions_at_258_workgroups(direct, request):
    """(e): the full oracle step for each of the three positions (one LU for all of them)."""
    if direct:
        request.getfixturevalue("direct_solve")
    mesh = LF.mesh_258_workgroups()
    n = len(mesh.sites)
    assert n == 65862 and -(-n // LF.WORKGROUP) == 258
    perm, ptrs = LF.host_order(mesh, direct_solve=direct)
    assert len(ptrs) == (2 if direct else 0)
    for row in (0, 256 * LF.WORKGROUP, n - 1):
        problem = LF.spiked_problem(mesh, int(perm[row]), LF.EPS_ONE_RETRY)
        out = LF.oracle_steps(problem, n_steps=1)
        assert out["retries"] == 1 and list(out["attempts"][0][0]["bad_sites"]) == [int(perm[row])]


def _spent_budget(mesh, perm):
    w, site = LF.last_workgroup_site(mesh, perm, LF.EPS_THREE_SHRINKS, max_solve_retries=[10, 10, 1])
    assert w == 5
    out = LF.oracle_steps(LF.spiked_problem(mesh, site, LF.EPS_THREE_SHRINKS), max_solve_retries=[10, 10, 1])
    assert len(out["steps"]) == 2 and np.all(out["dts"] <= LF.DT_INIT * LF.MULTIPLIER ** 3)
    assert [a["dt"] for a in out["attempts"][2]] == [1e-3, 2.5e-4, 6.25e-5] and all(a["failed"] for a in out["attempts"][2])
    assert out["error"] == ("Solver failed to converge in 1 retries at step 2 with dt = 6.25e-05."
                            " Try using a smaller dt_init.")


def test_conditions_for_the_spent_budget():
    """(f): epsilon_s = -1e6 in the last workgroup -- two accepted steps with three shrinks or more each, then a budget
    of 1 is spent after three attempts, with the reference's text."""
    mesh = LF.mesh_small()
    _spent_budget(mesh, LF.host_order(mesh, direct_solve=False)[0])


def test_conditions_for_the_spent_budget_on_the_two_level_order(two_level_solve):
    mesh = LF.mesh_small()
    _spent_budget(mesh, LF.host_order(mesh)[0])


def test_conditions_for_the_site_of_rank_one():
    """(g): a site rank 1 of two owns that rank 0 does not hold as a ghost."""
    from tdgl_amd.partition import build_local_problem, rcb_partition

    mesh = LF.mesh_small()
    part = rcb_partition(mesh.sites, 2)
    lp0, lp1 = build_local_problem(mesh, part, 0), build_local_problem(mesh, part, 1)
    row = lp1.n_interior - 1
    site = int(lp1.local_to_global[row])
    assert row // LF.WORKGROUP == (lp1.n_own - 1) // LF.WORKGROUP >= 1 and site not in set(lp0.local_to_global.tolist())
    out = LF.oracle_steps(LF.spiked_problem(mesh, site, LF.EPS_ONE_RETRY))
    assert out["retries"] == LF.N_STEPS


def test_the_controller_entry_is_well_conditioned():
    """max d|psi|^2 at the spiked site, the oracle's fp64 value against the same formula in ``np.longdouble``: the GPU
    tests hold the controller's history to 1e-11 max(1, value), and this is what the reference itself is worth there
    (measured: at most 3e-15 over the cases below)."""
    mesh = LF.mesh_small()
    perm, _ = LF.host_order(mesh, direct_solve=False)
    worst = 0.0
    for pos, (w, site) in LF.spike_sites(perm).items():
        for eps in (LF.EPS_ONE_RETRY, LF.EPS_THREE_SHRINKS):
            problem = LF.spiked_problem(mesh, site, eps)
            if not LF.conditions_hold(problem):
                continue
            out = LF.oracle_steps(problem)
            row = np.asarray(LF.oracle_solver(problem).operators.psi_laplacian[site].todense()).ravel()
            before = (problem["psi0"], problem["mu0"])
            for step in out["steps"]:
                worst = max(worst, LF.dmax_conditioning(problem, before, step, row))
                before = (step["psi"], step["mu"])
    print(f"oracle fp64 against longdouble, max d|psi|^2 at the spiked site: {worst:.2e}")
    assert worst < 1e-13  # (a hundredth of the GPU tests' 1e-11)
