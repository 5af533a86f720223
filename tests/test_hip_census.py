"""GPU tests of the census inside the time loops (csrc/census.inc): per accepted step one int32 row
``(n_plus, n_minus, w_0 .. w_{L-1})``, compared with the NumPy model (`census_model.census_row`:
`tdgl_amd.vortices.triangle_charges` + `loop_winding`) on the context's own psi and with the CPU oracle's census.

Inputs and the oracle record: tests/census_model.py; tests/test_census_host.py asserts on the CPU that the oracle's
census has the transitions these tests rely on (so none of them passes on all-zero rows) and that the vortex of the
189-site input lasts beyond step 1,100.

Comparisons with the model on the own state are exact: both apply the same comparisons of separately rounded products
to the same doubles.  Against the oracle the rows may differ only where a sign decision sits at a tie, that is next to
a transition: rows within 2 steps of an oracle transition are left out (at most 5 per transition), and the test
asserts that nothing else is.
"""

import os

import numpy as np
import pytest

import census_model as M
from conftest import load_golden
from helpers import GAMMA_DEFAULT, U_DEFAULT, edge_terminal, reference_mesh, uniform_field_A

pytestmark = pytest.mark.gpu

LOOPS = ("run_ahead", "classic", "amg_pcg")


def _solver(p, loop, monkeypatch, request, probes=None, epsilon=1.0, **kw):
    """A `TDGLSolver` on the problem's mesh in one of the three loops: the run-ahead loop (dense inverse), the classic
    loop with the same direct solve (TDGL_NO_RUN_AHEAD=1 at create) or the classic loop with AMG-PCG."""
    from tdgl_amd import SolverOptions, TDGLSolver

    if loop == "amg_pcg":
        extra = dict(sparse_solver="amg_pcg")
    else:
        request.getfixturevalue("direct_solve")
        extra = {}
    if loop == "classic":
        monkeypatch.setenv("TDGL_NO_RUN_AHEAD", "1")
    else:
        monkeypatch.delenv("TDGL_NO_RUN_AHEAD", raising=False)
    o = p["options"]
    opts = SolverOptions(solve_time=1e9, dt_init=o.dt_init, dt_max=o.dt_max, save_every=10**9, pcg_rtol=1e-12,
                         terminal_psi=kw.pop("terminal_psi", None), **extra)
    solver = TDGLSolver.from_dimensionless(p["mesh"], opts, p["A"], epsilon, U_DEFAULT, GAMMA_DEFAULT, probe_points=probes, **kw)
    assert solver.ctx.dense_direct == (loop != "amg_pcg")
    return solver


def _set_census(ctx, p, on=True):
    if on:
        ctx.set_census(p["mesh"].sites, p["mesh"].elements, p["loops"])
    else:
        ctx.set_census()


def _begin(ctx, p, psi0=None, retries=10):
    o = p["options"]
    ctx.set_state(p["psi0"] if psi0 is None else psi0, p["mu0"])
    ctx.set_controller(o.dt_init, o.dt_max, True, o.adaptive_window, retries, o.adaptive_time_step_multiplier)
    ctx.begin_stage()
    ctx.step_stats(reset=True)


def _stepwise(ctx, p, n_steps):
    """``n_steps`` calls of ``run(1)``, each followed by `get_state`: the rows, the model's rows on those states, dt."""
    rows, psis, dts = [], [], []
    for _ in range(n_steps):
        res = ctx.run(1)
        assert res["census"].shape == (1, 2 + len(p["loops"])) and res["census"].dtype == np.int32
        rows.append(res["census"][0])
        dts.append(res["dt"][0])
        psis.append(ctx.get_state()["psi"])
    return np.array(rows), M.census_rows(psis, p["mesh"], p["loops"]), np.array(dts)


# ------------------------------------------------------------------ 1. own state, three loops
def test_rows_equal_the_model_on_the_own_state_in_every_loop(monkeypatch, request):
    """Input B, 120 steps: taken one call per step every row equals the model on that call's psi; the same steps in one
    call give the same rows; run-ahead and classic rows are identical."""
    p = M.problem("B")
    n_steps = 120
    rows = {}
    for loop in LOOPS:
        ctx = _solver(p, loop, monkeypatch, request).ctx
        try:
            _set_census(ctx, p)
            _begin(ctx, p)
            got, want, dts = _stepwise(ctx, p, n_steps)
            assert np.array_equal(got, want), (loop, np.flatnonzero((got != want).any(axis=1)))
            _begin(ctx, p)
            once = ctx.run(n_steps)
            assert np.array_equal(once["dt"], dts), loop
            assert np.array_equal(once["census"], got), (loop, np.flatnonzero((once["census"] != got).any(axis=1)))
            if loop == "amg_pcg":
                assert ctx.step_stats()["pcg_iterations"] > 0
            rows[loop] = got
        finally:
            ctx.close()
        print(f"{loop}: transitions {M.transitions(rows[loop])}")
        assert len(M.transitions(rows[loop])) >= 2  # (not a constant: the vortex enters the hole)
    assert np.array_equal(rows["run_ahead"], rows["classic"])


# ------------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize("name, n_steps, max_excluded", [("A", 100, 10), ("B", 120, 5)])
def test_rows_follow_the_oracle(name, n_steps, max_excluded, monkeypatch, request):
    """The sequence of distinct rows equals the oracle's, and every row outside the windows around the oracle's
    transitions equals the oracle's row (measured on an MI355X: no row differs at all, inside or outside the windows).

    psi: the device's is within 1e-8 of the oracle's only for the first ~20 updates, before any transition.  The cause
    is the trajectory, not the device: on these inputs the oracle's own psi moves by E[k] = 1e-12 after the first
    update and by 1e-4 after 80 when its START is changed by one rounding (`census_model.oracle_sensitivity`; asserted
    on the CPU in tests/test_census_host.py), and the device, which starts 8e-13 (A) / 1.4e-12 (B) from the oracle
    after one update, follows that growth step for step (measured 1.4e-8 / 1.1e-9 after update 43, 2.5e-5 / 1.8e-6
    after update 76, against E = 2.1e-8 / 5.5e-9 and 1e-4 / 9e-6).  So what is asserted for psi, after EVERY update, is
    the bound that follows from it, `census_model.deviation_bound`: (k + 1) * 5e-12 * E[k] / E[0], wherever that is
    below 1 -- 2.5e-8 after update 22 and 3e-6 after update 43 on input A: a step that differed from the oracle's in
    more than rounding would be caught long before the first transition.  The rows agree although psi drifts apart:
    a count or a winding changes only when a zero of psi crosses a mesh edge.  (dt is printed: it is a function of
    psi's change per step and drifts with it; once the film has relaxed, an update at dt = 0.1 sits at the edge of
    failing and the oracle's own twins retry at different steps too.)"""
    p = M.problem(name)
    want, want_dt, _ = M.oracle_census(name, n_steps)
    want_psi, bound = M.oracle_states(name, n_steps), M.deviation_bound(name, n_steps)
    changes = [k for k, _ in M.transitions(want)][1:]
    near = np.zeros(n_steps, dtype=bool)
    for k in changes:
        near[max(k - 2, 0):k + 3] = True
    assert near.sum() <= max_excluded and len(changes) == max_excluded // 5
    ctx = _solver(p, "run_ahead", monkeypatch, request).ctx
    try:
        _set_census(ctx, p)
        _begin(ctx, p)
        got, dts, psis = [], [], []
        for _ in range(n_steps):
            res = ctx.run(1)
            got.append(res["census"][0])
            dts.append(res["dt"][0])
            psis.append(ctx.get_state()["psi"])
        got, dts = np.array(got), np.array(dts)
        _begin(ctx, p)
        once = ctx.run(n_steps)
    finally:
        ctx.close()
    dev = np.array([M.deviation(psis[k], want_psi[k]) for k in range(n_steps)])
    checked = np.flatnonzero(bound < 1.0)
    differs = (got != want).any(axis=1)
    dt_off = np.flatnonzero(np.abs(dts - want_dt) > 1e-9 * want_dt)
    show = [0, 21, 42, changes[0], changes[-1], changes[-1] + 3]
    print(f"input {name}: oracle transitions {M.transitions(want)}, device {M.transitions(got)}, rows that differ "
          f"{np.flatnonzero(differs)}; |psi - oracle| / bound after update k + 1: "
          + ", ".join(f"{k}: {dev[k]:.1e} / {bound[k]:.1e}" for k in show)
          + f"; bound below 1 up to update {checked[-1] + 1}, below 1e-8 up to update {np.flatnonzero(bound < 1e-8)[-1] + 1}; "
          f"largest dev / bound {np.max(dev[checked] / bound[checked]):.2g}; dt deviates by more than 1e-9 first at step "
          f"{dt_off[0] if len(dt_off) else None} ({len(dt_off)} steps)")
    assert np.array_equal(once["census"], got) and np.array_equal(once["dt"], dts)
    assert checked[-1] >= changes[0] + 3  # (the bound says something up to beyond the first transition)
    assert np.all(dev[checked] <= bound[checked]), (np.flatnonzero(dev[checked] > bound[checked]), dev[checked], bound[checked])
    assert [row for _, row in M.transitions(got)] == [row for _, row in M.transitions(want)]
    assert not differs[~near].any(), np.flatnonzero(differs & ~near)


# ------------------------------------------------------------------ 3. retries write no row
def _spiked_epsilon(p):
    mesh = p["mesh"]
    interior = np.setdiff1d(np.arange(len(mesh.sites)), mesh.boundary_indices)
    site = int(interior[np.argmin(np.linalg.norm(mesh.sites[interior] - np.array([-2.5, -2.5]), axis=1))])
    eps = np.ones(len(mesh.sites))
    eps[site] = -3.0e4  # (tests/local_failure.py: the update fails at dt = 1e-3 at this site alone)
    return eps


@pytest.mark.parametrize("loop", ["run_ahead", "classic"])
def test_a_failed_attempt_writes_no_row(loop, monkeypatch, request):
    p = M.problem("A")
    n_steps = 30
    ctx = _solver(p, loop, monkeypatch, request, epsilon=_spiked_epsilon(p)).ctx
    try:
        _set_census(ctx, p)
        _begin(ctx, p)
        got, want, dts = _stepwise(ctx, p, n_steps)
        assert ctx.step_stats()["psi_retries"] >= 1
        assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))
        _begin(ctx, p)
        once = ctx.run(n_steps)
        stats = ctx.step_stats()
        print(f"{loop}: {stats['psi_retries']} repeated updates in {stats['steps']} steps, transitions {M.transitions(got)}")
        assert stats["psi_retries"] >= 1 and stats["steps"] == n_steps == len(once["dt"])
        assert once["census"].shape == (n_steps, 3)
        assert np.array_equal(once["dt"], dts) and np.array_equal(once["census"], got)
        assert (got[:, :2] > 0).any()
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. across a ring flush
@pytest.mark.parametrize("probes", [None, (3, 77)], ids=["no_probes", "probes"])
@pytest.mark.parametrize("loop", ["run_ahead", "classic"])
def test_rows_across_a_flush_of_the_ring(loop, probes, monkeypatch, request):
    """1,100 steps of the 189-site input in one call (the ring holds 1,024) against the same run in calls of 100."""
    p = M.problem("A12")
    n_steps = 1100
    ctx = _solver(p, loop, monkeypatch, request, probes=probes).ctx
    try:
        _begin(ctx, p)
        ctx.run(300)  # (the run-ahead loop's batches have grown to their full length: both runs below start alike)
        runs = {}
        for census in (True, False):
            _set_census(ctx, p, census)
            _begin(ctx, p)
            res = ctx.run(n_steps)
            runs[census] = (res, ctx.step_stats()["host_syncs"])
        once = runs[True][0]
        assert runs[False][0]["census"] is None and once["census"].shape == (n_steps, 3)
        if probes is not None:
            assert runs[True][1] == runs[False][1], runs  # the census rides in the probe ring's synchronisations
        _set_census(ctx, p)
        _begin(ctx, p)
        parts = [ctx.run(100) for _ in range(n_steps // 100)]
        assert np.array_equal(np.concatenate([r["dt"] for r in parts]), once["dt"])
        chunks = np.concatenate([r["census"] for r in parts])
        assert np.array_equal(chunks, once["census"]), np.flatnonzero((chunks != once["census"]).any(axis=1))
        print(f"{loop}, probes {probes}: transitions {M.transitions(once['census'])}, host synchronisations "
              f"{runs[True][1]} with the census, {runs[False][1]} without")
        assert (once["census"][1024:, :2] > 0).any()  # (the vortex lasts: test_census_host.py)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. the census changes nothing
@pytest.mark.parametrize("loop", ["run_ahead", "classic"])
@pytest.mark.parametrize("name, n_steps", [("A", 100), ("B", 120)])
def test_census_changes_no_output(name, n_steps, loop, monkeypatch, request):
    p = M.problem(name)
    ctx = _solver(p, loop, monkeypatch, request, probes=(1, len(p["mesh"].sites) // 2)).ctx
    try:
        out = {}
        for census in (False, True):
            _set_census(ctx, p, census)
            _begin(ctx, p)
            out[census] = (ctx.run(n_steps), ctx.get_state())
        assert out[False][0]["census"] is None and len(out[True][0]["census"]) == n_steps
        for key in ("dt", "mu", "theta"):
            assert np.array_equal(out[False][0][key], out[True][0][key]), key
        for key in ("psi", "mu", "supercurrent", "normal_current"):
            assert np.array_equal(out[False][1][key], out[True][1][key]), key
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6. ensemble
def test_ensemble_rows_equal_each_replica_run_alone(monkeypatch, request):
    """R = 3 on the 95-site mesh: input A, input A with all charges reversed, psi_0 = 1, with end times that leave one
    replica dead for whole batches."""
    from tdgl_amd import SolverOptions
    from tdgl_amd.ensemble import EnsembleContext, build_context

    names = ("A", "A_reversed", "A_uniform")
    problems = [M.problem(n) for n in names]
    p0 = problems[0]
    end_time = np.array([np.inf, 0.8, 3.0])
    max_steps = np.array([100, 100, 100])
    alone = []
    for p, t_end in zip(problems, end_time):
        ctx = _solver(p, "run_ahead", monkeypatch, request).ctx
        try:
            _set_census(ctx, p)
            _begin(ctx, p)
            alone.append(ctx.run(100, t_end))
        finally:
            ctx.close()
    o = p0["options"]
    opts = SolverOptions(solve_time=1e9, dt_init=o.dt_init, dt_max=o.dt_max, save_every=10**9, pcg_rtol=1e-12, terminal_psi=None)
    ctx = build_context(p0["mesh"], opts, None, U_DEFAULT, GAMMA_DEFAULT)
    ens = None
    try:
        ens = EnsembleContext(ctx, 3)
        _set_census(ctx, p0)
        ens.set_census()
        for r, p in enumerate(problems):
            ens.set_link_exponents(r, p["A"])
            ens.set_mu_boundary(r, np.zeros(ctx.n_boundary))
            ens.set_epsilon(r, np.ones(ctx.n))
            ens.set_state(r, p["psi0"], p["mu0"])
            ens.set_controller(r, opts)
            ens.begin_stage(r)
        res = ens.run(max_steps, end_time)
        batches = ens.stats()["batches"]
        for r, name in enumerate(names):
            print(f"replica {r} ({name}): {len(res[r]['dt'])} steps, transitions {M.transitions(res[r]['census'])}")
            assert len(res[r]["dt"]) == len(alone[r]["dt"]), r
            assert res[r]["census"].shape == (len(res[r]["dt"]), 3)
            assert np.array_equal(res[r]["census"], alone[r]["census"]), (r, np.flatnonzero((res[r]["census"] != alone[r]["census"]).any(axis=1)))
        steps = [len(res[r]["dt"]) for r in range(3)]
        assert steps[1] < steps[2] < steps[0] == 100 and batches >= 3  # (replica 1 was dead for whole batches)
        assert (res[0]["census"][:, :2] > 0).any() and (res[1]["census"][:, 2] == -1).any()
        # the next call asks replica 0 alone for steps: the dead replicas gain no rows
        again = ens.run(np.array([10, 0, 0]), end_time)
        assert [len(a["census"]) for a in again] == [10, 0, 0] and [len(a["dt"]) for a in again] == [10, 0, 0]
        # the context's census changed behind the ensemble's back: refused by name until it is taken over again
        ctx.set_census(p0["mesh"].sites, p0["mesh"].elements, ())
        with pytest.raises(RuntimeError, match="tdgl_ensemble_set_census"):
            ens.run(np.array([1, 0, 0]), end_time)
        ctx.set_census()
        with pytest.raises(RuntimeError, match="tdgl_ensemble_set_census"):
            ens.run(np.array([1, 0, 0]), end_time)
        _set_census(ctx, p0)  # (even the same census again: another one as far as the ensemble can tell)
        with pytest.raises(RuntimeError, match="tdgl_ensemble_set_census"):
            ens.run(np.array([1, 0, 0]), end_time)
        ens.set_census()
        assert ens.run(np.array([3, 0, 0]), end_time)[0]["census"].shape == (3, 3)
    finally:
        if ens is not None:
            ens.close()
        ctx.close()


# ------------------------------------------------------------------ 7. edges of the contract
def test_rim_winding_is_undefined_with_terminals(monkeypatch, request):
    """A strip with two terminals has psi = 0 on the rim's terminal sites: the rim winding is WINDING_UNDEFINED in
    every row while the counts are those of the model."""
    from tdgl_amd.hipcore import WINDING_UNDEFINED

    mesh = reference_mesh(load_golden("mesh_strip"))
    terms = [edge_terminal(mesh, "source", -30.0), edge_terminal(mesh, "drain", 30.0)]
    p = dict(mesh=mesh, loops=M.loops_of(mesh), A=uniform_field_A(mesh, 0.3), mu0=np.zeros(len(mesh.sites)), options=M.options())
    solver = _solver(p, "amg_pcg", monkeypatch, request, terminal_psi=0.0, terminal_info=terms,
                     current_func={"source": 6.0, "drain": -6.0})
    ctx = solver.ctx
    try:
        assert len(p["loops"]) == 1 and WINDING_UNDEFINED == M.WINDING_UNDEFINED
        _set_census(ctx, p)
        _begin(ctx, p, psi0=solver.psi_init)
        solver.update_mu_boundary(0.0)
        got, want, _ = _stepwise(ctx, p, 12)
        assert np.array_equal(got, want)
        assert np.all(got[:, 2] == WINDING_UNDEFINED) and np.all(got[:, :2] >= 0)
    finally:
        ctx.close()


def test_bad_arguments_capacity_and_switching(monkeypatch, request):
    import ctypes as C

    from tdgl_amd import _lib
    from tdgl_amd.hipcore import TDGLContext
    from tdgl_amd.partition import build_local_problem, rcb_partition

    p = M.problem("A")
    mesh, loops = p["mesh"], p["loops"]
    n = len(mesh.sites)
    ctx = _solver(p, "run_ahead", monkeypatch, request).ctx
    try:
        _set_census(ctx, p)
        bad_elements = mesh.elements.copy()
        bad_elements[5, 1] = n
        bad_loop = [np.array(loops[0], dtype=np.int64)]
        bad_loop[0][3] = -1
        for args, text in (((mesh.sites, bad_elements, loops), "out of range"),
                           ((mesh.sites, mesh.elements, bad_loop), "out of range"),
                           ((mesh.sites, mesh.elements, [loops[0][:2]]), "at least 3")):
            with pytest.raises(ValueError, match=text):
                ctx.set_census(*args)
        # the context stays usable, with the census it had
        _begin(ctx, p)
        first = ctx.run(50)
        assert first["census"].shape == (50, 3) and (first["census"][:, :2] > 0).any()
        # capacity_rows below n_rows: the true number, the first rows only
        lib = _lib.load()
        rows = np.full((7, 3), 12345, dtype=np.int32)
        n_rows = C.c_int64(-1)
        assert lib.tdgl_get_census(ctx._ctx, 4, _lib.p_i32(rows), C.byref(n_rows)) == 0
        assert n_rows.value == 50 and np.array_equal(rows[:4], first["census"][:4]) and np.all(rows[4:] == 12345)
        assert lib.tdgl_get_census(ctx._ctx, 0, None, C.byref(n_rows)) == 0 and n_rows.value == 50
        # off and on again
        _set_census(ctx, p, False)
        _begin(ctx, p)
        assert ctx.run(50)["census"] is None
        assert lib.tdgl_get_census(ctx._ctx, 0, None, C.byref(n_rows)) == 0 and n_rows.value == 0
        _set_census(ctx, p)
        _begin(ctx, p)
        assert np.array_equal(ctx.run(50)["census"], first["census"])
        # loops alone, triangles alone
        ctx.set_census(None, None, loops)
        _begin(ctx, p)
        only_loops = ctx.run(50)["census"]
        assert np.array_equal(only_loops[:, 2], first["census"][:, 2]) and not only_loops[:, :2].any()
        ctx.set_census(mesh.sites, mesh.elements, ())
        _begin(ctx, p)
        assert np.array_equal(ctx.run(50)["census"], first["census"][:, :2])
    finally:
        ctx.close()
    # a rank of a one-process-per-GPU run refuses
    lp = build_local_problem(mesh, rcb_partition(mesh.sites, 2), 0)
    ctx = TDGLContext(lp.mesh, n_owned=lp.n_own)
    try:
        with pytest.raises(ValueError, match="one-process-per-GPU"):
            ctx.set_census(None, None, [np.arange(3)])  # (a rank's sub-mesh carries no triangles; one loop asks for the census)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 8. public surface
def _ring_device():
    import tdgl_amd as tdgl

    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    film = tdgl.Polygon("film", points=tdgl.geometry.box(6, 3))
    hole = tdgl.Polygon("hole", points=tdgl.geometry.circle(0.6, center=(0.5, 0.2)))
    device = tdgl.Device("plate", layer=layer, film=film, holes=[hole], length_units="um")
    device.make_mesh(max_edge_length=0.4, smooth=0)  # 460 sites
    return device


def _assert_census_matches_saved_steps(solution, device):
    dyn = solution.dynamics
    names = tuple(device.boundary_sites())
    assert dyn.loop_names == names and len(names) == 2
    k_steps = len(dyn.dt)
    assert dyn.windings.shape == (2, k_steps) and dyn.vortex_counts.shape == (2, k_steps)
    assert dyn.windings.dtype == np.int32 and dyn.vortex_counts.dtype == np.int32
    # (save_every = 1: saved step j holds psi after j steps; the step that ends the loop is not saved)
    assert len(solution.saved_steps) == k_steps and [s.step for s in solution.saved_steps] == list(range(k_steps))
    for k in range(k_steps - 1):
        solution.solve_step = k + 1
        w = solution.boundary_windings()
        charges = solution.vortices().charges
        assert [None if v == M.WINDING_UNDEFINED else int(v) for v in dyn.windings[:, k]] == [w[n] for n in names], k
        assert tuple(dyn.vortex_counts[:, k]) == (np.count_nonzero(charges > 0), np.count_nonzero(charges < 0)), k
    return dyn


def test_solve_and_solve_ensemble_with_vortex_census(direct_solve):
    import tdgl_amd as tdgl

    device = _ring_device()
    # (2.5 mT on this film: on the CPU oracle vortices and antivortices appear from step 26 on)
    opts = tdgl.SolverOptions(solve_time=0.3, dt_init=1e-3, dt_max=0.1, save_every=1, field_units="mT", vortex_census=True)
    field = 2.5
    solution = tdgl.solve(device, opts, applied_vector_potential=field)
    dyn = _assert_census_matches_saved_steps(solution, device)
    print(f"solve: {len(dyn.dt)} steps, net vorticity {dyn.net_vorticity()[-1]}, windings {dyn.windings[:, -1]}")
    assert len(dyn.dt) >= 40 and dyn.vortex_counts.any() and (dyn.windings[0] != 0).any()
    off = tdgl.solve(device, tdgl.SolverOptions(solve_time=0.3, dt_init=1e-3, dt_max=0.1, save_every=1, field_units="mT"),
                     applied_vector_potential=field)
    assert off.dynamics.windings is None and off.dynamics.vortex_counts is None and off.dynamics.loop_names is None
    assert np.array_equal(off.dynamics.dt, dyn.dt)
    sols = tdgl.solve_ensemble(device, opts, applied_vector_potential=[field, 0.0])
    ens = _assert_census_matches_saved_steps(sols[0], device)
    assert ens.vortex_counts.any()
    assert not sols[1].dynamics.vortex_counts.any() and not sols[1].dynamics.windings.any()
