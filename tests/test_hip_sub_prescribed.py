"""The substructured factors' sweep kernels entry by entry, at part sizes the test prescribes
(tests/prescribed_dissection.py): `k_sub_down`, `k_sub_down_lanes`, `k_sub_down_sym`, `k_sub_up<VT, R>`, `k_sub_repack`,
`k_pd_gather` / `k_pd_scatter` and the dense top separator behind them.

A. The fp32 factors as the CG's preconditioner, ONE application (`TDGLContext.precond_apply`) against the float64 model
   of exactly what the device stores (`rounded_to_storage`): per probe column

       d = max |z_dev - z_model| / max |z_model|  <=  max(F s, 8 kappa u),

   s = the storage error of that column (model with rounded factors against model with exact ones, host only: 1e-8 ..
   6e-8).  The device differs from the model by the order of its fp64 sums and by the top separator's inverse, which it
   forms itself: a few of that inverse's float32 roundings fall the other way.  Measured on the MI355X, largest d / s
   per case, over 34 to 60 probe columns each (F = four times the largest of them, and F <= 1 is a condition):

       mixed (257-row parts: whole blocks, lanes)       5.1e-8   (d = 2e-15: the order of the fp64 sums alone)
       tiles256 / 192 / 128 / 64 (up_R 4 / 3 / 2 / 1)   5.5e-8 / 0.0137 / 6.5e-7 / 8.6e-6
       lanes2048 (parts of 2048, 1, 2047 rows)          5.2e-8

   (0.0137, d = 4.8e-10 on a random column: the top inverse's roundings -- perturbing the host's inverse by 1e-11
   relative before rounding gives 0.05 s on the model.)  So F = 4 x 0.0137 = 0.055.

B. The fp64 direct solve (`poisson_solve`, one step of the time loop) with one level (built on the device, on the host),
   two and three levels (tiles and whole blocks) against `dense_reference.apply_reference` within 8 kappa u max |x|.

Probe columns: the unit vector at the first and the last row of one part of every distinct size on every level, the
first and last position of every level's separator, four standard-normal columns."""

import functools

import numpy as np
import pytest

import dense_reference as D
import prescribed_dissection as P
from helpers import uniform_field_A

pytestmark = pytest.mark.gpu

F = 0.055  # (four times the largest measured d / s: see the module docstring)


@functools.lru_cache(maxsize=None)
def _layout(name, K=3):
    return P.build_layout(name, K)


@functools.lru_cache(maxsize=None)
def _reference(lx):
    """(A, G, kappa) of `synthetic_mesh(lx)` in site order; once per module."""
    from helpers import synthetic_mesh

    A = D.poisson_matrix_of(synthetic_mesh(lx))
    G = D.pinv_reference(A)
    return A, G, D.condition_number(A, G)


@functools.lru_cache(maxsize=None)
def _model(name):
    """Layout ``name`` (three levels): probe columns (dissection order), the rounded model's answers, s per column."""
    lay = _layout(name)
    B = P.probe_columns(lay.ptrs, lay.n)
    exact = P.apply_levels(lay.levels, lay.G_top, B)
    rounded = P.apply_levels(*P.rounded_to_storage(lay.levels, lay.G_top), B)
    return B, rounded, np.abs(rounded - exact).max(axis=0) / np.abs(exact).max(axis=0)


def teardown_module(module):
    for f in (_layout, _reference, _model):
        f.cache_clear()


def _prescribe(monkeypatch, lists):
    """The product's three dissection functions replaced by the prescribed one (`TDGLContext._dissection_order` looks
    them up when called)."""
    from tdgl_amd import substructure

    for k, fn in enumerate(("substructure_order", "substructure_order2", "substructure_order3")):
        monkeypatch.setattr(substructure, fn, P.order_function(lists[:k + 1]))


def _report(name, lay):
    for k, d in enumerate(P.describe(lay.levels)):
        print(f"{name} level {k + 1}: {len(d['sizes'])} parts {d['sizes']}, separator sites per part {d['touch'][0]} .. "
              f"{d['touch'][1]}, separator {d['separator']}")


# ---- A: the fp32 preconditioner ------------------------------------------------------------------------------------
def _precond_ctx(name, monkeypatch, sym, blr_tol=None, rtol=1e-10):
    """(``blr_tol``: the top separator in block low-rank form at that tau, ``rtol``: the CG's tolerance to go with it --
    tests/test_hip_blr_form.py; None: dense tiles.)"""
    from tdgl_amd.hipcore import TDGLContext

    lay = _layout(name)
    # (the settings of test_hip_blr._precond_ctx; the dense fp32 top separator: the low-rank form has its own test,
    # tests/test_hip_blr_form.py, which calls this with blr_tol)
    for attr, value in (("DENSE_MAX_SITES", 199), ("SUB_MAX_SITES", 199), ("SUB2_MAX_SITES", 199), ("SUB3_MIN_SITES", 200),
                        ("SUB3_BIG", 6000), ("PD_MAX_SITES", 10 ** 9), ("PD_CHOICE", 1)):
        monkeypatch.setattr(TDGLContext, attr, value)
    monkeypatch.setenv("TDGL_PD_BLR", "0" if blr_tol is None else "1")
    if blr_tol is not None:
        monkeypatch.setenv("TDGL_PD_BLR_TOL", repr(float(blr_tol)))
    if sym:
        monkeypatch.setenv("TDGL_PD_SYM", "2")
    else:
        monkeypatch.delenv("TDGL_PD_SYM", raising=False)
    monkeypatch.delenv("TDGL_UP_PARTS", raising=False)
    _prescribe(monkeypatch, lay.lists)
    ctx = TDGLContext(lay.mesh)
    ctx.build_poisson(rtol=rtol)
    return ctx, lay


def _round_up(v, m):
    return (v + m - 1) // m * m


@pytest.mark.parametrize("name, sym", [("mixed", False), ("tiles256", True), ("tiles192", True), ("tiles128", True),
                                       ("tiles64", True), ("lanes2048", False)])
def test_one_preconditioner_application_matches_the_model_of_the_stored_factors(name, sym, monkeypatch):
    ctx, lay = _precond_ctx(name, monkeypatch, sym)
    try:
        assert ctx.precond_direct and not ctx.dense_direct, ctx.setup_times
        assert np.array_equal(ctx._pd_order[0], lay.perm) and not ctx.precond_direct_blr()["on"]
        np_max = [int(np.diff(ptr).max()) for ptr in lay.ptrs]
        assert ctx.precond_direct_layout() == ([_round_up(m, 16) for m in np_max] if sym else [0, 0, 0])
        if name.startswith("tiles"):  # (ceil(np_max / 64) row chunks per workgroup on the way up of level 1)
            assert (np_max[0] + 63) // 64 == {"tiles256": 4, "tiles192": 3, "tiles128": 2, "tiles64": 1}[name]
        _, _, kappa = _reference(P.LAYOUTS[name][0])
        floor = D.C_TOL * kappa * D.U
        B, z_model, s = _model(name)
        assert np.all(s > 0.0)
        rng = np.random.default_rng(7)
        rhs = rng.standard_normal(lay.n)
        before = ctx.poisson_solve(rhs)
        ratio = np.empty(B.shape[1])
        for j in range(B.shape[1]):
            r = B[lay.iperm, j]  # (site order: r[perm[i]] = B[i])
            z, rz = ctx.precond_apply(r)
            d = np.abs(z[lay.perm] - z_model[:, j]).max() / np.abs(z_model[:, j]).max()
            ratio[j] = d / s[j]
            assert abs(rz - r @ z) <= lay.n * D.U * np.abs(r * z).sum(), (j, rz, r @ z)
        after = ctx.poisson_solve(rhs)
        _report(name, lay)
        worst = int(np.argmax(ratio))
        print(f"{name}: kappa {kappa:.4g}, 8 kappa u {floor:.3g}, s {s.min():.3g} .. {s.max():.3g}, largest d / s = "
              f"{ratio.max():.3g} (column {worst} of {len(ratio)}; d = {ratio[worst] * s[worst]:.3g}), "
              f"random columns {ratio[-4:].max():.3g}")
        assert np.all(ratio * s <= np.maximum(F * s, floor)), (worst, ratio[worst], s[worst])
        # the CG's state is as it was: the same solve, bit for bit
        assert before[1] == after[1] and np.array_equal(before[0], after[0]) and before[2] == after[2]
        assert before[2] <= 1e-10 and 1 <= before[1] <= 3
    finally:
        ctx.close()


def test_a_part_of_2049_rows_is_refused_and_the_v_cycle_takes_over(monkeypatch):
    ctx, lay = _precond_ctx("lanes2049", monkeypatch, False)
    try:
        assert int(np.diff(lay.ptrs[0]).max()) == 2049
        assert not ctx.precond_direct and not ctx.dense_direct
        assert ctx.build_precond_direct(rtol=1e-10) is False
        assert "2049 rows (at most 2048" in ctx.setup_times["substructure_error"], ctx.setup_times
        with pytest.raises(RuntimeError, match="no substructure factors"):
            ctx.precond_apply(np.zeros(lay.n))
        rhs = np.random.default_rng(8).standard_normal(lay.n)
        mu, iters, relres = ctx.poisson_solve(rhs)
        assert relres <= 1e-10 and iters > 3  # (AMG-PCG)
        A, G, kappa = _reference(P.LAYOUTS["lanes2049"][0])
        x = D.apply_reference(A, D.rhs_to_b(lay.mesh, rhs), G)
        assert np.abs(mu - x).max() <= 1e-10 * kappa * np.abs(x).max()
    finally:
        ctx.close()


def test_precond_apply_is_refused_without_a_preconditioner(monkeypatch, substructured_solve):
    from tdgl_amd.hipcore import TDGLContext
    from tdgl_amd.partition import build_local_problem, rcb_partition

    lay = _layout("mixed", 1)
    # the factors are the SOLVER
    _prescribe(monkeypatch, lay.lists)
    ctx = TDGLContext(lay.mesh)
    try:
        with pytest.raises(RuntimeError, match="no substructure factors"):
            ctx.precond_apply(np.zeros(lay.n))
        ctx.build_poisson(rtol=1e-10)
        assert ctx.dense_direct and ctx.substructure
        with pytest.raises(RuntimeError, match="the factors are the mu solver"):
            ctx.precond_apply(np.zeros(lay.n))
    finally:
        ctx.close()
    # a rank of a one-process-per-GPU run
    lp = build_local_problem(lay.mesh, rcb_partition(lay.mesh.sites, 2), 0)
    ctx = TDGLContext(lp.mesh, n_owned=lp.n_own)
    try:
        with pytest.raises(RuntimeError, match="single-GPU contexts only"):
            ctx.precond_apply(np.zeros(ctx.n))
    finally:
        ctx.close()


# ---- B: the fp64 direct solve --------------------------------------------------------------------------------------
def _assert_matches(mu, x, kappa, what):
    tol = D.tolerance(kappa, x)
    err = np.abs(mu - x).max(axis=0)
    worst = int(np.argmax(err / tol))
    print(f"{what}: kappa {kappa:.4g}, max |mu - x| / max |x| = {D.max_rel_error(mu, x).max():.3g} "
          f"({(err / tol).max() * D.C_TOL:.3g} kappa u, column {worst} of {len(err)})")
    assert np.all(err <= tol), (what, worst, err[worst], tol[worst])
    assert np.all(np.abs(mu.mean(axis=0)) <= tol), what


def _check_probe_columns(ctx, lay, what):
    """Every probe column through `poisson_solve` (rhs = -e_j / areas applies pinv(A) to e_j - 1 / n)."""
    assert ctx.dense_direct and ctx.substructure, ctx.setup_times  # (the build's own check passed, nothing fell back)
    assert np.array_equal(ctx.perm, lay.perm)
    A, G, kappa = _reference(P.LAYOUTS[lay.name][0])
    rhs = -P.probe_columns(lay.ptrs, lay.n)[lay.iperm] / lay.mesh.areas[:, None]
    x = D.apply_reference(A, D.rhs_to_b(lay.mesh, rhs), G)
    mu = np.empty_like(x)
    for j in range(rhs.shape[1]):
        mu[:, j], iters, relres = ctx.poisson_solve(rhs[:, j])
        assert iters == 0, (j, iters, relres)
    _report(what, lay)
    _assert_matches(mu, x, kappa, what)


def _direct_ctx(name, K, monkeypatch):
    from tdgl_amd.hipcore import TDGLContext

    lay = _layout(name, K)
    _prescribe(monkeypatch, lay.lists)
    ctx = TDGLContext(lay.mesh)
    ctx.build_poisson(rtol=1e-10)
    return ctx, lay


@pytest.mark.parametrize("built_on", ["device", "host"])
def test_one_level_direct_solve_at_prescribed_part_sizes(built_on, monkeypatch, substructured_solve):
    """(The mixed list has parts of one row.)"""
    if built_on == "host":
        monkeypatch.setenv("TDGL_SUB_HOST", "1")
    else:
        monkeypatch.delenv("TDGL_SUB_HOST", raising=False)
    ctx, lay = _direct_ctx("mixed", 1, monkeypatch)
    try:
        assert ctx.dense_direct, ctx.setup_times
        assert ctx.substructure["built_on"] == built_on and ctx.substructure["parts"] == lay.levels[0].n_parts
        _check_probe_columns(ctx, lay, f"one level, built on the {built_on}")
    finally:
        ctx.close()


def _expected_tiles(lay, forced):
    return [bool(forced and int(np.diff(ptr).max()) <= 256) for ptr in lay.ptrs]


@pytest.mark.parametrize("name", ["mixed", "tiles256"])
def test_two_level_direct_solve_at_prescribed_part_sizes(name, monkeypatch, two_level_solve):
    """(Below 200k sites the separator rows of the way down carry their -E^T segments: no sparse coupling blocks.)"""
    ctx, lay = _direct_ctx(name, 2, monkeypatch)
    try:
        assert ctx.dense_direct, ctx.setup_times
        sub = ctx.substructure
        assert sub["levels"] == 2 and sub["built_on"] == "host" and not sub["sparse_separator_rhs"]
        assert sub["symmetric_tiles"] == _expected_tiles(lay, two_level_solve == "symmetric_tiles"), sub
        _check_probe_columns(ctx, lay, f"two levels, {name}, {two_level_solve}")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["mixed", "tiles256"])
def test_three_level_direct_solve_at_prescribed_part_sizes(name, monkeypatch, three_level_solve):
    ctx, lay = _direct_ctx(name, 3, monkeypatch)
    try:
        assert ctx.dense_direct, ctx.setup_times
        sub = ctx.substructure
        assert sub["levels"] == 3 and sub["sparse_separator_rhs"]
        assert sub["symmetric_tiles"] == _expected_tiles(lay, three_level_solve == "symmetric_tiles"), sub
        _check_probe_columns(ctx, lay, f"three levels, {name}, {three_level_solve}")
    finally:
        ctx.close()


def test_one_time_loop_step_on_two_prescribed_levels(monkeypatch, two_level_solve):
    """mu of one step of the time loop (the run-ahead path) against the reference solve of the right-hand side the host
    forms from the step's own psi."""
    from oracle.fv_operators import FVOperators, divergence_matrix
    from tdgl_amd import SolverOptions, TDGLSolver

    lay = _layout("mixed", 2)
    _prescribe(monkeypatch, lay.lists)
    mesh, n = lay.mesh, lay.n
    A, G, kappa = _reference(P.LAYOUTS["mixed"][0])
    A_link = uniform_field_A(mesh, 0.2)
    solver = TDGLSolver.from_dimensionless(mesh, SolverOptions(solve_time=1e9, dt_init=1e-3, save_every=10**6), A_link, 1.0)
    ctx = solver.ctx
    try:
        assert ctx.dense_direct and ctx.substructure["levels"] == 2 and np.array_equal(ctx.perm, lay.perm), ctx.setup_times
        assert ctx.substructure["symmetric_tiles"] == _expected_tiles(lay, two_level_solve == "symmetric_tiles")
        rng = np.random.default_rng(1000 + n)
        psi = (0.5 + 0.5 * rng.random(n)) * np.exp(2j * np.pi * rng.random(n))
        ctx.set_state(psi, 0.1 * rng.standard_normal(n))
        ctx.begin_stage()
        res = ctx.run(1)
        assert len(res["dt"]) == 1 and res["pcg_iters"].max() == 0
        st = ctx.get_state(supercurrent=False, normal_current=False)
        ops = FVOperators(mesh)
        ops.set_link_exponents(A_link)
        b = D.rhs_to_b(mesh, divergence_matrix(mesh) @ ops.get_supercurrent(st["psi"]))
        x = D.apply_reference(A, b, G)
        _assert_matches(st["mu"][:, None], x[:, None], kappa, f"time-loop step, two levels, {two_level_solve}")
        stats = ctx.direct_stats()
        assert not stats["fell_back"] and stats["max"] <= D.C_TOL * kappa * D.U, stats
    finally:
        ctx.close()
