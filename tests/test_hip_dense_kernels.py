"""The dense mu solve's own HIP kernels against a float64 pseudo-inverse, entry by entry (tests/dense_reference.py).

Three parts are checked, at site counts chosen on the 64-row blocks of the build and the 128 x 128 tiles of the
product (n < 64, n = 0 or 1 mod 128, a last partial tile row, a single tile):
  (a) the build (`tdgl_poisson_build_dense_inverse`: assembly, blocked Gauss-Jordan sweep, `k_dense_pack_sym`) and the
      single-run product (`k_dense_sym_tiles<double>` + `k_dense_sym_finish`) through `poisson_solve`: the whole
      operator up to 641 sites, unit vectors in the first, an off-diagonal and the last partial tile plus a random
      block above;
  (b) one step of the time loop (the run-ahead path: `dense_sym_finish_body` with a controller), mu against the
      reference solve of the right-hand side the host forms from the step's own psi;
  (c) the ensemble's product (`k_ens_dense_tiles` + `k_ens_finish`) for R replicas in groups of 16, with dead replicas
      and a whole dead group (the early return), each live replica against its own right-hand side.
The tolerance is the kappa-derived bound of dense_reference.tolerance, 8 kappa u max |x|: 1.8e-12 of max |mu| at 4k
sites, 3.6e-12 at 8k, 9e-16 at 3 sites -- at least 25 times tighter than the 1e-10 of the older checks everywhere.
"""

import functools
import os

import numpy as np
import pytest

import dense_reference as D
from helpers import uniform_field_A

pytestmark = pytest.mark.gpu

SIZES = [3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 641, 4095, 4096, 4097]
WHOLE_OPERATOR_MAX = 700  # up to here every column of G is recovered


@functools.lru_cache(maxsize=None)
def _reference(n):
    """(mesh, A, G, kappa) of the n-site mesh; built once per module (the host inverse takes seconds at 8k sites)."""
    mesh = D.mesh_with_sites(n)
    A = D.poisson_matrix_of(mesh)
    G = D.pinv_reference(A)
    return mesh, A, G, D.condition_number(A, G)


def teardown_module(module):
    _reference.cache_clear()


def _assert_device_built(ctx):
    assert "TDGL_DENSE_HOST" not in os.environ
    assert ctx.dense_direct and "dense_inverse_device" in ctx.setup_times and "dense_inverse_host" not in ctx.setup_times


def _assert_matches(mu, x, kappa, what):
    """mu [n, k] against the reference x [n, k]: every entry within the tolerance, zero mean.  Prints the deviation in
    units of kappa u max |x| (the PR reports it)."""
    tol = D.tolerance(kappa, x)
    err = np.abs(mu - x).max(axis=0)
    worst = int(np.argmax(err / tol))
    print(f"\n{what}: kappa {kappa:.4g}, max |mu - x| / max |x| = {D.max_rel_error(mu, x).max():.3g} "
          f"({(err / tol).max() * D.C_TOL:.3g} kappa u)")
    assert np.all(err <= tol), (what, worst, err[worst], tol[worst])
    assert np.all(np.abs(mu.mean(axis=0)) <= tol), what


@pytest.mark.parametrize("n", SIZES)
def test_device_inverse_and_product_match_the_float64_pseudo_inverse(n, direct_solve):
    from tdgl_amd.hipcore import TDGLContext

    mesh, A, G, kappa = _reference(n)
    ctx = TDGLContext(mesh)
    try:
        ctx.build_poisson(rtol=1e-12)
        _assert_device_built(ctx)
        rng = np.random.default_rng(n)
        if n <= WHOLE_OPERATOR_MAX:
            cols = np.arange(n)
            n_random = 4
        else:  # the first tile, both sides of the 64-row block and 128-site tile edges, the last partial tile
            cols = np.array([0, 63, 64, 127, 128, n - 129, n - 128, n - 1])
            n_random = 32
        E = np.zeros((n, len(cols)))
        E[cols, np.arange(len(cols))] = 1.0
        # (the library solves A mu = -areas * rhs, projected to zero mean: rhs = -e_j / areas applies G to e_j - 1 / n)
        rhs = np.column_stack([-E / mesh.areas[:, None], rng.standard_normal((n, n_random))])
        b = D.rhs_to_b(mesh, rhs)
        x = D.apply_reference(A, b, G)
        mu = np.empty_like(x)
        for j in range(rhs.shape[1]):
            mu[:, j], iters, relres = ctx.poisson_solve(rhs[:, j])
            assert iters == 0 and relres <= D.C_TOL * kappa * D.U, (j, relres)
        _assert_matches(mu, x, kappa, f"single-run solve, n = {n}")
    finally:
        ctx.close()


def _random_psi(rng, n):
    return (0.5 + 0.5 * rng.random(n)) * np.exp(2j * np.pi * rng.random(n))


def _host_b(mesh, A_link, psi):
    """The time loop's right-hand side of the mu solve from psi (oracle/tdgl_step.py `_observables`: no terminals, a
    static field), in float64 with the oracle's operators, as the library solves it."""
    from oracle.fv_operators import FVOperators, divergence_matrix

    ops = FVOperators(mesh)
    ops.set_link_exponents(A_link)
    return D.rhs_to_b(mesh, divergence_matrix(mesh) @ ops.get_supercurrent(psi))


@pytest.mark.parametrize("n", [65, 128, 129, 257, 4096, 4097])
def test_one_time_loop_step_solves_mu_like_the_float64_pseudo_inverse(n, direct_solve):
    from tdgl_amd import SolverOptions, TDGLSolver

    mesh, A, G, kappa = _reference(n)
    A_link = uniform_field_A(mesh, 0.2)
    solver = TDGLSolver.from_dimensionless(mesh, SolverOptions(solve_time=1e9, dt_init=1e-3, save_every=10**6), A_link, 1.0)
    ctx = solver.ctx
    try:
        _assert_device_built(ctx)
        rng = np.random.default_rng(1000 + n)
        ctx.set_state(_random_psi(rng, n), 0.1 * rng.standard_normal(n))
        ctx.begin_stage()
        res = ctx.run(1)
        assert len(res["dt"]) == 1 and res["pcg_iters"].max() == 0
        st = ctx.get_state(supercurrent=False, normal_current=False)
        x = D.apply_reference(A, _host_b(mesh, A_link, st["psi"]), G)
        _assert_matches(st["mu"][:, None], x[:, None], kappa, f"time-loop step, n = {n}")
        stats = ctx.direct_stats()
        assert not stats["fell_back"] and stats["max"] <= D.C_TOL * kappa * D.U, stats
    finally:
        ctx.close()


def _dead_replicas(R):
    """Replicas that take no step (max_steps 0: poisoned from the start).  R = 17 and R = 33 have a whole dead group of
    16 next to a live one: that group's workgroups of `k_ens_dense_tiles` return at once."""
    return {1: set(), 15: {3, 7}, 16: {0, 15}, 17: set(range(16)), 33: set(range(16, 32)) | {5}}[R]


@pytest.mark.parametrize("n, Rs", [(128, (1, 15, 16, 17, 33)), (129, (1, 15, 16, 17, 33)), (4097, (1, 15, 16, 17, 33)),
                                   (8193, (17,))])
def test_ensemble_product_matches_the_float64_pseudo_inverse(n, Rs, direct_solve):
    """n = 8,193 is above `TDGLContext.DENSE_MAX_SITES`: only the ensemble uses the dense inverse there."""
    from tdgl_amd import SolverOptions
    from tdgl_amd.ensemble import ENSEMBLE_MAX_SITES, EnsembleContext, build_context
    from tdgl_amd.hipcore import TDGLContext

    assert (n > TDGLContext.DENSE_MAX_SITES) == (n == 8193) and n <= ENSEMBLE_MAX_SITES
    mesh, A, G, kappa = _reference(n)
    opts = SolverOptions(solve_time=1e9, dt_init=1e-3, save_every=10**6)
    A_link = uniform_field_A(mesh, 0.2)
    ctx = build_context(mesh, opts, None, 5.79, 10.0)  # (as solve_ensemble sets it up: dense_max_sites=ENSEMBLE_MAX_SITES)
    try:
        _assert_device_built(ctx)
        for R in Rs:
            dead = _dead_replicas(R)
            assert any(r not in dead for r in range(R))
            rng = np.random.default_rng(100 * n + R)
            start = [(_random_psi(rng, n), 0.1 * rng.standard_normal(n)) for _ in range(R)]
            ens = EnsembleContext(ctx, R)
            try:
                for r in range(R):
                    ens.set_link_exponents(r, A_link)
                    ens.set_mu_boundary(r, np.zeros(ctx.n_boundary))
                    ens.set_epsilon(r, np.ones(n))
                    ens.set_state(r, *start[r])
                    ens.set_controller(r, opts)
                    ens.begin_stage(r)
                res = ens.run(np.array([0 if r in dead else 1 for r in range(R)]), np.full(R, np.inf))
                live = [r for r in range(R) if r not in dead]
                b, mu = [], []
                for r in range(R):
                    st = ens.get_state(r, currents=False)
                    if r in dead:  # untouched, bit for bit
                        assert len(res[r]["dt"]) == 0, r
                        assert np.array_equal(st["psi"], start[r][0]) and np.array_equal(st["mu"], start[r][1]), r
                    else:
                        assert len(res[r]["dt"]) == 1, r
                        b.append(_host_b(mesh, A_link, st["psi"]))
                        mu.append(st["mu"])
                x = D.apply_reference(A, np.column_stack(b), G)
                _assert_matches(np.column_stack(mu), x, kappa, f"ensemble, n = {n}, R = {R}, live {len(live)}")
            finally:
                ens.close()
    finally:
        ctx.close()
