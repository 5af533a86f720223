"""solve_ensemble on the substructured factors (csrc/ensemble_sub.inc): the ensemble's mu solve above the dense
inverse's cap, one and two levels, whole G blocks and symmetric tiles.

  * kernel level: one round of R replicas on small meshes with the path forced, every live replica's mu against the
    float64 pseudo-inverse (tests/dense_reference.py), dead replicas (whole dead groups of 8 among them) untouched;
  * fixture level: with the path forced, one replica of an ensemble reproduces the reference trajectories;
  * product sizes: the product's own path choice at ~20k and ~40k sites, every replica against tdgl.solve alone;
  * equal inputs in different groups of replicas give bit-identical results.
"""

import numpy as np
import pytest

import dense_reference as D
from conftest import load_golden
from helpers import edge_terminal, max_abs, reference_mesh, remove_mean, uniform_field_A
from test_hip_dense_kernels import _dead_replicas, _host_b, _random_psi
from test_hip_ensemble import _assert_like_fixture, _ensemble

pytestmark = pytest.mark.gpu


@pytest.fixture
def one_level(substructured_solve, monkeypatch):
    """The ensemble takes one level of substructured factors (parts of ~150 sites) from 200 sites up."""
    from tdgl_amd import ensemble

    monkeypatch.setattr(ensemble, "ENSEMBLE_DENSE_MAX_SITES", 199)
    return 1


@pytest.fixture
def two_levels(two_level_solve, monkeypatch):
    """... two levels (parts of ~60 sites in super-blocks of ~500), the first level as symmetric tiles or whole
    blocks (the `two_level_solve` fixture's parameter)."""
    from tdgl_amd import ensemble

    monkeypatch.setattr(ensemble, "ENSEMBLE_DENSE_MAX_SITES", 199)
    monkeypatch.setattr(ensemble, "ENSEMBLE_SUB_MAX_SITES", 199)
    return 2


def _one_round(n, levels):
    """One round of R replicas for every R of _dead_replicas on the n-site mesh, mu of the live replicas against the
    reference solve of their right-hand sides."""
    from tdgl_amd import SolverOptions
    from tdgl_amd.ensemble import EnsembleContext, build_context

    mesh = D.mesh_with_sites(n)
    A = D.poisson_matrix_of(mesh)
    G = D.pinv_reference(A)
    kappa = D.condition_number(A, G)
    opts = SolverOptions(solve_time=1e9, dt_init=1e-3, save_every=10**6)
    A_link = uniform_field_A(mesh, 0.2)
    ctx = build_context(mesh, opts, None, 5.79, 10.0)
    try:
        assert ctx.substructure is not None and ctx.substructure.get("levels", 1) == levels
        for R in (1, 15, 16, 17, 33):
            dead = _dead_replicas(R)
            rng = np.random.default_rng(100 * n + R)
            start = [(_random_psi(rng, n), 0.1 * rng.standard_normal(n)) for _ in range(R)]
            ens = EnsembleContext(ctx, R)
            try:
                assert ens.mu_path()[0] == levels and ens.mu_path()[1] > 0
                for r in range(R):
                    ens.set_link_exponents(r, A_link)
                    ens.set_mu_boundary(r, np.zeros(ctx.n_boundary))
                    ens.set_epsilon(r, np.ones(n))
                    ens.set_state(r, *start[r])
                    ens.set_controller(r, opts)
                    ens.begin_stage(r)
                res = ens.run(np.array([0 if r in dead else 1 for r in range(R)]), np.full(R, np.inf))
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
                mu = np.column_stack(mu)
                tol = D.tolerance(kappa, x)
                err = np.abs(mu - x).max(axis=0)
                print(f"\nlevels {levels}, n = {n}, R = {R}: kappa {kappa:.4g}, max |mu - x| / tol = {(err / tol).max():.3g}")
                assert np.all(err <= tol), (R, err.max(), tol.min())
                assert np.all(np.abs(mu.mean(axis=0)) <= tol), R
            finally:
                ens.close()
    finally:
        ctx.close()


def test_one_round_one_level_matches_the_float64_pseudo_inverse(one_level):
    _one_round(1500, 1)


def test_one_round_two_levels_matches_the_float64_pseudo_inverse(two_levels):
    _one_round(2600, 2)


def test_factors_the_ensemble_does_not_take_are_refused(three_level_solve):
    """Three levels: TDGL_ERR_ARG from tdgl_ensemble_create, with the reason."""
    from tdgl_amd.ensemble import EnsembleContext
    from tdgl_amd.hipcore import TDGLContext

    mesh = D.mesh_with_sites(2600)
    ctx = TDGLContext(mesh)
    try:
        ctx.build_poisson(rtol=1e-11)
        assert ctx.substructure is not None and ctx.substructure["levels"] == 3
        with pytest.raises(Exception, match="levels are not supported"):
            EnsembleContext(ctx, 2)
    finally:
        ctx.close()


def _assert_sub_stats(sol, levels):
    assert sol.stats["mu_solver"] == "substructured_ensemble" and sol.stats["mu_levels"] == levels


def test_transport_strip_one_level(one_level):
    g = load_golden("traj_transport_strip")
    mesh = reference_mesh(load_golden("mesh_strip"))
    terms = [edge_terminal(mesh, "source", -30.0), edge_terminal(mesh, "drain", 30.0)]
    cur = float(g["current"])
    sols = _ensemble(g, mesh, uniform_field_A(mesh, float(g["b"])), terminals=terms,
                     currents=[{"source": c, "drain": -c} for c in (cur, 0.5 * cur)])
    _assert_sub_stats(sols[0], 1)
    n_sim = int((g["call_time"] == 0).nonzero()[0][-1])
    _assert_like_fixture(g, sols[0], 1e-9, n_sim=n_sim)


def test_transport_strip_two_levels(two_levels):
    g = load_golden("traj_transport_strip")
    mesh = reference_mesh(load_golden("mesh_strip"))
    terms = [edge_terminal(mesh, "source", -30.0), edge_terminal(mesh, "drain", 30.0)]
    cur = float(g["current"])
    sols = _ensemble(g, mesh, uniform_field_A(mesh, float(g["b"])), terminals=terms,
                     currents=[{"source": c, "drain": -c} for c in (0.5 * cur, cur)])
    _assert_sub_stats(sols[1], 2)
    n_sim = int((g["call_time"] == 0).nonzero()[0][-1])
    _assert_like_fixture(g, sols[1], 1e-9, n_sim=n_sim)


def test_field_small_one_level(one_level):
    _field_small(1)


def test_field_small_two_levels(two_levels):
    _field_small(2)


def _field_small(levels):
    g = load_golden("traj_field_small")
    mesh = reference_mesh(load_golden("mesh_small"))
    b = float(g["b"])
    sols = _ensemble(g, mesh, [uniform_field_A(mesh, f) for f in (0.35, b, 0.0)])
    _assert_sub_stats(sols[1], levels)
    _assert_like_fixture(g, sols[1], 5e-8)


def _assert_like_single(ens, one, tol, levels, dt_tol, phases=True):
    """A replica of an ensemble against tdgl.solve of that replica alone (tests/test_hip_ensemble_dynamic.py)."""
    _assert_sub_stats(ens, levels)
    assert ens.stats["steps_thermalizing"] == one.stats["steps_thermalizing"]
    assert ens.stats["steps_simulating"] == one.stats["steps_simulating"]
    a, b = ens.dynamics, one.dynamics
    assert len(a.dt) == len(b.dt)
    assert max_abs(a.dt, b.dt) <= dt_tol * b.dt.max()
    assert max_abs(a.time, b.time) <= dt_tol * max(1.0, b.time.max())
    assert [s.step for s in ens.saved_steps] == [s.step for s in one.saved_steps]
    x, y = ens.tdgl_data, one.tdgl_data
    scale = max(1.0, np.abs(remove_mean(y.mu)).max())
    print(f"\nvs tdgl.solve: dt {max_abs(a.dt, b.dt) / b.dt.max():.3g}, |psi|^2 {max_abs(np.abs(x.psi) ** 2, np.abs(y.psi) ** 2):.3g}")
    assert max_abs(np.abs(x.psi) ** 2, np.abs(y.psi) ** 2) < tol
    assert max_abs(remove_mean(x.mu), remove_mean(y.mu)) < tol * scale
    assert max_abs(x.supercurrent, y.supercurrent) < tol * max(1.0, np.abs(y.supercurrent).max())
    assert max_abs(x.normal_current, y.normal_current) < tol * max(1.0, np.abs(y.normal_current).max())
    if b.mu is not None and b.mu.shape[0] > 1:
        assert max_abs(a.mu[0] - a.mu[1], b.mu[0] - b.mu[1]) < tol * max(scale, np.abs(b.mu[0] - b.mu[1]).max())
        if phases:
            assert max_abs(np.exp(1j * (a.theta[0] - a.theta[1])), np.exp(1j * (b.theta[0] - b.theta[1]))) < tol


def _device(L, W, h, terminals):
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box

    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    film = tdgl.Polygon("film", points=box(L, W))
    terms = [tdgl.Polygon("source", points=box(0.02, W, center=(-L / 2, 0))),
             tdgl.Polygon("drain", points=box(0.02, W, center=(L / 2, 0)))] if terminals else []
    device = tdgl.Device("d", layer=layer, film=film, terminals=terms,
                         probe_points=[(-L / 4, 0), (L / 4, 0)] if terminals else None, length_units="um")
    device.make_mesh(max_edge_length=h)
    return device


@pytest.mark.parametrize("shape, levels", [((8, 8, 0.068, False), 1), ((16, 4, 0.048, True), 2)])
def test_product_sizes_against_single_runs(shape, levels, direct_solve):
    """R = 4 with the product's choices: a ~20k-site film (one level) and a ~40k-site strip with terminals and probes
    (two levels, the first as symmetric tiles); static, LinearRamp x field and TabulatedCurrents replicas."""
    import tdgl_amd as tdgl
    from tdgl_amd.ensemble import ensemble_mu_path
    from tdgl_amd.parameter import TabulatedCurrents

    device = _device(*shape)
    n = len(device.mesh.sites)
    assert ensemble_mu_path(n) == levels and 18_000 < n < 45_000
    opts = tdgl.SolverOptions(solve_time=1, skip_time=0.25, field_units="mT", current_units="uA", save_every=40)
    # (fields of b = B / Bc2 ~ 0.1 - 0.25, Bc2 = 1.3 T here: on weak-field runs tdgl.solve's own direct and iterative mu
    # solves part within a few tens of steps, tests/test_hip_ensemble.py; currents below the phase-slip regime)
    ramp = tdgl.LinearRamp(tmin=0, tmax=0.75) * tdgl.ConstantField(300.0, field_units="mT", length_units="um")
    fields = [150.0, ramp, 200.0, 250.0]
    if shape[3]:
        table = TabulatedCurrents([0.0, 0.5, 1e9], dict(source=[0.0, 3.0, 3.0], drain=[0.0, -3.0, -3.0]))
        currents = [dict(source=2.0, drain=-2.0), None, table, None]
    else:
        currents = [None] * 4
    sols = tdgl.solve_ensemble(device, opts, applied_vector_potential=fields, terminal_currents=currents)
    if levels == 2:
        assert sols[0].stats["mu_levels"] == 2
    for r in range(4):
        one = tdgl.solve(device, opts, applied_vector_potential=fields[r], terminal_currents=currents[r])
        # (the factors' products sum in another order than the single run's kernels; vortex dynamics over ~10^3 steps
        # carry that to 1e-9 - 1e-8 in psi, as on the dense path -- tools/bench_ensemble.py's max_dev_* fields --, and the
        # adaptive dt, which follows the largest change of |psi|^2 anywhere, to ~1e-6.  The probes' phases are not
        # compared: at these fields vortex cores pass the probes, where the phase is undefined.)
        _assert_like_single(sols[r], one, 1e-7, levels, dt_tol=1e-5, phases=False)


def test_equal_inputs_in_different_groups_are_bit_identical(two_levels):
    """R = 33: replicas 3 and 20 (groups 0 and 2 of 8, 0 and 1 of the 16 of the top separator's product) have equal
    inputs."""
    g = load_golden("traj_field_small")
    mesh = reference_mesh(load_golden("mesh_small"))
    fields = [0.35 + 0.45 * k / 32 for k in range(33)]
    fields[20] = fields[3]
    sols = _ensemble(g, mesh, [uniform_field_A(mesh, f) for f in fields])
    _assert_sub_stats(sols[3], 2)
    assert np.array_equal(sols[3].dynamics.dt, sols[20].dynamics.dt)
    assert np.array_equal(sols[3].tdgl_data.psi, sols[20].tdgl_data.psi)
    assert np.array_equal(sols[3].tdgl_data.mu, sols[20].tdgl_data.mu)
    assert not np.array_equal(sols[3].tdgl_data.psi, sols[4].tdgl_data.psi)
