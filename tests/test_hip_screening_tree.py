"""The screening treecode on the device (``screening_method="tree"``, csrc/screening_tree.inc): against the all-pairs
kernel on the same context and against its NumPy model (tests/bltc_model.py), determinism, refusals, whole screening
runs and the reference's screening physics through the public API."""

import numpy as np
import pytest

from helpers import max_abs, synthetic_mesh

pytestmark = pytest.mark.gpu

TARGET = 1e-8


def _defaults():
    from tdgl_amd import SolverOptions

    o = SolverOptions(solve_time=1.0)
    return o.screening_tree_degree, o.screening_tree_theta


def _edge_current(mesh, kind, seed=7):
    """Random edge currents, or the edge projection of a smooth sheet current (a sinusoid plus an offset)."""
    em = mesh.edge_mesh
    if kind == "random":
        return np.random.default_rng(seed).standard_normal(len(em.edges))
    c = em.centers
    unit = em.directions / np.linalg.norm(em.directions, axis=1)[:, None]
    lx, ly = np.ptp(c[:, 0]), np.ptp(c[:, 1])
    F = np.column_stack([np.sin(2 * np.pi * c[:, 1] / ly) + 0.3, np.cos(2 * np.pi * c[:, 0] / lx) - 0.2])
    return (F * unit).sum(axis=1)


def _errors(mesh, areas, K, A_tree, A_direct, n_rows=1500):
    """max |dA| / max |A| over all edges, and max |dA|_e / (sum_j |w_j| / r_ej) on sampled edges."""
    from bltc_model import direct_sum, site_weights

    rows = np.random.default_rng(1).choice(len(A_direct), min(n_rows, len(A_direct)), replace=False)
    _, S = direct_sum(mesh.sites, mesh.edge_mesh.centers, site_weights(mesh, K, areas), rows)
    return (np.abs(A_tree - A_direct).max() / np.abs(A_direct).max(),
            (np.abs(A_tree[rows] - A_direct[rows]) / S).max())


def _strip_with_hole():
    from test_screening_tree_host import strip_with_hole

    return strip_with_hole()


@pytest.fixture(scope="module")
def mesh12k():
    return synthetic_mesh(100)


def test_tree_matches_the_all_pairs_kernel_and_the_model(mesh12k):
    from bltc_model import Treecode, site_weights
    from tdgl_amd.hipcore import TDGLContext

    p, theta = _defaults()
    mesh = mesh12k
    areas = 0.03 * mesh.areas
    ctx = TDGLContext(mesh)
    try:
        ctx.set_screening(mesh.sites, mesh.edge_mesh.centers, areas)
        assert ctx.screening_tree_stats()["clusters"] == 0
        K = {kind: _edge_current(mesh, kind) for kind in ("random", "smooth")}
        A_dir = {kind: ctx.evaluate_induced_vector_potential(k) for kind, k in K.items()}
        ctx.set_screening_tree(p, theta)
        model = Treecode(mesh.sites, mesh.edge_mesh.centers, p, theta)
        st = ctx.screening_tree_stats()
        assert st == dict(model.stats(), setup_us=st["setup_us"])  # the same trees and interaction lists
        for kind, k in K.items():
            A = ctx.evaluate_induced_vector_potential(k)
            err_max, err_sum = _errors(mesh, areas, k, A, A_dir[kind])
            assert (err_max if kind == "smooth" else err_sum) <= TARGET, (kind, err_max, err_sum)
            want = model.evaluate(site_weights(mesh, k, areas))
            assert max_abs(A, want) <= 1e-12 * np.abs(want).max(), kind  # the kernels run the stated algorithm
    finally:
        ctx.close()


@pytest.mark.parametrize("which", ["film_120k", "strip_with_hole"])
def test_tree_matches_the_all_pairs_kernel_on_larger_meshes(which):
    from tdgl_amd.hipcore import TDGLContext

    mesh = synthetic_mesh(320) if which == "film_120k" else _strip_with_hole()
    if which == "film_120k":
        assert len(mesh.sites) > 110_000
    areas = 0.03 * mesh.areas
    ctx = TDGLContext(mesh)
    try:
        ctx.set_screening(mesh.sites, mesh.edge_mesh.centers, areas)
        K = {kind: _edge_current(mesh, kind) for kind in ("random", "smooth")}
        A_dir = {kind: ctx.evaluate_induced_vector_potential(k) for kind, k in K.items()}
        ctx.set_screening_tree(*_defaults())
        for kind, k in K.items():
            err_max, err_sum = _errors(mesh, areas, k, ctx.evaluate_induced_vector_potential(k), A_dir[kind])
            assert (err_max if kind == "smooth" else err_sum) <= TARGET, (which, kind, err_max, err_sum)
    finally:
        ctx.close()


def test_tree_is_deterministic_and_refusals_keep_the_method(mesh12k):
    from tdgl_amd.hipcore import TDGLContext

    mesh = mesh12k
    ctx = TDGLContext(mesh)
    try:
        with pytest.raises(RuntimeError, match="call tdgl_set_screening first"):
            ctx.set_screening_tree(8, 0.6)
        ctx.set_screening(mesh.sites, mesh.edge_mesh.centers, 0.03 * mesh.areas)
        K = _edge_current(mesh, "random")
        A_dir = ctx.evaluate_induced_vector_potential(K)
        for bad in [(1, 0.6), (8, 1.5), (17, 0.5), (8, 0.0)]:  # refused with the all-pairs kernel active
            with pytest.raises(ValueError):
                ctx.set_screening_tree(*bad)
            assert np.array_equal(ctx.evaluate_induced_vector_potential(K), A_dir)
        ctx.set_screening_tree(*_defaults())
        A1 = ctx.evaluate_induced_vector_potential(K)
        A2 = ctx.evaluate_induced_vector_potential(K)
        assert np.array_equal(A1, A2)
        assert not np.array_equal(A1, A_dir)
        stats = ctx.screening_tree_stats()
        for bad in [(1, 0.6), (8, 1.5)]:  # refused with the tree active: the tree stays
            with pytest.raises(ValueError, match=r"screening_tree_(degree|theta) must be in"):
                ctx.set_screening_tree(*bad)
            assert np.array_equal(ctx.evaluate_induced_vector_potential(K), A1)
            assert ctx.screening_tree_stats() == stats
        ctx.set_screening_tree(0, 0.0)
        assert np.array_equal(ctx.evaluate_induced_vector_potential(K), A_dir)
        assert ctx.screening_tree_stats()["clusters"] == 0
    finally:
        ctx.close()


def _screening_device(width, height, xi=0.1):
    """The film of the reference's screening test (tdgl/test/test_solve.py:152-196), of the given size in um."""
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box

    layer = tdgl.Layer(coherence_length=xi, london_lambda=0.075, thickness=0.05)
    device = tdgl.Device("bar", layer=layer, film=tdgl.Polygon("film", points=box(width, height, points=301)),
                         length_units="um")
    device.make_mesh(max_edge_length=xi / 3, smooth=100)
    return device


def test_whole_screening_run_with_the_tree_follows_the_direct_one():
    """20 steps of fixed dt with screening to 1e-6 on a ~20k-site film, all-pairs against treecode."""
    import tdgl_amd as tdgl

    device = _screening_device(5.6, 2.8)
    assert len(device.mesh.sites) > 15_000
    runs = {}
    for method in ("direct", "tree"):
        options = tdgl.SolverOptions(solve_time=20e-5, dt_init=1e-5, dt_max=1e-5, adaptive=False, field_units="mT",
                                     save_every=1000, include_screening=True, screening_tolerance=1e-6,
                                     screening_method=method)
        runs[method] = tdgl.solve(device, options, applied_vector_potential=0.1)
    d, t = runs["direct"], runs["tree"]
    it_d, it_t = d.dynamics.screening_iterations, t.dynamics.screening_iterations
    assert len(it_d) >= 20 and np.array_equal(it_d, it_t), (it_d, it_t)
    assert it_d.max() > 1
    a_d, a_t = d.tdgl_data.induced_vector_potential, t.tdgl_data.induced_vector_potential
    assert np.abs(a_d).max() > 1e-3  # the run really screens
    assert max_abs(t.tdgl_data.psi, d.tdgl_data.psi) < 1e-7
    assert max_abs(t.tdgl_data.mu, d.tdgl_data.mu) < 1e-7
    assert max_abs(a_t, a_d) < 1e-7


def test_screening_restores_fluxoid_quantisation_with_the_tree():
    """test_screening_restores_fluxoid_quantisation (tests/test_hip_api.py) with screening_method="tree"."""
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box, circle

    device = _screening_device(2, 1)
    curves = [circle(0.25, center=(0, 0)), circle(0.1, center=(0.15, 0.25)), circle(0.3, center=(0.6, -0.1)),
              box(0.5, center=(-0.5, 0)), box(0.5, center=(-0.6, -0.2))]
    options = tdgl.SolverOptions(solve_time=2, field_units="mT", current_units="uA", include_screening=False)
    bare = tdgl.solve(device, options, applied_vector_potential=0.1)
    k_bare = np.linalg.norm(bare.current_density, axis=1).max()
    options.include_screening = True
    options.screening_tolerance = 1e-6
    options.dt_max = 1e-3
    options.screening_method = "tree"
    screened = tdgl.solve(device, options, applied_vector_potential=0.1)
    k_scr = np.linalg.norm(screened.current_density, axis=1).max()
    errors = []
    for curve in curves:
        fluxoid = screened.polygon_fluxoid(curve)
        errors.append(abs(sum(fluxoid).magnitude / fluxoid.flux_part.magnitude))
    assert max(errors) < 5e-2, errors
    assert np.isclose(k_scr / k_bare, 270 / 450, rtol=0.05), (k_bare, k_scr)


def test_one_million_sites(capsys):
    from tdgl_amd.hipcore import TDGLContext

    mesh = synthetic_mesh(920)
    assert len(mesh.sites) > 900_000
    areas = 0.03 * mesh.areas
    ctx = TDGLContext(mesh)
    try:
        ctx.set_screening(mesh.sites, mesh.edge_mesh.centers, areas)
        K = _edge_current(mesh, "smooth")
        A_dir = ctx.evaluate_induced_vector_potential(K)  # ~1.3 s
        ctx.set_screening_tree(*_defaults())
        A = ctx.evaluate_induced_vector_potential(K)
        st = ctx.screening_tree_stats()
        m = len(mesh.edge_mesh.edges)
        with capsys.disabled():
            print(f"\n1M-site treecode: {len(mesh.sites)} sites, {m} edges, {st}; pairs per target: far "
                  f"{st['far_pairs'] / m:.0f}, near {st['near_pairs'] / m:.0f} (all-pairs {len(mesh.sites)})")
        err = np.abs(A - A_dir).max() / np.abs(A_dir).max()
        assert err <= TARGET, err
        assert st["far_pairs"] + st["near_pairs"] < 0.02 * m * len(mesh.sites)
    finally:
        ctx.close()
