"""Fields of the sheet currents, the parts that need no GPU: the host backend against the reference's own
Biot-Savart loops (fixture `fields_reference_small`, tests/golden/generate_golden_fields.py), the ``backend`` keyword
of the `Solution` methods, and the C symbols of the device evaluator.  The yardstick of every comparison is derived in
tests/fields_model.py."""

import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import load_golden
from fields_model import assert_within_yardstick, host_sums


def sheet_solution(src_xy, areas, z0, Ks, Kn):
    """A Solution over bare sites (no mesh): what `field_at_position` / `vector_potential_at_position` read of a
    device, with the site current densities given directly."""
    import tdgl_amd as tdgl
    from tdgl_amd.solution import Solution, TDGLData

    class Given(Solution):
        supercurrent_density = property(lambda self: Ks)
        normal_current_density = property(lambda self: Kn)

    n = len(src_xy)
    device = SimpleNamespace(
        points=src_xy, mesh=SimpleNamespace(areas=areas), coherence_length=1.0, layer=SimpleNamespace(z0=z0),
        film=SimpleNamespace(contains_points=lambda p: np.zeros(len(p), dtype=bool)), length_units="um")
    step = TDGLData(step=0, time=0.0, dt=0.0, psi=np.ones(n, dtype=complex), mu=np.zeros(n), supercurrent=np.zeros(0),
                    normal_current=np.zeros(0))
    opts = tdgl.SolverOptions(solve_time=1.0, field_units="mT", current_units="uA")
    return Given(device=device, options=opts, saved_steps=[step], applied_vector_potential=0.0)


def field_prefactor():
    """mu_0 / 4 pi in mT per (uA / um): what `field_at_position` multiplies the bare sums with."""
    from tdgl_amd.device import CURRENT_UNITS, FIELD_UNITS, LENGTH_UNITS, MU_0

    return MU_0 / (4 * np.pi) * (CURRENT_UNITS["uA"] / LENGTH_UNITS["um"]) / FIELD_UNITS["mT"]


def reference_sums(g):
    """The fixture's outputs as bare sums: divided by the reference's own mu_0 / 4 pi."""
    pref = float(g["mu_0"]) / (4 * np.pi)
    return g["B_vector"] / pref, g["B_z"] / pref


def test_host_backend_reproduces_the_reference_fixture():
    g = load_golden("fields_reference_small")
    n = len(g["src_xy"])
    assert n == 500 and len(g["targets"]) == 64
    want_vec, want_z = reference_sums(g)
    model = host_sums(g["src_xy"], g["areas"], float(g["z0"]), g["K"], g["targets"])
    # the model (and with it the sums of magnitudes every other test uses) against the reference
    assert_within_yardstick(model["Z"][0], want_z, model["Z_abs"][0], n, "model B_z vs reference")
    assert_within_yardstick(model["Z"][0], want_vec[:, 2], model["Z_abs"][0], n, "model B_z vs reference vector loop")
    assert_within_yardstick(model["XY"][0], want_vec[:, :2], model["XY_abs"][0], n, "model B_xy vs reference")
    # the host backend of the Solution methods
    zero = np.zeros_like(g["K"])
    sol = sheet_solution(g["src_xy"], g["areas"], float(g["z0"]), g["K"], zero)
    pref = field_prefactor()
    got = sol.field_at_position(g["targets"], vector=True, with_units=False, return_sum=False, backend="host")
    assert np.all(got.normal_current == 0)
    assert_within_yardstick(got.supercurrent[:, 2] / pref, want_z, model["Z_abs"][0], n, "host B_z vs reference")
    assert_within_yardstick(got.supercurrent[:, :2] / pref, want_vec[:, :2], model["XY_abs"][0], n, "host B_xy vs reference")
    got_z = sol.field_at_position(g["targets"][:, :2], zs=g["targets"][:, 2].copy(), with_units=False, backend="host")
    assert_within_yardstick(got_z / pref, want_z, model["Z_abs"][0], n, "host B_z (vector=False) vs reference")


def _annulus_device(pitch=0.12):
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box, circle

    layer = tdgl.Layer(coherence_length=0.2, london_lambda=0.3, thickness=0.05)
    film = tdgl.Polygon("film", points=box(3.0, 2.0, points=161))
    hole = tdgl.Polygon("hole", points=circle(0.4, points=41, center=(0.5, 0.1)))
    device = tdgl.Device("plate", layer=layer, film=film, holes=[hole], length_units="um")
    device.make_mesh(max_edge_length=pitch)
    return device


def _fake_solution(device, Ks, Kn, psi, applied=0.0, **options):
    """A Solution whose site current densities are given directly (no solver run)."""
    import tdgl_amd as tdgl
    from tdgl_amd.solution import Solution, TDGLData

    class Given(Solution):
        supercurrent_density = property(lambda self: Ks)
        normal_current_density = property(lambda self: Kn)

    m = len(device.mesh.edge_mesh.edges)
    step = TDGLData(step=0, time=0.0, dt=0.0, psi=psi, mu=np.zeros(len(psi)), supercurrent=np.zeros(m),
                    normal_current=np.zeros(m))
    opts = tdgl.SolverOptions(solve_time=1.0, field_units="mT", current_units="uA", **options)
    return Given(device=device, options=opts, saved_steps=[step], applied_vector_potential=applied)


@pytest.fixture(scope="module")
def annulus_state():
    """The annulus of tests/test_host_logic.py with a rigid rotation as supercurrent and a random normal current."""
    from tdgl_amd.geometry import circle

    device = _annulus_device()
    n = len(device.points)
    r = device.points - (device.points * device.mesh.areas[:, None]).sum(0) / device.mesh.areas.sum()
    Ks = 2.0 * np.stack([-r[:, 1], r[:, 0]], axis=1)
    Kn = np.random.default_rng(5).normal(size=(n, 2))
    sol = _fake_solution(device, Ks, Kn, 0.8 * np.ones(n, dtype=complex), applied=0.3)
    rng = np.random.default_rng(6)
    positions = rng.uniform([-2.0, -1.5], [2.0, 1.5], size=(40, 2))
    ring = circle(0.5, points=101, center=(-0.7, -0.2))
    return sol, positions, ring


def _same_bits(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same_bits(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_host_backend_is_the_default_bit_for_bit(annulus_state):
    sol, positions, ring = annulus_state
    for kw in (dict(zs=0.7), dict(zs=0.7, vector=True), dict(zs=0.7, vector=True, return_sum=False),
               dict(zs=np.linspace(0.2, 3.0, len(positions)), with_units=False)):
        assert _same_bits(sol.field_at_position(positions, **kw), sol.field_at_position(positions, backend="host", **kw))
    for kw in (dict(zs=0.7), dict(zs=0.0, return_sum=False, with_units=False)):
        assert _same_bits(sol.vector_potential_at_position(positions, **kw),
                          sol.vector_potential_at_position(positions, backend="host", **kw))
    assert _same_bits(tuple(sol.polygon_fluxoid(ring)), tuple(sol.polygon_fluxoid(ring, backend="host")))
    with_units = sol.polygon_fluxoid(ring, backend="host")
    assert with_units.flux_part.units == "Phi_0" and np.isfinite(with_units.flux_part.magnitude)


def test_unknown_backend_is_refused(annulus_state):
    sol, positions, ring = annulus_state
    for call in (lambda: sol.field_at_position(positions, zs=0.7, backend="nonsense"),
                 lambda: sol.vector_potential_at_position(positions, zs=0.7, backend="nonsense"),
                 lambda: sol.polygon_fluxoid(ring, backend="nonsense")):
        with pytest.raises(ValueError, match=r"host.*hip"):
            call()


def test_hip_backend_without_a_gpu_says_so(annulus_state):
    import tdgl_amd as tdgl
    from tdgl_amd import _lib

    if _lib.load().tdgl_device_count() > 0:
        pytest.skip("a GPU is visible: the hip backend runs (tests/test_hip_fields.py)")
    sol, positions, ring = annulus_state
    for call in (lambda: sol.field_at_position(positions, zs=0.7, backend="hip"),
                 lambda: sol.vector_potential_at_position(positions, zs=0.7, backend="hip"),
                 lambda: sol.polygon_fluxoid(ring, backend="hip"),
                 lambda: tdgl.FieldEvaluator(sol.device, positions, zs=0.7)):
        with pytest.raises(RuntimeError, match="tdgl_device_count"):
            call()
    # the checks that both backends share come first
    with pytest.raises(ValueError, match="within a film"):
        sol.field_at_position(np.array([[0.0, 0.0]]), zs=0.0, backend="hip")


def test_field_plan_symbols_are_declared_and_resolve():
    from tdgl_amd import _lib

    names = ["tdgl_field_plan_create", "tdgl_field_plan_destroy", "tdgl_field_plan_eval", "tdgl_field_plan_stats"]
    lib = _lib.load()
    for name in names:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    # argument errors are reported before any device work, through the global tdgl_last_error(NULL)
    plan = C.c_void_p()
    status = lib.tdgl_field_plan_create(C.byref(plan), 0, 0, None, None, 0.0, 1, None)
    assert status == _lib.TDGL_ERR_ARG and not plan.value
    assert b"null array" in lib.tdgl_last_error(None)
    one = np.zeros(3)
    status = lib.tdgl_field_plan_create(C.byref(plan), 0, 0, _lib.p_f64(one), _lib.p_f64(one), 0.0, 1, _lib.p_f64(one))
    assert status == _lib.TDGL_ERR_ARG and b"n must be >= 1" in lib.tdgl_last_error(None)
    bad = np.array([np.nan, 0.0, 0.0])
    status = lib.tdgl_field_plan_create(C.byref(plan), 0, 1, _lib.p_f64(one), _lib.p_f64(one), 0.0, 1, _lib.p_f64(bad))
    assert status == _lib.TDGL_ERR_ARG and b"finite" in lib.tdgl_last_error(None)
    assert lib.tdgl_field_plan_eval(None, 1, None, 1, None, None, None) == _lib.TDGL_ERR_ARG
