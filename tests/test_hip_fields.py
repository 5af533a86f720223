"""Fields of the sheet currents on the device (csrc/fields.inc, `hipcore.FieldPlan`, `tdgl_amd.FieldEvaluator`,
``backend="hip"`` of the `Solution` methods) against the host formulas.  Every comparison uses the yardstick derived
in tests/fields_model.py: |got - want| <= (n + 16) 2^-53 sum|t| per target and component, `want` and `sum|t|` from
chunked float64 NumPy."""

from types import SimpleNamespace

import numpy as np
import pytest

from conftest import load_golden
from fields_model import U, assert_within_yardstick, host_sums, yardstick

pytestmark = pytest.mark.gpu


def random_sheet(n, m, seed):
    rng = np.random.default_rng(seed)
    z0 = -0.2
    src = rng.uniform([-5.0, -3.0], [5.0, 3.0], size=(n, 2))
    areas = rng.uniform(0.5, 1.5, size=n) * 60.0 / n
    K = rng.normal(size=(2, n, 2))
    tgt = np.column_stack([rng.uniform(-7.0, 7.0, m), rng.uniform(-5.0, 5.0, m),
                           z0 + rng.choice([-1.0, 1.0], m) * np.exp(rng.uniform(np.log(1e-2), np.log(30.0), m))])
    tgt[::7, 2] = z0  # some in the plane of the sheet (random, so never on a source)
    return src, areas, z0, K, tgt


def compare_with_model(got, model, what, f_count, n, label):
    S_A, S_z, S_xy = got
    worst = 0.0
    if what & 1:
        assert S_A.shape == (f_count, model["A"].shape[1], 2)
        worst = max(worst, assert_within_yardstick(S_A, model["A"][:f_count], model["A_abs"][:f_count], n, label + " A"))
    else:
        assert S_A is None
    if what & 2:
        worst = max(worst, assert_within_yardstick(S_z, model["Z"][:f_count], model["Z_abs"][:f_count], n, label + " B_z"))
    else:
        assert S_z is None
    if what & 4:
        worst = max(worst, assert_within_yardstick(S_xy, model["XY"][:f_count], model["XY_abs"][:f_count], n, label + " B_xy"))
    else:
        assert S_xy is None
    return worst


@pytest.mark.parametrize("m", [1, 255, 1000])
@pytest.mark.parametrize("n", [1, 63, 257, 70_001])
def test_plan_against_host_sums(n, m):
    """Every non-zero `what`, one and two current fields; outputs not asked for stay untouched; two calls give the
    same bits.  (n = 1, 63, 257: tiles that are mostly, partly and barely padding.)"""
    from tdgl_amd import _lib
    from tdgl_amd.hipcore import FieldPlan

    src, areas, z0, K, tgt = random_sheet(n, m, seed=1000 * n + m)
    model = host_sums(src, areas, z0, K, tgt)
    lib = _lib.load()
    with FieldPlan(src, areas, z0, tgt) as plan:
        for nf in (1, 2):
            for what in range(1, 8):
                got = plan.eval(K[:nf], what)
                compare_with_model(got, model, what, nf, n, f"n={n} m={m} nf={nf} what={what}")
                for a in got:
                    assert a is None or np.isfinite(a).all()
                again = plan.eval(K[:nf], what)
                for a, b in zip(got, again):
                    assert (a is None and b is None) or a.tobytes() == b.tobytes()
                # through the C ABI with buffers for everything: what was not asked for is not written
                sentinel = -12345.678
                bufs = [np.full((nf, m, 2), sentinel), np.full((nf, m), sentinel), np.full((nf, m, 2), sentinel)]
                Kc = np.ascontiguousarray(K[:nf])
                status = lib.tdgl_field_plan_eval(plan._plan, nf, _lib.p_f64(Kc), what, *[_lib.p_f64(b) for b in bufs])
                assert status == _lib.TDGL_OK
                for bit, buf, ref in zip((1, 2, 4), bufs, got):
                    if what & bit:
                        assert buf.tobytes() == ref.tobytes()
                    else:
                        assert np.all(buf == sentinel)
        st = plan.stats()
        assert st["pairs"] == n * m and st["launches"] == st["target_batches"] == 1 and st["source_chunks"] >= 1
        assert st["last_ms"] > 0


def test_plan_reproduces_the_reference_fixture():
    from tdgl_amd.hipcore import FieldPlan

    g = load_golden("fields_reference_small")
    n = len(g["src_xy"])
    pref = float(g["mu_0"]) / (4 * np.pi)
    model = host_sums(g["src_xy"], g["areas"], float(g["z0"]), g["K"], g["targets"])
    with FieldPlan(g["src_xy"], g["areas"], float(g["z0"]), g["targets"]) as plan:
        _, S_z, S_xy = plan.eval(g["K"], 6)
        _, S_z_alone, _ = plan.eval(g["K"], 2)
    for z in (S_z[0], S_z_alone[0]):
        assert_within_yardstick(z, g["B_z"] / pref, model["Z_abs"][0], n, "plan B_z vs reference")
        assert_within_yardstick(z, g["B_vector"][:, 2] / pref, model["Z_abs"][0], n, "plan B_z vs reference vector loop")
    assert_within_yardstick(S_xy[0], g["B_vector"][:, :2] / pref, model["XY_abs"][0], n, "plan B_xy vs reference")


def test_argument_errors_leave_the_plan_usable():
    from tdgl_amd import _lib
    from tdgl_amd.hipcore import FieldPlan

    src, areas, z0, K, tgt = random_sheet(300, 40, seed=3)
    lib = _lib.load()
    with FieldPlan(src, areas, z0, tgt) as plan:
        before = plan.eval(K, 7)
        with pytest.raises(ValueError, match="n_fields must be 1 or 2"):
            plan.eval(np.zeros((3, 300, 2)), 7)
        for what in (0, 8, -1):
            with pytest.raises(ValueError, match="what must be"):
                plan.eval(K, what)
        with pytest.raises(ValueError, match="Expected currents"):
            plan.eval(K[:, :10], 7)
        assert lib.tdgl_field_plan_eval(plan._plan, 2, None, 7, None, None, None) == _lib.TDGL_ERR_ARG
        assert b"null current array" in lib.tdgl_last_error(None)
        Kc = np.ascontiguousarray(K)
        assert lib.tdgl_field_plan_eval(plan._plan, 2, _lib.p_f64(Kc), 2, None, None, None) == _lib.TDGL_ERR_ARG
        assert b"null output" in lib.tdgl_last_error(None)
        after = plan.eval(K, 7)
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
    with pytest.raises(RuntimeError, match="closed"):
        plan.eval(K, 7)
    bad = tgt.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        FieldPlan(src, areas, z0, bad)
    bad[3, 1] = 2e100  # beyond the bound that keeps every squared distance finite
    with pytest.raises(ValueError, match="within"):
        FieldPlan(src, areas, z0, bad)
    bad_src = src.copy()
    bad_src[0, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        FieldPlan(bad_src, areas, z0, tgt)
    with pytest.raises(ValueError, match="m must be >= 1"):
        FieldPlan(src, areas, z0, np.zeros((0, 3)))
    with pytest.raises(ValueError, match="no HIP device"):
        FieldPlan(src, areas, z0, tgt, device_id=4096)


def test_padding_never_meets_an_infinity_at_the_largest_coordinates():
    """Three sources (253 padding rows in the tile) and targets at the edge of the accepted coordinate range: the
    squared distances to the padding at 1e150 stay finite, so zero weights never multiply an infinity."""
    from tdgl_amd.hipcore import FieldPlan

    s = 1e100
    src = np.array([[-s, -s], [s, 0.5 * s], [0.0, 0.0]])
    areas = np.array([1.0, 2.0, 3.0])
    K = np.array([[[1.0, -2.0], [0.5, 0.25], [-1.0, 1.0]]])
    tgt = np.array([[s, s, s], [-s, s, -s], [0.3 * s, -0.2 * s, 0.0], [s, -s, 1.0]])
    model = host_sums(src, areas, 0.0, K, tgt)
    with FieldPlan(src, areas, 0.0, tgt) as plan:
        got = plan.eval(K, 7)
    for a in got:
        assert np.isfinite(a).all()
    compare_with_model(got, model, 7, 1, 3, "coordinates of 1e100")


def test_coincident_target_and_site():
    from tdgl_amd.hipcore import FieldPlan

    src, areas, z0, K, tgt = random_sheet(300, 65, seed=9)
    hit = 17
    tgt[hit] = [src[41, 0], src[41, 1], z0]
    model = host_sums(src, areas, z0, K, tgt)
    assert not np.isfinite(model["A"][:, hit]).any()
    with FieldPlan(src, areas, z0, tgt) as plan:
        S_A, S_z, S_xy = plan.eval(K, 7)
    assert not np.isfinite(S_A[:, hit]).any() and not np.isfinite(S_z[:, hit]).any()
    assert not np.isfinite(S_xy[:, hit]).any()
    others = np.arange(len(tgt)) != hit
    assert np.isfinite(S_A[:, others]).all() and np.isfinite(S_z[:, others]).all() and np.isfinite(S_xy[:, others]).all()
    for got, key in ((S_A, "A"), (S_z, "Z"), (S_xy, "XY")):
        assert_within_yardstick(got[:, others], model[key][:, others], model[key + "_abs"][:, others], 300,
                                "neighbours of a coincident pair " + key)


# ---------------------------------------------------------------------------------------------------------------
def unit_factors(sol):
    from tdgl_amd.device import CURRENT_UNITS, FIELD_UNITS, LENGTH_UNITS, MU_0

    length = LENGTH_UNITS[sol.device.length_units]
    b = MU_0 / (4 * np.pi) * (CURRENT_UNITS[sol.current_units] / length) / FIELD_UNITS[sol.field_units]
    a = MU_0 / (4 * np.pi) * CURRENT_UNITS[sol.current_units] / (FIELD_UNITS[sol.field_units] * length)
    return a, b


def solution_model(sol, positions, zs):
    dev = sol.device
    K = np.stack([sol.supercurrent_density, sol.normal_current_density])
    tgt = np.column_stack([positions, zs * np.ones(len(positions))])
    return host_sums(dev.points, dev.mesh.areas * dev.coherence_length**2, dev.layer.z0, K, tgt, chunk=32)


def within(got, want, bound, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, label
    err = np.abs(got - want)
    pos = bound > 0
    print(f"{label}: max |hip - host| / bound = {float((err[pos] / bound[pos]).max()) if pos.any() else 0.0:.3e}")
    assert np.all(err <= bound), label


@pytest.fixture(scope="module")
def strip_solution():
    """A short solve of the quick-start strip (examples/quickstart.py): field, transport current, several saved steps."""
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box, circle

    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    film = tdgl.Polygon("film", points=box(6, 3))
    hole = tdgl.Polygon("hole", points=circle(0.6, center=(0.5, 0.2)))
    source = tdgl.Polygon("source", points=box(0.02, 3, center=(-3, 0)))
    drain = tdgl.Polygon("drain", points=box(0.02, 3, center=(3, 0)))
    device = tdgl.Device("strip", layer=layer, film=film, holes=[hole], terminals=[source, drain],
                         probe_points=[(-2, 0), (2, 0)], length_units="um")
    device.make_mesh(max_edge_length=0.12, smooth=2)
    options = tdgl.SolverOptions(solve_time=6, dt_init=1e-3, field_units="mT", current_units="uA", save_every=100)
    solution = tdgl.solve(device, options, applied_vector_potential=0.4, terminal_currents=dict(source=12.0, drain=-12.0))
    assert len(solution.saved_steps) >= 3
    assert np.abs(solution.supercurrent_density).max() > 0 and np.abs(solution.normal_current_density).max() > 0
    return solution


def test_solution_methods_with_the_hip_backend_equal_the_host_backend(strip_solution):
    from tdgl_amd.geometry import box

    sol = strip_solution
    n = len(sol.device.points)
    a_unit, b_unit = unit_factors(sol)
    rng = np.random.default_rng(11)
    m = 70
    pos = rng.uniform([-4.0, -2.5], [4.0, 2.5], size=(m, 2))
    z_arr = sol.device.layer.z0 + rng.choice([-1.0, 1.0], m) * rng.uniform(0.05, 3.0, m)
    for label, args, kw, zs in (("zs scalar", pos, dict(zs=0.8), 0.8 * np.ones(m)), ("zs array", pos, dict(zs=z_arr), z_arr),
                                ("(m, 3) positions", np.column_stack([pos, z_arr]), {}, z_arr)):
        model = solution_model(sol, pos, zs)
        bz = b_unit * yardstick(n, model["Z_abs"])           # [2, m]
        bxy = b_unit * yardstick(n, model["XY_abs"])         # [2, m, 2]
        bvec = np.concatenate([bxy, bz[:, :, None]], axis=2)  # [2, m, 3]
        for vector, bound in ((False, bz), (True, bvec)):
            host = sol.field_at_position(args, vector=vector, return_sum=False, backend="host", **kw)
            hip = sol.field_at_position(args, vector=vector, return_sum=False, backend="hip", **kw)
            assert type(hip) is type(host) and hip.supercurrent.units == host.supercurrent.units == "mT"
            within(hip.supercurrent, host.supercurrent, bound[0], f"field {label} vector={vector} supercurrent")
            within(hip.normal_current, host.normal_current, bound[1], f"field {label} vector={vector} normal current")
            host = sol.field_at_position(args, vector=vector, with_units=False, backend="host", **kw)
            hip = sol.field_at_position(args, vector=vector, with_units=False, backend="hip", **kw)
            assert type(hip) is np.ndarray
            # (adding the two parts rounds once more on each side)
            within(hip, host, bound[0] + bound[1] + 2 * U * np.abs(host), f"field {label} vector={vector} sum")
        ba = a_unit * yardstick(n, model["A_abs"])
        ba = np.concatenate([ba, np.zeros_like(ba[:, :, :1])], axis=2)
        host = sol.vector_potential_at_position(args, return_sum=False, backend="host", **kw)
        hip = sol.vector_potential_at_position(args, return_sum=False, backend="hip", **kw)
        assert set(hip) == set(host) and np.array_equal(hip["applied"], host["applied"])
        assert hip["supercurrent_density"].units == host["supercurrent_density"].units
        within(hip["supercurrent_density"], host["supercurrent_density"], ba[0], f"vector potential {label} supercurrent")
        within(hip["normal_current_density"], host["normal_current_density"], ba[1], f"vector potential {label} normal current")
        host = sol.vector_potential_at_position(args, with_units=False, backend="host", **kw)
        hip = sol.vector_potential_at_position(args, with_units=False, backend="hip", **kw)
        # (the applied part is the same array in both; the two additions round on each side)
        within(hip, host, ba[0] + ba[1] + 4 * U * np.abs(host), f"vector potential {label} sum")
    # fluxoid: the yardstick carried through the line integral, sum over the vertices of |dl| . bound
    from tdgl_amd.device import FIELD_UNITS, LENGTH_UNITS, PHI_0, Polygon

    poly = box(1.6, 1.6, points=121, center=(-1.7, 0.0))
    points = Polygon(points=poly).points
    z0 = sol.device.layer.z0
    model = solution_model(sol, points, z0 * np.ones(len(points)))
    bound_A = a_unit * yardstick(n, model["A_abs"]).sum(axis=0)  # [vertices, 2], both current fields
    dl = np.diff(points, axis=0, prepend=points[:1])
    scale = FIELD_UNITS[sol.field_units] * LENGTH_UNITS[sol.device.length_units] ** 2 / PHI_0
    host = sol.polygon_fluxoid(poly, with_units=False, backend="host")
    hip = sol.polygon_fluxoid(poly, with_units=False, backend="hip")
    bound = float((np.abs(dl) * bound_A).sum()) * scale + 4 * U * abs(host.flux_part)
    print(f"fluxoid: host {host.flux_part!r} hip {hip.flux_part!r} bound {bound:.3e}")
    assert abs(hip.flux_part - host.flux_part) <= bound and hip.supercurrent_part == host.supercurrent_part
    assert host.flux_part != 0.0
    # the shared checks
    for backend in ("host", "hip"):
        with pytest.raises(ValueError, match="Cannot interpolate fields within a film."):
            sol.field_at_position(np.array([[-1.0, 0.3]]), zs=z0, backend=backend)
        with pytest.raises(ValueError, match="zs cannot be specified"):
            sol.field_at_position(np.zeros((2, 3)), zs=1.0, backend=backend)
        with pytest.raises(ValueError, match="completely within"):
            sol.polygon_fluxoid(box(8.0, 1.0), backend=backend)


def test_field_evaluator_over_every_saved_step(strip_solution):
    import tdgl_amd as tdgl

    sol = strip_solution
    gx, gy = np.meshgrid(np.linspace(-3.5, 3.5, 24), np.linspace(-2.0, 2.0, 12))
    pos = np.column_stack([gx.ravel(), gy.ravel()])
    zs = 0.6
    count = len(sol.saved_steps)
    last = sol.solve_step
    try:
        with tdgl.FieldEvaluator(sol.device, pos, zs=zs, device_id=sol.options.device_id, field_units=sol.field_units,
                                 current_units=sol.current_units) as ev:
            movie = []
            for k in range(count):
                sol.load_tdgl_data(k)
                for kw in (dict(vector=True, return_sum=False), dict(vector=False, return_sum=True, with_units=False)):
                    one_shot = sol.field_at_position(pos, zs=zs, backend="hip", **kw)
                    through = ev.field(sol, **kw)
                    from_data = ev.field(sol.saved_steps[k], **kw)
                    for a, b, c in zip(*[x if isinstance(x, tuple) else (x,) for x in (one_shot, through, from_data)]):
                        assert type(a) is type(b) is type(c)
                        assert np.asarray(a).tobytes() == np.asarray(b).tobytes() == np.asarray(c).tobytes()
                movie.append(np.asarray(through))
                one_shot = sol.vector_potential_at_position(pos, zs=zs, return_sum=False, backend="hip")
                through = ev.vector_potential(sol, return_sum=False)
                from_data = ev.vector_potential(sol.saved_steps[k], return_sum=False)
                for name in ("supercurrent_density", "normal_current_density"):
                    assert one_shot[name].tobytes() == through[name].tobytes() == from_data[name].tobytes()
                assert np.array_equal(one_shot["applied"], through["applied"]) and np.all(from_data["applied"] == 0)
                total = ev.vector_potential(sol, with_units=False)
                assert total.tobytes() == sol.vector_potential_at_position(pos, zs=zs, with_units=False, backend="hip").tobytes()
            assert ev.plan.stats()["pairs"] == len(pos) * len(sol.device.points)
        assert any(not np.array_equal(movie[0], frame) for frame in movie[1:])  # the steps differ
        with pytest.raises(TypeError):
            ev.field(np.zeros(3))
    finally:
        sol.load_tdgl_data(last if last >= 0 else count + last)


def test_field_image_above_a_250k_site_film():
    """The size that motivates the device evaluator: a 128 x 128 image of the field 3 xi above a 460 xi square film with a
    rigid rotation as sheet current; 64 of its pixels against chunked host sums, and far above the film the field of the
    dipole `magnetic_moment` reports.  The host backend is never called on the image."""
    import tdgl_amd as tdgl
    from helpers import synthetic_mesh
    from tdgl_amd.device import MU_0
    from tdgl_amd.solution import Solution, TDGLData

    xi = 0.1
    mesh = synthetic_mesh(460)
    n = len(mesh.sites)
    assert 200_000 < n < 300_000
    device = SimpleNamespace(
        mesh=mesh, points=xi * np.asarray(mesh.sites), coherence_length=xi, layer=SimpleNamespace(z0=0.0),
        film=SimpleNamespace(contains_points=lambda p: np.ones(len(p), dtype=bool)), length_units="um")
    com = (mesh.sites * mesh.areas[:, None]).sum(axis=0) / mesh.areas.sum()
    r = xi * (mesh.sites - com[None, :])
    Ks = 2.0 * np.stack([-r[:, 1], r[:, 0]], axis=1)
    Kn = np.zeros_like(Ks)

    class Given(Solution):
        supercurrent_density = property(lambda self: Ks)
        normal_current_density = property(lambda self: Kn)

    step = TDGLData(step=0, time=0.0, dt=0.0, psi=np.ones(n, dtype=complex), mu=np.zeros(n), supercurrent=np.zeros(0),
                    normal_current=np.zeros(0))
    sol = Given(device=device, options=tdgl.SolverOptions(solve_time=1.0, field_units="mT", current_units="uA"),
                saved_steps=[step], applied_vector_potential=0.0)
    lo, hi = device.points.min(axis=0), device.points.max(axis=0)
    gx, gy = np.meshgrid(np.linspace(lo[0] - 2.0, hi[0] + 2.0, 128), np.linspace(lo[1] - 2.0, hi[1] + 2.0, 128))
    grid = np.column_stack([gx.ravel(), gy.ravel()])
    z = 3 * xi
    image = sol.field_at_position(grid, zs=z, vector=True, return_sum=False, with_units=False, backend="hip")
    assert image.supercurrent.shape == (128 * 128, 3) and np.isfinite(image.supercurrent).all()
    assert np.all(image.normal_current == 0)
    pick = np.random.default_rng(2).choice(len(grid), size=64, replace=False)
    tgt = np.column_stack([grid[pick], z * np.ones(64)])
    model = host_sums(device.points, mesh.areas * xi**2, 0.0, Ks[None], tgt, chunk=8)
    _, b_unit = unit_factors(sol)
    assert_within_yardstick(image.supercurrent[pick, 2] / b_unit, model["Z"][0], model["Z_abs"][0], n, "250k image B_z")
    assert_within_yardstick(image.supercurrent[pick, :2] / b_unit, model["XY"][0], model["XY_abs"][0], n, "250k image B_xy")
    # a polygon-sized request against the same sites (small m, large n), far above the film: the dipole field
    moment = sol.magnetic_moment(with_units=False)  # uA um^2
    height = 200 * (hi[0] - lo[0])
    centre = xi * com
    Bz = sol.field_at_position(np.array([[centre[0], centre[1]]]), zs=height, with_units=False, backend="hip")[0]
    dipole = MU_0 * (moment * 1e-6 * 1e-12) / (2 * np.pi * (height * 1e-6) ** 3) / 1e-3  # A m^2 -> T -> mT
    assert np.isclose(Bz, dipole, rtol=1e-4), (Bz, dipole)
