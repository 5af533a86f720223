"""Vortex cores, charges and boundary windings, the parts that need no GPU: the NumPy model (tests/vortex_model.py)
against the wrapped-phase forms, analytic fields and exact rational arithmetic; the host backend of
`Solution.vortices` / `Solution.boundary_windings` against the model; `Device.boundary_sites` and
`Solution.boundary_phases`; the C symbols' argument checks.  The device path: tests/test_hip_vortices.py."""

import ctypes as C

import numpy as np
import pytest

import vortex_model as vm
from conftest import load_golden

FIELD_SNAPSHOTS = ("snap0", "snap50", "snap200", "snap500", "final")
FIELD_CORES = (0, 12, 48, 40, 40)
TRANSPORT_SNAPSHOTS = ("snap10", "snap150", "final")


def small_device():
    import tdgl_amd as tdgl

    g = load_golden("mesh_small")
    lo, hi = g["mesh_sites"].min(axis=0), g["mesh_sites"].max(axis=0)
    film = tdgl.Polygon("film", points=[(lo[0], lo[1]), (hi[0], lo[1]), (hi[0], hi[1]), (lo[0], hi[1])])
    device = tdgl.Device("small", layer=tdgl.Layer(coherence_length=1.0, london_lambda=2.0, thickness=0.1), film=film)
    device.mesh_from_triangulation(g["mesh_sites"], g["mesh_elements"])
    return device


def polygon_device():
    import tdgl_amd as tdgl

    g = load_golden("mesh_polygon")
    device = tdgl.Device(
        "polygon", layer=tdgl.Layer(coherence_length=1.0, london_lambda=2.0, thickness=0.1),
        film=tdgl.Polygon("film", points=g["film"]),
        holes=[tdgl.Polygon("hole0", points=g["hole0"]), tdgl.Polygon("hole1", points=g["hole1"])])
    device.mesh_from_triangulation(g["mesh_sites"], g["mesh_elements"])
    return device


def solution_of(device, psi):
    """A Solution whose loaded step holds ``psi`` (no solver run)."""
    import tdgl_amd as tdgl
    from tdgl_amd.solution import Solution, TDGLData

    m = len(device.mesh.edge_mesh.edges)
    step = TDGLData(step=0, time=0.0, dt=0.0, psi=np.asarray(psi, dtype=complex), mu=np.zeros(len(psi)),
                    supercurrent=np.zeros(m), normal_current=np.zeros(m))
    return Solution(device=device, options=tdgl.SolverOptions(solve_time=1.0), saved_steps=[step])


@pytest.fixture(scope="module")
def small():
    device = small_device()
    sites, elements = device.points, device.triangles
    return device, sites, elements, vm.orientations(sites, elements)


@pytest.fixture(scope="module")
def polygon():
    device = polygon_device()
    sites, elements = device.points, device.triangles
    return device, sites, elements, vm.orientations(sites, elements), device.boundary_sites()


def linear_factor(sites, x0, y0, conjugate=False):
    psi = (sites[:, 0] - x0) + 1j * (sites[:, 1] - y0)
    return psi.conj() if conjugate else psi


def containing_triangle(sites, elements, x0, y0):
    """The triangle with (x0, y0) strictly inside, by exact rational barycentric signs."""
    from fractions import Fraction as F

    hits = []
    for t, (i, j, k) in enumerate(elements):
        r = [(F(float(sites[v, 0])) - F(x0), F(float(sites[v, 1])) - F(y0)) for v in (i, j, k)]
        s = [r[a][0] * r[b][1] - r[a][1] * r[b][0] for a, b in ((0, 1), (1, 2), (2, 0))]
        if all(v > 0 for v in s) or all(v < 0 for v in s):
            hits.append(t)
    assert len(hits) == 1
    return hits[0]


def stokes_sides(psi, elements, orient, loops):
    """(sum of the triangle charges, winding of the outer loop - sum of the hole windings), or None for the second
    when a loop's winding is not defined."""
    total = int(vm.charges(psi[None], elements, orient).sum())
    w = {name: vm.winding(psi, loop) for name, loop in loops.items()}
    if vm.WINDING_UNDEFINED in w.values():
        return total, None
    return total, w["film"] - sum(v for name, v in w.items() if name != "film")


def test_model_equals_the_wrapped_phase_count_on_the_field_snapshots(small):
    device, sites, elements, orient = small
    assert len(elements) == 943 and np.all(orient == 1)
    g = load_golden("traj_field_small")
    for snap, want in zip(FIELD_SNAPSHOTS, FIELD_CORES):
        psi = g[snap + "_psi"]
        got = vm.charges(psi[None], elements, orient)[0]
        assert np.array_equal(got, vm.wrapped_phase_charges(psi, elements, orient)), snap
        assert np.count_nonzero(got) == want, snap
        # the host backend is the model
        v = solution_of(device, psi).vortices()
        rec = vm.find(psi, sites, elements, orient)
        assert np.array_equal(v.triangles, rec["triangle"]) and np.array_equal(v.charges, rec["charge"])
        assert v.positions.shape == (want, 2) and np.all(np.abs(v.positions - rec["xy"]).max(axis=1, initial=0) <= rec["bound"])
        assert v.triangles.dtype == np.int32 and v.charges.dtype == np.int32


def test_model_reports_no_core_at_the_terminal_sites_where_psi_is_zero(polygon):
    device, sites, elements, orient, loops = polygon
    g = load_golden("traj_transport_polygon")
    fixed = g["fixed_sites"]
    spurious = 0
    for snap in TRANSPORT_SNAPSHOTS:
        psi = g[snap + "_psi"]
        assert np.all(psi[fixed] == 0) and len(fixed) == 20
        assert not vm.charges(psi[None], elements, orient).any(), snap
        assert len(solution_of(device, psi).vortices().charges) == 0
        wrapped = vm.wrapped_phase_charges(psi, elements, orient)
        # the wrapped form's windings all sit on triangles that touch a psi = 0 site
        assert np.isin(elements[wrapped != 0], fixed).any(axis=1).all()
        spurious += np.count_nonzero(wrapped)
    assert spurious > 0


@pytest.mark.parametrize("x0, y0", [(1.2345, -0.777), (-4.03125, 2.6), (0.013, 0.021)])
def test_one_linear_zero_is_one_core_in_its_triangle(small, x0, y0):
    device, sites, elements, orient = small
    t = containing_triangle(sites, elements, x0, y0)
    for conjugate, charge in ((False, 1), (True, -1)):
        psi = linear_factor(sites, x0, y0, conjugate)
        rec = vm.find(psi, sites, elements, orient)
        assert rec["triangle"].tolist() == [t] and rec["charge"].tolist() == [charge]
        assert np.abs(rec["xy"][0] - (x0, y0)).max() <= rec["bound"][0]
        v = solution_of(device, psi).vortices()
        assert v.triangles.tolist() == [t] and v.charges.tolist() == [charge]
        assert np.abs(v.positions[0] - (x0, y0)).max() <= rec["bound"][0]
        assert solution_of(device, psi).boundary_windings() == {"film": charge}


def test_a_zero_inside_a_hole_is_a_winding_and_no_core(polygon):
    device, sites, elements, orient, loops = polygon
    g = load_golden("mesh_polygon")
    x0, y0 = g["hole0"].mean(axis=0)
    assert device.holes[0].contains_points([(x0, y0)]).all() and not device.contains_points([(x0, y0)]).any()
    psi = linear_factor(sites, x0, y0)
    assert not vm.charges(psi[None], elements, orient).any()
    assert {name: vm.winding(psi, loop) for name, loop in loops.items()} == {"film": 1, "hole0": 1, "hole1": 0}
    sol = solution_of(device, psi)
    assert len(sol.vortices().charges) == 0
    assert sol.boundary_windings() == {"film": 1, "hole0": 1, "hole1": 0}
    assert sol.boundary_windings(backend="host") == sol.boundary_windings()


def test_stokes_identity_holds_exactly(small, polygon):
    rng = np.random.default_rng(11)
    for device, sites, elements, orient, loops in (small + ({"film": small[0].boundary_sites()["film"]},), polygon):
        lo, hi = sites.min(axis=0), sites.max(axis=0)
        for trial in range(6):
            psi = np.ones(len(sites), dtype=complex)
            for k in range(1 + trial):
                x0, y0 = rng.uniform(lo, hi)
                psi = psi * linear_factor(sites, x0, y0, conjugate=bool(rng.integers(2)))
            total, boundary = stokes_sides(psi, elements, orient, loops)
            assert boundary is not None and total == boundary
    device, sites, elements, orient = small
    g = load_golden("traj_field_small")
    loops = device.boundary_sites()
    for snap in FIELD_SNAPSHOTS:
        total, boundary = stokes_sides(g[snap + "_psi"], elements, orient, loops)
        assert boundary is not None and total == boundary, snap
        if snap == "snap200":
            assert total == 26
    device, sites, elements, orient, loops = polygon
    g = load_golden("traj_transport_polygon")
    for snap in TRANSPORT_SNAPSHOTS:  # the film's loop passes through the terminals' psi = 0 sites: not defined
        assert stokes_sides(g[snap + "_psi"], elements, orient, loops) == (0, None)
        w = solution_of(device, g[snap + "_psi"]).boundary_windings()
        assert w["film"] is None and isinstance(w["hole0"], int) and isinstance(w["hole1"], int)


def test_positions_agree_with_exact_rational_arithmetic(small):
    device, sites, elements, orient = small
    g = load_golden("traj_field_small")
    checked = 0
    frames = [g[snap + "_psi"] for snap in FIELD_SNAPSHOTS]
    rng = np.random.default_rng(12)  # ... and random fields spanning eight decades of |psi|
    frames += [(rng.normal(size=len(sites)) + 1j * rng.normal(size=len(sites))) * 10.0 ** rng.uniform(-4, 4, len(sites))
               for _ in range(2)]
    for psi in frames:
        rec = vm.find(psi, sites, elements, orient)
        host = solution_of(device, psi).vortices()
        assert np.array_equal(host.triangles, rec["triangle"])
        for k, t in enumerate(rec["triangle"]):
            i, j, l = elements[t]
            exact = vm.exact_position(psi[i], psi[j], psi[l], sites[i], sites[j], sites[l])
            assert np.abs(rec["xy"][k] - exact).max() <= rec["bound"][k]
            assert np.abs(host.positions[k] - exact).max() <= rec["bound"][k]
            checked += 1
    assert checked > 300


def test_boundary_sites_are_closed_counter_clockwise_chains_of_boundary_edges(polygon):
    device, sites, elements, orient, loops = polygon
    assert list(loops) == ["film", "hole0", "hole1"]
    assert [len(loops[name]) for name in loops] == [178, 40, 30]
    em = device.mesh.edge_mesh
    boundary = {tuple(sorted(e)) for e in em.edges[em.boundary_edge_indices].tolist()}
    used = set()
    for name, loop in loops.items():
        assert len(set(loop.tolist())) == len(loop)
        assert vm.shoelace(sites[loop]) > 0, name
        pairs = {tuple(sorted(p)) for p in zip(loop.tolist(), np.roll(loop, -1).tolist())}
        assert pairs <= boundary and not pairs & used
        used |= pairs
    assert used == boundary
    # every hole's loop lies on its polygon
    g = load_golden("mesh_polygon")
    for name in ("hole0", "hole1"):
        centre = g[name].mean(axis=0)
        radius = np.linalg.norm(g[name] - centre, axis=1)
        d = np.linalg.norm(sites[loops[name]] - centre, axis=1)
        assert d.min() >= radius.min() * 0.9 and d.max() <= radius.max() * 1.1
    import tdgl_amd as tdgl

    bare = tdgl.Device("bare", layer=device.layer, film=device.film)
    assert bare.boundary_sites() is None


def test_boundary_phases_is_the_unwrapped_angle_along_the_open_chain(polygon):
    device, sites, elements, orient, loops = polygon
    g = load_golden("mesh_polygon")
    psi = linear_factor(sites, *g["hole0"].mean(axis=0)) * np.exp(0.3j)
    sol = solution_of(device, psi)
    for delta in (False, True):
        got = sol.boundary_phases(delta=delta)
        assert list(got) == ["film", "hole0", "hole1"]
        for name, (indices, phases) in got.items():
            want = np.unwrap(np.angle(psi[loops[name]]))
            if delta:
                want = want - want[0]
            assert np.array_equal(indices, loops[name]) and np.array_equal(phases, want)
            assert got[name].indices is indices and got[name].phases is phases
    # the reference's quirk: the open chain misses the step from the last site back to the first
    ph = sol.boundary_phases(delta=True)["hole0"].phases
    assert 0.9 < ph[-1] / (2 * np.pi) < 1.0 and sol.boundary_windings()["hole0"] == 1


def test_a_loop_through_a_zero_of_psi_has_no_winding(polygon):
    device, sites, elements, orient, loops = polygon
    g = load_golden("mesh_polygon")
    psi = linear_factor(sites, *g["hole0"].mean(axis=0))
    psi[loops["hole1"][7]] = 0.0
    assert solution_of(device, psi).boundary_windings() == {"film": 1, "hole0": 1, "hole1": None}
    psi[loops["hole0"][3]] = complex(np.inf, 1.0)
    assert solution_of(device, psi).boundary_windings() == {"film": 1, "hole0": None, "hole1": None}
    # an edge that is a segment through the origin
    from tdgl_amd.vortices import loop_winding

    square = np.array([1 + 0j, 1j, -1 + 0j, -1j])
    assert loop_winding(square, [0, 1, 2, 3]) == 1 and loop_winding(square, [3, 2, 1, 0]) == -1
    assert loop_winding(square, [0, 2, 1]) is None and vm.winding(square, [0, 2, 1]) == vm.WINDING_UNDEFINED
    with pytest.raises(ValueError, match="at least 3"):
        loop_winding(square, [0, 1])


def test_loop_rule_equals_the_wrapped_phase_sum_on_random_polygons():
    rng = np.random.default_rng(13)
    from tdgl_amd.vortices import loop_winding

    defined = 0
    for trial in range(2000):
        k = int(rng.integers(3, 12))
        z = rng.normal(size=k) + 1j * rng.normal(size=k)
        if trial % 3 == 0:  # a half-integer grid: exact ties, zeros and segments through the origin happen
            z = np.round(2 * z) / 2
        w = vm.winding(z, np.arange(k))
        assert loop_winding(z, np.arange(k)) == (None if w == vm.WINDING_UNDEFINED else w)
        if w != vm.WINDING_UNDEFINED:
            u, v = z, np.roll(z, -1)
            if not np.any(u.real * v.imag == u.imag * v.real):  # (a wrapped difference of exactly pi has no sign)
                assert w == vm.wrapped_phase_winding(z, np.arange(k))
                defined += 1
    assert defined > 1500


def test_unknown_backend_is_refused_and_hip_without_a_gpu_says_so(small):
    import tdgl_amd as tdgl
    from tdgl_amd import _lib

    device, sites, elements, orient = small
    sol = solution_of(device, linear_factor(sites, 0.3, 0.2))
    for call in (lambda: sol.vortices(backend="nonsense"), lambda: sol.boundary_windings(backend="nonsense")):
        with pytest.raises(ValueError, match=r"host.*hip"):
            call()
    if _lib.load().tdgl_device_count() > 0:
        pytest.skip("a GPU is visible: the hip backend runs (tests/test_hip_vortices.py)")
    for call in (lambda: sol.vortices(backend="hip"), lambda: sol.boundary_windings(backend="hip"),
                 lambda: tdgl.VortexFinder(device)):
        with pytest.raises(RuntimeError, match="tdgl_device_count"):
            call()


def test_vortex_plan_symbols_are_declared_and_refuse_bad_arguments_by_message():
    from tdgl_amd import _lib

    lib = _lib.load()
    for name in ("tdgl_vortex_plan_create", "tdgl_vortex_plan_destroy", "tdgl_vortex_plan_find", "tdgl_vortex_plan_stats"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    sites = np.zeros((4, 2))
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    ptr = np.array([0, 3], dtype=np.int64)
    loop = np.array([0, 1, 2], dtype=np.int32)

    def create(n_sites=4, n_tri=1, tri=tri, n_loops=1, ptr=ptr, loop=loop):
        plan = C.c_void_p()
        status = lib.tdgl_vortex_plan_create(C.byref(plan), 0, n_sites, _lib.p_f64(sites), n_tri, _lib.p_i32(tri), n_loops,
                                             _lib.p_i64(ptr), _lib.p_i32(loop))
        assert status == _lib.TDGL_ERR_ARG and not plan.value
        return lib.tdgl_last_error(None)

    # argument errors are reported before any device work
    assert b"negative size" in create(n_sites=-1)
    assert b"negative size" in create(n_tri=-1)
    assert b"negative size" in create(n_loops=-1)
    assert b"n_sites must be" in create(n_sites=0, n_tri=0, n_loops=0)
    assert b"null array" in create(tri=None)
    assert b"out of range" in create(tri=np.array([[0, 1, 4]], dtype=np.int32))
    assert b"out of range" in create(tri=np.array([[0, -1, 2]], dtype=np.int32))
    assert b"at least 3" in create(ptr=np.array([0, 2], dtype=np.int64))
    assert b"loop site" in create(loop=np.array([0, 1, 7], dtype=np.int32))
    assert b"loop_ptr[0]" in create(ptr=np.array([1, 4], dtype=np.int64))
    assert lib.tdgl_vortex_plan_find(None, 1, None, 0, None, None, None, None) == _lib.TDGL_ERR_ARG
    assert lib.tdgl_vortex_plan_stats(None, None, None) == _lib.TDGL_ERR_ARG
