"""Currents and psi between the sites, the parts that need no GPU: the NumPy model (tests/sample_model.py) against
`Mesh.get_quantity_on_site` and `TriLinearInterpolator`; the grid search of csrc/sample_grid.h through
`tdgl_host_sample_locate` against the model's exhaustive search (triangles for equality, weights byte for byte); the C
symbols' argument checks; the error of the hip backend without a GPU.  The device path: tests/test_hip_sampling.py."""

import ctypes as C

import numpy as np
import pytest

import sample_model as sm
from conftest import load_golden

FIXTURES = ("mesh_small", "mesh_polygon", "mesh_irregular")


def delaunay_mesh(n_sites, seed):
    from scipy.spatial import Delaunay

    sites = np.random.default_rng(seed).uniform([-3.0, -1.0], [5.0, 4.0], size=(n_sites, 2))
    return sites, Delaunay(sites).simplices.astype(np.int32)


def triples_mesh(n_tri, seed):
    """Random index triples over a few random sites: overlapping triangles of every size; from 63 triangles on the
    first is degenerate (a repeated site) and lies over everything."""
    rng = np.random.default_rng(seed)
    n_sites = max(3, min(n_tri, 40))
    sites = rng.uniform(-2.0, 2.0, size=(n_sites, 2))
    elements = np.array([rng.choice(n_sites, 3, replace=False) for _ in range(n_tri)], dtype=np.int32)
    if n_tri >= 63:
        elements[0] = (elements[0, 0], elements[0, 0], elements[0, 1])
    return sites, elements


def fixture_mesh(name):
    g = load_golden(name)
    return g["mesh_sites"], g["mesh_elements"].astype(np.int32)


def rounding_of_the_coordinates(sites, elements):
    """Per triangle an a-priori bound on the error of a computed barycentric coordinate of a point p of the mesh's
    triangle t (a vertex, a midpoint, the centroid): p itself is rounded (u R, R the largest coordinate; the difference
    p - a of two points of one triangle then adds at most u L, L the triangle's longest edge), the two products and their
    sum round once more each (3 u L |inv|), so ``|error| <= u (R + 4 L) (|inv0| + |inv1| + |inv2| + |inv3|)``, taken
    twice for room.  Infinite for a degenerate triangle."""
    a, inv, usable = sm.triangle_geometry(sites, elements)
    tri = sites[elements]
    longest = np.sqrt(((tri - np.roll(tri, 1, axis=1)) ** 2).sum(axis=2)).max(axis=1)
    with np.errstate(invalid="ignore"):
        bound = 2 * sm.U * (np.abs(sites).max() + 4 * longest) * np.abs(inv).sum(axis=1)
    return np.where(usable, bound, np.inf)


def query_points(sites, elements, seed):
    """(every vertex, edge midpoint and centroid; which of them the rounding bound above guarantees a triangle; points
    that must not be located; points uniform in the inflated bounding box).

    A vertex or a midpoint has an exact barycentric coordinate 0 in each of its triangles: the computed one is
    >= -1e-12 for certain where the triangle's rounding bound is below 1e-12, which a needle of a random Delaunay
    triangulation's hull (aspect ratio beyond 1e3) does not meet.  Such a point, when it has no better triangle, is
    compared with the exhaustive search like every other, but is not required to be in a triangle."""
    tri = sites[elements]
    err = rounding_of_the_coordinates(sites, elements)
    fine = err <= sm.TOL
    used, where = np.unique(elements, return_inverse=True)
    site_fine = np.zeros(len(used), dtype=bool)
    np.logical_or.at(site_fine, where.reshape(-1), np.repeat(fine, 3))
    pairs = np.sort(np.concatenate([elements[:, [0, 1]], elements[:, [1, 2]], elements[:, [2, 0]]]), axis=1)
    edges, where = np.unique(pairs, axis=0, return_inverse=True)
    edge_fine = np.zeros(len(edges), dtype=bool)
    np.logical_or.at(edge_fine, where.reshape(-1), np.tile(fine, 3))
    keep = edges[:, 0] != edges[:, 1]
    edges, edge_fine = edges[keep], edge_fine[keep]
    used = sites[used]
    midpoints = (sites[edges[:, 0]] + sites[edges[:, 1]]) / 2
    centroids = (tri[:, 0] + tri[:, 1] + tri[:, 2]) / 3
    guaranteed = np.concatenate([site_fine, edge_fine, err <= 1 / 3])
    lo, hi = sites.min(axis=0), sites.max(axis=0)
    span = np.maximum(hi - lo, 1.0)
    rng = np.random.default_rng(seed)
    outside = np.concatenate([
        np.column_stack([rng.uniform(lo[0] - span[0], hi[0] + span[0], 40), hi[1] + rng.uniform(1e-6, 3.0, 40) * span[1]]),
        np.column_stack([rng.uniform(lo[0] - span[0], hi[0] + span[0], 40), lo[1] - rng.uniform(1e-6, 3.0, 40) * span[1]]),
        np.column_stack([hi[0] + rng.uniform(1e-6, 3.0, 40) * span[0], rng.uniform(lo[1] - span[1], hi[1] + span[1], 40)]),
        np.column_stack([lo[0] - rng.uniform(1e-6, 3.0, 40) * span[0], rng.uniform(lo[1] - span[1], hi[1] + span[1], 40)]),
        [[1e300, -1e300], [hi[0] + 1e-9 * span[0], hi[1] + 1e-9 * span[1]]]])
    uniform = rng.uniform(lo - 0.1 * span, hi + 0.1 * span, size=(1500, 2))
    return np.concatenate([used, midpoints, centroids]), guaranteed, outside, uniform


def assert_same_location(sites, elements, points, label):
    from tdgl_amd.hipcore import host_sample_locate

    want_t, want_w = sm.locate(sites, elements, points)
    got_t, got_w = host_sample_locate(sites, elements, points)
    assert got_t.dtype == np.int32 and np.array_equal(got_t, want_t), label
    assert got_w.tobytes() == want_w.tobytes(), label
    return got_t


CASES = ([("delaunay", n) for n in (3, 4, 64, 65, 1000, 20_000)] + [("fixture", name) for name in FIXTURES]
         + [("triples", n) for n in (1, 63, 257)])


@pytest.mark.parametrize("kind, which", CASES)
def test_grid_search_equals_the_exhaustive_search(kind, which):
    if kind == "delaunay":
        sites, elements = delaunay_mesh(which, seed=100 + which)
    elif kind == "triples":
        sites, elements = triples_mesh(which, seed=200 + which)
    else:
        sites, elements = fixture_mesh(which)
    located, guaranteed, outside, uniform = query_points(sites, elements, seed=7)
    label = f"{kind} {which}"
    t = assert_same_location(sites, elements, located, label)
    print(f"{label}: {len(t)} vertices, midpoints and centroids, {np.count_nonzero(~guaranteed)} without a guarantee, "
          f"{np.count_nonzero(t < 0)} in no triangle")
    assert np.all(t[guaranteed] >= 0), f"{label}: {np.count_nonzero(t[guaranteed] < 0)} vertices, midpoints or centroids in no triangle"
    if kind == "fixture":  # a mesher's triangles are all well shaped
        assert guaranteed.all()
    assert np.count_nonzero(~guaranteed) <= 0.01 * len(t) or kind == "triples"  # (the hull's needles are few)
    assert np.all(assert_same_location(sites, elements, outside, label) == -1), label
    t = assert_same_location(sites, elements, uniform, label)
    assert np.any(t >= 0) and np.any(t < 0), label
    if kind == "triples" and which >= 63:  # the degenerate triangle 0 lies over everything and is never chosen
        assert not np.any(t == 0) and np.any(t == 1)
    if which == "mesh_polygon":
        g = load_golden("mesh_polygon")
        holes = np.concatenate([c + s * (g[name] - c) for name in ("hole0", "hole1") for c in [g[name].mean(axis=0)]
                                for s in (0.0, 0.3, 0.8)])
        assert np.all(assert_same_location(sites, elements, holes, label) == -1)


def test_the_lowest_numbered_triangle_wins_where_triangles_overlap():
    from tdgl_amd.hipcore import host_sample_locate

    sites = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0], [4.0, 4.0], [1.0, 1.0], [2.0, 1.0], [1.0, 2.0]])
    elements = np.array([[4, 5, 6], [0, 1, 2], [1, 3, 2], [0, 1, 2]], dtype=np.int32)
    t, w = host_sample_locate(sites, elements, [[1.25, 1.25], [0.5, 0.5], [3.0, 3.0], [2.0, 2.0], [5.0, 5.0]])
    assert t.tolist() == [0, 1, 2, 1, -1]  # (2, 2) lies on the shared edge of 1 and 2
    assert w[0].tolist() == [0.5, 0.25, 0.25] and w[4].tolist() == [0.0, 0.0, 0.0]
    assert np.array_equal(t, sm.locate(sites, elements, [[1.25, 1.25], [0.5, 0.5], [3.0, 3.0], [2.0, 2.0], [5.0, 5.0]])[0])
    # no triangles, no points
    t, w = host_sample_locate(sites, np.zeros((0, 3), dtype=np.int32), [[1.0, 1.0]])
    assert t.tolist() == [-1] and not w.any()
    t, w = host_sample_locate(sites, elements, np.zeros((0, 2)))
    assert t.shape == (0,) and w.shape == (0, 3)
    # all sites on one line: every triangle is degenerate
    line = np.column_stack([np.arange(5.0), np.zeros(5)])
    t, _ = host_sample_locate(line, np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32), [[1.0, 0.0], [3.5, 0.0]])
    assert t.tolist() == [-1, -1] and sm.locate(line, [[0, 1, 2], [2, 3, 4]], [[1.0, 0.0]])[0].tolist() == [-1]


@pytest.mark.parametrize("name", FIXTURES)
def test_model_edge_to_site_equals_get_quantity_on_site_byte_for_byte(name):
    from tdgl_amd.finite_volume import Mesh

    sites, elements = fixture_mesh(name)
    mesh = Mesh.from_triangulation(sites, elements)
    em = mesh.edge_mesh
    rng = np.random.default_rng(3)
    values = rng.normal(size=(3, len(em.edges))) * 10.0 ** rng.uniform(-3, 3, size=(3, len(em.edges)))
    got = sm.site_density(len(sites), em.edges, em.normalized_directions, values)
    for k in range(3):
        want = mesh.get_quantity_on_site(values[k])
        assert got[k].shape == want.shape and got[k].tobytes() == np.ascontiguousarray(want).tobytes()
    # every site of a triangulation has an edge; the model's rows are np.bincount's order
    rows = sm.incidence_rows(len(sites), em.edges)
    assert min(len(r) for r in rows) >= 2 and sum(len(r) for r in rows) == 2 * len(em.edges)


@pytest.mark.parametrize("name", FIXTURES)
def test_model_agrees_with_the_host_interpolator_at_generic_points(name):
    from tdgl_amd.hipcore import host_sample_locate
    from tdgl_amd.triinterp import TriLinearInterpolator

    sites, elements = fixture_mesh(name)
    rng = np.random.default_rng(5)
    tri = sites[elements[rng.integers(0, len(elements), 600)]]
    w = rng.dirichlet([2.0, 2.0, 2.0], size=600)  # interior: every weight well above the tolerance
    w = w[w.min(axis=1) > 1e-3]
    points = np.einsum("mk,mkc->mc", w, tri[:len(w)])
    interp = TriLinearInterpolator(sites, elements)
    ref_t, ref_w = interp.locate(points)
    t, lam = host_sample_locate(sites, elements, points)
    assert np.array_equal(t, ref_t) and np.all(t >= 0)
    assert lam.tobytes() == ref_w.tobytes()
    vec = rng.normal(size=(len(sites), 2))
    psi = rng.normal(size=len(sites)) + 1j * rng.normal(size=len(sites))
    for values in (vec, psi):
        got = sm.sample(values, elements, t, lam)
        want = interp(values, points)
        parts = np.stack([values.real, values.imag], axis=-1) if np.iscomplexobj(values) else values
        bound = 8 * sm.U * (np.abs(lam)[:, :, None] * np.abs(parts[elements[t]])).sum(axis=1)
        err = np.abs(got - want)
        err = np.stack([np.abs((got - want).real), np.abs((got - want).imag)], axis=-1) if np.iscomplexobj(values) else err
        assert np.all(err <= bound)
    # outside: NaN in the model as in the interpolator
    far = sites.max(axis=0) + [[1.0, 1.0]]
    t, lam = host_sample_locate(sites, elements, far)
    assert np.isnan(sm.sample(vec, elements, t, lam)).all() and np.isnan(interp(vec, far)).all()
    assert np.isnan(sm.sample(psi, elements, t, lam)).all()


def test_model_moment_is_the_fsum_of_the_terms():
    sites, elements = fixture_mesh("mesh_small")
    rng = np.random.default_rng(9)
    g = rng.normal(size=(2, len(sites), 2))
    weight = rng.uniform(0.1, 1.0, len(sites))
    total, bound = sm.moment(sites, weight, (0.3, -0.2), g)
    plain = sm.moment_terms(sites, weight, (0.3, -0.2), g).sum(axis=-1)
    assert total.shape == (2,) and np.all(np.abs(plain - total) <= bound) and np.all(bound > 0)


def test_sample_symbols_are_declared_and_refuse_bad_arguments_by_message():
    from tdgl_amd import _lib

    lib = _lib.load()
    names = ("tdgl_sample_plan_create", "tdgl_sample_plan_destroy", "tdgl_sample_plan_location", "tdgl_sample_plan_eval",
             "tdgl_sample_plan_stats", "tdgl_host_sample_locate")
    for name in names:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    sites = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    weight, centre = np.ones(4), np.array([0.5, 0.5])
    edges = np.array([[0, 1], [1, 2], [2, 0], [1, 3], [3, 2]], dtype=np.int32)
    dirs = sm.directions(sites, edges)
    tri = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
    points = np.array([[0.2, 0.2], [0.9, 0.9]])
    default = dict(device_id=0, n_sites=4, sites=sites, weight=weight, centre=centre, n_edges=5, edges=edges, dirs=dirs,
                   n_tri=2, tri=tri, m=2, points=points)

    def create(**change):
        a = dict(default, **change)
        plan = C.c_void_p()
        status = lib.tdgl_sample_plan_create(
            C.byref(plan), a["device_id"], a["n_sites"], _lib.p_f64(a["sites"]), _lib.p_f64(a["weight"]), _lib.p_f64(a["centre"]),
            a["n_edges"], _lib.p_i32(a["edges"]), _lib.p_f64(a["dirs"]), a["n_tri"], _lib.p_i32(a["tri"]), a["m"],
            _lib.p_f64(a["points"]))
        if status == _lib.TDGL_OK:  # (a GPU is visible and nothing was wrong)
            lib.tdgl_sample_plan_destroy(plan)
            return b""
        assert status == _lib.TDGL_ERR_ARG and not plan.value
        return lib.tdgl_last_error(None)

    def bad(array, index, value):
        out = array.copy()
        out[index] = value
        return out

    # argument errors are reported before any device work
    for size in ("n_sites", "n_edges", "n_tri", "m"):
        assert b"negative size" in create(**{size: -1}), size
    assert b"n_sites must be" in create(n_sites=0, n_edges=0, n_tri=0, m=0)
    assert b"null sites_xy" in create(sites=None)
    assert b"null edges" in create(edges=None)
    assert b"null edge_dir" in create(dirs=None)
    assert b"null elements" in create(tri=None)
    assert b"null points_xy" in create(points=None)
    assert b"null centre_xy" in create(centre=None)
    assert b"edges: edge 3 names site 4, out of range" in create(edges=bad(edges, (3, 1), 4))
    assert b"edges: edge 0 names site -1" in create(edges=bad(edges, (0, 0), -1))
    assert b"elements: element 1 names site 7, out of range" in create(tri=bad(tri, (1, 2), 7))
    assert b"elements: element 0 names site -2" in create(tri=bad(tri, (0, 1), -2))
    assert b"sites_xy: site 2 is not finite" in create(sites=bad(sites, (2, 1), np.nan))
    assert b"points_xy: point 1 is not finite" in create(points=bad(points, (1, 0), np.inf))
    assert b"site_weight: the weight of site 3 is not finite" in create(weight=bad(weight, 3, -np.inf))
    assert b"centre_xy is not finite" in create(centre=np.array([np.nan, 0.0]))
    assert b"edge_dir: the direction of edge 4 is not finite" in create(dirs=bad(dirs, (4, 0), np.nan))
    assert b"edges: site 3 has no edge" in create(n_edges=3)
    assert b"edges: site 0 has no edge" in create(n_edges=0, edges=None, dirs=None)
    assert b"no HIP device 4096" in create(device_id=4096)
    assert b"no HIP device -1" in create(device_id=-1)
    null = C.c_void_p()
    assert lib.tdgl_sample_plan_create(None, 0, 4, None, None, None, 0, None, None, 0, None, 0, None) == _lib.TDGL_ERR_ARG
    assert b"null output pointer" in lib.tdgl_last_error(None)

    def refused(*args):
        assert lib.tdgl_sample_plan_eval(*args) == _lib.TDGL_ERR_ARG
        return lib.tdgl_last_error(None)

    assert b"n_fields must be 0, 1 or 2 (got 3)" in refused(null, 1, 3, None, None, None, None, None, None)
    assert b"n_fields must be 0, 1 or 2 (got -1)" in refused(null, 1, -1, None, None, None, None, None, None)
    assert b"n_frames must be >= 1 (got 0)" in refused(null, 0, 1, None, None, None, None, None, None)
    assert b"null plan" in refused(null, 1, 1, None, None, None, None, None, None)
    assert lib.tdgl_sample_plan_location(None, None, None) == _lib.TDGL_ERR_ARG and b"null plan" in lib.tdgl_last_error(None)
    assert lib.tdgl_sample_plan_stats(None, None, None) == _lib.TDGL_ERR_ARG and b"null plan" in lib.tdgl_last_error(None)
    lib.tdgl_sample_plan_destroy(None)

    def locate(**change):
        a = dict(default, **change)
        t, w = np.zeros(2, dtype=np.int32), np.zeros((2, 3))
        status = lib.tdgl_host_sample_locate(a["n_sites"], _lib.p_f64(a["sites"]), a["n_tri"], _lib.p_i32(a["tri"]), a["m"],
                                             _lib.p_f64(a["points"]), _lib.p_i32(a.get("t", t)), _lib.p_f64(a.get("w", w)))
        assert status == _lib.TDGL_ERR_ARG
        return lib.tdgl_last_error(None)

    assert b"tdgl_host_sample_locate: negative size" in locate(m=-1)
    assert b"n_sites must be" in locate(n_sites=0)
    assert b"null elements" in locate(tri=None)
    assert b"out of range" in locate(tri=bad(tri, (0, 0), 4))
    assert b"point 0 is not finite" in locate(points=bad(points, (0, 1), np.nan))
    assert b"site 0 is not finite" in locate(sites=bad(sites, (0, 0), np.inf))
    assert b"null triangle or weights" in locate(t=None)


def test_hip_backend_without_a_gpu_says_so(monkeypatch):
    import tdgl_amd as tdgl
    from tdgl_amd import _lib
    from test_vortices_host import small_device, solution_of

    device = small_device()
    sol = solution_of(device, np.ones(len(device.points), dtype=complex))
    points = np.array([[0.1, 0.2], [0.4, -0.3], [1.0, 1.0]])
    for call in (lambda: sol.interp_current_density(points, backend="nonsense"),
                 lambda: sol.interp_order_parameter(points, backend="nonsense"),
                 lambda: sol.current_through_path(points, backend="nonsense"),
                 lambda: sol.magnetic_moment(backend="nonsense")):
        with pytest.raises(ValueError, match=r"host.*hip"):
            call()
    monkeypatch.setattr(_lib, "device_count", lambda: 0)  # what this machine says, whether or not a GPU is visible
    for call in (lambda: sol.interp_current_density(points, backend="hip"),
                 lambda: sol.interp_order_parameter(points, backend="hip"),
                 lambda: sol.current_through_path(points, backend="hip"),
                 lambda: sol.magnetic_moment(backend="hip"),
                 lambda: tdgl.CurrentSampler(device, points), lambda: tdgl.CurrentSampler(device)):
        with pytest.raises(RuntimeError, match="tdgl_device_count"):
            call()
    # the default path is the host's, unchanged: a sampler is not even looked at
    assert np.array_equal(sol.interp_current_density(points, sampler=object()), sol.interp_current_density(points))
    assert sol.magnetic_moment(with_units=False, sampler=object()) == sol.magnetic_moment(with_units=False)
