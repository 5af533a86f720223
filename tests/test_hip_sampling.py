"""Currents and psi between the sites on the device (csrc/sample.inc, `hipcore.SamplePlan`, `tdgl_amd.CurrentSampler`,
``backend="hip"`` of `Solution.interp_current_density` / `interp_order_parameter` / `current_through_path` /
`magnetic_moment`) against the NumPy model of tests/sample_model.py: location, site densities, sampled densities and
psi BYTE FOR BYTE (every result is a fixed sequence of separately rounded operations), the moments within the
summation-order bound ``n 2^-53 sum |term|`` of the model's ``fsum``."""

import numpy as np
import pytest

import sample_model as sm
from conftest import load_golden

pytestmark = pytest.mark.gpu

MESHES = ("triangle", "mesh_small", "delaunay_1000", "mesh_polygon")
SIZES = (1, 63, 64, 65, 257, 70_001)
M_MAX = max(SIZES)
_CASES = {}


def mesh_case(name):
    """Per mesh, once: sites, edges, directions, elements, weights, centre, M_MAX points, Gaussian edge values
    [3, 2, E] and psi [3, n], and the model's answers for all of them (a case with fewer points, frames or fields is a
    slice: every point, frame and field is computed on its own)."""
    if name in _CASES:
        return _CASES[name]
    rng = np.random.default_rng(900 + MESHES.index(name))
    if name == "triangle":
        sites, elements = np.array([[0.25, -0.5], [3.0, 0.125], [1.0, 2.75]]), np.array([[0, 1, 2]], dtype=np.int32)
    elif name == "delaunay_1000":
        from scipy.spatial import Delaunay

        sites = rng.uniform([-3.0, -1.0], [5.0, 4.0], size=(1000, 2))
        elements = Delaunay(sites).simplices.astype(np.int32)
    else:
        g = load_golden(name)
        sites, elements = g["mesh_sites"], g["mesh_elements"].astype(np.int32)
    edges = sm.edges_of(elements)
    dirs = sm.directions(sites, edges)
    n = len(sites)
    weight = rng.uniform(0.2, 1.5, n)
    centre = sites.mean(axis=0) + 0.1
    lo, hi = sites.min(axis=0), sites.max(axis=0)
    tri = sites[elements]
    special = np.concatenate([sites[:20], (sites[edges[:20, 0]] + sites[edges[:20, 1]]) / 2, tri[:20].mean(axis=1)])
    points = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(M_MAX, 2))
    k = min(len(special), 40)
    points[3:3 + k] = special[:k]  # vertices, midpoints and centroids among the first 63
    values = rng.normal(size=(3, 2, len(edges)))
    psi = rng.normal(size=(3, n)) + 1j * rng.normal(size=(3, n))
    triangle, lam = sm.locate(sites, elements, points)
    g = sm.site_density(n, edges, dirs, values)
    case = dict(sites=sites, elements=elements, edges=edges, dirs=dirs, weight=weight, centre=centre, points=points,
                values=values, psi=psi, triangle=triangle, lam=lam, g=g,
                point_g=sm.sample(g, elements, triangle, lam), point_psi=sm.sample(psi, elements, triangle, lam),
                moment=sm.moment(sites, weight, centre, g))
    _CASES[name] = case
    return case


def open_plan(c, m, weights=True, **kw):
    from tdgl_amd.hipcore import SamplePlan

    extra = dict(weights=c["weight"], centre=c["centre"]) if weights else {}
    return SamplePlan(c["sites"], c["edges"], c["dirs"], c["elements"], c["points"][:m] if m else None, **extra, **kw)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).tobytes()


def raw_eval(plan, values, psi, site=True, point=True, point_psi=True, moment=True, fill=-77.0):
    """`tdgl_sample_plan_eval` with buffers prefilled with ``fill``; None instead of the outputs not asked for."""
    from tdgl_amd import _lib

    values = None if values is None else np.ascontiguousarray(values, dtype=float)
    psi = None if psi is None else np.ascontiguousarray(psi, dtype=complex)
    frames = len(values) if values is not None else len(psi)
    nf = 0 if values is None else values.shape[1]
    out_site = np.full((frames, nf, plan.n, 2), fill) if site else None
    out_point = np.full((frames, nf, plan.m, 2), fill) if point else None
    out_psi = np.full((frames, plan.m), complex(fill, fill)) if point_psi else None
    out_moment = np.full((frames, nf), fill) if moment else None
    _lib.check(plan._lib.tdgl_sample_plan_eval(plan._plan, frames, nf, _lib.p_f64(values), _lib.p_f64(psi), _lib.p_f64(out_site),
                                               _lib.p_f64(out_point), _lib.p_f64(out_psi), _lib.p_f64(out_moment)))
    return out_site, out_point, out_psi, out_moment


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("mesh", MESHES)
def test_plan_against_the_model(mesh, m):
    c = mesh_case(mesh)
    n = len(c["sites"])
    want_total, want_bound = c["moment"]
    with open_plan(c, m) as plan:
        triangle, lam = plan.location()
        assert same(triangle, c["triangle"][:m]) and same(lam, c["lam"][:m])
        if m >= 63:
            assert np.any(triangle >= 0) and np.any(triangle < 0)
        for frames in (1, 3):
            for fields in (1, 2):
                values, psi = c["values"][:frames, :fields], c["psi"][:frames]
                first = plan.eval(values, psi, site_density=True, point_density=True, point_psi=True, moment=True)
                site, point, point_psi, moment = first
                assert same(site, c["g"][:frames, :fields])
                assert same(point, c["point_g"][:frames, :fields, :m])  # NaN where the triangle is -1: the same bytes
                assert same(point_psi, c["point_psi"][:frames, :m])
                assert np.array_equal(np.isnan(point[0, 0, :, 0]), triangle < 0)
                err = np.abs(moment - want_total[:frames, :fields])
                print(f"{mesh} m={m} F={frames} fields={fields}: moment error / bound = "
                      f"{float((err / want_bound[:frames, :fields]).max()):.3e}")
                assert moment.shape == (frames, fields) and np.all(err <= want_bound[:frames, :fields])
                stats = plan.stats()
                assert stats["located"] == np.count_nonzero(triangle >= 0) and stats["frames"] == frames
                assert stats["chunks"] == 1 and stats["launches"] == 5 and stats["last_ms"] >= 0
                second = plan.eval(values, psi, site_density=True, point_density=True, point_psi=True, moment=True)
                assert all(same(a, b) for a, b in zip(first, second))
        # the second field of a pair is the first of its own call
        alone = plan.eval(c["values"][:1, 1:2], site_density=True, moment=True)
        assert same(alone[0], c["g"][:1, 1:2]) and alone[1] is None and alone[2] is None
        both = plan.eval(c["values"][:1], moment=True)[3]
        assert alone[3].tobytes() == both[:, 1:2].tobytes()
        assert n == plan.n and plan.m == m


def test_null_outputs_are_left_alone_and_the_others_do_not_depend_on_them():
    c = mesh_case("mesh_small")
    values, psi = c["values"], c["psi"]
    with open_plan(c, 257) as plan:
        full = raw_eval(plan, values, psi)
        assert same(full[0], c["g"]) and same(full[1], c["point_g"][:, :, :257]) and same(full[2], c["point_psi"][:, :257])
        assert not np.any(full[3] == -77.0)
        for keep in range(4):
            flags = [k == keep for k in range(4)]
            one = raw_eval(plan, values, psi, *flags)
            assert [o is None for o in one] == [not f for f in flags]
            assert same(one[keep], full[keep])
        nothing = raw_eval(plan, values, psi, False, False, False, False)
        assert nothing == (None, None, None, None)
        assert plan.stats()["launches"] == 0 and plan.stats()["chunks"] == 0
        # without psi and without edge values
        only_currents = raw_eval(plan, values, None, point_psi=False)
        assert all(same(a, b) for a, b in zip(only_currents[:2] + only_currents[3:], full[:2] + full[3:]))
        only_psi = raw_eval(plan, None, psi, site=False, point=False, moment=False)
        assert same(only_psi[2], full[2])
        # psi given and not asked for: not used
        unused = raw_eval(plan, values, psi, point_psi=False)
        assert unused[2] is None and same(unused[1], full[1])


def test_frames_in_several_chunks_give_the_same_bytes(monkeypatch):
    c = mesh_case("mesh_polygon")
    rng = np.random.default_rng(77)
    values = rng.normal(size=(5, 2, len(c["edges"])))
    psi = rng.normal(size=(5, len(c["sites"]))) + 1j * rng.normal(size=(5, len(c["sites"])))
    kw = dict(site_density=True, point_density=True, point_psi=True, moment=True)
    with open_plan(c, 65) as plan:
        whole = plan.eval(values, psi, **kw)
        assert plan.stats()["chunks"] == 1 and plan.stats()["frames"] == 5
    monkeypatch.setenv("TDGL_SAMPLE_CHUNK", "2")
    with open_plan(c, 65) as plan:
        parts = plan.eval(values, psi, **kw)
        assert plan.stats()["chunks"] == 3 and plan.stats()["frames"] == 5 and plan.stats()["launches"] == 15
    assert all(same(a, b) for a, b in zip(whole, parts))  # the moments included
    monkeypatch.setenv("TDGL_SAMPLE_CHUNK", "1")
    with open_plan(c, 65) as plan:
        single = plan.eval(values, psi, **kw)
        assert plan.stats()["chunks"] == 5
    assert all(same(a, b) for a, b in zip(whole, single))
    g = sm.site_density(len(c["sites"]), c["edges"], c["dirs"], values)
    total, bound = sm.moment(c["sites"], c["weight"], c["centre"], g)
    assert same(whole[0], g) and np.all(np.abs(whole[3] - total) <= bound)


def test_a_plan_without_points_serves_the_site_outputs():
    c = mesh_case("delaunay_1000")
    with open_plan(c, 0) as plan:
        assert plan.m == 0
        triangle, lam = plan.location()
        assert triangle.shape == (0,) and lam.shape == (0, 3)
        site, point, point_psi, moment = plan.eval(c["values"], site_density=True, moment=True)
        assert same(site, c["g"]) and point is None and point_psi is None
        assert np.all(np.abs(moment - c["moment"][0]) <= c["moment"][1])
        assert plan.stats()["located"] == 0 and plan.stats()["launches"] == 3
        with pytest.raises(ValueError, match="point_density needs points"):
            plan.eval(c["values"], point_density=True)
        with pytest.raises(ValueError, match="point_psi needs points"):
            plan.eval(psi=c["psi"], point_psi=True)
    with open_plan(c, 0, weights=False) as plan:
        assert same(plan.eval(c["values"], site_density=True)[0], c["g"])
        with pytest.raises(ValueError, match="moment needs the plan's site_weight"):
            plan.eval(c["values"], moment=True)
        assert same(plan.eval(c["values"], site_density=True)[0], c["g"])


def test_a_refused_eval_leaves_the_plan_usable():
    from tdgl_amd import _lib
    from tdgl_amd.hipcore import SamplePlan

    c = mesh_case("mesh_small")
    values, psi = c["values"], c["psi"]
    with open_plan(c, 64) as plan:
        before = plan.eval(values, psi, site_density=True, point_density=True, point_psi=True, moment=True)
        lib, p = plan._lib, plan._plan
        site = np.zeros((3, 2, plan.n, 2))
        ppsi = np.zeros((3, 64), dtype=complex)

        def refused(*args):
            assert lib.tdgl_sample_plan_eval(p, *args) == _lib.TDGL_ERR_ARG
            return lib.tdgl_last_error(None)

        f64 = _lib.p_f64
        assert b"n_fields must be 0, 1 or 2 (got 3)" in refused(3, 3, f64(values), None, f64(site), None, None, None)
        assert b"n_frames must be >= 1 (got 0)" in refused(0, 2, f64(values), None, f64(site), None, None, None)
        assert b"null edge_values with n_fields 2" in refused(3, 2, None, None, f64(site), None, None, None)
        assert b"site_density needs edge_values" in refused(3, 0, None, f64(psi), f64(site), None, None, None)
        assert b"moment needs edge_values" in refused(3, 0, None, f64(psi), None, None, None, f64(site))
        assert b"point_psi needs psi" in refused(3, 2, f64(values), None, None, None, f64(ppsi), None)
        assert not site.any() and not ppsi.any()
        with pytest.raises(ValueError, match="edge values of shape"):
            plan.eval(values[:, :, :-1], site_density=True)
        with pytest.raises(ValueError, match="psi of shape"):
            plan.eval(psi=psi[:, :-1], point_psi=True)
        after = plan.eval(values, psi, site_density=True, point_density=True, point_psi=True, moment=True)
        assert all(same(a, b) for a, b in zip(before, after))
    with pytest.raises(RuntimeError, match="closed"):
        plan.eval(values, site_density=True)
    with pytest.raises(ValueError, match="no HIP device 4096"):
        open_plan(c, 1, device_id=4096)
    with pytest.raises(ValueError, match="site 515 has no edge"):
        SamplePlan(c["sites"], c["edges"][~(c["edges"] == 515).any(axis=1)], c["dirs"][~(c["edges"] == 515).any(axis=1)],
                   c["elements"])
    with pytest.raises(ValueError, match="point 0 is not finite"):
        SamplePlan(c["sites"], c["edges"], c["dirs"], c["elements"], [[np.nan, 0.0]])
    with pytest.raises(ValueError, match="weights and centre go together"):
        SamplePlan(c["sites"], c["edges"], c["dirs"], c["elements"], weights=c["weight"])


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def strip_solution():
    """A short solve of the quick-start strip (examples/quickstart.py): field, transport current, several saved steps
    (the set-up of tests/test_hip_fields.py)."""
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
    options = tdgl.SolverOptions(solve_time=6, dt_init=1e-3, field_units="mT", current_units="uA", save_every=1000)
    solution = tdgl.solve(device, options, applied_vector_potential=0.4, terminal_currents=dict(source=12.0, drain=-12.0))
    assert len(solution.saved_steps) >= 3
    return solution


def within(got, want, bound, label):
    err = np.abs(np.asarray(got) - np.asarray(want))
    bound = np.broadcast_to(bound, err.shape)
    pos = bound > 0
    print(f"{label}: max |hip - host| / bound = {float((err[pos] / bound[pos]).max()) if pos.any() else 0.0:.3e}")
    assert np.all(err <= bound), label


def test_solution_methods_with_the_hip_backend_equal_the_host_backend(strip_solution):
    """Per saved step: the four methods with ``backend="hip"`` within ``8 u sum_k |w_k v_k|`` of ``backend="host"``
    (v the site values the host interpolates, in the units asked for); the path current and the moment within the sum
    of their terms' bounds.

    The total current density (``dataset=None``) is itself a sum of two terms: the kernel samples the supercurrent and
    the normal current separately (the C interface applies no prefactor and keeps the fields apart) and the host adds
    them on the sites before it interpolates.  Where the two nearly cancel, each side carries roundings of the size of
    the parts, not of the total; the bound of the total is therefore the sum of the two fields' bounds,
    ``8 u sum_k |w_k| (|K_s,k| + |K_n,k|)``.  (Measured on an MI355X against ``8 u sum_k |w_k (K_s + K_n)_k|``, which the
    first version of this test used, over 51 saved steps: up to 53 times that, at points where the parts are 10 to 25
    times the total; each single field and the total stayed below 0.6 of the bounds used here.  The test prints that
    ratio and, at the point where it is largest, how much larger the parts are than the total.)

    Path current: it is linear in the sampled densities, so the terms' bounds go through the same accumulation with
    absolute values; the accumulation itself (mean of two samples, two products and a sum for the normal component, the
    length, the trapezoid's mean, NumPy's pairwise sum of s terms) rounds at most 7 + log2(s) times per term on either
    side: ``2 (7 + log2 s) u sum |term|`` more.
    Moment: the two backends form r_i - r_cm as ``xi (s - c)`` and ``xi s - xi c`` (4 u (|x| + |cx|) apart at the most)
    and K = K0 g_s + K0 g_n before or after the sum (3 u); with the products and the area 8 u per term, plus the
    difference in r, plus twice the summation-order bound ``n u sum |term|``."""
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import path_vectors

    sol = strip_solution
    device = sol.device
    sites, elements = device.points, device.triangles
    n = len(sites)
    U = sm.U
    rng = np.random.default_rng(17)
    pos = rng.uniform([-3.2, -1.7], [3.2, 1.7], size=(300, 2))  # generic points: inside, in the hole, beyond the rim
    ys = np.sort(rng.uniform(-1.49, 1.49, 160))
    path = np.column_stack([-1.5 + 1e-3 * rng.uniform(-1, 1, len(ys)), ys])  # a cut across the strip, upwards
    inside = device.contains_points(pos)
    assert 20 < np.count_nonzero(~inside) < 150
    triangle, lam = sm.locate(sites, elements, pos)
    ptri, plam = sm.locate(sites, elements, path)
    assert np.all(ptri >= 0) and np.all(plam > 1e-9) and np.all(lam[triangle >= 0] > 1e-9)  # not on edges
    mesh, xi = device.mesh, device.coherence_length
    com = xi * ((mesh.sites * mesh.areas[:, None]).sum(axis=0) / mesh.areas.sum())
    lengths, normals = path_vectors(path)
    centres_inside = device.contains_points((path[:-1] + path[1:]) / 2)
    assert centres_inside.all()
    steps = range(len(sol.saved_steps))
    host = {key: [] for key in ("J", "psi", "I", "M")}
    with tdgl.CurrentSampler(device, pos, device_id=sol.options.device_id) as at_points, \
            tdgl.CurrentSampler(device, path, device_id=sol.options.device_id) as on_path:
        t_dev, lam_dev = at_points.location()
        assert np.array_equal(t_dev, triangle) and lam_dev.tobytes() == lam.tobytes()
        for step in steps:
            sol.load_tdgl_data(step)
            for dataset, units in ((None, None), ("supercurrent", "mA / mm"), ("normal_current", "uA / nm"), (None, "A / m")):
                want = sol.interp_current_density(pos, dataset=dataset, units=units)
                got = sol.interp_current_density(pos, dataset=dataset, units=units, backend="hip")
                kept = sol.interp_current_density(pos, dataset=dataset, units=units, backend="hip", sampler=at_points)
                assert got.tobytes() == kept.tobytes() and got.shape == want.shape == (300, 2)
                V = {None: np.abs(sol.supercurrent_density) + np.abs(sol.normal_current_density),
                     "supercurrent": sol.supercurrent_density,
                     "normal_current": sol.normal_current_density}[dataset] * sol._density_factor(units)
                bound = 8 * U * (np.abs(lam)[:, :, None] * np.abs(V[elements[np.maximum(triangle, 0)]])).sum(axis=1)
                bound[~inside | (triangle < 0)] = 0.0  # zero in both
                within(got, want, bound, f"step {step} current density {dataset} {units}")
                assert np.all(got[~inside] == 0)
                if dataset is None and bound.max() > 0:  # for the record: against the bound of the total alone
                    T = np.abs(sol.current_density * sol._density_factor(units))
                    alone = 8 * U * (np.abs(lam)[:, :, None] * T[elements[np.maximum(triangle, 0)]]).sum(axis=1)
                    ratio = np.where(bound > 0, np.abs(got - want) / np.where(alone > 0, alone, 1.0), 0.0)
                    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
                    print(f"step {step} current density total {units}: max |hip - host| / (8 u sum |w (K_s + K_n)|) = "
                          f"{float(ratio[worst]):.3e}, there sum |w| (|K_s| + |K_n|) / sum |w (K_s + K_n)| = "
                          f"{float(bound[worst] / alone[worst]) if alone[worst] > 0 else np.inf:.3e}")
                q = sol.interp_current_density(pos, dataset=dataset, units=units, with_units=True, backend="hip")
                assert q.units == sol.interp_current_density(pos, dataset=dataset, units=units, with_units=True).units
            want = sol.interp_order_parameter(pos)
            got = sol.interp_order_parameter(pos, backend="hip", sampler=at_points)
            assert got.tobytes() == sol.interp_order_parameter(pos, backend="hip").tobytes()
            psi = sol.tdgl_data.psi
            corner = psi[elements[np.maximum(triangle, 0)]]
            bound = 8 * U * np.stack([(np.abs(lam) * np.abs(corner.real)).sum(axis=1),
                                      (np.abs(lam) * np.abs(corner.imag)).sum(axis=1)], axis=1)
            assert np.array_equal(np.isnan(got.real), triangle < 0) and np.array_equal(np.isnan(want.real), triangle < 0)
            ok = triangle >= 0
            within(np.stack([got.real, got.imag], axis=1)[ok], np.stack([want.real, want.imag], axis=1)[ok], bound[ok],
                   f"step {step} psi")
            # the current through the cut
            for dataset, units in ((None, None), ("supercurrent", "mA")):
                want = sol.current_through_path(path, dataset=dataset, units=units, with_units=False)
                got = sol.current_through_path(path, dataset=dataset, units=units, with_units=False, backend="hip")
                kept = sol.current_through_path(path, dataset=dataset, units=units, with_units=False, backend="hip", sampler=on_path)
                assert got == kept
                V = sol.supercurrent_density if dataset else np.abs(sol.supercurrent_density) + np.abs(sol.normal_current_density)
                bJ = 8 * U * (np.abs(plam)[:, :, None] * np.abs(V[elements[ptri]])).sum(axis=1)
                J = sol.interp_current_density(path, dataset=dataset)
                b_edge = (bJ[:-1] + bJ[1:]) / 2
                b_y = (b_edge * np.abs(normals)).sum(axis=1) * lengths
                y_abs = ((np.abs(J[:-1]) + np.abs(J[1:])) / 2 * np.abs(normals)).sum(axis=1) * lengths
                rounds = 2 * (7 + np.log2(len(y_abs))) * U
                bound = float(((b_y[1:] + b_y[:-1]) / 2).sum() + rounds * ((y_abs[1:] + y_abs[:-1]) / 2).sum())
                bound *= 1.0 if units is None else 1e-3  # uA -> mA
                within(got, want, bound, f"step {step} path current {dataset} {units}")
                if dataset is None:
                    host["I"].append(want)
                    assert sol.current_through_path(path, backend="hip").units == sol.current_through_path(path).units
            # the moment
            want = sol.magnetic_moment(with_units=False)
            got = sol.magnetic_moment(with_units=False, backend="hip")
            assert got == sol.magnetic_moment(with_units=False, backend="hip", sampler=on_path)
            assert sol.magnetic_moment(backend="hip").units == sol.magnetic_moment().units
            Ks, Kn = np.abs(sol.supercurrent_density), np.abs(sol.normal_current_density)
            K = Ks + Kn
            rx, ry = np.abs(sites[:, 0] - com[0]), np.abs(sites[:, 1] - com[1])
            dx, dy = 4 * U * (np.abs(sites[:, 0]) + abs(com[0])), 4 * U * (np.abs(sites[:, 1]) + abs(com[1]))
            scale = 0.5 * mesh.areas * xi**2
            terms = (rx * K[:, 1] + ry * K[:, 0]) * scale
            bound = float((8 * U * terms + (dx * K[:, 1] + dy * K[:, 0]) * scale).sum() + 2 * n * U * terms.sum())
            within(got, want, bound, f"step {step} moment")
            host["J"].append(sol.interp_current_density(pos))
            host["psi"].append(sol.interp_order_parameter(pos))
            host["M"].append(want)
        # every saved step in one call each: the frames are the single calls', to the bit
        saved = sol.saved_steps
        J_all = at_points.current_density(saved)
        psi_all = at_points.order_parameter(saved)
        I_all = on_path.path_current(saved)
        M_all = on_path.magnetic_moment(saved)
        K_all = on_path.site_current_density(saved)
        assert J_all.shape == (len(saved), 300, 2) and psi_all.shape == (len(saved), 300)
        assert on_path.stats()["frames"] == len(saved)
        for step in steps:
            sol.load_tdgl_data(step)
            assert J_all[step].tobytes() == at_points.current_density(sol).tobytes()
            assert J_all[step].tobytes() == at_points.current_density(saved[step]).tobytes()
            assert psi_all[step].tobytes() == at_points.order_parameter(saved[step].psi).tobytes()
            assert I_all[step] == on_path.path_current(sol) and M_all[step] == on_path.magnetic_moment(sol)
            assert K_all[step].tobytes() == np.ascontiguousarray(sol.current_density).tobytes()  # get_quantity_on_site's bits
            arrays = (np.stack([s.supercurrent for s in saved]), np.stack([s.normal_current for s in saved]))
            assert at_points.current_density(arrays)[step].tobytes() == J_all[step].tobytes()
        # the cut carries the applied current (the reference's own tolerance); the first saved step is the initial
        # state, before any step: no current yet
        assert saved[0].time == 0 and I_all[0] == 0 and len(I_all) >= 3
        assert np.allclose(I_all[1:], 12.0, rtol=0.1), I_all
        assert np.allclose(host["I"][1:], 12.0, rtol=0.1)
        with pytest.raises(ValueError, match="Unexpected dataset"):
            at_points.current_density(sol, dataset="nonsense")
        with pytest.raises(TypeError):
            at_points.current_density(np.zeros(3))
    with tdgl.CurrentSampler(device, device_id=sol.options.device_id) as bare:
        assert bare.magnetic_moment(sol) == M_all[-1]
        with pytest.raises(ValueError, match="without positions"):
            bare.current_density(sol)
