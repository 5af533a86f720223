"""Vortex cores and loop windings on the device (csrc/vortices.inc, `hipcore.VortexPlan`, `tdgl_amd.VortexFinder`,
``backend="hip"`` of `Solution.vortices` / `Solution.boundary_windings`) against the NumPy model of
tests/vortex_model.py: counts, triangles, charges, their order and the windings for EQUALITY (every sign decision
compares two separately rounded products), core positions within the model's derived bound
``8 u (kappa + 1) r_max``."""

import ctypes as C

import numpy as np
import pytest

import vortex_model as vm

pytestmark = pytest.mark.gpu


def random_case(n_tri, n_frames, seed, n_sites=None):
    """Random sites, random index triples as triangles (about a quarter of them wind) and Gaussian psi."""
    rng = np.random.default_rng(seed)
    n_sites = n_sites or max(8, min(n_tri, 4000))
    sites = rng.uniform(-7.0, 9.0, size=(n_sites, 2))
    elements = rng.integers(0, n_sites, size=(n_tri, 3)).astype(np.int32)
    psi = rng.normal(size=(n_frames, n_sites)) + 1j * rng.normal(size=(n_frames, n_sites))
    return sites, elements, psi


def assert_records(got, want):
    counts, triangles, charges, xy = got[:4]
    assert np.array_equal(counts, want["counts"])
    assert np.array_equal(triangles, want["triangle"]) and np.array_equal(charges, want["charge"])
    assert xy.shape == want["xy"].shape
    if len(xy):
        assert np.all(np.abs(xy - want["xy"]).max(axis=1) <= want["bound"])


def raw_find(plan, psi, capacity, counts=True, records=True, xy=True, windings=False, fill=-77):
    """`tdgl_vortex_plan_find` with buffers prefilled with ``fill``; None instead of the outputs not asked for."""
    from tdgl_amd import _lib

    psi = np.ascontiguousarray(psi, dtype=complex)
    out_counts = np.full(len(psi), fill, dtype=np.int64) if counts else None
    out_tc = np.full((capacity, 2), fill, dtype=np.int32) if records else None
    out_xy = np.full((capacity, 2), float(fill)) if xy else None
    out_w = np.full((len(psi), plan.n_loops), fill, dtype=np.int32) if windings else None
    _lib.check(plan._lib.tdgl_vortex_plan_find(plan._plan, len(psi), _lib.p_f64(psi), capacity, _lib.p_i64(out_counts),
                                               _lib.p_i32(out_tc), _lib.p_f64(out_xy), _lib.p_i32(out_w)))
    return out_counts, out_tc, out_xy, out_w


@pytest.mark.parametrize("n_frames", [1, 3])
@pytest.mark.parametrize("n_tri", [1, 63, 64, 65, 257, 70_001])
def test_plan_against_the_model(n_tri, n_frames):
    from tdgl_amd.hipcore import VortexPlan

    sites, elements, psi = random_case(n_tri, n_frames, seed=1012 + n_tri + n_frames)
    want = vm.find(psi, sites, elements)
    total = int(want["counts"].sum())
    if n_tri >= 63:  # about a quarter of the triangles wind
        assert 0.15 * n_tri * n_frames < total < 0.35 * n_tri * n_frames
    else:  # (the seed is one at which the single triangle does)
        assert total >= 1
    with VortexPlan(sites, elements) as plan:
        first = plan.find(psi)
        assert_records(first, want)
        assert first[4] is not None and first[4].shape == (n_frames, 0)
        stats = plan.stats()
        assert stats["found"] == total and stats["frames"] == n_frames and stats["chunks"] == 1 and stats["last_ms"] >= 0
        second = plan.find(psi)
        for a, b in zip(first[:4], second[:4]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        # NULL outputs are left alone, and the others do not depend on them
        cap = total + 3
        full = raw_find(plan, psi, cap)
        assert np.array_equal(full[0], want["counts"]) and np.array_equal(full[1][:total, 0], want["triangle"])
        assert np.all(full[1][total:] == -77) and np.all(full[2][total:] == -77.0)  # nothing beyond the records
        only_counts = raw_find(plan, psi, cap, records=False, xy=False)
        assert np.array_equal(only_counts[0], want["counts"]) and only_counts[1] is None and only_counts[2] is None
        only_records = raw_find(plan, psi, cap, counts=False, xy=False)
        assert only_records[0] is None and only_records[1].tobytes() == full[1].tobytes()
        only_xy = raw_find(plan, psi, cap, counts=False, records=False)
        assert only_xy[2].tobytes() == full[2].tobytes()
        nothing = raw_find(plan, psi, cap, counts=False, records=False, xy=False)
        assert nothing == (None, None, None, None)


def test_frames_in_several_chunks_give_the_same_records(monkeypatch):
    from tdgl_amd.hipcore import VortexPlan

    sites, elements, psi = random_case(1000, 5, seed=21)
    loops = [np.arange(10), np.arange(700, 0, -3)]
    want = vm.find(psi, sites, elements)
    monkeypatch.setenv("TDGL_VORTEX_CHUNK", "2")
    with VortexPlan(sites, elements, loops) as plan:
        got = plan.find(psi)
        assert plan.stats()["chunks"] == 3 and plan.stats()["frames"] == 5
        assert_records(got, want)
        assert np.array_equal(got[4], vm.windings(psi, loops))
        assert np.array_equal(plan.windings(psi), got[4])


def test_zeros_and_nans_give_the_models_answer():
    from tdgl_amd.hipcore import VortexPlan

    sites, elements, psi = random_case(5000, 2, seed=31, n_sites=300)
    rng = np.random.default_rng(32)
    psi[0, rng.choice(300, 40, replace=False)] = 0.0
    psi[1, rng.choice(300, 20, replace=False)] = complex(np.nan, 1.0)
    psi[1, rng.choice(300, 20, replace=False)] = complex(0.5, np.nan)
    psi[0, rng.choice(300, 10, replace=False)] = complex(0.0, 1.0)  # (one part zero is an ordinary value)
    want = vm.find(psi, sites, elements)
    assert 100 < want["counts"].sum() < 0.25 * 2 * 5000 and np.isfinite(want["xy"]).all()
    with VortexPlan(sites, elements) as plan:
        assert_records(plan.find(psi), want)


def test_psi_identically_zero_gives_no_record():
    from tdgl_amd.hipcore import VortexPlan

    sites, elements, psi = random_case(300, 2, seed=41)
    with VortexPlan(sites, elements, [np.arange(5)]) as plan:
        counts, triangles, charges, xy, windings = plan.find(np.zeros_like(psi))
        assert counts.tolist() == [0, 0] and len(triangles) == len(charges) == len(xy) == 0
        assert windings.tolist() == [[vm.WINDING_UNDEFINED], [vm.WINDING_UNDEFINED]]
        untouched = raw_find(plan, np.zeros_like(psi), 4)
        assert untouched[0].tolist() == [0, 0] and np.all(untouched[1] == -77) and np.all(untouched[2] == -77.0)


def test_capacity_at_and_below_the_count():
    from tdgl_amd.hipcore import VortexPlan

    sites, elements, psi = random_case(3000, 3, seed=51)
    want = vm.find(psi, sites, elements)
    total = int(want["counts"].sum())
    assert total > 1024  # (above what VortexPlan.find tries first: it has to retry)
    with VortexPlan(sites, elements) as plan:
        exact = raw_find(plan, psi, total)
        assert np.array_equal(exact[0], want["counts"])
        assert np.array_equal(exact[1][:, 0], want["triangle"]) and np.array_equal(exact[1][:, 1], want["charge"])
        assert np.all(np.abs(exact[2] - want["xy"]).max(axis=1) <= want["bound"])
        below = raw_find(plan, psi, total - 1)
        assert np.array_equal(below[0], want["counts"])  # the true counts all the same
        assert below[1].tobytes() == exact[1][:-1].tobytes() and below[2].tobytes() == exact[2][:-1].tobytes()
        few = raw_find(plan, psi, 5)
        assert np.array_equal(few[0], want["counts"]) and few[1].tobytes() == exact[1][:5].tobytes()
        none = raw_find(plan, psi, 0)
        assert np.array_equal(none[0], want["counts"]) and none[1].shape == (0, 2)
        # find(): one retry with the exact capacity
        calls = []
        once = plan.find_once
        plan.find_once = lambda *a, **k: (calls.append(a[1]), once(*a, **k))[1]
        got = plan.find(psi)
        assert calls == [1024, total] and plan.last_capacity == total
        assert_records(got, want)
        calls.clear()
        plan.find(psi)
        assert calls == [total]
        from tdgl_amd import _lib

        with pytest.raises(ValueError, match="negative capacity"):
            raw_find(plan, psi, -1, records=False, xy=False)
        assert plan._lib.tdgl_vortex_plan_find(plan._plan, 0, _lib.p_f64(psi), 1, None, None, None, None) == _lib.TDGL_ERR_ARG
        assert b"n_frames" in plan._lib.tdgl_last_error(None)


def test_loops_of_every_length_against_the_model():
    from tdgl_amd.hipcore import VortexPlan

    rng = np.random.default_rng(61)
    n_sites = 90_000
    sites = rng.uniform(-1, 1, size=(n_sites, 2))
    lengths = [3, 63, 64, 65, 1000, 70_001, 3, 200]
    order = rng.permutation(n_sites)  # disjoint loops: what is planted in one does not reach another
    loops = np.split(order[:sum(lengths)], np.cumsum(lengths)[:-1])
    # smooth fields with a few zeros (a Gaussian psi would wind ~sqrt(length) times: a weaker check of long loops), and
    # sites with zeros, so that loops wind by small known numbers
    theta = np.linspace(0, 2 * np.pi, n_sites, endpoint=False)
    psi = np.stack([np.exp(3j * theta) * (1 + 0.3 * rng.uniform(-1, 1, size=n_sites)),
                    rng.normal(size=n_sites) + 1j * rng.normal(size=n_sites),
                    np.round(2 * rng.normal(size=n_sites)) / 2 + 0.5j * np.round(2 * rng.normal(size=n_sites))])
    for k in (4, 5):  # loops along the site order: the first frame winds 3 times around them
        loops[k] = np.sort(loops[k])
    psi[:2, loops[6][1]] = 0.0                      # undefined: a vertex is zero
    psi[:2, loops[7][[5, 6]]] = [1 + 1j, -2 - 2j]   # undefined: an edge through the origin
    psi[2, loops[7][5]] = complex(1.0, np.nan)
    want = vm.windings(psi, loops)
    assert want[0, 4] == 3 and want[0, 5] == 3
    assert np.all(want[:2, 6:] == vm.WINDING_UNDEFINED) and np.all(want[:2, :6] != vm.WINDING_UNDEFINED)
    assert want[2, 7] == vm.WINDING_UNDEFINED
    with VortexPlan(sites, np.zeros((0, 3), dtype=np.int32), loops) as plan:
        assert np.array_equal(plan.windings(psi), want)
        counts, triangles, charges, xy, windings = plan.find(psi)
        assert counts.tolist() == [0, 0, 0] and len(triangles) == 0 and np.array_equal(windings, want)
        assert np.array_equal(plan.windings(psi[1]), want[1:2])


def test_create_refusals_come_back_by_message():
    from tdgl_amd.hipcore import VortexPlan

    sites = np.random.default_rng(71).uniform(size=(10, 2))
    tri = np.array([[0, 1, 2], [3, 4, 5]])
    with pytest.raises(ValueError, match="element 1 names site 10, out of range"):
        VortexPlan(sites, np.array([[0, 1, 2], [3, 10, 5]]))
    with pytest.raises(ValueError, match="out of range"):
        VortexPlan(sites, np.array([[0, -1, 2]]))
    with pytest.raises(ValueError, match="loop 1 has 2 sites, a loop needs at least 3"):
        VortexPlan(sites, tri, [[0, 1, 2], [3, 4]])
    with pytest.raises(ValueError, match="loop site 12 out of range"):
        VortexPlan(sites, tri, [[0, 1, 12]])
    with pytest.raises(ValueError, match=r"sites \[n, 2\]"):
        VortexPlan(sites.T, tri)
    with pytest.raises(ValueError, match="no HIP device 4096"):
        VortexPlan(sites, tri, device_id=4096)
    with VortexPlan(sites, tri, [[0, 1, 2]]) as plan:
        with pytest.raises(ValueError, match="psi of shape"):
            plan.find(np.ones(9, dtype=complex))
    with pytest.raises(RuntimeError, match="closed"):
        plan.find(np.ones(10, dtype=complex))
    lib = plan._lib
    out = C.c_void_p()
    from tdgl_amd import _lib

    assert lib.tdgl_vortex_plan_create(C.byref(out), 0, -3, None, 0, None, 0, None, None) == _lib.TDGL_ERR_ARG
    assert b"negative size" in lib.tdgl_last_error(None) and not out.value


@pytest.fixture(scope="module")
def field_run():
    """One short solve of the 516-site film of the `traj_field_small` set-up (b = 0.5 Bc2), past vortex entry."""
    import tdgl_amd as tdgl
    from test_vortices_host import small_device

    device = small_device()
    options = tdgl.SolverOptions(solve_time=8.5, dt_init=1e-4, save_every=50, field_units="mT")
    solution = tdgl.solve(device, options, applied_vector_potential=0.5 * device.Bc2 / 1e-3)
    return device, solution


def test_end_to_end_on_a_solve_past_vortex_entry(field_run):
    import tdgl_amd as tdgl

    device, solution = field_run
    steps = solution.saved_steps
    assert len(steps) >= 5
    loops = device.boundary_sites()
    elements = device.triangles
    orient = vm.orientations(device.points, elements)
    host = solution.vortices(backend="host")
    hip = solution.vortices(backend="hip")
    assert len(host.charges) >= 10  # vortices have entered
    assert np.array_equal(hip.triangles, host.triangles) and np.array_equal(hip.charges, host.charges)
    assert hip.triangles.dtype == host.triangles.dtype and hip.charges.dtype == host.charges.dtype
    bound = vm.position_bound(solution.tdgl_data.psi, device.points, elements, host.triangles)
    assert np.all(np.abs(hip.positions - host.positions).max(axis=1) <= bound)
    assert solution.boundary_windings(backend="hip") == solution.boundary_windings(backend="host")
    assert solution.boundary_windings()["film"] == int(host.charges.sum()) > 0
    with tdgl.VortexFinder(device, device_id=solution.options.device_id) as finder:
        together = finder.find(steps)
        windings = finder.windings(steps)
        assert finder.stats()["frames"] == len(steps)
        assert len(together) == len(windings) == len(steps)
        entered = 0
        for k, step in enumerate(steps):
            alone = finder.find(step)
            for a, b in zip(alone, together[k]):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
            assert finder.windings(step.psi) == windings[k]
            # the discrete Stokes identity, exactly, on every saved step
            assert list(windings[k]) == ["film"] and windings[k]["film"] == int(together[k].charges.sum())
            want = vm.find(step.psi, device.points, elements, orient)
            assert np.array_equal(together[k].triangles, want["triangle"]) and np.array_equal(together[k].charges, want["charge"])
            assert windings[k]["film"] == vm.winding(step.psi, loops["film"])
            entered += len(alone.charges) > 0
        assert entered >= 2
        solution.load_tdgl_data(1)
        assert finder.find(solution).triangles.tobytes() == together[1].triangles.tobytes()
        many = finder.find(np.stack([s.psi for s in steps]))
        assert all(a.positions.tobytes() == b.positions.tobytes() for a, b in zip(many, together))
        with pytest.raises(TypeError):
            finder.find(np.zeros((2, 2, 2)))
