"""Linking vortex cores into tracks on the device (`tdgl_vortex_plan_link`, `hipcore.VortexPlan.link`,
`tdgl.VortexFinder.tracks`, ``tdgl.track_vortices(..., backend="hip")``; csrc/vortices.inc) against the plain-loop model
of tests/track_model.py: every output for EQUALITY (each decision compares identically rounded doubles), into buffers
prefilled with a sentinel so that an entry nobody wrote shows."""

import numpy as np
import pytest

import track_model as tm

pytestmark = pytest.mark.gpu

FILL = -77
# one triangle and, after its sites, a prescribed loop of five sites that no core sits on
SITES = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [-0.5, -0.5], [24.5, -0.5], [24.5, 24.5], [-0.5, 24.5], [11.5, -0.5]])
ELEMENTS = np.array([[0, 1, 2]], dtype=np.int32)
LOOP = np.array([3, 4, 5, 6, 7], dtype=np.int32)
OUTPUTS = tm.FIELDS


def open_plan(loops=(LOOP,)):
    from tdgl_amd.hipcore import VortexPlan

    return VortexPlan(SITES, ELEMENTS, list(loops))


def raw_link(plan, counts, xy, charges, r, skip=()):
    """`tdgl_vortex_plan_link` into prefilled buffers; None instead of the outputs named in ``skip``.  (status, dict)"""
    from tdgl_amd import _lib

    counts = np.asarray(counts, dtype=np.int64)
    total = max(int(counts.sum()), 0)
    out = {name: (None if name in skip else np.full(total, FILL, dtype=np.float64 if name == "near_d2" else np.int32))
           for name in OUTPUTS}
    status = plan._lib.tdgl_vortex_plan_link(
        plan._plan, len(counts), _lib.p_i64(counts), _lib.p_f64(np.ascontiguousarray(xy, dtype=float)),
        _lib.p_i32(np.ascontiguousarray(charges, dtype=np.int32)), float(r),
        *[_lib.p_i32(out[name]) for name in OUTPUTS[:5]], _lib.p_f64(out["near_d2"]))
    return status, out


@pytest.fixture(scope="module")
def cases():
    """{(counts, floats): (xy, charges, the model's answer)}, computed once."""
    made = {}
    for counts in tm.COUNT_SEQUENCES:
        for floats in (False, True) if counts == tm.COUNT_SEQUENCES[2] else (False,):
            xy, charges = tm.random_case(counts, seed=5, floats=floats)
            made[tuple(counts), floats] = (xy, charges, tm.link(counts, xy, charges, 5.0, SITES[LOOP]))
    return made


@pytest.mark.parametrize("counts, floats", [(c, False) for c in tm.COUNT_SEQUENCES] + [(tm.COUNT_SEQUENCES[2], True)])
def test_raw_link_equals_the_model(cases, counts, floats):
    xy, charges, want = cases[tuple(counts), floats]
    with open_plan() as plan:
        status, got = raw_link(plan, counts, xy, charges, 5.0)
        assert status == 0
        tm.assert_equal([got[name] for name in OUTPUTS], want)
        stats = plan.link_stats()
        assert stats["links"] == want["links"] and stats["frames"] == len(counts) and stats["last_ms"] >= 0
        again = raw_link(plan, counts, xy, charges, 5.0)[1]
        assert all(got[name].tobytes() == again[name].tobytes() for name in OUTPUTS)
        wrapped = plan.link(counts, xy, charges, 5.0)
        tm.assert_equal(wrapped, want)


def test_the_integer_cases_hold_ties_exact_radii_and_choices_not_returned(cases):
    totals = dict(ties=0, at_radius=0, non_mutual=0, links=0)
    for (counts, floats), (_, _, want) in cases.items():
        if not floats:
            for name in totals:
                totals[name] += want[name]
    print("over the integer cases:", totals)
    assert all(v > 0 for v in totals.values())
    big = cases[tuple(tm.COUNT_SEQUENCES[2]), False][2]
    assert big["ties"] > 0 and big["at_radius"] > 0 and big["non_mutual"] > 0 and big["links"] > 0
    assert np.any(big["end_partner"] >= 0) and np.any(big["start_partner"] >= 0)


def test_launches_in_several_chunks_of_jobs_give_the_same(cases, monkeypatch):
    counts = tm.COUNT_SEQUENCES[1]
    xy, charges, want = cases[tuple(counts), False]
    many = [3, 2, 4, 0, 5, 1, 6, 2, 3]
    xy9, charges9 = tm.random_case(many, seed=6)
    want9 = tm.link(many, xy9, charges9, 5.0, SITES[LOOP])
    assert want9["links"] > 0
    with open_plan() as plan:
        whole = plan.link(many, xy9, charges9, 5.0)
        launches = plan.link_stats()["launches"]
    monkeypatch.setenv("TDGL_VORTEX_LINK_JOBS", "2")
    with open_plan() as plan:
        tm.assert_equal(plan.link(many, xy9, charges9, 5.0), want9)
        assert plan.link_stats()["launches"] > launches
        tm.assert_equal(plan.link(counts, xy, charges, 5.0), want)
    tm.assert_equal(whole, want9)


def test_outputs_passed_as_null_leave_the_others_unchanged(cases):
    counts = tm.COUNT_SEQUENCES[1]
    xy, charges, want = cases[tuple(counts), False]
    with open_plan() as plan:
        full = raw_link(plan, counts, xy, charges, 5.0)[1]
        for name in OUTPUTS:
            status, got = raw_link(plan, counts, xy, charges, 5.0, skip=(name,))
            assert status == 0 and got[name] is None
            assert all(got[other].tobytes() == full[other].tobytes() for other in OUTPUTS if other != name), name
        only_near = raw_link(plan, counts, xy, charges, 5.0, skip=OUTPUTS[:4])[1]
        assert only_near["near"].tobytes() == full["near"].tobytes() and plan.link_stats()["links"] == 0
        assert plan.link_stats()["launches"] == 1  # work nobody asked for is not launched
        status, nothing = raw_link(plan, counts, xy, charges, 5.0, skip=OUTPUTS)
        assert status == 0 and plan.link_stats()["launches"] == 0 and plan.link_stats()["frames"] == len(counts)
    with open_plan(loops=()) as plan:  # a plan without loops
        status, got = raw_link(plan, counts, xy, charges, 5.0)
        assert status == 0 and np.all(got["near"] == -1) and np.all(got["near_d2"] == np.inf)
        assert got["next"].tobytes() == want["next"].tobytes() and got["end_partner"].tobytes() == want["end_partner"].tobytes()
        status, got = raw_link(plan, [3], xy[:3], charges[:3], 5.0)  # a single frame: nothing to launch at all
        assert status == 0 and plan.link_stats()["launches"] == 0
        assert all(np.all(got[name] == -1) for name in OUTPUTS[:5]) and np.all(got["near_d2"] == np.inf)


def test_nan_and_infinite_positions_equal_the_model():
    counts = [70, 70, 70]
    xy, charges = tm.random_case(counts, seed=7)
    rng = np.random.default_rng(8)
    xy[rng.choice(210, 12, replace=False), 0] = np.nan
    xy[rng.choice(210, 6, replace=False), 1] = np.inf
    want = tm.link(counts, xy, charges, 5.0, SITES[LOOP])
    assert want["links"] > 0 and np.count_nonzero(want["near"] == -1) >= 12
    with open_plan() as plan:
        tm.assert_equal(plan.link(counts, xy, charges, 5.0), want)


def test_refusals_come_back_by_status_and_message():
    from tdgl_amd import _lib

    xy, charges = tm.random_case([2, 2], seed=9)
    with open_plan() as plan:
        lib = plan._lib

        def refused(match, counts=(2, 2), xy=xy, charges=charges, r=1.0, n_frames=None, null=()):
            counts = np.asarray(counts, dtype=np.int64)
            args = dict(counts=_lib.p_i64(counts), xy=_lib.p_f64(np.ascontiguousarray(xy)), charges=_lib.p_i32(np.ascontiguousarray(charges, dtype=np.int32)))
            for name in null:
                args[name] = None
            out = np.full(8, FILL, dtype=np.int32)
            status = lib.tdgl_vortex_plan_link(plan._plan, len(counts) if n_frames is None else n_frames, args["counts"],
                                               args["xy"], args["charges"], r, _lib.p_i32(out), None, None, None, None, None)
            assert status == _lib.TDGL_ERR_ARG and match in lib.tdgl_last_error(None), lib.tdgl_last_error(None)
            assert np.all(out == FILL)

        refused(b"null counts", null=("counts",))
        refused(b"null xy or charges", null=("xy",))
        refused(b"null xy or charges", null=("charges",))
        refused(b"n_frames", n_frames=0)
        refused(b"negative count", counts=(2, -1))
        refused(b"2^31", counts=(2 ** 30, 2 ** 30))
        refused(b"2^31", counts=(2 ** 40,))
        refused(b"neither +1 nor -1", charges=np.array([1, 0, 1, 1]))
        refused(b"neither +1 nor -1", charges=np.array([1, 1, 1, 2]))
        for r in (-1.0, float("nan"), float("inf")):
            refused(b"max_distance", r=r)
        assert lib.tdgl_vortex_plan_link(None, 1, None, None, None, 1.0, *[None] * 6) == _lib.TDGL_ERR_ARG
        assert b"null plan" in lib.tdgl_last_error(None)
        # frames without cores need neither xy nor charges, and the plan is still usable
        empty = np.zeros(3, dtype=np.int64)
        assert lib.tdgl_vortex_plan_link(plan._plan, 3, _lib.p_i64(empty), None, None, 1.0, *[None] * 6) == 0
        with pytest.raises(ValueError, match="max_distance"):
            plan.link([2, 2], xy, charges, -1.0)
        with pytest.raises(ValueError, match="for these counts"):
            plan.link([2, 3], xy, charges, 1.0)
        assert len(plan.link([2, 2], xy, charges, 1.0)[0]) == 4
    with pytest.raises(RuntimeError, match="closed"):
        plan.link([2, 2], xy, charges, 1.0)


def test_link_leaves_the_stats_of_find_alone():
    rng = np.random.default_rng(10)
    psi = rng.normal(size=(2, len(SITES))) + 1j * rng.normal(size=(2, len(SITES)))
    xy, charges = tm.random_case([5, 6], seed=11)
    with open_plan() as plan:
        plan.find(psi)
        before = plan.stats()
        assert before["frames"] == 2 and before["launches"] > 0
        plan.link([5, 6], xy, charges, 5.0)
        assert plan.stats() == before
        want = tm.link([5, 6], xy, charges, 5.0, SITES[LOOP])
        stats = plan.link_stats()
        assert stats["links"] == want["links"] and stats["frames"] == 2 and stats["pairs"] >= 2 * 5 * 6 + 11 * len(LOOP)


@pytest.fixture(scope="module")
def small():
    from test_vortices_host import small_device

    return small_device()


def test_synthetic_scenario_through_the_finder(small):
    import tdgl_amd as tdgl

    psi = tm.scenario_psi(small.points)
    times = np.linspace(0.0, 5.5, tm.SCENARIO_FRAMES)
    host = tdgl.track_vortices(small, psi, tm.SCENARIO_R, times=times, backend="host")
    with tdgl.VortexFinder(small) as finder:
        hip = finder.tracks(psi, tm.SCENARIO_R, times=times)
        assert finder.link_stats()["frames"] == tm.SCENARIO_FRAMES and finder.link_stats()["links"] == 11 + 8 + 5 + 5
    tm.assert_scenario(hip)
    tm.assert_scenario(host)
    for name, a, b in zip(OUTPUTS[:5], hip.links, host.links):  # (the positions, and so near_d2, agree within a bound only)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    via = tdgl.track_vortices(small, psi, tm.SCENARIO_R, times=times, backend="hip")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(via.links, hip.links))
    with pytest.raises(TypeError):
        tdgl.VortexFinder.tracks(finder, psi)
    with pytest.raises(ValueError, match="max_distance"):
        tdgl.track_vortices(small, psi, -1.0, backend="hip")


@pytest.fixture(scope="module")
def field_run(small):
    """One short solve of the 516-site film of the `traj_field_small` set-up (b = 0.5 Bc2), past vortex entry."""
    import tdgl_amd as tdgl

    options = tdgl.SolverOptions(solve_time=8.5, dt_init=1e-4, save_every=50, field_units="mT")
    return tdgl.solve(small, options, applied_vector_potential=0.5 * small.Bc2 / 1e-3)


def test_tracks_of_a_solve_past_vortex_entry(small, field_run):
    import tdgl_amd as tdgl

    solution = field_run
    r = 3 * float(small.mesh.edge_mesh.edge_lengths.mean())
    host = tdgl.track_vortices(small, solution, r, backend="host")
    hip = tdgl.track_vortices(small, solution, r, backend="hip", device_id=solution.options.device_id)
    assert len(hip.frames) == len(solution.saved_steps) >= 5
    assert np.array_equal(hip.times, [step.time for step in solution.saved_steps])
    for name, a, b in zip(OUTPUTS[:5], hip.links, host.links):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    total = sum(len(v.charges) for v in hip.frames)
    assert total >= 10 and sum(len(t.frame_indices) for t in hip.tracks) == total
    seen = {(int(f), int(i)) for t in hip.tracks for f, i in zip(t.frame_indices, t.core_indices)}
    assert len(seen) == total  # every core in exactly one track
    for t in hip.tracks:
        assert all(hip.frames[f].charges[i] == t.charge for f, i in zip(t.frame_indices, t.core_indices))
        assert np.all(np.diff(t.frame_indices) == 1)
    entered = [t for t in hip.tracks if t.start.kind == "boundary" and t.start.loop == "film"]
    print(len(hip.tracks), "tracks,", len(entered), "entered through the rim; kinds:",
          sorted({(t.start.kind, t.end.kind) for t in hip.tracks}))
    assert len(entered) >= 1  # the vortices came in through the rim
    assert [(t.start.kind, t.start.loop, t.end.kind, t.end.partner) for t in hip.tracks] == \
        [(t.start.kind, t.start.loop, t.end.kind, t.end.partner) for t in host.tracks]
