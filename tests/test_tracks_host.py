"""Linking vortex cores into tracks, the parts that need no GPU: `tdgl_amd.vortices.link_frames` (vectorised NumPy, the
host backend) against the plain-loop model of tests/track_model.py for EQUALITY; hand-made cases with the expected
arrays written out; a synthetic scenario (one vortex at rest, one leaving through the rim, a pair annihilating) through
`tdgl.track_vortices`; the Python refusals.  The device path: tests/test_hip_tracks.py."""

import numpy as np
import pytest

import track_model as tm


def frames_of(counts, xy, charges):
    ends = np.cumsum(counts)
    return [(xy[e - c:e], charges[e - c:e]) for c, e in zip(counts, ends)]


def link(counts, xy, charges, r, loop_xy=None):
    """`link_frames` on a case given as the C entry takes it, checked against the model on the way."""
    from tdgl_amd.vortices import link_frames

    xy, charges = np.asarray(xy, dtype=float).reshape(-1, 2), np.asarray(charges, dtype=np.int32)
    got = link_frames(frames_of(counts, xy, charges), r, loop_xy)
    tm.assert_equal(got, tm.link(counts, xy, charges, r, loop_xy))
    return got


LOOP_XY = np.array([[0.0, 0.0], [24.0, 0.0], [24.0, 24.0], [0.0, 24.0], [12.0, 0.0]])


@pytest.mark.parametrize("floats", [False, True])
@pytest.mark.parametrize("counts", tm.COUNT_SEQUENCES)
def test_link_frames_equals_the_plain_loop_model(counts, floats, monkeypatch):
    import tdgl_amd.vortices as tv

    xy, charges = tm.random_case(counts, seed=5, floats=floats)
    want = tm.link(counts, xy, charges, 5.0, LOOP_XY)
    if not floats and sum(counts) > 500:  # the equality cannot pass vacuously
        assert want["ties"] > 0 and want["at_radius"] > 0 and want["non_mutual"] > 0 and want["links"] > 0
    tm.assert_equal(tv.link_frames(frames_of(counts, xy, charges), 5.0, LOOP_XY), want)
    monkeypatch.setattr(tv, "LINK_BLOCK", 7)  # ... nor depend on how the sources are blocked
    tm.assert_equal(tv.link_frames(frames_of(counts, xy, charges), 5.0, LOOP_XY), want)
    no_loops = tv.link_frames(frames_of(counts, xy, charges), 5.0)
    assert np.all(no_loops.near == -1) and np.all(no_loops.near_d2 == np.inf)
    assert no_loops.next.tobytes() == want["next"].tobytes()


def test_equal_distances_go_to_the_lower_index():
    got = link([1, 3], [[0, 0], [0, 1], [1, 0], [-1, 0]], [1, 1, 1, 1], 5.0)
    assert got.next.tolist() == [0, -1, -1, -1] and got.prev.tolist() == [-1, 0, -1, -1]


def test_a_target_at_exactly_the_radius_links_and_one_ulp_beyond_does_not():
    got = link([1, 1], [[1, 1], [4, 5]], [1, 1], 5.0)
    assert got.next.tolist() == [0, -1] and got.prev.tolist() == [-1, 0]
    beyond = 1 + 2.0 ** -52  # the same offset stretched to r (1 + 2^-52)
    assert 3 * beyond > 3 and 4 * beyond > 4
    got = link([1, 1], [[0, 0], [3 * beyond, 4 * beyond]], [1, 1], 5.0)
    assert got.next.tolist() == [-1, -1] and got.prev.tolist() == [-1, -1]
    got = link([1, 1], [[1, 1], [4, 5]], [1, 1], float(np.nextafter(5.0, 0.0)))  # ... and a radius one ulp short
    assert got.next.tolist() == [-1, -1] and got.prev.tolist() == [-1, -1]


def test_a_nearer_core_of_opposite_charge_is_ignored():
    got = link([1, 2], [[0, 0], [0.5, 0], [2, 0]], [1, -1, 1], 5.0)
    assert got.next.tolist() == [1, -1, -1] and got.prev.tolist() == [-1, -1, 0]


def test_a_choice_that_is_not_returned_links_nothing():
    # A = (0, 0) in frame 0 chooses B = (2, 0); B's nearest in frame 0 is C = (3, 0)
    got = link([2, 1], [[0, 0], [3, 0], [2, 0]], [1, 1, 1], 5.0)
    assert got.next.tolist() == [-1, 0, -1] and got.prev.tolist() == [-1, -1, 1]


def test_an_empty_frame_ends_every_track():
    got = link([2, 0, 2], [[0, 0], [5, 5], [0, 0], [5, 5]], [1, -1, 1, -1], 50.0)
    assert got.next.tolist() == [-1] * 4 and got.prev.tolist() == [-1] * 4
    # the two ends of frame 0 are an opposite pair within reach: an annihilation; the two starts of frame 2 likewise
    assert got.end_partner.tolist() == [1, 0, -1, -1] and got.start_partner.tolist() == [-1, -1, 1, 0]


def test_a_single_frame_links_nothing():
    got = link([3], [[0, 0], [1, 0], [0, 1]], [1, -1, 1], 5.0, LOOP_XY)
    for a in got[:4]:
        assert a.tolist() == [-1, -1, -1]
    assert got.near.tolist() == [0, 0, 0] and got.near_d2.tolist() == [0.0, 1.0, 1.0]


def test_a_nan_position_links_to_nothing_and_is_nobodys_target():
    nan = float("nan")
    got = link([2, 2], [[0, 0], [nan, 1], [nan, 0], [0, 1]], [1, 1, 1, 1], 5.0, LOOP_XY)
    assert got.next.tolist() == [1, -1, -1, -1] and got.prev.tolist() == [-1, -1, -1, 0]
    assert got.near.tolist() == [0, -1, -1, 0] and got.near_d2.tolist() == [0.0, np.inf, np.inf, 1.0]
    got = link([1, 1], [[0, 0], [np.inf, 0]], [1, 1], 5.0)
    assert got.next.tolist() == [-1, -1]


def test_mutually_nearest_opposite_ends_are_partners():
    # frame 0: + at (0, 0), - at (1, 0), + at (10, 10); frame 1: only the far + is left
    got = link([3, 1], [[0, 0], [1, 0], [10, 10], [10, 10]], [1, -1, 1, 1], 2.0)
    assert got.next.tolist() == [-1, -1, 0, -1] and got.prev.tolist() == [-1, -1, -1, 2]
    assert got.end_partner.tolist() == [1, 0, -1, -1] and got.start_partner.tolist() == [-1] * 4


def test_of_a_chain_of_three_ends_only_the_mutual_two_pair():
    # ends + (0, 0), - (1.5, 0), + (2.5, 0): the first chooses the second, which chooses the third, which chooses it back
    got = link([3, 0], [[0, 0], [1.5, 0], [2.5, 0]], [1, -1, 1], 2.0)
    assert got.end_partner.tolist() == [-1, 2, 1]
    # a core that goes on is no end, however near
    got = link([3, 1], [[0, 0], [1.5, 0], [2.5, 0], [2.5, 0]], [1, -1, 1, 1], 2.0)
    assert got.next.tolist() == [-1, -1, 0, -1] and got.end_partner.tolist() == [1, 0, -1, -1]


@pytest.fixture(scope="module")
def scenario():
    from test_vortices_host import small_device

    device = small_device()
    assert len(device.points) == 516
    return device, tm.scenario_psi(device.points)


def test_synthetic_scenario_gives_the_four_tracks(scenario):
    import tdgl_amd as tdgl

    device, psi = scenario
    times = np.linspace(0.0, 5.5, tm.SCENARIO_FRAMES)
    tracks = tdgl.track_vortices(device, psi, tm.SCENARIO_R, times=times)
    assert isinstance(tracks, tdgl.VortexTracks) and len(tracks) == 4
    tm.assert_scenario(tracks)
    print("A leaves at rim distance", tracks.tracks[1].end.distance)
    # the links are the model's
    counts = [len(v.charges) for v in tracks.frames]
    loops = device.boundary_sites()
    want = tm.link(counts, np.concatenate([v.positions for v in tracks.frames]),
                   np.concatenate([v.charges for v in tracks.frames]), tm.SCENARIO_R,
                   device.points[np.concatenate(list(loops.values()))])
    tm.assert_equal(tracks.links, want)
    assert [a.tolist() for a in tracks.next] == [a.tolist() for a in np.split(want["next"], np.cumsum(counts)[:-1])]
    (a,) = [t for t in tracks.tracks if len(t.frame_indices) == 9]
    assert np.array_equal(a.velocities, np.diff(a.positions, axis=0) / 0.5) and np.array_equal(a.times, times[:9])
    # A moves by 12 in x over the 5.5 of the call; a core's position is off by less than a mesh edge (about 1)
    assert np.allclose(a.velocities.mean(axis=0), [12 / 5.5, 0.0], atol=2 * 1.0 / 4.0)
    without = tdgl.track_vortices(device, psi, tm.SCENARIO_R)
    assert without.times is None and all(t.velocities.shape == (0, 2) and len(t.times) == 0 for t in without.tracks)
    # saved steps carry their own times
    from tdgl_amd.solution import TDGLData

    m = len(device.mesh.edge_mesh.edges)
    steps = [TDGLData(step=k, time=0.5 * k, dt=0.0, psi=frame, mu=np.zeros(len(frame)), supercurrent=np.zeros(m),
                      normal_current=np.zeros(m)) for k, frame in enumerate(psi)]
    from_steps = tdgl.track_vortices(device, steps, tm.SCENARIO_R)
    assert np.array_equal(from_steps.times, times) and from_steps.links.next.tobytes() == tracks.links.next.tobytes()
    # a radius too small to follow A's steps of 12 / 11 breaks its track into single frames that nothing explains
    short = tdgl.track_vortices(device, psi, 0.5)
    assert len(short.tracks) > 4 and any(t.end.kind == "unexplained" for t in short.tracks)


def test_python_refusals(scenario):
    import tdgl_amd as tdgl
    from tdgl_amd.vortices import link_frames

    device, psi = scenario
    with pytest.raises(TypeError):
        tdgl.track_vortices(device, psi)  # max_distance has no default
    with pytest.raises(TypeError):
        link_frames([(np.zeros((1, 2)), [1])])
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_distance"):
            tdgl.track_vortices(device, psi, bad)
        with pytest.raises(ValueError, match="max_distance"):
            link_frames([(np.zeros((1, 2)), [1])], bad)
    with pytest.raises(ValueError, match="unequal site counts"):
        tdgl.track_vortices(device, [psi[0], psi[1][:-1]], 1.0)
    with pytest.raises(ValueError, match="516 sites"):
        tdgl.track_vortices(device, psi[:, :-1], 1.0)
    with pytest.raises(ValueError, match="host.*hip"):
        tdgl.track_vortices(device, psi, 1.0, backend="nonsense")
    with pytest.raises(ValueError, match=r"\+1 or -1"):
        link_frames([(np.zeros((1, 2)), [2])], 1.0)
    with pytest.raises(ValueError, match="one time per frame"):
        tdgl.track_vortices(device, psi, 1.0, times=[0.0, 1.0])
    from tdgl_amd import _lib

    if _lib.load().tdgl_device_count() == 0:
        with pytest.raises(RuntimeError, match="tdgl_device_count"):
            tdgl.track_vortices(device, psi, 1.0, backend="hip")


def test_link_symbols_are_declared_and_refuse_a_null_plan():
    from tdgl_amd import _lib

    lib = _lib.load()
    for name in ("tdgl_vortex_plan_link", "tdgl_vortex_plan_link_stats"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    counts = np.array([0], dtype=np.int64)
    assert lib.tdgl_vortex_plan_link(None, 1, _lib.p_i64(counts), None, None, 1.0, *[None] * 6) == _lib.TDGL_ERR_ARG
    assert b"null plan" in lib.tdgl_last_error(None)
    assert lib.tdgl_vortex_plan_link_stats(None, None, None) == _lib.TDGL_ERR_ARG
