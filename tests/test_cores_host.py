"""CPU tests of the core records taken inside the time loops (``SolverOptions.vortex_cores``): the options and the
refusals, the host's assembly of a flush window (csrc/core_records.h through tdgl_host_core_records_assemble) against
the plain-loop model of tests/cores_model.py, `VortexCores`, the files with the option off, and that the oracle's
states have what tests/test_hip_cores.py relies on.
"""

import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import census_model as M
import cores_model as CM
import h5_recorder


# ------------------------------------------------------------------ options and refusals
def test_option_validation():
    from tdgl_amd import SolverOptions, SolverOptionsError

    o = SolverOptions(solve_time=1.0)
    assert (o.vortex_cores, o.vortex_cores_every, o.vortex_cores_capacity) == (False, 1, 262_144)
    SolverOptions(solve_time=1.0, vortex_cores=True, vortex_cores_every=3, vortex_cores_capacity=10).validate()
    SolverOptions(solve_time=1.0, vortex_cores=np.bool_(True), vortex_cores_every=np.int64(2)).validate()
    for bad in (1, "yes", None):
        with pytest.raises(SolverOptionsError, match="vortex_cores"):
            SolverOptions(solve_time=1.0, vortex_cores=bad).validate()
    for name in ("vortex_cores_every", "vortex_cores_capacity"):
        for bad in (0, -1, 1.5, True, None, "2"):
            with pytest.raises(SolverOptionsError, match=name):
                SolverOptions(solve_time=1.0, **{name: bad}).validate()


def test_distributed_solver_and_ensemble_refuse():
    from tdgl_amd import SolverOptions, SolverOptionsError
    from tdgl_amd.distributed import DistributedTDGL
    from tdgl_amd.ensemble import _refuse_options

    p = M.problem("A")
    opts = SolverOptions(solve_time=1.0, vortex_cores=True)
    with pytest.raises(SolverOptionsError, match="vortex_cores"):
        DistributedTDGL(p["mesh"], opts, p["A"], rank=0, world=1)
    with pytest.raises(SolverOptionsError, match="vortex_cores"):
        _refuse_options(opts, len(p["mesh"].sites))
    _refuse_options(SolverOptions(solve_time=1.0), len(p["mesh"].sites))


# ------------------------------------------------------------------ the assembly of a flush window
def _assemble_lib(rows, recorded, tri, chg, xy, capacity):
    from tdgl_amd import _lib

    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    recorded = np.ascontiguousarray(recorded, dtype=np.uint8)
    tri, chg = np.ascontiguousarray(tri, dtype=np.int32), np.ascontiguousarray(chg, dtype=np.int32)
    xy = np.ascontiguousarray(xy, dtype=float).reshape(-1, 2)
    n_rec, n_pool = int(np.count_nonzero(recorded)), len(tri)
    row, offset = np.full(n_rec, -7, dtype=np.int64), np.full(n_rec + 1, -7, dtype=np.int64)
    complete = np.full(n_rec, 9, dtype=np.uint8)
    o_tri, o_chg, o_xy = np.zeros(n_pool, dtype=np.int32), np.zeros(n_pool, dtype=np.int32), np.zeros((n_pool, 2))
    n_steps = C.c_int64(-1)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))  # noqa: E731
    status = lib.tdgl_host_core_records_assemble(
        len(rows), rows.shape[1], _lib.p_i32(rows), u8(recorded), n_pool, _lib.p_i32(tri), _lib.p_i32(chg), _lib.p_f64(xy),
        capacity, _lib.p_i64(row), _lib.p_i64(offset), u8(complete), _lib.p_i32(o_tri), _lib.p_i32(o_chg), _lib.p_f64(o_xy),
        C.byref(n_steps))
    assert status == 0 and n_steps.value == n_rec
    k = offset[-1]
    return row, offset, complete.astype(bool), o_tri[:k], o_chg[:k], o_xy[:k]


def _window(counts, recorded, capacity, seed, ncol=3):
    """Census rows with the given n_plus + n_minus, and a pool as the device leaves it: per recorded step its triangles
    in a shuffled order, only the first ``capacity`` slots written (the rest: a poison value)."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((len(counts), ncol), dtype=np.int32)
    tri, chg = [], []
    for r, c in enumerate(counts):
        plus = int(rng.integers(0, c + 1))
        rows[r, :2] = plus, c - plus
        rows[r, 2:] = rng.integers(-3, 4)
        if recorded[r]:
            t = rng.permutation(10 * c + 5)[:c]
            tri += list(t)
            chg += list(np.where(rng.permutation(c) < plus, 1, -1))
    tri, chg = np.array(tri, dtype=np.int32), np.array(chg, dtype=np.int32)
    xy = rng.standard_normal((len(tri), 2))
    held = min(len(tri), capacity)
    return rows, tri[:held], chg[:held], xy[:held]


ASSEMBLE_CASES = {
    # counts per row, recorded, capacity
    "plain": ([3, 5, 2, 7], [1, 1, 1, 1], 100),
    "empty_steps": ([0, 4, 0, 0, 6, 0], [1, 1, 1, 1, 1, 1], 100),
    "nothing_at_all": ([0, 0, 0], [1, 1, 1], 4),
    "every_3": ([4, 9, 9, 5, 9, 9, 6, 9], [1, 0, 0, 1, 0, 0, 1, 0], 100),
    "overflow_in_the_middle": ([4, 6, 5, 0, 3], [1, 1, 1, 1, 1], 12),
    "overflow_at_a_step_boundary": ([4, 6, 0, 5, 1], [1, 1, 1, 1, 1], 10),
    "overflow_in_the_first_step": ([8, 1], [1, 1], 5),
    "overflow_with_every_2": ([4, 50, 6, 50, 5, 50, 2], [1, 0, 1, 0, 1, 0, 1], 12),
    "many": (list(range(40, 0, -1)), [1] * 40, 1000),
}


@pytest.mark.parametrize("case", sorted(ASSEMBLE_CASES))
def test_assembly_equals_the_plain_loop(case):
    counts, recorded, capacity = ASSEMBLE_CASES[case]
    rows, tri, chg, xy = _window(counts, recorded, capacity, seed=len(case))
    want = CM.assemble(rows, recorded, list(tri), list(chg), [tuple(v) for v in xy], capacity)
    got = _assemble_lib(rows, recorded, tri, chg, xy, capacity)
    for g, w, name in zip(got, want, ("row", "offset", "complete", "triangles", "charges", "xy")):
        assert np.array_equal(g, w), (case, name, g, w)
    row, offset, complete, o_tri = got[:4]
    assert np.array_equal(row, np.flatnonzero(recorded))
    for k in range(len(row)):  # sorted within a step, whatever the pool's order was
        assert np.all(np.diff(o_tri[offset[k]:offset[k + 1]]) > 0)
    if case.startswith("overflow"):
        first_bad = int(np.flatnonzero(~complete)[0])
        assert not complete[first_bad:].any() and np.all(np.diff(offset[first_bad:]) == 0)
        assert complete[:first_bad].all()
    else:
        assert complete.all() and offset[-1] == sum(c for c, r in zip(counts, recorded) if r)
    if case == "overflow_at_a_step_boundary":
        assert list(complete) == [True, True, True, False, False]  # (an empty step at the brim is still complete)


def test_assembly_refuses_bad_arguments():
    from tdgl_amd import _lib

    lib = _lib.load()
    rows = np.array([[2, 1, 0]], dtype=np.int32)
    recorded = np.ones(1, dtype=np.uint8)
    u8 = recorded.ctypes.data_as(C.POINTER(C.c_uint8))
    i64 = np.zeros(2, dtype=np.int64)
    n_steps = C.c_int64(0)
    # the pool is shorter than the rows say
    status = lib.tdgl_host_core_records_assemble(1, 3, _lib.p_i32(rows), u8, 0, None, None, None, 10, _lib.p_i64(i64),
                                                 _lib.p_i64(i64), u8, None, None, None, C.byref(n_steps))
    assert status != 0
    status = lib.tdgl_host_core_records_assemble(1, 1, _lib.p_i32(rows), u8, 0, None, None, None, 10, _lib.p_i64(i64),
                                                 _lib.p_i64(i64), u8, None, None, None, C.byref(n_steps))
    assert status != 0


# ------------------------------------------------------------------ VortexCores
def _cores_of_oracle(name, n_steps, every=1):
    from tdgl_amd import VortexCores

    p = M.problem(name)
    mesh = p["mesh"]
    states = M.oracle_states(name, n_steps)
    steps = np.arange(0, n_steps, every)
    frames = CM.cores_of_states(states[steps], mesh)
    device = SimpleNamespace(points=mesh.sites, triangles=mesh.elements, boundary_sites=lambda: {"film": p["loops"][0]})
    times = 0.01 * (steps + 1.0)
    cores = VortexCores(steps, times, [len(f.charges) for f in frames], np.ones(len(frames), dtype=bool),
                        np.concatenate([f.positions for f in frames]), np.concatenate([f.charges for f in frames]),
                        np.concatenate([f.triangles for f in frames]), device=device)
    return cores, frames, p


def test_vortex_cores_slicing_and_tracks():
    from tdgl_amd.vortices import VortexTracks, link_frames

    cores, frames, p = _cores_of_oracle("A", 60, every=2)
    assert len(cores) == 30 == len(list(cores)) and cores.offsets[-1] == len(cores.charges) > 30
    assert np.array_equal(cores.steps, np.arange(0, 60, 2))
    for k in (0, 7, 29, -1):
        got, want = cores.frame(k), frames[k]
        assert np.array_equal(got.positions, want.positions) and np.array_equal(got.charges, want.charges)
        assert np.array_equal(got.triangles, want.triangles)
    with pytest.raises(IndexError):
        cores.frame(30)
    r = 0.8
    loop_xy = p["mesh"].sites[np.asarray(p["loops"][0])]
    want = link_frames(frames, r, loop_xy)
    tracks = cores.tracks(r)
    assert isinstance(tracks, VortexTracks) and len(tracks) >= 3
    for got_a, want_a in zip(tracks.links, want):
        assert np.array_equal(got_a, want_a)
    assert np.array_equal(tracks.times, cores.times)
    assert {t.charge for t in tracks} == {1, -1}
    part = cores.tracks(r, first=5, last=12)
    for got_a, want_a in zip(part.links, link_frames(frames[5:13], r, loop_xy)):
        assert np.array_equal(got_a, want_a)
    with pytest.raises(ValueError, match="backend"):
        cores.tracks(r, backend="cuda")
    with pytest.raises(ValueError, match="first"):
        cores.tracks(r, first=3, last=30)


def test_tracks_refuse_an_incomplete_frame_by_name():
    cores, _, _ = _cores_of_oracle("A", 20)
    cores.complete[11] = False
    with pytest.raises(ValueError, match="vortex_cores_capacity"):
        cores.tracks(0.8)
    assert len(cores.tracks(0.8, last=10).frames) == 11  # (a range without it is served)
    with pytest.raises(ValueError, match="vortex_cores_capacity"):
        cores.tracks(0.8, first=11, last=11)


def test_vortex_cores_checks_its_arrays():
    from tdgl_amd import VortexCores

    with pytest.raises(ValueError, match="records"):
        VortexCores([0, 1], [0.0, 0.1], [1, 2], [True, True], np.zeros((2, 2)), [1, 1], [0, 1])
    with pytest.raises(ValueError, match="per recorded step"):
        VortexCores([0, 1], [0.0], [1, 2], [True, True], np.zeros((3, 2)), [1, 1, 1], [0, 1, 2])
    empty = VortexCores([], [], [], [], np.zeros((0, 2)), [], [])
    assert len(empty) == 0 and list(empty) == [] and np.array_equal(empty.offsets, [0])


# ------------------------------------------------------------------ bookkeeping of a solve, and the files
class ScriptedCores:
    """`test_census_host.Scripted` with core records: every step's cores are `host_find` on the oracle's state."""

    def __init__(self, base, every):
        self.base, self.every = base, every
        self.index = 0  # running index of the next accepted step
        mesh = M.problem("A")["mesh"]
        self.frames = CM.cores_of_states(M.oracle_states("A", 100), mesh)

    def __getattr__(self, name):
        return getattr(self.base, name)

    def run(self, max_steps, end_time=np.inf):
        lo = self.base.k
        res = self.base.run(max_steps, end_time)
        k = len(res["dt"])
        steps = np.array([s for s in range(k) if (self.index + s) % self.every == 0], dtype=np.int64)
        self.index += k
        frames = [self.frames[lo + s] for s in steps]
        cat = lambda xs, empty: np.concatenate(xs) if xs else empty  # noqa: E731
        return dict(res, cores=dict(
            steps=steps, counts=np.array([len(f.charges) for f in frames], dtype=np.int64),
            complete=np.ones(len(frames), dtype=bool), triangles=cat([f.triangles for f in frames], np.zeros(0, np.int32)),
            charges=cat([f.charges for f in frames], np.zeros(0, np.int32)),
            positions=cat([f.positions for f in frames], np.zeros((0, 2)))))


def _solve_scripted(cores, every=1, **kw):
    from tdgl_amd import SolverOptions
    from tdgl_amd.ensemble import _ReplicaInputs
    from test_census_host import Scripted

    p = M.problem("A")
    mesh = p["mesh"]
    opts = SolverOptions(solve_time=3.0, dt_init=1e-3, save_every=7, vortex_cores=cores, vortex_cores_every=every, **kw)
    device = SimpleNamespace(mesh=mesh, points=mesh.sites, triangles=mesh.elements, boundary_sites=lambda: {"film": p["loops"][0]})
    solver = _ReplicaInputs.from_dimensionless(mesh, opts, p["A"], 1.0, device=device)
    base = Scripted(len(mesh.sites), len(mesh.edge_mesh.edges), cores)
    solver.ctx = ScriptedCores(base, every) if cores else base
    solver.census_loops = ("film",) if cores else None
    solver.records_cores = cores
    solver._h5_file_factory = h5_recorder.open_file
    return solver.solve(), solver.ctx


@pytest.mark.parametrize("skip_time, every", [(0.0, 1), (0.05, 1), (0.05, 3)])
def test_run_record_books_the_cores_of_the_saved_stage(skip_time, every):
    sol, src = _solve_scripted(True, every=every, skip_time=skip_time)
    dyn = sol.dynamics
    vc = dyn.vortex_cores
    lo, hi = src.base.stage_rows[-1]
    assert hi - lo >= 40 and (lo > 0) == bool(skip_time)
    want_rows = [r for r in range(lo, hi) if r % every == 0]  # (the scripted index runs on across the stages)
    assert np.array_equal(vc.steps, np.array(want_rows) - lo) and len(vc) == len(want_rows) > 10
    assert np.array_equal(vc.times, (dyn.time + dyn.dt)[vc.steps])  # after the step
    assert vc.complete.all()
    for k, r in enumerate(want_rows):
        got, want = vc.frame(k), src.frames[r]
        assert np.array_equal(got.triangles, want.triangles) and np.array_equal(got.charges, want.charges)
        assert np.array_equal(got.positions, want.positions)
        assert len(got.charges) == dyn.vortex_counts[:, vc.steps[k]].sum()
    assert dyn.vortex_counts is not None  # (the cores imply the census)
    off, _ = _solve_scripted(False, skip_time=skip_time)
    assert off.dynamics.vortex_cores is None and off.dynamics.vortex_counts is None
    assert np.array_equal(off.dynamics.dt, dyn.dt)


def test_files_do_not_hold_the_option_at_its_defaults_nor_the_records(tmp_path, monkeypatch):
    from test_census_host import _layout

    monkeypatch.chdir(tmp_path)
    h5_recorder.OPENED.clear()
    off, _ = _solve_scripted(False, output_file="off.h5")
    on, _ = _solve_scripted(True, every=2, vortex_cores_capacity=1000, output_file="on.h5")
    shapes_off, attrs_off = _layout(h5_recorder.OPENED[off.path])
    shapes_on, attrs_on = _layout(h5_recorder.OPENED[on.path])
    assert not [k for k in attrs_off["/solution/options"] if k.startswith("vortex_c")]
    assert not [k for k in shapes_off if "vortex" in k or "windings" in k]
    assert sorted(set(attrs_on["/solution/options"]) - set(attrs_off["/solution/options"])) == [
        "vortex_cores", "vortex_cores_capacity", "vortex_cores_every"]
    # on: the census' columns (implied) and nothing of the records themselves
    extra = sorted({k.rsplit("/", 1)[1] for k in shapes_on if k not in shapes_off})
    assert extra == ["vortex_counts", "windings"]
    # DynamicsData.to_hdf5 / from_hdf5: saved without the records, read back as None
    from tdgl_amd import DynamicsData

    g = h5_recorder.Group()
    on.dynamics.to_hdf5(g)
    assert not [k for k in g.keys() if "cores" in k]
    back = DynamicsData.from_hdf5(g)
    assert back.vortex_cores is None and np.array_equal(back.vortex_counts, on.dynamics.vortex_counts)


# ------------------------------------------------------------------ what the GPU tests rely on
def test_oracle_states_have_what_the_gpu_tests_rely_on():
    rows = M.oracle_census("A", 100)[0]
    assert (rows[:, 0] > 0).any() and (rows[:, 1] > 0).any()  # cores of both signs on A
    rows = M.oracle_census("B", 120)[0]
    counts = rows[:, :2].sum(axis=1)
    assert (counts > 0).any() and (np.diff(counts) != 0).any()  # a step on B at which the count changes
    rows = M.oracle_census("A12", 1200)[0]
    assert (rows[:1100, :2].sum(axis=1) >= 1).all()  # at least one core at every step up to 1,100 on A12
    # the dense state of the GPU tests: hundreds of cores, of both signs
    mesh = M.problem("B")["mesh"]
    dense = CM.cores_of_states([CM.dense_psi0(mesh)], mesh)[0]
    assert len(dense.charges) > 300 and {1, -1} == set(dense.charges.tolist())
    # the model's frames are what the census counts
    states = M.oracle_states("A", 20)
    for psi, row in zip(states, M.oracle_census("A", 100)[0][:20]):
        f = CM.cores_of_states([psi], M.problem("A")["mesh"])[0]
        assert (np.count_nonzero(f.charges > 0), np.count_nonzero(f.charges < 0)) == tuple(row[:2])
        assert np.all(np.diff(f.triangles) > 0)
