"""The census without a GPU: the oracle's record that the GPU tests compare with (tests/census_model.py), the
`DynamicsData` helpers, the option's validation, the run's bookkeeping and the HDF5 layout with the option on and off.

The first test is what keeps tests/test_hip_census.py from passing on all-zero rows: it asserts that the oracle's
census of both inputs has the transitions stated there."""

from types import SimpleNamespace

import numpy as np
import pytest

import census_model as M
import h5_recorder

W_UNDEF = M.WINDING_UNDEFINED


# ------------------------------------------------------------------ the oracle's record
def test_oracle_census_has_the_transitions():
    rows, _, _ = M.oracle_census("A", 100)
    p = M.problem("A")
    assert len(p["mesh"].sites) == 95 and len(p["mesh"].elements) == 153 and [len(l) for l in p["loops"]] == [35]
    # (k, row): row k describes psi after update k + 1
    assert M.transitions(rows) == [(0, (2, 1, 1)), (44, (1, 0, 1)), (73, (0, 0, 0))]
    rows, _, _ = M.oracle_census("B", 300)
    p = M.problem("B")
    assert len(p["mesh"].sites) == 1002 and [len(l) for l in p["loops"]] == [178, 40, 30]
    assert M.transitions(rows) == [(0, (1, 0, 2, 1, 0)), (84, (0, 0, 2, 1, 1))]
    assert M.transitions(M.oracle_census("B", 120)[0]) == M.transitions(rows)
    # the reversed start mirrors input A; the uniform one has nothing to count
    assert M.transitions(M.oracle_census("A_reversed", 100)[0]) == [(0, (1, 2, -1)), (44, (0, 1, -1)), (73, (0, 0, 0))]
    assert not M.oracle_census("A_uniform", 100)[0].any()


def test_the_vortex_of_the_189_site_input_lasts_beyond_the_ring():
    """b = 0.35 needs no raising: (1, 0, 1) from update 79 on, (2, 0, 2) from update 506 to beyond update 1,100."""
    rows, _, _ = M.oracle_census("A12", 1200)
    assert len(M.problem("A12")["mesh"].sites) == 189
    assert M.transitions(rows) == [(0, (2, 1, 1)), (78, (1, 0, 1)), (505, (2, 0, 2))]
    assert (rows[1024:1100, 0] > 0).all()


@pytest.mark.parametrize("name, n_steps, last", [("A", 100, 73), ("B", 120, 84)])
def test_oracle_trajectory_amplifies_one_rounding(name, n_steps, last):
    """Why the GPU test cannot hold psi to 1e-8 of the oracle's at the transitions: the oracle's own psi moves by
    ~1e-12 after the first update and by more than 1e-6 at the last transition when its start changes by one rounding.
    The census rows of the twins are nevertheless the oracle's own up to there."""
    E = M.oracle_sensitivity(name, n_steps)
    bound = M.deviation_bound(name, n_steps)
    print(f"input {name}: E after updates 1, 22, 43, {last + 1}: {E[0]:.1e}, {E[21]:.1e}, {E[42]:.1e}, {E[last]:.1e}; "
          f"bound below 1e-8 up to update {np.flatnonzero(bound < 1e-8)[-1] + 1}")
    assert 1e-13 < E[0] < 5e-12 and E[last] > 1e-6 and np.all(np.diff(E) >= 0)
    assert np.flatnonzero(bound < 1e-8)[-1] < M.transitions(M.oracle_census(name, n_steps)[0])[1][0]
    p = M.problem(name)
    for seed in M.SENSITIVITY_SEEDS:
        twin = M.census_rows(M.oracle_states(name, last + 4, seed), p["mesh"], p["loops"])
        assert np.array_equal(twin, M.oracle_census(name, n_steps)[0][:last + 4]), seed


@pytest.mark.parametrize("name, n_steps", [("A", 100), ("B", 300), ("A12", 1200), ("A_reversed", 100)])
def test_counts_and_windings_balance(name, n_steps):
    """w_rim - sum of w_holes == n_plus - n_minus in every row whose windings are all defined."""
    rows, _, _ = M.oracle_census(name, n_steps)
    w = rows[:, 2:].astype(np.int64)
    defined = (rows[:, 2:] != W_UNDEF).all(axis=1)
    assert defined.all()  # (no terminals: psi has no zero on a loop)
    assert np.array_equal(w[:, 0] - w[:, 1:].sum(axis=1), rows[:, 0].astype(np.int64) - rows[:, 1])


def test_model_marks_an_undefined_winding():
    p = M.problem("A")
    psi = p["psi0"].copy()
    psi[p["loops"][0][4]] = 0.0
    row = M.census_row(psi, p["mesh"], p["loops"])
    assert row[2] == W_UNDEF and row.dtype == np.int32 and tuple(row[:2]) == (2, 1)


# ------------------------------------------------------------------ DynamicsData
def _dynamics():
    from tdgl_amd import DynamicsData

    windings = np.array([[0, 0, W_UNDEF, 1, 1, W_UNDEF, 2, 1], [0, 0, 0, 0, 1, 1, 1, 1]], dtype=np.int32)
    counts = np.array([[0, 1, 2, 2, 1, 1, 3, 0], [0, 0, 1, 0, 0, 0, 1, 0]], dtype=np.int32)
    return DynamicsData(dt=np.full(8, 0.5), vortex_counts=counts, windings=windings, loop_names=("film", "hole"))


def test_dynamics_helpers():
    import tdgl_amd as tdgl

    assert tdgl.WINDING_UNDEFINED == W_UNDEF == -(2 ** 31)
    dyn = _dynamics()
    assert np.array_equal(dyn.net_vorticity(), [0, 1, 1, 2, 1, 1, 2, 0])
    w = dyn.winding("film")
    assert w.dtype == float and np.array_equal(np.isnan(w), [0, 0, 1, 0, 0, 1, 0, 0]) and np.array_equal(w[[0, 3, 6]], [0, 1, 2])
    assert np.array_equal(dyn.winding(1), dyn.winding("hole")) and not np.isnan(dyn.winding("hole")).any()
    # a defined winding against the previous DEFINED one: 0 -> 1 across the gap at step 3, 1 -> 2 at 6, 2 -> 1 at 7
    steps, times, old, new = dyn.winding_changes("film")
    assert np.array_equal(steps, [3, 6, 7]) and np.array_equal(old, [0, 1, 2]) and np.array_equal(new, [1, 2, 1])
    assert np.array_equal(times, dyn.time[[3, 6, 7]])
    steps, _, old, new = dyn.winding_changes("hole")
    assert np.array_equal(steps, [4]) and (old[0], new[0]) == (0, 1)
    with pytest.raises(KeyError, match="nothing"):
        dyn.winding("nothing")
    plain = tdgl.DynamicsData(dt=np.ones(3))
    assert plain.vortex_counts is None and plain.windings is None and plain.loop_names is None
    for call in (plain.net_vorticity, lambda: plain.winding("film"), lambda: plain.winding_changes("film")):
        with pytest.raises(ValueError, match="vortex_census"):
            call()


def test_dynamics_hdf5_round_trip_keeps_the_sentinel():
    from tdgl_amd import DynamicsData

    dyn = _dynamics()
    g = h5_recorder.Group()
    dyn.to_hdf5(g)
    assert set(g.keys()) == {"dt", "vortex_counts", "windings", "loop_names"}
    stored = g["windings"].value
    assert stored.dtype == float and stored.shape == (2, 8) and np.array_equal(np.isnan(stored), dyn.windings == W_UNDEF)
    assert g["vortex_counts"].value.dtype == float and g["vortex_counts"].shape == (2, 8)
    back = DynamicsData.from_hdf5(g)
    assert back.windings.dtype == np.int32 and np.array_equal(back.windings, dyn.windings)
    assert back.vortex_counts.dtype == np.int32 and np.array_equal(back.vortex_counts, dyn.vortex_counts)
    assert back.loop_names == ("film", "hole")
    # without a census the group is what it was
    g = h5_recorder.Group()
    DynamicsData(dt=np.ones(3), mu=np.zeros((2, 3)), theta=np.zeros((2, 3))).to_hdf5(g)
    assert set(g.keys()) == {"dt", "mu", "theta"}


# ------------------------------------------------------------------ option
def test_option_validation():
    from tdgl_amd import SolverOptions, SolverOptionsError

    assert SolverOptions(solve_time=1.0).vortex_census is False
    SolverOptions(solve_time=1.0, vortex_census=True).validate()
    SolverOptions(solve_time=1.0, vortex_census=np.bool_(True)).validate()
    for bad in (1, "yes", None):
        with pytest.raises(SolverOptionsError, match="vortex_census"):
            SolverOptions(solve_time=1.0, vortex_census=bad).validate()


def test_solver_without_a_device_and_distributed_solver_refuse():
    from tdgl_amd import SolverOptions, SolverOptionsError
    from tdgl_amd.distributed import DistributedTDGL
    from tdgl_amd.solver import install_census

    with pytest.raises(SolverOptionsError, match="vortex_census"):
        install_census(None, None)
    with pytest.raises(SolverOptionsError, match="vortex_census"):
        install_census(None, SimpleNamespace(mesh=None))
    p = M.problem("A")
    with pytest.raises(SolverOptionsError, match="vortex_census"):
        DistributedTDGL(p["mesh"], SolverOptions(solve_time=1.0, vortex_census=True), p["A"], rank=0, world=1)


# ------------------------------------------------------------------ bookkeeping and files
class Scripted:
    """The oracle's record of input A behind `TDGLContext`'s interface: ``run`` hands out the recorded steps (census
    rows only with ``census``) and ends a stage like the Runner does (the step that reaches the end time is taken, the
    time is not advanced)."""

    def __init__(self, n, m, census=True):
        self.rows, self.dts, _ = M.oracle_census("A", 100)
        self.n, self.m, self.census = n, m, census
        self.k = self.k0 = 0
        self.time, self.prev_dt = 0.0, 1e-3
        self.stage_rows = []  # the row index range of every stage

    def begin_stage(self):
        self.k0, self.time = self.k, 0.0
        self.stage_rows.append([self.k, self.k])

    def loop_state(self):
        return dict(step=self.k - self.k0, time=self.time, dt=self.prev_dt)

    def run(self, max_steps, end_time=np.inf):
        lo, reached = self.k, False
        for _ in range(int(max_steps)):
            taken = self.k
            if self.time >= end_time:
                reached = True
            else:
                self.prev_dt = float(self.dts[taken])
                self.time += self.prev_dt
                self.k += 1
            if reached:
                break
        hi = self.k + (1 if reached else 0)
        self.stage_rows[-1][1] = hi
        if reached:
            self.k = hi  # (the next stage continues behind the step that ended this one)
        return dict(dt=self.dts[lo:hi], mu=None, theta=None, pcg_iters=np.zeros(hi - lo, dtype=np.int32),
                    screening_iterations=np.zeros(hi - lo, dtype=np.int32), reached_end=reached,
                    census=self.rows[lo:hi] if self.census else None)

    def get_state(self, supercurrent=True, normal_current=True):
        out = dict(psi=np.ones(self.n, dtype=complex), mu=np.zeros(self.n))
        if supercurrent:
            out.update(supercurrent=np.zeros(self.m), normal_current=np.zeros(self.m))
        return out

    def link_scale(self):
        return 1.0

    def set_state(self, psi, mu):
        pass

    def set_controller(self, *a):
        pass

    def synchronize(self):
        pass

    def direct_stats(self):
        return {}


def _solve_scripted(census, **kw):
    from tdgl_amd import SolverOptions
    from tdgl_amd.ensemble import _ReplicaInputs

    p = M.problem("A")
    mesh = p["mesh"]
    opts = SolverOptions(solve_time=3.0, dt_init=1e-3, save_every=7, vortex_census=census, **kw)
    solver = _ReplicaInputs.from_dimensionless(mesh, opts, p["A"], 1.0, device=SimpleNamespace(mesh=mesh))
    solver.ctx = Scripted(len(mesh.sites), len(mesh.edge_mesh.edges), census)
    solver.census_loops = ("film",) if census else None
    solver._h5_file_factory = h5_recorder.open_file
    return solver.solve(), solver.ctx


@pytest.mark.parametrize("skip_time", [0.0, 0.05])
def test_run_record_books_the_census_like_the_other_columns(skip_time):
    """The simulated stage's rows in `DynamicsData`, a thermalisation stage's not -- as for dt."""
    sol, src = _solve_scripted(True, skip_time=skip_time)
    dyn = sol.dynamics
    lo, hi = src.stage_rows[-1]
    assert len(src.stage_rows) == (2 if skip_time else 1) and hi - lo >= 40 and (lo > 0) == bool(skip_time)
    assert np.array_equal(dyn.dt, src.dts[lo:hi])
    assert dyn.loop_names == ("film",)
    assert dyn.vortex_counts.dtype == np.int32 and np.array_equal(dyn.vortex_counts, src.rows[lo:hi, :2].T)
    assert dyn.windings.dtype == np.int32 and np.array_equal(dyn.windings, src.rows[lo:hi, 2:].T)
    assert len(dyn.winding_changes("film")[0]) == 0 and np.array_equal(np.unique(dyn.net_vorticity()), [1])
    off, _ = _solve_scripted(False, skip_time=skip_time)
    assert off.dynamics.vortex_counts is None and off.dynamics.windings is None and off.dynamics.loop_names is None
    assert np.array_equal(off.dynamics.dt, dyn.dt)


def _layout(group, prefix=""):
    """``{path: shape}`` of every dataset and ``{path: sorted attribute names}`` of every group below ``group``."""
    shapes, attrs = {}, {prefix or "/": sorted(k for k in group.attrs if k != "timestamp")}
    for name, item in group.items_.items():
        path = f"{prefix}/{name}"
        if isinstance(item, h5_recorder.Group):
            s, a = _layout(item, path)
            shapes.update(s)
            attrs.update(a)
        else:
            shapes[path] = item.shape
    return shapes, attrs


def test_streamed_file_names_and_shapes_with_the_option_on_and_off(tmp_path, monkeypatch):
    from tdgl_amd import DynamicsData

    monkeypatch.chdir(tmp_path)
    h5_recorder.OPENED.clear()
    on, src = _solve_scripted(True, output_file="on.h5")
    off, _ = _solve_scripted(False, output_file="off.h5")
    f_on, f_off = h5_recorder.OPENED[on.path], h5_recorder.OPENED[off.path]
    shapes_on, attrs_on = _layout(f_on)
    shapes_off, attrs_off = _layout(f_off)
    # off: no census dataset anywhere, no option attribute -- the layout of a file written before the option existed
    assert not [k for k in shapes_off if "vortex_counts" in k or "windings" in k]
    assert "vortex_census" not in attrs_off["/solution/options"]
    # on: the same layout plus the two running-state columns per save and the option's attribute
    extra = {k: v for k, v in shapes_on.items() if k not in shapes_off}
    n_saves = len([k for k in shapes_on if k.endswith("/running_state/dt")])
    assert n_saves >= 6
    assert sorted(extra) == sorted(f"/data/{k}/running_state/{name}" for k in range(1, n_saves + 1) for name in ("vortex_counts", "windings"))
    assert all(v == ((2, 7) if k.endswith("vortex_counts") else (7,)) for k, v in extra.items())
    assert {k: v for k, v in shapes_on.items() if k not in extra} == shapes_off
    assert sorted(set(attrs_on["/solution/options"]) - set(attrs_off["/solution/options"])) == ["vortex_census"]
    assert sorted(set(attrs_on["/solution"]) - set(attrs_off["/solution"])) == ["census_loop_names"]
    assert "census_loop_names" not in attrs_off["/solution"] and list(f_on["solution"].attrs["census_loop_names"]) == ["film"]
    changed = ("/solution/options", "/solution")
    assert {k: v for k, v in attrs_on.items() if k not in changed} == {k: v for k, v in attrs_off.items() if k not in changed}
    # the values: save k holds the steps since save k - 1, zero padded
    grp = f_on["data/2/running_state"]
    assert np.array_equal(grp["vortex_counts"].value, src.rows[7:14, :2].T) and np.array_equal(grp["windings"].value, src.rows[7:14, 2])
    # read back from the running-state buffers
    back = DynamicsData.from_hdf5(f_on)
    n = len(back.dt)
    # (the last save is a partial one, 52 = 7 * 7 + 3: it also holds the step that ended the loop, so the file has all 52)
    assert on.saved_step_index[-1][0] == 52 and n == len(on.dynamics.dt) == 52
    assert back.loop_names == ("film",) == on.dynamics.loop_names  # (from the solution group's attribute)
    assert back.windings.dtype == np.int32 and np.array_equal(back.windings, on.dynamics.windings[:, :n])
    assert np.array_equal(back.vortex_counts, on.dynamics.vortex_counts[:, :n])
    plain = DynamicsData.from_hdf5(f_off)
    assert plain.windings is None and plain.loop_names is None


def test_in_memory_solution_writes_the_same_columns():
    """`write_solution_h5` (a solution kept in memory) builds the running-state buffers from `DynamicsData`: NaN where a
    winding is not defined."""
    from tdgl_amd.io import _running_state_buffers

    sol, src = _solve_scripted(True)
    sol.dynamics.windings[0, 9] = W_UNDEF
    bufs = _running_state_buffers(sol)
    assert set(bufs[1]) == {"dt", "vortex_counts", "windings"}
    assert bufs[2]["vortex_counts"].shape == (2, 7) and bufs[2]["windings"].shape == (1, 7)
    assert np.array_equal(bufs[2]["vortex_counts"], src.rows[7:14, :2].T)
    assert np.isnan(bufs[2]["windings"][0, 2]) and np.array_equal(bufs[2]["windings"][0, [0, 1, 3]], src.rows[[7, 8, 10], 2])
    off, _ = _solve_scripted(False)
    assert set(_running_state_buffers(off)[1]) == {"dt"}
