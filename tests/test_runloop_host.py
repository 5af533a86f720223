"""The Runner's stage loop (`tdgl_amd.runloop`) through both of its drivers, `TDGLSolver.solve` and `EnsembleSolver._run`,
without a GPU: a scripted state source replays the calls a reference run recorded (tests/golden/generate_golden.py:
run_reference) and the loop must save, count and assemble what the reference's Runner did.  Times and dts are copies of
what the source reports, so they are compared exactly."""

from types import SimpleNamespace

import numpy as np
import pytest

import h5_recorder
from conftest import load_golden
from helpers import options_from_golden, reference_mesh, uniform_field_A


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    from tdgl_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", refuse)


@pytest.fixture(scope="module")
def mesh():
    return reference_mesh(load_golden("mesh_small"))


class Replay:
    """One recorded run as a state source with a ``run``: call k of the recording is step k of the replay.  ``cap``: hand
    out at most that many steps per ``run``.  Fields are tagged with the loop's step."""

    def __init__(self, g, end_times, mesh, cap=None):
        self.g, self.end_times, self.cap = g, list(end_times), cap
        self.n, self.m = len(mesh.sites), len(mesh.edge_mesh.edges)
        self.total = len(g["call_dt"])
        starts = np.flatnonzero(g["call_stage_step"] == 0)
        assert len(starts) == len(self.end_times)
        self.last = set(int(k) - 1 for k in starts[1:]) | {self.total - 1}  # the last recorded call of every stage
        self.k = 0            # the next recorded call
        self.ended = False    # the last call handed out ended its stage, and the next stage has not begun
        self.stages_begun = 0
        self.asked = []       # (steps asked for, steps since the stage began) of every run call
        self.currents_asked = []

    def begin_stage(self):
        self.stages_begun += 1
        self.ended = False

    def loop_state(self):
        g, k = self.g, self.k - 1 if self.ended else self.k
        time = float(g["final_runner_time"]) if self.ended and k == self.total - 1 else float(g["call_time"][k])
        return dict(step=int(g["call_stage_step"][k]), time=time, dt=float(g["call_state_dt"][k]))

    def run(self, max_steps, end_time=np.inf):
        assert not self.ended and end_time == self.end_times[self.stages_begun - 1]
        self.asked.append((int(max_steps), int(self.g["call_stage_step"][self.k])))
        lo = self.k
        hi = min(lo + int(max_steps), lo + (self.cap or self.total), min(k for k in self.last if k >= lo) + 1)
        self.k, self.ended = hi, (hi - 1) in self.last and hi > lo
        g = self.g
        return dict(dt=g["call_dt"][lo:hi], mu=g["call_mu_probe"][lo:hi], theta=g["call_theta_probe"][lo:hi],
                    pcg_iters=np.full(hi - lo, 3, dtype=np.int32), screening_iterations=np.zeros(hi - lo, dtype=np.int32),
                    reached_end=self.ended)

    def get_state(self, supercurrent=True, normal_current=True):
        assert supercurrent == normal_current
        self.currents_asked.append(supercurrent)
        step = self.loop_state()["step"]
        out = dict(psi=np.full(self.n, step + 0j), mu=np.full(self.n, float(step)))
        if supercurrent:
            out.update(supercurrent=np.full(self.m, float(step)), normal_current=np.full(self.m, -float(step)))
        return out

    def link_scale(self):
        return 1.0

    # what else TDGLSolver.solve asks of its context
    def set_state(self, psi, mu):
        pass

    def set_controller(self, *a):
        pass

    def synchronize(self):
        pass

    def direct_stats(self):
        return {}


class ReplayEnsemble:
    """R replays behind `EnsembleContext`'s interface."""

    def __init__(self, replays, m):
        self.reps, self.asked, self.ctx = replays, [], SimpleNamespace(m=m)
        for name in ("set_probes", "set_link_exponents", "set_mu_boundary", "set_epsilon", "set_epsilon_table", "set_state",
                     "set_controller"):
            setattr(self, name, lambda *a, **k: None)

    def begin_stage(self, r):
        self.reps[r].begin_stage()

    def loop_state(self, r):
        return self.reps[r].loop_state()

    def link_scale(self, r):
        return 1.0

    def get_state(self, r, currents=True):
        return self.reps[r].get_state(currents, currents)

    def run(self, max_steps, end_time):
        self.asked.append(tuple(int(k) for k in max_steps))
        empty = dict(dt=np.zeros(0), mu=np.zeros((0, 2)), theta=np.zeros((0, 2)), reached_end=False)
        out = []
        for rep, k, end in zip(self.reps, max_steps, end_time):
            res = rep.run(k, end) if k else dict(empty)
            out.append({key: res[key] for key in empty})  # (the ensemble reports no iteration counts)
        return out


def _options(g, **kw):
    from tdgl_amd import SolverOptions

    o = options_from_golden(g)
    return SolverOptions(solve_time=o.solve_time, skip_time=o.skip_time, dt_init=o.dt_init, dt_max=o.dt_max,
                         adaptive=o.adaptive, adaptive_window=o.adaptive_window, save_every=o.save_every, **kw)


def _end_times(opts):
    return ([opts.skip_time] if opts.skip_time else []) + [opts.solve_time]


def _inputs(g, mesh, opts):
    """A replica's inputs as `TDGLSolver` sets them up, with no device context behind them."""
    from tdgl_amd.ensemble import _ReplicaInputs

    return _ReplicaInputs.from_dimensionless(mesh, opts, uniform_field_A(mesh, 0.1), 1.0,
                                             probe_points=list(range(g["call_mu_probe"].shape[1])),
                                             device=SimpleNamespace(mesh=mesh))


def _solve_single(g, mesh, cap=None, prepare=None, **kw):
    opts = _options(g, **kw)
    solver = _inputs(g, mesh, opts)
    if prepare is not None:
        prepare(solver)
    solver.ctx = Replay(g, _end_times(opts), mesh, cap=cap)
    solver._h5_file_factory = h5_recorder.open_file
    return solver.solve(), solver.ctx


def _n_sim(g):
    return int((g["call_time"] == 0).nonzero()[0][-1])  # tests/test_hip_parity.py::test_runner_bookkeeping_matches_reference


def _assert_like_recording(g, sol, opts):
    n_sim = _n_sim(g)
    assert [s.step for s in sol.saved_steps] == list(g["save_step"])
    assert np.array_equal([s.time for s in sol.saved_steps], g["save_time"])
    assert np.array_equal([s.dt for s in sol.saved_steps], g["save_dt"])
    assert sol.stats["steps_thermalizing"] == n_sim
    assert sol.stats["steps_thermalizing"] + sol.stats["steps_simulating"] == len(g["call_dt"])
    dyn = sol.dynamics
    assert np.array_equal(dyn.dt, g["call_dt"][n_sim:])
    assert np.array_equal(dyn.mu, g["call_mu_probe"][n_sim:].T) and np.array_equal(dyn.theta, g["call_theta_probe"][n_sim:].T)
    # within a chunk the times are the chunk's start plus a running sum of at most save_every dts: one rounding each
    want_t = g["call_time"][n_sim:]
    assert np.abs(dyn.time - want_t).max() <= opts.save_every * np.finfo(float).eps * want_t.max()
    # every saved step holds the state of its step; the run's first save carries the reference's zero currents
    assert [int(s.psi[0].real) for s in sol.saved_steps] == list(g["save_step"])
    first = sol.saved_steps[0]
    assert not first.supercurrent.any() and not first.normal_current.any() and len(first.supercurrent) == len(first.applied_vector_potential)
    assert all(np.array_equal(s.supercurrent, np.full(len(s.supercurrent), float(s.step))) for s in sol.saved_steps[1:])


@pytest.mark.parametrize("case", ["runner_bookkeeping", "traj_dynamic_lag", "traj_transport_strip"])
def test_single_run_saves_and_counts_like_the_reference(case, mesh):
    """runner_bookkeeping: save_every 7, saves at 0, 7, 14 with a partial final save; traj_dynamic_lag: a final save one
    step after a regular one (2000, 2001); traj_transport_strip: thermalised, ends on 348."""
    g = load_golden(case)
    sol, src = _solve_single(g, mesh)
    opts = sol.options
    _assert_like_recording(g, sol, opts)
    # what the library was asked for: a stage begun per stage, whole chunks up to the next save, no currents for the first save
    assert src.stages_begun == len(_end_times(opts))
    assert all(chunk == opts.save_every - i % opts.save_every for chunk, i in src.asked)
    assert src.currents_asked == [False] + [True] * (len(g["save_step"]) - 1)
    assert sol.stats["mean_pcg_iterations"] == 3.0 and len(sol.dynamics.pcg_iterations) == len(sol.dynamics.dt)
    assert list(sol.stats)[:3] == ["steps_thermalizing", "steps_simulating", "mean_pcg_iterations"] and sol.stats["mu_solver"] == "amg_pcg"


@pytest.mark.parametrize("case", ["runner_bookkeeping", "traj_transport_strip"])
def test_running_state_holds_the_steps_since_the_previous_save(case, mesh, tmp_path, monkeypatch):
    """Streamed through the recorder: save k's running_state holds the per-step scalars of the steps since save k - 1; a
    partial final save (traj_transport_strip: 348) also holds the step that ended the loop (written into the buffer, not
    counted: runner.py:429-432).  runner_bookkeeping ends one step after a regular save (14), which no save holds."""
    monkeypatch.chdir(tmp_path)
    h5_recorder.OPENED.clear()
    g = load_golden(case)
    sol, _ = _solve_single(g, mesh, output_file="out.h5")
    n_sim, every, steps = _n_sim(g), int(g["opt_save_every"]), g["save_step"]
    f = h5_recorder.OPENED[sol.path]
    assert f.closed and len(sol.saved_steps) == 1 and sol.saved_steps[0].step == steps[-1]
    assert sol.saved_step_index == list(zip(steps, g["save_time"]))
    groups = [f[f"data/{k}"] for k in range(len(steps))]
    assert [grp.attrs["step"] for grp in groups] == list(steps)
    assert ["running_state" in grp for grp in groups] == list(g["save_has_running"])
    n_probe = g["call_mu_probe"].shape[1]
    for k, grp in enumerate(groups[1:], start=1):
        lo, hi = n_sim + steps[k - 1], n_sim + steps[k] + (1 if steps[k] % every else 0)
        assert hi == len(g["call_dt"]) or steps[k] % every == 0
        want = np.zeros((1 + 2 * n_probe, every))
        want[:, : hi - lo] = np.column_stack([g["call_dt"][lo:hi], g["call_mu_probe"][lo:hi], g["call_theta_probe"][lo:hi]]).T
        got = np.vstack([np.atleast_2d(grp[f"running_state/{name}"].value) for name in ("dt", "mu", "theta")])
        assert np.array_equal(got, want), k


CASES3 = ["traj_transport_strip", "traj_transport_polygon", "traj_transport_polygon_fixed_dt"]


def _solve_ensemble(mesh, cases, opts, caps=None, prepare=None):
    from tdgl_amd.ensemble import EnsembleSolver

    gs = [load_golden(c) for c in cases]
    replays = [Replay(g, _end_times(opts), mesh, cap=cap)
               for g, cap in zip(gs, caps or [None] * len(gs))]
    solver = EnsembleSolver(mesh, opts, [_inputs(g, mesh, opts) for g in gs])
    for rep in solver.reps if prepare is not None else ():
        prepare(rep)
    solver.mu_path = (0, 0)
    ens = ReplayEnsemble(replays, len(mesh.edge_mesh.edges))
    return gs, solver._run(SimpleNamespace(synchronize=lambda: None), ens, 0.0), ens


def test_ensemble_replicas_each_follow_their_own_recording(mesh):
    """Three replicas of one options object (save_every 100, thermalised) replay three recordings of different lengths:
    each reproduces its own saves and counts, they finish in different rounds, and a finished replica is asked for 0 steps."""
    from tdgl_amd import SolverOptions

    opts = SolverOptions(solve_time=1.0, skip_time=0.5, save_every=100)  # (a replay ends its stages where its recording does)
    gs, sols, ens = _solve_ensemble(mesh, CASES3, opts)
    for r, (g, sol) in enumerate(zip(gs, sols)):
        assert int(g["opt_save_every"]) == 100
        _assert_like_recording(g, sol, opts)
        assert sol.stats["replica"] == r and sol.stats["replicas"] == 3 and sol.stats["mu_solver"] == "dense_ensemble"
        assert sol.stats["mean_pcg_iterations"] == 0.0 and not sol.dynamics.pcg_iterations.any()
        assert len(sol.dynamics.pcg_iterations) == len(sol.dynamics.dt)
        assert ens.reps[r].stages_begun == 2
    asked = np.array(ens.asked)
    rounds = [int(np.flatnonzero(asked[:, r])[-1]) for r in range(3)]  # the last round each replica took part in
    assert len(set(rounds)) == 3 and max(rounds) == len(asked) - 1
    for r in range(3):
        assert (asked[: rounds[r] + 1, r] > 0).all() and not asked[rounds[r] + 1:, r].any()


@pytest.mark.parametrize("driver", ["single", "ensemble"])
def test_short_returns_change_nothing(driver, mesh):
    """A `run` that hands out fewer steps than asked for (here at most 3) leaves the saves and the dynamics as they are."""
    g = load_golden("traj_transport_strip")
    if driver == "single":
        (a, _), (b, src) = _solve_single(g, mesh), _solve_single(g, mesh, cap=3)
        assert max(chunk for chunk, _ in src.asked) > 3
    else:
        opts = _options(g)
        a, b = (_solve_ensemble(mesh, ["traj_transport_strip"], opts, caps=[cap])[1][0] for cap in (None, 3))
    _assert_like_recording(g, b, b.options)
    assert [s.step for s in a.saved_steps] == [s.step for s in b.saved_steps]
    assert np.array_equal(a.dynamics.dt, b.dynamics.dt)
    # (a chunk's times are its start plus a running sum: shorter chunks round differently, within the bound above)
    assert np.abs(a.dynamics.time - b.dynamics.time).max() <= b.options.save_every * np.finfo(float).eps * a.dynamics.time.max()


@pytest.mark.parametrize("driver", ["single", "ensemble"])
def test_saved_epsilon_of_a_table_on_the_device_is_that_of_the_last_step_taken(driver, mesh):
    """With epsilon(t) evaluated by the time loop itself the saved epsilon is what the reference's last update() evaluated
    (solver.py:645-648): at the time before the last step taken for a regular save (time - dt), at the loop's time for the
    first save and for the final partial one (the step that ended the loop did not move the time)."""
    from tdgl_amd.ensemble import _with_epsilon_table
    from tdgl_amd.parameter import PiecewiseLinear

    g = load_golden("traj_transport_strip")
    factor = PiecewiseLinear([0.0, 100.0], [0.0, 1.0])
    n = len(mesh.sites)

    def table(solver):
        _with_epsilon_table(solver, (np.ones(n), factor.times, factor.values), n)
        solver._epsilon_on_device = driver == "single"  # (TDGLSolver._setup and EnsembleSolver._run set it on upload)

    if driver == "single":
        sol, _ = _solve_single(g, mesh, prepare=table)
    else:
        sol = _solve_ensemble(mesh, ["traj_transport_strip"], _options(g), prepare=table)[1][0]
    t, dt, every = g["save_time"], g["save_dt"], int(g["opt_save_every"])
    assert g["save_step"][-1] % every and not (g["save_step"][:-1] % every).any()
    t_last = np.concatenate([[t[0]], t[1:-1] - dt[1:-1], [t[-1]]])
    assert [s.epsilon[0] for s in sol.saved_steps] == [factor(x) for x in t_last] and sol.dynamic_epsilon


def test_seed_and_epsilon_table_checks_keep_their_messages(mesh):
    from tdgl_amd.runloop import check_epsilon_table, check_seed

    device, other = SimpleNamespace(name="a"), SimpleNamespace(name="b")
    seed = SimpleNamespace(device=device, tdgl_data=SimpleNamespace(psi=np.ones(len(mesh.sites))))
    check_seed(seed, device, mesh)
    with pytest.raises(ValueError, match=r"^The seed_solution.device must be equal to the device being simulated\.$"):
        check_seed(seed, other, mesh)
    with pytest.raises(ValueError, match=r"^solve_ensemble: replica 2: the seed_solution.device must be equal to the device being simulated\.$"):
        check_seed(seed, other, mesh, prefix="solve_ensemble: replica 2: ")
    short = SimpleNamespace(device=device, tdgl_data=SimpleNamespace(psi=np.ones(5)))
    with pytest.raises(ValueError, match=rf"^The seed solution has 5 sites, the device's mesh {len(mesh.sites)}\.$"):
        check_seed(short, device, mesh)
    with pytest.raises(ValueError, match=rf"^solve_ensemble: replica 0: the seed solution has 5 sites, the device's mesh {len(mesh.sites)}\.$"):
        check_seed(short, device, mesh, prefix="solve_ensemble: replica 0: ")
    eps0 = np.array([0.5, 1.0])
    check_epsilon_table(eps0, np.array([0.2, 1.0]))
    with pytest.raises(ValueError, match=r"^The disorder parameter epsilon must be <= 1$"):
        check_epsilon_table(eps0, np.array([0.2, 1.5]))
    with pytest.raises(ValueError, match=r"^replica 1: The disorder parameter epsilon must be <= 1$"):
        check_epsilon_table(eps0, np.array([0.2, 1.5]), prefix="replica 1: ")
