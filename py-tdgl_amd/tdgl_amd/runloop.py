"""The Runner's stage loop (thermalise, simulate, save every ``save_every`` steps, one final partial save), written
once for ``TDGLSolver.solve`` and ``EnsembleSolver``.

`RunRecord` holds what one run accumulates and owns the loop's rules; a driver asks it how many steps to take
(`RunRecord.request`), has the library take them and hands the result back (`RunRecord.absorb`).  The record talks to the
device through a *state source* -- ``begin_stage()``, ``loop_state()``, ``get_state(supercurrent=, normal_current=)``,
``link_scale()``, ``link_term_scales()``, ``link_exponents()`` (with moving loops) and, with screening, ``induced_vector_potential()``: `hipcore.TDGLContext` as it is, or one replica of
an ensemble (`ensemble._Replica`) -- and reads the run's inputs from the ``TDGLSolver`` that set them up.  Nothing here
needs the library, so a scripted source can replay a recorded run through either driver.
"""

import numpy as np

from .io import RunningState
from .solution import WINDING_UNDEFINED, DynamicsData, Solution, TDGLData

STAGES = ("Thermalizing", "Simulating")


def census_columns(census) -> dict:
    """The int32 census rows [k, 2 + L] of a ``run`` as the running state's float columns: ``vortex_counts`` [k, 2] and
    ``windings`` [k, L] with NaN where a winding is not defined."""
    census = np.asarray(census)
    windings = census[:, 2:].astype(float)
    windings[census[:, 2:] == WINDING_UNDEFINED] = np.nan
    return dict(vortex_counts=census[:, :2].astype(float), windings=windings)


def check_seed(seed, device, mesh, prefix: str = "") -> None:
    """A seed solution must come from an equal device with as many sites; ``prefix`` names the replica."""
    if seed.device != device:
        msg = "the seed_solution.device must be equal to the device being simulated."
    elif len(seed.tdgl_data.psi) != len(mesh.sites):  # (equal devices may carry different meshes)
        msg = f"the seed solution has {len(seed.tdgl_data.psi)} sites, the device's mesh {len(mesh.sites)}."
    else:
        return
    raise ValueError(prefix + msg if prefix else msg[0].upper() + msg[1:])


def check_epsilon_table(epsilon0, factors, prefix: str = "") -> None:
    """epsilon(t) = factor(t) * epsilon0 must stay <= 1 at every node of the table."""
    if max(float(np.max(f * epsilon0)) for f in factors) > 1:
        raise ValueError(prefix + "The disorder parameter epsilon must be <= 1")


def save_step(source, solver, rec: "RunRecord", final: bool = False) -> None:
    """Take one saved step from ``source`` into ``rec`` (or through its handler to disk)."""
    ls = source.loop_state()
    if solver.device_evaluates_epsilon():
        # the reference saves the epsilon its last update() evaluated (solver.py:645-648): at the time of the last
        # step taken
        t_last = ls["time"] if (final or ls["step"] == 0) else ls["time"] - ls["dt"]
        solver.epsilon = np.asarray(solver.epsilon_func(max(t_last, 0.0)), dtype=float)
    if ls["step"] == 0 and not rec.saved and not rec.seeded:
        js = jn = np.zeros(solver.num_edges)  # reference initial values (solver.py:736-737)
        st = source.get_state(supercurrent=False, normal_current=False)
    else:
        st = source.get_state()
        js, jn = st["supercurrent"], st["normal_current"]
    a_ind = source.induced_vector_potential() if solver.screening is not None else None
    solver.note_applied(solver.field.applied(source))  # A_applied of the last step taken, where the device knows it
    data = TDGLData(ls["step"], ls["time"], ls["dt"], st["psi"], st["mu"], js, jn,
                    applied_vector_potential=solver.current_A_applied, epsilon=solver.epsilon,
                    induced_vector_potential=a_ind)
    if rec.handler is None:
        rec.saved.append(data)
        return
    fields = dict(psi=data.psi, mu=data.mu, supercurrent=js, normal_current=jn,
                  induced_vector_potential=np.zeros((solver.num_edges, 2)) if a_ind is None else a_ind)
    if solver.dynamic_vector_potential:
        fields["applied_vector_potential"] = solver.current_A_applied
    if solver.dynamic_epsilon:
        fields["epsilon"] = solver.epsilon
    state = dict(step=int(ls["step"]), time=float(ls["time"]), dt=float(ls["dt"]))
    rec.handler.save_time_step(state, fields, None if ls["step"] == 0 else rec.running.export())
    rec.saved[:] = [data]  # streaming keeps only the latest step in memory
    rec.saved_meta.append((data.step, data.time))


class RunRecord:
    """One run's progress through the stages and everything it has saved so far.  Creating it begins the first stage.

    ``per_step``: the inputs change on the host before every step, so a request is for one step.  ``handler``: an
    entered `io.DataHandler` that receives every saved step (with the running state since the previous one)."""

    def __init__(self, source, solver, options, per_step: bool = False, handler=None):
        self.source, self.solver, self.options = source, solver, options
        self.per_step, self.handler = per_step, handler
        self.stages = ([(STAGES[0], options.skip_time, False)] if options.skip_time else []) + [
            (STAGES[1], options.solve_time, True)]
        self.stage = self.i = 0
        self.done = False
        self.seeded = solver.seed_solution is not None or getattr(solver, "seed_state", None) is not None
        self.saved, self.saved_meta = [], []
        self.dyn = dict(dt=[], time=[], mu=[], theta=[], pcg_iters=[], screening_iterations=[], census=[])
        self.census_loops = getattr(solver, "census_loops", None)  # names of the census' loops; None: no census
        self.cores = [] if getattr(solver, "records_cores", False) else None  # SolverOptions.vortex_cores: per run call
        self.saved_rows = 0  # rows of the saved stage's dynamics so far
        self.n_steps = dict.fromkeys(STAGES, 0)
        self.running = None  # the per-step scalars between two saves: kept for a handler only
        if handler is not None:
            sizes = {"dt": 1}
            if solver.probe_points is not None:
                sizes["mu"] = sizes["theta"] = len(solver.probe_points)
            if solver.screening is not None:
                sizes["screening_iterations"] = 1
            if self.census_loops is not None:
                sizes["vortex_counts"], sizes["windings"] = 2, len(self.census_loops)
            self.running = RunningState(sizes, self.options.save_every)
        self.loop = None  # the loop state before the steps last asked for
        source.begin_stage()

    @property
    def since_save(self) -> int:
        """Steps of this stage taken since a save was last due (runner.py:398-401)."""
        return self.i % self.options.save_every

    def request(self):
        """``(max_steps, end_time)`` to ask ``run`` for next; takes the save that is due first.  A finished run asks
        for no steps."""
        if self.done:
            return 0, 0.0
        _, end_time, save = self.stages[self.stage]
        if self.since_save == 0:
            if save:
                save_step(self.source, self.solver, self)
            if self.running is not None:
                self.running.clear()
        self.loop = self.source.loop_state()
        return (1 if self.per_step else self.options.save_every - self.since_save), end_time

    def absorb(self, res) -> None:
        """Book the steps one ``run`` call took (``res``: its result for this run; fewer steps than asked for are
        fine) and, when they reached the stage's end, close the stage."""
        name, _, save = self.stages[self.stage]
        k, reached = len(res["dt"]), res["reached_end"]
        self.n_steps[name] += k
        if self.running is not None:
            if self.census_loops is not None:
                res = dict(res, **census_columns(res["census"]))
            cols = {key: res[key] for key in self.running.names_and_sizes if res[key] is not None}
            # (the step that ends the loop is written into the buffer but not counted, runner.py:429-432)
            self.running.extend({key: v[:k - 1] if reached else v for key, v in cols.items()})
            if reached:
                for key, v in cols.items():
                    self.running.append(key, np.asarray(v[k - 1]).reshape(-1))
        if save:
            if self.cores is not None and res.get("cores") is not None:
                self.cores.append(dict(res["cores"], steps=res["cores"]["steps"] + self.saved_rows))
            self.saved_rows += k
            self.dyn["time"].append(self.loop["time"] + np.concatenate([[0.0], np.cumsum(res["dt"][:-1])]))
            for key, column in self.dyn.items():
                if key != "time" and res.get(key) is not None:
                    column.append(res[key])
        if not reached:
            self.i += k
            return
        self.i += k - 1
        if save and self.since_save:
            save_step(self.source, self.solver, self, final=True)
        if self.stage + 1 < len(self.stages):
            self.stage += 1
            self.i = 0
            self.source.begin_stage()
        else:
            self.done = True

    def solution(self, total_seconds: float, **stats) -> Solution:
        """The run as a `Solution`; ``stats``: the caller's entries, after the step counts."""
        s, d = self.solver, self.dyn
        cat = lambda xs: np.concatenate(xs) if xs else np.array([])  # noqa: E731
        dt = cat(d["dt"])
        # (a library that reports no iteration counts -- the ensemble's direct mu solve -- took none)
        pcg = cat(d["pcg_iters"]) if d["pcg_iters"] else np.zeros(len(dt), dtype=np.int32)
        census = {}
        if self.census_loops is not None:
            rows = cat(d["census"]).astype(np.int32).reshape(-1, 2 + len(self.census_loops))
            census = dict(vortex_counts=rows[:, :2].T.copy(), windings=rows[:, 2:].T.copy(), loop_names=tuple(self.census_loops))
        if self.cores is not None:
            from .vortices import VortexCores

            join = lambda key, empty: np.concatenate([c[key] for c in self.cores]) if self.cores else empty  # noqa: E731
            steps = join("steps", np.zeros(0, dtype=np.int64))
            census["vortex_cores"] = VortexCores(
                steps, (cat(d["time"]) + dt)[steps], join("counts", np.zeros(0, dtype=np.int64)), join("complete", np.zeros(0, dtype=bool)),
                join("positions", np.zeros((0, 2))), join("charges", np.zeros(0, dtype=np.int32)),
                join("triangles", np.zeros(0, dtype=np.int32)), device=s.device)
        dynamics = DynamicsData(
            **census,
            dt=dt, time=cat(d["time"]), mu=cat(d["mu"]).T if d["mu"] else None,
            theta=cat(d["theta"]).T if d["theta"] else None, pcg_iterations=pcg,
            screening_iterations=cat(d["screening_iterations"]) if s.screening is not None else None,
        )
        return Solution(
            device=s.device, options=self.options, saved_steps=self.saved, dynamics=dynamics,
            dynamic_vector_potential=s.dynamic_vector_potential, dynamic_epsilon=s.dynamic_epsilon,
            applied_vector_potential=s.applied_vector_potential, terminal_currents=s.terminal_currents,
            disorder_epsilon=s.disorder_epsilon, total_seconds=total_seconds,
            stats=dict(steps_thermalizing=self.n_steps[STAGES[0]], steps_simulating=self.n_steps[STAGES[1]],
                       mean_pcg_iterations=float(pcg.mean()) if len(pcg) else 0.0, **stats),
        )
