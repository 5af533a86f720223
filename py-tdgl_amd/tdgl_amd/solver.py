"""``TDGLSolver`` / ``solve``: the reference's solver API (`tdgl/solver/solver.py:88-827`,
`tdgl/solver/solve.py:9-52`) driving the HIP time-stepping core.

What runs where:

* setup (this file, Python): unit scaling of the applied vector potential and terminal
  currents, epsilon evaluation, terminal detection -- the work of
  ``TDGLSolver.__init__`` (solver.py:117-323);
* every time step (libtdgl_hip, C++/HIP): psi update with retries, Poisson solve, currents,
  probe read-out, adaptive-dt controller and the Runner loop's time/step accounting
  (``tdgl_run``); Python is entered once per ``save_every`` steps (or once per step when the
  terminal currents are a function of time, because the callable lives in Python).

Time-dependent ``applied_vector_potential`` (a ``Parameter`` with a keyword-only ``t``) and
``disorder_epsilon`` are evaluated in Python once per step and uploaded; dA/dt and the link
variables are then formed on the device (``tdgl_update_link_exponents``).
``include_screening`` runs the reference's self-consistent loop for the induced vector
potential (solver.py:522-578, 654-688) entirely on the device; Python only hands over the site /
edge coordinates and the scaled site areas (solver.py:305-309).  The stage loop around `tdgl_run` is `runloop.RunRecord`.
"""

import inspect
import logging
import numbers
import time as _time
from typing import Callable, Dict, NamedTuple, Optional, Sequence, Union

import numpy as np

from . import applied_field
from .device import Device, TerminalInfo
from .io import DataHandler, write_solution_group
from .operators import MeshOperators
from .options import SolverOptions, SolverOptionsError
from .runloop import RunRecord, check_epsilon_table, check_seed
from .solution import Solution

logger = logging.getLogger("solver")


def validate_terminal_currents(terminal_currents, terminal_info: Sequence[TerminalInfo],
                               solver_options: SolverOptions, num_evals: int = 100) -> None:
    """Terminal currents must name known terminals and sum to zero (solver.py:35-60)."""
    known = {t.name for t in terminal_info}

    def check(currents: Dict[str, float]):
        unknown = set(currents).difference(known)
        if unknown:
            raise ValueError(f"Unknown terminal(s) in terminal currents: {list(unknown)}.")
        total = sum(currents.values())
        if total:
            raise ValueError(f"The sum of all terminal currents must be 0 (got {total:.2e}).")

    if callable(terminal_currents):
        for t in np.random.default_rng().random(num_evals) * solver_options.solve_time:
            check(terminal_currents(t))
    else:
        check(terminal_currents)


class SolverResult(NamedTuple):
    """Result of one solve step (same fields as solver.py:63-85)."""

    dt: float
    psi: np.ndarray
    mu: np.ndarray
    supercurrent: np.ndarray
    normal_current: np.ndarray
    A_induced: np.ndarray
    A_applied: Optional[np.ndarray] = None
    epsilon: Optional[np.ndarray] = None


def uniform_field_vector_potential(x, y, B):
    """Symmetric-gauge vector potential of a uniform field ``B`` (in [field] * [length]),
    centred on the bounding box of the evaluation points -- what the reference's
    ``ConstantField`` evaluates (`tdgl/em.py:437-472`, `tdgl/sources/constant.py:7-21`)."""
    xs = x - (x.min() + np.ptp(x) / 2)
    ys = y - (y.min() + np.ptp(y) / 2)
    return np.stack([-B * ys / 2, B * xs / 2, np.zeros_like(xs)], axis=1)


def install_census(ctx, device) -> tuple:
    """``SolverOptions.vortex_census``: set the context's census from the device's mesh and boundary loops -- the loops
    and names `VortexFinder` uses by default -- and return the loops' names."""
    if device is None or getattr(device, "mesh", None) is None:
        raise SolverOptionsError("vortex_census=True needs a Device with a mesh (its triangles and boundary loops).")
    loops = device.boundary_sites()
    ctx.set_census(device.points, device.triangles, list(loops.values()))
    return tuple(loops)


class TDGLSolver:
    """Solver for a TDGL model; same constructor as the reference (solver.py:117-125)."""

    def __init__(
        self,
        device: Device,
        options: SolverOptions,
        applied_vector_potential: Union[Callable, float] = 0.0,
        terminal_currents: Union[Callable, Dict[str, float], None] = None,
        disorder_epsilon: Union[Callable, float] = 1.0,
        seed_solution: Optional[Solution] = None,
    ):
        self.device = device
        self.options = options
        options.validate()
        self.terminal_currents = terminal_currents
        self.seed_solution = seed_solution
        if device.mesh is None:
            raise ValueError("The device has no mesh: call device.make_mesh() first.")
        mesh = device.mesh
        em = mesh.edge_mesh
        xi = device.coherence_length
        self.u, self.gamma = device.layer.u, device.layer.gamma
        self.probe_points = device.probe_point_indices
        self.num_edges = len(em.edges)
        self.sites = xi * mesh.sites
        self.edge_centers = xi * em.centers
        self.z0 = device.layer.z0 * np.ones(len(self.edge_centers))

        # ---- applied vector potential on the edges (solver.py:158-189) ------------------
        self.applied_vector_potential = applied_vector_potential
        self.A_scale = device.field_scale(options.field_units)
        self._set_field(applied_field.from_parameter(applied_vector_potential, self.edge_centers, self.z0, self.A_scale,
                                                     float(device.layer.z0)))

        # ---- disorder parameter epsilon on the sites (solver.py:191-216) ----------------
        self.epsilon_func = None
        self.dynamic_epsilon = False
        self._eps_table = None
        self._eps_spots = None
        from .parameter import EPS_SPOTS_MAX, HotSpotEpsilon, SeparableEpsilon, TabulatedCurrents

        if isinstance(disorder_epsilon, SeparableEpsilon):  # factor(t) * static(r): evaluated on the device
            eps0 = disorder_epsilon.static_values(self.sites)
            self._eps_table = (eps0, disorder_epsilon.factor.times, disorder_epsilon.factor.values)
        # static(r) - Gaussian spots: evaluated on the device too (more spots than it takes: the per-step callable)
        if isinstance(disorder_epsilon, HotSpotEpsilon) and len(disorder_epsilon.spots) <= EPS_SPOTS_MAX:
            self._eps_spots = (disorder_epsilon.static_values(self.sites), list(disorder_epsilon.spots))
        if callable(disorder_epsilon):
            spec = inspect.getfullargspec(disorder_epsilon)
            self.dynamic_epsilon = "t" in spec.kwonlyargs
            vectorized = spec.kwonlydefaults is not None and spec.kwonlydefaults.get("vectorized", False)

            def evaluate(**kw):  # solver.py:211-214, 364-381
                if vectorized:
                    return np.asarray(disorder_epsilon(self.sites, **kw), dtype=float)
                return np.array([float(disorder_epsilon(r, **kw)) for r in self.sites])

            if self.dynamic_epsilon:
                self.epsilon_func = lambda t: evaluate(t=t)  # noqa: E731
                epsilon = evaluate(t=0)
            else:
                epsilon = evaluate()
        else:
            epsilon = float(disorder_epsilon) * np.ones(len(self.sites))
        if np.any(epsilon > 1):
            raise ValueError("The disorder parameter epsilon must be <= 1")
        self.disorder_epsilon = disorder_epsilon
        self.epsilon = epsilon

        # ---- terminals and currents (solver.py:224-265) ------------------------------------
        self.terminal_info = device.terminal_info()
        self.terminal_names = [t.name for t in self.terminal_info]
        for t in self.terminal_info:
            if t.length == 0:
                raise ValueError(
                    f"Terminal {t.name!r} does not contain any points on the boundary of the mesh."
                )
        if terminal_currents and device.probe_points is None:
            logger.warning("The terminal currents are non-null, but the device has no probe points.")
        names = self.terminal_names
        self.dynamic_currents = callable(terminal_currents)
        if terminal_currents is None:
            terminal_currents = {name: 0 for name in names}
        if self.dynamic_currents:
            raw_func = terminal_currents
        else:
            const = {name: terminal_currents.get(name, 0) for name in names}
            unknown = set(terminal_currents).difference(names)
            if unknown:
                raise ValueError(f"Unknown terminal(s) in terminal currents: {list(unknown)}.")

            def raw_func(t):
                return const

        J_scale = device.current_scale(options.current_units)
        self._current_table = terminal_currents.scaled(J_scale) if isinstance(terminal_currents, TabulatedCurrents) else None
        self.current_func = lambda t: {k: J_scale * v for k, v in raw_func(t).items()}
        validate_terminal_currents(self.current_func, self.terminal_info, options)
        # ---- screening (solver.py:305-309) ------------------------------------------------------
        # (mu_0 / 4 pi) K0 / A0 = 1 / (pi Lambda): converts the 1/r integral of the sheet
        # current (units of K0) into a vector potential in units of A0 = xi Bc2.
        self.screening = None
        if options.include_screening:
            a_scale = 1.0 / (np.pi * device.Lambda)
            self.screening = dict(
                sites=self.sites, edge_centers=self.edge_centers, areas=a_scale * mesh.areas * xi**2
            )
        self._setup(mesh)

    @classmethod
    def from_dimensionless(cls, mesh, options: SolverOptions, link_exponents, epsilon=1.0,
                           u: float = 5.79, gamma: float = 10.0, terminal_info=(),
                           current_func=None, probe_points=None, device=None,
                           vector_potential_func=None, epsilon_func=None,
                           screening=None, vector_potential_ramp=None, vector_potential_table=None,
                           vector_potential_terms=None, vector_potential_loops=None, epsilon_spots=None) -> "TDGLSolver":
        """Build a solver directly from dimensionless inputs -- the arrays the reference's
        ``__init__`` ends up with (solver.py:185, 214, 225, 254-256): ``A[m, 2]``,
        ``epsilon[n]``, ``TerminalInfo`` records and ``t -> {name: dimensionless current}``.
        Used by the parity tests and the benchmark, whose configurations are stated in
        dimensionless form (b = B/Bc2, xi = 1).  ``screening``: ``{sites, edge_centers, areas}``
        (areas already multiplied by the kernel prefactor, solver.py:307-309); requires
        ``options.include_screening``.  ``vector_potential_ramp``: ``(A_base[m, 2], dict(tmin, tmax,
        initial, final))`` for ``A(t) = LinearRamp(t) * A_base`` evaluated by the library itself
        (then ``link_exponents`` must be its value at t = 0).  ``vector_potential_table``: ``(A_base[m, 2], times,
        values)`` for ``A(t) = TabulatedRamp(times, values)(t) * A_base``, evaluated by the library in the same way; a
        ramp and a table exclude each other.  ``vector_potential_terms``: ``(A0[m, 2] or None, [(A_k[m, 2], spec_k),
        ...])`` for the sum ``A(t) = A0 + f_1(t) A_1 + ... + f_K(t) A_K`` with ``spec_k`` a ramp's dict or a table's
        ``(times, values)``, evaluated by the library as well; it excludes the ramp and the table.
        ``vector_potential_loops``: a list of up to two ``dict(radius=, times=, centers=[n, 3] (or z= with centers
        [n, 2]), currents=)`` for moving current loops on top of ``vector_potential_terms`` or, without terms, of
        ``link_exponents`` (then the static part): lengths in the mesh's units, the film at z = 0, the currents with
        mu_0, the units and the field scale folded in (`tdgl_set_link_loops`); it excludes the ramp and the table too.
        ``epsilon_spots``: ``(eps0, spots)`` for ``epsilon(r, t) = eps0(r) - sum_k a_k(t) exp(-|r - c_k(t)|^2 / (2
        sigma_k(t)^2))`` with ``eps0`` a number or ``[n]`` and ``spots`` a list of up to four `HotSpot` (or ``dict(times=,
        centers=[n, 2], amplitudes=, sigmas=)``), lengths in the mesh's units, evaluated by the library
        (`tdgl_set_epsilon_spots`; ``epsilon`` is then its value at t = 0); it excludes ``epsilon_func``."""
        self = object.__new__(cls)
        options.validate()
        self.device = device
        self.options = options
        self.terminal_currents = None
        self.seed_solution = None
        self.u, self.gamma = u, gamma
        self.probe_points = None if probe_points is None else [int(p) for p in probe_points]
        self.num_edges = len(mesh.edge_mesh.edges)
        self.sites = mesh.sites
        self.applied_vector_potential = None
        self.disorder_epsilon = epsilon
        # optional time dependence: t -> A[m, 2] / t -> epsilon[n], already dimensionless
        self._set_field(applied_field.from_dimensionless(
            mesh.edge_mesh.centers, link_exponents, vector_potential_func, ramp=vector_potential_ramp,
            table=vector_potential_table, terms=vector_potential_terms, loops=vector_potential_loops))
        self.epsilon_func = epsilon_func
        self.dynamic_epsilon = epsilon_func is not None
        self.epsilon = np.asarray(epsilon, dtype=float) * np.ones(len(mesh.sites))
        self._eps_spots = None
        if epsilon_spots is not None:
            if epsilon_func is not None:
                raise ValueError("epsilon_spots and epsilon_func exclude each other.")
            from .parameter import HotSpot, HotSpotEpsilon

            eps0, spots = epsilon_spots
            spots = [s if isinstance(s, HotSpot) else HotSpot(s["times"], s["centers"], s["amplitudes"], s["sigmas"]) for s in spots]
            source = HotSpotEpsilon(np.asarray(eps0, dtype=float) * np.ones(len(mesh.sites)), spots)
            self._eps_spots = (source.static, spots)
            self.disorder_epsilon = source
            self.epsilon_func = lambda t: source(mesh.sites, t=t)  # noqa: E731
            self.dynamic_epsilon = True
            self.epsilon = self.epsilon_func(0.0)
        if np.any(self.epsilon > 1):
            raise ValueError("The disorder parameter epsilon must be <= 1")
        info = [t if isinstance(t, TerminalInfo) else TerminalInfo(
            t["name"], t["site_indices"], t.get("edge_indices", []), t["boundary_edge_indices"], t["length"])
            for t in terminal_info]
        self.terminal_info = tuple(sorted(info, key=lambda t: t.length))
        self.terminal_names = [t.name for t in self.terminal_info]
        from .parameter import TabulatedCurrents

        self._current_table = current_func if isinstance(current_func, TabulatedCurrents) else None
        self._eps_table = None
        self.dynamic_currents = callable(current_func)
        if not self.dynamic_currents:  # None or a constant {name: current} dict
            const = {name: 0 for name in self.terminal_names}
            const.update(current_func or {})
            current_func = lambda t: const  # noqa: E731
        self.current_func = current_func
        validate_terminal_currents(self.current_func, self.terminal_info, options)
        if options.include_screening and screening is None:
            raise ValueError("include_screening=True needs the screening geometry (sites, edge_centers, areas).")
        self.screening = dict(screening) if options.include_screening else None
        self._setup(mesh)
        return self

    def _set_field(self, field: applied_field.AppliedField) -> None:
        """``field`` describes the applied vector potential from here on; the solver starts with its initial A."""
        self.field = field
        self.dynamic_vector_potential = field.time_dependent
        self.vector_potential_func = field.value if field.time_dependent else None
        A = np.asarray(field.initial, dtype=float)
        if A.shape != (self.num_edges, 2):
            raise ValueError(f"Unexpected shape for vector_potential: {A.shape}.")
        self.current_A_applied = A

    def note_applied(self, A) -> None:
        """Keep ``A``, what the field says was applied, as ``current_A_applied``; None: it has nothing newer."""
        if A is not None:
            self.current_A_applied = A

    def terms_value(self, scales) -> np.ndarray:
        """`applied_field.TermsField.terms_value` of this solver's terms."""
        return self.field.terms_value(scales)

    def _setup_host(self, mesh) -> None:
        """The host-side part of the set-up (solver.py:258-289): fixed sites, initial values, mu boundary values."""
        em = mesh.edge_mesh
        idx = [np.asarray(t.site_indices) for t in self.terminal_info]
        self.fixed_sites = np.concatenate(idx).astype(np.int64) if idx else np.array([], dtype=np.int64)
        self.terminal_current_densities = {name: 0 for name in self.terminal_names}
        self.psi_init = np.ones(len(mesh.sites), dtype=np.complex128)
        if self.options.terminal_psi is not None:
            self.psi_init[self.fixed_sites] = self.options.terminal_psi
        self.mu_init = np.zeros(len(mesh.sites))
        self.mu_boundary = np.zeros(len(em.boundary_edge_indices))

    def _setup(self, mesh) -> None:
        """Device-side set-up shared by both constructors (solver.py:258-320)."""
        options = self.options
        self._setup_host(mesh)

        # ---- operators on the device (solver.py:267-282) --------------------------------------
        terminal_psi = options.terminal_psi
        self.operators = MeshOperators(
            mesh,
            options.sparse_solver,
            fixed_sites=self.fixed_sites,
            fix_psi=(terminal_psi is not None),
            u=self.u,
            gamma=self.gamma,
            device_id=options.device_id,
            pcg_rtol=options.pcg_rtol,
            pcg_max_iter=options.pcg_max_iter,
            amg_smoothing_sweeps=options.amg_smoothing_sweeps,
            edge_currents_every_step=options.edge_currents_every_step,
            precond_fp32=options.pcg_precond_fp32,
        )
        self.operators.build_operators()
        self.ctx = self.operators.ctx
        self.note_applied(self.field.install(self.operators))

        # ---- initial values (solver.py:284-289): _setup_host ----------------------------------------
        self.ctx.set_epsilon(self.epsilon)
        self.ctx.set_mu_boundary(self.mu_boundary)
        self.ctx.set_probes(self.probe_points)
        self.census_loops = None  # names of the loops of the in-loop census; None: off
        self.records_cores = bool(options.vortex_cores)  # Solution.dynamics.vortex_cores; implies the census
        if options.vortex_census or options.vortex_cores:
            self.census_loops = install_census(self.ctx, getattr(self, "device", None))
        if options.vortex_cores:
            self.ctx.set_core_records(self.device.points, options.vortex_cores_capacity, options.vortex_cores_every)
        self.ctx.set_controller(
            options.dt_init, options.dt_max, options.adaptive, options.adaptive_window,
            options.max_solve_retries, options.adaptive_time_step_multiplier,
        )
        if self.screening is not None:
            self.ctx.set_screening(
                self.screening["sites"], self.screening["edge_centers"], self.screening["areas"],
                max_iterations=options.max_iterations_per_step, tolerance=options.screening_tolerance,
                step_size=options.screening_step_size, step_drag=options.screening_step_drag,
            )
            if options.screening_method == "tree":
                self.ctx.set_screening_tree(options.screening_tree_degree, options.screening_tree_theta)
        # tabulated time dependence: uploaded once, evaluated by tdgl_run at every step's time
        self._currents_on_device = self._epsilon_on_device = False
        if self._current_table is not None and self.terminal_info:
            self.ctx.set_mu_boundary_table(*self._current_table_arrays())
            self._currents_on_device = True
        if self._eps_table is not None:
            eps0, times, values = self._eps_table
            check_epsilon_table(eps0, values)
            self.ctx.set_epsilon_table(eps0, times, values)
            self._epsilon_on_device = True
        if self._eps_spots is not None:
            eps0, spots = self._eps_spots
            self.ctx.set_epsilon_spots(self.sites, eps0, spots)
            self._epsilon_on_device = True
        self._device_holds = None  # (psi, mu) arrays known to equal the device state

    def _current_table_arrays(self):
        """The tabulated terminal currents as ``set_mu_boundary_table`` takes them: the times, the boundary-edge
        positions of each terminal and the current density of each terminal at each time."""
        tab = self._current_table
        names = self.terminal_names
        dens = np.array([
            (-1.0 / term.length) * sum(tab.tables[nm].values for nm in names if nm != term.name and nm in tab.tables)
            * np.ones(len(tab.times))
            for term in self.terminal_info
        ])
        return tab.times, [np.asarray(t.boundary_edge_indices) for t in self.terminal_info], dens

    # -- boundary conditions --------------------------------------------------------------------
    def update_mu_boundary(self, time: float) -> bool:
        """solver.py:325-345.  Returns True if mu_boundary changed (and was re-uploaded)."""
        if self._currents_on_device:
            return False  # tdgl_run evaluates the tables itself (tdgl_set_mu_boundary_table)
        changed = self._evaluate_mu_boundary(time)
        if changed:
            self.ctx.set_mu_boundary(self.mu_boundary)
        return changed

    def _evaluate_mu_boundary(self, time: float) -> bool:
        """The host half of update_mu_boundary: self.mu_boundary at ``time``; True if it changed."""
        currents = self.current_func(time)
        changed = False
        for term in self.terminal_info:
            density = (-1 / term.length) * sum(
                currents.get(name, 0) for name in self.terminal_names if name != term.name
            )
            if density != self.terminal_current_densities[term.name]:
                self.terminal_current_densities[term.name] = density
                self.mu_boundary[term.boundary_edge_indices] = density
                changed = True
        return changed

    def device_evaluates_field(self) -> bool:
        """A(t) = f(t) * A_base with f a LinearRamp or a TabulatedRamp, or a sum of a static field and such products
        (`Parameter.separable_terms`), with or without moving current loops (`Parameter.device_sources`): the time loop
        evaluates the factors and the loops' centres and currents itself."""
        return self.field.on_device

    def device_evaluates_epsilon(self) -> bool:
        """epsilon(t) is a table or a sum of hot spots the time loop evaluates itself (tdgl_set_epsilon_table,
        tdgl_set_epsilon_spots); the host keeps a copy."""
        return self.dynamic_epsilon and self._epsilon_on_device

    def update_dynamic_inputs(self, time: float, dt_prev: float) -> None:
        """solver.py:626-648: re-evaluate A(t) (-> link variables and dA/dt with the previous
        step's dt) and epsilon(t) before a step."""
        self.note_applied(self.field.advance(self.ctx, time, dt_prev))
        if self.dynamic_epsilon:
            self.epsilon = np.asarray(self.epsilon_func(time), dtype=float)
            if not self._epsilon_on_device:  # (on the device: this is the host's copy for the saved steps)
                if np.any(self.epsilon > 1):
                    raise ValueError("The disorder parameter epsilon must be <= 1")
                self.ctx.set_epsilon(self.epsilon)

    # -- one step through the reference's method seam ---------------------------------------------
    def update(self, state: Dict[str, numbers.Real], running_state, dt: float, *, psi, mu,
               supercurrent=None, normal_current=None, induced_vector_potential=None,
               applied_vector_potential=None, epsilon=None) -> SolverResult:
        """One call of ``TDGLSolver.update`` (solver.py:580-714).

        Compatibility entry point: the fields travel host -> device -> host on every call.
        ``solve()`` does not use it; it keeps the state resident and batches steps.
        """
        ctx = self.ctx
        held = self._device_holds
        if held is None or held[0] is not psi or held[1] is not mu:
            ctx.set_state(psi, mu)
        ctx.set_loop_state(state["step"], state["time"], state.get("dt", dt))
        self.update_mu_boundary(state["time"])
        self.update_dynamic_inputs(state["time"], dt)
        if self.screening is not None and induced_vector_potential is not None:
            ctx.set_induced_vector_potential(induced_vector_potential)
        res = ctx.run(1, np.inf)
        out = ctx.get_state()
        # The identity test above skips the upload when the caller hands back exactly these
        # arrays; make them read-only so that an in-place edit (seeding a vortex, zeroing a
        # region) fails loudly instead of being ignored -- edit a copy and pass that.
        out["psi"].setflags(write=False)
        out["mu"].setflags(write=False)
        self._device_holds = (out["psi"], out["mu"])
        step_dt = float(res["dt"][0])
        if running_state is not None:
            running_state.append("dt", step_dt)
            if self.screening is not None:
                running_state.append("screening_iterations", int(res["screening_iterations"][0]))
            if self.probe_points is not None:
                running_state.append("mu", res["mu"][0])
                running_state.append("theta", res["theta"][0])
        if self.screening is not None:
            a_ind = ctx.induced_vector_potential()
        else:
            a_ind = np.zeros((self.num_edges, 2)) if induced_vector_potential is None else induced_vector_potential
        extra = []
        self.note_applied(self.field.applied(ctx))
        if self.dynamic_vector_potential:
            extra.append(self.current_A_applied)
        if self.dynamic_epsilon:
            extra.append(self.epsilon)
        return SolverResult(step_dt, out["psi"], out["mu"], out["supercurrent"], out["normal_current"], a_ind, *extra)

    # -- the whole simulation ------------------------------------------------------------------------
    def solve(self) -> Optional[Solution]:
        """Run thermalisation + simulation stages with the reference's loop semantics
        (runner.py:288-454, `runloop.RunRecord`) and return the saved steps in memory."""
        opts = self.options
        opts.validate()
        ctx = self.ctx
        t_start = _time.perf_counter()
        seed = None
        if self.seed_solution is not None:
            check_seed(self.seed_solution, self.device, self.device.mesh)
            seed = self.seed_solution.tdgl_data
        ctx.set_state(*((self.psi_init, self.mu_init) if seed is None else (seed.psi, seed.mu)))
        if self.screening is not None:  # solver.py:738-745
            a0 = None if seed is None else seed.induced_vector_potential
            ctx.set_induced_vector_potential(np.zeros((self.num_edges, 2)) if a0 is None else a0)
        ctx.set_controller(
            opts.dt_init, opts.dt_max, opts.adaptive, opts.adaptive_window,
            opts.max_solve_retries, opts.adaptive_time_step_multiplier,
        )
        # Streaming output (runner.py:104-183): with SolverOptions.output_file every saved step is
        # written when it is taken, and only the latest one is kept in memory.
        handler = None
        if opts.output_file is not None:
            handler = DataHandler(opts.output_file, file_factory=getattr(self, "_h5_file_factory", None))
            try:
                handler.__enter__()
                handler.save_mesh(self.device.mesh)
                fixed = {}
                if not self.dynamic_vector_potential:
                    fixed["applied_vector_potential"] = self.current_A_applied
                if not self.dynamic_epsilon:
                    fixed["epsilon"] = self.epsilon
                handler.save_fixed_values(fixed)
            except BaseException:
                handler.close()  # no open files / stray .tmp left behind
                raise
        try:
            # inputs that live in Python are re-evaluated before every step
            per_step = ((self.dynamic_currents and not self._currents_on_device)
                        or (self.dynamic_epsilon and not self._epsilon_on_device)
                        or (self.dynamic_vector_potential and not self.device_evaluates_field()))
            rec = RunRecord(ctx, self, opts, per_step=per_step, handler=handler)
            while not rec.done:
                chunk, end_time = rec.request()
                self.update_mu_boundary(rec.loop["time"] if self.dynamic_currents else 0.0)
                self.update_dynamic_inputs(rec.loop["time"], rec.loop["dt"])
                rec.absorb(ctx.run(chunk, end_time))
            ctx.synchronize()
        except BaseException:
            if handler is not None:  # what has been saved stays on disk
                handler.close()
            raise
        solution = rec.solution(
            _time.perf_counter() - t_start,
            # which mu solve the mesh size selected (hipcore.TDGLContext.build_poisson)
            mu_solver=("direct (substructured)" if getattr(self.ctx, "substructure", None) else
                       "direct (dense inverse)" if getattr(self.ctx, "dense_direct", False) else
                       "pcg (AMG V-cycle or fp32-stored nested-dissection factors, by predicted cost)"
                       if getattr(self.ctx, "precond_direct", None) else "amg_pcg"),
            # the direct solves' in-loop guard: largest ||b - A mu|| / ||b|| over the checked steps
            # (one per batch of queued attempts), how many were checked, and whether a check above
            # 1e-9 sent the run back to AMG-PCG (never observed; the factors deliver 1e-14)
            **{"mu_residual_" + k: v for k, v in self.ctx.direct_stats().items()},
        )
        if handler is not None:
            solution.path = handler.output_path
            solution.saved_step_index = rec.saved_meta  # (step, time) of every group data/<k> on disk
            write_solution_group(handler.output_file, solution)  # solver.py:815-826 -> Solution.to_hdf5()
            handler.close()
        return solution


def solve(
    device: Device,
    options: SolverOptions,
    applied_vector_potential: Union[Callable, float] = 0,
    terminal_currents: Union[Callable, Dict[str, float], None] = None,
    disorder_epsilon: Union[float, Callable] = 1,
    seed_solution: Optional[Solution] = None,
) -> Union[Solution, None]:
    """Solve a TDGL model (`tdgl.solve`, tdgl/solver/solve.py:9-52)."""
    solver = TDGLSolver(
        device=device,
        options=options,
        applied_vector_potential=applied_vector_potential,
        terminal_currents=terminal_currents,
        disorder_epsilon=disorder_epsilon,
        seed_solution=seed_solution,
    )
    return solver.solve()
