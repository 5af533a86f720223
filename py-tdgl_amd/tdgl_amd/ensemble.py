"""``solve_ensemble``: R independent replicas of ONE device -- an IV curve, a field sweep, a set of disorder
realisations -- advanced together in one batched time loop on the GPU (``csrc/ensemble.inc``).

Each replica is what ``tdgl.solve(device, options, ...)`` would run for its own inputs: same saved steps, dynamics,
thermalisation, adaptive dt, retries and errors.  The replicas share the device, its mesh and the ``SolverOptions``;
the mu solve is the dense pseudo-inverse of the Poisson matrix up to ``ENSEMBLE_DENSE_MAX_SITES`` sites and the
substructured direct solve of one or two levels above (`ensemble_mu_path`), applied to all replicas' right-hand
sides in one pass over the factors per group of replicas.  A replica may be time dependent in the three forms the device evaluates itself, each with its own
parameters: a field ramp ``LinearRamp * (static field)`` or field table ``TabulatedRamp * (static field)``, or a sum of
a static field and up to four such products (``ConstantField(b) + TabulatedRamp(...) * <local field>``),
``TabulatedCurrents`` and a ``SeparableEpsilon``.  Not supported: other time-dependent inputs, a field ramp or field
table combined with one of the other tables in one replica, screening, ``output_file``, more
than ``ENSEMBLE_MAX_SITES`` sites.

The per-replica set-up (vector potential, epsilon, terminal currents -> mu boundary values) is ``TDGLSolver``'s
own, run without creating a device context (``_ReplicaInputs``); the stage loop is ``TDGLSolver.solve``'s too: one
``runloop.RunRecord`` per replica, all served by one ``EnsembleContext.run`` call per round.
"""

import ctypes as C
import time as _time
from typing import Callable, Dict, List, Optional, Sequence, Union

import numpy as np

from . import _lib
from ._lib import c128, f64, p_f64, p_i32
from .device import Device
from .hipcore import (FIELD_TERMS_MAX, TDGLContext, controller_struct, epsilon_spots_args, epsilon_table_args, link_table_args,
                      link_terms_args, mu_boundary_table_args, probe_args, read_census, read_loop_state)
from .options import SolverOptions, SolverOptionsError
from .runloop import RunRecord, check_epsilon_table, check_seed
from .solution import Solution
from .solver import TDGLSolver, install_census

# The ensemble's mu solve by mesh size, set by measurement (DESIGN.md "Ensembles").  Up to ENSEMBLE_DENSE_MAX_SITES the
# dense inverse (n^2 / 2 doubles, read once per 16 replicas and round: at R = 32 the ensemble's aggregate rate over
# tdgl.solve run one replica after another falls from 5.4x at 5,791 sites to 1.4x at 11,774 and 0.85x at 15,745 sites);
# above it the substructured factors of the single run (growing like n^1.5, read once per 8 replicas and round), one
# level up to ENSEMBLE_SUB_MAX_SITES (the single run's `TDGLContext.SUB_MAX_SITES`), two levels up to
# ENSEMBLE_MAX_SITES -- the single run's `DIRECT_SWITCH_MIN_SITES`, below which it takes the direct solve in every state.
ENSEMBLE_DENSE_MAX_SITES = 12_000
ENSEMBLE_SUB_MAX_SITES = 32_000
ENSEMBLE_MAX_SITES = 150_000


def ensemble_mu_path(n_sites: int) -> int:
    """Levels of the substructured mu solve the ensemble takes for a mesh of ``n_sites`` sites; 0: the dense inverse.
    Depends on the module's constants alone (not on `TDGLContext`'s size rule, which tests switch off)."""
    if n_sites > ENSEMBLE_MAX_SITES:
        raise ValueError(f"solve_ensemble: the mesh has {n_sites} sites, more than ENSEMBLE_MAX_SITES = {ENSEMBLE_MAX_SITES}.")
    if n_sites <= ENSEMBLE_DENSE_MAX_SITES:
        return 0
    return 1 if n_sites <= ENSEMBLE_SUB_MAX_SITES else 2


class _ReplicaInputs(TDGLSolver):
    """``TDGLSolver``'s set-up of one replica's inputs (link exponents, epsilon, terminal currents, initial values)
    without the device context: ``_setup`` stops after the host half."""

    def _setup(self, mesh) -> None:
        self._setup_host(mesh)
        self.ctx = None
        self._currents_on_device = self._epsilon_on_device = False
        self._evaluate_mu_boundary(0.0)


def _is_per_replica(value) -> bool:
    return isinstance(value, (list, tuple)) or (isinstance(value, np.ndarray) and value.ndim == 1)


def broadcast_replicas(**per_replica) -> tuple:
    """``(R, {name: list of R values})``: a list (tuple, 1-D array) gives one value per replica, anything else is
    the value of every replica.  R is the length of the lists (1 without any); lists of different lengths raise."""
    lengths = {name: len(v) for name, v in per_replica.items() if _is_per_replica(v)}
    if len(set(lengths.values())) > 1:
        raise ValueError(f"solve_ensemble: per-replica lists of different lengths: {lengths}")
    R = next(iter(lengths.values())) if lengths else 1
    if R < 1:
        raise ValueError(f"solve_ensemble: empty per-replica lists: {lengths}")
    return R, {name: list(v) if name in lengths else [v] * R for name, v in per_replica.items()}


def _refuse_options(options: SolverOptions, n_sites: int) -> None:
    if options.vortex_cores:
        raise SolverOptionsError("solve_ensemble: vortex_cores=True is not supported (the ensemble counts, "
                                 "vortex_census=True, but does not record cores); use tdgl.solve per replica.")
    if options.include_screening:
        raise ValueError("solve_ensemble: include_screening=True is not supported (the ensemble has static link variables).")
    if options.output_file is not None:
        raise ValueError("solve_ensemble: output_file is not supported (the solutions are returned in memory).")
    ensemble_mu_path(n_sites)  # (raises above ENSEMBLE_MAX_SITES)
    if options.adaptive and not 1 <= options.adaptive_window <= 128:
        raise ValueError(f"solve_ensemble: adaptive_window must be in [1, 128] (got {options.adaptive_window}).")


def _refuse_dynamic(r: int, rep: TDGLSolver) -> None:
    """Time dependence the ensemble evaluates on the device passes: a separable A whose factor is a LinearRamp or a
    TabulatedRamp, a sum of a static field and such products, TabulatedCurrents, a SeparableEpsilon, a HotSpotEpsilon of
    up to four spots (wherever a SeparableEpsilon may stand).  Anything else raises."""
    spots = getattr(rep, "_eps_spots", None)
    if rep.field.refusal is not None:
        raise ValueError(f"solve_ensemble: replica {r}: a time-dependent applied_vector_potential is supported only as "
                         "LinearRamp(...) * (static field), TabulatedRamp(...) * (static field), or a sum (static field) + f_1 * "
                         f"(static field) + ... of up to {FIELD_TERMS_MAX} such products; {rep.field.refusal}")
    if rep.dynamic_currents and rep._current_table is None:
        raise ValueError(f"solve_ensemble: replica {r}: time-dependent terminal_currents are not supported "
                         "(TabulatedCurrents are).")
    if rep.dynamic_epsilon and rep._eps_table is None and spots is None:
        raise ValueError(f"solve_ensemble: replica {r}: a time-dependent disorder_epsilon is not supported "
                         "(SeparableEpsilon is).")
    if rep.device_evaluates_field() and (rep._current_table is not None or rep._eps_table is not None or spots is not None):
        raise ValueError(f"solve_ensemble: replica {r}: {rep.field.noun} combined with TabulatedCurrents or a SeparableEpsilon "
                         "in one replica is not supported.")


def _check_seeds(device, mesh, seeds) -> None:
    for r, seed in enumerate(seeds):
        if seed is not None:
            check_seed(seed, device, mesh, prefix=f"solve_ensemble: replica {r}: ")


def solve_ensemble(
    device: Device,
    options: SolverOptions,
    applied_vector_potential: Union[Callable, float, Sequence] = 0,
    terminal_currents: Union[Dict[str, float], None, Sequence] = None,
    disorder_epsilon: Union[float, Callable, Sequence] = 1,
    seed_solutions: Optional[Sequence[Optional[Solution]]] = None,
) -> List[Solution]:
    """Solve R replicas of one device together; returns the R ``Solution`` objects ``tdgl.solve`` returns for each
    of them alone.  Every per-replica argument is a list of length R or one value for all replicas.

    Time-dependent replicas: ``applied_vector_potential`` may be ``LinearRamp(...) * <static field>`` or
    ``TabulatedRamp(...) * <static field>`` (tables of any length, each replica its own), or a sum of a static field
    and up to four such products (`Parameter.separable_terms`; each replica its own terms),
    ``terminal_currents`` a ``TabulatedCurrents``, ``disorder_epsilon`` a ``SeparableEpsilon`` or a ``HotSpotEpsilon`` of up
    to four spots -- one replica per bias current or per absorption site -- (one kind of table or
    ramp per replica, except that tabulated currents and a separable epsilon may go together).  Static, ramped and
    tabulated replicas may share one ensemble.

    A replica that spends its retry budget raises ``RuntimeError`` with the reference's message, prefixed by the
    replica index; no solution is returned then (like ``tdgl.solve``)."""
    if device.mesh is None:
        raise ValueError("The device has no mesh: call device.make_mesh() first.")
    _refuse_options(options, len(device.mesh.sites))
    R, args = broadcast_replicas(
        applied_vector_potential=applied_vector_potential, terminal_currents=terminal_currents,
        disorder_epsilon=disorder_epsilon, seed_solutions=seed_solutions,
    )
    _check_seeds(device, device.mesh, args["seed_solutions"])
    reps = []
    for r in range(R):
        rep = _ReplicaInputs(device, options, applied_vector_potential=args["applied_vector_potential"][r],
                             terminal_currents=args["terminal_currents"][r], disorder_epsilon=args["disorder_epsilon"][r],
                             seed_solution=args["seed_solutions"][r])
        _refuse_dynamic(r, rep)
        reps.append(rep)
    return EnsembleSolver(device.mesh, options, reps).solve()


def solve_ensemble_dimensionless(mesh, options: SolverOptions, link_exponents, epsilon=1.0, u: float = 5.79,
                                 gamma: float = 10.0, terminal_info=(), currents=None, probe_points=None,
                                 seed_states=None, vector_potential_ramp=None, epsilon_table=None,
                                 vector_potential_table=None, vector_potential_terms=None, epsilon_spots=None) -> List[Solution]:
    """``solve_ensemble`` from dimensionless inputs (``TDGLSolver.from_dimensionless``): ``link_exponents`` A[m, 2]
    (an array, or a list of them), ``epsilon`` (a scalar or an [n] array, or a list), ``currents``
    ({terminal: dimensionless current} or a ``TabulatedCurrents``, or a list), ``seed_states`` (None or a list of
    (psi, mu) / None).  Time dependence, one value or a list with None for the replicas without:
    ``vector_potential_ramp`` ``(A_base[m, 2], dict(tmin, tmax, initial, final))`` as in
    ``TDGLSolver.from_dimensionless`` (the replica's ``link_exponents`` may then be None: the ramp's value at t = 0),
    ``epsilon_table`` ``(epsilon0[n], times, factor)``: epsilon(t) = PiecewiseLinear(times, factor)(t) * epsilon0,
    ``vector_potential_table`` ``(A_base[m, 2], times, values)``: A(t) = TabulatedRamp(times, values)(t) * A_base (in a
    replica without a ramp; ``link_exponents`` may be None as for a ramp), ``vector_potential_terms`` ``(A0[m, 2] or
    None, [(A_k[m, 2], spec_k), ...])`` as in ``TDGLSolver.from_dimensionless`` (in a replica without ramp and table;
    ``link_exponents`` may be None), ``epsilon_spots`` ``(eps0, [spot, ...])`` as in ``TDGLSolver.from_dimensionless`` (in a
    replica without an ``epsilon_table``)."""
    return ensemble_dimensionless(mesh, options, link_exponents, epsilon, u, gamma, terminal_info, currents, probe_points,
                                  seed_states, vector_potential_ramp, epsilon_table, vector_potential_table,
                                  vector_potential_terms, epsilon_spots).solve()


def _one_or_list(value, is_one):
    """A tuple-valued per-replica argument: one value (``is_one``) stays as it is, a list is per replica."""
    if value is None or is_one(value):
        return _Same(value)
    if not isinstance(value, list):
        raise ValueError(f"solve_ensemble: expected one value or a list of them, got {type(value).__name__}")
    return value


class _Same:
    """One value for every replica (broadcast_replicas would take a tuple for a per-replica list)."""

    def __init__(self, value):
        self.value = value


def _with_epsilon_table(rep: TDGLSolver, table, n: int) -> None:
    """epsilon(t) = PiecewiseLinear(times, factor)(t) * epsilon0 on a dimensionless replica: what the constructor does
    for a SeparableEpsilon."""
    from .parameter import PiecewiseLinear

    eps0, times, factor = table
    eps0 = np.asarray(eps0, dtype=float) * np.ones(n)
    f = PiecewiseLinear(times, factor)
    rep._eps_table = (eps0, f.times, f.values)
    rep.epsilon_func = lambda t: f(t) * eps0  # noqa: E731
    rep.dynamic_epsilon = True
    rep.disorder_epsilon = eps0
    rep.epsilon = rep.epsilon_func(0.0)


def ensemble_dimensionless(mesh, options: SolverOptions, link_exponents, epsilon=1.0, u: float = 5.79,
                           gamma: float = 10.0, terminal_info=(), currents=None, probe_points=None,
                           seed_states=None, vector_potential_ramp=None, epsilon_table=None,
                           vector_potential_table=None, vector_potential_terms=None, epsilon_spots=None) -> "EnsembleSolver":
    """The `EnsembleSolver` behind `solve_ensemble_dimensionless` (its ``solve()`` returns the solutions)."""
    _refuse_options(options, len(mesh.sites))
    per = dict(link_exponents=link_exponents, currents=currents, seed_states=seed_states)
    if isinstance(epsilon, (list, tuple)):
        per["epsilon"] = epsilon
    ramps = _one_or_list(vector_potential_ramp, lambda v: isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], dict))
    tables = _one_or_list(epsilon_table, lambda v: isinstance(v, tuple) and len(v) == 3)
    fields = _one_or_list(vector_potential_table, lambda v: isinstance(v, tuple) and len(v) == 3)
    sums = _one_or_list(vector_potential_terms, lambda v: isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], list))
    spots = _one_or_list(epsilon_spots, lambda v: isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], list))
    for name, v in (("vector_potential_ramp", ramps), ("epsilon_table", tables), ("vector_potential_table", fields),
                    ("vector_potential_terms", sums), ("epsilon_spots", spots)):
        if not isinstance(v, _Same):
            per[name] = v
    R, args = broadcast_replicas(**per)
    eps = args.get("epsilon", [epsilon] * R)
    ramps = args.get("vector_potential_ramp", [getattr(ramps, "value", None)] * R)
    tables = args.get("epsilon_table", [getattr(tables, "value", None)] * R)
    fields = args.get("vector_potential_table", [getattr(fields, "value", None)] * R)
    sums = args.get("vector_potential_terms", [getattr(sums, "value", None)] * R)
    spots = args.get("epsilon_spots", [getattr(spots, "value", None)] * R)
    reps = []
    for r in range(R):
        if ramps[r] is not None and fields[r] is not None:
            raise ValueError(f"solve_ensemble: replica {r}: vector_potential_ramp and vector_potential_table exclude each other.")
        if sums[r] is not None and (ramps[r] is not None or fields[r] is not None):
            raise ValueError(f"solve_ensemble: replica {r}: vector_potential_terms excludes vector_potential_ramp and "
                             "vector_potential_table.")
        if spots[r] is not None and tables[r] is not None:
            raise ValueError(f"solve_ensemble: replica {r}: epsilon_spots and epsilon_table exclude each other.")
        # (link_exponents None: the field's value at t = 0, `applied_field.from_dimensionless`)
        rep = _ReplicaInputs.from_dimensionless(mesh, options, args["link_exponents"][r], eps[r], u, gamma,
                                                terminal_info=terminal_info, current_func=args["currents"][r],
                                                probe_points=probe_points, vector_potential_ramp=ramps[r],
                                                vector_potential_table=fields[r], vector_potential_terms=sums[r],
                                                epsilon_spots=spots[r])
        if tables[r] is not None:
            _with_epsilon_table(rep, tables[r], len(mesh.sites))
        _refuse_dynamic(r, rep)
        if args["seed_states"][r] is not None:
            rep.seed_state = args["seed_states"][r]
        reps.append(rep)
    return EnsembleSolver(mesh, options, reps)


class EnsembleContext:
    """Owns one ``tdgl_ensemble`` attached to a ``TDGLContext`` with a direct mu solve (the dense inverse, or the
    substructured factors of one or two levels)."""

    def __init__(self, ctx, n_replicas: int):
        self.ctx = ctx
        self._lib = _lib.load()
        self.R = int(n_replicas)
        self.n_probe = 0
        self.n_census = 0  # columns of a census row as taken over by set_census; 0: off
        self._ens = C.c_void_p()
        self._chk(self._lib.tdgl_ensemble_create(C.byref(self._ens), ctx._ctx, self.R))

    def _chk(self, status):
        _lib.check(status, self.ctx._ctx)

    def close(self):
        if self._ens:
            self._lib.tdgl_ensemble_destroy(self._ens)
            self._ens = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_link_exponents(self, r, A):
        A = f64(A)
        assert A.shape == (self.ctx.m, 2)
        self._chk(self._lib.tdgl_ensemble_set_link_exponents(self._ens, r, p_f64(A)))

    def set_mu_boundary(self, r, mu_b):
        mu_b = f64(mu_b)
        assert mu_b.shape == (self.ctx.n_boundary,)
        self._chk(self._lib.tdgl_ensemble_set_mu_boundary(self._ens, r, p_f64(mu_b) if len(mu_b) else None))

    def set_epsilon(self, r, eps):
        eps = f64(np.broadcast_to(eps, (self.ctx.n,)))  # (a scalar is every site's value, as in TDGLContext.set_epsilon)
        self._chk(self._lib.tdgl_ensemble_set_epsilon(self._ens, r, p_f64(eps)))

    def set_link_ramp(self, r, A_base, tmin, tmax, initial, final):
        """A(t) = LinearRamp(tmin, tmax, initial, final)(t) * A_base, evaluated inside ``run``."""
        A_base = f64(A_base)
        assert A_base.shape == (self.ctx.m, 2)
        self._chk(self._lib.tdgl_ensemble_set_link_ramp(self._ens, r, p_f64(A_base), float(tmin), float(tmax), float(initial),
                                                        float(final)))

    def set_link_table(self, r, A_base, times, values):
        """A(t) = PiecewiseLinear(times, values)(t) * A_base, evaluated inside ``run``."""
        A_base = f64(A_base)
        assert A_base.shape == (self.ctx.m, 2)
        self._chk(self._lib.tdgl_ensemble_set_link_table(self._ens, r, p_f64(A_base), *link_table_args(times, values)))

    def link_scale(self, r) -> float:
        v = C.c_double(0)
        self._chk(self._lib.tdgl_ensemble_get_link_scale(self._ens, r, C.byref(v)))
        return v.value

    def set_link_terms(self, r, A0, terms):
        """A(t) = A0 + f_1(t) A_1 + ... + f_K(t) A_K for replica r, evaluated inside ``run``
        (``TDGLContext.set_link_terms``'s arguments)."""
        self._chk(self._lib.tdgl_ensemble_set_link_terms(self._ens, r, *link_terms_args(self.ctx.m, A0, terms)))

    def link_term_scales(self, r):
        n, v = C.c_int32(0), np.zeros(FIELD_TERMS_MAX)
        self._chk(self._lib.tdgl_ensemble_get_link_term_scales(self._ens, r, C.byref(n), p_f64(v)))
        return v[:n.value]

    def set_mu_boundary_table(self, r, times, groups, densities):
        """``TDGLContext.set_mu_boundary_table`` for replica r; ``times=None``: off."""
        self._chk(self._lib.tdgl_ensemble_set_mu_boundary_table(self._ens, r, *mu_boundary_table_args(times, groups, densities)))

    def set_epsilon_table(self, r, epsilon0, times, factors):
        """``TDGLContext.set_epsilon_table`` for replica r; ``times=None``: off."""
        self._chk(self._lib.tdgl_ensemble_set_epsilon_table(self._ens, r, *epsilon_table_args(self.ctx.n, epsilon0, times, factors)))

    def set_epsilon_spots(self, r, sites, eps0, spots):
        """``TDGLContext.set_epsilon_spots`` for replica r (the site coordinates are the ensemble's: kept from the first
        call); ``spots`` empty or None: off."""
        if not spots:
            self._chk(self._lib.tdgl_ensemble_set_epsilon_spots(self._ens, r, None, None, 0, None, None, None, None, None, None))
            return
        self._chk(self._lib.tdgl_ensemble_set_epsilon_spots(self._ens, r, *epsilon_spots_args(self.ctx.n, sites, eps0, spots)))

    def epsilon(self, r):
        """Replica r's disorder parameter ``epsilon[n]`` in force on the device, whatever set it."""
        eps = np.zeros(self.ctx.n)
        self._chk(self._lib.tdgl_ensemble_get_epsilon(self._ens, r, p_f64(eps)))
        return eps

    def set_state(self, r, psi, mu):
        psi, mu = c128(psi), f64(mu)
        assert psi.shape == (self.ctx.n,) and mu.shape == (self.ctx.n,)
        self._chk(self._lib.tdgl_ensemble_set_state(self._ens, r, p_f64(psi), p_f64(mu)))

    def set_controller(self, r, options: SolverOptions):
        c = controller_struct(options.dt_init, options.dt_max, options.adaptive, options.adaptive_window,
                              options.max_solve_retries, options.adaptive_time_step_multiplier)
        self._chk(self._lib.tdgl_ensemble_set_controller(self._ens, r, C.byref(c)))

    def set_probes(self, sites):
        sites, self.n_probe = probe_args(sites)
        self._chk(self._lib.tdgl_ensemble_set_probes(self._ens, sites, self.n_probe))

    def set_census(self):
        """Take over the context's census (``ctx.set_census(...)`` first) for every replica: `run` then returns each
        replica's ``census`` rows."""
        self._chk(self._lib.tdgl_ensemble_set_census(self._ens))
        self.n_census = self.ctx.n_census

    def begin_stage(self, r):
        self._chk(self._lib.tdgl_ensemble_begin_stage(self._ens, r))

    def loop_state(self, r):
        return read_loop_state(self._chk, self._lib.tdgl_ensemble_get_loop_state, self._ens, r)

    def run(self, max_steps, end_time):
        """Up to ``max_steps[r]`` steps of every replica r, stopping at ``end_time[r]``.  Returns a list of dicts
        (``dt``, ``mu``, ``theta``, ``reached_end``) like ``TDGLContext.run``."""
        R = self.R
        ms = np.ascontiguousarray(max_steps, dtype=np.int64)
        et = f64(end_time)
        assert ms.shape == (R,) and et.shape == (R,)
        cap = max(int(ms.max()), 1)
        npb = self.n_probe
        dts = np.zeros((R, cap))
        mu_p = np.zeros((R, cap, npb)) if npb else None
        th_p = np.zeros((R, cap, npb)) if npb else None
        done = np.zeros(R, dtype=np.int64)
        reached = np.zeros(R, dtype=np.int32)
        failed = np.zeros(R, dtype=np.int32)
        status = self._lib.tdgl_ensemble_run(
            self._ens, ms.ctypes.data_as(C.POINTER(C.c_int64)), p_f64(et), cap, p_f64(dts), p_f64(mu_p), p_f64(th_p),
            done.ctypes.data_as(C.POINTER(C.c_int64)), p_i32(reached), p_i32(failed))
        self._chk(status)
        ncen = self.n_census
        census = [read_census(self._chk, ncen, self._lib.tdgl_ensemble_get_census, self._ens, r) if ncen else None
                  for r in range(R)]
        return [dict(dt=dts[r, :done[r]], mu=None if mu_p is None else mu_p[r, :done[r]],
                     theta=None if th_p is None else th_p[r, :done[r]], reached_end=bool(reached[r]), census=census[r])
                for r in range(R)]

    def get_state(self, r, currents=True):
        n, m = self.ctx.n, self.ctx.m
        psi, mu = np.empty(n, dtype=np.complex128), np.empty(n)
        js = np.empty(m) if currents else None
        jn = np.empty(m) if currents else None
        self._chk(self._lib.tdgl_ensemble_get_state(self._ens, r, p_f64(psi), p_f64(mu), p_f64(js), p_f64(jn)))
        return dict(psi=psi, mu=mu, supercurrent=js, normal_current=jn)

    def mu_path(self):
        """``(levels, factor_bytes)``: 0 levels = the dense inverse; the bytes of the factors one round reads."""
        levels, nbytes = C.c_int32(0), C.c_int64(0)
        self._chk(self._lib.tdgl_ensemble_get_mu_path(self._ens, C.byref(levels), C.byref(nbytes)))
        return levels.value, nbytes.value

    def stats(self):
        rounds, batches = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.tdgl_ensemble_get_stats(self._ens, C.byref(rounds), C.byref(batches)))
        return dict(rounds=rounds.value, batches=batches.value)


class _Replica:
    """Replica r of an ensemble as the state source of its `runloop.RunRecord` (`TDGLContext`'s method names)."""

    def __init__(self, ens: EnsembleContext, r: int):
        self.ens, self.r = ens, r

    def begin_stage(self):
        self.ens.begin_stage(self.r)

    def loop_state(self):
        return self.ens.loop_state(self.r)

    def link_scale(self):
        return self.ens.link_scale(self.r)

    def link_term_scales(self):
        return self.ens.link_term_scales(self.r)

    def get_state(self, supercurrent=True, normal_current=True):
        return self.ens.get_state(self.r, currents=supercurrent and normal_current)


def build_context(mesh, options: SolverOptions, fixed_sites, u: float, gamma: float):
    """A single-GPU context on ``mesh`` with the ensemble's direct mu solve (`ensemble_mu_path`): the dense inverse or
    the substructured factors, whatever `TDGLContext.DENSE_MAX_SITES` / `SUB_MAX_SITES` / `SUB2_MAX_SITES` say."""
    levels = ensemble_mu_path(len(mesh.sites))
    ctx = TDGLContext(mesh, fixed_sites=fixed_sites, fix_psi=options.terminal_psi is not None, u=u, gamma=gamma,
                      device_id=options.device_id, substructure_levels=levels or None)
    try:
        # (the substructured path: one AMG hierarchy, which the ensemble never runs; the factors built explicitly)
        ctx.build_poisson(rtol=options.pcg_rtol, max_iter=options.pcg_max_iter, nu=options.amg_smoothing_sweeps,
                          dense_max_sites=ENSEMBLE_DENSE_MAX_SITES, **(dict(amg_candidates=1) if levels else {}))
        if levels and not ctx.build_substructure(check_rtol=min(1e-11, float(options.pcg_rtol))):
            raise RuntimeError("solve_ensemble: the substructured factors of the Poisson matrix could not be built "
                               f"({ctx.setup_times.get('substructure_error', 'their residual check failed')})")
        if not getattr(ctx, "dense_direct", False):
            raise RuntimeError("solve_ensemble: the dense inverse of the Poisson matrix could not be built "
                               "(a mesh in several pieces?)")
    except BaseException:
        ctx.close()
        raise
    return ctx


class EnsembleSolver:
    """The Runner's loop (runner.py:288-454, `runloop.RunRecord`) for every replica of an ensemble."""

    def __init__(self, mesh, options: SolverOptions, replicas: Sequence[TDGLSolver]):
        self.mesh = mesh
        self.options = options
        self.reps = list(replicas)

    def solve(self) -> List[Solution]:
        opts = self.options
        opts.validate()
        reps, R = self.reps, len(self.reps)
        t_start = _time.perf_counter()
        r0 = reps[0]
        ctx = build_context(self.mesh, opts, r0.fixed_sites, r0.u, r0.gamma)
        ens = None
        try:
            ens = EnsembleContext(ctx, R)
            self.mu_path = ens.mu_path()
            self.setup_seconds = _time.perf_counter() - t_start
            return self._run(ctx, ens, t_start)
        finally:
            if ens is not None:
                self.ensemble_stats = ens.stats()
                ens.close()
            ctx.close()

    def _run(self, ctx, ens: EnsembleContext, t_start: float) -> List[Solution]:
        opts = self.options
        reps, R = self.reps, len(self.reps)
        ens.set_probes(reps[0].probe_points)
        if opts.vortex_census:
            names = install_census(ctx, reps[0].device)
            ens.set_census()
            for rep in reps:
                rep.census_loops = names
        for r, rep in enumerate(reps):
            rep.field.install_replica(ens, r, rep.current_A_applied)
            ens.set_mu_boundary(r, rep.mu_boundary)
            ens.set_epsilon(r, rep.epsilon)
            if rep._current_table is not None and rep.terminal_info:
                ens.set_mu_boundary_table(r, *rep._current_table_arrays())
            if rep._eps_table is not None:
                eps0, times, values = rep._eps_table
                check_epsilon_table(eps0, values, prefix=f"replica {r}: ")
                ens.set_epsilon_table(r, eps0, times, values)
                rep._epsilon_on_device = True
            if getattr(rep, "_eps_spots", None) is not None:
                eps0, spots = rep._eps_spots
                ens.set_epsilon_spots(r, rep.sites, eps0, spots)
                rep._epsilon_on_device = True
            seed = getattr(rep, "seed_state", None)
            if rep.seed_solution is not None:
                seed = (rep.seed_solution.tdgl_data.psi, rep.seed_solution.tdgl_data.mu)
            ens.set_state(r, *(seed if seed is not None else (rep.psi_init, rep.mu_init)))
            ens.set_controller(r, opts)
        records = [RunRecord(_Replica(ens, r), rep, opts) for r, rep in enumerate(reps)]
        while not all(rec.done for rec in records):
            max_steps, end_time = zip(*(rec.request() for rec in records))
            res = ens.run(max_steps, end_time)
            for rec, out in zip(records, res):
                if not rec.done:
                    rec.absorb(out)
        ctx.synchronize()
        mu_levels = self.mu_path[0]
        total = _time.perf_counter() - t_start
        return [rec.solution(total, mu_solver="substructured_ensemble" if mu_levels else "dense_ensemble", replica=r,
                             replicas=R, **(dict(mu_levels=mu_levels) if mu_levels else {}))
                for r, rec in enumerate(records)]
