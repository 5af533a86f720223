"""Recorded steps of the oracle WITH screening, for the teacher-forced tests of `step_screening` (csrc/run.inc,
csrc/screening.inc): the configurations, and for chosen steps of each everything the step starts from and produces.

A configuration is run once through `OracleSolver(..., screening=...)`.  At every chosen step k the state the step
starts from is kept (psi, mu, A_induced, the controller's tentative dt, the time, the boundary values of mu and, with a
moving field, the previous A and dt), and the step is taken THREE times from it, the oracle's own state
(`A_induced`, `tentative_dt`, the controller's history, the applied field it holds) put back before each:

  * ``whole``:  with the configuration's tolerance -- the step of the trajectory itself;
  * ``again``:  the same once more: the save and restore must reproduce it bit for bit;
  * ``single``: with tolerance 1e300, so that exactly one screening iteration runs (the loop is left when
    ``error < tolerance`` and the error starts at infinity): links from A_applied + A_induced, psi update, mu solve,
    currents, site average, 1/r sum, one heavy-ball update from zero velocity.

Per take: ``dt, psi, mu, js, jn, A_induced, iterations``, the relative change ``errors`` after every screening
iteration (`OracleSolver.last_screening_errors`), and ``attempts``: for every psi update tried, its dt, whether it failed and ``margin``, the smallest
``disc / (b^2 + 4 |z|^2 |w|^2)`` over the sites (disc = b^2 - 4 |z|^2 |w|^2 is what `psi_update` tests the sign of: the
decision survives a relative perturbation delta of either term as long as |margin| > delta).

Sizes: `set_screening_impl` splits the sites into tiles of 256 (one chunk per tile below ~12k sites) and
`k_induced_vector_potential` takes 512 edges per workgroup, `k_polyak` 256.
"""

from types import SimpleNamespace

import numpy as np

from conftest import load_golden
from helpers import GAMMA_DEFAULT, U_DEFAULT, edge_terminal, reference_mesh, uniform_field_A
from local_failure import discriminant

TOLERANCE = 1e-3
ONE_ITERATION = 1e300    # every finite error is below it: the loop is left after its first iteration
MARGIN_ERROR = 1e-6      # |e_i - tol| / tol of every iteration used: three decades above the one-step deviation 1e-9
MARGIN_DISC = 1e-9
MIN_A_INDUCED = 1e-3     # a step "really screens" when max |A_induced| after it exceeds this

_STRIP = dict(mesh="mesh_strip", terminals=(-30.0, 30.0), current=4.0, b=0.1, area_scale=0.01, ramp=None,
              step_size=0.1, step_drag=0.5, max_iterations=400, adaptive=True)
CONFIGS = {
    # 1107 sites = 4 * 256 + 83: five chunks, the last tile partial; 3163 edges: 7 edge blocks, 13 of k_polyak
    "C1": dict(_STRIP, dt_init=1e-3, dt_max=0.1, steps=(0, 2, 3, 12, 15), n_steps=20),
    # ... and every step's first psi update fails inside the screening loop
    "C2": dict(_STRIP, dt_init=2.0, dt_max=2.0, steps=(0, 1, 5), n_steps=10),
    # 516 sites: three chunks; 1458 edges: three edge blocks.  No terminals, fixed small step (with dt = 1e-3 or adaptive
    # steps the oracle itself does not converge here: the error divides by |A_e| on edges where A vanishes)
    "C3": dict(mesh="mesh_small", terminals=None, current=0.0, b=0.5, area_scale=0.05, ramp=None, step_size=0.1,
               step_drag=0.5, max_iterations=400, adaptive=False, dt_init=1e-5, dt_max=1e-5, steps=(0, 1, 4), n_steps=6),
    # the strip of C1 under A(t) = min(t / 1.0, 1) * A with a fixed small step: from step 1 on dA/dt is in the Poisson
    # right-hand side and in J_n (max |J_n| 0.32 -> 1.07) while A_induced moves
    "C5": dict(_STRIP, ramp=1.0, adaptive=False, dt_init=1e-5, dt_max=1e-5, steps=(1, 2, 5), n_steps=6),
    # C2 with dt shrunk by 0.7 per failure and six shrinks allowed per psi update (solver.py:475-485: a seventh raises):
    # step 0 fails six times in its first screening iteration and once more in its fifth, step 2 four and three times in
    # two iterations -- more than six per step, which only passes if every iteration has the whole budget again
    "C7": dict(_STRIP, dt_init=2.0, dt_max=2.0, multiplier=0.7, max_solve_retries=5, steps=(0, 2), n_steps=3),
}
# iteration counts of the oracle's first steps (tests/test_screening_step_host.py holds the helper to them)
ITERATIONS = {
    "C1": [304, 1, 14, 1, 13, 1, 12, 1, 11, 1, 10, 1, 51, 6, 6],
    "C2": [47, 21, 21],
    "C3": [23, 1, 1, 1, 1, 1],
    "C5": [19, 17, 4, 1, 1, 1],
    "C7": [37, 20, 17],
}


def problem(name):
    """Mesh, applied field, terminals, options and screening geometry of configuration ``name``."""
    c = CONFIGS[name]
    mesh = reference_mesh(load_golden(c["mesh"]))
    terms, current = [], None
    if c["terminals"]:
        terms = [edge_terminal(mesh, "source", c["terminals"][0]), edge_terminal(mesh, "drain", c["terminals"][1])]
        current = {"source": c["current"], "drain": -c["current"]}
    options = SimpleNamespace(
        solve_time=1e9, skip_time=0.0, dt_init=c["dt_init"], dt_max=c["dt_max"], adaptive=c["adaptive"],
        adaptive_window=10, max_solve_retries=c.get("max_solve_retries", 10),
        adaptive_time_step_multiplier=c.get("multiplier", 0.25), save_every=10**9, terminal_psi=0.0)
    screening = dict(sites=mesh.sites, edge_centers=mesh.edge_mesh.centers, areas=c["area_scale"] * mesh.areas,
                     tolerance=TOLERANCE, max_iterations=c["max_iterations"], step_size=c["step_size"],
                     step_drag=c["step_drag"])
    A = uniform_field_A(mesh, c["b"])
    field = scale = None
    if c["ramp"] is not None:  # A(t) = scale(t) * A
        scale = lambda t, _T=c["ramp"]: min(t / _T, 1.0)  # noqa: E731
        field = lambda t: scale(t) * A  # noqa: E731
    return SimpleNamespace(name=name, mesh=mesh, A=A, field=field, scale=scale, terminals=terms, current=current,
                           options=options, screening=screening, steps=tuple(c["steps"]), n_steps=c["n_steps"])


def _recording_oracle(p):
    from oracle import OracleSolver

    class Recording(OracleSolver):
        """`OracleSolver` that writes down every psi update it tries (same calls, same decisions)."""

        attempts = None

        def _euler_step(self, step, psi, abs_sq_psi, mu, dt):
            out = super()._euler_step(step, psi, abs_sq_psi, mu, dt)
            lap_psi = self.operators.psi_laplacian @ psi
            while True:  # the dts tried, up to the one that was accepted
                disc, b, _ = discriminant(psi, abs_sq_psi, mu, self.epsilon, self.gamma, self.u, dt, lap_psi)
                self.attempts.append(dict(dt=float(dt), failed=bool(np.any(disc < 0)),
                                          margin=float((disc / (2 * b**2 - disc)).min())))
                if dt == out[2]:
                    break
                dt = dt * self.options.adaptive_time_step_multiplier
            assert not self.attempts[-1]["failed"]
            return out

    cf = None if p.current is None else (lambda t: p.current)
    A0 = p.A if p.field is None else p.field(0.0)
    return Recording(p.mesh, A0, 1.0, U_DEFAULT, GAMMA_DEFAULT, p.options, terminals=p.terminals, current_func=cf,
                     vector_potential_func=p.field, screening=dict(p.screening))


def _save(solver):
    return dict(A_induced=solver.A_induced.copy(), tentative_dt=float(solver.tentative_dt),
                history=list(solver.d_psi_sq_vals), current_A=solver.current_A.copy())


def _restore(solver, saved):
    solver.A_induced = saved["A_induced"].copy()
    solver.tentative_dt = saved["tentative_dt"]
    solver.d_psi_sq_vals = list(saved["history"])
    solver.current_A = saved["current_A"].copy()
    solver.operators.set_link_exponents(solver.current_A)


def _take(solver, k, before, tolerance):
    """Step k from ``before`` with ``tolerance``; the oracle's own state is left as the step leaves it."""
    solver.screening["tolerance"] = tolerance
    solver.attempts = []
    state = {"step": k, "time": before["time"], "dt": before["dt_prev"]}
    dt, psi, mu, js, jn = solver.update(state, None, before["dt_prev"], psi=before["psi"].copy(), mu=before["mu"].copy())
    return dict(dt=float(dt), psi=psi.copy(), mu=mu.copy(), js=js.copy(), jn=jn.copy(), A_induced=solver.A_induced.copy(),
                iterations=int(solver.last_screening_iterations), errors=list(solver.last_screening_errors),
                attempts=solver.attempts, mu_boundary=solver.mu_boundary.copy(), A_applied=solver.current_A.copy())


_RECORDS = {}


def record(name):
    """``(problem, {k: dict(before=, whole=, again=, single=)}, iterations of every step run)`` of configuration
    ``name``; computed once per process and shared (do not write into the arrays)."""
    if name in _RECORDS:
        return _RECORDS[name]
    p = problem(name)
    solver = _recording_oracle(p)
    psi, mu = solver.psi_init.copy(), solver.mu_init.copy()
    t, t_prev, dt = 0.0, 0.0, p.options.dt_init
    rec, iterations = {}, []
    for k in range(p.n_steps):
        saved = _save(solver)
        before = dict(psi=psi.copy(), mu=mu.copy(), time=t, time_prev=t_prev, dt_prev=dt, A_induced=saved["A_induced"],
                      tentative_dt=saved["tentative_dt"], A_applied=saved["current_A"])
        if k in p.steps:
            single = _take(solver, k, before, ONE_ITERATION)
            _restore(solver, saved)
            again = _take(solver, k, before, TOLERANCE)
            _restore(solver, saved)
        whole = _take(solver, k, before, TOLERANCE)
        if k in p.steps:
            rec[k] = dict(before=before, whole=whole, again=again, single=single)
        iterations.append(whole["iterations"])
        dt, psi, mu = whole["dt"], whole["psi"], whole["mu"]
        t_prev, t = t, t + dt
    _RECORDS[name] = (p, rec, iterations)
    return _RECORDS[name]
