"""A psi update that fails at exactly ONE site, in a prescribed workgroup of `psi_update_body` -- the input and the
oracle record for tests/test_local_failure_host.py (CPU) and tests/test_hip_local_failure.py (GPU).

`psi_update_body` (csrc/kernels.inc) reports a step's outcome as one failure flag and one max d|psi|^2 per workgroup
of 256 rows; every reader of those arrays has its own indexing.  A time step far beyond stability fails everywhere at
once and sets every flag, so a reader that looks at the wrong entries passes.  Here the disorder parameter is 1
everywhere except epsilon_s << 0 at one site s: the discriminant of the quadratic for |psi'|^2 is negative at s alone
until dt has shrunk far enough, and the largest d|psi|^2 of the accepted attempt sits at s as well.

The helper's own conditions keep a test built on it from hiding a failure; `oracle_steps` asserts them on every call:

  * every failing attempt fails at exactly the spiked site;
  * min |disc| >= 1 over all sites on every attempt of every step used (no decision near a tie: disc elsewhere is
    ~676 with a rounding of ~1e-10);
  * the argmax of d|psi|^2 of every accepted spiked step is the spiked site.
"""

import functools
from types import SimpleNamespace

import numpy as np

from helpers import GAMMA_DEFAULT, U_DEFAULT, synthetic_mesh, uniform_field_A

WORKGROUP = 256          # rows per workgroup of psi_update_body (BLOCK, csrc/tdgl_internal.h)
DT_INIT = 1e-3
MULTIPLIER = 0.25
FIELD = 0.2
EPS_ONE_RETRY = -3.0e4   # fails at dt = 1e-3, succeeds at dt / 4
EPS_THREE_SHRINKS = -1.0e6
N_STEPS = 3              # a fourth step brings |disc| at the spiked site down to 0.17: stop at three
MIN_ABS_DISC = 1.0


def spiked_problem(mesh, site, eps_spike, seed=0):
    """A, epsilon, psi_0, mu_0 and options: epsilon = 1 except ``eps_spike`` at ``site`` (``site=None``: no spike).
    psi_0 = (0.5 + 0.5 rand) exp(0.3i randn), mu_0 = 0.1 randn from ``seed`` alone, so that problems on one mesh
    that differ in the spike share their start."""
    n = len(mesh.sites)
    rng = np.random.default_rng(seed)
    psi0 = (0.5 + 0.5 * rng.random(n)) * np.exp(0.3j * rng.standard_normal(n))
    mu0 = 0.1 * rng.standard_normal(n)
    eps = np.ones(n)
    if site is not None:
        eps[int(site)] = float(eps_spike)
    options = SimpleNamespace(
        solve_time=1e9, skip_time=0.0, dt_init=DT_INIT, dt_max=0.1, adaptive=True, adaptive_window=10,
        max_solve_retries=10, adaptive_time_step_multiplier=MULTIPLIER, save_every=10**9, terminal_psi=None)
    return dict(mesh=mesh, site=None if site is None else int(site), A=uniform_field_A(mesh, FIELD), epsilon=eps,
                psi0=psi0, mu0=mu0, options=options, u=U_DEFAULT, gamma=GAMMA_DEFAULT)


def discriminant(psi, abs_sq_psi, mu, epsilon, gamma, u, dt, lap_psi):
    """disc of `oracle.tdgl_step.psi_update`, the same expressions in the same order (``lap_psi`` = L psi)."""
    phase = np.exp(-1j * mu * dt)
    z = phase * gamma**2 / 2 * psi
    w = z * abs_sq_psi + phase * (psi + (dt / u) * np.sqrt(1 + gamma**2 * abs_sq_psi) * ((epsilon - abs_sq_psi) * psi + lap_psi))
    c = w.real * z.real + w.imag * z.imag
    b = 2 * c + 1
    w2 = np.absolute(w) ** 2
    return b**2 - 4 * np.absolute(z) ** 2 * w2, b, w2


_SOLVERS = {}


def _recording_solver(problem, max_solve_retries):
    """One `OracleSolver` per mesh (its LU does not depend on epsilon), with the controller reset."""
    from oracle import OracleSolver, psi_update

    class Recording(OracleSolver):
        """`OracleSolver._euler_step` with every attempt written down (same calls, same decisions)."""

        def _euler_step(self, step, psi, abs_sq_psi, mu, dt):
            opts = self.options
            lap = self.operators.psi_laplacian
            lap_psi = lap @ psi
            args = (psi, abs_sq_psi, mu, self.epsilon, self.gamma, self.u)
            attempts = []
            self.attempts.append(attempts)
            retries = 0
            while True:
                with np.errstate(all="raise"):  # (no overflow: the margin conditions rule it out)
                    disc = discriminant(*args, dt, lap_psi)[0]
                result = psi_update(*args, dt, lap)
                attempts.append(dict(dt=float(dt), bad_sites=np.flatnonzero(disc < 0), min_abs_disc=float(np.abs(disc).min()),
                                     failed=result is None))
                assert (result is None) == bool(np.any(disc < 0))
                if result is not None:
                    break
                if not opts.adaptive or retries > opts.max_solve_retries:
                    raise RuntimeError(
                        f"Solver failed to converge in {opts.max_solve_retries}"
                        f" retries at step {step} with dt = {dt:.2e}."
                        f" Try using a smaller dt_init."
                    )
                dt = dt * opts.adaptive_time_step_multiplier
                retries += 1
            d = np.absolute(result[1] - abs_sq_psi)
            self.accepted.append(dict(dmax=float(d.max()), argmax=int(np.argmax(d)), abs_sq=result[1]))
            return result[0], result[1], dt

    mesh = problem["mesh"]
    key = id(mesh)
    if key not in _SOLVERS:
        _SOLVERS.clear()  # (one mesh at a time: the factors of a 65k-site mesh are not kept beyond their use)
        _SOLVERS[key] = (mesh, Recording(mesh, problem["A"], 1.0, problem["u"], problem["gamma"], problem["options"]))
    solver = _SOLVERS[key][1]
    solver.options = SimpleNamespace(**vars(problem["options"]))
    solver.d_psi_sq_vals = []
    solver.tentative_dt = solver.options.dt_init
    solver.attempts, solver.accepted = [], []
    return solver


def oracle_steps(problem, n_steps=N_STEPS, max_solve_retries=10, warm_steps=0):
    """``warm_steps`` spike-free steps from (psi_0, mu_0), then ``n_steps`` with the problem's epsilon, by `OracleSolver`.
    ``max_solve_retries``: one budget, or one per step (warm steps included).

    Returns ``dict(attempts, steps, warm, error, retries, dts)``: per spiked step the list of its attempts
    (``dt, bad_sites, min_abs_disc, failed``), per accepted step ``dt, psi, mu, js, jn, dmax, argmax`` (``warm``: the
    same for the spike-free steps), the oracle's `RuntimeError` text when the retry budget was spent (the steps before
    it are returned), the number of failed attempts of the accepted steps and their dts.  Asserts the helper's three
    conditions (module docstring) on every attempt made."""
    solver = _recording_solver(problem, max_solve_retries)
    budgets = np.broadcast_to(np.asarray(max_solve_retries, dtype=int), (warm_steps + n_steps,))
    site = problem["site"]
    psi, mu = problem["psi0"].copy(), problem["mu0"].copy()
    t, dt = 0.0, problem["options"].dt_init
    out = dict(attempts=[], steps=[], warm=[], error=None, retries=0)
    for k in range(warm_steps + n_steps):
        spiked = k >= warm_steps
        solver.epsilon = problem["epsilon"] if spiked else np.ones(len(psi))
        n_acc = len(solver.accepted)
        solver.options.max_solve_retries = int(budgets[k])
        try:
            dt, psi, mu, js, jn = solver.update({"step": k, "time": t, "dt": dt}, None, dt, psi=psi, mu=mu)
        except RuntimeError as exc:
            out["error"] = str(exc)
        attempts = solver.attempts[-1]
        for a in attempts:
            assert a["min_abs_disc"] >= MIN_ABS_DISC, (k, a["dt"], a["min_abs_disc"])
            if a["failed"]:
                assert spiked and site is not None and list(a["bad_sites"]) == [site], (k, a["dt"], a["bad_sites"], site)
            else:
                assert len(a["bad_sites"]) == 0
        if spiked:
            out["attempts"].append(attempts)
        if out["error"] is not None:
            assert len(solver.accepted) == n_acc
            break
        acc = solver.accepted[-1]
        rec = dict(dt=float(dt), psi=psi.copy(), mu=mu.copy(), js=js, jn=jn, dmax=acc["dmax"], argmax=acc["argmax"],
                   abs_sq=acc["abs_sq"])
        assert solver.d_psi_sq_vals[-1] == acc["dmax"]
        if spiked:
            if site is not None:
                assert acc["argmax"] == site, (k, acc["argmax"], site)
            out["steps"].append(rec)
            out["retries"] += len(attempts) - 1
        else:
            out["warm"].append(rec)
        t += dt
    assert float(solver.tentative_dt) == problem["options"].dt_init  # (the controller's window is not reached)
    out["dts"] = np.array([s["dt"] for s in out["steps"]])
    return out


def dmax_conditioning(problem, rec_before, rec_after, lap_row):
    """|d|psi|^2 at the spiked site in fp64 - the same formula in ``np.longdouble``| for one accepted step: what the
    oracle's own fp64 value of the controller's history entry is worth.  ``rec_before`` / ``rec_after``: (psi, mu)
    the step started from and the accepted record; ``lap_row``: row s of the psi Laplacian (dense, complex)."""
    s = problem["site"]
    psi, mu = rec_before
    ld, cld = np.longdouble, np.clongdouble
    lap_psi = (lap_row.astype(cld) * psi.astype(cld)).sum()
    p = cld(psi[s])
    a2 = p.real * p.real + p.imag * p.imag
    disc, b, w2 = discriminant(p, a2, ld(mu[s]), ld(problem["epsilon"][s]), ld(problem["gamma"]), ld(problem["u"]),
                               ld(rec_after["dt"]), lap_psi)
    new_sq = (2 * w2) / (b + np.sqrt(disc))
    return abs(float(abs(new_sq - a2)) - rec_after["dmax"])


def oracle_solver(problem):
    """The mesh's `OracleSolver` (operators, LU) behind `oracle_steps`."""
    return _recording_solver(problem, 10)


def conditions_hold(problem, **kw) -> bool:
    """Whether `oracle_steps` accepts the problem (its three conditions) -- to choose a lane by, never a tolerance."""
    try:
        oracle_steps(problem, **kw)
    except AssertionError:
        return False
    return True


@functools.lru_cache(maxsize=None)
def mesh_small():
    """1,452 sites: 6 psi workgroups, the last one with 172 rows."""
    return synthetic_mesh(40, 30, pitch=1.0, jitter=0.05, seed=2)


@functools.lru_cache(maxsize=None)
def mesh_17_workgroups():
    """4,099 sites: 17 psi workgroups, the last one with 3 rows."""
    from dense_reference import mesh_with_sites

    return mesh_with_sites(4099)


@functools.lru_cache(maxsize=None)
def mesh_258_workgroups():
    """65,862 sites: 258 psi workgroups -- the readers' ``for (k = threadIdx.x; k < nfail; k += 256)`` loops take a
    second trip, whose first entry is workgroup 256; the last workgroup (257) has 70 rows."""
    return synthetic_mesh(238)


def workgroups(ctx):
    """Number of psi workgroups of the context's own rows (`ctx->psi_blocks` below the 2,048 cap)."""
    return -(-int(ctx.n_owned) // WORKGROUP)


def site_in_workgroup(ctx, w, lane, owned_global_ids=None):
    """External site index of internal row ``256 w + lane``.

    Direction: ``ctx.perm[internal] = external`` -- `tdgl_create` reads ``site_perm[i]`` as the external site stored
    in internal row i and builds its inverse from it, exactly as ``TDGLContext.iperm[perm] = arange(n)``, so
    ``ctx.iperm[external] = internal`` (asserted here).  ``w < 0`` counts from the last workgroup; ``lane=None`` is
    the last valid lane of workgroup ``w``.  For a rank of a decomposition (no reordering: its rows are its owned sites in
    order, then the ghosts) pass the local-to-global map of its owned rows as ``owned_global_ids``; the result is then
    a global site index."""
    nw = workgroups(ctx)
    w = w % nw
    last = min(WORKGROUP, int(ctx.n_owned) - WORKGROUP * w) - 1
    lane = last if lane is None else int(lane)
    assert 0 <= lane <= last
    row = WORKGROUP * w + lane
    site = int(ctx.perm[row])
    assert int(ctx.iperm[site]) == row
    if owned_global_ids is not None:
        assert site == row and len(owned_global_ids) == ctx.n_owned
        return int(owned_global_ids[row])
    return site


def host_order(mesh, direct_solve=True):
    """``(perm, sub_ptrs)`` a `TDGLContext` on ``mesh`` would have under the size limits in force now -- the lines of
    `TDGLContext.__init__` that choose the site order, which need no GPU (the GPU tests assert that their context's
    ``perm`` equals this one, so the CPU test checks the very sites they spike)."""
    from tdgl_amd.hipcore import TDGLContext, rcm_permutation

    em = mesh.edge_mesh
    stub = object.__new__(TDGLContext)
    stub.n = len(mesh.sites)
    stub._sub_ptrs, stub._pd_order = [], None
    stub.mu = TDGLContext.mu_plan(stub.n, 0, bool(direct_solve), None, reordered=True)
    perm = rcm_permutation(em.edges, stub.n)
    if stub.mu.levels:
        perm = stub._dissection_order(mesh, em, perm)
    stub._ctx = None  # (nothing to destroy)
    return np.asarray(perm), [np.asarray(p) for p in stub._sub_ptrs]


def spike_sites(perm, sub_ptrs=()):
    """The three spiked sites of a case: the first lane of workgroup 0, the first lane of a middle workgroup and the
    last valid lane of the last, partially filled workgroup (n mod 256 not in {0, 1}).  Under a dissection order the
    first is a row of a part interior and the last a row of the top separator (asserted)."""
    n = len(perm)
    assert n % WORKGROUP not in (0, 1)
    nw = -(-n // WORKGROUP)
    rows = dict(first=0, middle=WORKGROUP * (nw // 2), last=n - 1)
    if len(sub_ptrs):
        assert rows["first"] < sub_ptrs[0][-1] and rows["last"] >= sub_ptrs[-1][-1]
    return {k: (r // WORKGROUP, int(perm[r])) for k, r in rows.items()}


def last_workgroup_site(mesh, perm, eps_spike, **oracle_kw):
    """The site of the highest row of the last workgroup for which `oracle_steps(**oracle_kw)` accepts the spike
    (``eps_spike`` = -1e6 leaves |disc| < 1 at some boundary sites: those lanes are passed over)."""
    n = len(perm)
    for row in range(n - 1, WORKGROUP * ((n - 1) // WORKGROUP) - 1, -1):
        if conditions_hold(spiked_problem(mesh, int(perm[row]), eps_spike), **oracle_kw):
            return (n - 1) // WORKGROUP, int(perm[row])
    raise AssertionError("no lane of the last workgroup meets the helper's conditions")
