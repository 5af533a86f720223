"""Object wrapper over the C ABI (one method per entry point of include/tdgl_hip.h)."""

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import reverse_cuthill_mckee

from . import _lib
from ._lib import c128, f64, i32, p_f64, p_i32, p_i64
from .amg import Hierarchy, build_hierarchy


def rcm_permutation(edges: np.ndarray, n: int) -> np.ndarray:
    """Reverse Cuthill-McKee ordering of the site graph: ``perm[k]`` = reference id of the
    site stored at internal position ``k``."""
    i, j = edges[:, 0], edges[:, 1]
    g = sp.csr_matrix(
        (np.ones(2 * len(edges), dtype=np.int8), (np.concatenate([i, j]), np.concatenate([j, i]))),
        shape=(n, n),
    )
    return np.ascontiguousarray(reverse_cuthill_mckee(g, symmetric_mode=True), dtype=np.int32)


def poisson_matrix(edges, weights, n, iperm=None) -> sp.csr_matrix:
    """``A = -diag(a) L_mu``: ``A_ij = -w_ij``, ``A_ii = sum_j w_ij`` with
    ``w = dual_edge_lengths / edge_lengths`` (reference L_mu: operators.py:120-185 with
    U = 1, no fixed sites, operators.py:285)."""
    i, j = edges[:, 0], edges[:, 1]
    if iperm is not None:
        i, j = iperm[i], iperm[j]
    w = np.asarray(weights, dtype=float)
    A = sp.coo_matrix(
        (np.concatenate([-w, -w, w, w]), (np.concatenate([i, j, i, j]), np.concatenate([j, i, i, j]))),
        shape=(n, n),
    ).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


# ---- argument marshalling shared by `TDGLContext` and `ensemble.EnsembleContext` (the ensemble's entry points take the
# same arguments after a replica index).  The pointers keep their arrays alive.
def mu_boundary_table_args(times, groups, densities) -> tuple:
    """``(n_nodes, times, n_groups, group_ptr, group_pos, density)`` of tdgl_set_mu_boundary_table: ``groups[g]`` = the
    boundary-edge positions of terminal g, ``densities[g, k]`` at ``times[k]``; ``times=None`` switches the table off."""
    if times is None:
        return 0, None, 0, None, None, None
    t, d = f64(times), f64(densities)
    ptr = i32(np.concatenate([[0], np.cumsum([len(g) for g in groups])]))
    pos = i32(np.concatenate([np.asarray(g, dtype=np.int64) for g in groups]) if len(groups) else [])
    if d.shape != (len(groups), len(t)):
        raise ValueError(f"densities must have shape ({len(groups)}, {len(t)}), got {d.shape}")
    return len(t), p_f64(t), len(groups), p_i32(ptr), p_i32(pos if len(pos) else i32([0])), p_f64(d)


def epsilon_table_args(n: int, epsilon0, times, factors) -> tuple:
    """``(epsilon0, n_nodes, times, factor)`` of tdgl_set_epsilon_table on ``n`` sites; ``times=None``: off."""
    if times is None:
        return None, 0, None, None
    e0, t, fac = f64(np.broadcast_to(epsilon0, (n,))), f64(times), f64(factors)
    if t.shape != fac.shape:
        raise ValueError("times and factors must have the same length")
    return p_f64(e0), len(t), p_f64(t), p_f64(fac)


EPS_SPOTS_MAX = 4  # TDGL_EPS_SPOTS_MAX


def epsilon_spots_args(n: int, sites, eps0, spots) -> tuple:
    """``(sites, eps0, n_spots, tab_off, tab_times, tab_cx, tab_cy, tab_amp, tab_sigma)`` of tdgl_set_epsilon_spots on ``n``
    sites from ``sites`` [n, 2], the static part ``eps0`` (a number or [n]) and ``spots``: a list of `parameter.HotSpot`
    or of ``dict(times=, centers=, amplitudes=, sigmas=)``.  Shapes, the number of spots and the rules a `HotSpot` checks
    itself are refused here with ``ValueError``; the library checks the values once more."""
    from .parameter import HotSpot

    spots = [s if isinstance(s, HotSpot) else HotSpot(s["times"], s["centers"], s["amplitudes"], s["sigmas"]) for s in spots]
    if not 1 <= len(spots) <= EPS_SPOTS_MAX:
        raise ValueError(f"epsilon_spots: between 1 and {EPS_SPOTS_MAX} spots, got {len(spots)}.")
    xy = f64(sites)
    if xy.shape != (n, 2):
        raise ValueError(f"epsilon_spots: sites must have shape ({n}, 2), got {xy.shape}.")
    if not np.all(np.isfinite(xy)):
        raise ValueError("epsilon_spots: sites must be finite.")
    e0 = np.asarray(eps0, dtype=float)
    if e0.shape not in ((), (n,)):
        raise ValueError(f"epsilon_spots: eps0 must be a number or have shape ({n},), got {e0.shape}.")
    e0 = f64(np.broadcast_to(e0, (n,)))
    if not np.all(np.isfinite(e0)) or np.any(e0 > 1):
        raise ValueError("epsilon_spots: eps0 must be finite and <= 1 (the disorder parameter epsilon must be <= 1).")
    off = i32(np.concatenate([[0], np.cumsum([len(s.times) for s in spots])]))
    cols = [f64(np.concatenate([v(s) for s in spots])) for v in (
        lambda s: s.times, lambda s: s.centers[:, 0], lambda s: s.centers[:, 1], lambda s: s.amplitudes, lambda s: s.sigmas)]
    return (p_f64(xy), p_f64(e0), len(spots), p_i32(off), *[p_f64(c) for c in cols])


def link_table_args(times, values) -> tuple:
    """``(n_nodes, times, values)`` of tdgl_set_link_table; ``times=None``: off."""
    if times is None:
        return 0, None, None
    t, v = f64(times), f64(values)
    if t.ndim != 1 or t.shape != v.shape:
        raise ValueError("times and values must be one-dimensional and of equal length")
    return len(t), p_f64(t), p_f64(v)


FIELD_TERMS_MAX = 4  # TDGL_FIELD_TERMS_MAX


def link_terms_args(m: int, A0, terms) -> tuple:
    """``(A0, n_terms, bases, kind, ramp, tab_off, tab_times, tab_values)`` of tdgl_set_link_terms from ``A0`` ([m, 2]
    or None) and ``terms``: a list of ``(A_k[m, 2], spec_k)`` with ``spec_k`` a ramp's ``dict(tmin, tmax, initial,
    final)`` or a table's ``(times, values)``.  What only the shape of the arguments decides is refused here; the
    values (strictly increasing times, finite numbers, tmax > tmin, 1 <= K <= FIELD_TERMS_MAX) are the library's to
    refuse."""
    terms = list(terms)
    if A0 is not None:
        A0 = f64(A0)
        if A0.shape != (m, 2):
            raise ValueError(f"Unexpected shape for vector_potential: {A0.shape}.")
    K = len(terms)
    bases = np.zeros((max(K, 1), m, 2))
    kind = np.zeros(max(K, 1), dtype=np.int32)
    ramp = np.zeros((max(K, 1), 4))
    off = np.zeros(K + 1, dtype=np.int32)
    tt, tv = [], []
    for k, (base, spec) in enumerate(terms):
        base = f64(base)
        if base.shape != (m, 2):
            raise ValueError(f"Unexpected shape for vector_potential: {base.shape}.")
        bases[k] = base
        if isinstance(spec, dict):
            kind[k] = 1
            ramp[k] = [float(spec[name]) for name in ("tmin", "tmax", "initial", "final")]
        else:
            link_table_args(*spec)  # (its shape check)
            kind[k] = 2
            tt.append(f64(spec[0]))
            tv.append(f64(spec[1]))
        off[k + 1] = off[k] + (len(tt[-1]) if kind[k] == 2 else 0)
    times = f64(np.concatenate(tt)) if tt else np.zeros(1)
    values = f64(np.concatenate(tv)) if tv else np.zeros(1)
    return (p_f64(A0) if A0 is not None else None, K, p_f64(f64(bases)), p_i32(kind), p_f64(f64(ramp)), p_i32(off), p_f64(times),
            p_f64(values))


FIELD_LOOPS_MAX = 2  # TDGL_FIELD_LOOPS_MAX


def link_loops_args(m: int, edge_centres, z_film, loops) -> tuple:
    """``(n_loops, edge_centres, z_film, radius, tab_off, tab_times, tab_cx, tab_cy, tab_cz, tab_current)`` of
    tdgl_set_link_loops from ``edge_centres`` [m, 2], the film's height and ``loops``: a list of ``dict(times, centers
    [n, 3], currents [n], radius)`` -- every length in the units of ``edge_centres``, the currents with mu_0, the units
    and the solver's scale folded in.  Shapes, the number of loops and a loop's plane meeting the film's are refused
    here with ``ValueError``; the library checks the values once more."""
    loops = list(loops)
    if not 1 <= len(loops) <= FIELD_LOOPS_MAX:
        raise ValueError(f"between 1 and {FIELD_LOOPS_MAX} moving loops, got {len(loops)}.")
    ec = f64(edge_centres)
    if ec.shape != (m, 2):
        raise ValueError(f"Unexpected shape for the edge centres: {ec.shape}.")
    z_film = float(z_film)
    off = np.zeros(len(loops) + 1, dtype=np.int32)
    radius = np.zeros(len(loops))
    tt, cc, ii = [], [], []
    for k, lp in enumerate(loops):
        t = f64(np.atleast_1d(lp["times"]))
        c = f64(lp["centers"])
        cur = f64(np.asarray(lp["currents"], dtype=float) * np.ones(len(t)))
        if t.ndim != 1 or len(t) < 1 or c.shape != (len(t), 3) or cur.shape != t.shape:
            raise ValueError("a moving loop needs times [n], centers [n, 3] and currents [n] (or one number).")
        if np.any(np.diff(t) <= 0):
            raise ValueError("MovingCurrentLoop: times must increase strictly")
        side = c[:, 2] - z_film
        if np.any(side == 0) or np.any(side * side[0] < 0):
            raise ValueError("MovingCurrentLoop: the loop's plane must differ from the film's (centre z != layer z0, on "
                             "one side of it) at every node.")
        if not float(lp["radius"]) > 0:
            raise ValueError("MovingCurrentLoop: radius must be > 0.")
        radius[k] = float(lp["radius"])
        off[k + 1] = off[k] + len(t)
        tt.append(t), cc.append(c), ii.append(cur)
    times, cen, cur = f64(np.concatenate(tt)), np.concatenate(cc), f64(np.concatenate(ii))
    cols = [f64(cen[:, j]) for j in range(3)]
    return (len(loops), p_f64(ec), z_film, p_f64(radius), p_i32(off), p_f64(times), p_f64(cols[0]), p_f64(cols[1]), p_f64(cols[2]),
            p_f64(cur))


def controller_struct(dt_init, dt_max, adaptive, adaptive_window, max_solve_retries,
                      adaptive_time_step_multiplier) -> "_lib.Controller":
    return _lib.Controller(float(dt_init), float(dt_max), int(bool(adaptive)), int(adaptive_window),
                           int(max_solve_retries), float(adaptive_time_step_multiplier))


def census_args(triangles, loops) -> tuple:
    """``(n_tri, elements, n_loops, loop_ptr, loop_sites)`` of tdgl_set_census (the conventions of `VortexPlan`)."""
    elements = i32(np.asarray(triangles if triangles is not None else []).reshape(-1, 3))
    loops = [i32(np.asarray(loop).reshape(-1)) for loop in (loops if loops is not None else ())]
    loop_ptr = np.zeros(len(loops) + 1, dtype=np.int64)
    loop_ptr[1:] = np.cumsum([len(loop) for loop in loops])
    loop_sites = i32(np.concatenate(loops)) if loops else np.zeros(0, dtype=np.int32)
    return len(elements), elements, len(loops), loop_ptr, loop_sites


def read_census(chk, ncol, getter, *handle) -> np.ndarray:
    """All rows behind ``getter(*handle, capacity, rows, n_rows)``: asked for their number first."""
    n = C.c_int64(0)
    chk(getter(*handle, 0, None, C.byref(n)))
    rows = np.zeros((n.value, ncol), dtype=np.int32)
    if n.value:
        chk(getter(*handle, n.value, p_i32(rows), C.byref(n)))
    return rows


def read_core_records(chk, getter, *handle) -> dict:
    """Everything behind tdgl_get_core_records: asked for the numbers first."""
    ns, nr = C.c_int64(0), C.c_int64(0)
    chk(getter(*handle, 0, None, None, None, 0, None, None, None, C.byref(ns), C.byref(nr)))
    steps, counts = np.zeros(ns.value, dtype=np.int64), np.zeros(ns.value, dtype=np.int64)
    complete = np.zeros(ns.value, dtype=np.int32)
    triangles, charges = np.zeros(nr.value, dtype=np.int32), np.zeros(nr.value, dtype=np.int32)
    positions = np.zeros((nr.value, 2))
    if ns.value:
        chk(getter(*handle, ns.value, p_i64(steps), p_i64(counts), p_i32(complete), nr.value, p_i32(triangles),
                   p_i32(charges), p_f64(positions), C.byref(ns), C.byref(nr)))
    return dict(steps=steps, counts=counts, complete=complete.astype(bool), triangles=triangles, charges=charges,
                positions=positions)


def probe_args(sites) -> tuple:
    """``(sites, n_probe)`` of tdgl_set_probes; None or an empty list: no probes."""
    sites = i32([] if sites is None else sites)
    return (p_i32(sites) if len(sites) else None), len(sites)


def read_loop_state(chk, getter, *handle) -> dict:
    """The four outputs of ``getter(*handle, step, time, runner_dt, tentative_dt)``, its status through ``chk``."""
    step, t, rdt, tdt = C.c_int64(0), C.c_double(0), C.c_double(0), C.c_double(0)
    chk(getter(*handle, C.byref(step), C.byref(t), C.byref(rdt), C.byref(tdt)))
    return dict(step=step.value, time=t.value, dt=rdt.value, tentative_dt=tdt.value)


class _HierarchyInfo:
    """A rank's view of a decomposed hierarchy: the local levels plus the global sizes."""

    def __init__(self, local, sizes=None, operator_complexity=None):
        self.levels, self.coarse_pinv = local.levels, local.coarse_pinv
        self.sizes = list(sizes) if sizes is not None else local.sizes
        self.operator_complexity = operator_complexity if operator_complexity is not None else local.operator_complexity


class _Stopwatch:
    """Accumulates wall-clock seconds per set-up phase (``TDGLContext.setup_times``)."""

    def __init__(self, table, name):
        self.table, self.name = table, name

    def __enter__(self):
        import time

        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        import time

        self.table[self.name] = self.table.get(self.name, 0.0) + time.perf_counter() - self.t0


@dataclass(frozen=True)
class MuPlan:
    """What a context does about the mu equation (`TDGLContext.mu_plan`): decided once from the mesh size and the class's
    limits, it fixes the site order (`TDGLContext.__init__`) and what `TDGLContext.build_poisson` builds."""
    form: str                  # "amg": AMG-PCG alone | "dense": explicit pseudo-inverse | "sub": substructured direct solve
    #                            | "precond": three levels of fp32 factors as the CG's second preconditioner
    levels: int = 0            # dissection levels of "sub" (1-3) and "precond" (3)
    blocks: tuple = ()         # target sizes of a part, a super-block, a super-super-block (one per level)
    sparse_sep: bool = False   # separator right-hand sides through the sparse coupling blocks (no -E^T rows)
    switching: bool = False    # the time loop may pause the direct solve in stationary states
    amg_candidates: int = 1    # hierarchies built, the best one kept


_LEVEL_NAMES = (("parts", "separator"), ("super_blocks", "top_separator"), ("super_super_blocks", "top_top_separator"))


def _level_counts(levels) -> dict:
    """Parts and separator sites of every dissection level, under the names of `substructure` / `precond_direct`."""
    return {name: v for (a, b), lv in zip(_LEVEL_NAMES, levels) for name, v in ((a, lv.n_parts), (b, lv.n_sep))}


def _sym_tile_entries(m: int) -> int:
    """Entries of a symmetric m x m matrix kept as the 128 x 128 tiles on or below its diagonal (the top separator)."""
    t = (m + 127) // 128
    return t * (t + 1) // 2 * 128 * 128


def _factor_bytes(levels, tiles, sparse_sep=True, word=8, top=True) -> int:
    """Bytes one application of a dissection's explicit factors streams (``word`` bytes per entry): the G blocks of
    level k whole, or as the 16 x 16 tiles on or below their diagonal where ``tiles[k]``; the E blocks once on the way up
    and, as -E^T rows, once more on the way down unless ``sparse_sep`` replaces those by the coupling blocks (12 bytes
    per non-zero); ``top``: the last level's separator inverse."""
    tri = lambda m: ((m + 15) // 16) * (((m + 15) // 16) + 1) // 2 * 256
    entries = (sum((tri(g.shape[0]) if tiles[k] else g.size) for k, lv in enumerate(levels) for g in lv.G)
               + (1 if sparse_sep else 2) * sum(e.size for lv in levels for e in lv.E)
               + (_sym_tile_entries(levels[-1].n_sep) if top else 0))
    return int(word * entries + (12 * sum(lv.coupling.nnz for lv in levels) if sparse_sep else 0))


_BLR_ARRAYS = (("dense_ij", np.int32, "ndense", 1), ("Gd", np.float32, "ndense", 128 * 128), ("F", np.float32, "cols", 128),
               ("colbase", np.int64, "nt", 0), ("twin", np.int32, "cols", 1), ("items", np.int32, "nitems", 4),
               ("dslot_ptr", np.int32, "nt", 0), ("dslot", np.int32, "ndslot", 1))
_BLR_COUNTS = ("n", "nt", "ndense", "nitems", "cols", "ndslot", "pairs", "rank_max", "bytes", "dense_bytes")


def _blr_form_fill(size_call, fill_call=None) -> dict:
    """The two calls of a `tdgl_blr_form`: ``size_call(form)`` with every array NULL sets the counts, the arrays are
    allocated, ``fill_call(form)`` (default: the same call) fills them.  Returns the counts and the arrays (``Gd
    [ndense, 128, 128]``, ``items [nitems, 4]``, the others flat) as a dict."""
    form = _lib.BlrForm()
    size_call(form)
    arrays, keep = {}, {}
    for name, dtype, count, per in _BLR_ARRAYS:
        size = int(getattr(form, count)) * per if per else int(form.nt) + 1
        keep[name] = np.zeros(max(size, 1), dtype=dtype)  # (a count of 0: the pointer still is not NULL)
        arrays[name] = keep[name][:size]
        setattr(form, name, keep[name].ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))))
    (fill_call or size_call)(form)
    out = {name: int(getattr(form, name)) for name in _BLR_COUNTS}
    out.update(arrays)
    out["Gd"] = out["Gd"].reshape(-1, 128, 128)
    out["items"] = out["items"].reshape(-1, 4)
    return out


def host_blr_form(G, tol_abs) -> dict:
    """`tdgl_host_blr_form` (host only, no context): the block low-rank form of the symmetric ``G [n, n]`` with every
    off-diagonal 128 x 128 tile compressed to the absolute tolerance ``tol_abs``, by the code that builds the
    preconditioner's -- the counts ``n, nt, ndense, nitems, cols, ndslot, pairs, rank_max, bytes, dense_bytes`` and the
    arrays ``dense_ij, Gd, F, colbase, twin, items, dslot_ptr, dslot`` (layout: csrc/kernels.inc at BlrArgs)."""
    G = f64(G)
    n = G.shape[0]
    if G.shape != (n, n):
        raise ValueError(f"G must be [n, n], got {G.shape}")
    lib = _lib.load()
    return _blr_form_fill(lambda form: _lib.check(lib.tdgl_host_blr_form(n, p_f64(G), float(tol_abs), C.byref(form))))


class TDGLContext:
    """Owns one ``tdgl_ctx`` (device buffers + stream) for a mesh."""

    def __init__(self, mesh, fixed_sites=None, fix_psi=True, u=5.79, gamma=10.0, device_id=0,
                 reorder="rcm", n_owned=0, direct_solve=True, substructure_levels=None):
        """``n_owned`` > 0: one-process-per-GPU mode, ``mesh`` is a rank's sub-mesh from
        `partition.build_local_problem` (owned sites first, then ghosts; no reordering).
        ``direct_solve=False``: never use a direct mu solve (plain RCM site order, AMG-PCG whatever the
        mesh size; ``SolverOptions(sparse_solver="amg_pcg")``).
        ``substructure_levels`` 1 or 2: the site order of the substructured direct solve of that many levels
        whatever the mesh size and `DENSE_MAX_SITES` / `SUB_MAX_SITES` / `SUB2_MAX_SITES` say (part and
        super-block sizes as the size rule picks them; the factors: `build_substructure`)."""
        _lib.require_gpu()
        self._lib = _lib.load()
        self._ctx = C.c_void_p()
        # seconds spent in the set-up phases: "reorder" (RCM), "upload" (tdgl_create and every operator
        # upload), "amg_host" (aggregation, Galerkin products, collapsed / pre-multiplied operators)
        self.setup_times = {}
        em = mesh.edge_mesh
        self.n = len(mesh.sites)
        self.m = len(em.edges)
        self.n_boundary = len(em.boundary_edge_indices)
        self.n_probe = 0
        self.n_census = 0  # columns of a census row (2 + loops); 0: the census is off
        self.core_records = False  # set_core_records: `run` returns the cores of the recorded steps
        edges = i32(em.edges)
        self.n_owned = int(n_owned) if n_owned else self.n
        if n_owned:
            reorder = None
        self._sub_ptrs = []  # pointer arrays of the substructure site order, one per level (`build_substructure`)
        self._pd_order = None
        self.precond_direct = None
        self.direct_solve = bool(direct_solve)
        self.mu = self.mu_plan(self.n, n_owned, self.direct_solve, substructure_levels, reordered=reorder == "rcm")
        if reorder == "rcm":
            with _Stopwatch(self.setup_times, "reorder"):
                perm = rcm_permutation(em.edges, self.n)
                if self.mu.levels:
                    perm = self._dissection_order(mesh, em, perm)
        elif reorder is None or reorder == "none":
            perm = np.arange(self.n, dtype=np.int32)
        else:
            perm = i32(reorder)
        self.perm = perm
        self._n_eps_spots = 0  # hot spots in force (set_epsilon_spots)
        self.iperm = np.empty(self.n, dtype=np.int64)
        self.iperm[perm] = np.arange(self.n)
        fixed = i32([] if fixed_sites is None else fixed_sites)
        self._keep = dict(
            edges=edges, areas=f64(mesh.areas), el=f64(em.edge_lengths),
            dl=f64(em.dual_edge_lengths), dirs=f64(em.directions),
            bidx=i32(em.boundary_edge_indices), fixed=fixed, perm=perm,
        )
        k = self._keep
        desc = _lib.MeshDesc(
            n_sites=self.n, n_edges=self.m, n_boundary_edges=self.n_boundary,
            edges=p_i32(k["edges"]), areas=p_f64(k["areas"]), edge_lengths=p_f64(k["el"]),
            dual_edge_lengths=p_f64(k["dl"]), directions=p_f64(k["dirs"]),
            boundary_edge_indices=p_i32(k["bidx"]),
            fixed_sites=p_i32(fixed) if len(fixed) else None, n_fixed=len(fixed),
            fix_psi=int(bool(fix_psi)), site_perm=None if n_owned else p_i32(perm), u=float(u),
            gamma=float(gamma), n_owned=int(n_owned),
        )
        with _Stopwatch(self.setup_times, "upload"):
            _lib.check(self._lib.tdgl_create(C.byref(self._ctx), C.byref(desc), int(device_id)))
        self.hierarchy = None
        self.dense_direct = False  # mu solve = a direct one (set_dense_inverse / build_substructure)
        self.substructure = None

    def _dissection_order(self, mesh, em, perm):
        """Cuts the plan's dissection (`MuPlan.levels`, `MuPlan.blocks`), the sites of a part kept in the order of ``perm``
        (reverse Cuthill-McKee: the stencil's gathers stay local).  Form "sub": interiors part by part, then the
        separators level by level IS the context's site order -- sets `_sub_ptrs`, returns that permutation.  Form
        "precond": the context KEEPS ``perm`` (what the stencil kernels and the AMG hierarchy are fastest in); the factors
        become the CG's preconditioner and their order (`_pd_order`) lives inside its application."""
        from . import substructure

        rank = np.empty(self.n, dtype=np.int64)
        rank[perm] = np.arange(self.n)
        order = (substructure.substructure_order, substructure.substructure_order2, substructure.substructure_order3)[self.mu.levels - 1]
        cut = order(np.asarray(mesh.sites), em.edges, *self.mu.blocks, rank_hint=rank)
        if self.mu.form == "precond":
            self._pd_order = cut
            return perm
        self._sub_ptrs = list(cut[1:])
        return cut[0]

    # -- lifetime ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.tdgl_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, status):
        _lib.check(status, self._ctx)

    def synchronize(self):
        self._chk(self._lib.tdgl_synchronize(self._ctx))

    # -- Poisson set-up -------------------------------------------------------------------
    # meshes up to this many sites get the direct solve (one dense matrix-vector product per step,
    # `tdgl_poisson_set_dense_inverse`) unless build_poisson is told otherwise
    AMG_CANDIDATES = 3               # hierarchies built per iterative-regime mesh (the best one stays)
    AMG_CANDIDATES_MIN_SITES = 100_000
    DENSE_MAX_SITES = int(os.environ.get("TDGL_DENSE_MAX_SITES", "5000"))
    # ... and up to this many the substructured direct solve (`tdgl_poisson_set_substructure`): parts of
    # ~SUB_BLOCK sites with explicit inverses, a dense Schur complement on the separator
    SUB_MAX_SITES = int(os.environ.get("TDGL_SUB_MAX_SITES", "32000"))
    # (0 = by size: 192 sites per part up to 8k sites, 320 up to 60k, growing like n^(2/3) beyond -- the dense
    # Schur complement of the separator, ~2 n / sqrt(block) sites, is what grows fastest)
    SUB_BLOCK = int(os.environ.get("TDGL_SUB_BLOCK", "0"))
    # two levels of it (`tdgl_poisson_set_substructure_inner`) from there up to SUB2_MAX_SITES: parts of SUB2_BLOCK
    # sites inside super-blocks of SUB2_SUPER sites (0 = by size: 128 / 160 sites per part below / above 200k sites,
    # super-blocks of n / 60 sites but at least 2,048 -- the dense matrix of the top separator grows like n^2 /
    # SUB2_SUPER, the dense fine separators like n * SUB2_SUPER / SUB2_BLOCK).  Measured, steps/s with one level /
    # two levels: 23k sites 21.4k / 17.9k, 59k sites 9.4k / 14.2k, 120k sites 4.2k / 7.4k, 250k sites AMG-PCG 2.4k /
    # 3.9k (0.9 GB per solve there: G 232 MB, E 176, second level 234 + 164, top separator 224); the strip of 500k
    # sites stays iterative (1.8k against 3.8k steps/s in its stationary state, where the guess is exact).
    # (SUB_MAX_SITES = 0 switches both forms off)
    # Upper limit: the direct solve costs the same whatever the state, AMG-PCG as much as mu is unpredictable -- 350k
    # sites 3.0k against 2.0k steps/s, 450k 2.3k against 1.9k in an evolving vortex state; the 500k-site strip with terminals
    # in its STATIONARY state (an exact guess, 1.5 iterations) 1.8k against 3.8k -- which the time loop notices by itself
    # (`tdgl_direct_switching`); with three levels from 350k sites on: 600k sites 2.06k against 1.58k.
    # (round 6: from 400k sites the same factors in fp32 PRECONDITION the CG instead, `PD_MAX_SITES` below -- same-box
    # steps/s, direct solve / two-preconditioner CG, headline | vortex | 3,000-step stretch | late windows: 350k-site film 3,270 flat /
    # 2,912 | 2,777 | 3,554 | 4,655; 450k 2,620 flat / 2,647 | 2,712 | 3,378 | 2,655; 600k 2,068 flat / 2,137 | 2,231 | 2,607 |
    # 2,164; 501k-site strip 2,372 -> 4,714 once the loop has paused the direct solve / 3,655 -> 4,955 with no pause to wait
    # for and the context in reverse Cuthill-McKee order; 250k-site film 4,208 / 3,195: there the iterative step is
    # launch-bound and the direct solve in the run-ahead loop stays)
    SUB2_MAX_SITES = 400_000
    # from here on the separator right-hand sides of the way down come from the sparse coupling blocks (two more
    # launches, no -E^T rows: `tdgl_poisson_set_substructure_coupling`)
    # (measured: 60k sites 13.0k against 13.6k steps/s, 120k 7.5k / 8.1k, 160k 5.9k / 6.2k, 250k 4.1k / 3.9k)
    SUB2_SPARSE_SEP_MIN_SITES = 200_000
    # from here on a THIRD level (super-super-blocks of SUB3_BIG sites above the super-blocks, which then stay at 4,096
    # sites): the dense top separator of two levels is a third of the bytes there (240 of 758 MB per solve at 250k
    # sites; with three levels 29 + 23 + 22 MB)
    # (measured, steps/s with two / three levels: 250k sites 4.30k / 4.28k -- 766 against 609 MB per solve, three more
    # launches --, 450k sites 2.26k / 2.64k, 1.72 against 1.16 GB; 600k sites: 2.06k with three levels, AMG-PCG 1.58k)
    SUB3_MIN_SITES = 350_000
    SUB3_BIG = 32768
    # from here on the time loop may pause the direct solve in stationary states (`tdgl_direct_switching`): a 251k-site
    # strip with a transport current runs 7.1k steps/s on AMG-PCG (0 iterations) against 4.3k on the direct solve; below
    # ~150k sites the iterative step is launch-bound and the direct solve wins in every state
    DIRECT_SWITCH_MIN_SITES = 150_000
    SUB2_BLOCK = 0
    SUB2_SUPER = 0
    # above SUB2_MAX_SITES and up to here the three-level factors are built as well, stored in fp32, and PRECONDITION the
    # CG (`tdgl_poisson_set_substructure_precond`): at 1M sites the fp64 factors are 2.9 GB per solve -- 700 us, what
    # 7-8 AMG-preconditioned iterations cost --, in fp32 half of that buys 6.5 decades per application, i.e. ONE CG
    # iteration from the projection guess.  Per solve the library takes the V-cycle or the factors by predicted cost:
    # no state, no hysteresis -- a stationary strip runs on the V-cycle from its first step, a film in flux flow on the
    # factors, and the context keeps the reverse Cuthill-McKee order (16-bit column offsets in the stencil kernels).
    PD_MAX_SITES = int(os.environ.get("TDGL_PD_MAX_SITES", "1300000"))
    PD_CHOICE = 0  # 0: by predicted cost, 1: always the factors, 2: never (tests / A-B runs)
    # (part, super-block, super-super-block) sizes of the factors when they precondition: measured time of one application
    # at 1M sites with the final kernels (tools/exp_pd_blocks.py) 160/4096/32768 409 us, 128/4096/32768 407, 128/3072/24576 389,
    # 144/3072/24576 390 (and the shortest host set-up, 4.9 s), 112/3072/24576 398, 128/2048/16384 397, 128/3072/32768 390
    PD_BLOCKS = (144, 3072, 24576)

    @classmethod
    def mu_plan(cls, n, n_owned=0, direct_solve=True, substructure_levels=None, dense_max_sites=None, reordered=True) -> MuPlan:
        """The mu solver of a context on ``n`` sites (no GPU needed; the limits above are read from the class now).
        ``n_owned`` > 0 (one process per GPU) or ``reordered=False`` (the caller fixes the site order): no form that
        needs a site order or factors of its own -- and a rank that does not own every site solves iteratively.
        ``substructure_levels`` 1 or 2: the substructured solve of that many levels whatever the size rule says.
        ``dense_max_sites`` (`build_poisson` told its own dense limit): that limit instead of `DENSE_MAX_SITES`, and
        neither the substructured solve nor the preconditioner."""
        single = not n_owned or n_owned == n
        levels, precond = 0, False
        if reordered and not n_owned and dense_max_sites is None:
            if substructure_levels is not None:
                if substructure_levels not in (1, 2) or not direct_solve:
                    raise ValueError(f"substructure_levels must be 1 or 2 with a direct solve (got {substructure_levels})")
                levels = substructure_levels
            elif direct_solve and cls.SUB_MAX_SITES > 0:  # (SUB_MAX_SITES = 0 switches every form with factors off)
                if max(cls.SUB_MAX_SITES, cls.DENSE_MAX_SITES) < n <= cls.SUB2_MAX_SITES:
                    # beyond one level, up to SUB2_MAX_SITES, two levels (part interiors, the fine separators super-block
                    # by super-block, the top separator) -- and three from SUB3_MIN_SITES on: one more cut above, so
                    # that the dense top separator stays small
                    levels = 3 if n >= cls.SUB3_MIN_SITES else 2
                elif max(cls.SUB_MAX_SITES, cls.SUB2_MAX_SITES) < n <= cls.PD_MAX_SITES:
                    # larger still: three levels of dissection are cut all the same, their factors precondition the CG
                    levels, precond = 3, True
                elif cls.DENSE_MAX_SITES < n <= cls.SUB_MAX_SITES:
                    # mid-size meshes: one level ("interiors part by part, then the separator", substructure.py)
                    levels = 1
        if levels == 1:
            blocks = (cls.SUB_BLOCK or (192 if n <= 8000 else max(320, int(320 * (n / 60000.0) ** (2.0 / 3.0)))),)
        elif precond:
            blocks = (cls.SUB2_BLOCK or cls.PD_BLOCKS[0], cls.SUB2_SUPER or cls.PD_BLOCKS[1],
                      cls.PD_BLOCKS[2] if cls.SUB3_BIG == 32768 else cls.SUB3_BIG)
        elif levels:
            blocks = (cls.SUB2_BLOCK or (128 if n < 200_000 else 160),
                      *((cls.SUB2_SUPER or max(2048, n // 60),) if levels == 2 else (cls.SUB2_SUPER or 4096, cls.SUB3_BIG)))
        else:
            blocks = ()
        if levels:
            form = "precond" if precond else "sub"
        elif single and direct_solve and 2 <= n <= (cls.DENSE_MAX_SITES if dense_max_sites is None else int(dense_max_sites)):
            form = "dense"
        else:
            form = "amg"
        # (with the factors as second preconditioner the V-cycle only runs where the guess is good -- two or three
        # iterations per solve --, and 3 % fewer of those do not pay for two more hierarchies: 4.5 s of set-up at 1M sites)
        candidates = cls.AMG_CANDIDATES if (form == "amg" and single and n >= cls.AMG_CANDIDATES_MIN_SITES) else 1
        return MuPlan(form=form, levels=levels, blocks=blocks,
                      sparse_sep=levels == 3 or (levels == 2 and n >= cls.SUB2_SPARSE_SEP_MIN_SITES),
                      # large enough for the iterative solve to beat the direct one in a stationary state: let the loop choose
                      switching=form == "sub" and n >= cls.DIRECT_SWITCH_MIN_SITES, amg_candidates=candidates)

    def build_poisson(self, rtol=1e-10, max_iter=500, nu=2, check_every=0,
                      edge_currents_every_step=True, max_coarse=600, smoother="chebyshev",
                      cheb_lo=0.1, extrapolate=3, nu_fine=1, dense_max_sites=None, amg_candidates=None) -> Hierarchy:
        """AMG set-up on the host (the counterpart of the reference's LU factorisation,
        operators.py:305-308) + upload.  Single-GPU meshes of at most ``dense_max_sites`` sites
        (default `DENSE_MAX_SITES`; 0 = never) additionally get the explicit pseudo-inverse of the
        Poisson matrix and solve with it (`set_dense_inverse`).

        ``amg_candidates`` (default `AMG_CANDIDATES` from `AMG_CANDIDATES_MIN_SITES` = 100k sites on when the solve is iterative, else 1): the
        aggregation's priorities are hashed, and the hierarchies different seeds give differ by luck -- 0.286 to 0.308
        in the PCG's convergence factor at 1M sites, 7.50 to 7.79 iterations per step in the time loop, the one
        predicting the other (profiles/EXPERIMENTS.md).  So this many are built, each solves ONE fixed pseudo-random
        right-hand side on the device from a zero guess (20 ms), and the one with the smallest contraction per
        iteration stays (`setup_times["amg_candidates"]` lists the scores)."""
        k = self._keep
        with _Stopwatch(self.setup_times, "amg_host"):
            A = poisson_matrix(k["edges"].astype(np.int64), k["dl"] / k["el"], self.n, self.iperm)
        plan = self.mu if dense_max_sites is None else self.mu_plan(self.n, self.n_owned, self.direct_solve,
                                                                    dense_max_sites=dense_max_sites)
        if amg_candidates is None:
            amg_candidates = plan.amg_candidates
        if self.n_owned != self.n:
            amg_candidates = 1
        best, scores = None, []
        probe = None
        for c in range(max(1, int(amg_candidates))):
            with _Stopwatch(self.setup_times, "amg_host"):
                h = build_hierarchy(A, max_coarse=max_coarse, seed=c)
            self._shipped_plan = None
            self.set_hierarchy(h)
            self.set_poisson_options(rtol, max_iter, nu, check_every, edge_currents_every_step,
                                     smoother, cheb_lo, extrapolate, nu_fine)
            if amg_candidates <= 1:
                best = (0.0, c, h)
                break
            if probe is None:  # (the same for every candidate; zero mean: in the range of the operator)
                probe = np.random.default_rng(2024).standard_normal(self.n)
                probe -= probe.mean()
            with _Stopwatch(self.setup_times, "amg_probe"):
                _, its, relres = self.poisson_solve(probe / k["areas"])  # (the library solves A mu = -a * rhs: b = -probe)
            score = float(relres) ** (1.0 / max(int(its), 1)) if relres > 0 else 0.0
            scores.append(dict(seed=c, iterations=int(its), relres=float(relres), contraction=round(score, 4), sizes=h.sizes))
            if best is None or score < best[0]:
                best = (score, c, h)
        if amg_candidates > 1:
            self.setup_times["amg_candidates"] = scores
            if best[1] != scores[-1]["seed"]:  # the last one built is on the device: put the best one back
                self._shipped_plan = None
                self.set_hierarchy(best[2])
                self.set_poisson_options(rtol, max_iter, nu, check_every, edge_currents_every_step,
                                         smoother, cheb_lo, extrapolate, nu_fine)
        h = best[2]
        # (the factors are held to the tighter of 1e-11 and the iterative solve's tolerance)
        check = min(1e-11, float(rtol))
        if plan.form == "sub":
            self.build_substructure(A, check_rtol=check)
        elif plan.form == "precond":
            self.build_precond_direct(rtol=float(rtol))
        elif plan.form == "dense":
            self.build_dense_inverse(A, check_rtol=check)
        return h

    def _direct_solve_passes(self, check_rtol) -> bool:
        """Residual check of a freshly built direct solve on a white-noise right-hand side.  (A generic smooth one,
        L_mu applied to cos(pi x / Lx) cos(pi y / Ly), was tried as a second check in round 4: the factors of the 600 : 1
        graded mesh pass it at 1e-9 although they leave 2e-6 .. 6e-6 on the right-hand sides the time loop actually
        produces there -- only measuring THOSE catches it, which is what the in-loop guard does, `direct_stats`.)"""
        b = np.random.default_rng(0).standard_normal(self.n)
        _, _, relres = self.poisson_solve(b)
        return bool(relres <= check_rtol)

    def build_substructure(self, A=None, check_rtol=1e-11) -> bool:
        """Switch the mu solve to the substructured direct solve (`tdgl_poisson_set_substructure`); the
        context must have been created with the substructure site order (mid-size meshes are).  Checked on a
        random right-hand side like `build_dense_inverse`; returns whether it is on."""
        from . import substructure  # (its functions are looked up when called: tests replace `pack_for_device` there)

        if not self._sub_ptrs:
            raise ValueError("this context's site order is not a substructure order")
        if A is None:
            k = self._keep
            A = poisson_matrix(k["edges"].astype(np.int64), k["dl"] / k["el"], self.n, self.iperm)
        sec = C.c_double(0.0)
        if len(self._sub_ptrs) > 1:
            # two or three levels: the factors are formed on the host, the top separator's pseudo-inverse on the device
            sparse_sep = self.mu.sparse_sep
            with _Stopwatch(self.setup_times, "substructure_host"):
                try:
                    levels = substructure.build_substructure_levels(A, self._sub_ptrs)
                    packed = [substructure.pack_for_device(lv, sparse_sep) for lv in levels]
                except (ValueError, IndexError, np.linalg.LinAlgError) as exc:
                    # (a mesh the dissection cannot cut as it expects -- a super-block without interior, pieces that are
                    # not connected: the iterative solve takes it)
                    self.setup_times["substructure_error"] = repr(exc)
                    return False
            status, t_dev = self._upload_levels(levels, packed, sparse_sep)
            tiles = [0, 0, 0]
            if status == _lib.TDGL_OK:
                status, tiles = self._compact_direct_factors()
            sec = C.c_double(t_dev)
            info = dict(levels=len(levels), sparse_separator_rhs=sparse_sep, **_level_counts(levels), built_on="host",
                        symmetric_tiles=[bool(t) for t in tiles[:len(levels)]], bytes_per_solve=_factor_bytes(levels, tiles, sparse_sep))
            del levels, packed
        elif not os.environ.get("TDGL_SUB_HOST"):
            # the factors are formed on the device; the host only describes the structure
            with _Stopwatch(self.setup_times, "substructure_host"):
                try:
                    pl = substructure.plan_for_device(A, self._sub_ptrs[0])
                except ValueError:
                    return False
            p_i64 = lambda a: a.ctypes.data_as(_lib.c_i64p)
            d = _lib.SubstructurePlan(
                n_interior=pl["n_interior"], n_sep=pl["n_sep"], n_parts=pl["n_parts"], part_ptr=p_i32(pl["part_ptr"]),
                sep_ptr=p_i32(pl["sep_ptr"]), sep_idx=p_i32(pl["sep_idx"]), ent_ptr=p_i32(pl["ent_ptr"]), ent_row=p_i32(pl["ent_row"]),
                ent_val=p_f64(pl["ent_val"]), node_ptr=p_i32(pl["node_ptr"]), node_pair=p_i32(pl["node_pair"]),
                ass_indptr=p_i32(pl["ass_indptr"]), ass_indices=p_i32(pl["ass_indices"]), ass_data=p_f64(pl["ass_data"]),
                seg_ptr=p_i32(pl["seg_ptr"]), seg_val=p_i64(pl["seg_val"]), seg_x=p_i32(pl["seg_x"]), seg_len=p_i32(pl["seg_len"]),
                g_off=p_i64(pl["g_off"]), et_off=p_i64(pl["et_off"]), gvec_off=pl["gvec_off"], n_vals=pl["n_vals"],
                e_off=p_i64(pl["e_off"]), n_e=pl["n_e"],
            )
            status = self._lib.tdgl_poisson_build_substructure(self._ctx, C.byref(d), C.byref(sec))
            info = dict(parts=pl["parts"], separator=pl["separator"], bytes_per_solve=pl["bytes_per_solve"], built_on="device")
        else:
            with _Stopwatch(self.setup_times, "substructure_host"):
                try:
                    sub = substructure.build_substructure(A, self._sub_ptrs[0])
                except (ValueError, np.linalg.LinAlgError):
                    return False
                pk = substructure.pack_for_device(sub)
            status = self._lib.tdgl_poisson_set_substructure(self._ctx, C.byref(_lib.describe(pk)), C.byref(sec))
            info = dict(parts=sub.n_parts, separator=sub.n_sep, bytes_per_solve=_factor_bytes([sub], [0], sparse_sep=False), built_on="host")
        if status != _lib.TDGL_OK:
            self._note_library_error()
            return False
        self.setup_times["substructure_device"] = sec.value
        if not self._direct_solve_passes(check_rtol):
            self.set_dense_inverse(None)  # (also releases the substructure factors: back to AMG-PCG)
            return False
        self.substructure = info
        self.dense_direct = True
        if self.mu.switching:
            self.direct_switching(True)
        return True

    # the direct solve's levels of many small parts keep their symmetric G blocks as tiles on or below the diagonal
    # (`tdgl_poisson_set_substructure_layout`; False: whole blocks, the form of the earlier rounds)
    SUB_SYM_TILES = True

    def _compact_direct_factors(self):
        """After every level of a host-built direct solve has been uploaded: `(status, rows staged per level or 0)`."""
        status = self._lib.tdgl_poisson_set_substructure_layout(self._ctx, int(bool(self.SUB_SYM_TILES)))
        return status, (self.precond_direct_layout() if status == _lib.TDGL_OK else [0, 0, 0])

    def _note_library_error(self):
        """A refused upload: the library's message goes into ``setup_times["substructure_error"]``."""
        err = self._lib.tdgl_last_error(self._ctx)
        self.setup_times["substructure_error"] = err.decode() if isinstance(err, bytes) else str(err)

    def _upload_levels(self, levels, packed, sparse_sep=True):
        """The factors of a multi-level dissection (`substructure.build_substructure_levels`, `pack_for_device`) into the
        library: first level, inner levels, and with ``sparse_sep`` every level's sparse coupling block.  Returns
        (status, device seconds)."""
        sec = C.c_double(0.0)
        t_dev, status = 0.0, _lib.TDGL_OK
        for k, pk in enumerate(packed):
            call = self._lib.tdgl_poisson_set_substructure if k == 0 else self._lib.tdgl_poisson_set_substructure_inner
            status = call(self._ctx, C.byref(_lib.describe(pk)), C.byref(sec))
            t_dev += sec.value
            if status != _lib.TDGL_OK:
                return status, t_dev
        for k, lv in enumerate(levels if sparse_sep else ()):
            M = lv.coupling
            keep_c = (i32(M.indptr), i32(M.indices), f64(M.data))
            status = self._lib.tdgl_poisson_set_substructure_coupling(self._ctx, k, p_i32(keep_c[0]), p_i32(keep_c[1]), p_f64(keep_c[2]))
            if status != _lib.TDGL_OK:
                break
        return status, t_dev

    def build_precond_direct(self, rtol=1e-10) -> bool:
        """Three levels of nested dissection as the CG's PRECONDITIONER (`tdgl_poisson_set_substructure_precond`; the
        counterpart of the reference's LU, operators.py:305-308, above `SUB2_MAX_SITES`): factors formed on the host in
        the dissection's order (`_pd_order`), stored in fp32 on the device; the first level's two kernels read the
        residual and write the result through the dissection's map, so that the context keeps its reverse
        Cuthill-McKee order.  Checked on a white-noise right-hand side from a zero guess
        (the CG must get to ``rtol`` in at most three applications); returns whether it is on."""
        from . import substructure

        perm_d, p1, p2, p3 = self._pd_order
        k = self._keep
        iperm_d = np.empty(self.n, dtype=np.int64)
        iperm_d[perm_d] = np.arange(self.n)
        with _Stopwatch(self.setup_times, "substructure_host"):
            try:
                A_d = poisson_matrix(k["edges"].astype(np.int64), k["dl"] / k["el"], self.n, iperm_d)
                levels = substructure.build_substructure_levels(A_d, [p1, p2, p3])
                packed = [substructure.pack_for_device(lv, True) for lv in levels]
            except (ValueError, IndexError, np.linalg.LinAlgError) as exc:
                self.setup_times["substructure_error"] = repr(exc)
                return False
        status, t_dev = self._upload_levels(levels, packed)
        ta, tv = C.c_double(0.0), C.c_double(0.0)
        if status == _lib.TDGL_OK:
            keep_map = i32(perm_d)
            status = self._lib.tdgl_poisson_set_substructure_precond(self._ctx, p_i32(keep_map), 1, C.byref(ta), C.byref(tv))
        if status != _lib.TDGL_OK:
            self._note_library_error()
            self._chk(self._lib.tdgl_poisson_set_substructure(self._ctx, None, None))
            return False
        self.setup_times["substructure_device"] = t_dev
        tiles = self.precond_direct_layout()  # per level: G blocks as 16 x 16 tiles on or below the diagonal?
        # (the permutation: r read and z written through the map, 12 bytes per site each; as separate gather and scatter
        # kernels -- TDGL_PD_TWO_PASS -- 20 each: the vector once more in the dissection's order)
        perm_bytes = 20 if self.precond_apply_stats()["two_pass"] else 12
        info = dict(levels=3, storage="fp32", symmetric_tiles=[bool(t) for t in tiles], **_level_counts(levels),
                    bytes_per_application=_factor_bytes(levels, tiles, word=4) + 2 * perm_bytes * self.n,
                    t_apply_us=round(ta.value, 1), t_vcycle_us=round(tv.value, 1))
        blr = self.precond_direct_blr()
        if blr["on"]:  # (the top separator's tiles replaced by the block low-rank form)
            info["bytes_per_application"] += blr["bytes"] - 4 * _sym_tile_entries(levels[2].n_sep)
            info["top_separator_blr"] = blr
        del levels, packed
        # the check: with the factors forced, a white-noise right-hand side from a zero guess
        self._chk(self._lib.tdgl_poisson_precond_choice(self._ctx, 1))
        b = np.random.default_rng(0).standard_normal(self.n)
        _, its, relres = self.poisson_solve(b)
        self._chk(self._lib.tdgl_poisson_precond_choice(self._ctx, int(self.PD_CHOICE)))
        info.update(check_iterations=int(its), check_relres=float(relres))
        if not (relres <= rtol and its <= 3):
            self._chk(self._lib.tdgl_poisson_set_substructure(self._ctx, None, None))
            self.setup_times["substructure_error"] = f"preconditioner check: {its} iterations, relres {relres:.2e}"
            return False
        self.precond_direct = info
        self.precond_direct_stats(reset=True)
        return True

    def build_schur_precond(self, piece, allreduce_sum, allreduce_max, choice=None, fp32_storage=True) -> bool:
        """One-process-per-GPU mode: this rank's share of the RANK-LEVEL nested dissection (`schur_dd.SchurPiece`) as the
        CG's second preconditioner (`tdgl_poisson_schur_begin` ... `_finish`).  ``allreduce_sum(array) -> array`` /
        ``allreduce_max(array) -> array`` over the bootstrap group: the interface complement is summed ONCE, the measured
        times of the two preconditioners are agreed on (so that every rank takes the same choice in every solve).  Every
        rank calls this at the same point; returns whether the preconditioner is on (the same answer on every rank).
        ``fp32_storage=False`` keeps the local factors and the interface's pseudo-inverse in fp64 (tests)."""
        from . import substructure

        ok = 1.0
        levels = packed = None
        with _Stopwatch(self.setup_times, "substructure_host"):
            try:
                levels = substructure.build_substructure_levels(piece.A_II, piece.ptrs, gauge=False)
                packed = [substructure.pack_for_device(lv, True) for lv in levels]
            except (ValueError, IndexError, np.linalg.LinAlgError) as exc:
                self.setup_times["substructure_error"] = repr(exc)
                ok = 0.0
        if float(allreduce_max(np.array([1.0 - ok]))[0]) > 0.0:  # (some rank could not cut its interior: nobody uses it)
            return False
        keep = dict(interior=i32(piece.interior), gl=i32(piece.gamma_owned_local), gg=i32(piece.gamma_owned_gid),
                    gi=(i32(piece.A_GI.indptr), i32(piece.A_GI.indices), f64(piece.A_GI.data)),
                    ig=(i32(piece.A_IG.indptr), i32(piece.A_IG.indices), f64(piece.A_IG.data)))
        desc = _lib.SchurPiece(
            n_interior=piece.n_interior, n_gamma=piece.n_gamma, n_gamma_owned=len(keep["gl"]), interior=p_i32(keep["interior"]),
            gamma_owned_local=p_i32(keep["gl"]) if len(keep["gl"]) else None, gamma_owned_gid=p_i32(keep["gg"]) if len(keep["gg"]) else None,
            gi_indptr=p_i32(keep["gi"][0]), gi_indices=p_i32(keep["gi"][1]), gi_data=p_f64(keep["gi"][2]),
            ig_indptr=p_i32(keep["ig"][0]), ig_indices=p_i32(keep["ig"][1]), ig_data=p_f64(keep["ig"][2]))
        status = self._lib.tdgl_poisson_schur_begin(self._ctx, C.byref(desc))
        t_dev = 0.0
        if status == _lib.TDGL_OK:
            status, t_dev = self._upload_levels(levels, packed)
        ng = int(piece.n_gamma)
        S = np.zeros((ng, ng))
        if status == _lib.TDGL_OK:
            Cmat = np.zeros((ng, ng))
            status = self._lib.tdgl_poisson_schur_complement(self._ctx, p_f64(Cmat))
            S = piece.A_GG_owned.toarray() - Cmat
        failed = float(allreduce_max(np.array([0.0 if status == _lib.TDGL_OK else 1.0]))[0]) > 0.0
        if failed:
            if status != _lib.TDGL_OK:
                self._note_library_error()
            self._chk(self._lib.tdgl_poisson_set_substructure(self._ctx, None, None))
            return False
        with _Stopwatch(self.setup_times, "schur_sum"):
            S = np.ascontiguousarray(allreduce_sum(S))
        ta, tv = C.c_double(0.0), C.c_double(0.0)
        self._chk(self._lib.tdgl_poisson_schur_finish(self._ctx, p_f64(S), int(bool(fp32_storage)), C.byref(ta), C.byref(tv)))
        times = allreduce_max(np.array([ta.value, tv.value]))
        self._chk(self._lib.tdgl_poisson_set_precond_times(self._ctx, float(times[0]), float(times[1])))
        self._chk(self._lib.tdgl_poisson_precond_choice(self._ctx, int(self.PD_CHOICE if choice is None else choice)))
        self.setup_times["substructure_device"] = t_dev
        tiles = self.precond_direct_layout()
        word = 4 if fp32_storage else 8
        self.precond_direct = dict(
            kind="rank-level nested dissection", levels=len(levels), storage="fp32" if fp32_storage else "fp64", symmetric_tiles=[bool(t) for t in tiles[:len(levels)]], interior=int(piece.n_interior), interface=ng,
            interface_owned=int(len(keep["gl"])), parts=levels[0].n_parts, separator=levels[0].n_sep,
            bytes_per_application=int(2 * _factor_bytes(levels, tiles, word=word, top=False) + word * ng * ng // 2
                                      + 12 * (piece.A_GI.nnz + piece.A_IG.nnz)),
            allreduce_doubles_per_application=ng, t_apply_us=round(float(times[0]), 1), t_vcycle_us=round(float(times[1]), 1))
        self.precond_direct_stats(reset=True)
        return True

    def precond_direct_stats(self, reset=False):
        """`tdgl_get_precond_direct_stats`: solves / CG iterations by preconditioner since the last reset, the measured
        time per application of either, the decades per application observed with the factors."""
        o4, o3 = (C.c_int64 * 4)(), (C.c_double * 4)()
        self._chk(self._lib.tdgl_get_precond_direct_stats(self._ctx, o4, o3, int(bool(reset))))
        return dict(solves_factors=int(o4[0]), iterations_factors=int(o4[1]), solves_vcycle=int(o4[2]), iterations_vcycle=int(o4[3]),
                    handovers=int(o3[3]), t_apply_us=round(o3[0], 1), t_vcycle_us=round(o3[1], 1), decades_per_application=round(o3[2], 2))

    def precond_direct_blr(self):
        """`tdgl_get_precond_direct_blr`: the top separator of the fp32 factors in block low-rank form -- whether it is,
        tile pairs stored as factors, tiles kept dense, the largest rank, bytes per application (and with dense tiles),
        the truncation tau and the ||G||_2 it is relative to."""
        o6, o2 = (C.c_int64 * 6)(), (C.c_double * 2)()
        self._chk(self._lib.tdgl_get_precond_direct_blr(self._ctx, o6, o2))
        return dict(on=bool(o6[0]), pairs=int(o6[1]), dense_tiles=int(o6[2]), rank_max=int(o6[3]), bytes=int(o6[4]),
                    dense_bytes=int(o6[5]), tau=float(o2[0]), norm=float(o2[1]))

    def precond_direct_layout(self):
        """Per level of the fp32-stored factors: the rows of a part its way down stages when the level keeps only the
        tiles on or below the diagonal of its G blocks (`tdgl_get_precond_direct_layout`), 0 for whole blocks."""
        out = (C.c_int32 * 3)()
        self._chk(self._lib.tdgl_get_precond_direct_layout(self._ctx, out))
        return [int(v) for v in out]

    def precond_choice(self, mode: int):
        """0: the library chooses per solve by predicted cost, 1: always the factors, 2: always the AMG V-cycle."""
        self._chk(self._lib.tdgl_poisson_precond_choice(self._ctx, int(mode)))

    def direct_switching(self, on=None):
        """`tdgl_direct_switching`: let the time loop pause the direct mu solve while the state is stationary (AMG-PCG
        from the projection guess is then the cheaper solve) -- ``on`` True / False sets it, None only queries.
        Returns ``dict(switches, paused)``."""
        sw, pa = C.c_int64(0), C.c_int32(0)
        self._chk(self._lib.tdgl_direct_switching(self._ctx, -1 if on is None else int(bool(on)), C.byref(sw), C.byref(pa)))
        return dict(switches=int(sw.value), paused=bool(pa.value))

    def build_dense_inverse(self, A=None, check_rtol=1e-11) -> bool:
        """Switch the mu solve to the explicit pseudo-inverse (`tdgl_poisson_set_dense_inverse`): built on
        the device (`tdgl_poisson_build_dense_inverse`: a blocked symmetric sweep, `csrc/dense.inc`), or on the
        host with LAPACK when ``TDGL_DENSE_HOST`` is set.  The result is checked on a random right-hand side (``||b - A G b|| <= check_rtol ||b||``,
        the residual the library reports for a one-off solve); a matrix that fails, or whose
        factorisation breaks down (a mesh in several pieces), stays with AMG-PCG.  Returns whether the
        direct solve is on."""
        ok = False
        if not os.environ.get("TDGL_DENSE_HOST"):
            sec = C.c_double(0.0)
            status = self._lib.tdgl_poisson_build_dense_inverse(self._ctx, C.byref(sec))
            if status == _lib.TDGL_OK:
                self.setup_times["dense_inverse_device"] = sec.value
                ok = True
            elif status != _lib.TDGL_ERR_NOT_READY:
                return False  # (not positive definite on the complement of the constants)
        if not ok:
            from .amg import dense_pseudo_inverse

            if A is None:
                k = self._keep
                A = poisson_matrix(k["edges"].astype(np.int64), k["dl"] / k["el"], self.n, self.iperm)
            with _Stopwatch(self.setup_times, "dense_inverse_host"):
                G = dense_pseudo_inverse(A, check_rtol=check_rtol)
            if G is None:
                return False
            self.set_dense_inverse(G)
        if not self._direct_solve_passes(check_rtol):
            self.set_dense_inverse(None)
            return False
        self.dense_direct = True
        return True

    def set_dense_inverse(self, G):
        """Solve the mu equation as ``mu = G b`` from now on (``G`` = pinv of the level-0 Poisson
        matrix, dense [n, n], internal site order); ``None`` returns to AMG-PCG."""
        if G is None:
            self._chk(self._lib.tdgl_poisson_set_dense_inverse(self._ctx, None, 0))
            self.dense_direct = False
            self.substructure = None
            return
        G = f64(G)
        if G.shape != (self.n, self.n):
            raise ValueError(f"dense inverse must be [{self.n}, {self.n}], got {G.shape}")
        with _Stopwatch(self.setup_times, "upload"):
            self._chk(self._lib.tdgl_poisson_set_dense_inverse(self._ctx, p_f64(G), self.n))
        self.dense_direct = True

    # -- one process per GPU -------------------------------------------------------------
    def set_halo_plan(self, lp):
        """Register the halo plan of `partition.LocalProblem` ``lp``."""
        nbrs = i32(lp.neighbors)
        send_ptr = i32(np.concatenate([[0], np.cumsum([len(lp.send_idx[nb]) for nb in lp.neighbors])]))
        send_idx = i32(np.concatenate([lp.send_idx[nb] for nb in lp.neighbors]) if lp.neighbors else [])
        recv_ptr = i32([0] + [lp.recv_range[nb][1] - lp.n_own for nb in lp.neighbors])
        for k, nb in enumerate(lp.neighbors):  # ghost ranges are contiguous and in neighbour order
            assert lp.recv_range[nb][0] - lp.n_own == recv_ptr[k]
        self._halo_keep = (nbrs, send_ptr, send_idx, recv_ptr)
        plan = _lib.HaloPlan(
            rank=lp.rank, world=lp.world, n_global=lp.n_global, n_neighbors=len(nbrs),
            neighbor_ranks=p_i32(nbrs) if len(nbrs) else None, send_ptr=p_i32(send_ptr),
            send_idx=p_i32(send_idx) if len(send_idx) else None, recv_ptr=p_i32(recv_ptr),
        )
        self._chk(self._lib.tdgl_set_halo_plan(self._ctx, C.byref(plan)))

    def set_deep_halo_plan(self, dp):
        """Register the exchange of the PCG residual on the whole ghost zone of `partition.DeepPlan` ``dp``
        (`tdgl_set_deep_halo_plan`; after `set_halo_plan`, before `set_hierarchy_deep`)."""
        nbrs = sorted(set(dp.neighbors) | set(dp.send_idx))
        empty = np.empty(0, dtype=np.int64)
        send = [np.asarray(dp.send_idx.get(nb, empty)) for nb in nbrs]
        recv = [np.asarray(dp.recv_idx.get(nb, empty)) for nb in nbrs]
        a = (i32(nbrs), i32(np.concatenate([[0], np.cumsum([len(x) for x in send])])),
             i32(np.concatenate(send) if send else []), i32(np.concatenate([[0], np.cumsum([len(x) for x in recv])])),
             i32(np.concatenate(recv) if recv else []))
        self._deep_keep = a
        plan = _lib.DeepHaloPlan(
            n_ext=int(dp.n_ext), n_neighbors=len(nbrs), neighbor_ranks=p_i32(a[0]) if len(nbrs) else None,
            send_ptr=p_i32(a[1]), send_idx=p_i32(a[2]) if len(a[2]) else None, recv_ptr=p_i32(a[3]),
            recv_idx=p_i32(a[4]) if len(a[4]) else None, l1_interior=int(getattr(dp, "l1_interior", 0)))
        self._chk(self._lib.tdgl_set_deep_halo_plan(self._ctx, C.byref(plan)))
        self.deep_plan = dp

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _lib.check(_lib.load().tdgl_comm_unique_id(buf))
        return buf.raw

    def comm_init_rccl(self, unique_id: bytes):
        assert len(unique_id) == 128
        self._chk(self._lib.tdgl_comm_init_rccl(self._ctx, C.c_char_p(unique_id)))

    def comm_ipc_export(self, world: int):
        """``(handle: 64 bytes, table: int64[4 + 6 world])`` of this rank's inbox (`tdgl_comm_ipc_export`)."""
        handle = C.create_string_buffer(64)
        table = np.zeros(4 + 6 * int(world), dtype=np.int64)
        self._chk(self._lib.tdgl_comm_ipc_export(self._ctx, handle, table.ctypes.data_as(_lib.c_i64p), len(table)))
        return handle.raw, table

    def comm_init_ipc(self, handles, tables):
        """``handles``: the ranks' 64-byte handles in rank order, ``tables``: their tables (`tdgl_comm_init_ipc`)."""
        blob = b"".join(handles)
        tab = np.ascontiguousarray(np.stack(tables), dtype=np.int64)
        self._chk(self._lib.tdgl_comm_init_ipc(self._ctx, C.c_char_p(blob), tab.ctypes.data_as(_lib.c_i64p)))

    def comm_ipc_set_timeout(self, seconds: float):
        """Bound of the in-kernel waits of the peer-mapped transport (`tdgl_comm_ipc_set_timeout`; default 120 s, or
        ``TDGL_IPC_TIMEOUT_S``)."""
        self._chk(self._lib.tdgl_comm_ipc_set_timeout(self._ctx, float(seconds)))

    def comm_test_halo(self, vec, width=1, deep=False):
        """One exchange of ``vec``'s ghost entries through the context's transport (`tdgl_comm_test_halo`)."""
        v = np.ascontiguousarray(vec, dtype=np.float64).copy()
        self._chk(self._lib.tdgl_comm_test_halo(self._ctx, p_f64(v), int(width), int(bool(deep))))
        return v

    def comm_test_allreduce(self, buf, op="sum", as_f32=False):
        v = np.ascontiguousarray(buf, dtype=np.float64).copy()
        self._chk(self._lib.tdgl_comm_test_allreduce(self._ctx, p_f64(v), v.size, 0 if op == "sum" else 1, int(bool(as_f32))))
        return v

    def comm_init_callbacks(self, halo, allreduce):
        """``halo(send, send_off, recv, recv_off, ranks)`` and ``allreduce(buf, op)`` operate on
        NumPy views of the library's pinned host buffers (test transport)."""

        def _halo(user, send, send_off, recv, recv_off, nn, ranks):
            try:
                so = np.ctypeslib.as_array(send_off, shape=(nn + 1,))
                ro = np.ctypeslib.as_array(recv_off, shape=(nn + 1,))
                rk = np.ctypeslib.as_array(ranks, shape=(nn,))
                halo(np.ctypeslib.as_array(send, shape=(int(so[-1]),)), so,
                     np.ctypeslib.as_array(recv, shape=(int(ro[-1]),)), ro, rk)
                return 0
            except Exception:  # pragma: no cover
                import traceback

                traceback.print_exc()
                return 1

        def _allreduce(user, buf, count, op):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(int(count),)), int(op))
                return 0
            except Exception:  # pragma: no cover
                import traceback

                traceback.print_exc()
                return 1

        self._cb_keep = (_lib.HALO_FN(_halo), _lib.ALLREDUCE_FN(_allreduce))
        self._chk(self._lib.tdgl_comm_init_callbacks(self._ctx, self._cb_keep[0], self._cb_keep[1], None))

    def set_comm_overlap(self, mode="auto"):
        """Overlap halo exchanges with the ghost-free rows on a second HIP stream: ``"auto"``
        (default; only for partitions big enough to pay for the cross-stream dependencies),
        ``True`` / ``"always"``, ``False`` / ``"never"``."""
        code = {"auto": 1, "always": 2, "never": 0, True: 2, False: 0}[mode]
        self._chk(self._lib.tdgl_set_comm_overlap(self._ctx, code))

    def comm_stats(self, reset=False):
        """``dict(halos, halo_bytes, allreduces, allreduce_bytes)`` of this rank since the last reset."""
        out = (C.c_int64 * 4)()
        self._chk(self._lib.tdgl_get_comm_stats(self._ctx, out, int(bool(reset))))
        return dict(halos=out[0], halo_bytes=out[1], allreduces=out[2], allreduce_bytes=out[3])

    def comm_overlap(self):
        on, rows = C.c_int32(0), C.c_int64(0)
        self._chk(self._lib.tdgl_get_comm_overlap(self._ctx, C.byref(on), C.byref(rows)))
        return bool(on.value), rows.value

    def set_hierarchy_distributed(self, h: Hierarchy, lp):
        """Upload the GLOBAL hierarchy ``h`` with level 0 sliced for this rank
        (`partition.local_hierarchy_level0`) and the coarser levels replicated."""
        from .amg import Level
        from .partition import local_hierarchy_level0

        loc = local_hierarchy_level0(h, lp)
        lv0 = Level(A=loc["A"], dinv=loc["dinv"], rho=loc["rho"], P=loc["P"], R=loc["R"])
        hh = Hierarchy(levels=[lv0] + list(h.levels[1:]), coarse_pinv=h.coarse_pinv)
        self._local_level0 = lv0
        self._shipped_plan = None
        self.set_hierarchy(hh, n_cols0=lp.n_loc)
        self.hierarchy = h

    def set_hierarchy_sliced(self, level0: dict, coarse: dict, lp):
        """Upload a hierarchy given as this rank's level-0 slice (`partition.local_hierarchy_level0`)
        plus the replicated coarser levels (``dict(levels=[...], coarse_pinv=...)``): what
        `distributed.prepare_payloads` ships to a rank."""
        from .amg import Level

        lv0 = Level(A=level0["A"], dinv=level0["dinv"], rho=level0["rho"], P=level0["P"], R=level0["R"])
        hh = Hierarchy(levels=[lv0] + list(coarse["levels"]), coarse_pinv=coarse["coarse_pinv"])
        self._local_level0 = lv0
        self._shipped_plan = (coarse.get("plan_key"), coarse.get("plan")) if "plan" in coarse else None
        self.set_hierarchy(hh, n_cols0=lp.n_loc)
        self.hierarchy = _HierarchyInfo(hh, coarse.get("sizes"), coarse.get("operator_complexity"))

    def set_hierarchy_deep(self, dp, coarse: dict):
        """Two distributed AMG levels (`partition.DeepPlan` ``dp``: this rank's slices of level 0 and of the explicit
        operators of level 1) on top of the replicated levels >= 2 (``coarse``: ``levels`` = the global hierarchy's
        levels from 2 on, ``coarse_pinv``, ``plan`` = its collapsed chain)."""
        from .amg import Level

        lv0 = Level(A=dp.A, dinv=dp.dinv, rho=dp.rho, P=dp.P, R=None)
        stub = Level(A=None, dinv=None, rho=float(coarse["rho1"]))
        hh = Hierarchy(levels=[lv0, stub] + list(coarse["levels"]), coarse_pinv=coarse["coarse_pinv"])
        levels = (_lib.AmgLevel * len(hh.levels))()
        keep = []
        for idx, lv in enumerate(hh.levels):
            L = levels[idx]
            L.rho = float(lv.rho)
            if idx == 1:
                L.n, L.n_cols, L.explicit_only, L.n_coarse = int(dp.l1_x), int(dp.l1_loc), 1, int(dp.M.shape[0])
                continue
            A = lv.A.tocsr()
            arrs = dict(Ap=i32(A.indptr), Ai=i32(A.indices), Ad=f64(A.data), dinv=f64(lv.dinv))
            L.A_indptr, L.A_indices, L.A_data, L.dinv = p_i32(arrs["Ap"]), p_i32(arrs["Ai"]), p_f64(arrs["Ad"]), p_f64(arrs["dinv"])
            if idx == 0:
                L.n, L.n_cols, L.a_rows, L.p_rows = int(dp.n_own), int(dp.n_ext), int(dp.n1), int(dp.n2)
                P = lv.P.tocsr()
                arrs.update(Pp=i32(P.indptr), Pi=i32(P.indices), Pd=f64(P.data))
                L.n_coarse = int(dp.l1_x)
                L.P_indptr, L.P_indices, L.P_data = p_i32(arrs["Pp"]), p_i32(arrs["Pi"]), p_f64(arrs["Pd"])
            else:
                L.n = A.shape[0]
                if lv.P is not None:
                    P, R = lv.P.tocsr(), lv.R.tocsr()
                    arrs.update(Pp=i32(P.indptr), Pi=i32(P.indices), Pd=f64(P.data),
                                Rp=i32(R.indptr), Ri=i32(R.indices), Rd=f64(R.data))
                    L.n_coarse = P.shape[1]
                    L.P_indptr, L.P_indices, L.P_data = p_i32(arrs["Pp"]), p_i32(arrs["Pi"]), p_f64(arrs["Pd"])
                    L.R_indptr, L.R_indices, L.R_data = p_i32(arrs["Rp"]), p_i32(arrs["Ri"]), p_f64(arrs["Rd"])
            keep.append(arrs)
        pinv = f64(hh.coarse_pinv)
        with _Stopwatch(self.setup_times, "upload"):
            self._chk(self._lib.tdgl_poisson_set_hierarchy(self._ctx, levels, len(hh.levels), p_f64(pinv)))
        self._local_level0 = None
        self._deep = dp
        # the plan of the collapsed chain with this rank's slices in the place of level 1
        plan = dict(coarse["plan"])
        plan["mid"] = dict(plan["mid"]); plan["up"] = dict(plan["up"])
        plan["mid"][1] = dp.M
        plan["up"][1] = (dp.W, dp.V)
        self._shipped_plan = (coarse.get("plan_key"), plan)
        self.hierarchy = _HierarchyInfo(hh, coarse.get("sizes"), coarse.get("operator_complexity"))
        self.hierarchy.levels = hh.levels
        self.dense_direct = False
        self.substructure = None
        self._hier_epoch = getattr(self, "_hier_epoch", 0) + 1
        self._refresh_fused_restriction()
        self._set_fused_levels(hh)
        self._refresh_collapsed()

    def set_hierarchy(self, h: Hierarchy, n_cols0: int = 0):
        levels = (_lib.AmgLevel * len(h.levels))()
        keep = []
        for idx, lv in enumerate(h.levels):
            A = lv.A.tocsr()
            arrs = dict(
                Ap=i32(A.indptr), Ai=i32(A.indices), Ad=f64(A.data), dinv=f64(lv.dinv)
            )
            L = levels[idx]
            L.n = A.shape[0]
            L.n_cols = n_cols0 if idx == 0 else 0
            L.A_indptr, L.A_indices, L.A_data = p_i32(arrs["Ap"]), p_i32(arrs["Ai"]), p_f64(arrs["Ad"])
            L.dinv = p_f64(arrs["dinv"])
            L.rho = float(lv.rho)
            if lv.P is not None:
                P, R = lv.P.tocsr(), lv.R.tocsr()
                arrs.update(Pp=i32(P.indptr), Pi=i32(P.indices), Pd=f64(P.data),
                            Rp=i32(R.indptr), Ri=i32(R.indices), Rd=f64(R.data))
                L.n_coarse = P.shape[1]
                L.P_indptr, L.P_indices, L.P_data = p_i32(arrs["Pp"]), p_i32(arrs["Pi"]), p_f64(arrs["Pd"])
                L.R_indptr, L.R_indices, L.R_data = p_i32(arrs["Rp"]), p_i32(arrs["Ri"]), p_f64(arrs["Rd"])
            else:
                L.n_coarse = 0
            keep.append(arrs)
        pinv = f64(h.coarse_pinv)
        with _Stopwatch(self.setup_times, "upload"):
            self._chk(self._lib.tdgl_poisson_set_hierarchy(self._ctx, levels, len(h.levels), p_f64(pinv)))
        self.hierarchy = h
        self.dense_direct = False  # (tdgl_poisson_set_hierarchy releases the factors of a direct solve)
        self.substructure = None
        self._hier_epoch = getattr(self, "_hier_epoch", 0) + 1
        self._refresh_fused_restriction()
        self._set_fused_levels(h)
        self._refresh_collapsed()

    def _set_fused_levels(self, h, on=True):
        """Pre-multiplied transfer operators of the coarse levels (one launch instead of two on
        the way down and on the way up; `tdgl_poisson_set_fused_level`)."""
        from .amg import fused_level_operators

        for k in range(1, len(h.levels) - 1):
            if h.levels[k].A is None:  # a distributed level 1 (set_hierarchy_deep): explicit operators only
                continue
            if not on:
                self._chk(self._lib.tdgl_poisson_set_fused_level(self._ctx, k, None, None, None, None, None, None, None))
                continue
            with _Stopwatch(self.setup_times, "amg_host"):
                RA, AP, p_on_ap = fused_level_operators(h.levels[k])
            a = [i32(RA.indptr), i32(RA.indices), f64(RA.data), i32(AP.indptr), i32(AP.indices), f64(AP.data),
                 f64(p_on_ap)]
            with _Stopwatch(self.setup_times, "upload"):
                self._chk(self._lib.tdgl_poisson_set_fused_level(
                    self._ctx, k, p_i32(a[0]), p_i32(a[1]), p_f64(a[2]), p_i32(a[3]), p_i32(a[4]), p_f64(a[5]), p_f64(a[6])))

    def _refresh_fused_restriction(self):
        """(Re)build R0 (I - c A0 D0^-1) for the level-0 smoothing coefficient in use
        (single-GPU, degree-1 smoothing on level 0; `tdgl_poisson_set_fused_restriction`)."""
        h, o = getattr(self, "hierarchy", None), getattr(self, "poisson_options", None)
        if h is None or o is None or len(h.levels) < 2:
            return
        if o["nu_fine"] != 1 or not o.get("fused_restriction", True):
            self._chk(self._lib.tdgl_poisson_set_fused_restriction(self._ctx, 0, 0, None, None, None, 0.0))
            self._fusedR_key = None
            return
        from .amg import fused_restriction, fused_restriction_from, smoother_coefficients

        name = "jacobi" if o["smoother"] == 0 else "chebyshev"
        c = smoother_coefficients(h.levels[0].rho, 1, name, o["cheb_lo"])[1][0]
        lv0 = getattr(self, "_local_level0", None)
        dp = getattr(self, "_deep", None)
        if dp is not None:  # two distributed levels: the rows the root cut for this rank, for ITS coefficient
            if abs(dp.c - c) > 1e-12 * c:
                raise ValueError("the two-level decomposition was prepared for the default smoother settings "
                                 f"(level-0 coefficient {dp.c}); these options give {c}")
            key = (getattr(self, "_hier_epoch", 0), float(c))
            if getattr(self, "_fusedR_key", None) == key:
                return
            M = dp.F
            ip, ix, dx = i32(M.indptr), i32(M.indices), f64(M.data)
            with _Stopwatch(self.setup_times, "upload"):
                self._chk(self._lib.tdgl_poisson_set_fused_restriction(
                    self._ctx, M.shape[0], M.shape[1], p_i32(ip), p_i32(ix), p_f64(dx), float(c)))
            self._fusedR_key = key
            return
        if lv0 is None and self.n_owned != self.n:
            return
        key = (getattr(self, "_hier_epoch", 0), float(c))
        if getattr(self, "_fusedR_key", None) == key:  # already on the device for this hierarchy / coefficient
            return
        with _Stopwatch(self.setup_times, "amg_host"):
            if lv0 is not None:  # one process per GPU: this rank's slice in LOCAL numbering, ghost columns included
                M = fused_restriction_from(lv0.A, lv0.R, lv0.dinv, c)
            else:
                M = fused_restriction(h, c)
        ip, ix, dx = i32(M.indptr), i32(M.indices), f64(M.data)
        with _Stopwatch(self.setup_times, "upload"):
            self._chk(self._lib.tdgl_poisson_set_fused_restriction(
                self._ctx, M.shape[0], M.shape[1], p_i32(ip), p_i32(ix), p_f64(dx), float(c)))
        self._fusedR_key = key

    def _refresh_collapsed(self):
        """(Re)build the collapsed coarse chain for the smoother settings in use
        (`amg.collapsed_operators`; `tdgl_poisson_set_collapsed_level` / `_tail`)."""
        h, o = getattr(self, "hierarchy", None), getattr(self, "poisson_options", None)
        if h is None or o is None or len(h.levels) < 3:
            return
        lib, ctx = self._lib, self._ctx
        key = (getattr(self, "_hier_epoch", 0), o["nu"], o["smoother"], o["cheb_lo"], o.get("collapse", True),
               o.get("tail_cycles", 2))
        if getattr(self, "_collapsed_key", None) == key:
            return
        self._collapsed_key = key
        from .amg import collapsed_operators

        name = "jacobi" if o["smoother"] == 0 else "chebyshev"
        shipped = getattr(self, "_shipped_plan", None)
        if shipped is not None and shipped[0] == (o["nu"], o["smoother"], o["cheb_lo"], o.get("collapse", True),
                                                   o.get("tail_cycles", 2)):
            plan = shipped[1]  # built once by the root rank (distributed.prepare_payloads)
        elif getattr(self, "_deep", None) is not None:
            raise ValueError("the two-level decomposition was prepared for the default smoother settings; "
                             f"these options ({o['nu']}, {o['smoother']}, {o['cheb_lo']}) need another set-up")
        else:
            with _Stopwatch(self.setup_times, "amg_host"):
                plan = collapsed_operators(h, o["nu"], name, o["cheb_lo"], tail_cycles=o.get("tail_cycles", 2)) \
                    if (o.get("collapse", True) and o["nu"] == 2) else None
        self.collapsed_plan = plan
        for k in range(1, len(h.levels) - 1):
            M = None if plan is None else plan["mid"].get(k)
            if M is None:
                self._chk(lib.tdgl_poisson_set_collapsed_level(ctx, k, None, None, None))
            else:
                a = (i32(M.indptr), i32(M.indices), f64(M.data))
                self._chk(lib.tdgl_poisson_set_collapsed_level(ctx, k, p_i32(a[0]), p_i32(a[1]), p_f64(a[2])))
            up = None if plan is None else plan.get("up", {}).get(k)
            if up is None:
                self._chk(lib.tdgl_poisson_set_collapsed_up(ctx, k, None, None, None, None, None, None))
            else:
                W, V = up
                a = (i32(W.indptr), i32(W.indices), f64(W.data), i32(V.indptr), i32(V.indices), f64(V.data))
                self._chk(lib.tdgl_poisson_set_collapsed_up(ctx, k, p_i32(a[0]), p_i32(a[1]), p_f64(a[2]), p_i32(a[3]),
                                                            p_i32(a[4]), p_f64(a[5])))
        if plan is None:
            self._chk(lib.tdgl_poisson_set_collapsed_tail(ctx, None))
            return
        t = _lib.CollapsedTail()
        t.level, t.nu, t.smoother, t.cheb_lo = plan["tail"], int(o["nu"]), int(o["smoother"]), float(o["cheb_lo"])
        if plan["mode"] == "dense":
            keep = (f64(plan["B"]),)
            t.mode, t.G, t.g_rows = 0, p_f64(keep[0]), keep[0].shape[0]
        else:
            W = plan["W"]
            keep = (f64(plan["G"]), i32(W.indptr), i32(W.indices), f64(W.data), f64(plan["V"]))
            t.mode, t.G, t.g_rows = 1, p_f64(keep[0]), keep[0].shape[0]
            t.W_indptr, t.W_indices, t.W_data = p_i32(keep[1]), p_i32(keep[2]), p_f64(keep[3])
            t.v_cols = plan["V"].shape[1]
            t.V = p_f64(keep[4]) if t.v_cols else None
        self._chk(lib.tdgl_poisson_set_collapsed_tail(ctx, C.byref(t)))

    def set_poisson_options(self, rtol=1e-10, max_iter=500, nu=2, check_every=0,
                            edge_currents_every_step=True, smoother="chebyshev", cheb_lo=0.1,
                            extrapolate=3, nu_fine=1, fused_restriction=True, precond_fp32=True,
                            collapse=True, tail_cycles=2, guess_window=0, flexible_cg=False):
        kind = {"jacobi": 0, "chebyshev": 1}[smoother] if isinstance(smoother, str) else int(smoother)
        # storage of the V-cycle's operators: False / 0 fp64, 1 fp32, True / 2 fp32 + binary16 on level 0
        from .options import precond_storage_mode

        precond_fp32 = precond_storage_mode(precond_fp32)
        o = _lib.PoissonOptions(float(rtol), int(max_iter), int(nu), int(check_every),
                                int(bool(edge_currents_every_step)), kind, float(cheb_lo),
                                int(extrapolate), int(nu_fine), precond_fp32, int(guess_window), int(flexible_cg))
        self.poisson_options = dict(rtol=rtol, max_iter=max_iter, nu=nu, nu_fine=nu_fine, check_every=check_every,
                                    smoother=kind, cheb_lo=cheb_lo, extrapolate=int(extrapolate),
                                    fused_restriction=bool(fused_restriction), precond_fp32=precond_fp32,
                                    edge_currents_every_step=bool(edge_currents_every_step),
                                    collapse=bool(collapse), tail_cycles=int(tail_cycles),
                                    guess_window=int(guess_window), flexible_cg=int(flexible_cg))
        self._chk(self._lib.tdgl_set_poisson_options(self._ctx, C.byref(o)))
        self._refresh_fused_restriction()
        self._refresh_collapsed()

    # -- inputs ---------------------------------------------------------------------------
    def set_link_exponents(self, A):
        A = f64(A)
        if A.shape != (self.m, 2):
            raise ValueError(f"Unexpected shape for vector_potential: {A.shape}.")
        self._chk(self._lib.tdgl_set_link_exponents(self._ctx, p_f64(A)))

    def update_link_exponents(self, A_new, dt_prev):
        """Time-dependent A: new link exponents + dA/dt for the next step (solver.py:626-642)."""
        A_new = f64(A_new)
        if A_new.shape != (self.m, 2):
            raise ValueError(f"Unexpected shape for vector_potential: {A_new.shape}.")
        self._chk(self._lib.tdgl_update_link_exponents(self._ctx, p_f64(A_new), float(dt_prev)))

    def set_link_exponents_base(self, A_base, scale=1.0):
        """A = scale * A_base, A_base kept on the device (static semantics: dA/dt = 0)."""
        A_base = f64(A_base)
        if A_base.shape != (self.m, 2):
            raise ValueError(f"Unexpected shape for vector_potential: {A_base.shape}.")
        self._chk(self._lib.tdgl_set_link_exponents_base(self._ctx, p_f64(A_base), float(scale)))

    def update_link_scale(self, scale, dt_prev):
        """A <- scale * A_base with dA/dt from the previous A (no upload)."""
        self._chk(self._lib.tdgl_update_link_scale(self._ctx, float(scale), float(dt_prev)))

    def set_link_ramp(self, tmin, tmax, initial, final, on=True):
        """Let ``run`` evaluate A(t) = LinearRamp(t) * A_base itself before every step."""
        self._chk(self._lib.tdgl_set_link_ramp(self._ctx, int(bool(on)), float(tmin), float(tmax),
                                               float(initial), float(final)))

    def set_link_table(self, times, values):
        """Let ``run`` evaluate A(t) = PiecewiseLinear(times, values)(t) * A_base itself before every step (in the
        ramp's place); ``times=None``: off."""
        self._chk(self._lib.tdgl_set_link_table(self._ctx, *link_table_args(times, values)))

    def link_scale(self):
        v = C.c_double(0)
        self._chk(self._lib.tdgl_get_link_scale(self._ctx, C.byref(v)))
        return v.value

    def set_link_terms(self, A0, terms):
        """Let ``run`` evaluate A(t) = A0 + f_1(t) A_1 + ... + f_K(t) A_K itself before every step: ``A0`` [m, 2] or
        None, ``terms`` a list of ``(A_k[m, 2], spec_k)`` with ``spec_k`` a ramp's dict or a table's ``(times,
        values)`` (`link_terms_args`).  Replaces ramp and table."""
        self._chk(self._lib.tdgl_set_link_terms(self._ctx, *link_terms_args(self.m, A0, terms)))

    def update_link_terms(self, scales, dt_prev):
        """Move the sum of terms to the factors ``scales`` now, with dA/dt from the previous A (no upload)."""
        scales = f64(scales)
        self._chk(self._lib.tdgl_update_link_terms(self._ctx, p_f64(scales), float(dt_prev)))

    def link_term_scales(self):
        """The factors of the current A of a sum of terms (empty: no terms are set)."""
        n, v = C.c_int32(0), np.zeros(FIELD_TERMS_MAX)
        self._chk(self._lib.tdgl_get_link_term_scales(self._ctx, C.byref(n), p_f64(v)))
        return v[:n.value]

    def link_term_moves(self) -> int:
        """Steps that have moved the sum of terms since it was set (the others skipped the edge pass)."""
        v = C.c_int64(0)
        self._chk(self._lib.tdgl_get_link_term_moves(self._ctx, C.byref(v)))
        return v.value

    def set_link_loops(self, edge_centres, z_film, loops):
        """Add moving current loops to the field in force (a static A or a sum of terms): ``run`` evaluates their
        centres and currents itself before every step (`link_loops_args`).  ``loops`` empty or None: remove them."""
        if not loops:
            self._chk(self._lib.tdgl_set_link_loops(self._ctx, 0, None, 0.0, None, None, None, None, None, None, None))
            return
        self._chk(self._lib.tdgl_set_link_loops(self._ctx, *link_loops_args(self.m, edge_centres, z_film, loops)))

    def update_link_loops(self, term_scales, loop_params, dt_prev):
        """Move the field to the K factors and the loops' ``[L, 4]`` values (cx, cy, cz, current) now."""
        ts = f64(np.atleast_1d(term_scales)) if term_scales is not None and len(term_scales) else np.zeros(1)
        lp = f64(np.asarray(loop_params, dtype=float).reshape(-1))
        self._chk(self._lib.tdgl_update_link_loops(self._ctx, p_f64(ts), p_f64(lp), float(dt_prev)))

    def link_loop_params(self):
        """``[L, 4]``: centre x, y, z and current of every moving loop in the current A (empty: none are set)."""
        n, v = C.c_int32(0), np.zeros(4 * FIELD_LOOPS_MAX)
        self._chk(self._lib.tdgl_get_link_loop_params(self._ctx, C.byref(n), p_f64(v)))
        return v[:4 * n.value].reshape(n.value, 4)

    def link_exponents(self):
        """The applied vector potential ``A[m, 2]`` in force on the device, whatever set it."""
        A = np.zeros((self.m, 2))
        self._chk(self._lib.tdgl_get_link_exponents(self._ctx, p_f64(A)))
        return A

    def set_epsilon(self, eps):
        eps = f64(np.broadcast_to(eps, (self.n,)))
        self._chk(self._lib.tdgl_set_epsilon(self._ctx, p_f64(eps)))
        self._n_eps_spots = 0  # (plain values, a table and spots replace each other)

    def set_mu_boundary(self, mu_b):
        mu_b = f64(mu_b)
        assert mu_b.shape == (self.n_boundary,)
        self._chk(self._lib.tdgl_set_mu_boundary(self._ctx, p_f64(mu_b)))

    def set_mu_boundary_table(self, times, groups, densities):
        """Tabulated terminal current densities evaluated inside `run` (arguments: `mu_boundary_table_args`)."""
        self._chk(self._lib.tdgl_set_mu_boundary_table(self._ctx, *mu_boundary_table_args(times, groups, densities)))

    def set_epsilon_table(self, epsilon0, times, factors):
        """epsilon(r, t) = factor(t) * epsilon0(r) evaluated inside `run`; ``times=None``: off."""
        self._chk(self._lib.tdgl_set_epsilon_table(self._ctx, *epsilon_table_args(self.n, epsilon0, times, factors)))
        if times is not None:
            self._n_eps_spots = 0

    def set_epsilon_spots(self, sites, eps0, spots):
        """epsilon(r, t) = eps0(r) - sum_k a_k(t) exp(-|r - c_k(t)|^2 / (2 sigma_k(t)^2)) evaluated inside `run`
        (`epsilon_spots_args`); sets epsilon to its value at t = 0.  ``spots`` empty or None: off."""
        if not spots:
            self._chk(self._lib.tdgl_set_epsilon_spots(self._ctx, None, None, 0, None, None, None, None, None, None))
            self._n_eps_spots = 0
            return
        args = epsilon_spots_args(self.n, sites, eps0, spots)
        self._chk(self._lib.tdgl_set_epsilon_spots(self._ctx, *args))
        self._n_eps_spots = args[2]

    def update_epsilon_spots(self, values):
        """Apply the spots' ``[K, 4]`` values (cx, cy, a, sigma) now."""
        v = f64(np.asarray(values, dtype=float).reshape(-1, 4))
        if len(v) != self._n_eps_spots:
            raise ValueError(f"update_epsilon_spots: {self._n_eps_spots} spots are set, got values for {len(v)}.")
        self._chk(self._lib.tdgl_update_epsilon_spots(self._ctx, p_f64(v)))

    def epsilon_spot_values(self):
        """``[K, 4]``: centre x, y, amplitude and width of every spot of the epsilon in force (empty: none are set)."""
        n, v = C.c_int32(0), np.zeros(4 * EPS_SPOTS_MAX)
        self._chk(self._lib.tdgl_get_epsilon_spot_values(self._ctx, C.byref(n), p_f64(v)))
        return v[:4 * n.value].reshape(n.value, 4)

    def epsilon(self):
        """The disorder parameter ``epsilon[n]`` in force on the device, whatever set it."""
        eps = np.zeros(self.n)
        self._chk(self._lib.tdgl_get_epsilon(self._ctx, p_f64(eps)))
        return eps

    def set_state(self, psi, mu):
        psi, mu = c128(psi), f64(mu)
        assert psi.shape == (self.n,) and mu.shape == (self.n,)
        self._chk(self._lib.tdgl_set_state(self._ctx, p_f64(psi), p_f64(mu)))

    def set_controller(self, dt_init, dt_max, adaptive, adaptive_window, max_solve_retries,
                       adaptive_time_step_multiplier):
        c = controller_struct(dt_init, dt_max, adaptive, adaptive_window, max_solve_retries, adaptive_time_step_multiplier)
        self._chk(self._lib.tdgl_set_controller(self._ctx, C.byref(c)))

    def set_probes(self, sites):
        sites, self.n_probe = probe_args(sites)
        self._chk(self._lib.tdgl_set_probes(self._ctx, sites, self.n_probe))

    def set_census(self, points=None, triangles=None, loops=()):
        """Count vortices and loop windings at every accepted step inside `run` (csrc/census.inc): ``points`` [n, 2],
        ``triangles`` [t, 3] and ``loops`` (site-index sequences, closed, the first site not repeated) as for
        `VortexPlan`, in the reference numbering.  ``run`` then returns ``census`` [k, 2 + L] int32 rows
        ``(n_plus, n_minus, w_0 .. w_{L-1})`` with `WINDING_UNDEFINED` where a winding is not defined.  No triangles and
        no loops (the default arguments): off."""
        n_tri, elements, n_loops, loop_ptr, loop_sites = census_args(triangles, loops)
        if n_tri:  # (the points give the triangles' orientations)
            points = f64(points)
            if points.shape != (self.n, 2):
                raise ValueError(f"Expected points [{self.n}, 2] (got {points.shape}).")
        else:
            points = None
        self._chk(self._lib.tdgl_set_census(self._ctx, p_f64(points), n_tri, p_i32(elements), n_loops, p_i64(loop_ptr),
                                            p_i32(loop_sites)))
        self.n_census = (2 + n_loops) if (n_tri or n_loops) else 0

        self.core_records = False  # (they belong to the census they were set on)

    def census(self):
        """The census rows of the last `run`, [k, 2 + L] int32, or None when the census is off."""
        if not self.n_census:
            return None
        return read_census(self._chk, self.n_census, self._lib.tdgl_get_census, self._ctx)

    def set_core_records(self, points, capacity, every=1):
        """Record the vortex cores themselves after every accepted step whose running index -- counted from this call on,
        the first step being 0, across `run` calls -- is divisible by ``every``, out of the census' own launch
        (`set_census` with triangles first; csrc/census.inc).  ``points`` [n, 2] as for `set_census`; ``capacity``:
        records the device keeps between two flushes (every 1,024 steps and at the end of a `run`), 0 switches the
        records off, and so does every `set_census`.  ``run`` then returns ``cores``: ``steps`` (rows of the run's
        ``dt``), ``counts``, ``complete``, and the concatenated ``triangles``, ``charges``, ``positions`` [N, 2] -- per
        step what `VortexPlan.find` / `vortices.host_find` give for psi after that step.  A step whose records reach
        beyond the capacity, and every later one up to the next flush, is incomplete and has none."""
        capacity = int(capacity)
        points = f64(points) if capacity != 0 and points is not None else None
        if points is not None and points.shape != (self.n, 2):
            raise ValueError(f"Expected points [{self.n}, 2] (got {points.shape}).")
        self._chk(self._lib.tdgl_set_core_records(self._ctx, p_f64(points), capacity, int(every)))
        self.core_records = capacity > 0

    def cores(self):
        """The core records of the last `run` (see `set_core_records`), or None when they are off."""
        if not self.core_records:
            return None
        return read_core_records(self._chk, self._lib.tdgl_get_core_records, self._ctx)

    # -- time loop --------------------------------------------------------------------------
    def begin_stage(self):
        self._chk(self._lib.tdgl_begin_stage(self._ctx))

    def run(self, max_steps, end_time=np.inf):
        """Up to ``max_steps`` iterations of the reference's loop.  Returns a dict with
        ``dt[k]``, ``mu[k, n_probe]``, ``theta[k, n_probe]``, ``pcg_iters[k]``,
        ``reached_end``."""
        max_steps = int(max_steps)
        dts = np.zeros(max_steps)
        npb = self.n_probe
        mu_p = np.zeros((max_steps, npb)) if npb else None
        th_p = np.zeros((max_steps, npb)) if npb else None
        iters = np.zeros(max_steps, dtype=np.int32)
        scr_iters = np.zeros(max_steps, dtype=np.int32)
        done, reached = C.c_int64(0), C.c_int32(0)
        status = self._lib.tdgl_run(
            self._ctx, max_steps, float(end_time), p_f64(dts), p_f64(mu_p), p_f64(th_p),
            p_i32(iters), C.byref(done), C.byref(reached), p_i32(scr_iters),
        )
        self._chk(status)
        k = done.value
        return dict(
            dt=dts[:k], mu=None if mu_p is None else mu_p[:k],
            theta=None if th_p is None else th_p[:k], pcg_iters=iters[:k],
            screening_iterations=scr_iters[:k], reached_end=bool(reached.value), census=self.census(),
            cores=self.cores(),
        )

    # -- screening (solver.py:522-578, 654-688) -----------------------------------------------
    def set_screening(self, sites, edge_centers, areas, max_iterations=1000, tolerance=1e-3,
                      step_size=0.1, step_drag=0.5):
        """Enable the self-consistent induced vector potential.  ``sites`` / ``edge_centers`` are
        coordinates in the length unit of the 1/r kernel and ``areas`` the site areas already
        multiplied by the kernel's prefactor (so that A_induced comes out in units of the applied
        link exponents).  ``None`` for ``sites`` disables screening."""
        if sites is None:
            self._chk(self._lib.tdgl_set_screening(self._ctx, None, None, None, None))
            return
        opts = _lib.ScreeningOptions(int(max_iterations), float(tolerance), float(step_size), float(step_drag))
        sites, edge_centers, areas = f64(sites), f64(edge_centers), f64(areas)
        if sites.shape != (self.n, 2) or edge_centers.shape != (self.m, 2) or areas.shape != (self.n,):
            raise ValueError("set_screening: sites (n, 2), edge_centers (m, 2), areas (n,) expected")
        self._chk(self._lib.tdgl_set_screening(self._ctx, C.byref(opts), p_f64(sites), p_f64(edge_centers), p_f64(areas)))

    def set_screening_distributed(self, global_sites, global_areas, owned_global_ids, edge_centers,
                                  max_iterations=1000, tolerance=1e-3, step_size=0.1, step_drag=0.5):
        """Screening in one-process-per-GPU mode: global site arrays (global order), the global ids
        of this rank's owned sites and the centres of its local edges."""
        opts = _lib.ScreeningOptions(int(max_iterations), float(tolerance), float(step_size), float(step_drag))
        gs, ga, ec = f64(global_sites), f64(global_areas), f64(edge_centers)
        ids = np.ascontiguousarray(owned_global_ids, dtype=np.int64)
        if gs.ndim != 2 or gs.shape[1] != 2 or ga.shape != (len(gs),) or ec.shape != (self.m, 2) or len(ids) != self.n_owned:
            raise ValueError("set_screening_distributed: inconsistent array shapes")
        self._chk(self._lib.tdgl_set_screening_distributed(
            self._ctx, C.byref(opts), p_f64(gs), p_f64(ga), ids.ctypes.data_as(C.POINTER(C.c_int64)), p_f64(ec)))

    def set_induced_vector_potential(self, A):
        A = f64(A)
        if A.shape != (self.m, 2):
            raise ValueError("A_induced must have shape (n_edges, 2)")
        self._chk(self._lib.tdgl_set_induced_vector_potential(self._ctx, p_f64(A)))

    def evaluate_induced_vector_potential(self, edge_current):
        """One evaluation of the 1/r kernel for an edge current (no heavy-ball update)."""
        k = f64(edge_current)
        if k.shape != (self.m,):
            raise ValueError("edge_current must have shape (n_edges,)")
        A = np.empty((self.m, 2))
        self._chk(self._lib.tdgl_induced_vector_potential(self._ctx, p_f64(k), p_f64(A)))
        return A

    def set_screening_tree(self, degree, theta):
        """Evaluate the induced vector potential with the barycentric Lagrange treecode from now on (after
        `set_screening`): degree p in [2, 16] ((p + 1)^2 proxies per far cluster), acceptance parameter theta in
        (0, 1).  ``degree=0`` returns to the all-pairs kernel.  A refused call leaves the previous method in place."""
        self._chk(self._lib.tdgl_set_screening_tree(self._ctx, int(degree), float(theta)))

    def screening_tree_stats(self):
        """``dict(clusters, levels, batches, far_pairs, near_pairs, setup_us)`` of the active treecode (pairs summed
        over all edge centres); all zero with the all-pairs kernel."""
        out = (C.c_int64 * 6)()
        self._chk(self._lib.tdgl_get_screening_tree_stats(self._ctx, out))
        return dict(zip(("clusters", "levels", "batches", "far_pairs", "near_pairs", "setup_us"), (int(v) for v in out)))

    def induced_vector_potential(self):
        A = np.empty((self.m, 2))
        self._chk(self._lib.tdgl_get_induced_vector_potential(self._ctx, p_f64(A)))
        return A

    def step_stats(self, reset=False):
        """``dict(steps, psi_retries, pcg_iterations, host_syncs, host_wait_s, run_s, edge_current_launches)`` of
        `run` since the last reset (``host_wait_s``: time blocked in the synchronisations; ``run_s``: time inside
        `run`; ``edge_current_launches``: how often J_s / J_n were formed outside the run-ahead loop)."""
        out = (C.c_int64 * 6)()
        self._chk(self._lib.tdgl_get_step_stats(self._ctx, out, int(bool(reset))))
        edge = C.c_int64(0)
        self._chk(self._lib.tdgl_get_edge_current_launches(self._ctx, C.byref(edge), int(bool(reset))))
        return dict(steps=out[0], psi_retries=out[1], pcg_iterations=out[2], host_syncs=out[3],
                    host_wait_s=out[4] * 1e-9, run_s=out[5] * 1e-9, edge_current_launches=edge.value)

    def direct_stats(self):
        """In-loop guard of the direct mu solves: ``dict(max, checks, fell_back)`` -- the largest
        ``||b - A mu|| / ||b||`` measured on accepted steps, the number of steps checked, and whether a check
        above the limit released the factors (the run continued with AMG-PCG).  Refreshes `dense_direct` /
        `substructure` accordingly."""
        r, n, f = C.c_double(0), C.c_int64(0), C.c_int32(0)
        self._chk(self._lib.tdgl_get_direct_stats(self._ctx, C.byref(r), C.byref(n), C.byref(f)))
        if f.value:
            self.dense_direct = False
            self.substructure = None
        return dict(max=r.value, checks=n.value, fell_back=bool(f.value))

    def set_direct_guard(self, limit=1e-9):
        self._chk(self._lib.tdgl_set_direct_guard(self._ctx, float(limit)))

    def loop_state(self):
        return read_loop_state(self._chk, self._lib.tdgl_get_loop_state, self._ctx)

    def set_loop_state(self, step, time, runner_dt):
        self._chk(self._lib.tdgl_set_loop_state(self._ctx, int(step), float(time), float(runner_dt)))

    def controller_state(self, capacity=4096):
        """``dict(tentative_dt, history)`` of the adaptive-dt controller (solver.py:316-320): the
        newest ``capacity`` entries of ``d_psi_sq_vals``, oldest first."""
        tdt, n = C.c_double(0), C.c_int64(0)
        hist = np.zeros(int(capacity))
        self._chk(self._lib.tdgl_get_controller_state(self._ctx, C.byref(tdt), p_f64(hist), int(capacity), C.byref(n)))
        return dict(tentative_dt=tdt.value, history=hist[:min(n.value, int(capacity))].copy())

    def set_controller_state(self, tentative_dt, history=()):
        hist = f64(history)
        self._chk(self._lib.tdgl_set_controller_state(self._ctx, float(tentative_dt), p_f64(hist) if len(hist) else None,
                                                      len(hist)))

    def get_state(self, psi=True, mu=True, supercurrent=True, normal_current=True):
        out = {}
        a_psi = np.empty(self.n, dtype=np.complex128) if psi else None
        a_mu = np.empty(self.n) if mu else None
        a_js = np.empty(self.m) if supercurrent else None
        a_jn = np.empty(self.m) if normal_current else None
        self._chk(self._lib.tdgl_get_state(self._ctx, p_f64(a_psi), p_f64(a_mu), p_f64(a_js), p_f64(a_jn)))
        if psi:
            out["psi"] = a_psi
        if mu:
            out["mu"] = a_mu
        if supercurrent:
            out["supercurrent"] = a_js
        if normal_current:
            out["normal_current"] = a_jn
        return out

    # -- single operators ---------------------------------------------------------------------
    def apply_psi_laplacian(self, psi):
        psi = c128(psi)
        out = np.empty(self.n, dtype=np.complex128)
        self._chk(self._lib.tdgl_apply_psi_laplacian(self._ctx, p_f64(psi), p_f64(out)))
        return out

    def supercurrent(self, psi):
        psi = c128(psi)
        out = np.empty(self.m)
        self._chk(self._lib.tdgl_supercurrent(self._ctx, p_f64(psi), p_f64(out)))
        return out

    def normal_current(self, mu):
        mu = f64(mu)
        out = np.empty(self.m)
        self._chk(self._lib.tdgl_normal_current(self._ctx, p_f64(mu), p_f64(out)))
        return out

    def apply_psi_gradient(self, psi):
        psi = c128(psi)
        out = np.empty(self.m, dtype=np.complex128)
        self._chk(self._lib.tdgl_apply_psi_gradient(self._ctx, p_f64(psi), p_f64(out)))
        return out

    def apply_divergence(self, edge_field):
        f = f64(edge_field)
        if f.shape != (self.m,):
            raise ValueError(f"divergence acts on edge fields of shape ({self.m},), got {f.shape}")
        out = np.empty(self.n)
        self._chk(self._lib.tdgl_apply_divergence(self._ctx, p_f64(f), p_f64(out)))
        return out

    def apply_mu_laplacian(self, mu):
        mu = f64(mu)
        out = np.empty(self.n)
        self._chk(self._lib.tdgl_apply_mu_laplacian(self._ctx, p_f64(mu), p_f64(out)))
        return out

    def apply_mu_boundary_laplacian(self, mu_b):
        mu_b = f64(mu_b)
        if mu_b.shape != (self.n_boundary,):
            raise ValueError(f"mu_boundary has shape ({self.n_boundary},), got {mu_b.shape}")
        out = np.empty(self.n)
        self._chk(self._lib.tdgl_apply_mu_boundary_laplacian(self._ctx, p_f64(mu_b), p_f64(out)))
        return out

    def psi_update(self, psi, mu, dt):
        """Returns ``(psi_new, abs_sq_new)`` or ``None`` (like solve_for_psi_squared)."""
        psi, mu = c128(psi), f64(mu)
        out = np.empty(self.n, dtype=np.complex128)
        sq = np.empty(self.n)
        ok = C.c_int32(0)
        self._chk(self._lib.tdgl_psi_update(self._ctx, p_f64(psi), p_f64(mu), float(dt), p_f64(out), p_f64(sq), C.byref(ok)))
        return (out, sq) if ok.value else None

    def poisson_rhs(self, psi):
        psi = c128(psi)
        out = np.empty(self.n)
        self._chk(self._lib.tdgl_poisson_rhs(self._ctx, p_f64(psi), p_f64(out)))
        return out

    def poisson_stats(self):
        out = (C.c_int64 * 3)()
        self._chk(self._lib.tdgl_get_poisson_stats(self._ctx, out))
        return dict(fp64_fallbacks=out[0], last_iterations=out[1], graph=bool(out[2]))

    def pcg_prediction_stats(self):
        """``dict(queued, needed, extra_looks, rate)``: PCG iterations queued (frozen ones included) and needed since
        the context was created, host looks after the first batch of a solve, and the running estimate of the
        decades per iteration the batch size is predicted with (`tdgl_get_pcg_prediction_stats`)."""
        out, rate = (C.c_int64 * 3)(), C.c_double(0)
        self._chk(self._lib.tdgl_get_pcg_prediction_stats(self._ctx, out, C.byref(rate)))
        return dict(queued=out[0], needed=out[1], extra_looks=out[2], rate=rate.value)

    def guess_stats(self):
        """``dict(vectors, initial_relres)`` of the last solve's initial guess."""
        k, r = C.c_int32(0), C.c_double(0)
        self._chk(self._lib.tdgl_get_guess_stats(self._ctx, C.byref(k), C.byref(r)))
        return dict(vectors=k.value, initial_relres=r.value)

    def guess_gram(self):
        """Gram matrix ``G_ij = y_i . y_j`` (``y = A x``) of the projection guess's window (``[k, k]``, oldest first)."""
        k = C.c_int32(0)
        G = np.zeros(256)
        self._chk(self._lib.tdgl_get_guess_gram(self._ctx, C.byref(k), p_f64(G)))
        return G[:k.value * k.value].reshape(k.value, k.value).copy()

    def poisson_solve(self, rhs, mu0=None):
        rhs = f64(rhs)
        mu = np.zeros(self.n) if mu0 is None else f64(mu0).copy()
        it, rel = C.c_int32(0), C.c_double(0)
        self._chk(self._lib.tdgl_poisson_solve(self._ctx, p_f64(rhs), p_f64(mu), C.byref(it), C.byref(rel)))
        return mu, it.value, rel.value

    def vcycle(self, r):
        r = f64(r)
        z = np.empty(self.n)
        self._chk(self._lib.tdgl_vcycle(self._ctx, p_f64(r), p_f64(z)))
        return z

    def precond_apply(self, r):
        """`tdgl_precond_apply`: one application of the factor preconditioner, ``(z, r . z)``; the CG's state stays as it is."""
        r = f64(r)
        z = np.empty(self.n)
        rz = np.zeros(1)
        self._chk(self._lib.tdgl_precond_apply(self._ctx, p_f64(r), p_f64(z), p_f64(rz)))
        return z, float(rz[0])

    def precond_schur_apply(self, r_own):
        """`tdgl_precond_schur_apply`: one application of the rank-level dissection on this rank's owned rows (local site
        order), ``(z_own, r . z)``.  COLLECTIVE: every rank calls it at the same point (one all-reduce of |Gamma| doubles).
        The CG's state stays as it is."""
        r = f64(r_own)
        if r.shape != (self.n_owned,):
            raise ValueError(f"r must be [{self.n_owned}] (the owned sites), got {r.shape}")
        z = np.empty(self.n_owned)
        rz = np.zeros(1)
        self._chk(self._lib.tdgl_precond_schur_apply(self._ctx, p_f64(r), p_f64(z), p_f64(rz)))
        return z, float(rz[0])

    def precond_apply_stats(self):
        """`tdgl_get_precond_apply_stats`: ``dict(folded, two_pass)`` -- applications of the factor preconditioner so far,
        by the order they took (``TDGL_PD_TWO_PASS`` at context creation selects the second)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.tdgl_get_precond_apply_stats(self._ctx, C.byref(a), C.byref(b)))
        return dict(folded=a.value, two_pass=b.value)

    def vcycle_stored(self, r, q=None):
        """`tdgl_vcycle_stored`: one application of the V-cycle in the precisions the CG applies it in
        (``precond_fp32`` = 1 or 2), ``(z, r . z)`` or, with ``q``, ``(z, r . z, q . z)``: z is the stored fp32 z, the
        sums are the smoothing pass's partials.  The CG's state stays as it is.  RuntimeError where the CG would
        apply the fp64 cycle (`vcycle`) and in one-process-per-GPU contexts."""
        r = f64(r)
        z = np.empty(self.n)
        rz, qz = np.zeros(1), np.zeros(1)
        if q is None:
            self._chk(self._lib.tdgl_vcycle_stored(self._ctx, p_f64(r), None, p_f64(z), p_f64(rz), None))
            return z, float(rz[0])
        q = f64(q)
        self._chk(self._lib.tdgl_vcycle_stored(self._ctx, p_f64(r), p_f64(q), p_f64(z), p_f64(rz), p_f64(qz)))
        return z, float(rz[0]), float(qz[0])

    def index_forms(self) -> dict:
        """`tdgl_get_poisson_index_forms`: the index form every operator of the stored-precision V-cycle was built with
        on this context.  ``laplacian16`` (the site graph's pattern behind the psi and mu Laplacian kernels: 16-bit row
        deltas; needs no hierarchy), ``A16`` (level-0 A: 16-bit row deltas), ``P16`` (level-0 P: 16-bit offsets from a slice base),
        ``F16`` (the fused restriction: 16-bit offsets from a row base), ``tailW16`` (the collapsed tail's sparse W):
        True / False, None where the operator does not exist; ``level0_f16``: level 0 reads the binary16 copies (known
        after a solve or `vcycle_stored`); ``levels``; ``tail`` = (level, "dense" | "gwv") or None; ``mid`` = {k:
        dict(off16, f16)} for every intermediate level with an explicit way up."""
        n_out = 24
        out = (C.c_int32 * n_out)()
        self._chk(self._lib.tdgl_get_poisson_index_forms(self._ctx, out))
        flag = lambda v: None if v < 0 else bool(v)  # noqa: E731
        return dict(laplacian16=flag(out[8]), A16=flag(out[0]), P16=flag(out[1]), F16=flag(out[2]), tailW16=flag(out[3]), level0_f16=bool(out[4] > 0),
                    levels=int(out[5]), tail=None if out[6] < 1 else (int(out[6]), "gwv" if out[7] == 1 else "dense"),
                    mid={k: dict(off16=bool(out[8 + k] & 1), f16=bool(out[8 + k] & 2))
                         for k in range(1, n_out - 8) if out[8 + k] >= 0})

    def precond_direct_blr_form(self):
        """`tdgl_get_precond_direct_blr_form`: the arrays of the block low-rank form the preconditioner stores, copied
        back from the device (dict, see `host_blr_form`); RuntimeError when the form is not in use."""
        return _blr_form_fill(lambda form: self._chk(self._lib.tdgl_get_precond_direct_blr_form(self._ctx, C.byref(form))))

    def blr_apply(self, G, tol_abs, X):
        """`tdgl_blr_apply`: the block low-rank form of the symmetric ``G [n, n]`` at the absolute tolerance ``tol_abs``
        applied to every column of ``X [n, k]`` by the form's two kernels alone.  Returns ``(Y [n, k], form)`` with the
        form this call built; the context's factors and the CG's state stay as they are."""
        G = f64(G)
        X = f64(X)
        n = G.shape[0]
        if G.shape != (n, n) or X.ndim != 2 or X.shape[0] != n:
            raise ValueError(f"G must be [n, n] and X [n, k], got {G.shape} and {X.shape}")
        Xt = np.ascontiguousarray(X.T)
        Yt = np.empty_like(Xt)
        form = _blr_form_fill(lambda fm: _lib.check(self._lib.tdgl_host_blr_form(n, p_f64(G), float(tol_abs), C.byref(fm))),
                              lambda fm: self._chk(self._lib.tdgl_blr_apply(self._ctx, n, p_f64(G), float(tol_abs), Xt.shape[0],
                                                                            p_f64(Xt), p_f64(Yt), C.byref(fm))))
        return np.ascontiguousarray(Yt.T), form

    def guess_dots(self, vectors, b, newest=-1):
        """The projection guess's dot-product pass on ``vectors [k, n]`` and ``b [n]`` (parity tests): dict of
        ``(hi, lo)`` double-double sums ``bb, sb, yb [k, 2], yy [k, 2]`` (``yy``: ``vectors[newest] . vectors[j]``)."""
        V = np.ascontiguousarray(vectors, dtype=np.float64)
        b = f64(b)
        k, n = V.shape
        out = np.zeros(2 * 34)
        self._chk(self._lib.tdgl_guess_dots(self._ctx, k, n, p_f64(V), p_f64(b), int(newest), p_f64(out)))
        pairs = out.reshape(34, 2)
        return dict(bb=pairs[0], sb=pairs[1], yb=pairs[2:2 + k].copy(), yy=pairs[18:18 + k].copy())

    # -- measurement -----------------------------------------------------------------------------
    def time_kernel(self, kernel: int, reps: int = 20) -> float:
        ms = C.c_double(0)
        self._chk(self._lib.tdgl_time_kernel(self._ctx, int(kernel), int(reps), C.byref(ms)))
        return ms.value

    def profile_enable(self, on=True):
        self._chk(self._lib.tdgl_profile_enable(self._ctx, int(bool(on))))

    def profile_read_pcg(self):
        n, ms = C.c_int64(0), C.c_double(0)
        self._chk(self._lib.tdgl_profile_read_pcg(self._ctx, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def profile_read_direct(self):
        """(solves bracketed, their total milliseconds): the direct mu solve's launch sequence, one sample per
        run-ahead batch since `profile_enable`."""
        n, ms = C.c_int64(0), C.c_double(0)
        self._chk(self._lib.tdgl_profile_read_direct(self._ctx, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def precond_storage(self) -> int:
        """Storage of the V-cycle's operators in the last solve: 0 fp64, 1 fp32, 2 fp32 + binary16 on level 0."""
        mode = C.c_int32(0)
        self._chk(self._lib.tdgl_get_precond_storage(self._ctx, C.byref(mode)))
        return mode.value

    def profile_event_overhead(self, reps: int = 50) -> float:
        """Mean reading (ms) of an event pair with nothing in between."""
        ms = C.c_double(0)
        self._chk(self._lib.tdgl_profile_event_overhead(self._ctx, int(reps), C.byref(ms)))
        return ms.value

    def profile_read(self):
        n, ms = C.c_int64(0), C.c_double(0)
        self._chk(self._lib.tdgl_profile_read(self._ctx, C.byref(n), C.byref(ms)))
        return n.value, ms.value


class FieldPlan:
    """Owns one ``tdgl_field_plan`` (csrc/fields.inc): ``n`` current-carrying sites in the plane ``z = z0`` and ``m``
    target points kept on the device; :meth:`eval` returns the bare all-pairs sums for given site currents (no
    ``mu_0 / 4 pi``, no units).  Needs no ``TDGLContext``.  A context manager; freed on ``__del__`` too."""

    VECTOR_POTENTIAL, BZ, BXY = 1, 2, 4  # bits of ``what``

    def __init__(self, sites_xy, areas, z0, targets_xyz, device_id=0):
        _lib.require_gpu()
        self._lib = _lib.load()
        self._plan = C.c_void_p()
        sites_xy, areas, targets_xyz = f64(sites_xy), f64(areas), f64(targets_xyz)
        if sites_xy.ndim != 2 or sites_xy.shape[1] != 2 or areas.shape != (len(sites_xy),):
            raise ValueError(f"Expected sites [n, 2] and areas [n] (got {sites_xy.shape}, {areas.shape}).")
        if targets_xyz.ndim != 2 or targets_xyz.shape[1] != 3:
            raise ValueError(f"Expected targets [m, 3] (got {targets_xyz.shape}).")
        self.n, self.m = len(sites_xy), len(targets_xyz)
        _lib.check(self._lib.tdgl_field_plan_create(
            C.byref(self._plan), int(device_id), self.n, p_f64(sites_xy), p_f64(areas), float(z0), self.m,
            p_f64(targets_xyz)))

    def eval(self, K, what=7):
        """``K``: [n, 2] or [n_fields, n, 2] with ``n_fields`` 1 or 2.  Returns ``(S_A, S_z, S_xy)`` of shapes
        [n_fields, m, 2], [n_fields, m], [n_fields, m, 2]; ``None`` for the sums ``what`` does not ask for."""
        if not self._plan.value:
            raise RuntimeError("FieldPlan is closed.")
        K = f64(K)
        if K.ndim == 2:
            K = K[None]
        if K.ndim != 3 or K.shape[1:] != (self.n, 2):
            raise ValueError(f"Expected currents of shape [n_fields, {self.n}, 2] (got {K.shape}).")
        nf, what = K.shape[0], int(what)
        S_A = np.empty((nf, self.m, 2)) if what & 1 else None
        S_z = np.empty((nf, self.m)) if what & 2 else None
        S_xy = np.empty((nf, self.m, 2)) if what & 4 else None
        _lib.check(self._lib.tdgl_field_plan_eval(self._plan, nf, p_f64(K), what, p_f64(S_A), p_f64(S_z), p_f64(S_xy)))
        return S_A, S_z, S_xy

    def stats(self) -> dict:
        """Of the last evaluation: pairs, kernel launches, source chunks of the first target batch, target batches,
        and the device time in milliseconds between the upload of the currents and the read-back."""
        out, ms = (C.c_int64 * 4)(), C.c_double(0)
        _lib.check(self._lib.tdgl_field_plan_stats(self._plan, out, C.byref(ms)))
        return dict(pairs=out[0], launches=out[1], source_chunks=out[2], target_batches=out[3], last_ms=ms.value)

    def close(self):
        if getattr(self, "_plan", None) is not None and self._plan.value:
            self._lib.tdgl_field_plan_destroy(self._plan)
            self._plan = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


WINDING_UNDEFINED = -(2 ** 31)  # TDGL_WINDING_UNDEFINED


class VortexPlan:
    """Owns one ``tdgl_vortex_plan`` (csrc/vortices.inc): the sites, the triangles with their orientation and closed
    loops of sites kept on the device; :meth:`find` returns, for a batch of order parameters, the charged triangles with
    their core positions and the winding around every loop.  ``loops``: a sequence of site-index sequences (at least
    3 sites each, the first not repeated).  Needs no ``TDGLContext``.  A context manager; freed on ``__del__`` too."""

    def __init__(self, sites_xy, elements, loops=(), device_id=0):
        _lib.require_gpu()
        self._lib = _lib.load()
        self._plan = C.c_void_p()
        sites_xy = f64(sites_xy)
        if sites_xy.ndim != 2 or sites_xy.shape[1] != 2:
            raise ValueError(f"Expected sites [n, 2] (got {sites_xy.shape}).")
        elements = i32(np.asarray(elements).reshape(-1, 3))
        loops = [i32(np.asarray(loop).reshape(-1)) for loop in loops]
        loop_ptr = np.zeros(len(loops) + 1, dtype=np.int64)
        loop_ptr[1:] = np.cumsum([len(loop) for loop in loops])
        loop_sites = i32(np.concatenate(loops)) if loops else np.zeros(0, dtype=np.int32)
        self.n, self.n_tri, self.n_loops = len(sites_xy), len(elements), len(loops)
        self.last_capacity = 0  # records the last call of find() held: its next call starts there
        _lib.check(self._lib.tdgl_vortex_plan_create(
            C.byref(self._plan), int(device_id), self.n, p_f64(sites_xy), self.n_tri, p_i32(elements), self.n_loops,
            p_i64(loop_ptr), p_i32(loop_sites)))

    def _frames(self, psi):
        if not self._plan.value:
            raise RuntimeError("VortexPlan is closed.")
        psi = c128(psi)
        if psi.ndim == 1:
            psi = psi[None]
        if psi.ndim != 2 or psi.shape[1] != self.n or len(psi) < 1:
            raise ValueError(f"Expected psi of shape [n_frames, {self.n}] (got {psi.shape}).")
        return psi

    def find_once(self, psi, capacity, windings=True):
        """One call of ``tdgl_vortex_plan_find`` with room for ``capacity`` records: ``(counts [F], triangles [k],
        charges [k], xy [k, 2], windings [F, n_loops] or None)`` with ``k = min(counts.sum(), capacity)``, the first
        ``k`` records in (frame, triangle) order."""
        psi = self._frames(psi)
        capacity = int(capacity)
        counts = np.zeros(len(psi), dtype=np.int64)
        tri_charge = np.zeros((max(capacity, 0), 2), dtype=np.int32)
        xy = np.zeros((max(capacity, 0), 2))
        wind = np.zeros((len(psi), self.n_loops), dtype=np.int32) if windings else None
        _lib.check(self._lib.tdgl_vortex_plan_find(self._plan, len(psi), p_f64(psi), capacity, p_i64(counts),
                                                   p_i32(tri_charge), p_f64(xy), p_i32(wind)))
        k = min(int(counts.sum()), capacity)
        return counts, tri_charge[:k, 0].copy(), tri_charge[:k, 1].copy(), xy[:k], wind

    def find(self, psi, windings=True):
        """All records of ``psi`` ([n] or [F, n]): as :meth:`find_once`, retried exactly once with the exact capacity
        when the first call's did not hold them."""
        psi = self._frames(psi)
        capacity = max(self.last_capacity, 1024)
        out = self.find_once(psi, capacity, windings)
        total = int(out[0].sum())
        if total > capacity:
            capacity = total
            out = self.find_once(psi, capacity, windings)
        self.last_capacity = capacity
        return out

    def windings(self, psi):
        """The windings alone, [F, n_loops] int32 with ``WINDING_UNDEFINED`` where a loop's is not defined."""
        psi = self._frames(psi)
        wind = np.zeros((len(psi), self.n_loops), dtype=np.int32)
        _lib.check(self._lib.tdgl_vortex_plan_find(self._plan, len(psi), p_f64(psi), 0, None, None, None, p_i32(wind)))
        return wind

    def stats(self) -> dict:
        """Of the last call: charged triangles found, frames, chunks of frames, kernel launches, and the device time
        in milliseconds between the uploads of psi and the read-back."""
        out, ms = (C.c_int64 * 4)(), C.c_double(0)
        _lib.check(self._lib.tdgl_vortex_plan_stats(self._plan, out, C.byref(ms)))
        return dict(found=out[0], frames=out[1], chunks=out[2], launches=out[3], last_ms=ms.value)

    def link(self, counts, xy, charges, max_distance):
        """``tdgl_vortex_plan_link``: the cores of ``len(counts)`` frames (``counts[f]`` cores each, ``xy`` [total, 2]
        and ``charges`` [total] of all frames one after the other) linked from each frame to the next by mutual nearest
        neighbour of equal charge within ``max_distance``.  Returns ``(next, prev, end_partner, start_partner, near,
        near_d2)``, one entry per core: int32 indices within the neighbouring (for the partners: the same) frame or -1,
        ``near`` the position of the nearest loop site in the plan's concatenated loops with ``near_d2`` its squared
        distance (-1 and inf without loops).  The rule is DESIGN.md section 3, "Tracks"."""
        if not self._plan.value:
            raise RuntimeError("VortexPlan is closed.")
        counts = np.ascontiguousarray(np.asarray(counts).reshape(-1), dtype=np.int64)
        total = int(counts.sum()) if len(counts) and counts.min() >= 0 else 0
        xy = f64(np.asarray(xy, dtype=float).reshape(-1, 2))
        charges = i32(np.asarray(charges).reshape(-1))
        if counts.min(initial=0) >= 0 and (len(xy) != total or len(charges) != total):
            raise ValueError(f"Expected xy [{total}, 2] and charges [{total}] for these counts (got {xy.shape}, {charges.shape}).")
        out = [np.full(total, -1, dtype=np.int32) for _ in range(5)] + [np.full(total, np.inf)]
        _lib.check(self._lib.tdgl_vortex_plan_link(self._plan, len(counts), p_i64(counts), p_f64(xy), p_i32(charges),
                                                   float(max_distance), *[p_i32(a) for a in out[:5]], p_f64(out[5])))
        return tuple(out)

    def link_stats(self) -> dict:
        """Of the last :meth:`link`: links made, frames, pairs of points evaluated, kernel launches, and the device time
        in milliseconds between the upload of the records and the read-back.  :meth:`stats` stays that of the last find."""
        out, ms = (C.c_int64 * 4)(), C.c_double(0)
        _lib.check(self._lib.tdgl_vortex_plan_link_stats(self._plan, out, C.byref(ms)))
        return dict(links=out[0], frames=out[1], pairs=out[2], launches=out[3], last_ms=ms.value)

    def close(self):
        if getattr(self, "_plan", None) is not None and self._plan.value:
            self._lib.tdgl_vortex_plan_destroy(self._plan)
            self._plan = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_sample_locate(sites_xy, elements, points_xy):
    """``tdgl_host_sample_locate``: ``(triangle [m] int32, weights [m, 3])`` of the points on the triangulation, on the
    host (no GPU needed): the lowest-numbered triangle whose barycentric coordinates are all >= -1e-12, or -1."""
    sites_xy, points_xy = f64(sites_xy), f64(np.asarray(points_xy, dtype=float).reshape(-1, 2))
    elements = i32(np.asarray(elements).reshape(-1, 3))
    if sites_xy.ndim != 2 or sites_xy.shape[1] != 2:
        raise ValueError(f"Expected sites [n, 2] (got {sites_xy.shape}).")
    triangle = np.empty(len(points_xy), dtype=np.int32)
    weights = np.empty((len(points_xy), 3))
    _lib.check(_lib.load().tdgl_host_sample_locate(len(sites_xy), p_f64(sites_xy), len(elements), p_i32(elements),
                                                   len(points_xy), p_f64(points_xy), p_i32(triangle), p_f64(weights)))
    return triangle, weights


class SamplePlan:
    """Owns one ``tdgl_sample_plan`` (csrc/sample.inc): the sites, the edges with their unit directions, the triangles
    and ``m`` fixed points (located once, at construction) kept on the device; :meth:`eval` returns, for a batch of
    frames, the edge -> site densities, their values and psi's at the points and the dipole moments.  ``weights`` [n] with
    ``centre`` (x, y) enable the moments.  No physical prefactor.  Needs no ``TDGLContext``.  A context manager; freed on
    ``__del__`` too."""

    def __init__(self, sites_xy, edges, edge_dir, elements, points_xy=None, weights=None, centre=None, device_id=0):
        _lib.require_gpu()
        self._lib = _lib.load()
        self._plan = C.c_void_p()
        sites_xy = f64(sites_xy)
        if sites_xy.ndim != 2 or sites_xy.shape[1] != 2:
            raise ValueError(f"Expected sites [n, 2] (got {sites_xy.shape}).")
        edges = i32(np.asarray(edges).reshape(-1, 2))
        edge_dir = f64(edge_dir)
        if edge_dir.shape != (len(edges), 2):
            raise ValueError(f"Expected edge directions [{len(edges)}, 2] (got {edge_dir.shape}).")
        elements = i32(np.asarray(elements).reshape(-1, 3))
        points_xy = np.zeros((0, 2)) if points_xy is None else f64(np.asarray(points_xy, dtype=float).reshape(-1, 2))
        if (weights is None) != (centre is None):
            raise ValueError("weights and centre go together (both or neither).")
        if weights is not None:
            weights, centre = f64(weights), f64(centre)
            if weights.shape != (len(sites_xy),) or centre.shape != (2,):
                raise ValueError(f"Expected weights [{len(sites_xy)}] and centre [2] (got {weights.shape}, {centre.shape}).")
        self.n, self.n_edges, self.n_tri, self.m = len(sites_xy), len(edges), len(elements), len(points_xy)
        self.has_weights = weights is not None
        _lib.check(self._lib.tdgl_sample_plan_create(
            C.byref(self._plan), int(device_id), self.n, p_f64(sites_xy), p_f64(weights), p_f64(centre), self.n_edges,
            p_i32(edges), p_f64(edge_dir), self.n_tri, p_i32(elements), self.m, p_f64(points_xy)))

    def _open(self):
        if not self._plan.value:
            raise RuntimeError("SamplePlan is closed.")

    def location(self):
        """``(triangle [m] int32, weights [m, 3])`` of the plan's points: -1 and zeros where a point is in no triangle."""
        self._open()
        triangle = np.empty(self.m, dtype=np.int32)
        weights = np.empty((self.m, 3))
        _lib.check(self._lib.tdgl_sample_plan_location(self._plan, p_i32(triangle), p_f64(weights)))
        return triangle, weights

    def eval(self, edge_values=None, psi=None, site_density=False, point_density=False, point_psi=False, moment=False):
        """``edge_values``: [F, n_fields, n_edges] (``n_fields`` 1 or 2) or None; ``psi``: [F, n] complex or None.
        Returns ``(site_density [F, n_fields, n, 2], point_density [F, n_fields, m, 2], point_psi [F, m] complex,
        moment [F, n_fields])``, ``None`` for what is not asked for."""
        self._open()
        frames = None
        if edge_values is not None:
            edge_values = f64(edge_values)
            if edge_values.ndim != 3 or edge_values.shape[2] != self.n_edges:
                raise ValueError(f"Expected edge values of shape [n_frames, n_fields, {self.n_edges}] (got {edge_values.shape}).")
            frames = len(edge_values)
        if psi is not None:
            psi = c128(psi)
            if psi.ndim != 2 or psi.shape[1] != self.n or frames not in (None, len(psi)):
                raise ValueError(f"Expected psi of shape [n_frames, {self.n}] (got {psi.shape}).")
            frames = len(psi)
        if frames is None:
            raise ValueError("Expected edge values, psi or both.")
        nf = 0 if edge_values is None else edge_values.shape[1]
        out_site = np.empty((frames, nf, self.n, 2)) if site_density else None
        out_point = np.empty((frames, nf, self.m, 2)) if point_density else None
        out_psi = np.empty((frames, self.m), dtype=np.complex128) if point_psi else None
        out_moment = np.empty((frames, nf)) if moment else None
        _lib.check(self._lib.tdgl_sample_plan_eval(self._plan, frames, nf, p_f64(edge_values), p_f64(psi), p_f64(out_site),
                                                   p_f64(out_point), p_f64(out_psi), p_f64(out_moment)))
        return out_site, out_point, out_psi, out_moment

    def stats(self) -> dict:
        """Of the last call: points located in a triangle, frames, chunks of frames, kernel launches, and the device
        time in milliseconds between the uploads and the read-backs."""
        out, ms = (C.c_int64 * 4)(), C.c_double(0)
        _lib.check(self._lib.tdgl_sample_plan_stats(self._plan, out, C.byref(ms)))
        return dict(located=out[0], frames=out[1], chunks=out[2], launches=out[3], last_ms=ms.value)

    def close(self):
        if getattr(self, "_plan", None) is not None and self._plan.value:
            self._lib.tdgl_sample_plan_destroy(self._plan)
            self._plan = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
