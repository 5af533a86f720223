"""Float64 host model of SINGLE ranks of the rank-level nested dissection (tdgl_amd/schur_dd.py, csrc/schur.inc), without
a process group: for tests/test_schur_rank_host.py and tests/test_hip_schur_rank.py (test infrastructure; NumPy + SciPy).

The rank-local halves of one application (``solve(b)`` applies ``A_II^-1`` to ``b`` [n_I] or [n_I, k]):

    schur_share            A_GG_owned - A_GI A_II^-1 A_IG on the block of interface sites the rank's interior touches
    interior_solve         y_I = A_II^-1 r_I
    interface_share        t_r = r_G (owned interface rows) - A_GI y_I: the rank's term of the ONE sum of an application
    result_from_interface  z on the owned rows from x_G = S^+ sum_r t_r: x_I = y_I - A_II^-1 (A_IG x_G), x_G copied

`dist_model.schur_setup_dist` / `schur_apply_dist` are the gloo wrapper around them (SciPy's LU as ``solve``).  `Ranks`
holds every rank's pieces for one mesh and plays any subset of the ranks: all of them (the CPU test), or all but the one
a device runs (the GPU test, inside the all-reduce callback).  Its local solves are the launch sequence of the device
(`prescribed_dissection.apply_levels` on the gauge-free factors, a plain inverse on the top separator), with the factors
exact or rounded to what the device stores as fp32 (`prescribed_dissection.rounded_to_storage`, and ``S^+``); coupling
blocks, vectors and sums stay float64, as on the device.
"""

import contextlib
from types import SimpleNamespace

import numpy as np
import scipy.sparse.linalg as spla

import dense_reference as D
import prescribed_dissection as P


# name -> (mesh lx, ly, world, blocks of `schur_dd.local_dissection`, prescribed size lists or None, local levels, |Gamma|,
# {rank: (owned, touched) interface sites}): the shapes both tests assert before they rely on them
CASES = {
    "a": (40, 30, 3, (16, 80, 300), None, 2, 70, {0: (35, 35), 1: (35, 46), 2: (0, 52)}),
    "b": (60, 50, 3, (16, 80, 300), None, 3, 99, {1: (41, 69), 2: (0, 70)}),
    "c": (40, 30, 3, (60, 500, 3000), None, 1, 70, {1: (35, 46)}),
    "d": (70, 60, 2, (16, 80, 300), P.SIZES_MIXED, 3, 70, {0: (70, 70), 1: (0, None)}),
}


def build_case(name):
    lx, ly, world, blocks, lists = CASES[name][:5]
    return Ranks(lx, ly, world, blocks, lists)


# ---- the rank-local halves -----------------------------------------------------------------------------------------
def touched_sites(piece):
    """Positions in Gamma of the interface sites the rank's interior has an edge to."""
    return np.unique(piece.A_IG.indices)


def complement_share(piece, solve):
    """``C = A_GI A_II^-1 A_IG`` [n_gamma, n_gamma], zero outside the touched block."""
    touched = touched_sites(piece)
    X = solve(piece.A_IG[:, touched].toarray())
    out = np.zeros((piece.n_gamma, piece.n_gamma))
    out[np.ix_(touched, touched)] = piece.A_GI[touched] @ X
    return out


def schur_share(piece, solve):
    """The rank's term of ``S = A_GG - sum_r A_GI_r A_II_r^-1 A_I_rG``."""
    touched = touched_sites(piece)
    X = solve(piece.A_IG[:, touched].toarray())
    S = piece.A_GG_owned.toarray()
    S[np.ix_(touched, touched)] -= piece.A_GI[touched] @ X
    return S


def interior_solve(piece, solve, r_own):
    """``y_I = A_II^-1 r_I``; ``r_own`` [n_own] or [n_own, k] in the rank's local order (interior ids are owned ids)."""
    return solve(np.asarray(r_own, dtype=float)[piece.interior])


def interface_share(piece, r_own, y):
    r_own = np.asarray(r_own, dtype=float)
    t = np.zeros((piece.n_gamma,) + r_own.shape[1:])
    t[piece.gamma_owned_gid] = r_own[piece.gamma_owned_local]
    t -= piece.A_GI @ y
    return t


def result_from_interface(piece, solve, n_own, y, xg):
    xi = y - solve(piece.A_IG @ xg)
    z = np.zeros((n_own,) + xi.shape[1:])
    z[piece.interior] = xi
    z[piece.gamma_owned_local] = xg[piece.gamma_owned_gid]
    return z


# ---- every rank of one mesh ----------------------------------------------------------------------------------------
@contextlib.contextmanager
def prescribed_orders(lists):
    """The product's three dissection functions replaced by `prescribed_dissection.order_function(lists[:k])` while the
    pieces are cut (`schur_dd.local_dissection` looks them up when called); ``lists`` None: the product's own."""
    from tdgl_amd import substructure

    names = ("substructure_order", "substructure_order2", "substructure_order3")
    saved = [getattr(substructure, f) for f in names]
    try:
        if lists is not None:
            for k, f in enumerate(names):
                setattr(substructure, f, P.order_function(lists[:k + 1]))
        yield
    finally:
        for f, fn in zip(names, saved):
            setattr(substructure, f, fn)


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def condition_number_spd(A):
    """lambda_max / lambda_min of a sparse positive definite matrix, by Lanczos on A and on its LU solve (as
    `dense_reference.condition_number` does with the pseudo-inverse)."""
    n = A.shape[0]
    lu = spla.splu(A.tocsc())
    lmax = spla.eigsh(A, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0]
    inv = spla.LinearOperator((n, n), matvec=lu.solve, dtype=np.float64)
    gmax = spla.eigsh(inv, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0]
    return float(lmax * gmax)


class Ranks:
    """The global mesh cut ``world`` ways: `rcb_partition`, `interface_cover`, `gamma_numbering`, every rank's
    `LocalProblem` and `SchurPiece`, the float64 factors of every rank's interior (gauge-free) and the interface's
    pseudo-inverse -- exact and as stored in fp32."""

    def __init__(self, lx, ly, world, blocks, lists=None):
        from helpers import synthetic_mesh
        from tdgl_amd import substructure
        from tdgl_amd.partition import build_local_problem, rcb_partition
        from tdgl_amd.schur_dd import build_piece, gamma_numbering, interface_cover, interface_pinv

        self.mesh = mesh = synthetic_mesh(lx, ly)
        self.n = n = len(mesh.sites)
        self.world = int(world)
        self.A = D.poisson_matrix_of(mesh)
        self.part = rcb_partition(mesh.sites, self.world)
        self.is_gamma = interface_cover(mesh.edge_mesh.edges, self.part)
        self.gid, self.n_gamma = gamma_numbering(self.is_gamma)
        self.gamma_sites = np.flatnonzero(self.is_gamma)  # global site of every position in Gamma
        self.ranks = []
        with prescribed_orders(lists):
            for r in range(self.world):
                lp = build_local_problem(mesh, self.part, r)
                l2g = lp.local_to_global
                piece = build_piece(lp, self.is_gamma[l2g], self.gid[l2g], self.n_gamma, blocks=blocks)
                levels = substructure.build_substructure_levels(piece.A_II, piece.ptrs, gauge=False)
                G_top = np.linalg.inv(levels[-1].schur)
                self.ranks.append(SimpleNamespace(rank=r, lp=lp, piece=piece, own=l2g[: lp.n_own], levels=levels, G_top=G_top,
                                                  rounded=P.rounded_to_storage(levels, G_top), touched=touched_sites(piece)))
        self.S = sum(self.schur_share(r) for r in range(self.world))
        self.Spinv = interface_pinv(self.S)
        self.Spinv32 = _f32(self.Spinv)

    # -- one rank ------------------------------------------------------------------------------------------------------
    def solve(self, r, rounded=False):
        """``b -> A_II^-1 b`` of rank ``r`` by the device's launch sequence, with exact or fp32-stored factors."""
        m = self.ranks[r]
        levels, G_top = m.rounded if rounded else (m.levels, m.G_top)
        return lambda b: P.apply_levels(levels, G_top, b)

    def complement_share(self, r):
        return complement_share(self.ranks[r].piece, self.solve(r))

    def schur_share(self, r):
        """(With the fp64 factors: the complement is formed before the factors are converted.)"""
        return schur_share(self.ranks[r].piece, self.solve(r))

    def own_rows(self, r, R):
        """The rows of the global ``R`` [n] or [n, k] rank ``r`` owns, in its local order."""
        return np.asarray(R, dtype=float)[self.ranks[r].own]

    def interface_share(self, r, R, rounded=False):
        """``(y_I, t_r)`` of rank ``r`` for the global residual(s) ``R``."""
        m = self.ranks[r]
        r_own = self.own_rows(r, R)
        y = interior_solve(m.piece, self.solve(r, rounded), r_own)
        return y, interface_share(m.piece, r_own, y)

    def others_share(self, r, R, rounded=False):
        """``sum_{s != r} t_s``: what the other ranks add to rank ``r``'s buffer in the all-reduce, in rank order."""
        t = np.zeros((self.n_gamma,) + np.shape(R)[1:])
        for s in range(self.world):
            if s != r:
                t += self.interface_share(s, R, rounded)[1]
        return t

    def apply_rank(self, r, R, rounded=False):
        """One application as rank ``r`` sees it: ``(t_r, z_own)`` with every rank played by the model."""
        return self.interface_share(r, R, rounded)[1], self.apply(R, rounded)[self.ranks[r].own]

    # -- all ranks -----------------------------------------------------------------------------------------------------
    def apply(self, R, rounded=False):
        """``M R`` on the global site vector(s) ``R``, every rank played by the model (the sum in rank order)."""
        R = np.asarray(R, dtype=float)
        ys, t = [], np.zeros((self.n_gamma,) + R.shape[1:])
        for r in range(self.world):
            y, t_r = self.interface_share(r, R, rounded)
            ys.append(y)
            t += t_r
        xg = (self.Spinv32 if rounded else self.Spinv) @ t
        Z = np.zeros(R.shape)
        for r, m in enumerate(self.ranks):
            Z[m.own] = result_from_interface(m.piece, self.solve(r, rounded), m.lp.n_own, ys[r], xg)
        return Z

    def describe(self, r):
        """The shape facts of rank ``r`` a case relies on."""
        m = self.ranks[r]
        return dict(levels=len(m.piece.ptrs), interior=int(m.piece.n_interior), owned_interface=int(len(m.piece.gamma_owned_gid)),
                    touched_interface=int(len(m.touched)), top_separator=int(m.levels[-1].n_sep),
                    part_sizes=[sorted(set(np.diff(p).tolist())) for p in m.piece.ptrs])

    # -- probe columns -------------------------------------------------------------------------------------------------
    def probe_columns(self, r, seed=0, n_random=4):
        """Global zero-mean columns ``[n, k]`` for device rank ``r`` and what each is: ``e_i - 1 / n`` for the first and
        the last row of one part of every distinct size on every local level and of every local separator
        (`prescribed_dissection.probe_positions` through ``piece.interior``), for an interface site the rank owns, one
        it touches but does not own, a site in another rank's interior; then ``n_random`` standard-normal columns."""
        m = self.ranks[r]
        l2g = m.lp.local_to_global
        sites = [(int(l2g[m.piece.interior[p]]), "interior") for p in P.probe_positions(m.piece.ptrs, m.piece.n_interior)]
        if len(m.piece.gamma_owned_gid):
            own_touched = np.intersect1d(m.piece.gamma_owned_gid, m.touched)
            g = own_touched[len(own_touched) // 2] if len(own_touched) else m.piece.gamma_owned_gid[0]
            sites.append((int(self.gamma_sites[g]), "interface, owned"))
        foreign = np.setdiff1d(m.touched, m.piece.gamma_owned_gid)
        if len(foreign):
            sites.append((int(self.gamma_sites[foreign[len(foreign) // 2]]), "interface, touched and not owned"))
        other = self.ranks[(r + 1) % self.world]
        sites.append((int(other.lp.local_to_global[other.piece.interior[other.piece.n_interior // 2]]), "another rank's interior"))
        B = np.full((self.n, len(sites) + n_random), -1.0 / self.n)
        B[[s for s, _ in sites], np.arange(len(sites))] += 1.0
        rnd = np.random.default_rng(seed).standard_normal((self.n, n_random))
        B[:, len(sites):] = rnd - rnd.mean(axis=0)
        return B, [w for _, w in sites] + ["random"] * n_random


def storage_error(z_rounded, z_exact):
    """``s`` per column: max |rounded model - exact model| / max |exact model|."""
    return np.abs(z_rounded - z_exact).max(axis=0) / np.abs(z_exact).max(axis=0)
