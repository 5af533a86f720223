"""A nested dissection whose part sizes the TEST chooses, and a float64 model of what the device stores of its factors:
for tests/test_prescribed_dissection_host.py and tests/test_hip_sub_prescribed.py.

The product's partitioner (`substructure.substructure_order*`: recursive coordinate bisection) gives parts of about one
size per mesh, so the branches the factor kernels take on the part size -- ``ld = round_up(np, 16)``, chunks of
``min(64, round_up(ceil(np / pieces), 16))`` rows, 8 rows per wavefront in chunks of 32, column loops of 64 or 128 with a
tail, 16 x 16 tiles up to 256 rows, ``up_R = ceil(np_max / 64)``, the 2,048 rows the lane form stages -- are hit by
accident or not at all.  `dissect` cuts parts of exactly the sizes it is given; `apply_levels` is the launch sequence of
the solve on the host, `rounded_to_storage` the factors as the fp32 form keeps them.
"""

import copy

import numpy as np
import scipy.sparse as sp

from tdgl_amd.substructure import schur_pinv

# the size lists of the tests (level 1 / 2 / 3): both sides of every multiple the kernels branch on
SIZES_MIXED = ([1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257],
               [1, 15, 16, 17, 63, 64, 65, 129],
               [16, 17, 64, 65])
SIZES_TILES = [1, 15, 16, 17, 33, 64, 65, 128, 129, 192, 193, 255, 256]  # level 1 of the all-tiles cases (every part <= 256)


def capped(sizes, cap):
    return [s for s in sizes if s <= cap]


# name -> (edge length of `helpers.synthetic_mesh`, the three size lists)
LAYOUTS = {
    "mixed": (60, SIZES_MIXED),  # 257 on level 1: whole blocks, the lane form
    "tiles256": (60, (SIZES_TILES, SIZES_MIXED[1], SIZES_MIXED[2])),  # every part <= 256: tiles, up_R = 4
    "tiles192": (60, (capped(SIZES_TILES, 192), SIZES_MIXED[1], SIZES_MIXED[2])),  # up_R = 3
    "tiles128": (60, (capped(SIZES_TILES, 128), SIZES_MIXED[1], SIZES_MIXED[2])),  # up_R = 2
    "tiles64": (60, (capped(SIZES_TILES, 64), SIZES_MIXED[1], SIZES_MIXED[2])),  # up_R = 1
    "lanes2048": (70, ([2048, 1, 2047], SIZES_MIXED[1], SIZES_MIXED[2])),  # the largest part the lane form stages
    "lanes2049": (70, ([2049, 1, 2047], SIZES_MIXED[1], SIZES_MIXED[2])),  # one row more: refused
}


def graph_of_edges(edges, n):
    """The site graph of a mesh's edge list as a symmetric CSR pattern."""
    i, j = np.asarray(edges)[:, 0], np.asarray(edges)[:, 1]
    one = np.ones(len(i))
    return (sp.coo_matrix((one, (i, j)), shape=(n, n)) + sp.coo_matrix((one, (j, i)), shape=(n, n))).tocsr()


def _sweep(graph, order, sizes):
    """One level: ``graph`` symmetric CSR on m nodes, ``order`` the nodes in sweep order.  Part p takes the next
    ``sizes[p % len(sizes)]`` nodes that are neither in a part nor in the separator; every still-free neighbour of those
    nodes then becomes separator; a last part that cannot be filled goes to the separator.  Returns (parts: list of node
    arrays in sweep order, separator: node array in sweep order)."""
    indptr, indices = graph.indptr, graph.indices
    m = graph.shape[0]
    FREE, PART, SEP = 0, 1, 2
    state = np.zeros(m, dtype=np.int8)
    parts, pos, p = [], 0, 0
    while True:
        want = int(sizes[p % len(sizes)])
        assert want >= 1
        taken = []
        while pos < m and len(taken) < want:
            v = int(order[pos])
            pos += 1
            if state[v] == FREE:
                taken.append(v)
        if len(taken) < want:  # (the sweep is at its end: what was collected is separator)
            state[taken] = SEP
            break
        taken = np.asarray(taken, dtype=np.int64)
        state[taken] = PART
        nb = np.concatenate([indices[indptr[v]:indptr[v + 1]] for v in taken])
        state[nb[state[nb] == FREE]] = SEP
        parts.append(taken)
        p += 1
    # (every node behind `pos` was visited or made separator; nodes never reached do not exist: pos == m here)
    sep = np.asarray([v for v in order if state[v] != PART], dtype=np.int64)
    return parts, sep


def dissect(A, xy, sizes_per_level):
    """``(perm, [ptr_1, ..., ptr_K])`` for K = len(sizes_per_level) in (1, 2, 3): level 1 on the graph of ``A`` (any
    symmetric sparse matrix on the sites, only its pattern is used), the sites swept in ``lexsort((y, x))`` order; level
    k + 1 on the Schur graph of level k's separator -- two separator sites adjacent if they are adjacent in level k's
    graph or touch a common part of level k --, swept by the same coordinates.  The sweep is monotone, so every cut
    edge ends in the separator (`substructure.build_substructure_levels` checks that itself).

    ``perm`` (internal -> site) lists the level-1 interiors part by part, then the level-2 parts, ..., then the top
    separator; the pointer arrays are absolute, int32, each starting where the previous one ends, like
    `substructure.substructure_order3` returns them."""
    K = len(sizes_per_level)
    assert K in (1, 2, 3)
    graph = sp.csr_matrix(A, copy=True)
    graph.data[:] = 1.0
    graph.setdiag(0.0)
    graph.eliminate_zeros()
    graph = ((graph + graph.T) > 0).astype(np.float64).tocsr()
    xy = np.asarray(xy, dtype=float)
    ids = np.arange(graph.shape[0], dtype=np.int64)  # the level's nodes as sites
    chunks, ptrs, offset = [], [], 0
    for k in range(K):
        order = np.lexsort((xy[ids, 1], xy[ids, 0]))
        parts, sep = _sweep(graph, order, sizes_per_level[k])
        assert parts, f"level {k + 1}: not a single part of {sizes_per_level[k][0]} sites fits"
        assert len(sep) >= 2, f"level {k + 1}: no separator"
        sizes = np.array([len(p) for p in parts], dtype=np.int64)
        ptrs.append((offset + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int32))
        offset += int(sizes.sum())
        chunks.extend(ids[p] for p in parts)
        if k < K - 1:  # the Schur graph of this level's separator
            m = graph.shape[0]
            part_of = np.full(m, -1, dtype=np.int64)
            for p, nodes in enumerate(parts):
                part_of[nodes] = p
            local = np.full(m, -1, dtype=np.int64)
            local[sep] = np.arange(len(sep))
            coo = graph.tocoo()
            ss = (local[coo.row] >= 0) & (local[coo.col] >= 0)
            sp_ = (local[coo.row] >= 0) & (part_of[coo.col] >= 0)
            touch = sp.coo_matrix((np.ones(int(sp_.sum())), (local[coo.row[sp_]], part_of[coo.col[sp_]])),
                                  shape=(len(sep), len(parts))).tocsr()
            nxt = sp.coo_matrix((np.ones(int(ss.sum())), (local[coo.row[ss]], local[coo.col[ss]])),
                                shape=(len(sep), len(sep))).tocsr() + touch @ touch.T
            nxt.setdiag(0.0)
            nxt.eliminate_zeros()
            graph = (nxt > 0).astype(np.float64).tocsr()
        ids = ids[sep]
    chunks.append(ids)  # the top separator
    perm = np.concatenate(chunks).astype(np.int32)
    assert len(perm) == len(xy)
    return perm, ptrs


def order_function(sizes_per_level):
    """A stand-in for `substructure.substructure_order` / `_order2` / `_order3` (by the number of levels): the product's
    arguments, the prescribed dissection's result -- for ``monkeypatch.setattr(tdgl_amd.substructure, ...)``."""
    def order(sites, edges, *blocks, rank_hint=None):
        sites = np.asarray(sites, dtype=float)
        perm, ptrs = dissect(graph_of_edges(edges, len(sites)), sites, sizes_per_level)
        return (perm, *ptrs)
    return order


def describe(levels):
    """Per level: the part sizes, the smallest / largest number of separator sites a part touches, the separator."""
    out = []
    for lv in levels:
        cnt = [len(s) for s in lv.sep_idx]
        out.append(dict(sizes=np.diff(lv.part_ptr).tolist(), touch=(min(cnt), max(cnt)), separator=int(lv.n_sep)))
    return out


def probe_positions(ptrs, n):
    """The probe columns' unit vectors, as positions in the dissection's order: the first and the last row of one part
    (the first) of every distinct size on every level, and the first and last position of every level's separator."""
    pos = []
    for ptr in ptrs:
        ptr = np.asarray(ptr, dtype=np.int64)
        sizes = np.diff(ptr)
        for s in np.unique(sizes):
            p = int(np.flatnonzero(sizes == s)[0])
            pos += [int(ptr[p]), int(ptr[p + 1]) - 1]
        pos += [int(ptr[-1]), n - 1]
    return np.array(sorted(set(pos)), dtype=np.int64)


def probe_columns(ptrs, n, seed=0, n_random=4):
    """``[n, k]`` in the dissection's order: the unit vectors of `probe_positions`, then ``n_random`` standard-normal
    columns."""
    pos = probe_positions(ptrs, n)
    B = np.zeros((n, len(pos) + n_random))
    B[pos, np.arange(len(pos))] = 1.0
    B[:, len(pos):] = np.random.default_rng(seed).standard_normal((n, n_random))
    return B


# ---- the float64 model ---------------------------------------------------------------------------------------------
def apply_levels(levels, G_top, b, sparse_sep=True):
    """The bare launch sequence of the substructured solve on ``b`` (in the dissection's order): ways down, ``G_top @
    r_S``, ways up, the mean from ``g`` and ``u`` -- what `substructure.solve_host_levels(levels, b, sparse_sep,
    remove_mean=False)` does, with the top separator's (pseudo-)inverse passed in (bit for bit the same with
    ``G_top = schur_pinv(levels[-1].schur)``).  ``b`` [n] or [n, k]."""
    n = levels[0].n
    vec = np.asarray(b, dtype=float)
    ys, total = [], 0.0
    for lv in levels:
        nI = lv.n_interior
        y = np.empty((nI,) + vec.shape[1:])
        r = vec[nI:].copy()
        for p in range(lv.n_parts):
            a, e = int(lv.part_ptr[p]), int(lv.part_ptr[p + 1])
            y[a:e] = lv.G[p] @ vec[a:e]
            if not sparse_sep:
                r[lv.sep_idx[p]] -= lv.E[p].T @ vec[a:e]
            total += lv.g[a:e] @ vec[a:e]
        if sparse_sep:
            r -= lv.coupling @ y
        ys.append(y)
        vec = r
    x = G_top @ vec
    total += levels[-1].u @ x
    for lv, y in zip(reversed(levels), reversed(ys)):
        full = np.empty((lv.n,) + x.shape[1:])
        for p in range(lv.n_parts):
            a, e = int(lv.part_ptr[p]), int(lv.part_ptr[p + 1])
            full[a:e] = y[a:e] - lv.E[p] @ x[lv.sep_idx[p]]
        full[lv.n_interior:] = x
        x = full
    return x - total / n


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def rounded_to_storage(levels, G_top):
    """``(levels, G_top)`` as `tdgl_poisson_set_substructure_precond(..., fp32_storage=1)` keeps them: exactly the arrays
    rounded to float32 that the device stores as float32 --

    * every level's value pool ``[1.0 | G_p | -E_p^T | g]`` (`k_sub_repack<float>` for the blocks, `k_to_float` for
      ``g``): ``G``, ``E`` and ``g``;
    * the top separator's inverse (`dense_to_fp32`).

    Float64 on the device, hence here: ``u`` (`SubLevel::u`), the sparse coupling blocks (`Csr::data`; the way down
    reads them with `launch_csr` on the fp64 values), every vector, every multiply-add and the sums of the mean."""
    out = []
    for lv in levels:
        c = copy.copy(lv)
        c.G = [_f32(G) for G in lv.G]
        c.E = [_f32(E) for E in lv.E]
        c.g = _f32(lv.g)
        out.append(c)
    return out, _f32(G_top)


def top_inverse(levels):
    return schur_pinv(levels[-1].schur)


def build_layout(name, K=3):
    """Everything the tests need of layout ``name`` cut to ``K`` levels, on the host: the mesh, its Poisson matrix in
    site order (``A``) and in the dissection's order (``A_d``), ``perm`` / ``iperm``, the pointer arrays, the float64
    factors (`substructure.build_substructure_levels`, what the product builds from the same dissection) and the top
    separator's pseudo-inverse."""
    from types import SimpleNamespace

    import dense_reference as D
    from helpers import synthetic_mesh
    from tdgl_amd import substructure
    from tdgl_amd.hipcore import poisson_matrix

    lx, lists = LAYOUTS[name]
    lists = tuple(lists[:K])
    mesh = synthetic_mesh(lx)
    n = len(mesh.sites)
    em = mesh.edge_mesh
    A = D.poisson_matrix_of(mesh)
    perm, ptrs = dissect(A, mesh.sites, lists)
    iperm = np.empty(n, dtype=np.int64)
    iperm[perm] = np.arange(n)
    A_d = poisson_matrix(em.edges.astype(np.int64), em.dual_edge_lengths / em.edge_lengths, n, iperm)
    levels = substructure.build_substructure_levels(A_d, ptrs)
    return SimpleNamespace(name=name, K=K, lists=lists, mesh=mesh, n=n, A=A, A_d=A_d, perm=perm, iperm=iperm, ptrs=ptrs,
                           levels=levels, G_top=top_inverse(levels))
