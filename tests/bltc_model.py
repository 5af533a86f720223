"""Host model of the screening treecode (test infrastructure; NumPy).

It restates, with NumPy arithmetic, exactly the barycentric Lagrange treecode the HIP library runs for
``screening_method="tree"`` (`py-tdgl_amd/csrc/screening_tree.inc`, DESIGN.md §3 "Screening"):

* a source tree over the sites, split at the midpoint of tight bounding boxes (in two along each axis, or along
  the long axis only when the aspect ratio exceeds sqrt(2)), leaves of at most (p + 1)^2 sites;
* target batches over the edge centres, leaves of at most 64, split along the long axis only;
* proxy charges on (p + 1)^2 Chebyshev points of the second kind per cluster: the leaves from their sources,
  every parent from its children through the transfer matrices;
* one interaction list per batch from the acceptance test (r_cluster + r_batch) < theta |c_cluster - c_batch|.

The trees and the lists are built with the same floating-point operations as the C++ set-up, so the model takes
the same decisions, and its result agrees with the kernels' to round-off.  `tests/test_screening_tree_host.py`
checks it against the float64 direct sum; `tests/test_hip_screening_tree.py` checks the kernels against it.
"""

import math

import numpy as np

BATCH = 64


def build_tree(x, y, leaf_max, quad):
    """Nodes (dicts: x0, x1, y0, y1, begin, end, level, child0, nchild, parent) and the point order ``idx``
    (tree position -> input index); every node is the contiguous range idx[begin:end]."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    idx = np.arange(len(x))
    nodes = [dict(begin=0, end=len(x), level=0, parent=-1)]
    sqrt2 = math.sqrt(2.0)
    stack = [0]
    while stack:
        i = stack.pop()
        nd = nodes[i]
        sl = idx[nd["begin"]:nd["end"]]
        xs, ys = x[sl], y[sl]
        x0, x1, y0, y1 = float(xs.min()), float(xs.max()), float(ys.min()), float(ys.max())
        nd.update(x0=x0, x1=x1, y0=y0, y1=y1, child0=-1, nchild=0)
        w, h = x1 - x0, y1 - y0
        if len(sl) <= leaf_max or (w == 0.0 and h == 0.0):
            continue
        if quad and not (w > sqrt2 * h) and not (h > sqrt2 * w):
            sx = sy = True
        else:
            sx = w >= h
            sy = not sx
        xm, ym = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
        code = ((xs >= xm) & sx).astype(np.int64) + 2 * ((ys >= ym) & sy).astype(np.int64)
        counts = np.bincount(code, minlength=4)
        if np.count_nonzero(counts) < 2:
            continue
        idx[nd["begin"]:nd["end"]] = sl[np.argsort(code, kind="stable")]
        c0, start = len(nodes), nd["begin"]
        for c in range(4):
            if counts[c]:
                nodes.append(dict(begin=start, end=start + int(counts[c]), level=nd["level"] + 1, parent=i))
                start += int(counts[c])
        nd["child0"], nd["nchild"] = c0, len(nodes) - c0
        stack.extend(range(len(nodes) - 1, c0 - 1, -1))  # depth first, children in order (as the C++ recursion)
    return nodes, idx


def chebyshev(a, b, P):
    """P Chebyshev points of the second kind over [a, b]."""
    return 0.5 * (a + b) + 0.5 * (b - a) * np.cos(np.pi * np.arange(P) / (P - 1))


def basis(x, s):
    """Barycentric Lagrange basis of the nodes s at the points x: [len(x), len(s)]."""
    P = len(s)
    wb = (-1.0) ** np.arange(P)
    wb[0] *= 0.5
    wb[-1] *= 0.5
    d = np.asarray(x, dtype=np.float64)[:, None] - s[None, :]
    hit = d == 0.0
    t = np.where(hit, 0.0, wb[None, :] / np.where(hit, 1.0, d))
    rows = np.flatnonzero(hit.any(axis=1))
    sums = t.sum(axis=1, keepdims=True)
    sums[rows] = 1.0
    L = t / sums
    if len(rows):
        L[rows] = 0.0
        L[rows, hit[rows].argmax(axis=1)] = 1.0
    return L


class Treecode:
    """The set-up for one (sites, edge centres, degree, theta); `evaluate` is one evaluation of the sum."""

    def __init__(self, sites, centers, degree, theta):
        self.sites = np.asarray(sites, dtype=np.float64)
        self.centers = np.asarray(centers, dtype=np.float64)
        self.P = P = int(degree) + 1
        self.PP = PP = P * P
        self.theta = float(theta)
        self.nodes, self.sperm = build_tree(self.sites[:, 0], self.sites[:, 1], PP, True)
        tnodes, self.tperm = build_tree(self.centers[:, 0], self.centers[:, 1], BATCH, False)
        nodes = self.nodes
        nn = len(nodes)
        self.px = np.array([chebyshev(nd["x0"], nd["x1"], P) for nd in nodes])
        self.py = np.array([chebyshev(nd["y0"], nd["y1"], P) for nd in nodes])
        self.levels = 1 + max(nd["level"] for nd in nodes)
        # transfer child -> parent: T[c][k', k] = L_parent,k'(p_child,k)
        self.tx, self.ty = np.zeros((nn, P, P)), np.zeros((nn, P, P))
        for c in range(1, nn):
            p = nodes[c]["parent"]
            self.tx[c] = basis(self.px[c], self.px[p]).T
            self.ty[c] = basis(self.py[c], self.py[p]).T
        cx = [0.5 * (nd["x0"] + nd["x1"]) for nd in nodes]
        cy = [0.5 * (nd["y0"] + nd["y1"]) for nd in nodes]
        wh = [(nd["x1"] - nd["x0"], nd["y1"] - nd["y0"]) for nd in nodes]
        rad = [0.5 * math.sqrt(w * w + h * h) for w, h in wh]
        self.batches = sorted((nd for nd in tnodes if nd["nchild"] == 0), key=lambda nd: nd["begin"])
        self.far, self.near = [], []
        self.far_pairs = self.near_pairs = 0
        for bt in self.batches:
            bx, by = 0.5 * (bt["x0"] + bt["x1"]), 0.5 * (bt["y0"] + bt["y1"])
            bw, bh = bt["x1"] - bt["x0"], bt["y1"] - bt["y0"]
            br = 0.5 * math.sqrt(bw * bw + bh * bh)
            far, near, stack = [], [], [0]
            while stack:
                c = stack.pop()
                nd = nodes[c]
                dx, dy = cx[c] - bx, cy[c] - by
                accept = (rad[c] + br) < self.theta * math.sqrt(dx * dx + dy * dy)
                if accept and nd["end"] - nd["begin"] > PP:
                    far.append(c)
                elif accept or nd["nchild"] == 0:
                    if near and near[-1][1] == nd["begin"]:
                        near[-1][1] = nd["end"]
                    else:
                        near.append([nd["begin"], nd["end"]])
                else:
                    stack.extend(range(nd["child0"] + nd["nchild"] - 1, nd["child0"] - 1, -1))
            nt = bt["end"] - bt["begin"]
            self.far.append(np.array(far, dtype=np.int64))
            self.near.append(near)
            self.far_pairs += nt * len(far) * PP
            self.near_pairs += nt * sum(b - a for a, b in near)

    def stats(self):
        return dict(clusters=len(self.nodes), levels=self.levels, batches=len(self.batches),
                    far_pairs=self.far_pairs, near_pairs=self.near_pairs)

    def charges(self, w):
        """Proxy charges [n_nodes, P, P, 2] for the site weights w [n_sites, 2] (site order)."""
        P, nodes = self.P, self.nodes
        ws, xs = np.asarray(w, dtype=np.float64)[self.sperm], self.sites[self.sperm]
        q = np.zeros((len(nodes), P, P, 2))
        for i, nd in enumerate(nodes):
            if nd["nchild"] == 0:
                b, e = nd["begin"], nd["end"]
                Lx, Ly = basis(xs[b:e, 0], self.px[i]), basis(xs[b:e, 1], self.py[i])
                q[i] = np.einsum("jk,jl,jc->klc", Lx, Ly, ws[b:e])
        for lv in range(self.levels - 1, -1, -1):
            for i, nd in enumerate(nodes):
                if nd["level"] == lv and nd["nchild"] > 0:
                    for c in range(nd["child0"], nd["child0"] + nd["nchild"]):
                        q[i] += np.einsum("ak,klc,bl->abc", self.tx[c], q[c], self.ty[c])
        return q

    def evaluate(self, w):
        """A [n_edges, 2] (edge order of ``centers``) = sum_j w_j / |r_e - r_j| through the treecode."""
        P = self.P
        q = self.charges(w)
        ws, xs = np.asarray(w, dtype=np.float64)[self.sperm], self.sites[self.sperm]
        A = np.zeros((len(self.centers), 2))
        gx = np.repeat(self.px[:, :, None], P, axis=2)  # proxy (k, l) at (px[k], py[l])
        gy = np.repeat(self.py[:, None, :], P, axis=1)
        for bt, far, near in zip(self.batches, self.far, self.near):
            tg = self.tperm[bt["begin"]:bt["end"]]
            tx, ty = self.centers[tg, 0][:, None], self.centers[tg, 1][:, None]
            acc = np.zeros((len(tg), 2))
            if len(far):
                X, Y = gx[far].reshape(-1), gy[far].reshape(-1)
                acc += (1.0 / np.sqrt((tx - X) ** 2 + (ty - Y) ** 2)) @ q[far].reshape(-1, 2)
            if near:
                j = np.concatenate([np.arange(a, b) for a, b in near])
                acc += (1.0 / np.sqrt((tx - xs[j, 0]) ** 2 + (ty - xs[j, 1]) ** 2)) @ ws[j]
            A[tg] = acc
        return A


def direct_sum(sites, centers, w, rows=None, chunk=1024):
    """The float64 all-pairs sum on the edge centres ``rows`` (all by default): A [k, 2] and sum_j |w_j| / r [k, 2]."""
    rows = np.arange(len(centers)) if rows is None else np.asarray(rows)
    w = np.asarray(w, dtype=np.float64)
    A, S = np.zeros((len(rows), 2)), np.zeros((len(rows), 2))
    for a in range(0, len(rows), chunk):
        c = centers[rows[a:a + chunk]]
        rinv = 1.0 / np.sqrt((c[:, 0:1] - sites[None, :, 0]) ** 2 + (c[:, 1:2] - sites[None, :, 1]) ** 2)
        A[a:a + chunk] = rinv @ w
        S[a:a + chunk] = rinv @ np.abs(w)
    return A, S


def site_weights(mesh, edge_current, areas):
    """area_j K_site[j] of an edge current: the site average of Mesh.get_quantity_on_site, which
    `tdgl_induced_vector_potential` forms on the device."""
    em = mesh.edge_mesh
    n = len(mesh.sites)
    unit = em.directions / np.linalg.norm(em.directions, axis=1)[:, None]
    verts = np.concatenate([em.edges[:, 0], em.edges[:, 1]])
    counts = np.bincount(verts, minlength=n)
    K = np.asarray(edge_current, dtype=np.float64)
    J = np.stack([np.bincount(verts, weights=np.tile(K * unit[:, k], 2), minlength=n) / counts / 2 for k in range(2)],
                 axis=1)
    return np.asarray(areas)[:, None] * J
