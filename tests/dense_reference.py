"""A float64 reference for the dense mu solve (the explicit pseudo-inverse G of the Poisson matrix), and meshes with an
exact number of sites, for tests/test_dense_reference_host.py and tests/test_hip_dense_kernels.py.

Conventions of the library (`TDGLContext.poisson_solve`, the time loop): A is the symmetric positive semi-definite
Poisson matrix (`hipcore.poisson_matrix`, null space = the constants), the solve is A mu = b with b = -areas * rhs
projected to zero mean, and mu is returned with zero mean.

Error model (the tolerance is derived, not fitted): an explicit inverse X of A computed in fp64 satisfies
||X A - I|| <= c kappa u (Gauss-Jordan / Cholesky-based inversion, Higham, Accuracy and Stability, ch. 14), so
X b - x = (X A - I) x is at most c kappa u |x| in size, and the product X b adds at most n u sum_j |X_ij| |b_j|, which
for these operators is of the order of u |x| (the smooth modes that dominate x are the ones G amplifies).  kappa is
the condition number of A on the complement of the constants, lambda_max(A) / lambda_2(A).  The reference applies
pinv(A) once more to the residual formed in extended precision, which leaves it within ~(kappa u)^2 + u of x: far
below the tolerance.
"""

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.sparse.csgraph import connected_components

from tdgl_amd.amg import exact_pinv
from tdgl_amd.finite_volume import Mesh
from tdgl_amd.hipcore import poisson_matrix
from tdgl_amd.meshgen import hex_jitter_points, triangulate

U = np.finfo(np.float64).eps / 2  # unit round-off of fp64
# c of the error model: small and fixed.  (LAPACK's inverse on the host, under the same model, reaches 1.9 kappa u at
# three sites -- where the product's own rounding is all there is -- and 0.2 to 1.4 kappa u from 63 to 8,193 sites;
# tests/test_dense_reference_host.py holds it to this bound.)
C_TOL = 8.0


def mesh_with_sites(n, seed=0):
    """A connected triangulated mesh with exactly ``n`` sites: the ``n`` points of a jittered hex lattice nearest to its
    centre, Delaunay-triangulated, without the long thin triangles that fill the concave steps of such a point set's
    convex hull (their circumcentres lie far outside, which would give a few cells huge areas and the matrix a
    condition number 100 x that of the lattice).  Every triangle kept is close to equilateral."""
    n = int(n)
    side = 2.0 * np.sqrt(n) + 4.0
    pts = hex_jitter_points(side, seed=seed)
    # (ties broken by the index: the lattice's jitter keeps the distances apart anyway)
    pts = pts[np.argsort(np.hypot(pts[:, 0], pts[:, 1]), kind="stable")[:n]]
    tri = triangulate(pts)
    p = pts[tri]
    longest = np.linalg.norm(p - np.roll(p, 1, axis=1), axis=2).max(axis=1)
    tri = tri[longest < 1.25 * np.median(longest)]
    p = pts[tri]
    area = 0.5 * ((p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1]))
    assert len(tri) >= 1 and np.all(np.abs(area) > 0.3), (n, seed, np.abs(area).min() if len(area) else None)
    assert len(np.unique(tri)) == n, (n, seed)  # every site is in a triangle that was kept
    mesh = Mesh.from_triangulation(pts, tri)
    assert len(mesh.sites) == n
    em = mesh.edge_mesh
    graph = sp.coo_matrix((np.ones(len(em.edges)), (em.edges[:, 0], em.edges[:, 1])), shape=(n, n))
    assert connected_components(graph, directed=False)[0] == 1, (n, seed)
    return mesh


def poisson_matrix_of(mesh):
    """The library's Poisson matrix in the mesh's own site order (CSR)."""
    em = mesh.edge_mesh
    return poisson_matrix(em.edges.astype(np.int64), em.dual_edge_lengths / em.edge_lengths, len(mesh.sites)).tocsr()


def pinv_reference(A):
    """pinv(A), float64, dense: LAPACK's inverse of A + J with J = 1 1^T / n, less J."""
    return exact_pinv(A)


def condition_number(A, G):
    """kappa = lambda_max(A) / lambda_2(A) on the complement of the constants: lambda_max of the sparse A and
    1 / lambda_2 = lambda_max of G = pinv(A) by Lanczos (the whole spectrum, ``eigvalsh``, costs as much as the inverse
    itself at a few thousand sites; tests/test_dense_reference_host.py checks the two agree)."""
    n = A.shape[0]
    if n <= 64:
        ev = np.linalg.eigvalsh(A.toarray())
        return float(ev[-1] / ev[1])
    lmax = spla.eigsh(A, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0]
    gmax = spla.eigsh(spla.aslinearoperator(G), k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0]
    return float(lmax * gmax)


def rhs_to_b(mesh, rhs):
    """The right-hand side the library solves for: b = -areas * rhs, projected to zero mean.  ``rhs`` [n] or [n, k]."""
    rhs = np.asarray(rhs, dtype=float)
    a = mesh.areas if rhs.ndim == 1 else mesh.areas[:, None]
    b = -a * rhs
    return b - b.mean(axis=0)


def _residual_ld(A, b, x):
    """b - A x with every product and sum in np.longdouble, from the sparse A; x, b [n] or [n, k]."""
    A = A.tocsr()
    data = A.data.astype(np.longdouble)
    xl = np.asarray(x).astype(np.longdouble)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    prods = data[:, None] * xl.reshape(len(xl), -1)[A.indices]
    Ax = np.zeros((A.shape[0], prods.shape[1]), dtype=np.longdouble)
    np.add.at(Ax, rows, prods)
    return np.asarray(b).astype(np.longdouble).reshape(Ax.shape) - Ax


def apply_reference(A, b, G=None):
    """x = pinv(A) b (b zero-mean, [n] or [n, k]), refined once: x0 = G b, x = x0 + G r with r = b - A x0 formed in
    extended precision; returned with zero mean like the library's mu."""
    G = pinv_reference(A) if G is None else G
    b = np.asarray(b, dtype=float)
    x0 = G @ b
    r = _residual_ld(A, b, x0).astype(np.float64).reshape(b.shape)
    x = x0 + G @ r
    return x - x.mean(axis=0)


def residual_bound(A, b, x):
    """What a backward-stable x leaves: the componentwise bound C_TOL u (|A| |x| + |b|) of |b - A x|, largest entry."""
    absAx = abs(A) @ np.abs(x)
    return C_TOL * U * float(np.max(absAx + np.abs(b)))


def tolerance(kappa, x_ref):
    """Largest admissible |mu - x_ref| of a computed inverse's solve, per column: C_TOL kappa u max|x_ref|."""
    x_ref = np.asarray(x_ref)
    return C_TOL * kappa * U * np.abs(x_ref).max(axis=0)


def max_rel_error(x, x_ref):
    """max |x - x_ref| / max |x_ref|, per column (the quantity the tolerance bounds, in units of max |x_ref|)."""
    x, x_ref = np.asarray(x), np.asarray(x_ref)
    return np.abs(x - x_ref).max(axis=0) / np.abs(x_ref).max(axis=0)
