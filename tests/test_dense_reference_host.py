"""The float64 reference of tests/test_hip_dense_kernels.py on its own, without a GPU: the exact-size meshes, the refined
pseudo-inverse solve and its agreement with LAPACK's inverse under the kappa-derived tolerance."""

import numpy as np
import pytest

import dense_reference as D

SIZES = [3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 641]


@pytest.mark.parametrize("n", SIZES + [4097])
def test_mesh_with_sites_has_exactly_n_sites(n):
    mesh = D.mesh_with_sites(n)
    assert len(mesh.sites) == n and len(mesh.areas) == n
    assert np.all(mesh.areas > 0) and np.all(mesh.edge_mesh.dual_edge_lengths > 0)
    A = D.poisson_matrix_of(mesh)
    assert abs(A - A.T).max() == 0.0 and np.abs(A @ np.ones(n)).max() < 1e-12 * abs(A).max()


@pytest.mark.parametrize("n", [3, 5, 64, 129, 641])
def test_condition_number_matches_the_whole_spectrum(n):
    A = D.poisson_matrix_of(D.mesh_with_sites(n))
    ev = np.linalg.eigvalsh(A.toarray())
    assert abs(ev[0]) < 1e-12 * ev[-1] and ev[1] > 1e-6 * ev[-1]  # one null vector: the constants
    assert D.condition_number(A, D.pinv_reference(A)) == pytest.approx(ev[-1] / ev[1], rel=1e-5)


@pytest.mark.parametrize("n", SIZES + [4095, 4097])
def test_refined_reference_meets_its_residual_bound_and_agrees_with_lapack(n):
    mesh = D.mesh_with_sites(n)
    A = D.poisson_matrix_of(mesh)
    G = D.pinv_reference(A)
    kappa = D.condition_number(A, G)
    assert 0.3 * n < kappa < 0.6 * n + 5  # (a hex lattice: kappa grows like n)
    rng = np.random.default_rng(n)
    cols = np.arange(n) if n <= 700 else np.array([0, 63, 64, 127, 128, n - 129, n - 128, n - 1])
    E = np.zeros((n, len(cols)))
    E[cols, np.arange(len(cols))] = 1.0
    b = np.column_stack([E, D.rhs_to_b(mesh, rng.standard_normal((n, 8)))])
    b -= b.mean(axis=0)
    x = D.apply_reference(A, b, G)
    assert np.abs(x.mean(axis=0)).max() < 1e-15 * np.abs(x).max()
    res = np.abs(D._residual_ld(A, b, x)).max(axis=0).astype(float)
    for j in range(b.shape[1]):
        assert res[j] <= D.residual_bound(A, b[:, j], x[:, j]), j
    # LAPACK's inverse, applied without refinement, is a computed inverse like the device's: within the tolerance
    y = G @ b
    y -= y.mean(axis=0)
    assert np.all(np.abs(y - x).max(axis=0) <= D.tolerance(kappa, x)), (D.max_rel_error(y, x) / (kappa * D.U)).max()
