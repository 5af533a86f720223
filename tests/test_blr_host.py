"""The block low-rank compression of the preconditioner's top separator (dense.inc: blr_compress_block), on the host:
rank-revealing on exact low-rank blocks, within its tolerance on a smooth kernel, and it gives up where a block is not
compressible."""

import ctypes as C

import numpy as np

from tdgl_amd import _lib

B, KMAX = 128, 32


def _compress(A, tol, kmax=KMAX):
    lib = _lib.load()
    A = np.ascontiguousarray(A, dtype=np.float64)
    Q, W = np.zeros(kmax * B), np.zeros(kmax * B)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    k = lib.tdgl_host_blr_compress(f(A), B, tol, kmax, f(Q), f(W))
    if k < 0:
        return k, None, None
    return k, Q[: k * B].reshape(k, B).T, W[: k * B].reshape(k, B).T


def test_exact_low_rank_block_is_found_at_its_rank():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((B, 5)) @ rng.standard_normal((5, B))
    k, Q, W = _compress(A, 1e-9 * np.linalg.norm(A, 2))
    assert k == 5
    assert np.allclose(Q.T @ Q, np.eye(k), atol=1e-13)
    assert np.linalg.norm(Q @ W.T - A, 2) <= 1e-9 * np.linalg.norm(A, 2)


def test_smooth_kernel_block_meets_its_tolerance():
    # two separated pieces of a curve, log kernel: what an off-diagonal block of a separator's Green's function looks like
    s = np.linspace(0.0, 1.0, B)
    x, y = np.stack([s, 0 * s], 1), np.stack([2.5 + s, 0.3 + 0.2 * s], 1)
    A = -np.log(np.linalg.norm(x[:, None, :] - y[None, :, :], axis=2))
    for tau in (1e-6, 1e-8):
        tol = tau * np.linalg.norm(A, 2)
        k, Q, W = _compress(A, tol)
        sv = np.linalg.svd(A, compute_uv=False)
        assert 0 < k <= KMAX and k >= int((sv > tol).sum())
        assert np.linalg.norm(Q @ W.T - A, 2) <= tol


def test_incompressible_block_stays_dense():
    A = np.random.default_rng(2).standard_normal((B, B))
    assert _compress(A, 1e-6 * np.linalg.norm(A, 2))[0] == -1


def test_zero_block_has_rank_zero():
    assert _compress(np.zeros((B, B)), 1e-12)[0] == 0
