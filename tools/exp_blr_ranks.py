"""Ranks of the off-diagonal blocks of the preconditioner's top separator inverse (CPU, no GPU): the mesh of bench.py's
film of side `side`, the dissection and factors as the library builds them (`substructure_order3` with
`TDGLContext.PD_BLOCKS`, `build_substructure_levels`), `schur_pinv` of the top separator's complement, then the SVD of
every off-diagonal block pair of B x B at every tau (singular values below tau * ||G||_2 dropped; a block whose rank
exceeds B / 4 stays dense).  Reports the storage (fp32, diagonal blocks as symmetric halves), the rank statistics and,
per tau, ||(G~ - G) x|| / ||G x|| for random x of mean zero.

    python tools/exp_blr_ranks.py [side=930] [B=128] [tau ...]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "py-tdgl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
from helpers import synthetic_mesh  # noqa: E402
from tdgl_amd.hipcore import TDGLContext, poisson_matrix  # noqa: E402
from tdgl_amd.substructure import build_substructure_levels, schur_pinv, substructure_order3  # noqa: E402

side = float(sys.argv[1]) if len(sys.argv) > 1 else 930.0
B = int(sys.argv[2]) if len(sys.argv) > 2 else 128
taus = [float(t) for t in sys.argv[3:]] or [1e-6, 1e-7, 1e-8]
t0 = time.perf_counter()
mesh = synthetic_mesh(side)
em = mesh.edge_mesh
n = len(mesh.sites)
perm, p1, p2, p3 = substructure_order3(np.asarray(mesh.sites), em.edges, *TDGLContext.PD_BLOCKS)
iperm = np.empty(n, dtype=np.int64)
iperm[perm] = np.arange(n)
A = poisson_matrix(em.edges.astype(np.int64), em.dual_edge_lengths / em.edge_lengths, n, iperm)
levels = build_substructure_levels(A, [p1, p2, p3])
G = schur_pinv(levels[-1].schur)
m = G.shape[0]
norm = np.linalg.norm(G, 2)
nb = (m + B - 1) // B
print(json.dumps(dict(sites=n, top_separator=m, blocks_per_side=nb, norm=float(norm), setup_s=round(time.perf_counter() - t0, 1))), flush=True)
sv = {}
for I in range(nb):
    for J in range(I):
        blk = G[I * B:(I + 1) * B, J * B:(J + 1) * B]
        u, s, vt = np.linalg.svd(blk, full_matrices=False)
        sv[I, J] = (u, s, vt)
rng = np.random.default_rng(0)
X = rng.standard_normal((m, 4))
X -= X.mean(0)
GX = G @ X
diag_bytes = sum(4 * (min(B, m - I * B) * (min(B, m - I * B) + 1) // 2) for I in range(nb))
for tau in taus:
    tol = tau * norm
    ranks, nbytes, Gt = [], diag_bytes, G.copy()
    for (I, J), (u, s, vt) in sv.items():
        r = int((s > tol).sum())
        bi, bj = u.shape[0], vt.shape[1]
        if r > B // 4:
            nbytes += 4 * bi * bj
            continue
        ranks.append(r)
        nbytes += 4 * r * (bi + bj)
        approx = (u[:, :r] * s[:r]) @ vt[:r]
        Gt[I * B:I * B + bi, J * B:J * B + bj] = approx
        Gt[J * B:J * B + bj, I * B:I * B + bi] = approx.T
    err = np.linalg.norm(Gt @ X - GX, axis=0) / np.linalg.norm(GX, axis=0)
    rk = np.array(ranks) if ranks else np.zeros(1)
    print(json.dumps(dict(B=B, tau=tau, storage_MB=round(nbytes / 1e6, 1), dense_MB=round(4 * m * (m + 1) / 2 / 1e6, 1),
                          pairs_low_rank=len(ranks), pairs_dense=len(sv) - len(ranks), rank_median=float(np.median(rk)),
                          rank_p90=float(np.percentile(rk, 90)), rank_max=int(rk.max()), rel_err_max=float(err.max()))), flush=True)
