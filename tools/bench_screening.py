"""Dev benchmark: the induced vector potential of screening, all-pairs kernel against the treecode, and whole screening
steps with each.

    python tools/bench_screening.py [--steps K] [L ...]   # film side lengths in xi (100 / 320 / 460 / 920 -> 12k / 120k / 250k / 1M sites)

Per film one JSON line: the all-pairs kernel alone (pairs/s, fp64 TFLOP/s at 12 algorithmic flops per (edge, site) pair:
tdgl/solver/screening.py:35-42 -- 2 sub, 2 mul, 1 add, 1 sqrt, 2 mul, 2 div, 2 add), one treecode evaluation at the
default (degree, theta) (`tdgl_time_kernel` 22: gather, upward pass, evaluation), its pairs per edge centre (far:
proxies, near: sources), its set-up time, its error against the all-pairs kernel for a smooth sheet current
(max |dA| / max |A|), and milliseconds per screening iteration in K whole steps with each method (the all-pairs one only
up to 300k sites)."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, "tests"); sys.path.insert(0, "py-tdgl_amd"); sys.path.insert(0, ".")
from helpers import synthetic_mesh, uniform_field_A, U_DEFAULT, GAMMA_DEFAULT  # noqa: E402
from tdgl_amd import SolverOptions, TDGLSolver  # noqa: E402

args = sys.argv[1:]
steps = 10
if "--steps" in args:
    i = args.index("--steps")
    steps = int(args[i + 1])
    del args[i:i + 2]


def smooth_current(mesh):
    em = mesh.edge_mesh
    c = em.centers
    unit = em.directions / np.linalg.norm(em.directions, axis=1)[:, None]
    lx, ly = np.ptp(c[:, 0]), np.ptp(c[:, 1])
    F = np.column_stack([np.sin(2 * np.pi * c[:, 1] / ly) + 0.3, np.cos(2 * np.pi * c[:, 0] / lx) - 0.2])
    return (F * unit).sum(axis=1)


def ms_per_iteration(s, ctx, k):
    """k whole steps from the initial state: (ms per screening iteration, iterations)."""
    ctx.set_state(s.psi_init, s.mu_init)
    ctx.set_induced_vector_potential(np.zeros((s.num_edges, 2)))
    ctx.set_controller_state(1e-5)
    ctx.set_loop_state(0, 0.0, 1e-5)
    ctx.begin_stage()
    ctx.synchronize()
    t0 = time.perf_counter()
    res = ctx.run(k)
    wall = time.perf_counter() - t0
    iters = int(res["screening_iterations"].sum())
    return 1e3 * wall / max(iters, 1), iters


for L in [int(a) for a in args] or [100, 320, 460, 920]:
    mesh = synthetic_mesh(L)
    n, m = len(mesh.sites), len(mesh.edge_mesh.edges)
    # fixed dt: with the reference's loop every screening iteration advances psi by dt again, so
    # the adaptive controller's large steps stall the iteration (reference and oracle alike)
    # (the field and the kernel prefactor 1 / (pi Lambda) of the reference's screening test, tests/test_hip_api.py:
    # 0.1 mT on xi = 0.1 um, lambda = 0.075 um, d = 0.05 um; the stronger field of earlier rounds made the
    # reference's heavy-ball iteration stall at step 0)
    opts = SolverOptions(solve_time=1e9, dt_init=1e-5, dt_max=1e-5, adaptive=False, save_every=10**9, include_screening=True,
                         screening_tolerance=1e-6, max_iterations_per_step=1000)
    s = TDGLSolver.from_dimensionless(
        mesh, opts, uniform_field_A(mesh, 3.03e-3), 1.0, U_DEFAULT, GAMMA_DEFAULT,
        screening=dict(sites=mesh.sites, edge_centers=mesh.edge_mesh.centers, areas=mesh.areas / (np.pi * 1.125)))
    ctx = s.ctx
    ctx.set_state(s.psi_init, s.mu_init)
    ctx.begin_stage()
    ms = ctx.time_kernel(7, reps=5 if n < 500_000 else 2)
    pairs = float(n) * m
    tf = 12 * pairs / (ms * 1e-3) / 1e12
    # (the kernel is bound by the fp64 VECTOR rate, 78.6 TFLOP/s on MI355X: a reciprocal square root per pair, not a contraction)
    roofline = dict(bound="fp64 vector", kernel="k_induced_vector_potential", achieved=round(tf, 2), peak=78.6, unit="TFLOP/s",
                    frac=round(tf / 78.6, 4), flops_per_pair=12, pairs=pairs, avg_launch_ms=ms)
    line = dict(L=L, sites=n, edges=m, kernel_ms=ms, pairs_per_s=pairs / (ms * 1e-3), tflops_fp64=tf,
                roofline_screening=roofline)
    K = smooth_current(mesh)
    A_dir = ctx.evaluate_induced_vector_potential(K)
    if n <= 300_000 and steps > 0:
        try:
            line["direct_ms_per_screening_iteration"], line["direct_screening_iterations"] = ms_per_iteration(s, ctx, steps)
        except RuntimeError as exc:
            line["direct_steps_failed"] = str(exc)
    t0 = time.perf_counter()
    ctx.set_screening_tree(opts.screening_tree_degree, opts.screening_tree_theta)
    setup_s = time.perf_counter() - t0
    st = ctx.screening_tree_stats()
    tree_ms = ctx.time_kernel(22, reps=20)
    A_tree = ctx.evaluate_induced_vector_potential(K)
    line.update(tree_degree=opts.screening_tree_degree, tree_theta=opts.screening_tree_theta, tree_ms=tree_ms,
                tree_speedup=ms / tree_ms, tree_setup_s=setup_s, tree_stats=st,
                far_pairs_per_target=st["far_pairs"] / m, near_pairs_per_target=st["near_pairs"] / m,
                tree_pairs_per_s=(st["far_pairs"] + st["near_pairs"]) / (tree_ms * 1e-3),
                tree_error_vs_direct=float(np.abs(A_tree - A_dir).max() / np.abs(A_dir).max()))
    if steps > 0:
        try:
            line["tree_ms_per_screening_iteration"], line["tree_screening_iterations"] = ms_per_iteration(s, ctx, steps)
        except RuntimeError as exc:
            line["tree_steps_failed"] = str(exc)
    print(json.dumps(line), flush=True)
    ctx.close()
