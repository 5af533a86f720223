"""Dev benchmark: the fields of the sheet currents on the device (csrc/fields.inc) next to the all-pairs screening kernel.

    python tools/bench_fields.py [--reps K] [L ...]   # film side lengths in xi (70 / 460 / 920 -> 5.8k / 250k / 1M sites)

Per film and per number of targets m in {256, 128^2, 512^2} one JSON line: milliseconds per evaluation of everything at
once (`what` = 7: vector potential, B_z, in-plane B; two current fields), pairs/s and fp64 TFLOP/s at the stated flops
per pair; the same for B_z of one field alone; the pair rate of the all-pairs screening kernel
(`k_induced_vector_potential`, `tdgl_time_kernel` 7) at the same n in the same run; for the smallest size only, the wall
time of the host backend for the same three quantities.

Flops per pair, counted from the kernel source with an FMA as two and the hardware reciprocal square root as one:
2 (dx, dy) + 4 (r^2: two FMAs) + 1 + 8 (1/sqrt and its cubic correction: mul, FMA, mul, FMA, FMA) = 15 shared by
everything; + 2 for 1/r^3 when a field component is asked for; per current field + 4 (A: two FMAs) + 5 (B_z: mul, two
FMAs) + 4 (in-plane B: two FMAs).  `what` = 7 with two fields: 15 + 2 + 2 x 13 = 43 (26 instructions); B_z of one field:
15 + 2 + 5 = 22 (15 instructions).  The screening kernel by the same rule: 2 + 3 (mul, FMA) + 9 + 4 = 18 (12
instructions; tools/bench_screening.py quotes the reference formula's 12 algorithmic flops instead).
"""
import json
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, "tests"); sys.path.insert(0, "py-tdgl_amd"); sys.path.insert(0, ".")
from helpers import synthetic_mesh, uniform_field_A, U_DEFAULT, GAMMA_DEFAULT  # noqa: E402
import tdgl_amd as tdgl  # noqa: E402
from tdgl_amd import SolverOptions, TDGLSolver  # noqa: E402
from tdgl_amd.hipcore import FieldPlan  # noqa: E402
from tdgl_amd.solution import Solution, TDGLData  # noqa: E402

args = sys.argv[1:]
reps = 3
if "--reps" in args:
    i = args.index("--reps")
    reps = int(args[i + 1])
    del args[i:i + 2]

FP64_VECTOR_PEAK = 78.6  # TFLOP/s, MI355X
SCREENING_FLOPS = 18


def flops_per_pair(what, n_fields):
    per_field = (4 if what & 1 else 0) + (5 if what & 2 else 0) + (4 if what & 4 else 0)
    return 15 + (2 if what & 6 else 0) + n_fields * per_field


def targets(mesh, m, z):
    lo, hi = mesh.sites.min(axis=0), mesh.sites.max(axis=0)
    if m == 256:  # a fluxoid polygon's worth of points: a circle inside the film
        t = 2 * np.pi * np.arange(m) / m
        xy = (lo + hi) / 2 + 0.3 * (hi - lo).min() * np.column_stack([np.cos(t), np.sin(t)])
    else:
        side = int(round(np.sqrt(m)))
        gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], side), np.linspace(lo[1], hi[1], side))
        xy = np.column_stack([gx.ravel(), gy.ravel()])
    return np.column_stack([xy, z * np.ones(len(xy))])


def timed(plan, K, what):
    plan.eval(K, what)  # warm-up: code object, buffers
    ms = [(plan.eval(K, what), plan.stats()["last_ms"])[1] for _ in range(reps)]
    return float(np.mean(ms)), float(np.min(ms)), plan.stats()


def host_wall(mesh, K, tgt):
    """Seconds the host backend takes for the same three quantities of both fields."""
    class Given(Solution):
        supercurrent_density = property(lambda self: K[0])
        normal_current_density = property(lambda self: K[1])

    n = len(mesh.sites)
    device = SimpleNamespace(mesh=mesh, points=np.asarray(mesh.sites), coherence_length=1.0, layer=SimpleNamespace(z0=0.0),
                             film=SimpleNamespace(contains_points=lambda p: np.ones(len(p), dtype=bool)), length_units="um")
    step = TDGLData(step=0, time=0.0, dt=0.0, psi=np.ones(n, dtype=complex), mu=np.zeros(n), supercurrent=np.zeros(0),
                    normal_current=np.zeros(0))
    sol = Given(device=device, options=tdgl.SolverOptions(solve_time=1.0), saved_steps=[step], applied_vector_potential=0.0)
    t0 = time.perf_counter()
    sol.field_at_position(tgt, vector=True, return_sum=False, with_units=False)
    sol.vector_potential_at_position(tgt, return_sum=False, with_units=False)
    return time.perf_counter() - t0


for L in [int(a) for a in args] or [70, 460, 920]:
    mesh = synthetic_mesh(L)
    n, n_edges = len(mesh.sites), len(mesh.edge_mesh.edges)
    # the parent's yardstick: the all-pairs screening kernel at the same n (set up as in tools/bench_screening.py)
    opts = SolverOptions(solve_time=1e9, dt_init=1e-5, dt_max=1e-5, adaptive=False, save_every=10**9, include_screening=True,
                         screening_tolerance=1e-6, max_iterations_per_step=1000)
    s = TDGLSolver.from_dimensionless(
        mesh, opts, uniform_field_A(mesh, 3.03e-3), 1.0, U_DEFAULT, GAMMA_DEFAULT,
        screening=dict(sites=mesh.sites, edge_centers=mesh.edge_mesh.centers, areas=mesh.areas / (np.pi * 1.125)))
    ctx = s.ctx
    ctx.set_state(s.psi_init, s.mu_init)
    ctx.begin_stage()
    scr_ms = ctx.time_kernel(7, reps=5 if n < 500_000 else 2)
    scr_pairs_per_s = float(n) * n_edges / (scr_ms * 1e-3)
    ctx.close()
    rng = np.random.default_rng(L)
    K = rng.normal(size=(2, n, 2))
    for m in (256, 128 * 128, 512 * 512):
        tgt = targets(mesh, m, 3.0)
        with FieldPlan(mesh.sites, mesh.areas, 0.0, tgt) as plan:
            ms, ms_min, st = timed(plan, K, 7)
            bz_ms, bz_min, _ = timed(plan, K[:1], 2)
        pairs = float(n) * m
        rate, bz_rate = pairs / (ms * 1e-3), pairs / (bz_ms * 1e-3)
        tf, bz_tf = flops_per_pair(7, 2) * rate / 1e12, flops_per_pair(2, 1) * bz_rate / 1e12
        scr_tf = SCREENING_FLOPS * scr_pairs_per_s / 1e12
        line = dict(
            L=L, sites=n, targets=m, pairs=pairs, reps=reps,
            all_two_fields=dict(what=7, n_fields=2, ms=ms, ms_min=ms_min, pairs_per_s=rate, flops_per_pair=flops_per_pair(7, 2),
                                tflops_fp64=tf, frac_of_fp64_vector_peak=tf / FP64_VECTOR_PEAK),
            bz_one_field=dict(what=2, n_fields=1, ms=bz_ms, ms_min=bz_min, pairs_per_s=bz_rate,
                              flops_per_pair=flops_per_pair(2, 1), tflops_fp64=bz_tf,
                              frac_of_fp64_vector_peak=bz_tf / FP64_VECTOR_PEAK),
            launches=st["launches"], target_batches=st["target_batches"], source_chunks=st["source_chunks"],
            ms_per_launch=ms / max(st["launches"], 1),
            screening_kernel=dict(kernel="k_induced_vector_potential", edges=n_edges, ms=scr_ms, pairs_per_s=scr_pairs_per_s,
                                  flops_per_pair=SCREENING_FLOPS, tflops_fp64=scr_tf),
            rate_per_flop_vs_screening=tf / scr_tf,
        )
        if L == 70 and m == 256:
            line["host_backend_wall_s"] = host_wall(mesh, K, tgt)
        print(json.dumps(line), flush=True)
