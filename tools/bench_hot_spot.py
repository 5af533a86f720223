"""Cost of a Gaussian hot spot in epsilon(r, t): one spot scanned across the square film of `--side` (70: 5,791 sites) in a
uniform field, its centre, amplitude and width moving in every step:
  "spots"     the spot as a device source (tdgl_set_epsilon_spots; run-ahead loop where the mu solve is direct),
  "per_step"  the same epsilon evaluated in NumPy and uploaded before every step -- what a `disorder_epsilon(r, *, t)` written
              by the user costs, and all a commit without device spots can do (`--variants per_step` runs there too: the
              script carries its own restatement of the spot and imports nothing newer),
  "static"    epsilon = 1: what a step costs when nothing moves.
The variants alternate, `--repeats` times each; per variant the median steps/s and the spread (min, max), host
synchronisations per step, and the ratios.  For fresh processes run one variant and one repeat per invocation and merge the
lines (`--merge FILE ...`).  `--big SIDE`: only sets the spots up on a film of that side and applies them `--launches`
times (for a kernel trace of k_eps_spots at a size the time loop is not run at).
    python tools/bench_hot_spot.py [--side 70] [--steps 4000] [--repeats 3] > profiles/EPS_spots_s70.json"""
import argparse
import json
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=float, default=70.0)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--variants", default="spots,per_step,static")
ap.add_argument("--label", default=None, help="a name for this tree in the merged output (e.g. parent)")
ap.add_argument("--merge", nargs="*", default=None, help="merge the JSON lines of earlier invocations instead of running")
ap.add_argument("--big", type=float, default=None)
ap.add_argument("--launches", type=int, default=50)
args = ap.parse_args()
variants = args.variants.split(",")


def summarise(workload, runs):
    out = dict(workload=workload, variants={})
    for k, rs in runs.items():
        rates = sorted(r["steps_per_s"] for r in rs)
        out["variants"][k] = dict(steps_per_s_median=round(float(np.median(rates)), 1), steps_per_s_min=round(rates[0], 1),
                                  steps_per_s_max=round(rates[-1], 1), host_syncs_per_step=round(rs[0]["host_syncs_per_step"], 3),
                                  time_reached=round(rs[0]["time"], 3), runs=len(rs))
    med = {k: v["steps_per_s_median"] for k, v in out["variants"].items()}
    for a, b, name in (("spots", "per_step", "spots_over_per_step"), ("spots", "parent:per_step", "spots_over_parent_per_step"),
                       ("spots", "static", "spots_over_static"), ("static", "parent:static", "static_over_parent_static")):
        if a in med and b in med:
            out[name] = round(med[a] / med[b], 3)
    return out


if args.merge is not None:
    runs, workload = {}, None
    for name in args.merge:
        for line in open(name):
            if line.startswith("{"):
                rec = json.loads(line)
                workload = workload or rec["workload"]
                for k, rs in rec["raw"].items():
                    runs.setdefault(k, []).extend(rs)
    print(json.dumps(summarise(workload, runs)))
    sys.exit(0)

sys.path.insert(0, "py-tdgl_amd"); sys.path.insert(0, ".")
from tdgl_amd import SolverOptions, TDGLSolver  # noqa: E402
from tdgl_amd.finite_volume import Mesh  # noqa: E402
from tdgl_amd.meshgen import hex_jitter_points, triangulate  # noqa: E402

side = args.big if args.big is not None else args.side
pts = hex_jitter_points(side)
mesh = Mesh.from_triangulation(pts, triangulate(pts))
sites = mesh.sites
c = mesh.edge_mesh.centers
xc, yc = c[:, 0].min() + np.ptp(c[:, 0]) / 2, c[:, 1].min() + np.ptp(c[:, 1]) / 2
A0 = np.column_stack([-0.1 * (c[:, 1] - yc) / 2, 0.1 * (c[:, 0] - xc) / 2])
# (dt <= 0.05: 4,200 steps end before t = 210 -- every value of the spot moves in every measured step)
TIMES = np.array([0.0, 400.0])
CENTERS = np.array([[xc - 0.3 * side, yc - 0.1 * side], [xc + 0.3 * side, yc + 0.2 * side]])
AMPS, SIGMAS = np.array([0.3, 0.8]), np.array([2.0, 6.0])
SPOT = dict(times=TIMES, centers=CENTERS, amplitudes=AMPS, sigmas=SIGMAS)


def spot_epsilon(t):
    cx, cy, a, s = (float(np.interp(t, TIMES, v)) for v in (CENTERS[:, 0], CENTERS[:, 1], AMPS, SIGMAS))
    dx, dy = sites[:, 0] - cx, sites[:, 1] - cy
    return 1.0 - a * np.exp(-((dx * dx + dy * dy) / (2.0 * (s * s))))


def make(kind):
    opts = SolverOptions(solve_time=1e9, dt_init=1e-3, dt_max=0.05, save_every=10**9)
    if kind == "spots":
        return TDGLSolver.from_dimensionless(mesh, opts, A0, 1.0, epsilon_spots=(1.0, [SPOT]))
    if kind == "per_step":
        return TDGLSolver.from_dimensionless(mesh, opts, A0, spot_epsilon(0.0), epsilon_func=spot_epsilon)
    return TDGLSolver.from_dimensionless(mesh, opts, A0, 1.0)


if args.big is not None:
    from tdgl_amd.hipcore import TDGLContext

    ctx = TDGLContext(mesh)
    ctx.set_epsilon_spots(sites, 1.0, [SPOT])
    for k in range(args.launches):
        ctx.update_epsilon_spots([[xc + 0.01 * k, yc, 0.5, 3.0]])
    ctx.synchronize()
    print(json.dumps(dict(sites=len(sites), launches=args.launches + 1, epsilon_min=float(ctx.epsilon().min()))))
    ctx.close()
    sys.exit(0)


def run(kind):
    """steps/s of `--steps` steps after 200 warm-up steps, through what `solve()` does per chunk of steps."""
    solver = make(kind)
    ctx = solver.ctx
    ctx.set_state(solver.psi_init, solver.mu_init)
    ctx.begin_stage()
    per_step = kind == "per_step"

    def advance(n):
        done = 0
        while done < n:
            ls = ctx.loop_state()
            solver.update_dynamic_inputs(ls["time"], ls["dt"])
            done += len(ctx.run(1 if per_step else n - done)["dt"])

    advance(200)
    ctx.synchronize()
    ctx.step_stats(reset=True)
    t0 = time.perf_counter()
    advance(args.steps)
    ctx.synchronize()
    el = time.perf_counter() - t0
    st = ctx.step_stats()
    out = dict(steps_per_s=args.steps / el, host_syncs_per_step=st["host_syncs"] / max(st["steps"], 1), time=ctx.loop_state()["time"])
    ctx.close()
    return out


workload = (f"square film, {len(mesh.sites)} sites, field 0.1, one hot spot (a 0.3 -> 0.8, sigma 2 -> 6) scanned across the film, "
            f"{args.steps} adaptive steps after 200 warm-up steps")
prefix = f"{args.label}:" if args.label else ""
runs = {prefix + k: [] for k in variants}
for _ in range(args.repeats):  # alternated
    for k in variants:
        runs[prefix + k].append(run(k))
out = summarise(workload, runs)
out["raw"] = runs
print(json.dumps(out))
