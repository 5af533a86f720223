"""Cost of a moving current loop as an applied-field source: a uniform bias plus one loop scanned across the square film of
`--side` (70: 5,791 sites), its centre and current moving in every step:
  "loops"     the loop as a device source (tdgl_set_link_loops; run-ahead loop where the mu solve is direct),
  "per_step"  the same field evaluated in NumPy and uploaded before every step -- what a MovingCurrentLoop written by the
              user costs on a commit without device sources (`--variants per_step` runs there too: the script carries its own
              restatement of the loop's potential and imports nothing newer),
  "static"    the bias field alone: what a step costs when nothing moves.
The variants alternate, `--repeats` times each; per variant the median steps/s and the spread (min, max), host
synchronisations per step, and the ratio of a moving step to a static one.  For fresh processes run one variant and one
repeat per invocation and merge the lines (`--merge FILE ...`).
    python tools/bench_moving_loop.py [--side 70] [--steps 4000] [--repeats 3] > profiles/FIELD_loop_s70.json"""
import argparse
import json
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=float, default=70.0)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--variants", default="loops,per_step,static")
ap.add_argument("--merge", nargs="*", default=None, help="merge the JSON lines of earlier invocations instead of running")
args = ap.parse_args()
variants = args.variants.split(",")


def summarise(workload, runs):
    out = dict(workload=workload, variants={})
    for k, rs in runs.items():
        rates = sorted(r["steps_per_s"] for r in rs)
        out["variants"][k] = dict(steps_per_s_median=round(float(np.median(rates)), 1), steps_per_s_min=round(rates[0], 1),
                                  steps_per_s_max=round(rates[-1], 1), host_syncs_per_step=round(rs[0]["host_syncs_per_step"], 3),
                                  time_reached=round(rs[0]["time"], 3), runs=len(rs))
        if "moving_steps" in rs[0]:
            out["variants"][k]["moving_steps"] = rs[0]["moving_steps"]
    med = {k: v["steps_per_s_median"] for k, v in out["variants"].items()}
    if "loops" in med and "per_step" in med:
        out["loops_over_per_step"] = round(med["loops"] / med["per_step"], 3)
    if "loops" in med and "static" in med:
        out["moving_step_over_static_step"] = round(med["static"] / med["loops"], 3)  # (time per step)
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

pts = hex_jitter_points(args.side)
mesh = Mesh.from_triangulation(pts, triangulate(pts))
c = mesh.edge_mesh.centers
xc, yc = c[:, 0].min() + np.ptp(c[:, 0]) / 2, c[:, 1].min() + np.ptp(c[:, 1]) / 2
A0 = np.column_stack([-0.1 * (c[:, 1] - yc) / 2, 0.1 * (c[:, 0] - xc) / 2])
# (dt <= 0.05: 4,200 steps end before t = 210 -- the loop moves and its current changes in every measured step)
RADIUS, HEIGHT = 5.0, 2.0
TIMES = np.array([0.0, 400.0])
CENTERS = np.array([[xc - 0.3 * args.side, yc - 0.1 * args.side, HEIGHT], [xc + 0.3 * args.side, yc + 0.2 * args.side, HEIGHT]])
CURRENTS = np.array([2.0, 3.0])  # (dimensionless; field under the loop I a^2 / (2 (a^2 + z^2)^(3/2)) = 0.08 I)
LOOP = dict(times=TIMES, centers=CENTERS, currents=CURRENTS, radius=RADIUS)


def loop_A(t):
    """I(t) H (-dy, dx): the loop's potential through the arithmetic-geometric mean, without cancellation."""
    cx, cy, cur = (float(np.interp(t, TIMES, v)) for v in (CENTERS[:, 0], CENTERS[:, 1], CURRENTS))
    dx, dy = c[:, 0] - cx, c[:, 1] - cy
    rho = np.sqrt(dx * dx + dy * dy)
    z2, sp, sm = HEIGHT * HEIGHT, RADIUS + rho, RADIUS - rho
    d2 = sp * sp + z2
    b0 = np.sqrt((sm * sm + z2) / d2)
    cr = (2.0 * RADIUS) / (d2 * (1.0 + b0))
    cc, an, bn, sr, p = cr * rho, 0.5 * (1.0 + b0), np.sqrt(b0), 2.0 * (cr * cr), 4.0
    with np.errstate(under="ignore"):
        for _ in range(6):
            a1 = 0.5 * (an + bn)
            bn = np.sqrt(an * bn)
            q = cc / (4.0 * a1)
            cr, cc = cr * q, cc * q
            sr, p, an = sr + p * (cr * cr), p * 2.0, a1
    h = cur * ((sr * np.sqrt(d2)) / (8.0 * an))
    return np.column_stack([-(dy * h), dx * h])


def field(t):
    return A0 + loop_A(t)


def make(kind):
    opts = SolverOptions(solve_time=1e9, dt_init=1e-3, dt_max=0.05, save_every=10**9)
    if kind == "loops":
        return TDGLSolver.from_dimensionless(mesh, opts, A0, 1.0, vector_potential_loops=[LOOP])
    if kind == "per_step":
        return TDGLSolver.from_dimensionless(mesh, opts, field(0.0), 1.0, vector_potential_func=field)
    return TDGLSolver.from_dimensionless(mesh, opts, A0, 1.0)


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
    if kind == "loops":
        out["moving_steps"] = ctx.link_term_moves()
    ctx.close()
    return out


workload = (f"square film, {len(mesh.sites)} sites, bias 0.1 + one loop (radius {RADIUS}, height {HEIGHT}) scanned across the film "
            f"with a rising current, {args.steps} adaptive steps after 200 warm-up steps")
runs = {k: [] for k in variants}
for _ in range(args.repeats):  # alternated
    for k in variants:
        runs[k].append(run(k))
out = summarise(workload, runs)
out["raw"] = runs
print(json.dumps(out))
