"""Cost of a sum of field terms A(t) = A_0 + f_1(t) A_1 + f_2(t) A_2 (a uniform bias, a ramped uniform field, a flux spot
driven up, held and down through zero) on the square film of `--side` (70: 5,791 sites):
  "terms"     the sum as terms the device evaluates (tdgl_set_link_terms; run-ahead loop where the mu solve is direct),
  "per_step"  the same field evaluated in Python and uploaded before every step -- what the equivalent CompositeParameter
              costs on a commit without the terms (`--variants per_step` runs there too: nothing newer is imported),
  "static"    the bias field alone: what a step costs when nothing moves.
The variants alternate, `--repeats` times each; per variant the median steps/s and the spread (min, max), host
synchronisations per step, and the ratio of a moving step to a static one.
    python tools/bench_field_terms.py [--side 70] [--steps 4000] [--repeats 3] > profiles/FIELD_terms_5k.json"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, "py-tdgl_amd"); sys.path.insert(0, ".")
from tdgl_amd import SolverOptions, TDGLSolver  # noqa: E402
from tdgl_amd.finite_volume import Mesh  # noqa: E402
from tdgl_amd.meshgen import hex_jitter_points, triangulate  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=float, default=70.0)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--variants", default="terms,per_step,static")
args = ap.parse_args()
variants = args.variants.split(",")

pts = hex_jitter_points(args.side)
mesh = Mesh.from_triangulation(pts, triangulate(pts))
c = mesh.edge_mesh.centers
xc, yc = c[:, 0].min() + np.ptp(c[:, 0]) / 2, c[:, 1].min() + np.ptp(c[:, 1]) / 2


def uniform(b):
    return np.column_stack([-b * (c[:, 1] - yc) / 2, b * (c[:, 0] - xc) / 2])


def spot(x0, y0, sigma, flux):
    dx, dy = c[:, 0] - x0, c[:, 1] - y0
    r2 = np.maximum(dx * dx + dy * dy, 1e-24)
    g = flux / (2 * np.pi * r2) * -np.expm1(-r2 / (2 * sigma**2))
    return np.column_stack([-g * dy, g * dx])


A0, A1, A2 = uniform(0.1), uniform(0.15), spot(xc + 0.15 * args.side, yc - 0.1 * args.side, 0.1 * args.side, 0.2 * 2 * np.pi * (0.1 * args.side) ** 2)
# (dt <= 0.05: 4,200 steps end before t = 210 -- every measured step lies on a slope of at least one factor)
RAMP = dict(tmin=0.0, tmax=400.0, initial=0.0, final=1.0)
TABLE = ([0.0, 100.0, 150.0, 400.0], [0.0, 1.0, 1.0, -0.6])


def ramp(t):
    return RAMP["initial"] + (RAMP["final"] - RAMP["initial"]) * min(max((t - RAMP["tmin"]) / (RAMP["tmax"] - RAMP["tmin"]), 0.0), 1.0)


def field(t):
    return (A0 + ramp(t) * A1) + float(np.interp(t, *TABLE)) * A2


def make(kind):
    opts = SolverOptions(solve_time=1e9, dt_init=1e-3, dt_max=0.05, save_every=10**9)
    kw = {
        "terms": lambda: dict(vector_potential_terms=(A0, [(A1, RAMP), (A2, TABLE)])),
        "per_step": lambda: dict(vector_potential_func=field),
        "static": lambda: dict(),
    }[kind]()
    return TDGLSolver.from_dimensionless(mesh, opts, field(0.0), 1.0, **kw)


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
    if kind == "terms":
        out["moving_steps"] = ctx.link_term_moves()
    ctx.close()
    return out


out = dict(workload=f"square film, {len(mesh.sites)} sites, bias 0.1 + ramped 0.15 + flux spot (peak 0.2), {args.steps} adaptive steps "
                    "after 200 warm-up steps", variants={})
runs = {k: [] for k in variants}
for _ in range(args.repeats):  # alternated
    for k in variants:
        runs[k].append(run(k))
for k in variants:
    rates = sorted(r["steps_per_s"] for r in runs[k])
    out["variants"][k] = dict(steps_per_s_median=round(float(np.median(rates)), 1), steps_per_s_min=round(rates[0], 1),
                              steps_per_s_max=round(rates[-1], 1), host_syncs_per_step=round(runs[k][0]["host_syncs_per_step"], 3),
                              time_reached=round(runs[k][0]["time"], 3))
    if "moving_steps" in runs[k][0]:
        out["variants"][k]["moving_steps"] = runs[k][0]["moving_steps"]
med = {k: out["variants"][k]["steps_per_s_median"] for k in variants}
if "terms" in med and "per_step" in med:
    out["terms_over_per_step"] = round(med["terms"] / med["per_step"], 3)
if "terms" in med and "static" in med:
    out["moving_step_over_static_step"] = round(med["static"] / med["terms"], 3)  # (time per step)
print(json.dumps(out))
