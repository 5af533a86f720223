"""Cost of the tabulated field waveform A(t) = TabulatedRamp(t) * A_base on the 5,791-site film (b_peak = 0.3):
  (a) an up-hold-down sweep as a table the device evaluates (run-ahead loop) against the same sweep as a Python
      callable (one host round trip and one upload per step): the gain;
  (b) a two-node table against the LinearRamp it equals: the table path should cost what the ramp costs.
The variants of a pair alternate, `--repeats` times each; per variant the median steps/s and the spread (min, max).
    python tools/bench_field_table.py [--steps 4000] [--repeats 5] > profiles/field_table_5k.json"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, "py-tdgl_amd"); sys.path.insert(0, ".")
from tdgl_amd import SolverOptions, TDGLSolver  # noqa: E402
from tdgl_amd.finite_volume import Mesh  # noqa: E402
from tdgl_amd.meshgen import hex_jitter_points, triangulate  # noqa: E402
from tdgl_amd.parameter import PiecewiseLinear  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

pts = hex_jitter_points(70)
mesh = Mesh.from_triangulation(pts, triangulate(pts))
c = mesh.edge_mesh.centers
b = 0.3
A_base = np.column_stack([-b * (c[:, 1] - (c[:, 1].min() + np.ptp(c[:, 1]) / 2)) / 2, b * (c[:, 0] - (c[:, 0].min() + np.ptp(c[:, 0]) / 2)) / 2])
SWEEP = ([0.0, 100.0, 150.0, 250.0], [0.0, 1.0, 1.0, 0.0])  # up, hold, down: the steps measured lie inside it
RAMP = dict(tmin=0.0, tmax=250.0, initial=0.0, final=1.0)  # (dt <= 0.05: 4,200 steps end before t = 210)
sweep = PiecewiseLinear(*SWEEP)


def make(kind):
    opts = SolverOptions(solve_time=1e9, dt_init=1e-3, dt_max=0.05, save_every=10**9)
    kw = {
        "sweep_table": dict(vector_potential_table=(A_base, *SWEEP)),
        "sweep_callable": dict(vector_potential_func=lambda t: sweep(t) * A_base),
        "two_node_table": dict(vector_potential_table=(A_base, [RAMP["tmin"], RAMP["tmax"]], [RAMP["initial"], RAMP["final"]])),
        "linear_ramp": dict(vector_potential_ramp=(A_base, RAMP)),
    }[kind]
    return TDGLSolver.from_dimensionless(mesh, opts, 0.0 * A_base, 1.0, **kw)


def run(kind):
    """steps/s of `--steps` steps after 200 warm-up steps, through what `solve()` does per chunk of steps."""
    solver = make(kind)
    ctx = solver.ctx
    ctx.set_state(solver.psi_init, solver.mu_init)
    ctx.begin_stage()
    per_step = kind == "sweep_callable"

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
    out = dict(steps_per_s=args.steps / el, host_syncs_per_step=st["host_syncs"] / max(st["steps"], 1), time=ctx.loop_state()["time"],
               link_scale=ctx.link_scale() if not per_step else None)
    ctx.close()
    return out


out = dict(workload=f"square film, {len(mesh.sites)} sites, b_peak {b}, {args.steps} adaptive steps after 200 warm-up steps", pairs={})
for pair in (("sweep_table", "sweep_callable"), ("two_node_table", "linear_ramp")):
    runs = {k: [] for k in pair}
    for _ in range(args.repeats):  # alternated
        for k in pair:
            runs[k].append(run(k))
    res = {}
    for k in pair:
        rates = sorted(r["steps_per_s"] for r in runs[k])
        res[k] = dict(steps_per_s_median=round(float(np.median(rates)), 1), steps_per_s_min=round(rates[0], 1), steps_per_s_max=round(rates[-1], 1),
                      host_syncs_per_step=round(runs[k][0]["host_syncs_per_step"], 3), time_reached=round(runs[k][0]["time"], 3))
    res["ratio_of_medians"] = round(res[pair[0]]["steps_per_s_median"] / res[pair[1]]["steps_per_s_median"], 3)
    out["pairs"]["  vs  ".join(pair)] = res
print(json.dumps(out))
