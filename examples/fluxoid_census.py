"""When does the fluxoid of a hole jump, when does a vortex enter?  The census of every step, out of the time loop.

A 6 x 3 um film with a round hole (xi = 0.5 um, lambda = 2 um, d = 0.1 um) sits in a perpendicular field that ramps
from 0 to `field` mT.  With `SolverOptions(vortex_census=True)` the time loop counts, after every accepted step and on
the device, the mesh triangles around which psi winds (by sign) and the winding around the film's rim and around the
hole: `solution.dynamics.vortex_counts`, `.windings`, `.winding_changes(name)`.  Nothing is saved for it: `save_every`
stays at 1000 and the run stays in the run-ahead loop.  Printed: the times at which the hole's fluxoid and the number
of vortices in the film change.

    python examples/fluxoid_census.py [field_mT]
    python examples/fluxoid_census.py --bench [--out FILE] [--sides 70 600] [--steps 4000 400] [--rounds 3] [--modes ...]

`--bench` measures what the census costs a run of `tdgl.solve`'s loop: the census off, the census on, and what a user
had to do before it existed ("today": `save_every=1`, then `tdgl.VortexFinder` over the saved steps), alternated in one
process and repeated, on the square film of side 70 xi (5,791 sites, run-ahead loop) and of side 600 xi (above 400k
sites, AMG-PCG) in the field b = B / Bc2 = 0.1 from psi = 1 -- a film that a few vortices enter -- at a fixed time
step, so that every window is the same run of `--steps` steps.  One JSON line per window (steps/s, host
synchronisations per step) goes to `--out` (default profiles/CENSUS_bench.jsonl).  `--package DIR` imports `tdgl_amd`
from another checkout's `py-tdgl_amd` (with `--modes off`: the same run on the parent commit, for the "off" rate).
Run on an MI355X.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PACKAGE = sys.argv[sys.argv.index("--package") + 1] if "--package" in sys.argv[:-1] else os.path.join(ROOT, "py-tdgl_amd")
sys.path.insert(0, PACKAGE)
import tdgl_amd as tdgl  # noqa: E402
from tdgl_amd.geometry import box, circle  # noqa: E402


def example(field: float) -> None:
    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    film = tdgl.Polygon("film", points=box(6, 3))
    hole = tdgl.Polygon("hole", points=circle(0.6, center=(0.5, 0.2)))
    device = tdgl.Device("plate", layer=layer, film=film, holes=[hole], length_units="um")
    device.make_mesh(max_edge_length=0.12, smooth=2)

    ramp = tdgl.LinearRamp(tmin=0, tmax=60, initial=0, final=1) * tdgl.ConstantField(field, field_units="mT", length_units="um")
    options = tdgl.SolverOptions(solve_time=80, field_units="mT", current_units="uA", save_every=1000, vortex_census=True)
    solver = tdgl.TDGLSolver(device, options, applied_vector_potential=ramp)
    solver.ctx.step_stats(reset=True)
    solution = solver.solve()
    stats = solver.ctx.step_stats()
    dyn = solution.dynamics
    print(f"{len(dyn.dt)} steps of {len(device.points)} sites in {solution.total_seconds:.2f} s, {len(solution.saved_steps)} of them "
          f"saved, {stats['host_syncs'] / max(stats['steps'], 1):.3f} host synchronisations per step; loops {dyn.loop_names}")
    for name in dyn.loop_names:
        steps, times, old, new = dyn.winding_changes(name)
        print(f"winding around {name!r}: {len(steps)} changes")
        for k, t, a, b in zip(steps, times, old, new):
            print(f"  t = {t:7.3f} tau_0 (B = {field * min(t / 60, 1):.3f} mT, step {k}): {a:+d} -> {b:+d}")
    n = dyn.vortex_counts.sum(axis=0)
    (at,) = np.nonzero(n[1:] != n[:-1])
    print(f"charged triangles in the film: {len(at)} changes")
    for k in at[:40] + 1:
        print(f"  t = {dyn.time[k]:7.3f} tau_0 (step {k}): {dyn.vortex_counts[0, k]} vortices, {dyn.vortex_counts[1, k]} antivortices")
    undefined = np.isnan(dyn.winding("film")).sum()
    w = dyn.windings[:, -1]
    print(f"at the end: net vorticity {dyn.net_vorticity()[-1]:+d} = winding(film) {w[0]:+d} - winding(hole) {w[1]:+d}; "
          f"{undefined} steps with an undefined rim winding")


# ------------------------------------------------------------------ --bench
BC2_MT = 0.32911  # Phi_0 / (2 pi xi^2) at xi = 1 um


def _solver(side: float, mode: str, steps: int):
    """A `TDGLSolver` on the square film of ``side`` coherence lengths (xi = 1 um) at b = 0.1, fixed dt = 0.01."""
    from tdgl_amd.meshgen import hex_jitter_points, triangulate

    layer = tdgl.Layer(coherence_length=1.0, london_lambda=2.0, thickness=0.1, gamma=10)
    device = tdgl.Device("film", layer=layer, film=tdgl.Polygon("film", points=box(side, side)), length_units="um")
    pts = hex_jitter_points(side, side)  # (side 70: the 5,791 sites of the small benchmark film)
    device.mesh_from_triangulation(pts, triangulate(pts))
    dt = 0.01
    extra = dict(vortex_census=True) if mode == "on" else {}
    if side > 200:
        extra["sparse_solver"] = "amg_pcg"
    options = tdgl.SolverOptions(solve_time=(steps - 0.5) * dt, dt_init=dt, adaptive=False, field_units="mT",
                                 save_every=1 if mode == "today" else 10**9, **extra)
    return device, tdgl.TDGLSolver(device, options, applied_vector_potential=0.1 * BC2_MT)


def _window(device, solver, mode):
    """One timed `solve()`: (steps, seconds, host syncs, last census row or None)."""
    ctx = solver.ctx
    ctx.synchronize()
    ctx.step_stats(reset=True)
    t0 = time.perf_counter()
    solution = solver.solve()
    row = None
    if mode == "today":
        with tdgl.VortexFinder(device, device_id=0) as finder:
            frames = finder.find(solution.saved_steps[1:])
            wind = finder.windings(solution.saved_steps[1:])
        row = [int(np.sum(frames[-1].charges > 0)), int(np.sum(frames[-1].charges < 0)), *wind[-1].values()]
    elif mode == "on":
        dyn = solution.dynamics
        row = [int(v) for v in dyn.vortex_counts[:, -1]] + [int(v) for v in dyn.windings[:, -1]]
    seconds = time.perf_counter() - t0
    stats = ctx.step_stats()
    return stats["steps"], seconds, stats["host_syncs"], row


def bench(out: str, sides, steps, rounds: int, modes) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    steps = list(steps) + [steps[-1]] * (len(sides) - len(steps))
    with open(out, "a") as fh:
        for side, n in zip(sides, steps):
            runs = {mode: _solver(side, mode, n if mode != "today" else max(n // 10, 20)) for mode in modes}
            for device, solver in runs.values():
                solver.solve()  # warm-up: the same run once, untimed
            for rnd in range(rounds):
                for mode, (device, solver) in runs.items():
                    done, seconds, syncs, row = _window(device, solver, mode)
                    ctx = solver.ctx
                    line = dict(bench="census", package=os.path.relpath(PACKAGE, ROOT), sites=len(device.points),
                                triangles=len(device.triangles),
                                loop="amg_pcg" if side > 200 else ("run_ahead" if ctx.dense_direct else "classic"),
                                mode=mode, round=rnd, steps=done, seconds=round(seconds, 6), steps_per_s=round(done / seconds, 1),
                                host_syncs_per_step=round(syncs / done, 4), last_row=row)
                    print(json.dumps(line), flush=True)
                    fh.write(json.dumps(line) + "\n")
                    fh.flush()
            for device, solver in runs.values():
                solver.ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("field", nargs="?", type=float, default=1.2, help="final field of the ramp in mT")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "CENSUS_bench.jsonl"))
    ap.add_argument("--sides", nargs="+", type=float, default=[70.0, 600.0])
    ap.add_argument("--steps", nargs="+", type=int, default=[4000, 400], help="steps per window, one number per side")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["off", "on", "today"], choices=["off", "on", "today"])
    ap.add_argument("--package", default=None, help="directory to import tdgl_amd from (default: this checkout's py-tdgl_amd)")
    args = ap.parse_args()
    if args.bench:
        bench(args.out, args.sides, args.steps, args.rounds, args.modes)
    else:
        example(args.field)
