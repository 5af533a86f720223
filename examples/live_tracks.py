"""Where do the vortices go, step by step?  Tracks out of the time loop, of a run that saves nothing.

A 6 x 3 um film with a round hole (xi = 0.5 um, lambda = 2 um, d = 0.1 um) sits in a perpendicular field that ramps
from 0 to `field` mT.  With `SolverOptions(vortex_cores=True)` the launch that counts the vortices after every accepted
step (`vortex_census`) also writes one record per core -- triangle, charge, position -- and
`solution.dynamics.vortex_cores.tracks(r)` links them into tracks with velocities at step resolution.  Nothing is saved
for it: `save_every` stays at 1000, the run stays in the run-ahead loop, and psi is never uploaded again.

    python examples/live_tracks.py [field_mT]
    python examples/live_tracks.py --bench [--out FILE] [--sides 70 600] [--b 0.1 0.1] [--steps 4000 400] [--rounds 3] [--modes ...]

`--bench` measures what the records cost a run of `tdgl.solve`'s loop: everything off, the census on, the cores on
(with their tracks), and what a user had to do before ("today": `save_every=1`, then `tdgl.VortexFinder.tracks` over the
saved steps), alternated in one process and repeated, on the square film of side 70 xi (5,791 sites, run-ahead loop) and
of side 600 xi (above 400k sites, AMG-PCG) in the field b = B / Bc2 of `--b` from psi = 1 at a fixed time step, so that
every window is the same run of `--steps` steps.  One JSON line per window (steps/s over the whole window, the seconds
of the loop alone, host synchronisations per step, records, incomplete steps) goes to `--out` (default
profiles/CORES_bench.jsonl).  `--package DIR` imports `tdgl_amd` from another checkout's `py-tdgl_amd` (with `--modes
off`: the same run on the parent commit, for the "off" rate; `--label` names it in the lines).  Run on an MI355X.
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
    options = tdgl.SolverOptions(solve_time=80, field_units="mT", current_units="uA", save_every=1000, vortex_cores=True)
    solver = tdgl.TDGLSolver(device, options, applied_vector_potential=ramp)
    solver.ctx.step_stats(reset=True)
    solution = solver.solve()
    stats = solver.ctx.step_stats()
    cores = solution.dynamics.vortex_cores
    print(f"{len(solution.dynamics.dt)} steps of {len(device.points)} sites in {solution.total_seconds:.2f} s, "
          f"{len(solution.saved_steps)} of them saved, {stats['host_syncs'] / max(stats['steps'], 1):.3f} host synchronisations "
          f"per step; {len(cores.charges)} core records in {len(cores)} steps, {int((~cores.complete).sum())} steps incomplete")
    t0 = time.perf_counter()
    tracks = cores.tracks(max_distance=0.25)
    print(f"{len(tracks)} tracks in {time.perf_counter() - t0:.2f} s")
    for k, tr in enumerate(tracks):
        if len(tr.frame_indices) < 20:
            continue
        speed = np.hypot(*tr.velocities.T)
        print(f"  track {k}: charge {tr.charge:+d}, t = {tr.times[0]:7.3f} .. {tr.times[-1]:7.3f} tau_0, {len(tr.frame_indices)} steps, "
              f"({tr.positions[0, 0]:+.2f}, {tr.positions[0, 1]:+.2f}) -> ({tr.positions[-1, 0]:+.2f}, {tr.positions[-1, 1]:+.2f}) um, "
              f"median speed {np.median(speed):.3f} um / tau_0, starts: {tr.start.kind}"
              f"{' at ' + str(tr.start.loop) if tr.start.loop else ''}, ends: {tr.end.kind}{' at ' + str(tr.end.loop) if tr.end.loop else ''}")


# ------------------------------------------------------------------ --bench
BC2_MT = 0.32911  # Phi_0 / (2 pi xi^2) at xi = 1 um
MODES = ("off", "census", "cores", "today")
TRACK_RADIUS = 1.0  # um: how far a core may move in one step of the bench's films


def _solver(side: float, b: float, mode: str, steps: int):
    """A `TDGLSolver` on the square film of ``side`` coherence lengths (xi = 1 um) at the field ``b`` Bc2, fixed dt = 0.01."""
    from tdgl_amd.meshgen import hex_jitter_points, triangulate

    layer = tdgl.Layer(coherence_length=1.0, london_lambda=2.0, thickness=0.1, gamma=10)
    device = tdgl.Device("film", layer=layer, film=tdgl.Polygon("film", points=box(side, side)), length_units="um")
    pts = hex_jitter_points(side, side)  # (side 70: the 5,791 sites of the small benchmark film)
    device.mesh_from_triangulation(pts, triangulate(pts))
    dt = 0.01
    extra = {"census": dict(vortex_census=True), "cores": dict(vortex_cores=True)}.get(mode, {})
    if side > 200:
        extra["sparse_solver"] = "amg_pcg"
    options = tdgl.SolverOptions(solve_time=(steps - 0.5) * dt, dt_init=dt, adaptive=False, field_units="mT",
                                 save_every=1 if mode == "today" else 10**9, **extra)
    return device, tdgl.TDGLSolver(device, options, applied_vector_potential=b * BC2_MT)


def _window(device, solver, mode):
    """One timed `solve()` with what the mode is for: (steps, seconds, host syncs, what was found)."""
    ctx = solver.ctx
    ctx.synchronize()
    ctx.step_stats(reset=True)
    t0 = time.perf_counter()
    solution = solver.solve()
    found = dict(solve_seconds=round(time.perf_counter() - t0, 6))  # the loop alone, before the cores are found / linked
    if mode == "today":
        with tdgl.VortexFinder(device, device_id=0) as finder:
            tracks = finder.tracks(solution.saved_steps[1:], TRACK_RADIUS)
        found.update(records=int(sum(len(f.charges) for f in tracks.frames)), tracks=len(tracks))
    elif mode == "census":
        found.update(last_counts=[int(v) for v in solution.dynamics.vortex_counts[:, -1]])
    elif mode == "cores":
        cores = solution.dynamics.vortex_cores
        found.update(records=int(len(cores.charges)), incomplete=int((~cores.complete).sum()),
                     last_counts=[int(v) for v in solution.dynamics.vortex_counts[:, -1]])
        if cores.complete.all():
            found["tracks"] = len(cores.tracks(TRACK_RADIUS, backend="hip"))
    seconds = time.perf_counter() - t0
    stats = ctx.step_stats()
    return stats["steps"], seconds, stats["host_syncs"], found


def bench(out: str, sides, fields, steps, rounds: int, modes, label=None) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    steps = list(steps) + [steps[-1]] * (len(sides) - len(steps))
    fields = list(fields) + [fields[-1]] * (len(sides) - len(fields))
    with open(out, "a") as fh:
        for side, b, n in zip(sides, fields, steps):
            runs = {mode: _solver(side, b, mode, n if mode != "today" else max(n // 10, 20)) for mode in modes}
            for device, solver in runs.values():
                solver.solve()  # warm-up: the same run once, untimed
            for rnd in range(rounds):
                for mode, (device, solver) in runs.items():
                    # (the window before this one may have ended in host work -- "today" links its tracks in Python -- with
                    # the GPU idle and its clocks down: the same run once more, untimed, right before the timed one)
                    solver.solve()
                    done, seconds, syncs, found = _window(device, solver, mode)
                    ctx = solver.ctx
                    line = dict(bench="cores", package=label or os.path.relpath(PACKAGE, ROOT), sites=len(device.points),
                                triangles=len(device.triangles), b=b,
                                loop="amg_pcg" if side > 200 else ("run_ahead" if ctx.dense_direct else "classic"),
                                mode=mode, round=rnd, steps=done, seconds=round(seconds, 6), steps_per_s=round(done / seconds, 1),
                                host_syncs_per_step=round(syncs / done, 4), **found)
                    print(json.dumps(line), flush=True)
                    fh.write(json.dumps(line) + "\n")
                    fh.flush()
            for device, solver in runs.values():
                solver.ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("field", nargs="?", type=float, default=1.2, help="final field of the ramp in mT")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "CORES_bench.jsonl"))
    ap.add_argument("--sides", nargs="+", type=float, default=[70.0, 600.0])
    ap.add_argument("--b", nargs="+", type=float, default=[0.1], help="field in units of Bc2, one number per side")
    ap.add_argument("--steps", nargs="+", type=int, default=[4000, 400], help="steps per window, one number per side")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=MODES)
    ap.add_argument("--package", default=None, help="directory to import tdgl_amd from (default: this checkout's py-tdgl_amd)")
    ap.add_argument("--label", default=None, help="what the lines' package field says (default: the package's path)")
    args = ap.parse_args()
    if args.bench:
        bench(args.out, args.sides, args.b, args.steps, args.rounds, args.modes, args.label)
    else:
        example(args.field)
