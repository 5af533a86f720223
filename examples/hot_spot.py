"""A photon's hot spot in a current-biased strip: does it trigger a voltage pulse?  One replica per bias current.

A 8 x 2 um strip (xi = 0.5 um, lambda = 2 um, d = 0.1 um) carries a bias current between two terminals; two probes read the
voltage along it.  At t0 a hot spot appears in the middle of the strip -- a local suppression of the critical temperature,
written as py-tdgl's `disorder_epsilon(r, *, t)` --, widens and fades:

    HotSpotEpsilon(1.0, [HotSpot(times, centers, amplitudes, sigmas)])
    epsilon(r, t) = 1 - a(t) exp(-|r - c|^2 / (2 sigma(t)^2))

The time loop evaluates the spot on the device, so the run stays in the run-ahead loop (far fewer host synchronisations than
steps), and `solve_ensemble` runs every bias current in one call: a detection-probability curve.  A phase slip across the
strip passes 2 pi of phase between the probes, the time integral of the voltage pulse it makes; a replica whose voltage
integral after t0 exceeds its level before t0 by more than pi has detected the photon.
Run on an MI355X:  python examples/hot_spot.py [--small] [--bench]
  --small   a coarser mesh, fewer currents and a shorter run (what the test suite runs)
  --bench   one bias current three ways -- the spot as a device source, the same HotSpotEpsilon forced down the per-step
            callable path, and no spot at all -- with steps/s and host synchronisations per step of each
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-tdgl_amd"))
import tdgl_amd as tdgl  # noqa: E402
from tdgl_amd.geometry import box  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true")
ap.add_argument("--bench", action="store_true")
args = ap.parse_args()

layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
film = tdgl.Polygon("film", points=box(8, 2))
source = tdgl.Polygon("source", points=box(0.02, 2, center=(-4, 0)))
drain = tdgl.Polygon("drain", points=box(0.02, 2, center=(4, 0)))
device = tdgl.Device("strip", layer=layer, film=film, terminals=[source, drain], probe_points=[(-3, 0), (3, 0)],
                     length_units="um")
device.make_mesh(max_edge_length=0.3 if args.small else 0.12, smooth=2)
print(device)

# the spot: nothing until t0, then a rise within one time unit to a deep, narrow suppression that widens and fades
T0, T_END = (4.0, 14.0) if args.small else (10.0, 40.0)
times = [T0, T0 + 1.0, T0 + 0.4 * (T_END - T0), T0 + 0.8 * (T_END - T0)]
spot = tdgl.HotSpot(times, centers=(0.0, 0.2), amplitudes=[0.0, 1.0, 0.5, 0.0], sigmas=[0.3, 0.4, 0.8, 1.0])
epsilon = tdgl.HotSpotEpsilon(1.0, [spot])
options = tdgl.SolverOptions(solve_time=T_END, field_units="mT", current_units="uA", save_every=200)


def detected(solution):
    """(excess voltage integral after t0 in units of pi, True if a phase slip crossed the strip)."""
    dyn = solution.dynamics
    v, before = dyn.voltage(), dyn.time < T0
    level = np.average(v[before], weights=dyn.dt[before]) if before.any() else 0.0
    excess = float(np.sum((v[~before] - level) * dyn.dt[~before])) / np.pi
    return excess, abs(excess) > 1.0


if args.bench:
    current = 12.0
    bias = dict(source=current, drain=-current)

    class Opaque:
        """The same HotSpotEpsilon behind a plain callable: the solver cannot see the spots and calls it before every step."""

        def __call__(self, r, *, t=0.0, vectorized=True):
            return epsilon(r, t=t)

    for name, eps in (("device source", epsilon), ("per-step callable", Opaque()), ("no spot", 1.0)):
        solver = tdgl.TDGLSolver(device, options, terminal_currents=bias, disorder_epsilon=eps)
        solver.ctx.step_stats(reset=True)
        t_start = time.perf_counter()
        solution = solver.solve()
        seconds = time.perf_counter() - t_start
        stats = solver.ctx.step_stats()
        steps = solution.stats["steps_simulating"]
        print(f"{name:18s} {steps:6d} steps, {steps / seconds:9.1f} steps/s, {stats['host_syncs'] / max(stats['steps'], 1):.3f} host "
              f"synchronisations per step, excess voltage integral {detected(solution)[0]:+.2f} pi")
    sys.exit(0)

currents = np.linspace(4.0, 16.0, 4 if args.small else 13)  # uA
t_start = time.perf_counter()
solutions = tdgl.solve_ensemble(device, options, terminal_currents=[dict(source=I, drain=-I) for I in currents],
                                disorder_epsilon=epsilon)
print(f"{len(solutions)} replicas in {time.perf_counter() - t_start:.2f} s; mu solve: {solutions[0].stats['mu_solver']}")
for I, sol in zip(currents, solutions):
    excess, hit = detected(sol)
    steps = sol.stats["steps_simulating"]
    print(f"bias {I:6.2f} uA: {steps:6d} steps, voltage integral after t0 {excess:+7.2f} pi above the level before -> "
          f"{'pulse' if hit else 'no pulse'}")

# one of them alone, to show where the time loop ran
solver = tdgl.TDGLSolver(device, options, terminal_currents=dict(source=currents[-1], drain=-currents[-1]), disorder_epsilon=epsilon)
assert solver.device_evaluates_epsilon()
solver.ctx.step_stats(reset=True)
solution = solver.solve()
stats = solver.ctx.step_stats()
print(f"alone at {currents[-1]:.2f} uA: {solution.stats['steps_simulating']} steps, {stats['host_syncs']} host synchronisations "
      f"({stats['host_syncs'] / max(stats['steps'], 1):.3f} per step)")
