"""A field coil scanned across a film with a hole: a moving current loop as the applied field.

A 6 x 4 um film (xi = 0.5 um, lambda = 2 um, d = 0.1 um) with a round hole sits in a small uniform bias field.  A coil of
0.8 um radius, 0.5 um above the film, is energised and then scanned along x across the hole, as a susceptometer's field
coil or a SQUID-on-tip would be.  The field is written as in py-tdgl,

    ConstantField(0.05) + MovingCurrentLoop(times, centers, radius=0.8, current=currents, current_units="mA")

which `Parameter.device_sources()` recognises as a static part plus one moving loop: the time loop evaluates the loop's
centre, its current and its vector potential on the device, so the run stays in the run-ahead loop (far fewer host
synchronisations than steps) instead of calling Python before every step.  The fluxoid of a contour around the hole is read
from every saved step.
Run on an MI355X:  python examples/scanning_coil.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-tdgl_amd"))
import tdgl_amd as tdgl  # noqa: E402
from tdgl_amd.geometry import box, circle  # noqa: E402

layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
device = tdgl.Device("film", layer=layer, film=tdgl.Polygon("film", points=box(6, 4)),
                     holes=[tdgl.Polygon("hole", points=circle(0.6))], length_units="um")
device.make_mesh(max_edge_length=0.2, smooth=2)
print(device)

bias = tdgl.ConstantField(0.05, field_units="mT", length_units="um")
# energise the coil at rest left of the hole (t = 0 .. 5), scan it across (5 .. 45), switch it off (45 .. 50)
times = [0.0, 5.0, 45.0, 50.0]
centers = [[-2.2, 0.3, 0.5], [-2.2, 0.3, 0.5], [2.2, 0.3, 0.5], [2.2, 0.3, 0.5]]
currents = [0.0, 1.5, 1.5, 0.0]  # mA: mu_0 I a^2 / (2 (a^2 + z^2)^(3/2)) = 0.72 mT under the coil
coil = tdgl.MovingCurrentLoop(times, centers, radius=0.8, current=currents, current_units="mA", field_units="mT", length_units="um")
field = bias + coil
static, terms, loops = field.device_sources()
print(f"field: a static part, {len(terms)} time-scaled term(s), {len(loops)} moving loop(s)")

options = tdgl.SolverOptions(solve_time=55, field_units="mT", current_units="uA", save_every=100)
solver = tdgl.TDGLSolver(device, options, applied_vector_potential=field)
assert solver.device_evaluates_field()
solver.ctx.step_stats(reset=True)
solution = solver.solve()
stats = solver.ctx.step_stats()
print(f"{solution.stats['steps_simulating']} steps in {solution.total_seconds:.2f} s, {stats['host_syncs']} host synchronisations "
      f"({stats['host_syncs'] / max(stats['steps'], 1):.3f} per step); the field moved in {solver.ctx.link_term_moves()} of the steps")

contour = circle(0.9, points=201)
print("  time   coil x   fluxoid around the hole [Phi_0] (flux part + supercurrent part)")
for k, t in enumerate(solution.times):
    solution.load_tdgl_data(k)
    fluxoid = solution.polygon_fluxoid(contour, with_units=False)
    print(f"{t:6.2f}  {np.interp(t, times, [c[0] for c in centers]):+6.2f}   {sum(fluxoid):+.4f}  ({fluxoid.flux_part:+.4f} {fluxoid.supercurrent_part:+.4f})")
