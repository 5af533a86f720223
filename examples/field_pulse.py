"""A bias field plus a pulsed local flux spot: the sum of a static and a time-scaled field term.

A 4 x 4 um film (xi = 0.5 um, lambda = 2 um, d = 0.1 um) is cooled in a uniform bias field of 0.3 mT; a local coil then
sends a pulse through a Gaussian flux spot off centre: up, a hold, down through zero.  The field is written as a plain
`Parameter` sum, as in py-tdgl's `ConstantField(b) + Scale(...) * CurrentLoop(...)`,

    ConstantField(0.3) + TabulatedRamp(times, values) * Parameter(flux_spot, ...)

which `Parameter.separable_terms()` recognises as A_0 + f_1(t) A_1: the time loop evaluates it on the device, so the run
stays in the run-ahead loop (far fewer host synchronisations than steps) instead of calling Python before every step.
Run on an MI355X:  python examples/field_pulse.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-tdgl_amd"))
import tdgl_amd as tdgl  # noqa: E402
from tdgl_amd.geometry import box  # noqa: E402


def flux_spot(x, y, z, *, x0=0.0, y0=0.0, sigma=1.0, flux=1.0):
    """Vector potential of a Gaussian flux spot, A_phi = flux / (2 pi r) (1 - exp(-r^2 / 2 sigma^2)), in mT um."""
    dx, dy = x - x0, y - y0
    r2 = np.maximum(dx * dx + dy * dy, 1e-24)
    g = flux / (2 * np.pi * r2) * -np.expm1(-r2 / (2 * sigma**2))
    return np.stack([-g * dy, g * dx, np.zeros_like(dx)], axis=1)


layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
device = tdgl.Device("film", layer=layer, film=tdgl.Polygon("film", points=box(4, 4)), length_units="um")
device.make_mesh(max_edge_length=0.15, smooth=2)
print(device)

bias = tdgl.ConstantField(0.3, field_units="mT", length_units="um")
pulse = tdgl.TabulatedRamp([5.0, 10.0, 20.0, 25.0], [0.0, 1.0, 1.0, -0.3])
spot = tdgl.Parameter(flux_spot, x0=0.8, y0=-0.5, sigma=0.4, flux=1.2)  # peak field flux / (2 pi sigma^2) = 1.2 mT
field = bias + pulse * spot
static, products = field.separable_terms()
print(f"field: A_0 + {len(products)} time-scaled term(s)")

options = tdgl.SolverOptions(solve_time=30, field_units="mT", current_units="uA", save_every=100)
solver = tdgl.TDGLSolver(device, options, applied_vector_potential=field)
assert solver.device_evaluates_field()
solver.ctx.step_stats(reset=True)
solution = solver.solve()
stats = solver.ctx.step_stats()
print(f"{solution.stats['steps_simulating']} steps in {solution.total_seconds:.2f} s, {stats['host_syncs']} host synchronisations "
      f"({stats['host_syncs'] / max(stats['steps'], 1):.3f} per step); the field moved in {solver.ctx.link_term_moves()} of the steps")
print(f"min |psi| = {np.abs(solution.tdgl_data.psi).min():.3f}; factor of the pulse at the end: {solver.ctx.link_term_scales()[0]:+.2f}")
