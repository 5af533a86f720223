"""IV curve of the quick-start strip in ONE call: one replica per bias current, advanced together on the GPU.

Each replica is what `tdgl.solve` would run for its current alone; `mean_voltage` of each gives the curve.
Run on an MI355X:  python examples/iv_curve.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-tdgl_amd"))
import tdgl_amd as tdgl  # noqa: E402
from tdgl_amd.geometry import box, circle  # noqa: E402

layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
film = tdgl.Polygon("film", points=box(6, 3))
hole = tdgl.Polygon("hole", points=circle(0.6, center=(0.5, 0.2)))
source = tdgl.Polygon("source", points=box(0.02, 3, center=(-3, 0)))
drain = tdgl.Polygon("drain", points=box(0.02, 3, center=(3, 0)))
device = tdgl.Device("strip", layer=layer, film=film, holes=[hole], terminals=[source, drain],
                     probe_points=[(-2, 0), (2, 0)], length_units="um")
device.make_mesh(max_edge_length=0.12, smooth=2)
print(device)

currents = np.linspace(0.0, 40.0, 16)  # uA
options = tdgl.SolverOptions(solve_time=60, skip_time=20, field_units="mT", current_units="uA", save_every=200)
solutions = tdgl.solve_ensemble(device, options, applied_vector_potential=0.4,
                                terminal_currents=[dict(source=I, drain=-I) for I in currents])
print(f"{len(solutions)} replicas in {solutions[0].total_seconds:.2f} s; mu solve: {solutions[0].stats['mu_solver']}")
print("   I [uA]   <V> [V0]   steps")
for I, sol in zip(currents, solutions):
    steps = sol.stats["steps_thermalizing"] + sol.stats["steps_simulating"]
    print(f"{I:9.2f} {sol.dynamics.mean_voltage():10.4f} {steps:7d}")
