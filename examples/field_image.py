"""Field image: B_z of the currents on a grid at a height above the quick-start strip, evaluated on the GPU.

The strip of examples/quickstart.py (6 x 3 um, a round hole, 0.4 mT applied field, 12 uA transport current) is solved
for a short time; `tdgl.FieldEvaluator` keeps the sites and the grid on the device and evaluates every saved step, so
that only the site currents travel per frame.  The last frame and the movie are saved as `.npy`.
Run on an MI355X:  python examples/field_image.py [height_um] [pixels_x]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-tdgl_amd"))
import tdgl_amd as tdgl  # noqa: E402
from tdgl_amd.geometry import box, circle  # noqa: E402

height = float(sys.argv[1]) if len(sys.argv) > 1 else 0.5
nx = int(sys.argv[2]) if len(sys.argv) > 2 else 256
ny = nx // 2

layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
film = tdgl.Polygon("film", points=box(6, 3))
hole = tdgl.Polygon("hole", points=circle(0.6, center=(0.5, 0.2)))
source = tdgl.Polygon("source", points=box(0.02, 3, center=(-3, 0)))
drain = tdgl.Polygon("drain", points=box(0.02, 3, center=(3, 0)))
device = tdgl.Device("strip", layer=layer, film=film, holes=[hole], terminals=[source, drain],
                     probe_points=[(-2, 0), (2, 0)], length_units="um")
device.make_mesh(max_edge_length=0.12, smooth=2)

options = tdgl.SolverOptions(solve_time=30, field_units="mT", current_units="uA", save_every=200)
solution = tdgl.solve(device, options, applied_vector_potential=0.4, terminal_currents=dict(source=12.0, drain=-12.0))

gx, gy = np.meshgrid(np.linspace(-4, 4, nx), np.linspace(-2, 2, ny))
grid = np.column_stack([gx.ravel(), gy.ravel()])

# one image of the loaded (last) step through the Solution method ...
image = solution.field_at_position(grid, zs=height, with_units=False, backend="hip").reshape(ny, nx)
np.save("field_image.npy", image)
print(f"B_z of the currents {height} um above the film: {image.min():.4g} ... {image.max():.4g} mT "
      f"({nx} x {ny} pixels, {len(device.points)} sites) -> field_image.npy")

# ... and every saved step with the sites and the grid kept on the device
with tdgl.FieldEvaluator(device, grid, zs=height, device_id=options.device_id) as evaluator:
    frames = []
    for k in range(len(solution.saved_steps)):
        solution.load_tdgl_data(k)
        frames.append(evaluator.field(solution, with_units=False).reshape(ny, nx))
np.save("field_movie.npy", np.stack(frames))
print(f"{len(frames)} frames -> field_movie.npy; times {solution.times[0]:.2f} ... {solution.times[-1]:.2f} tau_0")
