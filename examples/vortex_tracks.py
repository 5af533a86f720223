"""Vortex cores of every saved step: a film with a hole in a field, the cores found on the GPU.

A 6 x 3 um film with a round hole is solved in a perpendicular field strong enough for vortices to enter.
`tdgl.VortexFinder` keeps the mesh and the boundary loops on the device and finds, for all saved steps in one call, the
mesh triangles around which psi winds (with the position of the zero of psi inside each) and the winding around the
film's rim and around the hole.  Per step one line: the time, the number of cores by sign, the windings, and the check
that the cores account for them: sum of charges = winding(film) - winding(hole).  Then `finder.tracks` links the cores
of consecutive steps into tracks, also on the device, and every track gets one line: its charge, its first and last
time, its length, how it started and ended (through which boundary loop, or with which other track as a pair) and its
mean speed.
Run on an MI355X:  python examples/vortex_tracks.py [field_mT]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-tdgl_amd"))
import tdgl_amd as tdgl  # noqa: E402
from tdgl_amd.geometry import box, circle  # noqa: E402

field = float(sys.argv[1]) if len(sys.argv) > 1 else 1.2

layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
film = tdgl.Polygon("film", points=box(6, 3))
hole = tdgl.Polygon("hole", points=circle(0.6, center=(0.5, 0.2)))
device = tdgl.Device("plate", layer=layer, film=film, holes=[hole], length_units="um")
device.make_mesh(max_edge_length=0.12, smooth=2)

options = tdgl.SolverOptions(solve_time=40, field_units="mT", current_units="uA", save_every=1000)
solution = tdgl.solve(device, options, applied_vector_potential=field)

with tdgl.VortexFinder(device, device_id=options.device_id) as finder:
    frames = finder.find(solution.saved_steps)
    windings = finder.windings(solution.saved_steps)
    print(f"{len(frames)} saved steps of {len(device.points)} sites, {len(device.triangles)} triangles: "
          f"{finder.stats()['last_ms']:.3f} ms on the device for the windings of all of them")
    # the same cores linked from step to step: a vortex moves by less than `reach` between two saved steps
    reach = 6 * 0.12
    tracks = finder.tracks(solution.saved_steps, max_distance=reach)
    print(f"{finder.link_stats()['links']} links into {len(tracks)} tracks: {finder.link_stats()['last_ms']:.3f} ms on the device")

for time, cores, w in zip(solution.times, frames, windings):
    plus, minus = int(np.sum(cores.charges > 0)), int(np.sum(cores.charges < 0))
    if None in w.values():
        balance = "a loop passes through a zero of psi"
    else:
        balance = "accounted for" if plus - minus == w["film"] - w["hole"] else "NOT accounted for"
    print(f"t = {time:7.2f} tau_0: {plus:3d} vortices, {minus:3d} antivortices; winding film {w['film']}, hole {w['hole']}"
          f" ({balance})")

last = frames[-1]
np.save("vortex_cores.npy", np.column_stack([last.positions, last.charges]))
print(f"cores of the last step (x, y in {device.length_units}, charge) -> vortex_cores.npy; the host backend agrees: "
      f"{np.array_equal(solution.vortices().triangles, last.triangles)}")

print(f"tracks (max_distance {reach:.2f} {device.length_units}): charge, first .. last time, steps, start -> end, mean speed")
def told(event):
    if event.kind == "pair":
        return f"pair with track {event.partner}"
    return f"{event.kind} ({event.loop})" if event.kind == "boundary" else event.kind


for k, track in enumerate(tracks):
    speed = np.hypot(*track.velocities.T).mean() if len(track.velocities) else 0.0
    print(f"track {k:3d}: {track.charge:+d}, t = {track.times[0]:7.2f} .. {track.times[-1]:7.2f} tau_0, {len(track.times):3d} steps, "
          f"{told(track.start)} -> {told(track.end)}, {speed:.4f} {device.length_units}/tau_0")
