"""Current maps, I(t) through a cut and M(t) of every saved step: one sampler on the GPU, one call each.

The quick-start strip (a 6 x 3 um film with a round hole, a perpendicular field, a transport current between two
terminals) is solved for a short time with several saved steps.  One `tdgl.CurrentSampler` keeps the mesh and a raster of
positions over the film on the device, a second one a path across the strip; from them come, for all saved steps in one
call each, the sheet current density on the raster (|K| images -> current_maps.npy), the current through the path and
the magnetic moment.  The raster lives on the mesh triangulation: between the sites the densities are the piecewise-linear
interpolant of `Solution.interp_current_density`, zero in the hole and beyond the rim.
Run on an MI355X:  python examples/current_maps.py [field_mT]

    python examples/current_maps.py --bench [L] [--frames F] [--raster N]

measures instead: a square film of side L xi (70 -> 5.8k sites, 920 -> 1M sites), an N x N raster (default 256) and F
frames (default 32) of Gaussian edge currents per call; one JSON line with the mesh size, the points, the frames, the
device time per frame (`last_ms`), the wall time per frame including the uploads and read-backs, and the wall time per
frame of the NumPy path (`Solution.interp_current_density`, its interpolator already built) on the same box.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-tdgl_amd"))
import tdgl_amd as tdgl  # noqa: E402
from tdgl_amd.geometry import box, circle  # noqa: E402


def raster_over(lo, hi, nx, ny):
    """Cell centres of an nx x ny raster over the box, [ny * nx, 2], row by row."""
    xs = lo[0] + (np.arange(nx) + 0.5) * (hi[0] - lo[0]) / nx
    ys = lo[1] + (np.arange(ny) + 0.5) * (hi[1] - lo[1]) / ny
    X, Y = np.meshgrid(xs, ys)
    return np.column_stack([X.ravel(), Y.ravel()])


def bench(args):
    from tdgl_amd.meshgen import hex_jitter_points, triangulate
    from tdgl_amd.solution import Solution, TDGLData

    def option(flag, default):
        if flag in args:
            i = args.index(flag)
            value = int(args[i + 1])
            del args[i:i + 2]
            return value
        return default

    frames, side = option("--frames", 32), option("--raster", 256)
    L = int(args[0]) if args else 70
    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1)
    points = hex_jitter_points(L) * layer.coherence_length
    lo, hi = points.min(axis=0), points.max(axis=0)
    film = tdgl.Polygon("film", points=box(hi[0] - lo[0], hi[1] - lo[1], center=tuple((lo + hi) / 2)))
    device = tdgl.Device("film", layer=layer, film=film, length_units="um")
    device.mesh_from_triangulation(points, triangulate(points))
    n, n_edges = len(device.points), len(device.mesh.edge_mesh.edges)
    raster = raster_over(lo, hi, side, side)
    rng = np.random.default_rng(L)
    js, jn = rng.normal(size=(frames, n_edges)), rng.normal(size=(frames, n_edges))
    t0 = time.perf_counter()
    with tdgl.CurrentSampler(device, raster) as sampler:
        setup_s = time.perf_counter() - t0
        sampler.current_density((js[:1], jn[:1]))  # warm-up: code object, buffers
        wall, dev = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            K = sampler.current_density((js, jn))
            wall.append(time.perf_counter() - t0)
            dev.append(sampler.stats()["last_ms"])
        stats = sampler.stats()
    options = tdgl.SolverOptions(solve_time=1.0, current_units="uA")
    host_frames = min(frames, 2)
    t0 = time.perf_counter()
    steps = [TDGLData(step=k, time=0.0, dt=0.0, psi=np.ones(n, dtype=complex), mu=np.zeros(n), supercurrent=js[k],
                      normal_current=jn[k]) for k in range(host_frames)]
    solution = Solution(device=device, options=options, saved_steps=steps)
    solution._interpolator("linear")
    host_setup_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    for k in range(host_frames):
        solution.load_tdgl_data(k)
        host = solution.interp_current_density(raster)
    host_s = (time.perf_counter() - t0) / host_frames
    scale = np.abs(host).max()
    line = dict(L=L, sites=n, edges=n_edges, triangles=len(device.triangles), points=len(raster), frames=frames,
                located=stats["located"], chunks=stats["chunks"], launches=stats["launches"], sampler_setup_s=setup_s,
                device_ms_per_frame=float(np.min(dev)) / frames, wall_ms_per_frame=1e3 * float(np.min(wall)) / frames,
                numpy_setup_s=host_setup_s, numpy_wall_ms_per_frame=1e3 * host_s,
                max_difference_over_scale=float(np.abs(K[host_frames - 1] - host).max() / scale))
    print(json.dumps(line), flush=True)


def main(args):
    field = float(args[0]) if args else 0.4
    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    film = tdgl.Polygon("film", points=box(6, 3))
    hole = tdgl.Polygon("hole", points=circle(0.6, center=(0.5, 0.2)))
    source = tdgl.Polygon("source", points=box(0.02, 3, center=(-3, 0)))
    drain = tdgl.Polygon("drain", points=box(0.02, 3, center=(3, 0)))
    device = tdgl.Device("strip", layer=layer, film=film, holes=[hole], terminals=[source, drain],
                         probe_points=[(-2, 0), (2, 0)], length_units="um")
    device.make_mesh(max_edge_length=0.12, smooth=2)
    options = tdgl.SolverOptions(solve_time=20, field_units="mT", current_units="uA", save_every=200)
    solution = tdgl.solve(device, options, applied_vector_potential=field, terminal_currents=dict(source=12.0, drain=-12.0))
    steps = solution.saved_steps

    nx, ny = 192, 96
    raster = raster_over((-3.0, -1.5), (3.0, 1.5), nx, ny)
    path = np.column_stack([np.full(201, -1.5), np.linspace(-1.5, 1.5, 201)])  # a cut across the strip, upwards
    with tdgl.CurrentSampler(device, raster, device_id=options.device_id) as images, \
            tdgl.CurrentSampler(device, path, device_id=options.device_id) as cut:
        K = images.current_density(steps)  # [F, ny * nx, 2] in uA / um, zero in the hole
        ms = images.stats()["last_ms"]
        current = cut.path_current(steps)
        moment = cut.magnetic_moment(steps)
    maps = np.hypot(K[..., 0], K[..., 1]).reshape(len(steps), ny, nx)
    print(f"{len(steps)} saved steps of {len(device.points)} sites at {len(raster)} raster points: {ms:.3f} ms on the "
          f"device for all the maps")
    for t, image, i, m in zip(solution.times, maps, current, moment):
        print(f"t = {t:7.2f} tau_0: max |K| {image.max():8.3f} uA/um, I through the cut {i:7.3f} uA, M {m:9.4f} uA um^2")
    np.save("current_maps.npy", maps)
    solution.load_tdgl_data(-1)
    host = solution.current_through_path(path, with_units=False)
    print(f"|K| of every saved step [{len(steps)}, {ny}, {nx}] -> current_maps.npy; the host backend's current through "
          f"the cut at the last step: {host:.3f} uA")


if __name__ == "__main__":
    argv = sys.argv[1:]
    if "--bench" in argv:
        argv.remove("--bench")
        bench(argv)
    else:
        main(argv)
