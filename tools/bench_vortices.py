"""Dev benchmark: vortex cores and boundary windings on the device (csrc/vortices.inc) next to the host backend.

    python tools/bench_vortices.py [--reps K] [--out FILE] [L ...]   # film side lengths in xi (70 / 460 / 920 -> 5.8k / 250k / 1M sites)

Per film and per number of frames F in {1, 32} one JSON line, printed and appended to FILE (default
profiles/VORTEX_bench.jsonl): the device time of one `VortexPlan.find` with records and windings (between the uploads
of psi and the read-back, `last_ms`), its wall time per frame including the upload of psi and the read-back, the wall
time per frame of the host backend (`tdgl_amd.vortices.host_find` + `loop_winding`, NumPy) for the same frames on the
same box, and the bytes the kernels must move per frame (16 n for psi once + 12 t for the triangles + t for the
orientation + 2 t for the charges written and read back) with the rate that gives at the device time.

psi is a lattice of vortices (a product would overflow; the phase is the sum of the cores' angles, the amplitude a
tanh profile per core) with about one core per 400 sites, so the record stream is what a vortex state gives.

    python tools/bench_vortices.py --link [--reps K] [--out FILE] [cores ...]   # cores per frame (100 / 1000 / 10000)

The link lines alone (`"link": true`), one per number of cores per frame, 32 frames of random clouds each: the device
time of one `VortexPlan.link` (between the upload of the records and the read-back), its wall time, the wall time of the
host backend `tdgl_amd.vortices.link_frames` for the same frames on the same box (timed on the first three frames and
scaled to all of them where all would take minutes; `host_frames_timed` says which) and their ratio.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, "tests"); sys.path.insert(0, "py-tdgl_amd"); sys.path.insert(0, ".")
from helpers import synthetic_mesh  # noqa: E402
from tdgl_amd.hipcore import VortexPlan  # noqa: E402
from tdgl_amd.vortices import boundary_loops, host_find, link_frames, loop_winding, triangle_orientations  # noqa: E402

args = sys.argv[1:]
reps, out_path = 3, os.path.join("profiles", "VORTEX_bench.jsonl")
for flag in ("--reps", "--out"):
    if flag in args:
        i = args.index(flag)
        if flag == "--reps":
            reps = int(args[i + 1])
        else:
            out_path = args[i + 1]
        del args[i:i + 2]


def vortex_state(sites, n_cores, rng):
    lo, hi = sites.min(axis=0), sites.max(axis=0)
    cores = rng.uniform(lo, hi, size=(n_cores, 2))
    theta, amp = np.zeros(len(sites)), np.ones(len(sites))
    for x0, y0 in cores:
        dx, dy = sites[:, 0] - x0, sites[:, 1] - y0
        theta += np.arctan2(dy, dx)
        amp *= np.tanh(np.hypot(dx, dy))
    return amp * np.exp(1j * theta)


def bench_link(cores, frames=32):
    """One line for linking `frames` random clouds of `cores` cores each (`VortexPlan.link`): a cloud of mean spacing 4
    in a square, every core displaced by a Gaussian step of 0.3 from frame to frame, about 2 % of the cores missing per
    frame, each frame in an order of its own; r = 1.5; the loop is the square's rim at spacing 1."""
    rng = np.random.default_rng(cores)
    side = 4.0 * np.sqrt(cores)
    home = rng.uniform(0, side, size=(cores, 2))
    charge = rng.choice([-1, 1], size=cores).astype(np.int32)
    per_frame = []
    for f in range(frames):
        home = home + 0.3 * rng.normal(size=home.shape)
        keep = rng.permutation(cores)[:cores - cores // 50]
        per_frame.append((home[keep], charge[keep]))
    counts = [len(c) for _, c in per_frame]
    xy, charges = np.concatenate([p for p, _ in per_frame]), np.concatenate([c for _, c in per_frame])
    k = int(np.ceil(side))
    edge = np.arange(k, dtype=float) * side / k
    rim = np.concatenate([np.column_stack([edge, 0 * edge]), np.column_stack([0 * edge + side, edge]),
                          np.column_stack([side - edge, 0 * edge + side]), np.column_stack([0 * edge, side - edge])])
    sites = np.concatenate([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], rim])
    with VortexPlan(sites, np.array([[0, 1, 2]], dtype=np.int32), [np.arange(3, len(sites))]) as plan:
        plan.link(counts, xy, charges, 1.5)  # warm-up: code object, buffers
        dev_ms, wall_s = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = plan.link(counts, xy, charges, 1.5)
            wall_s.append(time.perf_counter() - t0)
            dev_ms.append(plan.link_stats()["last_ms"])
        stats = plan.link_stats()
    # the host backend on the same box: all frames where that takes seconds, the first three otherwise (scaled by pairs)
    host_frames = frames if cores <= 1000 else 3
    t0 = time.perf_counter()
    host = link_frames(per_frame[:host_frames], 1.5, sites[3:])
    host_s = time.perf_counter() - t0
    n_host = sum(counts[:host_frames - 1])
    assert np.array_equal(host.next[:n_host], got[0][:n_host]) and np.array_equal(host.near[:n_host], got[4][:n_host])
    ms = float(np.min(dev_ms))
    host_ms = 1e3 * host_s * (frames - 1) / (host_frames - 1)
    return dict(link=True, cores_per_frame=cores, frames=frames, reps=reps, loop_sites=len(rim), links=stats["links"],
                pairs=stats["pairs"], launches=stats["launches"], device_ms=ms, device_ms_mean=float(np.mean(dev_ms)),
                wall_ms=1e3 * float(np.min(wall_s)), host_frames_timed=host_frames, host_wall_ms=host_ms,
                host_over_wall=host_ms / (1e3 * float(np.min(wall_s))), device_gpairs_per_s=stats["pairs"] / (ms * 1e-3) / 1e9)


if "--link" in args:  # the link lines alone:  --link [cores per frame ...]
    args.remove("--link")
    for cores in [int(a) for a in args] or [100, 1000, 10000]:
        line = bench_link(cores)
        print(json.dumps(line), flush=True)
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")
    sys.exit(0)

for L in [int(a) for a in args] or [70, 460, 920]:
    mesh = synthetic_mesh(L)
    sites, elements = np.asarray(mesh.sites), np.asarray(mesh.elements)
    n, t = len(sites), len(elements)
    loops = boundary_loops(mesh.edge_mesh.edges, mesh.edge_mesh.boundary_edge_indices, sites)
    rng = np.random.default_rng(L)
    base = vortex_state(sites, min(64, max(4, n // 400)), rng)
    orient = triangle_orientations(sites, elements)
    with VortexPlan(sites, elements, loops) as plan:
        for F in (1, 32):
            # distinct frames: a global phase and a small perturbation each
            psi = np.stack([base * np.exp(1j * rng.uniform(0, 2 * np.pi)) * (1 + 0.01 * rng.normal(size=n)) for _ in range(F)])
            plan.find(psi)  # warm-up: code object, buffers, the capacity
            dev_ms, wall_s = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                counts = plan.find(psi)[0]
                wall_s.append(time.perf_counter() - t0)
                dev_ms.append(plan.stats()["last_ms"])
            stats = plan.stats()
            host_frames = psi[:min(F, 2)]
            t0 = time.perf_counter()
            for frame in host_frames:
                host = host_find(frame, sites, elements, orient)
                for loop in loops:
                    loop_winding(frame, loop)
            host_s = (time.perf_counter() - t0) / len(host_frames)
            assert len(host.charges) == counts[len(host_frames) - 1]
            bytes_per_frame = 16 * n + 12 * t + t + 2 * t
            ms = float(np.min(dev_ms))
            line = dict(L=L, sites=n, triangles=t, loops=len(loops), loop_sites=int(sum(len(l) for l in loops)), frames=F,
                        reps=reps, cores_per_frame=float(np.mean(counts)), chunks=stats["chunks"], launches=stats["launches"],
                        device_ms=ms, device_ms_mean=float(np.mean(dev_ms)), device_ms_per_frame=ms / F,
                        wall_ms_per_frame=1e3 * float(np.min(wall_s)) / F, host_wall_ms_per_frame=1e3 * host_s,
                        bytes_per_frame=bytes_per_frame, device_gb_per_s=bytes_per_frame * F / (ms * 1e-3) / 1e9)
            print(json.dumps(line), flush=True)
            with open(out_path, "a") as f:
                f.write(json.dumps(line) + "\n")
