#!/usr/bin/env python
"""Aggregate throughput of `solve_ensemble` against the same runs made one after another with `tdgl.solve`.

    python tools/bench_ensemble.py --side 70 --replicas 32 --solve-time 20
    python tools/bench_ensemble.py --side 116 --replicas 32 --dense-max-sites 16000   # the dense inverse beyond its cap
    python tools/bench_ensemble.py --side 224 --replicas 32 --solve-time 5        # substructured factors, two levels
    python tools/bench_ensemble.py --side 70 --replicas 32 --ramp                 # field ramps evaluated on the device

Synthetic square film (`hex_jitter_points(side, side)`: side 70 = 5,791 sites, 100 = 11,774, 116 = 15,745, 140 ~ 23k,
224 ~ 59k, 320 ~ 120k) in a uniform field, one field per replica spread over [b_min, b_max].  Prints ONE JSON line:
  replicas, sites, replica_steps_per_s   the ensemble's loop (set-up excluded): accepted steps of all replicas / s
  sequential_steps_per_s                 `TDGLSolver.solve` (the product's single-run path) of the first
                                         `--sequential` replicas, one after another, set-up excluded
  speedup                                replica_steps_per_s / sequential_steps_per_s
  round_us, rounds                       mean wall time of one round (one attempt of every live replica)
  mu_levels                              the ensemble's mu solve: 0 = dense inverse, 1 or 2 = substructured levels
  factor_bytes_per_round                 bytes of the factors one round streams (dense tiles once per 16 replicas,
                                         the levels' pools once per 8)
  factor_GBps_if_whole_round             those bytes / round_us: a floor on the mu solve's achieved bandwidth
  max_dev_*                              largest deviation of any sequentially-run replica from its ensemble copy
With --ramp every replica's field is LinearRamp(tmin=0, tmax=T/2, final=b_r) x the uniform field, held after T/2
(T = --solve-time); the numbers above are then those of the ramped runs (sequential: tdgl.solve of the same ramps),
and it adds
  static_round_us                        round_us of the same ensemble with the static fields b_r
  ramp_round_us, settled_round_us        round_us of the ramped ensemble over [0, T/2] (every replica ramping) and
                                         over (T/2, T] (every ramp settled): the difference of a run to T/2 and one
                                         to T
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "py-tdgl_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=70)
    ap.add_argument("--replicas", type=int, default=32)
    ap.add_argument("--solve-time", type=float, default=20.0)
    ap.add_argument("--b-min", type=float, default=0.1)
    ap.add_argument("--b-max", type=float, default=0.6)
    ap.add_argument("--sequential", type=int, default=4, help="replicas also run one after another (their rate is the baseline)")
    ap.add_argument("--max-sites", type=int, default=None, help="raise ENSEMBLE_MAX_SITES (to measure beyond the cap)")
    ap.add_argument("--dense-max-sites", type=int, default=None, help="set ENSEMBLE_DENSE_MAX_SITES (the dense / substructured crossover)")
    ap.add_argument("--ramp", action="store_true", help="ramp each replica's field over the first half of the run")
    args = ap.parse_args()

    from tdgl_amd import SolverOptions, TDGLSolver, ensemble
    from tdgl_amd.ensemble import ensemble_dimensionless

    if args.max_sites is not None:
        ensemble.ENSEMBLE_MAX_SITES = args.max_sites
    if args.dense_max_sites is not None:
        ensemble.ENSEMBLE_DENSE_MAX_SITES = args.dense_max_sites
        ensemble.ENSEMBLE_MAX_SITES = max(ensemble.ENSEMBLE_MAX_SITES, args.dense_max_sites)
    from tdgl_amd.finite_volume import Mesh
    from tdgl_amd.meshgen import hex_jitter_points, triangulate

    pts = hex_jitter_points(args.side, args.side)
    mesh = Mesh.from_triangulation(pts, triangulate(pts))
    n = len(mesh.sites)
    c = mesh.edge_mesh.centers
    xc, yc = c[:, 0].min() + np.ptp(c[:, 0]) / 2, c[:, 1].min() + np.ptp(c[:, 1]) / 2

    def A(b):
        return np.column_stack([-b * (c[:, 1] - yc) / 2, b * (c[:, 0] - xc) / 2])

    R = args.replicas
    fields = np.linspace(args.b_min, args.b_max, R)

    def ramp(b):  # A(t) = LinearRamp(0, T/2, 0 -> 1)(t) x A(b)
        return (A(b), dict(tmin=0.0, tmax=args.solve_time / 2, initial=0.0, final=1.0))

    def run(solve_time, ramped):
        opts = SolverOptions(solve_time=solve_time, save_every=100_000)
        if ramped:
            solver = ensemble_dimensionless(mesh, opts, [None] * R, vector_potential_ramp=[ramp(b) for b in fields])
        else:
            solver = ensemble_dimensionless(mesh, opts, [A(b) for b in fields])
        t0 = time.perf_counter()
        sols = solver.solve()
        return solver, sols, time.perf_counter() - t0 - solver.setup_seconds

    extra = {}
    if args.ramp:
        s_static, _, loop_static = run(args.solve_time, False)
        s_half, _, loop_half = run(args.solve_time / 2, True)
        extra["static_round_us"] = round(1e6 * loop_static / max(s_static.ensemble_stats["rounds"], 1), 2)
        extra["ramp_round_us"] = round(1e6 * loop_half / max(s_half.ensemble_stats["rounds"], 1), 2)
    opts = SolverOptions(solve_time=args.solve_time, save_every=100_000)
    solver, sols, loop = run(args.solve_time, args.ramp)
    steps = sum(len(s.dynamics.dt) for s in sols)
    rounds = solver.ensemble_stats["rounds"]
    if args.ramp:
        extra["settled_round_us"] = round(1e6 * (loop - loop_half) / max(rounds - s_half.ensemble_stats["rounds"], 1), 2)

    seq_steps, seq_time, dev = 0, 0.0, dict(dt=0.0, abs_psi2=0.0, mu=0.0, js=0.0)
    for r in range(min(args.sequential, R)):
        if args.ramp:
            one = TDGLSolver.from_dimensionless(mesh, opts, 0.0 * A(fields[r]), vector_potential_ramp=ramp(fields[r])).solve()
        else:
            one = TDGLSolver.from_dimensionless(mesh, opts, A(fields[r])).solve()
        seq_steps += len(one.dynamics.dt)
        seq_time += one.total_seconds
        a, b = sols[r], one
        k = min(len(a.dynamics.dt), len(b.dynamics.dt))
        dev["dt"] = max(dev["dt"], float(np.abs(a.dynamics.dt[:k] - b.dynamics.dt[:k]).max() / b.dynamics.dt.max())
                        if len(a.dynamics.dt) == len(b.dynamics.dt) else float("inf"))
        x, y = a.tdgl_data, b.tdgl_data
        dev["abs_psi2"] = max(dev["abs_psi2"], float(np.abs(np.abs(x.psi) ** 2 - np.abs(y.psi) ** 2).max()))
        dev["mu"] = max(dev["mu"], float(np.abs((x.mu - x.mu.mean()) - (y.mu - y.mu.mean())).max()))
        dev["js"] = max(dev["js"], float(np.abs(x.supercurrent - y.supercurrent).max()))

    levels, factor_bytes = solver.mu_path
    ens_rate = steps / loop
    seq_rate = seq_steps / seq_time if seq_time > 0 else float("nan")
    round_us = 1e6 * loop / max(rounds, 1)
    print(json.dumps(dict(
        metric="ensemble replica-steps/s vs sequential tdgl.solve", replicas=R, sites=n, solve_time=args.solve_time,
        replica_steps=steps, loop_seconds=round(loop, 4), setup_seconds=round(solver.setup_seconds, 3),
        replica_steps_per_s=round(ens_rate, 1), sequential_runs=min(args.sequential, R), sequential_steps_per_s=round(seq_rate, 1),
        speedup=round(ens_rate / seq_rate, 2), rounds=rounds, batches=solver.ensemble_stats["batches"], round_us=round(round_us, 2),
        mu_levels=levels, factor_bytes_per_round=factor_bytes,
        factor_GBps_if_whole_round=round(factor_bytes / (round_us * 1e-6) / 1e9, 1),
        steps_min=min(len(s.dynamics.dt) for s in sols), steps_max=max(len(s.dynamics.dt) for s in sols),
        max_dev_dt_rel=dev["dt"], max_dev_abs_psi2=dev["abs_psi2"], max_dev_mu=dev["mu"], max_dev_js=dev["js"],
        ramp=args.ramp, **extra,
    )))


if __name__ == "__main__":
    main()
