"""GPU tests of the core records taken inside the time loops (csrc/census.inc, ``tdgl_set_core_records``,
``SolverOptions.vortex_cores``): after every recorded accepted step one record per charged triangle of the live psi --
triangle, charge, position --, out of the census' own launch.

The model is `tdgl_amd.vortices.host_find` on the context's own psi after the step (tests/cores_model.py): triangles and
charges are compared exactly and in order (both sides apply the same comparisons of separately rounded products to the
same doubles, and the host sorts a step's records by triangle), positions within the bound of DESIGN.md section 3,
``8 u (kappa + 1) r_max`` (`vortex_model.position_bound`).  Inputs: tests/census_model.py; tests/test_cores_host.py
asserts on the CPU that they hold what these tests rely on, so none passes on empty records.
"""

import ctypes as C

import numpy as np
import pytest

import census_model as M
import cores_model as CM
import vortex_model as VM
from test_hip_census import LOOPS, _begin, _ring_device, _set_census, _solver, _spiked_epsilon

pytestmark = pytest.mark.gpu

CAPACITY = 4096


def _cores_on(ctx, p, capacity=CAPACITY, every=1):
    _set_census(ctx, p)
    ctx.set_core_records(p["mesh"].sites, capacity, every)


def _assert_frame(got, psi, mesh, what):
    """One recorded step against `host_find` on its psi."""
    want = CM.cores_of_states([psi], mesh)[0]
    assert np.array_equal(got.triangles, want.triangles), (what, got.triangles, want.triangles)
    assert np.array_equal(got.charges, want.charges), what
    bound = VM.position_bound(np.asarray(psi), mesh.sites, mesh.elements, want.triangles)
    err = np.abs(got.positions - want.positions).max(axis=1) if len(want.charges) else np.zeros(0)
    assert np.all(err <= bound), (what, err, bound)
    return len(want.charges)


def _stepwise(ctx, p, n_steps):
    """``n_steps`` calls of ``run(1)``, each followed by `get_state` and compared with the model; the calls' records
    joined as one run's would be."""
    parts, dts, counts = [], [], []
    for k in range(n_steps):
        res = ctx.run(1)
        cores = res["cores"]
        assert list(cores["steps"]) == [0] and cores["complete"].all(), k
        assert cores["counts"][0] == res["census"][0, :2].sum()
        counts.append(_assert_frame(CM.frames_of(cores)[0], ctx.get_state()["psi"], p["mesh"], k))
        parts.append(dict(cores, steps=cores["steps"] + k))
        dts.append(res["dt"][0])
    joined = {key: np.concatenate([c[key] for c in parts]) for key in parts[0]}
    return joined, np.array(dts), np.array(counts)


# ------------------------------------------------------------------ 1. own state, three loops
@pytest.mark.parametrize("name, max_blocks", [("A", None), ("B", None), ("B", 2)], ids=["A", "B", "B_two_workgroups"])
def test_records_equal_host_find_on_the_own_state_in_every_loop(name, max_blocks, monkeypatch, request):
    """120 steps, one call per step: every step's records equal `host_find` on that call's psi; the same steps in one
    call give the same bytes; run-ahead and classic are byte-identical.  With the workgroup cap at 2, input B's 1.9k
    triangles take four trips through the stride loop."""
    p = M.problem(name)
    if max_blocks is None:
        monkeypatch.delenv("TDGL_CENSUS_MAX_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("TDGL_CENSUS_MAX_BLOCKS", str(max_blocks))
        assert len(p["mesh"].elements) > 3 * 256 * max_blocks
    n_steps = 120
    records = {}
    for loop in LOOPS:
        ctx = _solver(p, loop, monkeypatch, request).ctx
        try:
            _cores_on(ctx, p)
            _begin(ctx, p)
            joined, dts, counts = _stepwise(ctx, p, n_steps)
            _begin(ctx, p)
            once = ctx.run(n_steps)
            assert np.array_equal(once["dt"], dts), loop
            assert np.array_equal(once["cores"]["steps"], np.arange(n_steps))
            assert CM.records_bytes(once["cores"]) == CM.records_bytes(joined), loop
            records[loop] = CM.records_bytes(joined)
            print(f"{name}, {loop}: cores per step {counts.min()} .. {counts.max()}, {counts.sum()} records")
            assert counts.max() >= 1 and len(set(counts.tolist())) >= 2  # (not empty, not constant)
            if name == "A":
                assert {1, -1} <= set(joined["charges"].tolist())
        finally:
            ctx.close()
    assert records["run_ahead"] == records["classic"]


# ------------------------------------------------------------------ 2. dense state, 3. overflow
def _dense_steps(ctx, p, psi0, n_calls=3):
    _begin(ctx, p, psi0=psi0)
    out = []
    for k in range(n_calls):
        res = ctx.run(1)
        out.append((res, ctx.get_state()["psi"]))
    return out


@pytest.mark.parametrize("loop", ["run_ahead", "classic"])
def test_dense_state_many_hits_in_every_wave(loop, monkeypatch, request):
    """psi_0 random on input B's mesh: hundreds of cores per step, many per wavefront and some in every wavefront."""
    monkeypatch.delenv("TDGL_CENSUS_MAX_BLOCKS", raising=False)
    p = M.problem("B")
    mesh = p["mesh"]
    ctx = _solver(p, loop, monkeypatch, request).ctx
    try:
        _cores_on(ctx, p)
        for k, (res, psi) in enumerate(_dense_steps(ctx, p, CM.dense_psi0(mesh))):
            cores = res["cores"]
            assert cores["complete"].all() and list(cores["steps"]) == [0]
            n = _assert_frame(CM.frames_of(cores)[0], psi, mesh, k)
            print(f"{loop}: step {k}: {n} cores")
            assert n > 64 and n == res["census"][0, :2].sum()
    finally:
        ctx.close()


@pytest.mark.parametrize("loop", ["run_ahead", "classic"])
def test_overflow_marks_the_rest_of_the_window_incomplete(loop, monkeypatch, request):
    monkeypatch.delenv("TDGL_CENSUS_MAX_BLOCKS", raising=False)
    p = M.problem("B")
    mesh = p["mesh"]
    psi0 = CM.dense_psi0(mesh)
    ctx = _solver(p, loop, monkeypatch, request).ctx
    try:
        _cores_on(ctx, p)
        full = _dense_steps(ctx, p, psi0)
        counts = [int(res["cores"]["counts"][0]) for res, _ in full]
        capacity = counts[0] + counts[1] // 2  # between the first step's count and the sum of two
        assert counts[0] < capacity < counts[0] + counts[1]
        runs = []
        for _ in range(2):
            _cores_on(ctx, p, capacity=capacity)
            _begin(ctx, p, psi0=psi0)
            res = ctx.run(3)  # one window: no flush between the steps
            after = ctx.run(1)  # behind the flush that ended the call above
            psi_after = ctx.get_state()["psi"]
            runs.append((res, after))
        res, after = runs[0]
        cores = res["cores"]
        assert list(cores["steps"]) == [0, 1, 2]
        assert list(cores["complete"]) == [True, False, False] and list(cores["counts"]) == [counts[0], 0, 0]
        assert np.array_equal(res["census"][:, :2].sum(axis=1), counts)  # the counts stay exact
        assert np.array_equal(res["census"], np.concatenate([r["census"] for r, _ in full]))
        first = CM.frames_of(full[0][0]["cores"])[0]
        got = CM.frames_of(cores)[0]
        assert np.array_equal(got.triangles, first.triangles) and np.array_equal(got.charges, first.charges)
        assert np.array_equal(got.positions, first.positions)
        assert after["cores"]["complete"].all() and after["cores"]["counts"][0] == after["census"][0, :2].sum() > 64
        _assert_frame(CM.frames_of(after["cores"])[0], psi_after, mesh, "after the flush")
        assert CM.records_bytes(runs[1][0]["cores"]) == CM.records_bytes(cores)
        assert CM.records_bytes(runs[1][1]["cores"]) == CM.records_bytes(after["cores"])
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. a failed attempt writes no record
@pytest.mark.parametrize("loop", ["run_ahead", "classic"])
def test_a_failed_attempt_writes_no_record(loop, monkeypatch, request):
    monkeypatch.delenv("TDGL_CENSUS_MAX_BLOCKS", raising=False)
    p = M.problem("A")
    n_steps = 30
    ctx = _solver(p, loop, monkeypatch, request, epsilon=_spiked_epsilon(p)).ctx
    try:
        _cores_on(ctx, p)
        _begin(ctx, p)
        joined, dts, counts = _stepwise(ctx, p, n_steps)
        assert ctx.step_stats()["psi_retries"] >= 1 and counts.sum() > 0
        _begin(ctx, p)
        once = ctx.run(n_steps)
        stats = ctx.step_stats()
        print(f"{loop}: {stats['psi_retries']} repeated updates in {stats['steps']} steps, {counts.sum()} records")
        assert stats["psi_retries"] >= 1 and stats["steps"] == n_steps == len(once["dt"])
        assert np.array_equal(once["dt"], dts)
        assert CM.records_bytes(once["cores"]) == CM.records_bytes(joined)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. across a flush of the ring
@pytest.mark.parametrize("probes", [None, (3, 77)], ids=["no_probes", "probes"])
@pytest.mark.parametrize("loop", ["run_ahead", "classic"])
def test_records_across_a_flush_of_the_ring(loop, probes, monkeypatch, request):
    """1,100 steps of the 189-site input in one call (the ring holds 1,024) against the same run in calls of 100."""
    monkeypatch.delenv("TDGL_CENSUS_MAX_BLOCKS", raising=False)
    p = M.problem("A12")
    n_steps = 1100
    ctx = _solver(p, loop, monkeypatch, request, probes=probes).ctx
    try:
        _begin(ctx, p)
        ctx.run(300)  # (the run-ahead loop's batches have grown to their full length: the runs below start alike)
        runs = {}
        for cores in (True, False):
            _set_census(ctx, p)
            if cores:
                ctx.set_core_records(p["mesh"].sites, CAPACITY)
            _begin(ctx, p)
            res = ctx.run(n_steps)
            runs[cores] = (res, ctx.step_stats()["host_syncs"])
        once = runs[True][0]
        assert runs[False][0]["cores"] is None
        assert np.array_equal(once["census"], runs[False][0]["census"]) and np.array_equal(once["dt"], runs[False][0]["dt"])
        n_flushes = 2  # at 1,024 rows and when the call ends
        print(f"{loop}, probes {probes}: host synchronisations {runs[True][1]} with the records, {runs[False][1]} census only")
        assert runs[True][1] <= runs[False][1] + n_flushes
        cores = once["cores"]
        assert np.array_equal(cores["steps"], np.arange(n_steps)) and cores["complete"].all()
        assert np.array_equal(cores["counts"], once["census"][:, :2].sum(axis=1))
        assert (cores["counts"] >= 1).all()  # (the vortex lasts: test_cores_host.py)
        _cores_on(ctx, p)
        _begin(ctx, p)
        parts, at = [], 0
        for _ in range(n_steps // 100):
            r = ctx.run(100)
            parts.append(dict(r["cores"], steps=r["cores"]["steps"] + at))
            at += len(r["dt"])
        joined = {key: np.concatenate([c[key] for c in parts]) for key in parts[0]}
        assert CM.records_bytes(joined) == CM.records_bytes(cores)
        _assert_frame(CM.frames_of(parts[-1])[-1], ctx.get_state()["psi"], p["mesh"], "the last step")
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6. every
@pytest.mark.parametrize("loop", ["run_ahead", "classic"])
def test_every_third_running_index_across_calls(loop, monkeypatch, request):
    monkeypatch.delenv("TDGL_CENSUS_MAX_BLOCKS", raising=False)
    p = M.problem("A")
    calls = (10, 7, 13)
    ctx = _solver(p, loop, monkeypatch, request).ctx
    try:
        out = {}
        for every in (1, 3):
            _cores_on(ctx, p, every=every)
            _begin(ctx, p)
            frames, at = {}, 0
            for n in calls:
                res = ctx.run(n)
                assert len(res["dt"]) == n and len(res["census"]) == n  # (rows at every step)
                for s, f in zip(res["cores"]["steps"], CM.frames_of(res["cores"])):
                    frames[at + int(s)] = f
                at += n
            out[every] = frames
        assert sorted(out[1]) == list(range(sum(calls)))
        assert sorted(out[3]) == [k for k in range(sum(calls)) if k % 3 == 0]
        n_records = 0
        for k, f in out[3].items():
            want = out[1][k]
            assert np.array_equal(f.triangles, want.triangles) and np.array_equal(f.charges, want.charges), k
            assert np.array_equal(f.positions, want.positions), k
            n_records += len(f.charges)
        assert n_records > 0
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7. the records change nothing
@pytest.mark.parametrize("loop", ["run_ahead", "classic"])
@pytest.mark.parametrize("name, n_steps", [("A", 100), ("B", 120)])
def test_records_change_no_output(name, n_steps, loop, monkeypatch, request):
    monkeypatch.delenv("TDGL_CENSUS_MAX_BLOCKS", raising=False)
    p = M.problem(name)
    ctx = _solver(p, loop, monkeypatch, request, probes=(1, len(p["mesh"].sites) // 2)).ctx
    try:
        out = {}
        for mode in ("census", "cores", "off_again"):
            if mode == "census":
                _set_census(ctx, p)
            elif mode == "cores":
                ctx.set_core_records(p["mesh"].sites, CAPACITY)
            else:
                ctx.set_core_records(None, 0)
            _begin(ctx, p)
            out[mode] = (ctx.run(n_steps), ctx.get_state())
        assert out["census"][0]["cores"] is None and out["off_again"][0]["cores"] is None
        assert len(out["cores"][0]["cores"]["steps"]) == n_steps and len(out["cores"][0]["cores"]["charges"]) > 0
        for mode in ("cores", "off_again"):
            for key in ("dt", "mu", "theta", "census"):
                assert np.array_equal(out["census"][0][key], out[mode][0][key]), (mode, key)
            for key in ("psi", "mu", "supercurrent", "normal_current"):
                assert np.array_equal(out["census"][1][key], out[mode][1][key]), (mode, key)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 8. arguments and switching
def test_bad_arguments_switching_and_true_counts(monkeypatch, request):
    from tdgl_amd import _lib
    from tdgl_amd.hipcore import TDGLContext
    from tdgl_amd.partition import build_local_problem, rcb_partition

    monkeypatch.delenv("TDGL_CENSUS_MAX_BLOCKS", raising=False)
    p = M.problem("A")
    mesh, loops = p["mesh"], p["loops"]
    lib = _lib.load()
    ctx = _solver(p, "run_ahead", monkeypatch, request).ctx
    try:
        with pytest.raises(ValueError, match="census"):  # no census
            ctx.set_core_records(mesh.sites, 100)
        ctx.set_census(None, None, loops)
        with pytest.raises(ValueError, match="triangles"):  # a census without triangles
            ctx.set_core_records(mesh.sites, 100)
        _cores_on(ctx, p, capacity=CAPACITY, every=2)
        for args, text in (((mesh.sites, -1, 1), "capacity"), ((mesh.sites, 100, 0), "every"), ((None, 100, 1), "null")):
            with pytest.raises(ValueError, match=text):
                ctx.set_core_records(*args)
        # the previous state stays: every second step
        _begin(ctx, p)
        res = ctx.run(50)
        cores = res["cores"]
        assert np.array_equal(cores["steps"], np.arange(0, 50, 2)) and cores["counts"].sum() > 0
        # capacities below the numbers: the true numbers, the first entries only; capacity 0: the numbers alone
        ns, nr = C.c_int64(-1), C.c_int64(-1)
        assert lib.tdgl_get_core_records(ctx._ctx, 0, None, None, None, 0, None, None, None, C.byref(ns), C.byref(nr)) == 0
        assert ns.value == 25 and nr.value == cores["counts"].sum() == len(cores["charges"])
        step, count = np.full(6, -5, dtype=np.int64), np.full(6, -5, dtype=np.int64)
        complete = np.full(6, -5, dtype=np.int32)
        tri, chg, xy = np.full(4, -5, dtype=np.int32), np.full(4, -5, dtype=np.int32), np.full((4, 2), -5.0)
        assert lib.tdgl_get_core_records(ctx._ctx, 3, _lib.p_i64(step), _lib.p_i64(count), _lib.p_i32(complete), 2, _lib.p_i32(tri),
                                         _lib.p_i32(chg), _lib.p_f64(xy), C.byref(ns), C.byref(nr)) == 0
        assert ns.value == 25 and nr.value == len(cores["charges"])
        assert list(step[:3]) == [0, 2, 4] and np.all(step[3:] == -5) and np.array_equal(count[:3], cores["counts"][:3])
        assert np.all(complete[:3] == 1) and np.all(complete[3:] == -5)
        assert np.array_equal(tri[:2], cores["triangles"][:2]) and np.all(tri[2:] == -5) and np.all(xy[2:] == -5.0)
        assert lib.tdgl_get_core_records(ctx._ctx, 3, None, None, None, 0, None, None, None, C.byref(ns), C.byref(nr)) != 0
        # tdgl_set_census switches the records off
        _set_census(ctx, p)
        _begin(ctx, p)
        again = ctx.run(50)
        assert again["cores"] is None and np.array_equal(again["census"], res["census"])
        assert lib.tdgl_get_core_records(ctx._ctx, 0, None, None, None, 0, None, None, None, C.byref(ns), C.byref(nr)) == 0
        assert ns.value == 0 and nr.value == 0
    finally:
        ctx.close()
    # a rank of a one-process-per-GPU run refuses
    lp = build_local_problem(mesh, rcb_partition(mesh.sites, 2), 0)
    ctx = TDGLContext(lp.mesh, n_owned=lp.n_own)
    try:
        with pytest.raises(ValueError, match="one-process-per-GPU"):
            ctx.set_core_records(np.zeros((ctx.n, 2)), 100)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 9. public surface
def test_solve_with_vortex_cores(direct_solve):
    import tdgl_amd as tdgl

    device = _ring_device()
    # (2.5 mT on this film: vortices and antivortices appear from about step 26 on, tests/test_hip_census.py)
    kw = dict(solve_time=0.3, dt_init=1e-3, dt_max=0.1, save_every=1, field_units="mT")
    field = 2.5
    solution = tdgl.solve(device, tdgl.SolverOptions(vortex_cores=True, **kw), applied_vector_potential=field)
    dyn = solution.dynamics
    vc = dyn.vortex_cores
    k_steps = len(dyn.dt)
    assert isinstance(vc, tdgl.VortexCores) and len(vc) == k_steps >= 40 and vc.complete.all()
    assert np.array_equal(vc.steps, np.arange(k_steps)) and np.array_equal(vc.times, dyn.time + dyn.dt)
    assert dyn.vortex_counts is not None and np.array_equal(vc.counts, dyn.vortex_counts.sum(axis=0))
    assert vc.counts.sum() > 0
    # (save_every = 1: saved step j holds psi after j steps; the step that ends the loop is not saved)
    assert len(solution.saved_steps) == k_steps
    elements = np.asarray(device.triangles)
    for k in range(k_steps - 1):
        solution.solve_step = k + 1
        want, got = solution.vortices(), vc.frame(k)
        assert np.array_equal(got.triangles, want.triangles) and np.array_equal(got.charges, want.charges), k
        bound = VM.position_bound(solution.tdgl_data.psi, device.points, elements, want.triangles)
        err = np.abs(got.positions - want.positions).max(axis=1) if len(want.charges) else np.zeros(0)
        assert np.all(err <= bound), (k, err, bound)
    # tracks from the records, psi never uploaded: host and hip give identical links
    r = 0.5
    host = vc.tracks(r, last=k_steps - 2)
    hip = vc.tracks(r, backend="hip", last=k_steps - 2)
    for a, b in zip(host.links, hip.links):
        assert np.array_equal(a, b)
    # ... and the tracks of the saved steps 1 .. k_steps - 1, which hold the same states
    saved = tdgl.track_vortices(device, list(solution.saved_steps)[1:], r)
    assert len(host) == len(saved) > 0
    print(f"solve: {k_steps} steps, {vc.counts.sum()} records, {len(host)} tracks")
    for a, b in zip(host, saved):
        assert a.charge == b.charge and np.array_equal(a.frame_indices, b.frame_indices)
        assert np.allclose(a.times, b.times, rtol=1e-12, atol=0.0)  # (the state's time: that of the saved step)
    # off: no records, the same steps
    off = tdgl.solve(device, tdgl.SolverOptions(**kw), applied_vector_potential=field)
    assert off.dynamics.vortex_cores is None and off.dynamics.vortex_counts is None
    assert np.array_equal(off.dynamics.dt, dyn.dt)
    # refusals by name
    with pytest.raises(tdgl.SolverOptionsError, match="vortex_cores"):
        tdgl.solve_ensemble(device, tdgl.SolverOptions(vortex_cores=True, **kw), applied_vector_potential=[field, 0.0])
    from tdgl_amd.distributed import DistributedTDGL

    p = M.problem("A")
    with pytest.raises(tdgl.SolverOptionsError, match="vortex_cores"):
        DistributedTDGL(p["mesh"], tdgl.SolverOptions(solve_time=1.0, vortex_cores=True), p["A"], rank=0, world=1)
