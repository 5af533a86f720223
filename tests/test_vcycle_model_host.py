"""The float64 model of the stored-precision V-cycle (tests/vcycle_model.py) held to the host restatements of the cycle
before the device is held to the model (tests/test_hip_vcycle_stored.py).  No GPU.

Hierarchy: `synthetic_mesh(150)`, `max_coarse=40` -- 26,361 sites, levels 26361 / 2565 / 145 / 7, a "gwv" tail on level 1.

* unrounded, the model is `vcycle_collapsed_host` (6e-16 max |z| measured) and, with `tail_cycles=1` or no plan at all
  (every level a fused one), `vcycle_host`, within 1e-14 max |z|;
* the storage error s = max |z_rounded - z_exact| / max |z_exact| per probe column is positive, below 1e-6 in fp32
  (measured 4e-8 .. 1.1e-7) and below 5e-3 with binary16 on level 0 (3e-4 .. 7e-4): about 7 x of room, the bounds guard
  the model, not a kernel;
* sensitivity: with one mistake of a SELL / offset-form builder planted, the model leaves the GPU test's tolerance
  (`vcycle_model.within_tolerance`) on at least one probe column."""

import functools

import numpy as np
import pytest

import dense_reference as D
import vcycle_model as VM
from helpers import synthetic_mesh


@functools.lru_cache(maxsize=None)
def _setup():
    from tdgl_amd.amg import build_hierarchy, collapsed_operators

    mesh = synthetic_mesh(150)
    h = build_hierarchy(D.poisson_matrix_of(mesh), max_coarse=40)
    plans = {tc: collapsed_operators(h, 2, "chebyshev", 0.1, tail_cycles=tc) for tc in (1, 2)}
    B, names = VM.probe_columns(h, np.asarray(mesh.sites))
    return h, plans, B, names


@functools.lru_cache(maxsize=None)
def _answers(mode):
    """The model's answers on the probe columns, default plan: mode 0 exact, 1 fp32, 2 binary16 on level 0."""
    h, plans, B, _ = _setup()
    return VM.StoredCycle(h, plans[2], VM.Storage.mode(mode)).apply(B)


def teardown_module(module):
    for f in (_setup, _answers):
        f.cache_clear()


def test_the_hierarchy_is_the_one_the_figures_were_measured_on():
    h, plans, B, names = _setup()
    assert h.sizes == [26361, 2565, 145, 7]
    assert plans[2]["mode"] == "gwv" and plans[2]["tail"] == 1 and not plans[2]["mid"]
    assert B.shape[0] == 26361 and B.shape[1] == len(names) >= 16 and np.abs(B.mean(axis=0)).max() < 1e-15
    # the probe rows are distinct and cover both ends of the numbering and of the coarse numbering
    rows = VM.probe_rows(h)
    assert {0, 63, 64, 255, 256, 26360, 26361 // 64 * 64} <= set(rows)
    assert "aggregate 0" in rows.values() and "last aggregate" in rows.values()


def test_unrounded_model_is_the_host_cycle():
    from tdgl_amd.amg import vcycle_collapsed_host, vcycle_host

    h, plans, B, names = _setup()
    kw = dict(nu=2, smoother="chebyshev", nu_fine=1)
    z2 = _answers(0)
    z1 = VM.StoredCycle(h, plans[1]).apply(B)
    z0 = VM.StoredCycle(h, None).apply(B)
    worst = {}
    for j in range(B.shape[1]):
        host2 = vcycle_collapsed_host(h, plans[2], B[:, j], **kw)
        host = vcycle_host(h, B[:, j], **kw)
        for tag, got, want in (("collapsed", z2[:, j], host2), ("tail_cycles=1", z1[:, j], host), ("fused levels", z0[:, j], host)):
            d = np.abs(got - want).max() / np.abs(want).max()
            worst[tag] = max(worst.get(tag, 0.0), d)
            assert d <= 1e-14, (tag, names[j], d)
        # a column at a time and all at once give the same model
        assert np.abs(VM.StoredCycle(h, plans[2]).apply(B[:, j]) - z2[:, j]).max() <= 1e-14 * np.abs(z2[:, j]).max()
    print("unrounded model against the host cycle, max |dz| / max |z|:", {k: f"{v:.2g}" for k, v in worst.items()})
    # two cycles on the tail are another preconditioner than one
    assert np.abs(z2 - z1).max() > 1e-3 * np.abs(z1).max()


@pytest.mark.parametrize("mode, bound", [(1, 1e-6), (2, 5e-3)])
def test_storage_error_of_the_model(mode, bound):
    s = VM.storage_error(_answers(mode), _answers(0))
    print(f"storage mode {mode}: s = {s.min():.3g} .. {s.max():.3g} over {len(s)} columns")
    assert np.all(s > 0.0) and np.all(s < bound), (s.min(), s.max())
    # the rounded model holds fp32 numbers
    z = _answers(mode)
    assert np.array_equal(z, z.astype(np.float32).astype(np.float64))


def test_compare_counts_what_it_says():
    z = _answers(1)[:, :3]
    assert VM.within_tolerance(VM.compare(z, z)) and VM.compare(z, z)["ulps"] == 0.0
    one_up = np.nextafter(z.astype(np.float32), np.float32(np.inf)).astype(np.float64)
    c = VM.compare(one_up, z)
    assert c["excess"] == 0 and c["unequal"] == z.size and 0.99 <= c["ulps"] <= 1.01 and not VM.within_tolerance(c)
    two = z.copy()
    i = int(np.argmax(np.abs(z[:, 1])))
    two[i, 1] = z[i, 1] * (1 + 2.5 * VM.ULP32)
    c = VM.compare(two, z)
    assert c["excess"] == 1 and list(c["excess_columns"]) == [1] and not VM.within_tolerance(c)


def _fault_cases():
    h, _, _, _ = _setup()
    lv = h.levels[0]
    n = lv.A.shape[0]
    last_slice = (n - 1) // VM.WAVE
    padded = VM.sell_padded_rows(lv.A)
    return {
        "one column of a P row in the last slice moved by one": VM.Faults(p_column_shift_row=n - 1),
        "a padded SELL slot of A holds a value": VM.Faults(a_padded_slot_row=int(padded[len(padded) // 2])),
        "P's slice base off by one in the last slice": VM.Faults(p_slice_base_shift=last_slice),
        "P's slice base off by one in slice 4": VM.Faults(p_slice_base_shift=4),
        "dinv left unrounded": VM.Faults(dinv_unrounded=True),
    }


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("fault", ["one column of a P row in the last slice moved by one", "a padded SELL slot of A holds a value",
                                   "P's slice base off by one in the last slice", "P's slice base off by one in slice 4",
                                   "dinv left unrounded"])
def test_a_planted_fault_leaves_the_tolerance(fault, mode):
    h, plans, B, names = _setup()
    good = _answers(mode)
    bad = VM.StoredCycle(h, plans[2], VM.Storage.mode(mode), faults=_fault_cases()[fault]).apply(B)
    whole = VM.compare(bad, good)
    per_column = [VM.compare(bad[:, j], good[:, j]) for j in range(B.shape[1])]
    caught = [names[j] for j, c in enumerate(per_column) if not VM.within_tolerance(c)]
    print(f"mode {mode}, {fault}: {whole['excess']} entries beyond the bound, {whole['unequal']} of {whole['size']} not "
          f"bit-equal, largest deviation {whole['ulps']:.3g} fp32 units; caught on {len(caught)} of {len(names)} columns")
    assert caught, fault
    assert not VM.within_tolerance(whole)
