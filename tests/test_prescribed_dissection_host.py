"""The prescribed dissection and the float64 model of the stored factors (tests/prescribed_dissection.py), on the host:
what tests/test_hip_sub_prescribed.py holds the factor kernels against must itself be right, and its criterion must be
able to fail."""

import functools

import numpy as np
import pytest

import dense_reference as D
import prescribed_dissection as P
from tdgl_amd import substructure


@functools.lru_cache(maxsize=None)
def _layout(name, K):
    return P.build_layout(name, K)


@functools.lru_cache(maxsize=None)
def _reference(lx):
    """(A, G, kappa) of `synthetic_mesh(lx)` in site order, once per module (the inverse takes seconds)."""
    from helpers import synthetic_mesh

    A = D.poisson_matrix_of(synthetic_mesh(lx))
    G = D.pinv_reference(A)
    return A, G, D.condition_number(A, G)


def teardown_module(module):
    _layout.cache_clear()
    _reference.cache_clear()


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("name", list(P.LAYOUTS))
def test_parts_have_exactly_the_prescribed_sizes(name, K):
    """``perm`` is a permutation, the parts have the sizes of the lists, cycled (the sweep's last, unfilled, part is
    separator), the pointer arrays are absolute and of the product's dtypes, and `build_substructure_levels` accepts
    the dissection (it raises where a cut edge does not end in the separator)."""
    lay = _layout(name, K)
    assert lay.perm.dtype == np.int32 and np.array_equal(np.sort(lay.perm), np.arange(lay.n))
    assert len(lay.ptrs) == K and lay.ptrs[0][0] == 0
    for k, (ptr, sizes) in enumerate(zip(lay.ptrs, lay.lists)):
        assert ptr.dtype == np.int32
        got = np.diff(ptr)
        assert len(got) >= min(len(sizes), 3), (k, got)
        assert np.array_equal(got, [sizes[p % len(sizes)] for p in range(len(got))]), (k, got)
        if k:
            assert ptr[0] == lay.ptrs[k - 1][-1]
    assert lay.ptrs[-1][-1] <= lay.n - 2
    assert len(lay.levels) == K and lay.levels[-1].schur is not None
    for lv, ptr in zip(lay.levels, lay.ptrs):
        assert lv.n_parts == len(ptr) - 1 and min(len(s) for s in lv.sep_idx) >= 1
    if name == "mixed" and K == 3:  # (the figures of the layout's first trial)
        assert [lv.n_parts for lv in lay.levels] == [31, 12, 7] and [lv.n_sep for lv in lay.levels] == [1584, 1165, 906]
        assert P.describe(lay.levels)[0]["touch"] == (3, 146)


def test_apply_levels_is_solve_host_levels_bit_for_bit():
    lay = _layout("mixed", 3)
    rng = np.random.default_rng(1)
    for sparse_sep in (True, False):
        b = rng.standard_normal(lay.n)
        assert np.array_equal(P.apply_levels(lay.levels, lay.G_top, b, sparse_sep),
                              substructure.solve_host_levels(lay.levels, b, sparse_sep=sparse_sep, remove_mean=False))
    # ... and column by column the same as on a block of columns, to a few ulps of the result
    B = P.probe_columns(lay.ptrs, lay.n)[:, -6:]
    X = P.apply_levels(lay.levels, lay.G_top, B)
    for j in range(B.shape[1]):
        x = P.apply_levels(lay.levels, lay.G_top, B[:, j])
        assert np.abs(X[:, j] - x).max() <= 1e-13 * np.abs(x).max()


@pytest.mark.parametrize("name, K", [("mixed", 1), ("mixed", 2), ("mixed", 3), ("tiles256", 3), ("lanes2048", 3)])
def test_host_factors_match_the_float64_pseudo_inverse(name, K):
    """`solve_host_levels` on the probe columns against `dense_reference.apply_reference` within the kappa-derived
    tolerance (8 kappa u max |x|, ~2e-12 of max |x| at 4.3k sites; measured 2e-14 .. 6e-14)."""
    lay = _layout(name, K)
    A, G, kappa = _reference(P.LAYOUTS[name][0])
    B = P.probe_columns(lay.ptrs, lay.n)
    B -= B.mean(axis=0)
    x_ref = D.apply_reference(A, B[lay.iperm], G)
    worst = 0.0
    for j in range(B.shape[1]):
        x = substructure.solve_host_levels(lay.levels, B[:, j])[lay.iperm]
        err = np.abs(x - x_ref[:, j]).max()
        worst = max(worst, err / np.abs(x_ref[:, j]).max())
        assert err <= D.tolerance(kappa, x_ref[:, j]), (j, err)
    print(f"\n{name}, {K} levels: kappa {kappa:.4g}, worst max |x - x_ref| / max |x_ref| = {worst:.3g} "
          f"(bound {D.C_TOL * kappa * D.U:.3g})")


def storage_error(lay, B):
    """Per column of ``B``: ``s = max |apply(rounded) - apply(exact)| / max |apply(exact)|`` and the two results."""
    l32, G32 = P.rounded_to_storage(lay.levels, lay.G_top)
    exact = P.apply_levels(lay.levels, lay.G_top, B)
    rounded = P.apply_levels(l32, G32, B)
    return np.abs(rounded - exact).max(axis=0) / np.abs(exact).max(axis=0), rounded, (l32, G32)


@pytest.mark.parametrize("name", ["mixed", "tiles256", "tiles192", "tiles128", "tiles64", "lanes2048"])
def test_storage_error_is_positive_for_every_probe_column(name):
    """No tolerance of the device test is ever zero: rounding the stored arrays to float32 moves every probe column's
    answer (measured over the six layouts: 1e-8 .. 6e-8 of max |z|, the random columns 3e-8 .. 6e-8), and never by more than a few float32
    round-offs."""
    lay = _layout(name, 3)
    s, _, _ = storage_error(lay, P.probe_columns(lay.ptrs, lay.n))
    print(f"\n{name}: s from {s.min():.3g} to {s.max():.3g}; random columns {s[-4:].min():.3g} .. {s[-4:].max():.3g}")
    assert np.all(s > 0.0) and np.all(s < 1e-6), s
    _, _, kappa = _reference(P.LAYOUTS[name][0])
    assert np.all(s[-4:] > 100 * D.C_TOL * kappa * D.U)  # (the random columns: s, not the floor, is the bound there)


def _mutated(levels32, which):
    """The rounded factors with one defect of the kind a sweep kernel can have."""
    import copy

    out = [copy.copy(lv) for lv in levels32]
    if which == "dropped column":  # the last column of one level-1 G_p (the tail of a chunk)
        lv, p = out[0], int(np.argmax(np.diff(out[0].part_ptr) == 65))
        lv.G = list(lv.G)
        lv.G[p] = lv.G[p].copy()
        lv.G[p][:, -1] = 0.0
    elif which == "dropped -E^T row":  # one row of a level-2 part's -E^T block (= a column of E_p)
        lv, p = out[1], int(np.argmax(np.diff(out[1].part_ptr) == 17))
        lv.E = list(lv.E)
        lv.E[p] = lv.E[p].copy()
        lv.E[p][:, lv.E[p].shape[1] // 2] = 0.0
    elif which == "shifted block":  # one part's G block read a row too far
        lv, p = out[0], int(np.argmax(np.diff(out[0].part_ptr) == 33))
        lv.G = list(lv.G)
        lv.G[p] = np.roll(lv.G[p], 1, axis=0)
    else:
        raise ValueError(which)
    return out


@pytest.mark.parametrize("which, at_least", [("dropped column", 1000.0), ("dropped -E^T row", 1.0), ("shifted block", 1.0)])
def test_the_criterion_has_teeth(which, at_least):
    """The device test admits ``d <= max(f s, 8 kappa u)`` per probe column with f <= 1.  Shown on the MODEL (never on a
    kernel): with f = 1, the most the device test may ever admit, one defect of the rounded factors moves some probe
    column's answer by this many times its bound (mixed layout, 4,305 sites; the figure is the largest d / max(s, 8 kappa
    u) over the probe columns) --

      the last column of the 65-row level-1 part's G_p zeroed     2.5e+07  (required: > 1000; the random columns alone: 5e+05 .. 1.5e+06)
      one -E^T row of the 17-row level-2 part zeroed              2.3e+06  (random columns: 1e+05 .. 2.3e+06)
      the 33-row level-1 part's G block shifted by a row          3.2e+07  (random columns: 3.5e+06 .. 6.5e+06)

    so a sweep that drops the tail of a chunk, loses a part's -E^T row or mis-places a block cannot pass."""
    lay = _layout("mixed", 3)
    _, _, kappa = _reference(P.LAYOUTS["mixed"][0])
    B = P.probe_columns(lay.ptrs, lay.n)
    s, rounded, (l32, G32) = storage_error(lay, B)
    bad = P.apply_levels(_mutated(l32, which), G32, B)
    d = np.abs(bad - rounded).max(axis=0) / np.abs(rounded).max(axis=0)
    ratio = d / np.maximum(s, D.C_TOL * kappa * D.U)
    print(f"\n{which}: largest d / bound {ratio.max():.3g} (column {int(np.argmax(ratio))} of {len(ratio)}); "
          f"random columns {ratio[-4:].min():.3g} .. {ratio[-4:].max():.3g}")
    assert ratio.max() > at_least
    assert np.all(ratio[-4:] > at_least)  # every random column sees it, not only the unit vector that hits the defect
