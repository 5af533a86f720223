"""The two kernels of the block low-rank top separator, `k_blr_project` and `k_blr_finish` (kernels.inc; launched by
`blr_launch`, factors.inc), entry by entry against the float64 model of the stored form (tests/blr_model.py).

A. The kernels alone (`tdgl_blr_apply`): on the matrices of tests/test_blr_form_host.py the whole operator is recovered
   with ONE call over all n unit vectors, four standard-normal columns and the all-ones column, and every entry is
   compared with `blr_model.apply` on the form that call built:

       |y_dev - y_model|_i  <=  2 k u S_i,    u = 2^-53,  k = 128 nt + max R_K + 64,

   S_i = the model's sum of absolute values of every product that enters row i (|Gd| |x| + |F_K| (|F_twin|^T |x|)), k the
   additions on the longest path through both launches, rounded up; the factor 2 covers the model's own rounding and
   the second-order terms.  A summation-order bound: nothing measured went into it.  A second call returns the same bits.
   Largest err / (u S) per case, measured on the MI355X (bound 2 k):

       n100 (one dense tile)                         2.0    (bound 384)
       n129_rank1 / n193_rank3 (R_K 4, 4)            2.2 / 2.1  (648)
       n703_mixed (R_K 48, 76, 0, 24, 16, 48)        7.7    (1816)
       n768_rank32 (R_K 160 x 6)                     8.1    (1984)
       n768_r130 (R_K 160 x 4, 132, 132)             9.2    (1984)
       n1025_random (nt 9, R_K 40 .. 52, last 4)     4.0    (2536)

   Value-only mutations of the kernels that this part catches (tried on a scratch copy): the last group of every item
   skipped in `k_blr_project`; every projection written to its own slot instead of its twin's; the last dense slot of every
   row block left out in `k_blr_finish` -- each fails every case that has the feature (all but n100; all seven).

B. In the preconditioner: the prescribed `mixed` layout (three levels, a top separator of 906 sites = 8 tiles, the last
   with 10 live rows) with TDGL_PD_BLR=1 and TDGL_PD_BLR_TOL=1e-4.  The stored form is read back
   (`tdgl_get_precond_direct_blr_form`), checked against the host's float64 inverse of the top separator, and put into
   the model of tests/test_hip_sub_prescribed.py in place of G_top: the model then holds exactly what the device stores,
   so one application per probe column must agree within that module's floor 8 kappa u alone.

   Measured: the stored form has 23 pairs and 13 dense tiles (5 off the diagonal), R_K 36, 52, 72, 44, 40, 44, 40, 20,
   largest rank 27, 0.512 of the dense tiles' bytes, ||G||_2 estimate 108.1; its largest tile error is 0.97 of the bound;
   largest d / floor = 6.9e-4 over 60 probe columns (d = 1.6e-15, floor 8 kappa u = 2.3e-12, kappa 2541).

C. Refusals of the two entries."""

import ctypes as C
import functools

import numpy as np
import pytest

import blr_model as M
import dense_reference as D
import prescribed_dissection as P
import test_hip_sub_prescribed as SP
from helpers import synthetic_mesh

pytestmark = pytest.mark.gpu

DT = M.DT


@pytest.fixture(scope="module")
def small_ctx():
    """Any context will do for `tdgl_blr_apply`: it lends its device and stream."""
    from tdgl_amd.hipcore import TDGLContext

    ctx = TDGLContext(synthetic_mesh(8))
    yield ctx
    ctx.close()


def teardown_module(module):
    SP.teardown_module(SP)


# ---- A: the kernels alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.CASES))
def test_the_two_kernels_match_the_model_of_the_form_entry_by_entry(name, small_ctx):
    from tdgl_amd.hipcore import host_blr_form

    G, _ = M.case_matrix(name)
    n = G.shape[0]
    X = np.hstack([np.eye(n), np.random.default_rng(2).standard_normal((n, 4)), np.ones((n, 1))])
    Y, form = small_ctx.blr_apply(G, M.TOL_ABS, X)
    # the form the call built is the one the host entry builds of the same matrix
    want = host_blr_form(G, M.TOL_ABS)
    assert sorted(form) == sorted(want)
    for key, value in want.items():
        assert np.array_equal(form[key], value), key
    y, S = M.apply(form, X)
    k = M.additions_on_the_longest_path(form)
    err = np.abs(Y - y)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(S > 0.0, err / (M.U * S), 0.0)
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{name}: n {n}, nt {form['nt']}, R_K {np.diff(form['colbase']).tolist()}, dense tiles {form['ndense']}, items "
          f"{form['nitems']}: largest err / (u S) = {ratio.max():.3g} (row {i}, column {j} of {X.shape[1]}; bound 2 k = {2 * k}), "
          f"unit vectors {ratio[:, :n].max():.3g}, random and ones {ratio[:, n:].max():.3g}")
    assert np.isfinite(Y).all()
    assert np.all(err <= 2 * k * M.U * S), (i, j, err[i, j], S[i, j])  # (S_i = 0: the entry is exactly zero)
    Y2, _ = small_ctx.blr_apply(G, M.TOL_ABS, X)
    assert np.array_equal(Y, Y2)


# ---- B: in the preconditioner ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rounded_levels(name):
    lay = SP._layout(name)
    return P.rounded_to_storage(lay.levels, lay.G_top)[0]


def _tile(G, I, J):
    n = G.shape[0]
    out = np.zeros((DT, DT))
    sub = G[I * DT:min((I + 1) * DT, n), J * DT:min((J + 1) * DT, n)]
    out[:sub.shape[0], :sub.shape[1]] = sub
    return out


def test_the_stored_form_in_the_preconditioner_and_one_application_per_probe_column(monkeypatch):
    """(CG tolerance 1e-5: the build keeps the factors only if its check solve gets to the tolerance in three
    applications; with the top separator truncated at 1e-4 the float64 model of that CG stands at 2e-5 after two and at
    1e-7 after three, at 1e-10 only after five.)"""
    rtol = 1e-5
    ctx, lay = SP._precond_ctx("mixed", monkeypatch, False, blr_tol=1e-4, rtol=rtol)
    try:
        assert ctx.precond_direct and not ctx.dense_direct, ctx.setup_times
        assert np.array_equal(ctx._pd_order[0], lay.perm)
        info = ctx.precond_direct_blr()
        assert info["on"] and info["tau"] == 1e-4, info
        form = ctx.precond_direct_blr_form()
        n_top = lay.G_top.shape[0]
        assert (form["n"], form["nt"]) == (n_top, M.tiles_of(n_top)) == (906, 8)
        assert (form["pairs"], form["ndense"], form["rank_max"], form["bytes"], form["dense_bytes"]) == \
               (info["pairs"], info["dense_tiles"], info["rank_max"], info["bytes"], info["dense_bytes"])
        nt, got = form["nt"], M.ranks(form)
        print(f"mixed, tau 1e-4: ||G||_2 estimate {info['norm']:.6g}, {form['pairs']} pairs, {form['ndense']} dense tiles "
              f"({form['ndense'] - nt} off the diagonal), R_K {np.diff(form['colbase']).tolist()}, largest rank {form['rank_max']}, "
              f"items {form['nitems']}, bytes {form['bytes'] / form['dense_bytes']:.3f} of the dense tiles'")
        print("ranks (-1: dense):", got.tolist())
        # the stored form itself, against the host's float64 inverse of the top separator
        assert 0.0 < info["norm"] <= (1.0 + 1e-6) * np.linalg.norm(lay.G_top, 2)  # (a power iteration: from below)
        tol_abs = info["tau"] * info["norm"]
        Gs = M.decode(form)
        assert np.array_equal(Gs, Gs.T)
        worst = 0.0
        for I in range(nt):
            for J in range(I + 1):
                if got[I, J] < 0:
                    weight = np.abs(_tile(Gs, I, J))
                else:
                    Us, Ws = M.pair_factors(form, I, J)
                    weight = np.abs(Us) @ np.abs(Ws).T
                err = np.linalg.norm(_tile(Gs, I, J) - _tile(lay.G_top, I, J))
                bound = tol_abs + 2.0 ** -22 * np.linalg.norm(weight)
                worst = max(worst, err / bound)
                assert err <= bound, (I, J, int(got[I, J]), err, bound)
        print(f"stored form against the float64 inverse: largest tile error / bound {worst:.3g}")
        # one application per probe column against the model that holds the decoded form
        _, _, kappa = SP._reference(P.LAYOUTS["mixed"][0])
        floor = D.C_TOL * kappa * D.U
        B = P.probe_columns(lay.ptrs, lay.n)
        z_model = P.apply_levels(_rounded_levels("mixed"), Gs, B)
        rhs = np.random.default_rng(7).standard_normal(lay.n)
        before = ctx.poisson_solve(rhs)
        d = np.empty(B.shape[1])
        for j in range(B.shape[1]):
            r = B[lay.iperm, j]  # (site order: r[perm[i]] = B[i])
            z, rz = ctx.precond_apply(r)
            d[j] = np.abs(z[lay.perm] - z_model[:, j]).max() / np.abs(z_model[:, j]).max()
            assert abs(rz - r @ z) <= lay.n * D.U * np.abs(r * z).sum(), (j, rz, r @ z)
        after = ctx.poisson_solve(rhs)
        worst = int(np.argmax(d))
        print(f"mixed, block low-rank top: kappa {kappa:.4g}, floor 8 kappa u {floor:.3g}, largest d / floor = {d.max() / floor:.3g} "
              f"(column {worst} of {len(d)}; d = {d[worst]:.3g}), random columns {d[-4:].max() / floor:.3g}")
        assert np.all(d <= floor), (worst, d[worst], floor)
        # the CG's state is as it was: the same solve, bit for bit
        assert before[1] == after[1] and np.array_equal(before[0], after[0]) and before[2] == after[2]
        assert before[2] <= rtol and 1 <= before[1] <= 3
    finally:
        ctx.close()


# ---- C: refusals ----------------------------------------------------------------------------------------------------
def test_the_stored_form_is_refused_when_the_form_is_not_in_use(monkeypatch, small_ctx):
    with pytest.raises(RuntimeError, match="not in block low-rank form"):
        small_ctx.precond_direct_blr_form()  # (no factors at all)
    ctx, _ = SP._precond_ctx("mixed", monkeypatch, False)  # (TDGL_PD_BLR=0: the dense fp32 tiles)
    try:
        assert ctx.precond_direct and not ctx.precond_direct_blr()["on"]
        with pytest.raises(RuntimeError, match="not in block low-rank form"):
            ctx.precond_direct_blr_form()
    finally:
        ctx.close()


def test_blr_apply_refuses_bad_arguments(small_ctx):
    from tdgl_amd import _lib

    lib, h = small_ctx._lib, small_ctx._ctx
    n = 5
    G, X, Y = np.eye(n), np.ones((2, n)), np.zeros((2, n))
    g, x, y = _lib.p_f64(G), _lib.p_f64(X), _lib.p_f64(Y)
    assert lib.tdgl_blr_apply(h, n, g, 1e-9, 2, x, y, None) == _lib.TDGL_OK and np.array_equal(Y, X)
    for args, what in (((h, n, None, 1e-9, 2, x, y, None), "null argument"), ((h, n, g, 1e-9, 2, None, y, None), "null argument"),
                       ((h, n, g, 1e-9, 2, x, None, None), "null argument"), ((h, 0, g, 1e-9, 2, x, y, None), "n must be in"),
                       ((h, n, g, 1e-9, 0, x, y, None), "no vectors"), ((h, n, g, -1e-9, 2, x, y, None), "tolerance must be >= 0"),
                       ((h, n, g, float("nan"), 2, x, y, None), "tolerance must be >= 0")):
        status = lib.tdgl_blr_apply(*args)
        assert status == _lib.TDGL_ERR_ARG, (what, status)
        with pytest.raises(ValueError, match=what):
            small_ctx._chk(status)
    assert lib.tdgl_blr_apply(None, n, g, 1e-9, 2, x, y, None) == _lib.TDGL_ERR_ARG
    # a form with some arrays given and some not
    form = _lib.BlrForm()
    keep = np.zeros(4, dtype=np.int32)
    form.twin = keep.ctypes.data_as(_lib.c_i32p)
    assert lib.tdgl_blr_apply(h, n, g, 1e-9, 2, x, y, C.byref(form)) == _lib.TDGL_ERR_ARG
    with pytest.raises(ValueError, match="every array of the form, or none"):
        small_ctx._chk(_lib.TDGL_ERR_ARG)
    with pytest.raises(ValueError, match=r"G must be \[n, n\] and X \[n, k\]"):
        small_ctx.blr_apply(G, 1e-9, np.ones((n + 1, 2)))
