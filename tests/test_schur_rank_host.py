"""The float64 model of single ranks of the rank-level dissection (tests/schur_rank_model.py) against references of its
own, on the CPU: it is the reference of tests/test_hip_schur_rank.py, so it is held here first.

With every rank played by the model, on the shapes of `schur_rank_model.CASES`:

* the gauge-free local factors through `prescribed_dissection.apply_levels` are ``A_II^-1`` (SciPy's LU) within
  8 kappa_I u -- both are backward-stable solves of a matrix of condition kappa_I (measured: 2e-15 .. 2e-14, kappa_I
  465 .. 3500);
* the exact model applied to zero-mean columns is ``pinv(A)`` times the column up to a constant, within
  `dense_reference.tolerance` = 8 kappa u max |x| (measured: 1e-13 .. 5e-13 against 1e-12 .. 3e-12).  The columns must
  be zero-mean: ``M 1 != 0``, and a unit vector that is not projected differs from ``pinv`` by 10 %;
* the rank-local halves reproduce the sequence `dist_model.schur_apply_dist` ran before it was split, bit for bit;
* the storage error s (model with the fp32-stored factors against the exact model, per column) is positive: 1e-8 ..
  7e-8;
* the model with the fp32-stored factors contracts the residual of random zero-mean columns to 2e-7 .. 6e-7 of ||r||:
  DESIGN.md's "~1e-6 per application", held to 1e-6.
"""

import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import dense_reference as D
import schur_rank_model as M


@functools.lru_cache(maxsize=None)
def _case(name):
    h = M.build_case(name)
    G = D.pinv_reference(h.A)
    return h, G, D.condition_number(h.A, G)


def teardown_module(module):
    _case.cache_clear()


def _device_rank(name):
    return sorted(M.CASES[name][7])[-1]


@pytest.mark.parametrize("name", list(M.CASES))
def test_the_cases_have_the_shapes_they_were_chosen_for(name):
    h, _, _ = _case(name)
    _, _, world, _, lists, levels, n_gamma, ranks = M.CASES[name]
    assert h.world == world and h.n_gamma == n_gamma and n_gamma % 16 != 0 and n_gamma % 64 != 0
    for r, (owned, touched) in ranks.items():
        d = h.describe(r)
        assert d["levels"] == levels and d["owned_interface"] == owned, (r, d)
        assert touched is None or d["touched_interface"] == touched, (r, d)
        assert d["interior"] + d["owned_interface"] == h.ranks[r].lp.n_own
    # every site is interior to exactly one rank or in Gamma
    seen = np.zeros(h.n, dtype=int)
    for m in h.ranks:
        seen[m.lp.local_to_global[m.piece.interior]] += 1
    seen[h.gamma_sites] += 1
    assert np.all(seen == 1)
    if lists is not None:  # (d: the prescribed sizes, 1 .. 257 rows on level 1; top separators of 475 / 562 sites)
        assert [h.describe(r)["part_sizes"][0] for r in (0, 1)] == [sorted(lists[0])] * 2
        assert [h.describe(r)["top_separator"] for r in (0, 1)] == [475, 562]


@pytest.mark.parametrize("name", list(M.CASES))
def test_gauge_free_levels_are_the_inverse_of_the_interior_block(name):
    h, _, _ = _case(name)
    for r, m in enumerate(h.ranks):
        assert all(np.all(lv.g == 0.0) for lv in m.levels) and np.all(m.levels[-1].u == 0.0)  # no gauge is carried
        lu = spla.splu(m.piece.A_II.tocsc())
        b = np.random.default_rng(r).standard_normal((m.piece.n_interior, 4))
        want = lu.solve(b)
        kappa_I = M.condition_number_spd(m.piece.A_II)
        err = np.abs(h.solve(r)(b) - want).max(axis=0)
        print(f"{name} rank {r}: kappa_I {kappa_I:.4g}, max |apply_levels - LU| / max |x| = {(err / np.abs(want).max(axis=0)).max():.3g}")
        assert np.all(err <= D.tolerance(kappa_I, want)), (r, err)


@pytest.mark.parametrize("name", list(M.CASES))
def test_the_exact_model_is_the_pseudo_inverse_on_zero_mean_columns(name):
    h, G, kappa = _case(name)
    B, _ = h.probe_columns(_device_rank(name))
    assert np.abs(B.sum(axis=0)).max() <= 1e-12
    Z = h.apply(B)
    X = G @ B
    err = np.abs((Z - Z.mean(axis=0)) - X).max(axis=0)
    tol = D.tolerance(kappa, X)
    print(f"{name}: kappa {kappa:.4g}, 8 kappa u {D.C_TOL * kappa * D.U:.3g}, max |M r - pinv(A) r| / max |x| = "
          f"{(err / np.abs(X).max(axis=0)).max():.3g} over {B.shape[1]} columns")
    assert np.all(err <= tol), (int(np.argmax(err / tol)), (err / tol).max())
    # ... and what a device rank is handed in the all-reduce completes its own term to the sum of the application
    for r in range(h.world):
        t_r, z_r = h.apply_rank(r, B)
        assert np.array_equal(z_r, Z[h.ranks[r].own])
        t = t_r + h.others_share(r, B)
        x_gamma = Z[h.gamma_sites]
        assert np.abs(h.Spinv @ t - x_gamma).max() <= D.C_TOL * kappa * D.U * np.abs(x_gamma).max()
    # a unit vector that is not projected is NOT what pinv returns
    e = np.zeros(h.n)
    e[h.n // 2] = 1.0
    z = h.apply(e)
    x = G @ e
    assert np.abs((z - z.mean()) - x).max() > 0.01 * np.abs(x).max()


def _unsplit_sequence(h, lus, Spinv, R):
    """`dist_model.schur_apply_dist` as it was before its rank-local halves were split out, every rank in this process
    (the all-reduce: the sum in rank order)."""
    ys, ts = [], []
    for m, lu in zip(h.ranks, lus):
        lp, piece = m.lp, m.piece
        r_loc = np.zeros(lp.n_loc)
        r_loc[: lp.n_own] = R[m.own]
        y = lu.solve(r_loc[piece.interior])
        t = np.zeros(piece.n_gamma)
        t[piece.gamma_owned_gid] = r_loc[piece.gamma_owned_local]
        t -= piece.A_GI @ y
        ys.append(y)
        ts.append(t)
    t = np.zeros(h.n_gamma)
    for t_r in ts:
        t += t_r
    xg = Spinv @ t
    out = []
    for m, lu, y in zip(h.ranks, lus, ys):
        piece = m.piece
        xi = y - lu.solve(piece.A_IG @ xg)
        z = np.zeros(m.lp.n_own)
        z[piece.interior] = xi
        z[piece.gamma_owned_local] = xg[piece.gamma_owned_gid]
        out.append(z)
    return ts, out


@pytest.mark.parametrize("name", ["a", "d"])
def test_the_split_halves_reproduce_the_unsplit_sequence_bit_for_bit(name):
    from tdgl_amd.schur_dd import interface_pinv

    h, _, _ = _case(name)
    lus = [spla.splu(m.piece.A_II.tocsc()) for m in h.ranks]
    # set-up: the share of S as `schur_setup_dist` formed it
    S = np.zeros((h.n_gamma, h.n_gamma))
    for m, lu in zip(h.ranks, lus):
        piece = m.piece
        touched = np.unique(piece.A_IG.indices)
        X = lu.solve(piece.A_IG[:, touched].toarray())
        share = piece.A_GG_owned.toarray()
        share[np.ix_(touched, touched)] -= piece.A_GI[touched] @ X
        assert np.array_equal(share, M.schur_share(piece, lu.solve))
        assert np.array_equal(piece.A_GG_owned.toarray() - M.complement_share(piece, lu.solve), share)
        S += share
    Spinv = interface_pinv(S)
    R = np.random.default_rng(5).standard_normal(h.n)
    R -= R.mean()
    ts, zs = _unsplit_sequence(h, lus, Spinv, R)
    t = np.zeros(h.n_gamma)
    ys = []
    for m, lu, t_want in zip(h.ranks, lus, ts):
        y = M.interior_solve(m.piece, lu.solve, R[m.own])
        t_r = M.interface_share(m.piece, R[m.own], y)
        assert np.array_equal(t_r, t_want)
        ys.append(y)
        t += t_r
    for m, lu, y, z_want in zip(h.ranks, lus, ys, zs):
        assert np.array_equal(M.result_from_interface(m.piece, lu.solve, m.lp.n_own, y, Spinv @ t), z_want)


@pytest.mark.parametrize("name", list(M.CASES))
def test_the_storage_error_and_the_contraction_of_the_rounded_model(name):
    h, _, _ = _case(name)
    B, what = h.probe_columns(_device_rank(name))
    Ze, Zr = h.apply(B), h.apply(B, rounded=True)
    s = M.storage_error(Zr, Ze)
    rnd = [j for j, w in enumerate(what) if w == "random"]
    assert len(rnd) == 4
    res = np.linalg.norm(B[:, rnd] - h.A @ Zr[:, rnd], axis=0) / np.linalg.norm(B[:, rnd], axis=0)
    exact = np.linalg.norm(B[:, rnd] - h.A @ Ze[:, rnd], axis=0) / np.linalg.norm(B[:, rnd], axis=0)
    print(f"{name}: s {s.min():.3g} .. {s.max():.3g}; ||r - A M r|| / ||r|| with the fp32-stored factors {res.min():.3g} .. "
          f"{res.max():.3g}, exact {exact.max():.3g}")
    assert np.all(s > 0.0) and np.all(s < 1e-6)  # (fp32: u = 6e-8 per stored entry)
    assert np.all(res <= 1e-6) and np.all(res > exact)
    # the device rank's own rows carry a storage error too (what the GPU test scales its bound with)
    r = _device_rank(name)
    own = h.ranks[r].own
    assert np.all(M.storage_error(Zr[own], Ze[own]) > 0.0)
