"""The block low-rank form of the preconditioner's top separator as the product's host code builds it
(`tdgl_host_blr_form`: dense.inc, blr_form_host -- compression, column placement, items, dense slots, byte counts), on
symmetric matrices whose tiles have prescribed ranks (tests/blr_model.py), at the absolute tolerance 1e-9.  No GPU.

The cases are the smallest at which each branch of the layout exists (`blr_model.CASES`).  tests/test_hip_blr_form.py
runs the two kernels on the same matrices; the last test here checks the condition on the inputs that keeps every stored
column visible there."""

import ctypes as C
import functools

import numpy as np
import pytest

import blr_model as M

DT = M.DT


@functools.lru_cache(maxsize=None)
def _case(name):
    from tdgl_amd.hipcore import host_blr_form

    G, table = M.case_matrix(name)
    return G, table, host_blr_form(G, M.TOL_ABS)


def teardown_module(module):
    _case.cache_clear()


def _expected_ranks(table, nt):
    want = np.zeros((nt, nt), dtype=np.int64)
    for I in range(nt):
        for J in range(I):
            want[I, J] = table[I][J] if table[I][J] <= M.KMAX else -1
        want[I, I] = -1
    return want


def _padded_tile(G, I, J):
    n = G.shape[0]
    Gp = np.zeros((M.tiles_of(n) * DT,) * 2)
    Gp[:n, :n] = G
    return Gp[I * DT:(I + 1) * DT, J * DT:(J + 1) * DT]


ALL = pytest.mark.parametrize("name", list(M.CASES))


@ALL
def test_found_ranks_are_the_prescribed_ones_and_every_tile_is_dense_or_a_pair(name):
    G, table, form = _case(name)
    n, nt = G.shape[0], M.tiles_of(G.shape[0])
    assert (form["n"], form["nt"]) == (n, nt)
    want = _expected_ranks(table, nt)
    got = M.ranks(form)
    assert np.array_equal(got, want), (got, want)
    # the dense tiles: in tile order, none twice, every diagonal tile among them
    ij = [(int(v) >> 16, int(v) & 0xffff) for v in form["dense_ij"]]
    assert ij == sorted(set(ij)) and all(J <= I < nt for I, J in ij) and form["ndense"] == len(ij)
    assert all((I, I) in ij for I in range(nt))
    # every off-diagonal tile is exactly one of dense or pair: no column's pair lies in a dense tile, the counts add up
    _, blk = M.all_columns(form)
    twin = form["twin"]
    live = np.flatnonzero(twin >= 0)
    pair_tiles = {(max(int(blk[a]), int(blk[twin[a]])), min(int(blk[a]), int(blk[twin[a]]))) for a in live}
    assert not pair_tiles & set(ij)
    assert form["pairs"] == nt * (nt - 1) // 2 - (len(ij) - nt) == int((want[np.tril_indices(nt, -1)] >= 0).sum())
    assert form["rank_max"] == max(0, int(want.max()))


@ALL
def test_dense_tiles_are_the_float32_of_the_fp64_tiles_bit_for_bit(name):
    G, _, form = _case(name)
    assert form["Gd"].dtype == np.float32 and form["Gd"].shape == (form["ndense"], DT, DT)
    for d, v in enumerate(form["dense_ij"]):
        I, J = int(v) >> 16, int(v) & 0xffff
        want = _padded_tile(G, I, J).astype(np.float32)
        assert np.array_equal(form["Gd"][d].view(np.uint32), want.view(np.uint32)), (I, J)


@ALL
def test_columns_twins_and_padding(name):
    G, table, form = _case(name)
    n, nt = G.shape[0], M.tiles_of(G.shape[0])
    colbase, twin = form["colbase"], form["twin"]
    R = np.array(M.block_column_counts(table, nt))
    assert colbase[0] == 0 and np.all(colbase % 4 == 0)
    assert np.array_equal(np.diff(colbase), (R + 3) // 4 * 4) and form["cols"] == colbase[-1] == len(twin)
    assert len(form["F"]) == form["cols"] * DT
    cols, blk = M.all_columns(form)
    # twin == -1 exactly on the padding columns (the last ones of their block), and those columns of F are all zero
    padding = np.concatenate([np.arange(colbase[K] + R[K], colbase[K + 1]) for K in range(nt)]).astype(np.int64)
    assert np.array_equal(np.flatnonzero(twin < 0), padding) and np.all(twin[padding] == -1)
    assert not cols[:, padding].any()
    # an involution on the live columns, between different row blocks
    live = np.flatnonzero(twin >= 0)
    assert np.all(twin[live] < form["cols"]) and np.array_equal(twin[twin[live]], live)
    assert np.all(blk[twin[live]] != blk[live])
    assert cols[:, live].any(axis=0).all()
    # rows beyond n of the last row block are exactly zero (both halves)
    last = cols[:, blk == nt - 1]
    assert not last[n - (nt - 1) * DT:].any()


@ALL
def test_items_cover_every_group_once(name):
    _, _, form = _case(name)
    nt, items = form["nt"], form["items"]
    assert items.shape == (form["nitems"], 4)
    groups = np.diff(form["colbase"]) // 4
    seen = [np.zeros(g, dtype=int) for g in groups]
    for K, g0, g1, pad in items:
        assert 0 <= K < nt and 0 <= g0 < g1 <= groups[K] and g1 - g0 <= M.ITEM_GROUPS and pad == 0
        seen[K][g0:g1] += 1
    assert all(np.all(s == 1) for s in seen)
    assert form["nitems"] == int(((groups + M.ITEM_GROUPS - 1) // M.ITEM_GROUPS).sum())
    assert [tuple(r[:2]) for r in items] == sorted(tuple(r[:2]) for r in items)  # (block by block, ascending)


@ALL
def test_dense_slots_are_the_dense_tiles_of_each_row_block(name):
    _, _, form = _case(name)
    nt = form["nt"]
    dense = {(int(v) >> 16, int(v) & 0xffff) for v in form["dense_ij"]}
    ptr = form["dslot_ptr"]
    assert ptr[0] == 0 and ptr[-1] == form["ndslot"] == len(form["dslot"])
    for K in range(nt):
        want = [J for J in range(nt) if (max(K, J), min(K, J)) in dense]
        assert form["dslot"][ptr[K]:ptr[K + 1]].tolist() == want, K


@ALL
def test_byte_counts(name):
    _, _, form = _case(name)
    nt = form["nt"]
    assert form["dense_bytes"] == nt * (nt + 1) // 2 * DT * DT * 4
    assert form["bytes"] == form["ndense"] * DT * DT * 4 + 2 * form["cols"] * DT * 4


@ALL
def test_stored_pairs_reproduce_their_tiles(name):
    """|| U_s W_s^T - G_IJ ||_F <= tol_abs + 2^-22 || |U_s| |W_s|^T ||_F per pair tile (two float32 roundings are 2 x 2^-24
    entry by entry; a factor 2 over that), and the whole decoded matrix is symmetric."""
    G, _, form = _case(name)
    nt = form["nt"]
    Gs = M.decode(form)
    assert Gs.shape == G.shape and np.array_equal(Gs, Gs.T)
    got = M.ranks(form)
    worst = 0.0
    for I in range(nt):
        for J in range(I):
            if got[I, J] < 0:
                continue
            Us, Ws = M.pair_factors(form, I, J)
            assert Us.shape == Ws.shape == (DT, got[I, J])
            n = G.shape[0]
            tile = np.zeros((DT, DT))
            blockI, blockJ = slice(I * DT, min((I + 1) * DT, n)), slice(J * DT, min((J + 1) * DT, n))
            sub = Gs[blockI, blockJ]
            tile[:sub.shape[0], :sub.shape[1]] = sub
            assert np.allclose(tile, Us @ Ws.T, rtol=0, atol=1e-15)  # (decode places the pair where the model says)
            err = np.linalg.norm(Us @ Ws.T - _padded_tile(G, I, J))
            bound = M.TOL_ABS + 2.0 ** -22 * np.linalg.norm(np.abs(Us) @ np.abs(Ws).T)
            worst = max(worst, err / bound)
            assert err <= bound, (I, J, err, bound)
    print(f"{name}: largest error / bound over the pair tiles {worst:.3g}")


@ALL
def test_the_model_applies_what_it_decodes(name):
    """`blr_model.apply` (projections, twins, dense slots) against `blr_model.decode` (outer products) on random
    columns: two routes through the same arrays, within the summation-order bound of the GPU test."""
    G, _, form = _case(name)
    X = np.random.default_rng(11).standard_normal((G.shape[0], 3))
    y, S = M.apply(form, X)
    k = M.additions_on_the_longest_path(form)
    assert np.all(np.abs(y - M.decode(form) @ X) <= 2 * k * M.U * S)
    y1, S1 = M.apply(form, X[:, 0])
    assert y1.shape == S1.shape == (G.shape[0],)  # (one vector: the same numbers up to the order of NumPy's own sums)
    assert np.all(np.abs(y1 - y[:, 0]) <= 2 * k * M.U * S1) and np.allclose(S1, S[:, 0], rtol=1e-12, atol=0)


@ALL
def test_no_stored_column_pair_is_negligible(name):
    """A condition on the INPUTS of tests/test_hip_blr_form.py: every stored pair of columns carries at least 0.05 of the
    largest one's weight, so a kernel that drops or misplaces any of them moves the result far beyond rounding."""
    _, _, form = _case(name)
    cols, _ = M.all_columns(form)
    twin = form["twin"]
    live = np.flatnonzero(twin >= 0)
    if len(live) == 0:
        assert name == "n100"
        return
    w = np.linalg.norm(cols[:, live], axis=0) * np.linalg.norm(cols[:, twin[live]], axis=0)
    assert w.min() >= 0.05 * w.max(), (w.min(), w.max())


# ---- what each case is there for ------------------------------------------------------------------------------------
def test_the_cases_reach_the_branches_they_are_meant_to():
    f = {name: _case(name)[2] for name in M.CASES}
    R = {name: np.diff(f[name]["colbase"]) for name in M.CASES}
    # one diagonal tile: no column, no item -- the arrays are empty
    assert (f["n100"]["nt"], f["n100"]["ndense"], f["n100"]["cols"], f["n100"]["nitems"]) == (1, 1, 0, 0)
    assert len(f["n100"]["items"]) == 0 and len(f["n100"]["F"]) == 0 and len(f["n100"]["twin"]) == 0
    # one column per block padded to four: three columns without a twin each
    assert R["n129_rank1"].tolist() == [4, 4] and f["n129_rank1"]["twin"].tolist() == [4, -1, -1, -1, 0, -1, -1, -1]
    assert R["n193_rank3"].tolist() == [4, 4] and 193 - DT - M.HALF == 1
    # every residue of the unpadded column count, an empty block between full ones, dense tiles among the pairs
    table = M.rank_table_703()
    raw = M.block_column_counts(table, 6)
    assert sorted({r % 4 for r in raw}) == [0, 1, 2, 3] and raw[2] == 0 and raw[1] > 0 and raw[3] > 0
    assert R["n703_mixed"][2] == 0 and f["n703_mixed"]["ndense"] == 6 + 3
    assert {table[I][J] for I in range(6) for J in range(I)} == {0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33}
    # 40 groups per block: more than the 32 of one trip of the finish loop, five items
    assert R["n768_rank32"].tolist() == [160] * 6 and f["n768_rank32"]["nitems"] == 30
    # 33 groups: an item of a single group, one valid group in the second trip
    assert R["n768_r130"][5] == 132 and M.block_column_counts(M.rank_table_768_mixed(), 6)[5] == 130
    last = [r for r in f["n768_r130"]["items"].tolist() if r[0] == 5][-1]
    assert last == [5, 32, 33, 0]
    assert f["n1025_random"]["nt"] == 9 and M.ranks(f["n1025_random"])[8, :8].max() == 1


# ---- the entry's error conventions ----------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    from tdgl_amd import _lib

    lib = _lib.load()
    G = np.eye(5)
    p = _lib.p_f64(G)
    form = _lib.BlrForm()
    assert lib.tdgl_host_blr_form(5, p, 1e-9, C.byref(form)) == _lib.TDGL_OK and form.ndense == 1
    assert lib.tdgl_host_blr_form(5, None, 1e-9, C.byref(form)) == _lib.TDGL_ERR_ARG
    assert lib.tdgl_host_blr_form(5, p, 1e-9, None) == _lib.TDGL_ERR_ARG
    assert lib.tdgl_host_blr_form(0, p, 1e-9, C.byref(form)) == _lib.TDGL_ERR_ARG
    assert lib.tdgl_host_blr_form(5, p, -1e-9, C.byref(form)) == _lib.TDGL_ERR_ARG
    assert lib.tdgl_host_blr_form(5, p, float("nan"), C.byref(form)) == _lib.TDGL_ERR_ARG
    # some arrays given and some not
    keep = np.zeros(4, dtype=np.int32)
    form = _lib.BlrForm()
    form.twin = keep.ctypes.data_as(_lib.c_i32p)
    assert lib.tdgl_host_blr_form(5, p, 1e-9, C.byref(form)) == _lib.TDGL_ERR_ARG
    with pytest.raises(ValueError, match="every array of the form, or none"):
        _lib.check(_lib.TDGL_ERR_ARG)
    # every array given, but counts that are not this matrix's
    from tdgl_amd.hipcore import _blr_form_fill

    def sized_for_another(fm):
        _lib.check(lib.tdgl_host_blr_form(5, p, 1e-9, C.byref(fm)))
        fm.ndense = 2

    with pytest.raises(ValueError, match="not those of the sizing call"):
        _blr_form_fill(sized_for_another, lambda fm: _lib.check(lib.tdgl_host_blr_form(5, p, 1e-9, C.byref(fm))))
