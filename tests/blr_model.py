"""A float64 model of the preconditioner's top separator in block low-rank form, NumPy only: for
tests/test_blr_form_host.py and tests/test_hip_blr_form.py.

The form (csrc/kernels.inc at `BlrArgs`) of a symmetric matrix of order n in nt = ceil(n / 128) row
blocks of 128 rows (zero padded): every tile (I, J), J <= I, is either a dense float32 tile -- ``dense_ij[d] = I << 16 |
J``, ``Gd[d]`` row major -- or a pair of float32 factors, G_IJ ~ U W^T.  Row block K owns the columns
``colbase[K] .. colbase[K + 1]`` (R_K of them, a multiple of 4; the last ones padding): every U of a pair (K, J), every W
of a pair (I, K).  Entry (row, c) of block K's columns is at

    F[128 colbase[K] + ((row // 64) R_K + c) 64 + row % 64]

and ``twin[a]`` is the column that carries the other factor of column a's pair (-1: padding).  The product applies the
form in two launches: every column's projection c = F_K^T x_K goes to its twin's slot of ``coef``; then y_K = the dense
tiles of row block K (``dslot[dslot_ptr[K] : dslot_ptr[K + 1]]``: their J, the diagonal included) applied to x_J + F_K
coef_K.  The wavefront items ``(K, g0, g1, 0)`` split the groups of four columns of a block into runs of at most 8.

`decode` and `apply` read the arrays by this description alone, `prescribed_matrix` makes symmetric matrices whose tiles
have the ranks a test asks for."""

import numpy as np

DT, HALF, KMAX, ITEM_GROUPS = 128, 64, 32, 8
U = 2.0 ** -53


def tiles_of(n):
    return (n + DT - 1) // DT


def block_columns(form, K):
    """F_K as a float64 matrix [128, R_K] (the padding columns included)."""
    cb, ce = int(form["colbase"][K]), int(form["colbase"][K + 1])
    R = ce - cb
    flat = np.asarray(form["F"][DT * cb:DT * ce], dtype=np.float64)
    return flat.reshape(2, R, HALF).transpose(0, 2, 1).reshape(DT, R)  # (half, column, row in half) -> (row, column)


def all_columns(form):
    """([128, cols] every block's columns side by side -- column a of the result is column a of ``twin`` --, the row block
    of every column)."""
    nt = int(form["nt"])
    cols = np.concatenate([block_columns(form, K) for K in range(nt)], axis=1) if nt else np.zeros((DT, 0))
    return cols, np.repeat(np.arange(nt), np.diff(form["colbase"]))


def dense_tiles(form):
    """{(I, J): float64 tile [128, 128]} of the tiles kept dense, J <= I."""
    return {(int(ij) >> 16, int(ij) & 0xffff): np.asarray(form["Gd"][d], dtype=np.float64) for d, ij in enumerate(form["dense_ij"])}


def ranks(form):
    """[nt, nt] lower triangle: the number of column pairs of tile (I, J), -1 for a dense tile (above the diagonal: 0)."""
    nt = int(form["nt"])
    out = np.zeros((nt, nt), dtype=np.int64)
    _, blk = all_columns(form)
    twin = np.asarray(form["twin"])
    live = np.flatnonzero(twin >= 0)
    for a in live:
        I, J = int(blk[a]), int(blk[twin[a]])
        if I > J:
            out[I, J] += 1
    for (I, J) in dense_tiles(form):
        out[I, J] = -1
    return out


def pair_factors(form, I, J):
    """(U_s, W_s) [128, r] float64: the stored columns of the pair tile (I, J), I > J, in storage order."""
    cols, blk = all_columns(form)
    twin = np.asarray(form["twin"])
    a = np.flatnonzero((blk == I) & (twin >= 0))
    a = a[blk[twin[a]] == J]
    return cols[:, a], cols[:, twin[a]]


def decode(form):
    """The matrix the stored form represents, [n, n] float64: the dense tiles and their transposes, and for every twin
    pair of columns their outer product in the tile of their two row blocks (and its transpose)."""
    n, nt = int(form["n"]), int(form["nt"])
    Gs = np.zeros((nt * DT, nt * DT))
    for (I, J), tile in dense_tiles(form).items():
        Gs[I * DT:(I + 1) * DT, J * DT:(J + 1) * DT] = tile
        if I != J:
            Gs[J * DT:(J + 1) * DT, I * DT:(I + 1) * DT] = tile.T
    cols, blk = all_columns(form)
    twin = np.asarray(form["twin"])
    for a in np.flatnonzero(twin >= 0):
        I, J = int(blk[a]), int(blk[twin[a]])
        if I > J:
            outer = np.outer(cols[:, a], cols[:, twin[a]])
            Gs[I * DT:(I + 1) * DT, J * DT:(J + 1) * DT] += outer
            Gs[J * DT:(J + 1) * DT, I * DT:(I + 1) * DT] += outer.T
    return Gs[:n, :n]


def apply(form, x):
    """``(y, S)`` for ``x`` [n] or [n, k]: y by the stated algorithm -- c = F_K^T x_K per row block, coef[twin[a]] =
    c[a], y_K = the dense slots of K + F_K coef_K --, and S = |Gd| |x| + |F_K| (|F_twin|^T |x|), the sum of the absolute
    values of every product that enters y, per row."""
    n, nt = int(form["n"]), int(form["nt"])
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    xp = np.zeros((nt * DT, 1 if one else x.shape[1]))
    xp[:n] = x[:, None] if one else x
    cols, blk = all_columns(form)
    twin = np.asarray(form["twin"])
    live = np.flatnonzero(twin >= 0)
    coef = np.zeros((cols.shape[1], xp.shape[1]))
    coef_abs = np.zeros_like(coef)
    for K in range(nt):
        a = live[blk[live] == K]
        xk = xp[K * DT:(K + 1) * DT]
        coef[twin[a]] = cols[:, a].T @ xk
        coef_abs[twin[a]] = np.abs(cols[:, a]).T @ np.abs(xk)
    tiles = dense_tiles(form)
    y, S = np.zeros_like(xp), np.zeros_like(xp)
    for K in range(nt):
        yk, sk = np.zeros((DT, xp.shape[1])), np.zeros((DT, xp.shape[1]))
        for J in form["dslot"][form["dslot_ptr"][K]:form["dslot_ptr"][K + 1]]:
            J = int(J)
            tile = tiles[(K, J)] if K >= J else tiles[(J, K)].T
            yk += tile @ xp[J * DT:(J + 1) * DT]
            sk += np.abs(tile) @ np.abs(xp[J * DT:(J + 1) * DT])
        cb, ce = int(form["colbase"][K]), int(form["colbase"][K + 1])
        FK = block_columns(form, K)
        yk += FK @ coef[cb:ce]
        sk += np.abs(FK) @ coef_abs[cb:ce]
        y[K * DT:(K + 1) * DT], S[K * DT:(K + 1) * DT] = yk, sk
    y, S = y[:n], S[:n]
    return (y[:, 0], S[:, 0]) if one else (y, S)


def additions_on_the_longest_path(form):
    """k of the summation-order bound 2 k u S: 128 nt for the dense tiles of a row, max R_K for the columns, 64 for the
    shuffles, the LDS meeting and the projections' share that exceeds a dense row -- rounded up."""
    return DT * int(form["nt"]) + int(np.diff(form["colbase"]).max()) + 64


# ---- test matrices with prescribed block ranks ----------------------------------------------------------------------
def _orthonormal(rng, rows, r):
    q, _ = np.linalg.qr(rng.standard_normal((rows, r)))
    return q


def prescribed_matrix(n, rank_table, seed=0):
    """A symmetric [n, n] matrix whose tile (I, J), I > J, is sum over k < r of s_k a_k b_k^T with r =
    ``rank_table[I][J]``, random orthonormal a_k, b_k (zero beyond row n) and singular values s_k drawn from [0.5, 1] --
    rank 0: a zero tile; the diagonal tiles are random symmetric.  The live rows of the last row block bound the ranks of
    its tiles (asserted)."""
    rng = np.random.default_rng(seed)
    nt = tiles_of(n)
    G = np.zeros((n, n))
    for I in range(nt):
        ri = min(DT, n - I * DT)
        for J in range(I):
            r = int(rank_table[I][J])
            assert 0 <= r <= ri, (I, J, r, ri)
            if r == 0:
                continue
            a, b = _orthonormal(rng, ri, r), _orthonormal(rng, DT, r)
            s = rng.uniform(0.5, 1.0, r)
            tile = (a * s) @ b.T
            G[I * DT:I * DT + ri, J * DT:(J + 1) * DT] = tile
            G[J * DT:(J + 1) * DT, I * DT:I * DT + ri] = tile.T
        m = rng.standard_normal((ri, ri)) / np.sqrt(DT)
        G[I * DT:I * DT + ri, I * DT:I * DT + ri] = 0.5 * (m + m.T)
    return G


def uniform_ranks(nt, r):
    return [[r] * nt for _ in range(nt)]


def rank_table_703():
    """nt = 6, every rank of {0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33}: R_K = 47, 74, 0, 21, 16, 46 (R_K mod 4 = 3, 2, 0, 1,
    0, 2); row block 2 has no column (its partners are dense or of rank 0) between blocks that have some; the dense
    off-diagonal tiles (2, 1), (4, 2), (5, 2) stand next to factor pairs."""
    t = [[0] * 6 for _ in range(6)]
    t[1][0] = 32
    t[2][0], t[2][1] = 0, 33
    t[3][0], t[3][1], t[3][2] = 7, 9, 0
    t[4][0], t[4][1], t[4][2], t[4][3] = 5, 2, 33, 1
    t[5][0], t[5][1], t[5][2], t[5][3], t[5][4] = 3, 31, 33, 4, 8
    return t


def rank_table_768_mixed():
    """nt = 6: row block 5's partners of ranks 32, 32, 32, 32, 2 (R_5 = 130, padded to 132: 33 groups), 32 elsewhere."""
    t = uniform_ranks(6, 32)
    t[5][4] = 2
    return t


def rank_table_1025(seed=5):
    """nt = 9, ranks random in 0 .. 12; the last row block has one live row: ranks 0 or 1 there."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 13, size=(9, 9)).tolist()
    t[8] = rng.integers(0, 2, size=9).tolist()
    t[8][3] = 1
    return t


def block_column_counts(rank_table, nt):
    """R_K (before padding) that a rank table gives: ranks >= 33 are dense tiles and contribute nothing."""
    R = [0] * nt
    for I in range(nt):
        for J in range(I):
            r = int(rank_table[I][J])
            if r <= KMAX:
                R[I] += r
                R[J] += r
    return R


# ---- the cases of the host and the GPU tests: the smallest sizes at which each branch of the layout exists --------------
TOL_ABS = 1e-9
CASES = {
    "n100": (100, lambda: uniform_ranks(1, 0)),              # one diagonal tile, no column, no item
    "n129_rank1": (129, lambda: uniform_ranks(2, 1)),        # last block: one live row; 1 column padded to 4
    "n193_rank3": (193, lambda: uniform_ranks(2, 3)),        # the second 64-row half of the last block holds one row
    "n703_mixed": (703, rank_table_703),                     # every R_K mod 4, an empty block, dense tiles among pairs
    "n768_rank32": (768, lambda: uniform_ranks(6, 32)),      # R_K = 160: 40 groups, 5 items, two trips of the finish loop
    "n768_r130": (768, rank_table_768_mixed),                # R_5 = 130 -> 132: 33 groups, an item of one group
    "n1025_random": (1025, rank_table_1025),                 # nt = 9, the last block one row
}


def case_matrix(name):
    """(G, rank table) of case ``name`` (deterministic)."""
    n, table = CASES[name]
    table = table()
    return prescribed_matrix(n, table, seed=1000 + list(CASES).index(name)), table
