"""Float64 model of ONE application of the V-cycle in the precisions the device stores it in (`vcycle0_f32`,
csrc/vcycle.inc; `TDGLContext.vcycle_stored`), for tests/test_vcycle_model_host.py and tests/test_hip_vcycle_stored.py.
Host only: NumPy / SciPy and `tdgl_amd.amg`.

The device keeps every VECTOR below level 0 and all its arithmetic in fp64; what is reduced is the storage of the
operators and of the two level-0 iterates.  So the model rounds the objects the device rounds -- the PRE-MULTIPLIED
F = R (I - c A D^-1), R A, A P, M, W, V, G, B, never their factors -- and evaluates in fp64:

    bc = F~ b;   xc = coarse(bc)                      (fp64 vectors below level 0)
    x  = fl32(c d~inv b + P~ xc)
    z  = fl32(x + c d~inv (b - A~ x))

`Storage` says what `~` means per operator group: None (exact), np.float32 or np.float16.  With `Storage.exact()` the
model is `vcycle_collapsed_host` (with a plan) or `vcycle_host` (without) re-associated.

coarse(): the recursion of `vcycle_collapsed_host` through the rounded plan -- an intermediate level with explicit
operators is  e = W~ b + V~ coarse(M~ b),  the tail  B~ b  or  y = G~ b, W~ [b ; y] + V~ y[:v]  -- and, for a level that
has no explicit operators (collapse=False), the fused level of the device: the two-step pre-smoothing on A~, the
restricted residual R~ b - (RA)~ x, then x' = x + P~ e with the first post-smoothing step through A~ x + (AP)~ e (P~ on
AP's pattern), the remaining steps on A~; dinv and the coarsest pseudo-inverse stay fp64 there.

`Faults` plants the mistakes a SELL / offset-form builder can make into the level-0 operators (sensitivity tests)."""

from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import scipy.sparse as sp

from tdgl_amd.amg import fused_level_operators, fused_restriction, smoother_coefficients

WAVE = 64  # rows per SELL slice (csrc/tdgl_internal.h)
ULP32 = 2.0 ** -23  # one unit in the last place of an fp32 number, relative to it, at most
FLOOR = 1e-12  # relative to max |z|: what tests/test_hip_parity.py holds the fp64 cycle's restatements to
UNEQUAL_CAP = 1e-4  # share of entries that may differ from the model as fp32 numbers (a rounding falling the other way)


@dataclass
class Storage:
    level0: Optional[type] = None   # A, P, F of level 0
    dinv0: Optional[type] = None    # level-0 dinv
    iterates: Optional[type] = None  # the two level-0 iterates x and z
    coarse: Optional[type] = None   # M, the tail's G / W / V / B, a fused level's A, R, RA, AP, P
    mid: dict = field(default_factory=dict)  # {k: dtype} of an intermediate level's explicit W, V (default: `coarse`)

    @classmethod
    def exact(cls):
        return cls()

    @classmethod
    def mode(cls, mode, level0_f16=None, mid_f16=()):
        """What the device stores for ``precond_fp32 = mode``: 1 = fp32 throughout; 2 = binary16 for A, P, F of level 0
        when it takes that path (``level0_f16``, default yes) and for W, V of the intermediate levels ``mid_f16``."""
        if mode == 0:
            return cls.exact()
        f16 = mode == 2 and (True if level0_f16 is None else bool(level0_f16))
        return cls(level0=np.float16 if f16 else np.float32, dinv0=np.float32, iterates=np.float32, coarse=np.float32,
                   mid={int(k): np.float16 for k in (mid_f16 if mode == 2 else ())})


@dataclass
class Faults:
    """Mistakes planted into the level-0 operators as the device would see them."""
    p_column_shift_row: Optional[int] = None   # the first column index of this row of P moved by one
    p_slice_base_shift: Optional[int] = None   # every column of P's rows in this slice moved by one (slice_base off by one)
    a_padded_slot_row: Optional[int] = None    # a padded SELL slot of this row of A holds the row's first value again
    dinv_unrounded: bool = False               # dinv stays fp64


def rounded(M, dt):
    """``M`` (sparse or dense) with its values rounded to ``dt`` and widened again; ``dt`` None: ``M`` itself."""
    if dt is None:
        return M
    if sp.issparse(M):
        M = M.tocsr(copy=True)
        M.data = M.data.astype(dt).astype(np.float64)
        return M
    return np.asarray(M).astype(dt).astype(np.float64)


def _shift_columns(P, rows, first_only):
    """``P`` with the column indices of ``rows`` moved by one (down where the row's largest column is the last one)."""
    P = P.tocsr(copy=True)
    P.sort_indices()
    idx = P.indices.copy()
    for i in rows:
        lo, hi = P.indptr[i], P.indptr[i + 1]
        if hi == lo:
            continue
        step = 1 if idx[lo:hi].max() + 1 < P.shape[1] else -1
        if first_only:
            # (the moved index must not land on another entry of the row: that would only re-weight it)
            taken = set(idx[lo:hi].tolist())
            k = next(k for k in range(lo, hi) if idx[k] + step not in taken)
            idx[k] += step
        else:
            idx[lo:hi] += step
    # (no canonical form: scipy's products take the entries as they stand)
    return sp.csr_matrix((P.data.copy(), idx, P.indptr.copy()), shape=P.shape)


def sell_padded_rows(A):
    """Rows of ``A`` that have at least one padded slot in the 64-row SELL layout (fewer entries than their slice's widest)."""
    deg = np.diff(A.tocsr().indptr)
    n = len(deg)
    width = np.maximum.reduceat(deg, np.arange(0, n, WAVE))
    return np.flatnonzero(deg < np.repeat(width, WAVE)[:n])


class StoredCycle:
    """The cycle of hierarchy ``h`` through ``plan`` (`collapsed_operators`' dict, or None: every level below level 0
    is a fused level) with the operators rounded as ``storage`` says.  ``apply(B)``: every column of ``B [n, k]``."""

    def __init__(self, h, plan=None, storage=None, nu=2, smoother="chebyshev", cheb_lo=0.1, faults=None):
        st = storage or Storage.exact()
        fl = faults or Faults()
        self.h, self.st, self.nu, self.smoother, self.cheb_lo = h, st, nu, smoother, cheb_lo
        lv = h.levels[0]
        assert len(h.levels) >= 2, "the stored-precision cycle needs two levels"
        self.c = smoother_coefficients(lv.rho, 1, smoother, cheb_lo)[1][0]
        A0, P0 = lv.A.tocsr(), lv.P.tocsr()
        if fl.p_column_shift_row is not None:
            P0 = _shift_columns(P0, [fl.p_column_shift_row], first_only=True)
        if fl.p_slice_base_shift is not None:
            s = fl.p_slice_base_shift
            P0 = _shift_columns(P0, range(s * WAVE, min((s + 1) * WAVE, P0.shape[0])), first_only=False)
        if fl.a_padded_slot_row is not None:
            i = fl.a_padded_slot_row
            assert i in sell_padded_rows(A0)
            k = A0.indptr[i]  # (the padding repeats the row's first column; here with its value)
            A0 = (A0 + sp.csr_matrix(([A0.data[k]], ([i], [A0.indices[k]])), shape=A0.shape)).tocsr()
        self.F = rounded(fused_restriction(h, self.c), st.level0)
        self.A0, self.P0 = rounded(A0, st.level0), rounded(P0, st.level0)
        self.dinv0 = lv.dinv if fl.dinv_unrounded else rounded(lv.dinv, st.dinv0)
        self.plan = None
        if plan is not None:
            p = dict(plan)
            p["mid"] = {k: rounded(M, st.coarse) for k, M in plan["mid"].items()}
            p["up"] = {k: tuple(rounded(M, st.mid.get(k, st.coarse)) for M in WV) for k, WV in plan.get("up", {}).items()}
            for key in ("G", "W", "V", "B"):
                if key in p:
                    p[key] = rounded(p[key], st.coarse)
            self.plan = p
        self._fused = {}

    # -- the levels below level 0 -----------------------------------------------------------------------------------
    def _fused_level(self, k):
        """(A, R, RA, AP, P on AP's pattern) of level ``k``, rounded: what `tdgl_poisson_set_fused_level` holds."""
        if k not in self._fused:
            lv = self.h.levels[k]
            RA, AP, p_on_ap = fused_level_operators(lv)
            Pp = sp.csr_matrix((p_on_ap, AP.indices, AP.indptr), shape=AP.shape)
            self._fused[k] = tuple(rounded(M, self.st.coarse) for M in (lv.A.tocsr(), lv.R.tocsr(), RA, AP, Pp))
        return self._fused[k]

    def coarse(self, k, b):
        h, plan, nu = self.h, self.plan, self.nu
        if k == len(h.levels) - 1:
            return h.coarse_pinv @ b
        if plan is not None and k == plan["tail"]:
            if plan["mode"] == "dense":
                return plan["B"] @ b
            y = plan["G"] @ b
            return plan["W"] @ np.concatenate([b, y]) + plan["V"] @ y[: plan["V"].shape[1]]
        if plan is not None and k in plan["up"]:
            W, V = plan["up"][k]
            return W @ b + V @ self.coarse(k + 1, plan["mid"][k] @ b)
        lv = h.levels[k]
        A, R, RA, AP, Pp = self._fused_level(k)
        dinv = lv.dinv[:, None] if b.ndim == 2 else lv.dinv
        c1, c2 = smoother_coefficients(lv.rho, nu, self.smoother, self.cheb_lo)
        d = c2[0] * dinv * b
        x = d.copy()
        for s in range(1, nu):
            d = c1[s] * d + c2[s] * dinv * (b - A @ x)
            x = x + d
        bc = plan["mid"][k] @ b if (plan is not None and k in plan["mid"]) else R @ b - RA @ x
        e = self.coarse(k + 1, bc)
        # x' = x + P e and the first post-smoothing step, A x' formed as A x + (A P) e
        d = c2[0] * dinv * (b - (A @ x + AP @ e))
        x = (x + Pp @ e) + d
        for s in range(1, nu):
            d = c1[s] * d + c2[s] * dinv * (b - A @ x)
            x = x + d
        return x

    # -- level 0 ------------------------------------------------------------------------------------------------------
    def apply(self, B):
        B = np.asarray(B, dtype=np.float64)
        dinv = self.dinv0[:, None] if B.ndim == 2 else self.dinv0
        xc = self.coarse(1, self.F @ B)
        x = rounded(self.c * dinv * B + self.P0 @ xc, self.st.iterates)
        return rounded(x + self.c * dinv * (B - self.A0 @ x), self.st.iterates)


# ---- probe columns --------------------------------------------------------------------------------------------------
def probe_rows(h):
    """Rows of level 0 (the hierarchy's own order) where a kernel of the cycle can go wrong, as {row: why}: the ends of
    the first workgroups' slices, the last row, a row of largest and one of smallest degree, the fine rows of the first
    and the last aggregate, and the first row of P's last slice."""
    lv = h.levels[0]
    n = lv.A.shape[0]
    deg = np.diff(lv.A.tocsr().indptr)
    rows = {}
    for j in (0, 63, 64, 255, 256, n - 1):
        rows.setdefault(int(j), f"row {j}")
    rows.setdefault(int(np.argmax(deg)), "largest degree")
    rows.setdefault(int(np.argmin(deg)), "smallest degree")
    n_coarse = lv.P.shape[1]
    for i in np.flatnonzero(lv.agg == 0):
        rows.setdefault(int(i), "aggregate 0")
    for i in np.flatnonzero(lv.agg == n_coarse - 1):
        rows.setdefault(int(i), "last aggregate")
    rows.setdefault(int((n - 1) // WAVE * WAVE), "first row of the last slice")
    return rows


def probe_columns(h, coords, seed=11):
    """``(B [n, k], names)`` in the hierarchy's order: e_j - 1/n for `probe_rows`, one smooth column (cos of the site
    coordinates ``coords [n, 2]``, given in the same order) and four standard-normal ones, every column with zero mean."""
    n = h.levels[0].A.shape[0]
    rows = probe_rows(h)
    cols, names = [], []
    for j, why in rows.items():
        e = np.full(n, -1.0 / n)
        e[j] += 1.0
        cols.append(e)
        names.append(f"e_{j} ({why})")
    span = np.ptp(coords, axis=0)
    smooth = np.cos(np.pi * (coords[:, 0] - coords[:, 0].min()) / span[0]) * np.cos(np.pi * (coords[:, 1] - coords[:, 1].min()) / span[1])
    cols.append(smooth - smooth.mean())
    names.append("cos x cos y")
    rng = np.random.default_rng(seed)
    for k in range(4):
        v = rng.standard_normal(n)
        cols.append(v - v.mean())
        names.append(f"normal {k}")
    return np.column_stack(cols), names


# ---- the comparison the GPU test makes ------------------------------------------------------------------------------
def compare(z, z_model):
    """``z`` against ``z_model`` ([n] or [n, k], both holding fp32 numbers): dict(excess = entries beyond
    2^-23 |z_model| + 1e-12 max |z_model| per column, unequal = entries that differ as fp32 numbers, size, ulps = the
    largest deviation in units of the model entry's fp32 spacing)."""
    z, zm = np.atleast_2d(np.asarray(z).T).T, np.atleast_2d(np.asarray(z_model).T).T
    dev = np.abs(z - zm)
    bound = ULP32 * np.abs(zm) + FLOOR * np.abs(zm).max(axis=0)
    unequal = z.astype(np.float32) != zm.astype(np.float32)
    # (entries near zero by cancellation are measured in units of the floor, not of their own tiny spacing)
    unit = np.maximum(np.spacing(np.abs(zm).astype(np.float32)).astype(np.float64), FLOOR * np.abs(zm).max(axis=0))
    ulps = dev / unit
    return dict(excess=int((dev > bound).sum()), excess_columns=np.flatnonzero((dev > bound).any(axis=0)),
                unequal=int(unequal.sum()), size=int(z.size), ulps=float(ulps.max()))


def within_tolerance(cmp) -> bool:
    """The two conditions of tests/test_hip_vcycle_stored.py on `compare`'s result."""
    return cmp["excess"] == 0 and cmp["unequal"] <= UNEQUAL_CAP * cmp["size"]


def storage_error(z_rounded, z_exact):
    """s per column: max |z_rounded - z_exact| / max |z_exact|."""
    return np.abs(z_rounded - z_exact).max(axis=0) / np.abs(z_exact).max(axis=0)
