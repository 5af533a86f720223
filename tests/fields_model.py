"""Host-side yardstick for the fields of sheet currents (tests/test_fields_host.py, tests/test_hip_fields.py).

`host_sums` evaluates, in float64 NumPy and in target chunks, the bare all-pairs sums that `tdgl_field_plan_eval`
returns (no mu_0 / 4 pi), with the formulas of the host backend of `Solution.field_at_position` /
`vector_potential_at_position`, and next to every sum the sum of the magnitudes of its terms.

The yardstick.  A sum of N terms t_j evaluated in fp64 in any order, each term carrying a few roundings (the
corrected 1 / sqrt, its cube, the products), is off by at most (N + 16) * 2^-53 * sum_j |t_j|.  N is the number of
sources.  The terms are the products that are accumulated, as the reference's own loop accumulates them
(`tdgl/em.py:_biot_savart_2d_z` keeps `pref * Jx * dy` and `pref * Jy * dx` in two separate sums): for B_z that is
a_j |Kx_j dy| / r^3 + a_j |Ky_j dx| / r^3, not |Kx_j dy - Ky_j dx|, because the difference inside one term can cancel
and no fp64 evaluation -- the host's and the reference's included -- is accurate relative to the cancelled value.
"""

import numpy as np

U = 2.0 ** -53


def yardstick(n_sources: int, abs_sum):
    return (n_sources + 16) * U * np.asarray(abs_sum)


def host_sums(src_xy, areas, z0, K, targets, chunk=128):
    """K: [nf, n, 2]; targets [m, 3].  Returns a dict of arrays: ``A`` [nf, m, 2], ``Z`` [nf, m], ``XY`` [nf, m, 2]
    and ``A_abs``, ``Z_abs``, ``XY_abs`` of the same shapes (sums of the terms' magnitudes)."""
    src_xy, areas, targets = np.asarray(src_xy, float), np.asarray(areas, float), np.asarray(targets, float)
    K = np.asarray(K, float)
    if K.ndim == 2:
        K = K[None]
    nf, m = len(K), len(targets)
    out = {k: np.zeros((nf, m, 2)) for k in ("A", "A_abs", "XY", "XY_abs")}
    out.update({k: np.zeros((nf, m)) for k in ("Z", "Z_abs")})
    with np.errstate(divide="ignore", invalid="ignore"):
        for lo in range(0, m, chunk):
            t = targets[lo:lo + chunk]
            dx = t[:, None, 0] - src_xy[None, :, 0]
            dy = t[:, None, 1] - src_xy[None, :, 1]
            dz = t[:, 2] - z0
            r2 = dx**2 + dy**2 + dz[:, None] ** 2
            rho, r3 = np.sqrt(r2), r2**1.5
            for f in range(nf):
                J = K[f]
                out["A"][f, lo:lo + chunk] = (J[None, :, :] / rho[:, :, None] * areas[None, :, None]).sum(axis=1)
                out["A_abs"][f, lo:lo + chunk] = (np.abs(J)[None, :, :] / rho[:, :, None] * np.abs(areas)[None, :, None]).sum(axis=1)
                jx, jy = (J[:, 0] * areas)[None, :], (J[:, 1] * areas)[None, :]
                out["Z"][f, lo:lo + chunk] = ((jx * dy - jy * dx) / r3).sum(axis=1)
                out["Z_abs"][f, lo:lo + chunk] = ((np.abs(jx * dy) + np.abs(jy * dx)) / r3).sum(axis=1)
                out["XY"][f, lo:lo + chunk, 0] = (jy * dz[:, None] / r3).sum(axis=1)
                out["XY"][f, lo:lo + chunk, 1] = (-jx * dz[:, None] / r3).sum(axis=1)
                out["XY_abs"][f, lo:lo + chunk, 0] = (np.abs(jy * dz[:, None]) / r3).sum(axis=1)
                out["XY_abs"][f, lo:lo + chunk, 1] = (np.abs(jx * dz[:, None]) / r3).sum(axis=1)
    return out


def worst_ratio(got, want, abs_sum):
    """max |got - want| / sum|t| over the entries whose terms are not all zero (those must agree exactly)."""
    got, want, abs_sum = np.asarray(got), np.asarray(want), np.asarray(abs_sum)
    err = np.abs(got - want)
    zero = abs_sum == 0
    assert np.all(err[zero] == 0)
    return float((err[~zero] / abs_sum[~zero]).max()) if (~zero).any() else 0.0


def assert_within_yardstick(got, want, abs_sum, n_sources, label=""):
    ratio = worst_ratio(got, want, abs_sum)
    bound = (n_sources + 16) * U
    print(f"fields yardstick {label}: max |got - want| / sum|t| = {ratio:.3e}  (bound {bound:.3e}, n = {n_sources})")
    assert ratio <= bound, (label, ratio, bound)
    return ratio
