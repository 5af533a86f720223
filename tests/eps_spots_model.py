"""A NumPy model of the hot spots in epsilon (tdgl_set_epsilon_spots, k_eps_spots), written from the arithmetic the
header states and independent of the package:

    epsilon(r, t) = eps0(r) - sum_k a_k(t) exp(-|r - c_k(t)|^2 / (2 sigma_k(t)^2))

Per site, spots in spot order, every operation rounded on its own:

    dx = x - cx;  dy = y - cy;  d2 = dx*dx + dy*dy
    den = 2.0 * (s*s);  g = exp(-(d2 / den))
    acc = eps0;  acc = acc - a*g

The four values of a spot at time t are piecewise linear over the spot's nodes and constant outside them, by the
library's table_value: v[k-1] + (v[k] - v[k-1]) * ((t - t[k-1]) / (t[k] - t[k-1])) with t[k] the first node behind t.
The only operation in which the device may differ from this model is exp."""

import numpy as np

EPS = 2.0 ** -52


def table_value(times, values, t):
    times, values = np.asarray(times, dtype=float), np.asarray(values, dtype=float)
    t = float(t)
    if t <= times[0]:
        return float(values[0])
    if t >= times[-1]:
        return float(values[-1])
    hi = int(np.searchsorted(times, t, side="right"))
    t0, t1 = times[hi - 1], times[hi]
    return float(values[hi - 1] + (values[hi] - values[hi - 1]) * ((t - t0) / (t1 - t0)))


def spot_values(spots, t):
    """[K, 4] = cx, cy, a, sigma of ``spots`` (dicts of times, centers [n, 2], amplitudes [n], sigmas [n]) at t."""
    out = np.zeros((len(spots), 4))
    for k, s in enumerate(spots):
        c = np.asarray(s["centers"], dtype=float)
        n = len(s["times"])
        cols = (c[:, 0], c[:, 1], np.asarray(s["amplitudes"], dtype=float) * np.ones(n), np.asarray(s["sigmas"], dtype=float) * np.ones(n))
        out[k] = [table_value(s["times"], col, t) for col in cols]
    return out


def epsilon(sites, eps0, values):
    sites = np.asarray(sites, dtype=float)
    x, y = sites[:, 0], sites[:, 1]
    acc = np.asarray(eps0, dtype=float) * np.ones(len(sites))
    for cx, cy, a, s in np.asarray(values, dtype=float).reshape(-1, 4):
        dx = x - cx
        dy = y - cy
        d2 = dx * dx + dy * dy
        den = 2.0 * (s * s)
        g = np.exp(-(d2 / den))
        acc = acc - a * g
    return acc


def value_bound(values):
    """Per-site bound on |epsilon_device - epsilon_model| at the same values, for |eps0| <= 1 and K <= 4 spots:
    8 * 2^-52 * (1 + sum_k a_k).

    Derivation (e = 2^-52).  Everything up to the argument of exp is the same bits on both sides.  OpenCL bounds a double
    exp at 3 ulp and the same is allowed for NumPy's; g = 1 only at d2 = 0, where both are exact, and an ulp of g < 1 is at
    most e / 2: the two g differ by at most 6 ulp <= 3 e.  The product a*g < a is rounded once on either side, by at most
    half an ulp <= a e / 2 each: the two products differ by at most 3 e a + e a = 4 e a.  A subtraction rounds its
    result, of magnitude at most 1 + sum a, by at most half an ulp <= (1 + sum a) e / 2 on either side: e (1 + sum a) per
    subtraction, 4 e (1 + sum a) for K = 4.  Together 4 e sum a + 4 e (1 + sum a) <= 8 e (1 + sum a)."""
    v = np.asarray(values, dtype=float).reshape(-1, 4)
    return 8.0 * EPS * (1.0 + v[:, 2].sum())
