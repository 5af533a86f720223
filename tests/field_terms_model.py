"""What the tests of the sums of field terms share (tests/test_field_terms_host.py, tests/test_hip_field_terms.py): the
fixture's field as the library's arguments, the two factor evaluators in the library's arithmetic, the left-to-right sum,
and a NumPy model of the step rule (move, skip, settled)."""

from bisect import bisect_right

import numpy as np


def ramp_value(t, tmin, tmax, initial, final):
    """linear_ramp_value (csrc/kernels.inc), operation for operation."""
    if t < tmin:
        return initial
    if t < tmax:
        return initial + (final - initial) * (t - tmin) / (tmax - tmin)
    return final


def table_value(t, times, values):
    """table_value (csrc/kernels.inc), operation for operation: not np.interp, whose last bit may differ."""
    times, values = [float(x) for x in times], [float(x) for x in values]
    if t <= times[0]:
        return values[0]
    if t >= times[-1]:
        return values[-1]
    k = bisect_right(times, t)
    t0, t1 = times[k - 1], times[k]
    return values[k - 1] + (values[k] - values[k - 1]) * ((t - t0) / (t1 - t0))


def factor_value(spec, t):
    return ramp_value(t, spec["tmin"], spec["tmax"], spec["initial"], spec["final"]) if isinstance(spec, dict) else table_value(t, *spec)


def factor_end(spec):
    """(time from which the factor is constant, its value there)."""
    return (spec["tmax"], spec["final"]) if isinstance(spec, dict) else (float(spec[0][-1]), float(spec[1][-1]))


def terms_sum(A0, bases, scales):
    """((A0 + s_1 A_1) + s_2 A_2) + ..., every product rounded before it is added; without A0 from the first product."""
    A = scales[0] * bases[0]
    if A0 is not None:
        A = A0 + A
    for s, base in zip(scales[1:], bases[1:]):
        A = A + s * base
    return A


def flux_spot_A(mesh, x, y, sigma, flux):
    """The vector potential of a Gaussian flux spot on the edge centres: A_phi = flux / (2 pi r) (1 - exp(-r^2 / 2 sigma^2))."""
    c = mesh.edge_mesh.centers
    dx, dy = c[:, 0] - x, c[:, 1] - y
    r2 = np.maximum(dx * dx + dy * dy, 1e-24)
    g = flux / (2 * np.pi * r2) * -np.expm1(-r2 / (2 * sigma**2))
    return np.column_stack([-g * dy, g * dx])


def fixture_terms(g):
    """``(A0, [(A_1, ramp), (A_2, table)])`` of fixture traj_field_terms_small: `vector_potential_terms`."""
    ramp = {k: float(g["ramp_" + k]) for k in ("tmin", "tmax", "initial", "final")}
    return g["A0"], [(g["A1"], ramp), (g["A2"], (g["table_times"], g["table_values"]))]


class StepRule:
    """The rule of the time loop for a sum of terms, one `begin_step(time)` per step (retries never get here).

    A step moves nothing only when every factor equals its last two evaluations and a dynamic update has run.  The field
    is settled once the time has passed every term's end and every factor has been seen twice at its end value; from then
    on nothing is evaluated and there is no dA/dt term."""

    def __init__(self, specs):
        self.specs = list(specs)
        self.scale = [factor_value(s, 0.0) for s in self.specs]
        self.prev = list(self.scale)
        self.has_dadt = False
        self.moves = 0

    def settled(self, time):
        return all(time >= factor_end(s)[0] and a == factor_end(s)[1] and b == factor_end(s)[1]
                   for s, a, b in zip(self.specs, self.scale, self.prev))

    def begin_step(self, time):
        """'settled', 'skip' or 'move'."""
        if self.settled(time):
            self.has_dadt = False
            return "settled"
        s = [factor_value(spec, time) for spec in self.specs]
        if self.has_dadt and s == self.scale and s == self.prev:
            return "skip"
        self.prev, self.scale, self.has_dadt = self.scale, s, True
        self.moves += 1
        return "move"


def ulp_close(a, b, ulps, magnitude=None):
    """|a - b| <= ulps * spacing(magnitude) elementwise (magnitude: max(|a|, |b|) unless given)."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    mag = np.maximum(np.abs(a), np.abs(b)) if magnitude is None else np.asarray(magnitude, dtype=float)
    return bool(np.all(np.abs(a - b) <= ulps * np.spacing(mag)))
