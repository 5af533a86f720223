"""What the tests of the moving current loops share (tests/test_moving_loop_host.py, tests/test_hip_moving_loop.py): a NumPy
restatement of the loop's vector potential without cancellation, the loops' tables in the library's arithmetic, the
fixture's field as the library's arguments, and the terms' `StepRule` extended by the loops' four values."""

import numpy as np

from field_terms_model import factor_end, factor_value, table_value

AGM_STEPS = 6


def loop_H(dx, dy, z, a):
    """H = G / rho of a loop of radius ``a`` at the in-plane offsets dx, dy from its axis, a height z != 0 from its plane:
    A = I H (-dy, dx).  With d^2 = (a + rho)^2 + z^2, m = 4 a rho / d^2:  (2 - m) K - 2 E = K sum_n 2^n c_n^2 over the
    differences of the arithmetic-geometric mean, b0 = sqrt(1 - m) without forming 1 - m, c_0 / rho = 2 a / (d^2 (1 + b0))
    carried next to c_0 so that nothing is divided by rho; AGM_STEPS halvings, no exit that depends on the data."""
    dx, dy, z = np.broadcast_arrays(np.asarray(dx, dtype=float), np.asarray(dy, dtype=float), np.asarray(z, dtype=float))
    rho = np.sqrt(dx * dx + dy * dy)
    z2, sp, sm = z * z, a + rho, a - rho
    d2 = sp * sp + z2
    b0 = np.sqrt((sm * sm + z2) / d2)
    ob = 1.0 + b0
    cr = (2.0 * a) / (d2 * ob)
    c = cr * rho
    an, bn, sr, p = 0.5 * ob, np.sqrt(b0), 2.0 * (cr * cr), 4.0
    with np.errstate(under="ignore"):
        for _ in range(AGM_STEPS):
            a1 = 0.5 * (an + bn)
            bn = np.sqrt(an * bn)
            q = c / (4.0 * a1)
            cr, c = cr * q, c * q
            sr = sr + p * (cr * cr)
            p, an = p * 2.0, a1
    return (sr * np.sqrt(d2)) / (8.0 * an)


def loop_G(dx, dy, z, a):
    """The dimensionless G = A_phi / (mu_0 I) = rho H."""
    return np.sqrt(np.asarray(dx, dtype=float) ** 2 + np.asarray(dy, dtype=float) ** 2) * loop_H(dx, dy, z, a)


def loop_A(points, z_film, centre, a, current):
    """[n, 2]: I H (-dy, dx) at ``points`` [n, 2] in the film's plane, for a loop centred at ``centre`` (x, y, z)."""
    dx, dy = points[:, 0] - centre[0], points[:, 1] - centre[1]
    h = current * loop_H(dx, dy, z_film - centre[2], a)
    return np.column_stack([-(dy * h), dx * h])


def loop_values(loop, t):
    """Centre x, y, z and current of ``loop`` (dict(times, centers[n, 3], currents[n], radius)) at t: `table_value`."""
    c = np.asarray(loop["centers"], dtype=float)
    return [table_value(t, loop["times"], c[:, j]) for j in range(3)] + [table_value(t, loop["times"], loop["currents"])]


def loops_field(points, z_film, loops, t, under=None):
    """``under`` (the static part or the terms' sum at t; None: zero) plus the loops in loop order."""
    A = np.zeros((len(points), 2)) if under is None else np.array(under, dtype=float)
    for lp in loops:
        v = loop_values(lp, t)
        A = A + loop_A(points, z_film, v[:3], lp["radius"], v[3])
    return A


def fixture_loop(g):
    """The loop of fixture traj_moving_loop_small as `vector_potential_loops` takes it."""
    return dict(times=g["loop_times"], centers=g["loop_centers"], currents=g["loop_currents"], radius=float(g["loop_radius"]))


class StepRule:
    """`field_terms_model.StepRule` extended: a step moves nothing only when every factor AND every loop's four values
    equal their last two evaluations and a dynamic update has run; settled once the time has passed every term's end and
    every loop's last node and everything has been seen twice at its end value."""

    def __init__(self, specs, loops):
        self.specs, self.loops = list(specs), list(loops)
        self.cur = self._evaluate(0.0)
        self.prev = list(self.cur)
        self.has_dadt = False
        self.moves = 0

    def _evaluate(self, t):
        return [factor_value(s, t) for s in self.specs] + [v for lp in self.loops for v in loop_values(lp, t)]

    def _ends(self):
        ends = [factor_end(s) for s in self.specs]
        for lp in self.loops:
            c = np.asarray(lp["centers"], dtype=float)
            t_end = float(lp["times"][-1])
            ends += [(t_end, float(c[-1, j])) for j in range(3)] + [(t_end, float(lp["currents"][-1]))]
        return ends

    def settled(self, time):
        return all(time >= te and a == ve and b == ve for (te, ve), a, b in zip(self._ends(), self.cur, self.prev))

    def begin_step(self, time):
        """'settled', 'skip' or 'move'."""
        if self.settled(time):
            self.has_dadt = False
            return "settled"
        v = self._evaluate(time)
        if self.has_dadt and v == self.cur and v == self.prev:
            return "skip"
        self.prev, self.cur, self.has_dadt = self.cur, v, True
        self.moves += 1
        return "move"
