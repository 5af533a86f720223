"""Generate `loop_potential_reference.npz`: the vector potential of a current loop at prescribed points, from the REFERENCE's
own `em.current_loop_vector_potential` and from 40-digit arithmetic (build container only; needs mpmath).

    python tests/golden/generate_golden_loop.py [--out DIR]

Three loop geometries (radius, centre with height), each with its own 1,458 points (mesh_small's edge count) in the film's
plane z = 0, placed around the loop's axis at distances rho spread logarithmically so that m = 4 a rho / ((a + rho)^2 + z^2)
covers [1e-12, 1 - 1e-8]: about 200 points hug the wire, one lies exactly on the axis.  What is exact is computed from the
differences points - centre as a double forms them, so every evaluation sees the same rho.

Stored: the geometries and points, `A_reference` (the reference's values in T m for a current of 1 uA and lengths in um) and
its `mu_0`, `G_exact` = A_phi / (mu_0 I) at 40 digits, `reference_ok` = |ref / (mu_0 I) - G_exact| <= 1e-10 G_exact (the
reference's formula cancels for small m and is NaN on the axis), and `model_worst_rel`, the worst relative error of the
NumPy restatement in tests/loop_field_model.py against `G_exact`.  Data only (no reference source text).
"""

import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import generate_golden as gg  # noqa: E402  (imports the reference through _reference_shim)
from loop_field_model import loop_G  # noqa: E402
from tdgl import em  # noqa: E402

N_POINTS = 1458
# radius, centre x, y, z; the film is the plane z = 0.  The third hugs the film: 1 - m reaches (z / 2a)^2 = 1e-8
GEOMETRIES = np.array([[2.0, 0.25, -0.125, 1.0], [0.5, -3.0, 2.0, -0.25], [1.5, 1.0, 1.0, 3e-4]])
CURRENT_UA = 1.0


class _Quantity:
    """Stand-in for what the reference asks of its unit registry: lengths in um and currents in uA to SI, and a unit an
    array may be multiplied by without changing."""

    __array_ufunc__ = None  # (ndarray * _Quantity -> _Quantity.__rmul__)

    def __init__(self, magnitude=1.0):
        self.magnitude = magnitude

    def to(self, _units):
        return self

    def __rmul__(self, other):
        return other


class _Units:
    FACTORS = {"um": 1e-6, "uA": 1e-6}

    def __call__(self, name):
        return _Quantity(self.FACTORS.get(name, 1.0))


def make_points(rng, a, cx, cy):
    n_wire, n_mid = 200, 800
    n_far = N_POINTS - 1 - n_wire - n_mid
    wire = a * (1.0 + rng.choice([-1.0, 1.0], n_wire) * 10.0 ** rng.uniform(-9, -2, n_wire))
    mid = a * 10.0 ** rng.uniform(-2.4, 2.4, n_mid)
    far = a * 10.0 ** np.where(rng.random(n_far) < 0.5, rng.uniform(-13, -2.4, n_far), rng.uniform(2.4, 13, n_far))
    rho = np.concatenate([[0.0], wire, mid, far])
    th = rng.uniform(0, 2 * np.pi, N_POINTS)
    ux, uy = np.cos(th), np.sin(th)
    # The points at the wire lie along +-x and +-y from the axis, so that rho = |dx| or |dy| is a double: next to the wire a
    # change of rho by one unit in the last place moves G by up to 3e-14 (relative, third geometry), and the comparison is to
    # measure the algorithm, not how well G is conditioned with respect to a rounded sqrt(dx^2 + dy^2)
    quarter = rng.integers(0, 4, n_wire)
    ux[1:1 + n_wire], uy[1:1 + n_wire] = np.array([1.0, 0.0, -1.0, 0.0])[quarter], np.array([0.0, 1.0, 0.0, -1.0])[quarter]
    return np.column_stack([cx + rho * ux, cy + rho * uy])


def exact_G(dx, dy, z, a):
    # (40 correct digits: (2 - m) K - 2 E loses 2 log10(1 / m) digits to cancellation, up to 26 here, so work with 70)
    mp.mp.dps = 70
    out = np.zeros(len(dx))
    for k in range(len(dx)):
        x, y = mp.mpf(float(dx[k])), mp.mpf(float(dy[k]))
        rho = mp.sqrt(x * x + y * y)
        if rho == 0:
            continue
        d2 = (mp.mpf(a) + rho) ** 2 + mp.mpf(z) ** 2
        m = 4 * mp.mpf(a) * rho / d2
        out[k] = float(((2 - m) * mp.ellipk(m) - 2 * mp.ellipe(m)) * mp.sqrt(d2) / (4 * mp.pi * rho))
    return out


def main():
    em.ureg = _Units()
    rng = np.random.default_rng(20261019)
    points = np.zeros((len(GEOMETRIES), N_POINTS, 2))
    A_ref = np.zeros((len(GEOMETRIES), N_POINTS, 2))
    G_exact = np.zeros((len(GEOMETRIES), N_POINTS))
    ok = np.zeros((len(GEOMETRIES), N_POINTS), dtype=bool)
    m_all, worst = [], 0.0
    for g, (a, cx, cy, cz) in enumerate(GEOMETRIES):
        points[g] = make_points(rng, a, cx, cy)
        dx, dy = points[g, :, 0] - cx, points[g, :, 1] - cy
        rho = np.hypot(dx, dy)
        G_exact[g] = exact_G(dx, dy, 0.0 - cz, a)
        pos = np.column_stack([points[g], np.zeros(N_POINTS)])
        with np.errstate(all="ignore"):
            ref = np.asarray(em.current_loop_vector_potential(pos, loop_center=(cx, cy, cz), loop_radius=a, current=CURRENT_UA,
                                                              length_units="um", current_units="uA"))
        A_ref[g] = ref[:, :2]
        with np.errstate(all="ignore"):
            G_ref = (-dy * ref[:, 0] + dx * ref[:, 1]) / rho / (em.mu_0 * CURRENT_UA * 1e-6)
            ok[g] = np.abs(G_ref - G_exact[g]) <= 1e-10 * G_exact[g]
        ok[g, 0] = False  # (the axis: G_exact = 0, the reference NaN)
        model = loop_G(dx, dy, 0.0 - cz, a)
        assert model[0] == 0.0 and G_exact[g, 0] == 0.0
        worst = max(worst, float(np.max(np.abs(model[1:] - G_exact[g, 1:]) / G_exact[g, 1:])))
        m_all.append(4 * a * rho[1:] / ((a + rho[1:]) ** 2 + cz * cz))
    m_all = np.concatenate(m_all)
    print("m in [%.3g, 1 - %.3g]; reference_ok %.3f; model_worst_rel %.3g; min m among not-ok %.3g, max m among not-ok %.3g" % (
        m_all.min(), 1 - m_all.max(), ok.mean(), worst, m_all[~ok[:, 1:].ravel()].min(), m_all[~ok[:, 1:].ravel()].max()))
    assert m_all.min() <= 1e-12 and 1 - m_all.max() <= 1.01e-8
    assert ok.mean() >= 0.6
    assert worst <= 1e-14
    gg.save("loop_potential_reference", geometries=GEOMETRIES, points=points, current_uA=CURRENT_UA, A_reference=A_ref,
            mu_0=em.mu_0, G_exact=G_exact, reference_ok=ok, model_worst_rel=worst)


if __name__ == "__main__":
    main()
