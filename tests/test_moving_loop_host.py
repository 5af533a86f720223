"""Current loops as applied-field sources on the host (no GPU needed): `CurrentLoop` and `MovingCurrentLoop` against 40-digit
values and the reference's own, the axis, the units, `device_sources()` and what it leaves to the per-step path,
`separable_terms()` unchanged, the refusals, the ensemble's message, and the step-rule model pinned to the fixture."""

import pickle

import numpy as np
import pytest

from conftest import load_golden
from field_terms_model import ulp_close
from helpers import GAMMA_DEFAULT, U_DEFAULT, max_abs, options_from_golden, reference_mesh, remove_mean
from loop_field_model import StepRule, fixture_loop, loop_G, loop_values, loops_field
from test_field_terms_host import TIMES, VALUES, _fields, _left_to_right


def _G_from(A, unit):
    return np.hypot(A[:, 0], A[:, 1]) / unit


# ---------------------------------------------------------------- values
def test_current_loop_values_against_the_fixture():
    """|G - G_exact| <= 8 model_worst_rel G_exact on every point (the bound of the GPU test), within 2e-10 G_exact of the
    reference where the reference is within 1e-10, exactly zero and finite on the axis -- for `CurrentLoop`, for
    `MovingCurrentLoop` at a time between two nodes that puts it in the same place, and for the tests' own model."""
    import tdgl_amd as tdgl
    from tdgl_amd.device import MU_0

    f = load_golden("loop_potential_reference")
    bound = 8.0 * float(f["model_worst_rel"])
    assert bound <= 1e-13
    assert abs(MU_0 / float(f["mu_0"]) - 1) < 1e-9  # (the package's constant is CODATA 2018's, to the digits given)
    unit = MU_0 * 1e-6 / (1e-3 * 1e-6)  # mu_0 (1 uA) in mT um
    for g, (a, cx, cy, cz) in enumerate(f["geometries"]):
        pts, G_exact, ok = f["points"][g], f["G_exact"][g], f["reference_ok"][g]
        x, y, z = pts[:, 0], pts[:, 1], np.zeros(len(pts))
        static = tdgl.CurrentLoop(current=float(f["current_uA"]), radius=a, center=(cx, cy, cz))
        # (centre and current reach the geometry's at t = 0.5 exactly: the nodes are symmetric about it)
        moving = tdgl.MovingCurrentLoop([0.0, 1.0], [[cx - 0.5, cy + 0.25, cz], [cx + 0.5, cy - 0.25, cz]], radius=a, current=[0.5, 1.5])
        dx, dy = x - cx, y - cy
        for name, A in (("CurrentLoop", static(x, y, z)), ("MovingCurrentLoop", moving(x, y, z, t=0.5))):
            assert A.shape == (len(pts), 3) and np.all(A[:, 2] == 0) and np.all(np.isfinite(A)), name
            assert A[0, 0] == 0.0 and A[0, 1] == 0.0, name
            G = _G_from(A, unit)
            # (the division by `unit` and the product with it round once each: two more half-spacings)
            assert np.all(np.abs(G - G_exact) <= (bound + 2.3e-16) * G_exact), name
            ref = f["A_reference"][g] / (float(f["mu_0"]) * 1e-6)
            assert np.all(np.abs(G[ok] - np.hypot(ref[ok, 0], ref[ok, 1])) <= 2e-10 * G_exact[ok]), name
            assert np.all(np.abs(A[:, 0] * dx + A[:, 1] * dy) <= 4 * np.spacing(np.abs(A[:, 0] * dx))), name
        model = loop_G(dx, dy, -cz, a)
        assert np.all(np.abs(model - G_exact) <= float(f["model_worst_rel"]) * G_exact)
    assert f["reference_ok"].mean() >= 0.6 and not f["reference_ok"][:, 0].any()


def test_finite_near_the_axis_and_far_away():
    import tdgl_amd as tdgl

    loop = tdgl.CurrentLoop(current=1.0, radius=2.0, center=(0.0, 0.0, 1.0))
    r = np.concatenate([[0.0], 10.0 ** np.arange(-300.0, 150.0, 7.0)])
    A = loop(r, np.zeros_like(r), np.zeros_like(r))
    assert np.all(np.isfinite(A)) and np.all(A[:, 0] == 0) and A[0, 1] == 0 and np.all(A[(r > 0) & (r < 1e60), 1] > 0)
    # near the axis A_phi = mu_0 I rho a^2 / (4 (a^2 + z^2)^(3/2)) to O((rho / a)^2)
    near = r[(r > 1e-200) & (r < 1e-9)]
    want = 1.25663706212e-6 * 1e-6 / 1e-9 * near * 4.0 / (4 * 5.0 ** 1.5)
    assert np.all(np.abs(loop(near, 0 * near, 0 * near)[:, 1] / want - 1) < 1e-14)


def test_units_against_the_field_on_the_axis():
    """B_z = mu_0 I a^2 / (2 (a^2 + z^2)^(3/2)) on the axis, from a central-difference curl of A with h = 1e-3 a.  The
    difference quotient's truncation error is h^2 / 6 times a third derivative of size B / a^2 times a factor of order one:
    1e-6 relative, asserted at 1e-5; rounding adds 1e-16 / 1e-3."""
    import tdgl_amd as tdgl

    a, z, I_mA = 2.0, 1.0, 3.0
    want_T = 1.25663706212e-6 * (I_mA * 1e-3) * (a * 1e-6) ** 2 / (2 * ((a * 1e-6) ** 2 + (z * 1e-6) ** 2) ** 1.5)
    h = 1e-3 * a
    for field_units, per_T in (("mT", 1e3), ("uT", 1e6), ("G", 1e4)):
        loop = tdgl.CurrentLoop(current=I_mA, radius=a, center=(0.5, -0.25, z), current_units="mA", field_units=field_units)
        x, y = 0.5 + np.array([h, -h, 0.0, 0.0]), -0.25 + np.array([0.0, 0.0, h, -h])
        A = loop(x, y, np.zeros(4))
        Bz = (A[0, 1] - A[1, 1]) / (2 * h) - (A[2, 0] - A[3, 0]) / (2 * h)
        assert abs(Bz / (want_T * per_T) - 1) < 1e-5, field_units
    with pytest.raises(ValueError, match="Unsupported current unit"):
        tdgl.CurrentLoop(current=1.0, radius=1.0, center=(0, 0, 1), current_units="furlong")


def test_parameter_behaviour_of_the_moving_loop():
    import tdgl_amd as tdgl

    make = lambda: tdgl.MovingCurrentLoop([0.0, 1.0, 2.0], [[0, 0, 1], [1, 1, 1], [1, 2, 1]], radius=2.0, current=3.0)  # noqa: E731
    p, q = make(), make()
    assert p.time_dependent and p == q and "moving_loop_vector_potential" in repr(p)
    assert pickle.loads(pickle.dumps(p)) == p
    assert p != tdgl.MovingCurrentLoop([0.0, 1.0, 2.0], [[0, 0, 1], [1, 1, 1], [1, 2, 1]], radius=2.5, current=3.0)
    assert set(p.loop) == {"times", "centers", "currents", "radius", "unit_factor"} and np.array_equal(p.loop["currents"], [3.0] * 3)
    x, y, z = np.array([0.3, -1.0]), np.array([0.2, 0.5]), np.zeros(2)
    # constant outside the nodes, the static loop at a node
    assert np.array_equal(p(x, y, z, t=-1.0), p(x, y, z, t=0.0)) and np.array_equal(p(x, y, z, t=5.0), p(x, y, z, t=2.0))
    assert np.array_equal(p(x, y, z, t=1.0), tdgl.CurrentLoop(current=3.0, radius=2.0, center=(1, 1, 1))(x, y, z))
    static = tdgl.CurrentLoop(current=3.0, radius=2.0, center=(1, 1, 1))
    assert not static.time_dependent and static == tdgl.CurrentLoop(current=3.0, radius=2.0, center=[1, 1, 1])
    assert pickle.loads(pickle.dumps(static)) == static


# ---------------------------------------------------------------- the parameter algebra
def test_static_loops_go_to_the_device_as_terms():
    import tdgl_amd as tdgl

    B, F, G, ramp, wave = _fields()
    loop = tdgl.CurrentLoop(current=2.0, radius=1.0, center=(0.5, 0.0, 0.7))
    static, products = (ramp * loop).separable_terms()
    assert static is None and len(products) == 1 and products[0][0].ramp is not None and products[0][1] == loop
    assert (ramp * loop).separable_product() is not None
    static, products = (tdgl.ConstantField(0.1) + wave * loop).separable_terms()
    assert static == tdgl.ConstantField(0.1) and len(products) == 1 and products[0][0].table is not None and products[0][1] == loop


def test_device_sources():
    import tdgl_amd as tdgl
    from tdgl_amd.parameter import FIELD_LOOPS_MAX

    assert FIELD_LOOPS_MAX == 2
    B, F, G, ramp, wave = _fields()
    mk = lambda cur, r=1.0: tdgl.MovingCurrentLoop([0.0, 1.0], [[0, 0, 1], [1, 1, 1]], radius=r, current=cur)  # noqa: E731
    L1, L2, L3 = mk([0.0, 2.0]), mk(1.5, 2.0), mk(1.0, 3.0)
    static, terms, loops = (B + L1).device_sources()
    assert static == B and terms == [] and len(loops) == 1 and np.array_equal(loops[0]["currents"], [0.0, 2.0]) and loops[0]["radius"] == 1.0
    assert L1.device_sources()[0] is None and L1.device_sources()[1] == [] and len(L1.device_sources()[2]) == 1
    static, terms, loops = (L1 + ramp * F + B + L2 - wave * G).device_sources()
    assert static == B and len(terms) == 2 and [lp["radius"] for lp in loops] == [1.0, 2.0]
    assert terms[0][0].ramp is not None and terms[1][0].table is not None
    assert (B + L1 + L2 + L3).device_sources() is None
    static, terms, loops = (B - L2).device_sources()
    assert np.array_equal(loops[0]["currents"], [-1.5, -1.5]) and np.array_equal(L2.loop["currents"], [1.5, 1.5])
    static, terms, loops = (B - (F - L1)).device_sources()
    assert np.array_equal(loops[0]["currents"], [0.0, 2.0]) and static is not None
    for name, p in {"a loop times a ramp": B + ramp * L1, "a loop times a number": B + 2.0 * L1, "a negated loop": B + (-L1),
                    "a quotient": B + L1 / ramp, "five products": L1 + ramp * F + wave * G + ramp * G + wave * F + ramp * B}.items():
        assert p.time_dependent and p.device_sources() is None, name
    # without loops it is separable_terms with an empty third entry; static parameters are the sum without anything else
    assert (B + ramp * F).device_sources() == (*(B + ramp * F).separable_terms(), [])
    assert B.device_sources() == (B, [], [])
    # separable_terms and separable_product do not know loops
    for p in (B + L1, L1, L1 + ramp * F):
        assert p.separable_terms() is None and p.separable_product() is None


def test_separable_terms_is_unchanged_on_the_field_terms_inputs():
    """The cases of tests/test_field_terms_host.py once more, through both methods."""
    B, F, G, ramp, wave = _fields()
    x, y, z = np.array([0.0, 1.0, 2.5, -3.0]), np.array([0.5, -0.5, 0.0, 2.0]), np.zeros(4)
    mag = 2.0 * sum(np.abs(np.asarray(q(x, y, z))) for q in (B, F, G))
    cases = {"static + product": (B + ramp * F, 1, True), "two products, no static part": (ramp * F + wave * G, 2, False),
             "a difference in brackets": (B - (ramp * F - G), 1, True), "three leaves and a scaled static": (2.0 * B + ramp * F - wave * G, 2, True),
             "a single product": (ramp * F, 1, False)}
    for name, (p, K, has_static) in cases.items():
        static, products = p.separable_terms()
        assert len(products) == K and (static is not None) == has_static, name
        s2, p2, loops = p.device_sources()
        assert loops == [] and len(p2) == K and (s2 is not None) == has_static, name
        for t in (0.0, 1.7, 9.0):
            assert ulp_close(_left_to_right((static, products), x, y, z, t), np.asarray(p(x, y, z, t=t)), 4, magnitude=mag), (name, t)
    assert (B + ramp * wave * F).separable_terms() is None and (B + ramp * wave * F).device_sources() is None
    assert TIMES == [1.0, 3.0, 4.5, 7.0] and VALUES == [0.0, 2.0, 2.0, -1.0]


# ---------------------------------------------------------------- refusals
def test_value_errors():
    import tdgl_amd as tdgl
    from tdgl_amd.hipcore import link_loops_args

    good = dict(times=[0.0, 1.0], centers=[[0, 0, 1], [1, 1, 1]], radius=1.0, current=1.0)
    for name, kw in {"decreasing times": dict(times=[1.0, 0.0]), "equal times": dict(times=[1.0, 1.0]),
                     "centers of another length": dict(centers=[[0, 0, 1]] * 3), "centers without z": dict(centers=[[0, 0], [1, 1]]),
                     "currents of another length": dict(current=[1.0, 2.0, 3.0]), "radius 0": dict(radius=0.0),
                     "a non-finite centre": dict(centers=[[0, np.nan, 1], [1, 1, 1]])}.items():
        with pytest.raises(ValueError):
            tdgl.MovingCurrentLoop(**{**good, **kw}), name
    with pytest.raises(ValueError):
        tdgl.CurrentLoop(current=1.0, radius=-1.0, center=(0, 0, 1))
    with pytest.raises(ValueError):
        tdgl.CurrentLoop(current=1.0, radius=1.0, center=(0, 0))
    # the loop's plane in the plane of the points: on evaluation, and before anything reaches the library
    x = np.array([0.0, 1.0])
    with pytest.raises(ValueError, match="plane"):
        tdgl.CurrentLoop(current=1.0, radius=1.0, center=(0, 0, 0.5))(x, x, 0.5 * np.ones(2))
    with pytest.raises(ValueError, match="plane"):
        tdgl.MovingCurrentLoop([0.0, 1.0], [[0, 0, 1], [1, 1, 0]], radius=1.0, current=1.0)(x, x, np.zeros(2), t=1.0)
    ec = np.zeros((4, 2))
    loop = dict(times=[0.0, 1.0], centers=np.array([[0, 0, 1.0], [1, 1, 1.0]]), currents=[1.0, 1.0], radius=1.0)
    assert link_loops_args(4, ec, 0.0, [loop])[0] == 1
    for name, (z0, loops) in {"cz == z0": (1.0, [loop]), "cz == z0 at one node": (0.0, [dict(loop, centers=np.array([[0, 0, 1.0], [1, 1, 0.0]]))]),
                              "crossing the film": (0.0, [dict(loop, centers=np.array([[0, 0, 1.0], [1, 1, -1.0]]))]),
                              "three loops": (0.0, [loop] * 3), "no loop": (0.0, []), "decreasing times": (0.0, [dict(loop, times=[1.0, 0.0])]),
                              "currents of another length": (0.0, [dict(loop, currents=[1.0, 2.0, 3.0])])}.items():
        with pytest.raises(ValueError):
            link_loops_args(4, ec, z0, loops), name
    with pytest.raises(ValueError):
        link_loops_args(5, ec, 0.0, [loop])


@pytest.fixture(scope="module")
def device():
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box

    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    dev = tdgl.Device("film", layer=layer, film=tdgl.Polygon("film", points=box(4, 2)), length_units="um")
    dev.make_mesh(max_edge_length=0.3)
    return dev


def test_solve_ensemble_refuses_a_moving_loop_by_name(device, monkeypatch):
    import tdgl_amd as tdgl
    from tdgl_amd import ensemble, hipcore

    def refuse(*a, **k):
        raise AssertionError("a GPU context was created")

    monkeypatch.setattr(hipcore.TDGLContext, "__init__", refuse)
    monkeypatch.setattr(ensemble, "build_context", refuse)
    opts = tdgl.SolverOptions(solve_time=1.0, field_units="mT", current_units="uA")
    loop = tdgl.MovingCurrentLoop([0.0, 1.0], [[-1, 0, 0.5], [1, 0, 0.5]], radius=0.5, current=100.0)
    with pytest.raises(ValueError, match=r"replica 1: .*up to 4 such products; a MovingCurrentLoop is evaluated on the device by solve\(\) alone"):
        tdgl.solve_ensemble(device, opts, applied_vector_potential=[tdgl.ConstantField(0.1), tdgl.ConstantField(0.1) + loop])
    # in the film's plane: refused when the solver's inputs are set up, with the film's height known
    flat = tdgl.MovingCurrentLoop([0.0, 1.0], [[-1, 0, 0.0], [1, 0, 0.0]], radius=0.5, current=100.0)
    with pytest.raises(ValueError, match="plane"):
        tdgl.solve_ensemble(device, opts, applied_vector_potential=tdgl.ConstantField(0.1) + flat)


# ---------------------------------------------------------------- the fixture
def test_step_rule_model_is_pinned_to_the_moving_loop_fixture():
    """The model's four values equal the reference's at every call up to np.interp's rounding; it moves exactly where a
    value changed in this call or the one before; the run holds moving steps, a joint hold and settled steps."""
    g = load_golden("traj_moving_loop_small")
    loop = fixture_loop(g)
    rule = StepRule([], [loop])
    t, seen = g["call_time"], g["call_loop_values"]
    kinds, vals = [], []
    for k in range(len(t)):
        kinds.append(rule.begin_step(float(t[k])))
        vals.append(list(rule.cur))
        assert ulp_close(loop_values(loop, float(t[k])), seen[k], 2, magnitude=np.maximum(np.abs(seen[k]), 4.0)), k
    vals = np.array(vals)
    all_vals = np.vstack([loop_values(loop, 0.0), vals])
    changed = np.any(np.diff(all_vals, axis=0) != 0, axis=1)
    before = np.concatenate([[False], changed[:-1]])
    for k, kind in enumerate(kinds):
        if kind == "move":
            assert changed[k] or before[k] or k == 0, k
        else:
            assert not changed[k], k
    assert kinds.count("move") == rule.moves >= 10 and kinds.count("settled") >= 3
    hold = [kind for kind, x in zip(kinds, t) if 2.0 < x < 2.3]
    assert hold.count("skip") >= 3
    assert not np.any(np.isin(g["loop_times"], t))


def test_oracle_with_the_model_field_reproduces_the_moving_loop_fixture():
    """The CPU oracle driven by the tests' cancellation-free loop model against the reference driven by its own loop formula,
    at the 1e-8 of the GPU tests: on this mesh the reference's formula is within 1e-10 of the exact potential (m > 1e-2)."""
    from oracle.tdgl_step import OracleSolver, run_time_loop

    g = load_golden("traj_moving_loop_small")
    mesh = reference_mesh(load_golden("mesh_small"))
    opts = options_from_golden(g)
    loop, centres = fixture_loop(g), mesh.edge_mesh.centers

    def field(t):
        return loops_field(centres, 0.0, [loop], t, g["A0"])

    solver = OracleSolver(mesh, field(0.0), 1.0, U_DEFAULT, GAMMA_DEFAULT, opts, probe_points=[int(p) for p in g["probe_points"]],
                          vector_potential_func=field)
    out = run_time_loop(solver, opts)
    tol = 1e-8
    dts = out["log"].array("dt")
    assert len(dts) == len(g["call_dt"])
    assert max_abs(dts, g["call_dt"]) <= tol * g["call_dt"].max()
    assert max_abs(np.abs(out["psi"]) ** 2, np.abs(g["final_psi"]) ** 2) < tol
    assert max_abs(out["supercurrent"], g["final_supercurrent"]) < tol
    assert max_abs(out["normal_current"], g["final_normal_current"]) < tol
    scale = max(1.0, np.abs(remove_mean(g["final_mu"])).max())
    assert max_abs(remove_mean(out["mu"]), remove_mean(g["final_mu"])) < tol * scale
    assert np.abs(g["final_supercurrent"]).max() > 1e-2
