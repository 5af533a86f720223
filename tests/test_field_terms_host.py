"""Sums of a static and time-scaled field terms A(t) = A_0 + f_1(t) A_1 + ... + f_K(t) A_K on the host (no GPU needed): the
CPU oracle reproduces the reference fixture, `separable_terms()` recognises the sums it should and nothing else,
solve_ensemble takes, broadcasts and refuses terms before a GPU context exists, and a NumPy model of the step rule is
pinned to what the reference did call by call."""

import numpy as np
import pytest

from conftest import load_golden
from field_terms_model import StepRule, factor_value, fixture_terms, terms_sum, ulp_close
from helpers import GAMMA_DEFAULT, U_DEFAULT, align_phase, max_abs, options_from_golden, reference_mesh, remove_mean

TIMES = [1.0, 3.0, 4.5, 7.0]
VALUES = [0.0, 2.0, 2.0, -1.0]


# ---------------------------------------------------------------- the fixture
def test_oracle_reproduces_the_field_terms_fixture():
    """traj_field_terms_small at the tolerance tests/test_oracle_golden.py uses for traj_dynamic_small (1e-12), with that
    file's `_assert_trajectory` checks."""
    from oracle.tdgl_step import OracleSolver, run_time_loop

    g = load_golden("traj_field_terms_small")
    mesh = reference_mesh(load_golden("mesh_small"))
    opts = options_from_golden(g)
    A0, A1, A2 = g["A0"], g["A1"], g["A2"]
    ramp = fixture_terms(g)[1][0][1]

    def field(t):
        return A0 + factor_value(ramp, t) * A1 + float(np.interp(t, g["table_times"], g["table_values"])) * A2

    solver = OracleSolver(mesh, field(0.0), 1.0, U_DEFAULT, GAMMA_DEFAULT, opts, probe_points=[int(p) for p in g["probe_points"]],
                          vector_potential_func=field)
    out = run_time_loop(solver, opts)
    tol = 1e-12
    log = out["log"]
    dts = log.array("dt")
    assert len(dts) == len(g["call_dt"]) == out["book"]["calls"]
    assert max_abs(dts, g["call_dt"]) <= tol * g["call_dt"].max()
    assert max_abs(np.abs(out["psi"]) ** 2, np.abs(g["final_psi"]) ** 2) < tol
    assert max_abs(out["supercurrent"], g["final_supercurrent"]) < tol
    assert max_abs(out["normal_current"], g["final_normal_current"]) < tol
    scale = max(1.0, np.abs(remove_mean(g["final_mu"])).max())
    assert max_abs(remove_mean(out["mu"]), remove_mean(g["final_mu"])) < tol * scale
    assert max_abs(align_phase(out["psi"], g["final_psi"]), g["final_psi"]) < tol
    mu_p, th_p = log.array("mu"), log.array("theta")
    assert max_abs(mu_p[:, 0] - mu_p[:, 1], g["call_mu_probe"][:, 0] - g["call_mu_probe"][:, 1]) < tol * scale
    assert max_abs(np.exp(1j * (th_p[:, 0] - th_p[:, 1])), np.exp(1j * (g["call_theta_probe"][:, 0] - g["call_theta_probe"][:, 1]))) < tol
    # the field did act: both terms left their mark on the final state
    assert np.abs(g["final_supercurrent"]).max() > 1e-2


def test_step_rule_model_is_pinned_to_the_fixture():
    """The model's factors equal the reference's at every call (it re-evaluates A before every step; the model skips and
    settles only where nothing changes), it moves exactly where a factor changed in this call or the one before, and the
    fixture holds every kind of step: only term 1, only term 2, both, a joint hold, settled steps."""
    g = load_golden("traj_field_terms_small")
    specs = [spec for _, spec in fixture_terms(g)[1]]
    rule = StepRule(specs)
    t, f = g["call_time"], np.column_stack([g["call_f1"], g["call_f2"]])
    kinds, seen = [], []
    for time in t:
        kinds.append(rule.begin_step(float(time)))
        seen.append(list(rule.scale))
    seen = np.array(seen)
    # (the reference's table is np.interp, whose operations are ordered differently: a few roundings at the size of the
    # nodes' values, which is the size of the terms the difference near the zero crossing is formed from)
    assert np.array_equal(seen[:, 0], f[:, 0]) and ulp_close(seen[:, 1], f[:, 1], 2, magnitude=np.abs(g["table_values"]).max())
    start = np.array([[factor_value(s, 0.0) for s in specs]])
    changed = np.any(np.diff(np.concatenate([start, seen]), axis=0) != 0, axis=1)
    after = np.concatenate([[True], changed[:-1]])  # (the first step always moves: no dynamic update has run)
    settled = np.array([k == "settled" for k in kinds])
    assert np.array_equal(np.array([k == "move" for k in kinds]), (changed | after) & ~settled)
    m = np.diff(np.concatenate([start, seen]), axis=0) != 0
    assert np.any(m[:, 0] & ~m[:, 1]) and np.any(~m[:, 0] & m[:, 1]) and np.any(m[:, 0] & m[:, 1])
    tmax, t_hold_end, t_end = float(g["ramp_tmax"]), float(g["table_times"][2]), float(g["table_times"][-1])
    hold = [k for k, time in zip(kinds, t) if tmax < time < t_hold_end]
    assert hold.count("skip") >= 3 and "settled" not in hold
    # settled: from the third call at or behind the last node on (two evaluations at the end values first), to the end
    first = int(np.argmax(settled))
    assert settled[first:].all() and not settled[:first].any() and settled.sum() >= 3
    assert t[first] >= t_end and np.sum(t[:first] >= t_end) == 2
    assert rule.moves == kinds.count("move") < len(kinds) - 6
    # the left-to-right sum is the reference's field at every call up to the rounding of its own order of operations
    A0, (A1, _), (A2, _) = g["A0"], *fixture_terms(g)[1]
    for k in (0, len(t) // 2, len(t) - 1):
        want = A0 + f[k, 0] * A1 + f[k, 1] * A2
        assert ulp_close(terms_sum(A0, [A1, A2], seen[k]), want, 4, magnitude=np.abs(A0) + np.abs(A1) + np.abs(A2))


# ---------------------------------------------------------------- the parameter algebra
def _fields():
    import tdgl_amd as tdgl

    return (tdgl.ConstantField(1.0), tdgl.ConstantField(0.3), tdgl.ConstantField(-2.0), tdgl.LinearRamp(tmin=0.5, tmax=2.0, initial=0.2, final=1.5),
            tdgl.TabulatedRamp(TIMES, VALUES))


def _left_to_right(terms, x, y, z, t):
    static, products = terms
    A0 = None if static is None else np.asarray(static(x, y, z))
    return terms_sum(A0, [np.asarray(q(x, y, z)) for _, q in products], [f.scalar(t) for f, _ in products])


def test_separable_terms_recognises_sums_differences_and_orderings():
    import tdgl_amd as tdgl

    B, F, G, ramp, wave = _fields()
    x, y = np.array([0.0, 1.0, 2.5, -3.0]), np.array([0.5, -0.5, 0.0, 2.0])
    z = np.zeros(4)
    mag = 2.0 * sum(np.abs(np.asarray(q(x, y, z))) for q in (B, F, G))
    cases = {
        "static + product": (B + ramp * F, 1, True),
        "product + static": (ramp * F + B, 1, True),
        "static field on the left of the factor": (B + F * ramp, 1, True),
        "two products, no static part": (ramp * F + wave * G, 2, False),
        "static - product": (B - wave * G, 1, True),
        "product - static": (wave * G - B, 1, True),
        "statics fold": (B + ramp * F + G, 1, True),
        "a difference in brackets": (B - (ramp * F - G), 1, True),
        "three leaves and a scaled static": (2.0 * B + ramp * F - wave * G, 2, True),
        "a single product": (ramp * F, 1, False),
    }
    for name, (p, K, has_static) in cases.items():
        terms = p.separable_terms()
        assert terms is not None, name
        static, products = terms
        assert len(products) == K and (static is not None) == has_static, name
        assert all((f.ramp is not None) != (f.table is not None) and not q.time_dependent for f, q in products), name
        assert static is None or not static.time_dependent, name
        # (no addend of any case exceeds 2 |leaf|: the factors stay within [-1, 2] and one case scales B by 2; a reordered
        # sum of at most five addends differs by at most four roundings of at most one spacing of their total)
        for t in (0.0, 1.7, 3.3, 9.0):
            assert ulp_close(_left_to_right(terms, x, y, z, t), np.asarray(p(x, y, z, t=t)), 4, magnitude=mag), (name, t)
    # the order of the products is the order they appear in; a subtracted leaf enters negated, exactly
    static, products = (B - wave * G + ramp * F).separable_terms()
    assert [f.table is not None for f, _ in products] == [True, False]
    assert np.array_equal(np.asarray(products[0][1](x, y, z)), -np.asarray(G(x, y, z)))
    static, products = (ramp * F - B - G).separable_terms()
    assert np.array_equal(np.asarray(static(x, y, z)), -np.asarray(B(x, y, z)) + -np.asarray(G(x, y, z)))
    # a parameter without time dependence is the sum without products
    assert B.separable_terms() == (B, [])
    assert tdgl.Parameter.separable_terms(ramp) is None


def test_separable_terms_refuses_everything_else():
    import tdgl_amd as tdgl
    from tdgl_amd.parameter import FIELD_TERMS_MAX

    B, F, G, ramp, wave = _fields()

    def anything(x, y, z, *, t):
        return np.sin(t) * np.ones_like(x)

    assert FIELD_TERMS_MAX == 4
    refused = {
        "a product of two factors": B + ramp * wave * F,
        "a product of two factors, bracketed": B + ramp * (wave * F),
        "**": B + (ramp * F) ** 2,
        "a power of a factor": B + ramp ** 2 * F,
        "a Scale with a function of its own": B + tdgl.Scale(anything) * F,
        "a quotient": B + F / ramp,
        "a bare number": B + ramp * F + 1.0,
        "a time-dependent field that is no product": tdgl.Parameter(lambda x, y, z, *, t: np.stack([x * t, y, z], axis=1), time_dependent=True) + B,
        "K = 5": B + ramp * F + wave * G + ramp * G + wave * F + ramp * B,
    }
    for name, p in refused.items():
        assert p.time_dependent and p.separable_terms() is None, name
    four = B + ramp * F + wave * G + ramp * G + wave * F
    assert len(four.separable_terms()[1]) == 4


# ---------------------------------------------------------------- solve_ensemble before a context exists
@pytest.fixture(scope="module")
def device():
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box

    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    film = tdgl.Polygon("film", points=box(4, 2))
    source = tdgl.Polygon("source", points=box(0.02, 2, center=(-2, 0)))
    drain = tdgl.Polygon("drain", points=box(0.02, 2, center=(2, 0)))
    dev = tdgl.Device("strip", layer=layer, film=film, terminals=[source, drain], probe_points=[(-1, 0), (1, 0)],
                      length_units="um")
    dev.make_mesh(max_edge_length=0.3)
    return dev


class _Reached(Exception):
    pass


@pytest.fixture
def no_gpu(monkeypatch):
    """Creating a device context fails the test; reaching the ensemble's solver raises _Reached (the inputs passed)."""
    from tdgl_amd import ensemble, hipcore

    def refuse(*a, **k):
        raise AssertionError("a GPU context was created")

    def reached(self):
        raise _Reached(self.reps)

    monkeypatch.setattr(hipcore.TDGLContext, "__init__", refuse)
    monkeypatch.setattr(ensemble, "build_context", refuse)
    monkeypatch.setattr(ensemble.EnsembleSolver, "solve", reached)


def _options(**kw):
    import tdgl_amd as tdgl

    base = dict(solve_time=1.0, field_units="mT", current_units="uA")
    base.update(kw)
    return tdgl.SolverOptions(**base)


def _replicas(call):
    with pytest.raises(_Reached) as info:
        call()
    return info.value.args[0]


def test_solve_ensemble_accepts_sums_next_to_single_products_and_static_fields(device, no_gpu):
    import tdgl_amd as tdgl

    B, F, G, ramp, wave = _fields()
    reps = _replicas(lambda: tdgl.solve_ensemble(device, _options(), applied_vector_potential=[
        B + wave * G, wave * F, 0.0, ramp * F - G + wave * B]))
    assert [r.field.kind for r in reps] == ["terms", "table", "static", "terms"]
    assert [r.device_evaluates_field() for r in reps] == [True, True, False, True]
    A0, terms = reps[0].field.A0, reps[0].field.terms
    assert A0 is not None and len(terms) == 1 and np.array_equal(terms[0][1][0], TIMES) and np.array_equal(terms[0][1][1], VALUES)
    A0, terms = reps[3].field.A0, reps[3].field.terms
    assert len(terms) == 2 and isinstance(terms[0][1], dict) and terms[0][1]["final"] == 1.5
    # every base carries the device's field scale, and the links start at the sum's value at t = 0
    ex, ey = reps[3].edge_centers[:, 0], reps[3].edge_centers[:, 1]
    assert np.array_equal(A0, reps[3].A_scale * -np.asarray(G(ex, ey, reps[3].z0))[:, :2])
    assert np.array_equal(terms[0][0], reps[3].A_scale * np.asarray(F(ex, ey, reps[3].z0))[:, :2])
    assert np.array_equal(reps[3].current_A_applied, (A0 + 0.2 * terms[0][0]) + VALUES[0] * terms[1][0])
    assert np.array_equal(reps[3].vector_potential_func(2.0), (A0 + 1.5 * terms[0][0]) + 1.0 * terms[1][0])


def test_solve_ensemble_refuses_what_is_no_sum_of_terms(device, no_gpu):
    import tdgl_amd as tdgl
    from tdgl_amd.parameter import PiecewiseLinear, SeparableEpsilon, TabulatedCurrents

    B, F, G, ramp, wave = _fields()

    def anything(x, y, z, *, t):
        return np.sin(t) * np.ones_like(x)

    # the refusal names the new form
    with pytest.raises(ValueError, match=r"replica 1: .*or a sum \(static field\) \+ f_1 \* \(static field\) \+ \.\.\. of up to 4 such products"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=[B + wave * G, B + tdgl.Scale(anything) * F])
    with pytest.raises(ValueError, match="replica 0: .*up to 4 such products"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=B + ramp * F + wave * G + ramp * G + wave * F + ramp * B)
    table = TabulatedCurrents([0.0, 1.0], dict(source=[0.0, 1.0], drain=[0.0, -1.0]))
    with pytest.raises(ValueError, match="replica 1: a sum of field terms combined with TabulatedCurrents"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=B + wave * G, terminal_currents=[None, table])
    eps = SeparableEpsilon(lambda r: np.ones(len(r)), PiecewiseLinear([0.0, 1.0], [1.0, 0.5]))
    with pytest.raises(ValueError, match="replica 0: a sum of field terms combined"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=B + wave * G, disorder_epsilon=eps)


def test_dimensionless_field_terms_broadcast(device, no_gpu):
    from tdgl_amd import SolverOptions, TDGLSolver
    from tdgl_amd.ensemble import ensemble_dimensionless

    mesh = device.mesh
    m = len(mesh.edge_mesh.edges)
    base = np.ones((m, 2))
    opts = SolverOptions(solve_time=1.0)
    ramp = dict(tmin=0.0, tmax=2.0, initial=0.5, final=1.0)
    terms = (0.25 * base, [(base, ramp), (2.0 * base, (TIMES, VALUES))])
    # one sum for every replica; link exponents from the sum at t = 0
    ens = ensemble_dimensionless(mesh, opts, [None, None], vector_potential_terms=terms)
    assert len(ens.reps) == 2
    assert [r.field.kind for r in ens.reps] == ["terms", "terms"]
    assert all(np.array_equal(r.current_A_applied, 0.75 * base) and r.dynamic_vector_potential for r in ens.reps)
    assert np.array_equal(ens.reps[0].vector_potential_func(2.0), (0.25 * base + 1.0 * base) + 1.0 * (2.0 * base))
    # a list with None: static, ramped, tabulated and summed replicas in one ensemble
    ens = ensemble_dimensionless(mesh, opts, [None, np.zeros((m, 2)), None, None],
                                 vector_potential_ramp=[None, None, (base, ramp), None],
                                 vector_potential_table=[(base, TIMES, VALUES), None, None, None],
                                 vector_potential_terms=[None, None, None, (None, [(base, (TIMES, VALUES))])])
    assert [r.field.kind for r in ens.reps] == ["table", "static", "ramp", "terms"]
    assert [r.device_evaluates_field() for r in ens.reps] == [True, False, True, True]
    assert ens.reps[3].field.A0 is None and np.array_equal(ens.reps[3].current_A_applied, 0.0 * base)
    with pytest.raises(ValueError, match="different lengths"):
        ensemble_dimensionless(mesh, opts, [np.zeros((m, 2))] * 2, vector_potential_terms=[terms] * 3)
    # terms exclude the ramp and the table of the same replica
    with pytest.raises(ValueError, match="vector_potential_terms excludes"):
        ensemble_dimensionless(mesh, opts, None, vector_potential_ramp=(base, ramp), vector_potential_terms=terms)
    with pytest.raises(ValueError, match="vector_potential_terms excludes"):
        ensemble_dimensionless(mesh, opts, [np.zeros((m, 2)), None], vector_potential_table=[None, (base, TIMES, VALUES)],
                               vector_potential_terms=[None, terms])
    with pytest.raises(ValueError, match="vector_potential_terms excludes"):
        TDGLSolver.from_dimensionless(mesh, opts, 0.75 * base, vector_potential_table=(base, TIMES, VALUES), vector_potential_terms=terms)
    # K = 0 and K = 5
    for bad in ((None, []), (None, [(base, ramp)] * 5)):
        with pytest.raises(ValueError, match="between 1 and 4 terms"):
            ensemble_dimensionless(mesh, opts, None, vector_potential_terms=bad)
    with pytest.raises(ValueError, match="a sum of field terms combined"):
        ensemble_dimensionless(mesh, opts, None, vector_potential_terms=terms, epsilon_table=(np.full(len(mesh.sites), 0.9), [0.0], [1.0]))
