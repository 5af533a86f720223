"""`tdgl_amd.applied_field`: each kind of applied vector potential issues exactly the library calls its row of the
table in DESIGN.md ("The applied field in Python") names, seen through recording stubs in place of the operators, the context
and the ensemble.  No GPU, no mesh: six edge centres."""

from types import SimpleNamespace

import numpy as np
import pytest

import tdgl_amd as tdgl
from tdgl_amd import applied_field as af
from tdgl_amd.parameter import LinearRamp, PiecewiseLinear, _loop_potential

M = 6
_rng = np.random.default_rng(20)
CENTRES = _rng.uniform(-2.0, 2.0, (M, 2))
EX, EY, Z0 = CENTRES[:, 0], CENTRES[:, 1], 0.1 * np.ones(M)
BASE, A0, A1, A2, GIVEN = _rng.normal(size=(5, M, 2))
A_SCALE = 0.37
RAMP = dict(tmin=-1.0, tmax=3.0, initial=0.25, final=1.5)  # (0.5625 at t = 0)
TIMES, VALUES = np.array([-1.0, 1.0, 3.0]), np.array([0.2, 0.8, 0.4])  # (0.5 at t = 0)
TERMS = [(A1, RAMP), (A2, (TIMES, VALUES))]
LOOP = dict(times=np.array([-0.5, 2.0]), centers=np.array([[-1.0, 0.2, 0.6], [1.0, -0.3, 0.9]]), currents=np.array([0.5, 2.0]),
            radius=0.7)
KINDS = ["static", "callable", "scaled", "ramp", "table", "terms", "loops"]


class Recorder:
    """Stands for the operators, their context, an ensemble or a state source: records ``(name, args, kwargs)`` of every
    call and answers with ``returns[name]``."""

    def __init__(self, **returns):
        self.calls, self.returns, self.ctx = [], returns, self

    def __getattr__(self, name):
        def call(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            return self.returns.get(name)

        return call


def _equal(a, b) -> bool:
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        return isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b) and all(map(_equal, a, b))
    if a is None or b is None:
        return a is b
    return np.array_equal(a, b)


def _assert_calls(rec, want):
    assert [c[0] for c in rec.calls] == [w[0] for w in want]
    for (name, args, kwargs), w in zip(rec.calls, want):
        assert _equal(args, w[1]) and _equal(kwargs, w[2] if len(w) > 2 else {}), name


def _on_edges(q, **kw):
    return A_SCALE * np.asarray(q(EX, EY, Z0, **kw))[:, :2]


def _pulse(x, y, z, *, t):
    return np.ones_like(x) * (1.0 + t) * (t < 1)


def _swirl(x, y, z, *, t):
    return np.stack([(1.0 + t) * y, -x, 0 * x], axis=1)


def _parameters():
    """Per kind: ``(applied_vector_potential, what its field must hold)``, the expected arrays worked out here."""
    F = tdgl.ConstantField(1.0, field_units="mT", length_units="um")
    B = tdgl.ConstantField(0.4, field_units="mT", length_units="um")
    ramp, wave = tdgl.LinearRamp(**RAMP), tdgl.TabulatedRamp(TIMES, VALUES)
    pulse = tdgl.Parameter(_pulse, time_dependent=True)
    pulse.uniform_in_space = True
    loop = tdgl.MovingCurrentLoop(LOOP["times"], LOOP["centers"], radius=LOOP["radius"], current=LOOP["currents"])
    unit = loop.loop["unit_factor"]
    loops = [dict(LOOP, currents=A_SCALE * unit * LOOP["currents"])]
    xs, ys = EX - (EX.min() + np.ptp(EX) / 2), EY - (EY.min() + np.ptp(EY) / 2)
    return {
        "static": (0.3, dict(A=A_SCALE * np.stack([-0.3 * ys / 2, 0.3 * xs / 2], axis=1))),
        "callable": (tdgl.Parameter(_swirl, time_dependent=True), dict(A=_on_edges(_swirl, t=0))),
        "scaled": (pulse * F, dict(base=_on_edges(F), f0=1.0)),
        "ramp": (ramp * F, dict(base=_on_edges(F), f0=0.5625)),
        "table": (wave * F, dict(base=_on_edges(F), f0=0.5)),
        "terms": (B + wave * F, dict(A0=_on_edges(B), terms=[(_on_edges(F), (TIMES, VALUES))])),
        "loops": (B + loop, dict(A0=_on_edges(B), loops=loops)),
        "loops over terms": (ramp * F + loop, dict(A0=None, terms=[(_on_edges(F), RAMP)], loops=loops)),
    }


def _dimensionless():
    """The same kinds from `TDGLSolver.from_dimensionless`'s keyword arguments."""
    loop2 = dict(LOOP, centers=LOOP["centers"][:, :2], z=0.6, currents=1.5)  # (centres [n, 2] with one z, one current)
    full2 = dict(LOOP, centers=np.column_stack([LOOP["centers"][:, :2], [0.6, 0.6]]), currents=np.array([1.5, 1.5]))
    scale = lambda t: 1.0 + t  # noqa: E731
    return {
        "static": (dict(link_exponents=GIVEN), dict(A=GIVEN)),
        "callable": (dict(link_exponents=GIVEN, vector_potential_func=lambda t: scale(t) * BASE), dict(A=GIVEN)),
        "ramp": (dict(link_exponents=GIVEN, ramp=(BASE, RAMP)), dict(base=BASE, f0=0.5625)),
        "table": (dict(link_exponents=GIVEN, table=(BASE, TIMES, VALUES)), dict(base=BASE, f0=0.5)),
        "terms": (dict(link_exponents=GIVEN, terms=(A0, TERMS)), dict(A0=A0, terms=TERMS)),
        "loops": (dict(link_exponents=GIVEN, loops=[loop2]), dict(A0=GIVEN, loops=[full2])),
        "loops over terms": (dict(terms=(None, TERMS), loops=[LOOP]), dict(A0=None, terms=TERMS, loops=[LOOP])),
    }


def _fields():
    """``(constructor, kind, field, what it must hold, the film's z)`` for every kind either constructor expresses."""
    out = []
    for name, (applied, want) in _parameters().items():
        out.append(("parameter", name, af.from_parameter(applied, CENTRES, Z0, A_SCALE, 0.1), want, 0.1))
    for name, (kw, want) in _dimensionless().items():
        out.append(("dimensionless", name, af.from_dimensionless(CENTRES, **kw), want, 0.0))
    out.append(("direct", "scaled", af.ScaledField(BASE, lambda t: 2.0 - t), dict(base=BASE, f0=2.0), 0.0))
    return out


def _install_row(name, want, z_film):
    """The row of the table: the calls ``install`` issues on a single solver."""
    if name in ("static", "callable"):
        return [("set_link_exponents", (want["A"],))]
    if name in ("scaled", "ramp", "table"):
        more = {"scaled": [], "ramp": [("set_link_ramp", (), RAMP)], "table": [("set_link_table", (TIMES, VALUES))]}[name]
        return [("set_link_exponents_base", (want["base"], want["f0"]))] + more
    under = [("set_link_terms", (want["A0"], want["terms"]))] if "terms" in want else [("set_link_exponents", (want["A0"],))]
    if name == "terms":
        return under
    return under + [("set_link_loops", (CENTRES, z_film, want["loops"])), ("link_exponents", ())]


def test_install_issues_the_calls_of_its_row():
    seen = set()
    for how, name, field, want, z_film in _fields():
        assert field.kind == name.split()[0] and field.on_device == (field.kind in ("ramp", "table", "terms", "loops"))
        assert field.time_dependent == (field.kind != "static")
        applied_by_device = np.full((M, 2), 7.0)
        rec = Recorder(link_exponents=applied_by_device)
        got = field.install(rec)
        _assert_calls(rec, _install_row(name, want, z_film))
        assert got is (applied_by_device if field.kind == "loops" else None), (how, name)
        seen.add((how, field.kind))
    assert seen >= {("parameter", k) for k in KINDS} | {("dimensionless", k) for k in KINDS if k != "scaled"}


def test_install_replica_issues_the_calls_of_its_row():
    for how, name, field, want, _ in _fields():
        if field.kind in ("scaled", "loops"):
            continue  # (refused before this point: test_the_ensemble_refuses_three_kinds_in_its_own_words)
        ens = Recorder()
        field.install_replica(ens, 2, GIVEN)
        _assert_calls(ens, {"static": [("set_link_exponents", (2, GIVEN))], "callable": [("set_link_exponents", (2, GIVEN))],
                            "ramp": [("set_link_ramp", (2, want.get("base")), RAMP)],
                            "table": [("set_link_table", (2, want.get("base"), TIMES, VALUES))],
                            "terms": [("set_link_terms", (2, want.get("A0"), want.get("terms")))]}[name])


def test_the_ensemble_refuses_three_kinds_in_its_own_words():
    from tdgl_amd.ensemble import _refuse_dynamic

    head = ("solve_ensemble: replica 3: a time-dependent applied_vector_potential is supported only as LinearRamp(...) * "
            "(static field), TabulatedRamp(...) * (static field), or a sum (static field) + f_1 * (static field) + ... of up to "
            "4 such products; ")
    tails = {"scaled": "this one's time factor is not a LinearRamp or a TabulatedRamp.",
             "loops": "a MovingCurrentLoop is evaluated on the device by solve() alone, not per replica.",
             "callable": "this one is not of that form."}
    nouns = {"ramp": "a field ramp", "table": "a field table", "terms": "a sum of field terms"}
    for how, name, field, _, _ in _fields():
        rep = SimpleNamespace(field=field, dynamic_vector_potential=field.time_dependent, dynamic_currents=False,
                              dynamic_epsilon=False, _current_table=None, _eps_table=None,
                              device_evaluates_field=lambda f=field: f.on_device)
        if field.kind in tails:
            with pytest.raises(ValueError) as info:
                _refuse_dynamic(3, rep)
            assert str(info.value) == head + tails[field.kind]
            continue
        _refuse_dynamic(3, rep)  # accepted
        if field.kind in nouns:  # ... but not next to the other tables
            rep._eps_table = object()
            with pytest.raises(ValueError) as info:
                _refuse_dynamic(3, rep)
            assert str(info.value) == (f"solve_ensemble: replica 3: {nouns[field.kind]} combined with TabulatedCurrents or a "
                                       "SeparableEpsilon in one replica is not supported.")


def test_applied_reads_back_what_the_last_step_applied():
    on_device = np.full((M, 2), 7.0)
    for how, name, field, want, _ in _fields():
        source = Recorder(link_exponents=on_device, link_term_scales=np.array([0.3, 0.7]), link_scale=0.4)
        got = field.applied(source)
        if field.kind == "loops":
            assert got is on_device and [c[0] for c in source.calls] == ["link_exponents"]
        elif field.kind == "terms":
            bases = [b for b, _ in want["terms"]] + [None]
            model = 0.3 * bases[0] if want["A0"] is None else want["A0"] + 0.3 * bases[0]
            assert np.array_equal(got, model if len(want["terms"]) == 1 else model + 0.7 * bases[1])
            assert np.array_equal(got, field.terms_value(np.array([0.3, 0.7])[:len(want["terms"])]))
        elif field.kind in ("scaled", "ramp", "table"):
            assert np.array_equal(got, 0.4 * want["base"]) and [c[0] for c in source.calls] == ["link_scale"]
        else:
            assert got is None and not source.calls


def _loops_at(t, A):
    for lp in [LOOP]:
        c = [float(np.interp(t, lp["times"], lp["centers"][:, j])) for j in range(3)]
        A = A + _loop_potential(EX, EY, 0.0, c, lp["radius"], float(np.interp(t, lp["times"], lp["currents"])))[:, :2]
    return A


def test_without_link_exponents_the_solver_starts_at_the_value_at_zero():
    want = {
        "ramp": (dict(ramp=(BASE, RAMP)), LinearRamp(**RAMP).scalar(0.0) * BASE),
        "table": (dict(table=(BASE, TIMES, VALUES)), PiecewiseLinear(TIMES, VALUES)(0.0) * BASE),
        "terms": (dict(terms=(A0, TERMS)), (A0 + 0.5625 * A1) + 0.5 * A2),
        "loops": (dict(loops=[LOOP]), _loops_at(0.0, np.zeros((M, 2)))),
        "loops over terms": (dict(terms=(A0, TERMS), loops=[LOOP]), _loops_at(0.0, (A0 + 0.5625 * A1) + 0.5 * A2)),
    }
    for name, (kw, initial) in want.items():
        field = af.from_dimensionless(CENTRES, None, **kw)
        assert field.kind == name.split()[0] and np.array_equal(field.initial, initial), name
        assert np.array_equal(field.value(0.0), initial) and np.abs(initial).max() > 0
        given = af.from_dimensionless(CENTRES, GIVEN, **kw)  # (link_exponents given: the solver starts there)
        assert given.initial is GIVEN or np.array_equal(given.initial, GIVEN)
    assert np.array_equal(af.from_dimensionless(CENTRES, GIVEN, loops=[LOOP]).value(1.0), _loops_at(1.0, GIVEN))


def test_the_dimensionless_arguments_exclude_each_other_in_the_same_words():
    ramp, table, terms = (BASE, RAMP), (BASE, TIMES, VALUES), (A0, TERMS)
    for kw, text in ((dict(ramp=ramp, table=table), "vector_potential_ramp and vector_potential_table exclude each other."),
                     (dict(terms=terms, ramp=ramp), "vector_potential_terms excludes vector_potential_ramp and vector_potential_table."),
                     (dict(terms=terms, table=table), "vector_potential_terms excludes vector_potential_ramp and vector_potential_table."),
                     (dict(loops=[LOOP], ramp=ramp), "vector_potential_loops excludes vector_potential_ramp and vector_potential_table."),
                     (dict(terms=(A0, []), ), "vector_potential_terms: between 1 and 4 terms, got 0.")):
        with pytest.raises(ValueError) as info:
            af.from_dimensionless(CENTRES, GIVEN, **kw)
        assert str(info.value) == text
    with pytest.raises(ValueError, match="the loop's plane must differ from the film's"):  # (link_loops_args, at construction)
        af.from_dimensionless(CENTRES, GIVEN, loops=[dict(LOOP, centers=LOOP["centers"] * [1, 1, 0])])


def test_advance_is_the_host_path_of_the_two_host_kinds():
    for how, name, field, want, _ in _fields():
        ctx = Recorder()
        got = field.advance(ctx, 0.75, 0.01)
        if field.kind == "scaled":
            _assert_calls(ctx, [("update_link_scale", (field.factor(0.75), 0.01))])
            assert got is None and field.factor(0.75) == (1.75 if how == "parameter" else 1.25)
        elif field.kind == "callable":
            model = _on_edges(_swirl, t=0.75) if how == "parameter" else 1.75 * BASE
            _assert_calls(ctx, [("update_link_exponents", (model, 0.01))])
            assert np.array_equal(got, model) and np.array_equal(field.value(0.75), model) and got.dtype == float
        else:
            assert got is None and not ctx.calls, (how, name)


def test_recognition_order_from_a_parameter():
    kinds = {name: af.from_parameter(applied, CENTRES, Z0, A_SCALE, 0.1) for name, (applied, _) in _parameters().items()}
    assert {name: f.kind for name, f in kinds.items()} == {
        "static": "static", "callable": "callable", "scaled": "scaled", "ramp": "ramp", "table": "table", "terms": "terms",
        "loops": "loops", "loops over terms": "loops"}
    assert kinds["loops"].under.kind == "static" and kinds["loops over terms"].under.kind == "terms"
    assert kinds["ramp"].ramp == RAMP and _equal(kinds["table"].table, (TIMES, VALUES))
    static = af.from_parameter(tdgl.ConstantField(0.4, field_units="mT", length_units="um"), CENTRES, Z0, A_SCALE, 0.1)
    assert static.kind == "static" and not static.time_dependent and static.value(3.0) is static.initial
