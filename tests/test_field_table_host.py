"""The tabulated field waveform A(t) = TabulatedRamp(times, values)(t) * A_static on the host: the parameter itself, how
solve_ensemble and its dimensionless form take, broadcast and refuse it -- all decided before a GPU context exists (no GPU
needed)."""

import numpy as np
import pytest

TIMES = [1.0, 3.0, 4.5, 7.0]
VALUES = [0.0, 2.0, 2.0, -1.0]


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


def test_tabulated_ramp_is_a_piecewise_linear_factor():
    import tdgl_amd as tdgl

    f = tdgl.TabulatedRamp(TIMES, VALUES)
    assert isinstance(f, tdgl.Parameter)
    assert f.time_dependent and f.uniform_in_space and f.ramp is None
    assert isinstance(f.table, tdgl.PiecewiseLinear)
    assert np.array_equal(f.table.times, TIMES) and np.array_equal(f.table.values, VALUES)
    x = np.zeros(3)
    # at the nodes, between them, before the first (the hold rule) and after the last
    for t in TIMES + [2.0, 3.7, 5.75, 6.999, -4.0, 0.0, 0.999, 7.0001, 1e9]:
        want = float(np.interp(t, TIMES, VALUES))
        assert f.scalar(t) == want
        assert f(x, x, x, t=t) == want
        assert f.table(t) == want
    assert f.scalar(0.5) == VALUES[0] and f.scalar(100.0) == VALUES[-1]
    one = tdgl.TabulatedRamp([2.0], [0.7])  # one node: a constant
    assert one.scalar(0.0) == one.scalar(2.0) == one.scalar(5.0) == 0.7


def test_tabulated_ramp_validation():
    import tdgl_amd as tdgl

    for times, values in (([[0.0, 1.0]], [[0.0, 1.0]]), ([0.0, 1.0], [0.0, 1.0, 2.0]), ([], [])):
        with pytest.raises(ValueError, match="one-dimensional and of equal length"):
            tdgl.TabulatedRamp(times, values)
    for times in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0]):
        with pytest.raises(ValueError, match="increase strictly"):
            tdgl.TabulatedRamp(times, [0.0, 1.0, 2.0])


def test_product_with_a_static_field_is_separable():
    import tdgl_amd as tdgl

    field = tdgl.ConstantField(1.0, field_units="mT", length_units="um")
    for product in (tdgl.TabulatedRamp(TIMES, VALUES) * field, field * tdgl.TabulatedRamp(TIMES, VALUES)):
        sep = product.separable_product()
        assert sep is not None
        factor, static = sep
        assert factor.table is not None and not static.time_dependent
        x, y = np.array([0.0, 1.0, 2.0]), np.array([0.5, -0.5, 0.0])
        assert np.allclose(product(x, y, 0 * x, t=2.0), 1.0 * static(x, y, 0 * x))
        assert np.allclose(product(x, y, 0 * x, t=6.0), float(np.interp(6.0, TIMES, VALUES)) * static(x, y, 0 * x))


def test_solve_ensemble_accepts_tables_next_to_ramps_and_static_fields(device, no_gpu):
    import tdgl_amd as tdgl

    field = tdgl.ConstantField(1.0, field_units="mT", length_units="um")
    reps = _replicas(lambda: tdgl.solve_ensemble(device, _options(), applied_vector_potential=[
        tdgl.TabulatedRamp(TIMES, VALUES) * field, tdgl.LinearRamp(tmin=0, tmax=2) * field, 0.0,
        tdgl.TabulatedRamp([0.0, 0.5], [1.0, 0.25]) * field]))
    assert [r.field.kind for r in reps] == ["table", "ramp", "static", "table"]
    assert [r.device_evaluates_field() for r in reps] == [True, True, False, True]
    times, values = reps[0].field.table
    assert np.array_equal(times, TIMES) and np.array_equal(values, VALUES)
    assert len(reps[3].field.table[0]) == 2  # (tables of different lengths)
    # the links start at the table's value at t = 0
    assert np.array_equal(reps[0].current_A_applied, VALUES[0] * reps[0].field.base)
    assert np.array_equal(reps[3].current_A_applied, 1.0 * reps[3].field.base)
    assert np.abs(reps[3].field.base).max() > 0


def test_solve_ensemble_refuses_a_field_table_with_other_tables(device, no_gpu):
    import tdgl_amd as tdgl
    from tdgl_amd.parameter import PiecewiseLinear, SeparableEpsilon, TabulatedCurrents

    field = tdgl.ConstantField(1.0, field_units="mT", length_units="um")
    wave = tdgl.TabulatedRamp(TIMES, VALUES) * field
    table = TabulatedCurrents([0.0, 1.0], dict(source=[0.0, 1.0], drain=[0.0, -1.0]))
    with pytest.raises(ValueError, match="replica 1: a field table combined with TabulatedCurrents"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=wave, terminal_currents=[None, table])
    eps = SeparableEpsilon(lambda r: np.ones(len(r)), PiecewiseLinear([0.0, 1.0], [1.0, 0.5]))
    with pytest.raises(ValueError, match="replica 0: a field table combined"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=wave, disorder_epsilon=eps)

    # a callable factor that is no table stays refused, in the words the ramp's refusal uses
    def pulse(x, y, z, *, t):
        return np.ones_like(x) * (t < 1)

    factor = tdgl.Parameter(pulse, time_dependent=True)
    factor.uniform_in_space = True
    with pytest.raises(ValueError, match="not a LinearRamp"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=[wave, factor * field])


def test_dimensionless_field_tables_broadcast(device, no_gpu):
    from tdgl_amd import SolverOptions, TDGLSolver
    from tdgl_amd.ensemble import ensemble_dimensionless

    mesh = device.mesh
    m = len(mesh.edge_mesh.edges)
    base = np.ones((m, 2))
    opts = SolverOptions(solve_time=1.0)
    wave = (base, TIMES, VALUES)
    # one table for every replica; link exponents from the table at t = 0
    ens = ensemble_dimensionless(mesh, opts, [None, None], vector_potential_table=(base, [0.0, 2.0], [0.5, 1.0]))
    assert len(ens.reps) == 2
    assert all(r.field.kind == "table" and np.array_equal(r.current_A_applied, 0.5 * base) for r in ens.reps)
    assert np.array_equal(ens.reps[0].vector_potential_func(1.0), 0.75 * base)
    # a list with None: static, ramped and tabulated replicas in one ensemble, tables of different lengths
    ramp = dict(tmin=0.0, tmax=2.0, initial=0.5, final=1.0)
    ens = ensemble_dimensionless(mesh, opts, [None, np.zeros((m, 2)), None, None],
                                 vector_potential_ramp=[None, None, (base, ramp), None],
                                 vector_potential_table=[wave, None, None, (2.0 * base, [0.5], [3.0])])
    assert [r.field.kind for r in ens.reps] == ["table", "static", "ramp", "table"]
    assert np.array_equal(ens.reps[3].current_A_applied, 6.0 * base)
    # lists of different lengths
    with pytest.raises(ValueError, match="different lengths"):
        ensemble_dimensionless(mesh, opts, [np.zeros((m, 2))] * 2, vector_potential_table=[wave] * 3)
    with pytest.raises(ValueError, match="different lengths"):
        ensemble_dimensionless(mesh, opts, None, vector_potential_ramp=[(base, ramp)] * 2, vector_potential_table=[wave] * 3)
    # a ramp and a table for one replica
    with pytest.raises(ValueError, match="exclude each other"):
        ensemble_dimensionless(mesh, opts, None, vector_potential_ramp=(base, ramp), vector_potential_table=wave)
    with pytest.raises(ValueError, match="exclude each other"):
        ensemble_dimensionless(mesh, opts, [None, None], vector_potential_ramp=[None, (base, ramp)],
                               vector_potential_table=[wave, wave])
    with pytest.raises(ValueError, match="exclude each other"):
        TDGLSolver.from_dimensionless(mesh, opts, 0.5 * base, vector_potential_ramp=(base, ramp), vector_potential_table=wave)
    # a field table and an epsilon table in one replica
    with pytest.raises(ValueError, match="a field table combined"):
        ensemble_dimensionless(mesh, opts, None, vector_potential_table=wave,
                               epsilon_table=(np.full(len(mesh.sites), 0.9), [0.0], [1.0]))
