"""solve_ensemble's handling of time-dependent replicas on the host: which drives pass (the three forms the device
evaluates itself), which are refused, and the per-replica broadcasting of the dimensionless ramp and epsilon tables,
all decided before a GPU context exists (no GPU needed)."""

import numpy as np
import pytest


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


def test_device_evaluable_drives_are_accepted(device, no_gpu):
    import tdgl_amd as tdgl
    from tdgl_amd.parameter import PiecewiseLinear, SeparableEpsilon, TabulatedCurrents

    field = tdgl.ConstantField(1.0, field_units="mT", length_units="um")
    reps = _replicas(lambda: tdgl.solve_ensemble(device, _options(), applied_vector_potential=[
        tdgl.LinearRamp(tmin=0, tmax=2) * field, 0.5, tdgl.LinearRamp(tmin=1, tmax=3, initial=0.2, final=0.7) * field]))
    assert [r.field.kind for r in reps] == ["ramp", "static", "ramp"]
    assert reps[2].field.ramp == dict(tmin=1, tmax=3, initial=0.2, final=0.7)
    table = TabulatedCurrents([0.0, 1.0], dict(source=[0.0, 1.0], drain=[0.0, -1.0]))
    reps = _replicas(lambda: tdgl.solve_ensemble(device, _options(), terminal_currents=[table, dict(source=1, drain=-1)]))
    assert reps[0]._current_table is not None and reps[1]._current_table is None
    times, groups, dens = reps[0]._current_table_arrays()
    assert dens.shape == (2, 2) and len(groups) == 2
    eps = SeparableEpsilon(lambda r: np.ones(len(r)), PiecewiseLinear([0.0, 1.0], [1.0, 0.5]))
    reps = _replicas(lambda: tdgl.solve_ensemble(device, _options(), disorder_epsilon=[eps, 1.0]))
    assert reps[0]._eps_table is not None and reps[0].dynamic_epsilon and not reps[1].dynamic_epsilon
    # tabulated currents and a separable epsilon in one replica
    _replicas(lambda: tdgl.solve_ensemble(device, _options(), terminal_currents=table, disorder_epsilon=eps))


def test_other_time_dependence_is_refused(device, no_gpu):
    import tdgl_amd as tdgl
    from tdgl_amd.parameter import PiecewiseLinear, SeparableEpsilon, TabulatedCurrents

    def A_t(x, y, z, *, t):
        return np.stack([0 * x, t * x, 0 * x], axis=1)

    with pytest.raises(ValueError, match="applied_vector_potential"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=[0.0, tdgl.Parameter(A_t, time_dependent=True)])

    def pulse(x, y, z, *, t):
        return np.ones_like(x) * (t < 1)

    factor = tdgl.Parameter(pulse, time_dependent=True)
    factor.uniform_in_space = True
    field = tdgl.ConstantField(1.0, field_units="mT", length_units="um")
    assert (factor * field).separable_product() is not None
    with pytest.raises(ValueError, match="not a LinearRamp"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=[factor * field, 0.0])
    with pytest.raises(ValueError, match="terminal_currents"):
        tdgl.solve_ensemble(device, _options(), terminal_currents=[lambda t: dict(source=t, drain=-t), None])

    def eps_t(r, *, t):
        return 1.0

    with pytest.raises(ValueError, match="disorder_epsilon"):
        tdgl.solve_ensemble(device, _options(), disorder_epsilon=[1.0, eps_t])
    ramp = tdgl.LinearRamp(tmin=0, tmax=2) * field
    table = TabulatedCurrents([0.0, 1.0], dict(source=[0.0, 1.0], drain=[0.0, -1.0]))
    eps = SeparableEpsilon(lambda r: np.ones(len(r)), PiecewiseLinear([0.0, 1.0], [1.0, 0.5]))
    with pytest.raises(ValueError, match="replica 1: a field ramp combined"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=ramp, terminal_currents=[None, table])
    with pytest.raises(ValueError, match="a field ramp combined"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=ramp, disorder_epsilon=eps)


def test_dimensionless_ramps_and_epsilon_tables_broadcast(device, no_gpu):
    from tdgl_amd import SolverOptions
    from tdgl_amd.ensemble import ensemble_dimensionless

    mesh = device.mesh
    m, n = len(mesh.edge_mesh.edges), len(mesh.sites)
    base = np.ones((m, 2))
    ramp = dict(tmin=0.0, tmax=2.0, initial=0.5, final=1.0)
    opts = SolverOptions(solve_time=1.0)
    # one (A_base, ramp) for every replica; link exponents from the ramp at t = 0
    ens = ensemble_dimensionless(mesh, opts, [None, None], vector_potential_ramp=(base, ramp))
    assert len(ens.reps) == 2
    assert all(r.field.kind == "ramp" and np.array_equal(r.current_A_applied, 0.5 * base) for r in ens.reps)
    # a list with None for a static replica
    ens = ensemble_dimensionless(mesh, opts, [None, np.zeros((m, 2)), None],
                                 vector_potential_ramp=[(base, ramp), None, (base, dict(ramp, final=3.0))])
    assert [r.field.kind for r in ens.reps] == ["ramp", "static", "ramp"]
    assert ens.reps[2].field.ramp["final"] == 3.0
    # epsilon tables: one for all, or one per replica
    eps0 = np.full(n, 0.9)
    ens = ensemble_dimensionless(mesh, opts, np.zeros((m, 2)), epsilon_table=(eps0, [0.0, 1.0], [1.0, 0.5]))
    assert len(ens.reps) == 1 and ens.reps[0].dynamic_epsilon
    assert np.allclose(ens.reps[0].epsilon_func(0.5), 0.75 * eps0)
    ens = ensemble_dimensionless(mesh, opts, np.zeros((m, 2)),
                                 epsilon_table=[(eps0, [0.0, 1.0], [1.0, 0.5]), None, (1.0, [0.0], [0.8])])
    assert [r.dynamic_epsilon for r in ens.reps] == [True, False, True]
    assert np.array_equal(ens.reps[2].epsilon, np.full(n, 0.8))
    # lists of different lengths
    with pytest.raises(ValueError, match="different lengths"):
        ensemble_dimensionless(mesh, opts, [np.zeros((m, 2))] * 2, vector_potential_ramp=[(base, ramp)] * 3)
    with pytest.raises(ValueError, match="different lengths"):
        ensemble_dimensionless(mesh, opts, np.zeros((m, 2)), epsilon=[1.0, 1.0],
                               epsilon_table=[(eps0, [0.0], [1.0])] * 3)
    # a ramp and an epsilon table in one replica
    with pytest.raises(ValueError, match="a field ramp combined"):
        ensemble_dimensionless(mesh, opts, None, vector_potential_ramp=(base, ramp), epsilon_table=(eps0, [0.0], [1.0]))
