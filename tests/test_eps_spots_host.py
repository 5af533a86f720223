"""Hot spots in epsilon on the host: the NumPy model against the closed form of the reference fixture's moving spot,
what TDGLSolver and solve_ensemble recognise as device-evaluable, what the constructors refuse, and solve_ensemble's
argument handling -- all decided before a GPU context exists (no GPU needed)."""

import inspect

import numpy as np
import pytest

import eps_spots_model as model
from conftest import load_golden
from helpers import reference_mesh
from test_ensemble_dynamic_host import _options, _Reached, _replicas, device, no_gpu  # noqa: F401  (fixtures)

# the fixture's spot: epsilon = 1 - 0.6 exp(-|r - c(t)|^2 / 4), c(t) = (-6 + 1.5 t, 1); the nodes reach past its last call
FIXTURE_SPOT = dict(times=[0.0, 16.0], centers=[[-6.0, 1.0], [18.0, 1.0]], amplitudes=0.6, sigmas=np.sqrt(2.0))


def _closed_form(sites, t):
    c = np.array([-6.0 + 1.5 * t, 1.0])
    return 1.0 - 0.6 * np.exp(-((sites - c) ** 2).sum(axis=1) / 4.0)


def test_model_reproduces_the_fixtures_closed_form():
    """One spot with nodes t = [0, 16], cx = [-6, 18], cy = 1, a = 0.6, sigma = sqrt 2 at every call_time of
    traj_dynamic_small, within 4 * 2^-52 (measured: 2.2e-16); and so does the package's HotSpotEpsilon, bit for bit the
    model."""
    import tdgl_amd as tdgl

    g = load_golden("traj_dynamic_small")
    sites = reference_mesh(load_golden("mesh_small")).sites
    assert g["call_time"][-1] > 8.0  # (nodes ending at 8 would be off by 3e-4 there)
    eps = tdgl.HotSpotEpsilon(1.0, [tdgl.HotSpot(**FIXTURE_SPOT)])
    worst = 0.0
    for t in g["call_time"]:
        want = _closed_form(sites, float(t))
        got = model.epsilon(sites, 1.0, model.spot_values([FIXTURE_SPOT], t))
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.array_equal(eps(sites, t=float(t)), got)
    print(f"model vs closed form over {len(g['call_time'])} call times: worst {worst:.2e}")
    assert worst <= 4 * model.EPS
    # nodes that end at t = 8 hold the centre there: off at the fixture's last call
    short = dict(FIXTURE_SPOT, times=[0.0, 8.0], centers=[[-6.0, 1.0], [6.0, 1.0]])
    t = float(g["call_time"][-1])
    assert np.abs(model.epsilon(sites, 1.0, model.spot_values([short], t)) - _closed_form(sites, t)).max() > 1e-4


def test_table_value_is_the_librarys():
    from tdgl_amd.parameter import table_value

    times, values = [0.0, 0.7, 1.9, 4.0], [0.3, -1.1, 2.5, 2.0]
    for t in (-1.0, 0.0, 0.1, 0.7, 1.0, 1.9, 3.999, 4.0, 9.0):
        assert table_value(np.array(times), np.array(values), t) == model.table_value(times, values, t)
    assert model.table_value(times, values, -1.0) == 0.3 and model.table_value(times, values, 9.0) == 2.0
    assert model.table_value(times, values, 1.3) == -1.1 + (2.5 - -1.1) * ((1.3 - 0.7) / (1.9 - 0.7))


def test_hot_spot_epsilon_is_recognised(device, no_gpu):
    import tdgl_amd as tdgl

    spot = tdgl.HotSpot([0.0, 1.0], [[-1.0, 0.0], [1.0, 0.2]], [0.0, 0.5], [0.2, 0.4])
    eps = tdgl.HotSpotEpsilon(lambda r: 0.9 * np.ones(len(r)), [spot])
    # the reference's calling convention
    spec = inspect.getfullargspec(eps)
    assert spec.kwonlyargs == ["t", "vectorized"] and spec.kwonlydefaults == dict(t=0.0, vectorized=True)
    r = np.array([[0.0, 0.1], [0.5, -0.3]])
    assert eps(r, t=0.5).shape == (2,) and isinstance(eps(r[0], t=0.5), float) and eps(r[0], t=0.5) == eps(r, t=0.5)[0]
    assert np.array_equal(eps(r), np.full(2, 0.9))  # a = 0 at t = 0: exactly the static part
    reps = _replicas(lambda: tdgl.solve_ensemble(device, _options(), disorder_epsilon=[eps, 1.0]))
    assert reps[0]._eps_spots is not None and reps[0].dynamic_epsilon and reps[0]._eps_table is None
    assert reps[1]._eps_spots is None and not reps[1].dynamic_epsilon
    eps0, spots = reps[0]._eps_spots
    assert np.array_equal(eps0, np.full(len(device.mesh.sites), 0.9)) and spots == [spot]
    assert np.array_equal(reps[0].epsilon, eps(reps[0].sites, t=0.0))
    # four spots pass, five fall back to the per-step callable (which the ensemble refuses, as any callable)
    reps = _replicas(lambda: tdgl.solve_ensemble(device, _options(), disorder_epsilon=tdgl.HotSpotEpsilon(1.0, [spot] * 4)))
    assert len(reps[0]._eps_spots[1]) == 4
    five = tdgl.HotSpotEpsilon(1.0, [spot] * 5)
    with pytest.raises(ValueError, match=r"replica 0: a time-dependent disorder_epsilon is not supported \(SeparableEpsilon is\)"):
        tdgl.solve_ensemble(device, _options(), disorder_epsilon=five)
    from tdgl_amd.ensemble import _ReplicaInputs

    rep = _ReplicaInputs(device, _options(), disorder_epsilon=five)
    assert rep._eps_spots is None and rep.dynamic_epsilon and rep.epsilon_func is not None
    assert not rep.device_evaluates_epsilon()
    # tabulated currents go with spots as with a SeparableEpsilon; a device-evaluated field does not, in the same words
    from tdgl_amd.parameter import TabulatedCurrents

    table = TabulatedCurrents([0.0, 1.0], dict(source=[0.0, 1.0], drain=[0.0, -1.0]))
    _replicas(lambda: tdgl.solve_ensemble(device, _options(), terminal_currents=table, disorder_epsilon=eps))
    ramp = tdgl.LinearRamp(tmin=0, tmax=2) * tdgl.ConstantField(1.0, field_units="mT", length_units="um")
    with pytest.raises(ValueError, match="replica 0: a field ramp combined with TabulatedCurrents or a SeparableEpsilon in one replica is not supported"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=ramp, disorder_epsilon=eps)


def test_every_rule_refuses_and_names_its_argument():
    import tdgl_amd as tdgl
    from tdgl_amd.hipcore import epsilon_spots_args

    ok = dict(times=[0.0, 1.0], centers=[[0.0, 0.0], [1.0, 0.0]], amplitudes=[0.1, 0.2], sigmas=[1.0, 2.0])
    tdgl.HotSpot(**ok)
    for bad, name in (
        (dict(times=[0.0, 0.0]), "times"), (dict(times=[1.0, 0.0]), "times"), (dict(times=[0.0, np.inf]), "times"),
        (dict(centers=[[0.0, 0.0], [np.nan, 0.0]]), "centers"), (dict(centers=[[0.0, 0.0]]), "centers"),
        (dict(amplitudes=[0.1, -0.2]), "amplitudes"), (dict(amplitudes=[0.1, np.inf]), "amplitudes"),
        (dict(amplitudes=[0.1, 0.2, 0.3]), "amplitudes"),
        (dict(sigmas=[1.0, 0.0]), "sigmas"), (dict(sigmas=[1.0, -1.0]), "sigmas"), (dict(sigmas=[np.nan, 1.0]), "sigmas"),
        (dict(sigmas=[1.0, 1e-170]), "sigmas"),  # sigma^2 underflows: a site at the centre would get 0 / 0
    ):
        with pytest.raises(ValueError, match=name):
            tdgl.HotSpot(**dict(ok, **bad))
    with pytest.raises(ValueError, match="spots"):
        tdgl.HotSpotEpsilon(1.0, [])
    # an array-valued static belongs to the site array it was made for: a single point, or other points, are refused
    arr = tdgl.HotSpotEpsilon(np.array([0.5, 0.6, 0.7]), [tdgl.HotSpot(**ok)])
    assert arr(np.zeros((3, 2)), t=0.5).shape == (3,)
    for r in (np.zeros(2), np.zeros((2, 2))):
        with pytest.raises(ValueError, match="static"):
            arr(r, t=0.5)
    sites = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    args = epsilon_spots_args(3, sites, 0.5, [ok, tdgl.HotSpot(0.0, [0.5, 0.5], 0.3, 0.7)])
    assert args[2] == 2 and list(args[3][:3]) == [0, 2, 3]
    for call, name in (
        (lambda: epsilon_spots_args(3, sites, 0.5, []), "spots"),
        (lambda: epsilon_spots_args(3, sites, 0.5, [ok] * 5), "spots"),
        (lambda: epsilon_spots_args(3, sites[:2], 0.5, [ok]), "sites"),
        (lambda: epsilon_spots_args(3, sites + np.inf, 0.5, [ok]), "sites"),
        (lambda: epsilon_spots_args(3, sites, [0.5, 0.5], [ok]), "eps0"),
        (lambda: epsilon_spots_args(3, sites, [0.5, 1.5, 0.5], [ok]), "eps0"),
        (lambda: epsilon_spots_args(3, sites, np.nan, [ok]), "eps0"),
    ):
        with pytest.raises(ValueError, match=name):
            call()


def test_dimensionless_epsilon_spots_broadcast(device, no_gpu):
    from tdgl_amd import SolverOptions
    from tdgl_amd.ensemble import ensemble_dimensionless

    mesh = device.mesh
    n, m = len(mesh.sites), len(mesh.edge_mesh.edges)
    opts = SolverOptions(solve_time=1.0)
    spot = dict(times=[0.0, 1.0], centers=[[-1.0, 0.0], [1.0, 0.0]], amplitudes=0.5, sigmas=0.3)
    eps0 = np.full(n, 0.9)

    def reps_of(**kw):
        with pytest.raises(_Reached) as info:
            ensemble_dimensionless(mesh, opts, np.zeros((m, 2)), **kw).solve()
        return info.value.args[0]

    # one value for every replica ...
    reps = reps_of(epsilon_spots=(eps0, [spot]), currents=[None, None])
    assert len(reps) == 2 and all(r._eps_spots is not None and r.dynamic_epsilon for r in reps)
    assert np.array_equal(reps[0].epsilon, model.epsilon(mesh.sites, eps0, model.spot_values([spot], 0.0)))
    assert np.array_equal(reps[0].epsilon_func(0.4), model.epsilon(mesh.sites, eps0, model.spot_values([spot], 0.4)))
    # ... or a list with None for the replicas without, next to tables
    reps = reps_of(epsilon_spots=[(eps0, [spot]), None, (1.0, [spot, spot]), None],
                   epsilon_table=[None, (eps0, [0.0, 1.0], [1.0, 0.5]), None, None])
    assert [r._eps_spots is not None for r in reps] == [True, False, True, False]
    assert [r._eps_table is not None for r in reps] == [False, True, False, False]
    assert len(reps[2]._eps_spots[1]) == 2 and not reps[3].dynamic_epsilon
    with pytest.raises(ValueError, match="replica 1: epsilon_spots and epsilon_table exclude each other"):
        reps_of(epsilon_spots=[None, (eps0, [spot])], epsilon_table=[None, (eps0, [0.0], [1.0])])
    with pytest.raises(ValueError, match="different lengths"):
        reps_of(epsilon_spots=[(eps0, [spot])] * 3, currents=[None, None])
    with pytest.raises(ValueError, match="amplitudes"):
        reps_of(epsilon_spots=(eps0, [dict(spot, amplitudes=-0.5)]))
    # with a device-evaluated field in one replica: refused in the words of the table's refusal
    base = np.ones((m, 2))
    with pytest.raises(ValueError, match="a field ramp combined with TabulatedCurrents or a SeparableEpsilon"):
        reps_of(vector_potential_ramp=(base, dict(tmin=0.0, tmax=1.0, initial=0.0, final=1.0)), epsilon_spots=(eps0, [spot]))
