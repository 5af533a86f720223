"""solve_ensemble's argument handling on the host: broadcasting of the per-replica arguments and every refusal,
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


@pytest.fixture
def no_gpu(monkeypatch):
    """Any attempt to create a device context fails the test."""
    from tdgl_amd import ensemble, hipcore

    def refuse(*a, **k):
        raise AssertionError("a GPU context was created")

    monkeypatch.setattr(hipcore.TDGLContext, "__init__", refuse)
    monkeypatch.setattr(ensemble, "build_context", refuse)


def _options(**kw):
    import tdgl_amd as tdgl

    base = dict(solve_time=1.0, field_units="mT", current_units="uA")
    base.update(kw)
    return tdgl.SolverOptions(**base)


def test_broadcasting_of_per_replica_arguments():
    from tdgl_amd.ensemble import broadcast_replicas

    R, args = broadcast_replicas(a=[0.0, 0.1, 0.2], b=dict(source=1, drain=-1), c=None, d=np.array([1.0, 0.9, 0.8]))
    assert R == 3
    assert args["a"] == [0.0, 0.1, 0.2]
    assert args["b"] == [dict(source=1, drain=-1)] * 3
    assert args["c"] == [None] * 3
    assert args["d"] == [1.0, 0.9, 0.8]
    R, args = broadcast_replicas(a=0.5, b=None)
    assert R == 1 and args == dict(a=[0.5], b=[None])
    fn = lambda r: 1.0  # noqa: E731
    R, args = broadcast_replicas(a=fn, b=(1, 2))
    assert R == 2 and args["a"] == [fn, fn]


def test_replica_inputs_match_the_solver_set_up(device):
    """The per-replica inputs are TDGLSolver's own: vector potential, epsilon and mu boundary values."""
    from tdgl_amd.ensemble import _ReplicaInputs

    opts = _options()
    eps = lambda r: 1.0 - 0.1 * (r[0] > 0)  # noqa: E731
    rep = _ReplicaInputs(device, opts, applied_vector_potential=0.3, terminal_currents=dict(source=2.0, drain=-2.0),
                         disorder_epsilon=eps)
    assert rep.ctx is None
    assert rep.current_A_applied.shape == (len(device.mesh.edge_mesh.edges), 2)
    assert np.abs(rep.current_A_applied).max() > 0
    assert set(np.unique(rep.epsilon)) == {0.9, 1.0}
    term = {t.name: t for t in rep.terminal_info}
    J = device.current_scale("uA") * 2.0
    assert np.allclose(rep.mu_boundary[term["source"].boundary_edge_indices], J / term["source"].length)
    assert np.allclose(rep.mu_boundary[term["drain"].boundary_edge_indices], -J / term["drain"].length)


def test_mismatched_list_lengths_raise(device, no_gpu):
    import tdgl_amd as tdgl

    with pytest.raises(ValueError, match="different lengths"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=[0.0, 0.1],
                            terminal_currents=[dict(source=i, drain=-i) for i in range(3)])


def test_screening_is_refused(device, no_gpu):
    import tdgl_amd as tdgl

    with pytest.raises(ValueError, match="include_screening"):
        tdgl.solve_ensemble(device, _options(include_screening=True), applied_vector_potential=[0.0, 0.1])


def test_output_file_is_refused(device, no_gpu, tmp_path):
    import tdgl_amd as tdgl

    with pytest.raises(ValueError, match="output_file"):
        tdgl.solve_ensemble(device, _options(output_file=str(tmp_path / "out.h5")), applied_vector_potential=[0.0, 0.1])


def test_time_dependent_drives_are_refused(device, no_gpu):
    import tdgl_amd as tdgl

    def A_t(x, y, z, *, t):
        return np.stack([0 * x, t * x, 0 * x], axis=1)

    with pytest.raises(ValueError, match="applied_vector_potential"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=[0.0, tdgl.Parameter(A_t, time_dependent=True)])
    with pytest.raises(ValueError, match="terminal_currents"):
        tdgl.solve_ensemble(device, _options(), terminal_currents=[lambda t: dict(source=t, drain=-t), None])

    def eps_t(r, *, t):
        return 1.0

    with pytest.raises(ValueError, match="disorder_epsilon"):
        tdgl.solve_ensemble(device, _options(), disorder_epsilon=[1.0, eps_t])


def test_too_many_sites_is_refused(device, no_gpu, monkeypatch):
    import tdgl_amd as tdgl
    from tdgl_amd import ensemble

    monkeypatch.setattr(ensemble, "ENSEMBLE_MAX_SITES", len(device.mesh.sites) - 1)
    with pytest.raises(ValueError, match="ENSEMBLE_MAX_SITES"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=[0.0, 0.1])


def test_seed_of_another_device_is_refused(device, no_gpu):
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box

    other = tdgl.Device("other", layer=device.layer, film=tdgl.Polygon("film", points=box(3, 3)), length_units="um")
    other.make_mesh(max_edge_length=0.4)
    n = len(other.mesh.sites)
    data = tdgl.TDGLData(0, 0.0, 0.1, np.ones(n, dtype=complex), np.zeros(n), np.zeros(1), np.zeros(1))
    seed = tdgl.Solution(device=other, options=_options(), saved_steps=[data], dynamics=tdgl.DynamicsData(dt=np.zeros(1)))
    with pytest.raises(ValueError, match="replica 1: the seed_solution.device must be equal"):
        tdgl.solve_ensemble(device, _options(), applied_vector_potential=[0.0, 0.1], seed_solutions=[None, seed])
