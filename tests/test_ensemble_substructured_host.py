"""solve_ensemble above the dense inverse's cap, on the host: the rule that picks the ensemble's mu solve (dense
inverse, one or two levels of substructured factors, refusal), a mesh of ~15k sites getting through the argument
checks to the context's set-up, and the refusals that stay (no GPU needed)."""

import pytest


@pytest.fixture(scope="module")
def big_device():
    """A film of ~15k sites: above the dense inverse's cap."""
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box

    layer = tdgl.Layer(coherence_length=0.5, london_lambda=2.0, thickness=0.1, gamma=10)
    film = tdgl.Polygon("film", points=box(30, 12))
    source = tdgl.Polygon("source", points=box(0.02, 12, center=(-15, 0)))
    drain = tdgl.Polygon("drain", points=box(0.02, 12, center=(15, 0)))
    dev = tdgl.Device("strip", layer=layer, film=film, terminals=[source, drain], probe_points=[(-5, 0), (5, 0)],
                      length_units="um")
    dev.make_mesh(max_edge_length=0.185)
    return dev


class _Reached(Exception):
    pass


@pytest.fixture
def stop_at_context(monkeypatch):
    """No device context: `build_context` raises _Reached (with the mesh's site count) instead, and creating a
    `TDGLContext` fails the test."""
    from tdgl_amd import ensemble, hipcore

    def refuse(*a, **k):
        raise AssertionError("a GPU context was created")

    def reached(mesh, *a, **k):
        raise _Reached(len(mesh.sites))

    monkeypatch.setattr(hipcore.TDGLContext, "__init__", refuse)
    monkeypatch.setattr(ensemble, "build_context", reached)


def _options(**kw):
    import tdgl_amd as tdgl

    base = dict(solve_time=1.0, field_units="mT", current_units="uA")
    base.update(kw)
    return tdgl.SolverOptions(**base)


def test_mu_path_rule():
    from tdgl_amd import ensemble
    from tdgl_amd.ensemble import ensemble_mu_path

    assert ensemble.ENSEMBLE_DENSE_MAX_SITES == 12_000
    assert ensemble.ENSEMBLE_DENSE_MAX_SITES < ensemble.ENSEMBLE_SUB_MAX_SITES < ensemble.ENSEMBLE_MAX_SITES <= 150_000
    assert ensemble_mu_path(2) == 0
    assert ensemble_mu_path(5_791) == 0
    assert ensemble_mu_path(12_000) == 0
    assert ensemble_mu_path(12_001) == 1
    assert ensemble_mu_path(23_000) == 1
    assert ensemble_mu_path(ensemble.ENSEMBLE_SUB_MAX_SITES) == 1
    assert ensemble_mu_path(ensemble.ENSEMBLE_SUB_MAX_SITES + 1) == 2
    assert ensemble_mu_path(59_000) == 2
    assert ensemble_mu_path(ensemble.ENSEMBLE_MAX_SITES) == 2
    with pytest.raises(ValueError, match="ENSEMBLE_MAX_SITES"):
        ensemble_mu_path(ensemble.ENSEMBLE_MAX_SITES + 1)


def test_mu_path_rule_follows_the_ensemble_constants_only(monkeypatch):
    """Tests force the substructured path on small meshes through the ensemble's constants; the size rule of
    `TDGLContext` (switched off in the test session) plays no part."""
    from tdgl_amd import ensemble
    from tdgl_amd.ensemble import ensemble_mu_path
    from tdgl_amd.hipcore import TDGLContext

    monkeypatch.setattr(TDGLContext, "DENSE_MAX_SITES", 10 ** 9)
    monkeypatch.setattr(TDGLContext, "SUB_MAX_SITES", 10 ** 9)
    monkeypatch.setattr(TDGLContext, "SUB2_MAX_SITES", 10 ** 9)
    assert ensemble_mu_path(20_000) == 1
    monkeypatch.setattr(ensemble, "ENSEMBLE_DENSE_MAX_SITES", 199)
    assert ensemble_mu_path(199) == 0
    assert ensemble_mu_path(1_000) == 1
    monkeypatch.setattr(ensemble, "ENSEMBLE_SUB_MAX_SITES", 199)
    assert ensemble_mu_path(1_000) == 2


def test_a_15k_site_device_reaches_the_context_set_up(big_device, stop_at_context):
    import tdgl_amd as tdgl
    from tdgl_amd.ensemble import ENSEMBLE_DENSE_MAX_SITES, ensemble_mu_path

    n = len(big_device.mesh.sites)
    assert 14_000 < n < 17_000 and n > ENSEMBLE_DENSE_MAX_SITES
    assert ensemble_mu_path(n) == 1
    with pytest.raises(_Reached) as got:
        tdgl.solve_ensemble(big_device, _options(), applied_vector_potential=[0.0, 0.1],
                            terminal_currents=[dict(source=1.0, drain=-1.0), None])
    assert got.value.args[0] == n


def test_refusals_that_stay(big_device, stop_at_context):
    import tdgl_amd as tdgl
    from tdgl_amd.parameter import Parameter

    with pytest.raises(ValueError, match="include_screening"):
        tdgl.solve_ensemble(big_device, _options(include_screening=True), applied_vector_potential=[0.0, 0.1])
    with pytest.raises(ValueError, match="output_file"):
        tdgl.solve_ensemble(big_device, _options(output_file="out.h5"), applied_vector_potential=[0.0, 0.1])

    def A_t(x, y, z, *, t):
        import numpy as np

        return np.stack([0 * x, t * x, 0 * x], axis=1)

    with pytest.raises(ValueError, match="applied_vector_potential"):
        tdgl.solve_ensemble(big_device, _options(), applied_vector_potential=[0.0, Parameter(A_t, time_dependent=True)])
    with pytest.raises(ValueError, match="terminal_currents"):
        tdgl.solve_ensemble(big_device, _options(), terminal_currents=[lambda t: dict(source=t, drain=-t), None])
