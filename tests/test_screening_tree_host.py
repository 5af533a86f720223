"""CPU tests of the screening treecode (``SolverOptions.screening_method="tree"``): the options, the NumPy model of
the barycentric Lagrange treecode (tests/bltc_model.py) against the float64 direct sum, and the refusal of
one-process-per-GPU mode before any device work."""

import dataclasses

import numpy as np
import pytest

from bltc_model import Treecode, basis, direct_sum
from helpers import synthetic_mesh

TARGET = 1e-8  # two decades under the tightest screening_tolerance of the reference's tests (1e-6)


def strip_with_hole(max_edge_length=0.35):
    """A 4:1 strip with a round hole (~10.7k sites at the default pitch), meshed by the library's polygon mesher."""
    import tdgl_amd as tdgl
    from tdgl_amd.geometry import box, circle

    layer = tdgl.Layer(coherence_length=1.0, london_lambda=2.0, thickness=0.1)
    device = tdgl.Device("strip", layer=layer, film=tdgl.Polygon("film", points=box(40.0, 10.0)),
                         holes=[tdgl.Polygon("hole", points=circle(2.5, center=(-8.0, 0.5)))], length_units="um")
    device.make_mesh(max_edge_length=max_edge_length)
    return device.mesh


def weights(mesh, kind, seed=3):
    """area * K_site: a smooth sheet current (a sinusoid plus an offset) or random weights."""
    x, y = mesh.sites[:, 0], mesh.sites[:, 1]
    a = mesh.areas
    if kind == "smooth":
        lx, ly = np.ptp(x), np.ptp(y)
        return a[:, None] * np.column_stack([np.sin(2 * np.pi * y / ly) + 0.3, np.cos(2 * np.pi * x / lx) - 0.2])
    return a[:, None] * np.random.default_rng(seed).standard_normal((len(x), 2))


_MESHES = {}


def _mesh(name):
    if name not in _MESHES:
        _MESHES[name] = synthetic_mesh(92) if name == "film" else strip_with_hole()
    return _MESHES[name]


def _error(mesh, A_tree, w, rows):
    """The two measures of the accuracy target: max |dA| / max |A| (smooth currents) and
    max |dA|_e / (sum_j |w_j| / r_ej) (random weights, where A itself cancels)."""
    A, S = direct_sum(mesh.sites, mesh.edge_mesh.centers, w, rows)
    return np.abs(A_tree[rows] - A).max() / np.abs(A).max(), (np.abs(A_tree[rows] - A) / S).max()


def test_options_default_to_the_direct_sum_and_validate_the_tree_fields():
    from tdgl_amd import SolverOptions, SolverOptionsError

    o = SolverOptions(solve_time=1.0)
    o.validate()
    assert o.screening_method == "direct"
    assert 2 <= o.screening_tree_degree <= 16 and 0 < o.screening_tree_theta < 1
    names = [f.name for f in dataclasses.fields(SolverOptions)]
    # after device_id: none of the reference's fields move
    assert names[names.index("device_id") + 1:] == ["screening_method", "screening_tree_degree", "screening_tree_theta"]
    SolverOptions(solve_time=1.0, include_screening=True, screening_method="tree", screening_tree_degree=2,
                  screening_tree_theta=0.99).validate()
    bad = [
        (dict(screening_method="fmm"), r"screening_method must be one of \['direct', 'tree'\] \(got 'fmm'\)"),
        (dict(screening_tree_degree=1), r"screening_tree_degree must be in \[2, 16\] \(got 1\)"),
        (dict(screening_tree_degree=17), r"screening_tree_degree must be in \[2, 16\] \(got 17\)"),
        (dict(screening_tree_degree=8.5), r"screening_tree_degree must be in \[2, 16\]"),
        (dict(screening_tree_theta=0.0), r"screening_tree_theta must be in \(0, 1\) \(got 0.0\)"),
        (dict(screening_tree_theta=1.0), r"screening_tree_theta must be in \(0, 1\) \(got 1.0\)"),
        (dict(screening_tree_theta=1.5), r"screening_tree_theta must be in \(0, 1\) \(got 1.5\)"),
    ]
    for kw, msg in bad:
        with pytest.raises(SolverOptionsError, match=msg):
            SolverOptions(solve_time=1.0, **kw).validate()


def test_model_trees_are_contiguous_and_respect_the_leaf_sizes():
    mesh = _mesh("film")
    tc = Treecode(mesh.sites, mesh.edge_mesh.centers, 8, 0.6)
    assert sorted(tc.sperm) == list(range(len(mesh.sites)))
    for nd in tc.nodes:
        if nd["nchild"]:
            kids = tc.nodes[nd["child0"]:nd["child0"] + nd["nchild"]]
            assert kids[0]["begin"] == nd["begin"] and kids[-1]["end"] == nd["end"]
            assert all(a["end"] == b["begin"] for a, b in zip(kids, kids[1:]))
            assert nd["end"] - nd["begin"] > tc.PP
        else:
            assert nd["end"] - nd["begin"] <= tc.PP
        xs = mesh.sites[tc.sperm[nd["begin"]:nd["end"]]]
        assert xs[:, 0].min() == nd["x0"] and xs[:, 0].max() == nd["x1"]  # tight boxes
    assert all(0 < b["end"] - b["begin"] <= 64 for b in tc.batches)
    assert tc.batches[0]["begin"] == 0 and tc.batches[-1]["end"] == len(mesh.edge_mesh.edges)
    # every target sees every source exactly once: far clusters and near ranges partition the sources
    n = len(mesh.sites)
    for far, near in zip(tc.far[::37], tc.near[::37]):
        seen = np.zeros(n, dtype=int)
        for c in far:
            seen[tc.nodes[c]["begin"]:tc.nodes[c]["end"]] += 1
        for a, b in near:
            seen[a:b] += 1
        assert (seen == 1).all()
    st = tc.stats()
    assert st["far_pairs"] + st["near_pairs"] < 0.5 * n * len(mesh.edge_mesh.edges)


def test_model_transfer_reproduces_the_charges_from_the_particles():
    """The upward pass (parents from their children) equals the parents' charges computed from their own sources:
    the parent's Lagrange basis has degree <= p in x and y, so the child's interpolation reproduces it exactly."""
    mesh = _mesh("film")
    tc = Treecode(mesh.sites, mesh.edge_mesh.centers, 6, 0.6)
    w = weights(mesh, "random")
    q = tc.charges(w)
    xs, ws = mesh.sites[tc.sperm], w[tc.sperm]
    inner = [i for i, nd in enumerate(tc.nodes) if nd["nchild"]]
    for i in inner[:: max(1, len(inner) // 12)]:
        b, e = tc.nodes[i]["begin"], tc.nodes[i]["end"]
        want = np.einsum("jk,jl,jc->klc", basis(xs[b:e, 0], tc.px[i]), basis(xs[b:e, 1], tc.py[i]), ws[b:e])
        assert np.abs(q[i] - want).max() < 1e-12 * np.abs(ws[b:e]).sum()


@pytest.mark.parametrize("name", ["film", "strip_with_hole"])
def test_model_meets_the_accuracy_target_at_the_defaults(name):
    from tdgl_amd import SolverOptions

    o = SolverOptions(solve_time=1.0)
    mesh = _mesh(name)
    assert 9_000 < len(mesh.sites) < 13_000
    tc = Treecode(mesh.sites, mesh.edge_mesh.centers, o.screening_tree_degree, o.screening_tree_theta)
    rows = np.random.default_rng(11).choice(len(mesh.edge_mesh.edges), 3000, replace=False)
    for kind in ("smooth", "random"):
        w = weights(mesh, kind)
        err_max, err_sum = _error(mesh, tc.evaluate(w), w, rows)
        err = err_max if kind == "smooth" else err_sum
        assert err <= TARGET, (name, kind, err_max, err_sum)


def test_model_error_falls_monotonically_with_the_degree():
    from tdgl_amd import SolverOptions

    theta = SolverOptions(solve_time=1.0).screening_tree_theta
    mesh = _mesh("film")
    w = weights(mesh, "smooth")
    rows = np.random.default_rng(5).choice(len(mesh.edge_mesh.edges), 1500, replace=False)
    errs = [_error(mesh, Treecode(mesh.sites, mesh.edge_mesh.centers, p, theta).evaluate(w), w, rows)[0]
            for p in range(4, 13)]
    assert all(b < a for a, b in zip(errs, errs[1:])), errs
    assert errs[0] > 1e3 * errs[-1], errs


def test_distributed_mode_refuses_the_tree_before_any_device_work(monkeypatch):
    from tdgl_amd import SolverOptions, hipcore
    from tdgl_amd.distributed import DistributedTDGL

    def no_device(*a, **k):
        raise AssertionError("device work started")

    monkeypatch.setattr(hipcore.TDGLContext, "__init__", no_device)
    mesh = synthetic_mesh(12)
    opts = SolverOptions(solve_time=1.0, include_screening=True, screening_method="tree")
    scr = dict(sites=mesh.sites, edge_centers=mesh.edge_mesh.centers, areas=0.01 * mesh.areas)
    with pytest.raises(ValueError, match="screening_method='tree' is not supported in one-process-per-GPU mode"):
        DistributedTDGL(mesh, opts, np.zeros((len(mesh.edge_mesh.edges), 2)), rank=0, world=1, screening=scr)
