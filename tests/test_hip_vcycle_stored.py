"""ONE application of the V-cycle in the precisions the CG applies it in (`vcycle0_f32`, csrc/vcycle.inc; reached
through `TDGLContext.vcycle_stored`) against the float64 model of what the device stores (tests/vcycle_model.py,
itself held to the host restatements by tests/test_vcycle_model_host.py).  A CG converges with a preconditioner that
is wrong in one row, one padded lane or one slice base, so the solves that use this cycle cannot see such a mistake;
this file looks at every entry of z.

Every context: the direct solves and the factor preconditioner switched off (`DENSE_MAX_SITES = SUB_MAX_SITES =
SUB2_MAX_SITES = 0`, `PD_CHOICE = 2`), one AMG candidate.  `precond_storage()`, `index_forms()` and the collapsed
plan are asserted per case, so that a case cannot silently run another path.

  A  mesh_with_sites(4161): two levels, no collapsed chain; P's and A's last SELL slice has a single row; the coarse
     solve is k_dense_matvec.
  B  synthetic_mesh(150), max_coarse=40 (26361 / 2580 / 140 / 9 in the context's order): "gwv" tail on level 1 (k_dense_rows<float>,
     k_tail_up<8, float, uint16_t>); with tail_cycles=1 (no dense V); with collapse=False (the fused levels' fp32
     k_csr_multi<4, C_PRE2 | C_SMOOTH, 4, float>, k_csr_dual<16, D_RESTRICT, 4, 8, float>, k_csr_dual<4, D_PSMOOTH, 4, 2,
     float>); and with the plan `collapsed_operators(tail_rows=1000, dense_rows=200, mid_up=False)` -- an explicit M on
     level 1 without an explicit way up, which the product never builds: the only way to k_csr_down<32, 8, float>.
  C  synthetic_mesh(300), max_coarse=40 (104,620 sites): one intermediate level above a dense tail: k_csr_multi<32, C_AX, 8,
     float>, k_mid_up<8, 8, 2, half_t | float>, k_dense_rows<float>.
  D  A and B with TDGL_INDEX32=1: every index form int32 (k_csr_multi<16, C_AX, 4, float> for the fused restriction,
     k_sell_transfer<T_BASE, float, float, int32_t>, k_sell_spmv<SMOOTH, ., int32_t, float, float, float>, k_tail_up<8, float,
     int32_t>), a request for storage 2 served as 1; and B's mesh with `collapsed_operators(tail_rows=1000,
     dense_rows=200)` (a mid level above a dense tail at 26k sites): the int32 way up, k_csr_dual<16, D_RESTRICT, 4, 2, float>.
  E  mesh_with_sites(33000), reorder="none", relabelled so that one mesh edge joins sites 0 and 32767 (16-bit row
     deltas just fit) or 0 and 32768 (they do not: the int32 k_sell_spmv and k_psi_laplacian by the natural trigger).
     On both: the cycle, and `apply_psi_laplacian` / `apply_mu_laplacian` (k_mu_laplacian reads int32 columns on
     either) against the oracle's matrices at 1e-13 relative.

A, B, C run with storage 1 and 2; every column goes through `vcycle_stored` without q (DOT_BY) and with q (DOT_BY2).

Probe columns (`vcycle_model.probe_columns`; rows counted in the CONTEXT's order, where the slices are; handed over
in site order): e_j - 1/n for j = 0, 63, 64, 255, 256, n - 1, a row of largest and one of smallest degree, the fine
rows of the first and of the last aggregate, the first row of the last slice; cos x cos y; four standard-normal ones.

Per column, against the model:
  * per entry |z_dev - z_model| <= 2^-23 |z_model| + 1e-12 max |z_model|: one fp32 unit in the last place (z is stored
    in fp32; device and model round the same fp64 value up to the order of its sums) plus the floor
    tests/test_hip_parity.py holds the fp64 cycle's restatements to;
  * over a case at most 1 entry in 10^4 not bit-equal to the model as fp32 (the model in two summation orders, CSR
    and CSC products, differs in 0 of 2.1 million entries; arithmetic in fp32 on the device would break this at once);
  * |rz - r . z_dev| <= n u sum |r_i z_i|, the same for qz; z with q is z without q bit for bit;
  * a `poisson_solve` of a fixed right-hand side before and after all applications: the same mu bit for bit, the same
    iteration count and residual.

Measured on the MI355X (s = the model's storage error per column, min .. max, storage 1 | storage 2; in EVERY case 0
entries beyond the bound, 0 entries not bit-equal to the model and a largest deviation of 0 fp32 units):

    case                                   levels                      columns  entries    s, storage 1          s, storage 2
    A                                      4161 / 425                  25       104,025    4.0e-8 .. 1.3e-7      1.7e-4 .. 7.0e-4
    B, two tail cycles                     26361 / 2580 / 140 / 9      20       527,220    4.5e-8 .. 1.3e-7      3.4e-4 .. 7.0e-4
    B, one tail cycle                                                                      5.2e-8 .. 1.4e-7      2.9e-4 .. 6.8e-4
    B, fused levels                                                                        5.8e-8 .. 1.9e-7      2.9e-4 .. 6.8e-4
    B, explicit M, no way up                                                               4.3e-8 .. 1.8e-7      3.4e-4 .. 6.9e-4
    C                                      104620 / 10106 / 560 / 29   28       2,929,360  4.7e-8 .. 1.5e-7      2.8e-4 .. 8.6e-4
    D: A | B | B with a mid level (int32)  (served as storage 1)                           4.0e-8 .. 1.3e-7 | 4.5e-8 .. 1.3e-7 | 4.8e-8 .. 1.3e-7
    E, edge 0 - 32767 (storage 2)          33000 / 3230 / 180          28       924,000                          2.6e-4 .. 8.6e-4
    E, edge 0 - 32768 (served as 1)                                                        4.9e-8 .. 1.5e-7
    E, psi / mu Laplacian against the oracle's matrices, both numberings: 3.6e-16 / 2.7e-16 of the largest entry

(The comparison does see a device that gathers wrongly: with one column index of P's last row moved by one in what the
device is GIVEN, case A leaves the bound in 100 entries, on every one of its 25 columns, by up to 1.8e5 fp32 units, and
agrees in every bit again with the model that has the same index moved.)  C takes 0.6 s per case, host set-up included:
it stays at the mesh of test_collapsed_coarse_chain_matches_host_restatement[300-...] in tests/test_hip_parity.py.

Not covered here: the one-process-per-GPU forms of the cycle (k_sell_spmv<SMOOTH, DOT_NONE, ...> with z on ghost rows,
the `z64` form with a double result, the split restriction around the halo exchange); the natural trigger of P's
int32 form, which needs more than 65,536 coarse rows, about 700k sites (D reaches the kernel through the switch); and
the int32 forms of the time loops' stencil kernels, k_psi_laplacian_ra / k_psi_laplacian_ra_fresh (run-ahead loop) and
k_ens_laplacian* (`solve_ensemble`): E applies the operator through `apply_psi_laplacian` alone."""

import functools

import numpy as np
import pytest

import dense_reference as D
import vcycle_model as VM
from helpers import synthetic_mesh, uniform_field_A

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "A":
        return D.mesh_with_sites(4161)
    if name == "B":
        return synthetic_mesh(150)
    if name == "C":
        return synthetic_mesh(300)
    if name.startswith("E"):
        return _relabelled(D.mesh_with_sites(33000), int(name[1:]))
    raise KeyError(name)


def teardown_module(module):
    _mesh.cache_clear()


def _relabelled(mesh, target):
    """``mesh`` with a neighbour of site 0 given the label ``target`` (the labels in between move down by one): one mesh
    edge then joins sites 0 and ``target``, every other edge joins labels as close as before, give or take one."""
    from tdgl_amd.finite_volume import Mesh

    edges = mesh.edge_mesh.edges
    nb = np.concatenate([edges[edges[:, 0] == 0, 1], edges[edges[:, 1] == 0, 0]])
    b = int(nb.min())
    n = len(mesh.sites)
    assert 0 < b < target < n
    new = np.arange(n)
    new[b] = target
    new[b + 1:target + 1] -= 1
    pts = np.empty_like(mesh.sites)
    pts[new] = mesh.sites
    out = Mesh.from_triangulation(pts, new[np.asarray(mesh.elements)])
    e = np.sort(out.edge_mesh.edges, axis=1)
    span = e[:, 1] - e[:, 0]
    assert span.max() == target and (span == target).sum() == 1 and tuple(e[np.argmax(span)]) == (0, target)
    return out


def _context(mesh, monkeypatch, max_coarse=600, index32=False, plan_kw=None, **ctx_kw):
    from tdgl_amd import amg
    from tdgl_amd.hipcore import TDGLContext

    for attr, value in (("DENSE_MAX_SITES", 0), ("SUB_MAX_SITES", 0), ("SUB2_MAX_SITES", 0), ("PD_CHOICE", 2)):
        monkeypatch.setattr(TDGLContext, attr, value)
    if index32:
        monkeypatch.setenv("TDGL_INDEX32", "1")
    else:
        monkeypatch.delenv("TDGL_INDEX32", raising=False)
    if plan_kw:  # (`_refresh_collapsed` looks the function up when called)
        monkeypatch.setattr(amg, "collapsed_operators", functools.partial(amg.collapsed_operators, **plan_kw))
    ctx = TDGLContext(mesh, **ctx_kw)
    assert ctx.mu.form == "amg" and not ctx.mu.levels
    h = ctx.build_poisson(rtol=1e-10, max_coarse=max_coarse, amg_candidates=1)
    assert not ctx.dense_direct and not ctx.precond_direct
    return ctx, h


def _check(ctx, h, mesh, what, requested, served, forms, plan_mode, n_mid, **options):
    """The assertions of the module docstring on one context.  ``forms``: the entries of `index_forms()` this case is
    about; ``plan_mode``: None (no collapsed plan), "gwv" or "dense"."""
    n = ctx.n
    ctx.set_poisson_options(rtol=1e-10, precond_fp32=requested, **options)
    plan = getattr(ctx, "collapsed_plan", None) if len(h.levels) >= 3 else None
    assert (plan is None) == (plan_mode is None), (h.sizes, plan and plan["mode"])
    if plan is not None:
        assert plan["mode"] == plan_mode and len(plan["mid"]) == n_mid, (h.sizes, plan["mode"], plan["tail"], list(plan["mid"]))
    rng = np.random.default_rng(12)
    rhs = rng.standard_normal(n)
    before = ctx.poisson_solve(rhs)
    assert before[2] <= 1e-10 and before[1] > 3  # (AMG-PCG)
    assert ctx.precond_storage() == served
    got = ctx.index_forms()
    assert got["levels"] == len(h.levels)
    for key, value in forms.items():
        assert got[key] == value, (key, got)
    assert got["level0_f16"] == (served == 2)
    assert got["tail"] == (None if plan is None else (plan["tail"], plan["mode"]))
    # the model of exactly this storage
    mid_f16 = [k for k, v in got["mid"].items() if v["f16"]]
    assert sorted(got["mid"]) == (sorted(plan["up"]) if plan is not None else [])
    B, names = VM.probe_columns(h, np.asarray(mesh.sites)[ctx.perm])
    exact = VM.StoredCycle(h, plan).apply(B)
    model = VM.StoredCycle(h, plan, VM.Storage.mode(served, level0_f16=served == 2, mid_f16=mid_f16)).apply(B)
    s = VM.storage_error(model, exact)
    assert np.all(s > 0.0) and np.all(s < (5e-3 if served == 2 else 1e-6)), (s.min(), s.max())
    q = rng.standard_normal(n)
    z_dev = np.empty_like(B)
    for j in range(B.shape[1]):
        r = np.empty(n)
        r[ctx.perm] = B[:, j]  # (site order: the context's row i is site perm[i])
        z, rz = ctx.vcycle_stored(r)
        z2, rz2, qz2 = ctx.vcycle_stored(r, q)
        assert np.array_equal(z, z2), (names[j], np.abs(z - z2).max())
        bound = n * D.U * np.abs(r * z).sum()
        assert abs(rz - r @ z) <= bound and abs(rz2 - r @ z) <= bound, (names[j], rz, rz2, r @ z, bound)
        assert abs(qz2 - q @ z) <= n * D.U * np.abs(q * z).sum(), (names[j], qz2, q @ z)
        z_dev[:, j] = z[ctx.perm]
    after = ctx.poisson_solve(rhs)
    cmp = VM.compare(z_dev, model)
    print(f"{what}: levels {h.sizes}, {B.shape[1]} columns, s {s.min():.3g} .. {s.max():.3g}, not bit-equal {cmp['unequal']} of "
          f"{cmp['size']}, largest deviation {cmp['ulps']:.3g} fp32 units, beyond the bound {cmp['excess']}")
    assert cmp["excess"] == 0, (what, [names[j] for j in cmp["excess_columns"]])
    assert cmp["unequal"] <= VM.UNEQUAL_CAP * cmp["size"], (what, cmp)
    # the CG's state is as it was: the same solve, bit for bit
    assert before[1] == after[1] and np.array_equal(before[0], after[0]) and before[2] == after[2]


ALL16 = dict(A16=True, P16=True, F16=True)
ALL32 = dict(A16=False, P16=False, F16=False)


@pytest.mark.parametrize("storage", [1, 2])
def test_two_levels_with_a_single_row_in_the_last_slice(storage, monkeypatch):
    mesh = _mesh("A")
    ctx, h = _context(mesh, monkeypatch)
    try:
        assert len(h.levels) == 2 and ctx.n == 4161 and ctx.n % VM.WAVE == 1
        _check(ctx, h, mesh, f"A, storage {storage}", storage, storage, dict(ALL16, tailW16=None), None, 0)
    finally:
        ctx.close()


B_VARIANTS = {
    "two tail cycles": (dict(), None, "gwv", 0, dict(tailW16=True)),
    "one tail cycle": (dict(tail_cycles=1), None, "gwv", 0, dict(tailW16=True)),
    "fused levels": (dict(collapse=False), None, None, 0, dict(tailW16=None)),
    "explicit M, no way up": (dict(), dict(tail_rows=1000, dense_rows=200, mid_up=False), "dense", 1, dict(tailW16=None)),
}


@pytest.mark.parametrize("storage", [1, 2])
@pytest.mark.parametrize("variant", list(B_VARIANTS))
def test_sparse_dense_tail_and_fused_levels(variant, storage, monkeypatch):
    options, plan_kw, plan_mode, n_mid, forms = B_VARIANTS[variant]
    mesh = _mesh("B")
    ctx, h = _context(mesh, monkeypatch, max_coarse=40, plan_kw=plan_kw)
    try:
        assert h.sizes == [26361, 2580, 140, 9]  # (in the context's reverse Cuthill-McKee order)
        _check(ctx, h, mesh, f"B, {variant}, storage {storage}", storage, storage, dict(ALL16, **forms), plan_mode, n_mid, **options)
        if variant == "two tail cycles":
            assert ctx.collapsed_plan["V"].shape[1] > 0
        if variant == "explicit M, no way up":
            assert ctx.index_forms()["mid"] == {} and sorted(ctx.collapsed_plan["mid"]) == [1]
    finally:
        ctx.close()


@pytest.mark.parametrize("storage", [1, 2])
def test_intermediate_level_above_a_dense_tail(storage, monkeypatch):
    mesh = _mesh("C")
    ctx, h = _context(mesh, monkeypatch, max_coarse=40)
    try:
        _check(ctx, h, mesh, f"C, storage {storage}", storage, storage, dict(ALL16, tailW16=None), "dense", 1)
        assert ctx.index_forms()["mid"] == {1: dict(off16=True, f16=storage == 2)}
    finally:
        ctx.close()


D_CASES = {
    "A": ("A", 600, None, None, 0, dict(tailW16=None), {}),
    "B": ("B", 40, None, "gwv", 0, dict(tailW16=False), {}),
    "B, mid level": ("B", 40, dict(tail_rows=1000, dense_rows=200), "dense", 1, dict(tailW16=None), {1: dict(off16=False, f16=False)}),
}


@pytest.mark.parametrize("case", list(D_CASES))
def test_every_index_form_int32(case, monkeypatch):
    name, max_coarse, plan_kw, plan_mode, n_mid, forms, mid = D_CASES[case]
    mesh = _mesh(name)
    ctx, h = _context(mesh, monkeypatch, max_coarse=max_coarse, index32=True, plan_kw=plan_kw)
    try:
        assert ctx.index_forms()["laplacian16"] is False
        _check(ctx, h, mesh, f"D, {case}, TDGL_INDEX32=1, storage 2 requested", 2, 1, dict(ALL32, **forms), plan_mode, n_mid)
        assert ctx.index_forms()["mid"] == mid
    finally:
        ctx.close()


@pytest.mark.parametrize("target, fits", [(32767, True), (32768, False)])
def test_row_deltas_at_the_edge_of_16_bits(target, fits, monkeypatch):
    from oracle.fv_operators import laplacian_matrix

    mesh = _mesh(f"E{target}")
    ctx, h = _context(mesh, monkeypatch, reorder="none")
    try:
        assert np.array_equal(ctx.perm, np.arange(ctx.n)) and ctx.n == 33000
        assert ctx.index_forms()["laplacian16"] is fits
        _check(ctx, h, mesh, f"E, an edge between sites 0 and {target}", 2, 2 if fits else 1,
               dict(A16=fits, P16=True, F16=True, tailW16=True), "gwv", 0)
        # the stencil kernels on the same pattern, against the oracle's matrices
        rng = np.random.default_rng(13)
        A_link = uniform_field_A(mesh, 0.1)
        ctx.set_link_exponents(A_link)
        psi = rng.standard_normal(ctx.n) + 1j * rng.standard_normal(ctx.n)
        want = laplacian_matrix(mesh, link_exponents=A_link)[0] @ psi
        got = ctx.apply_psi_laplacian(psi)
        d_psi = np.abs(got - want).max() / np.abs(want).max()
        mu = rng.standard_normal(ctx.n)
        want = laplacian_matrix(mesh)[0] @ mu
        got = ctx.apply_mu_laplacian(mu)
        d_mu = np.abs(got - want).max() / np.abs(want).max()
        print(f"E, {target}: psi Laplacian {d_psi:.3g}, mu Laplacian {d_mu:.3g} (relative to the largest entry)")
        assert d_psi < 1e-13 and d_mu < 1e-13
    finally:
        ctx.close()
