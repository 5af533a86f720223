"""The preconditioner's top separator in block low-rank form (dense.inc: dense_to_blr; kernels.inc: k_blr_project /
k_blr_finish) against the dense fp32 tiles it replaces (TDGL_PD_BLR=0), on a three-level preconditioner of ~110k sites:
what the form does for the CG.  What the form and its two kernels must compute entry by entry is in
tests/test_blr_form_host.py (the arrays, on the host) and tests/test_hip_blr_form.py (the kernels against the float64 model
of tests/blr_model.py); the compression of a single block in tests/test_blr_host.py."""

import numpy as np
import pytest

from helpers import synthetic_mesh

pytestmark = pytest.mark.gpu


def _precond_ctx(mesh, monkeypatch, blr):
    from tdgl_amd.hipcore import TDGLContext

    # (the `precond_direct_solve` fixture's settings, super-super-blocks of 6,000 sites: a top separator of ~2.2k sites)
    for name, value in (("DENSE_MAX_SITES", 199), ("SUB_MAX_SITES", 199), ("SUB2_MAX_SITES", 199), ("SUB3_MIN_SITES", 200),
                        ("SUB3_BIG", 6000), ("PD_MAX_SITES", 10 ** 9), ("PD_CHOICE", 1)):
        monkeypatch.setattr(TDGLContext, name, value)
    monkeypatch.setenv("TDGL_PD_BLR", "1" if blr else "0")
    ctx = TDGLContext(mesh)
    ctx.build_poisson(rtol=1e-10)
    assert ctx.precond_direct and not ctx.dense_direct, ctx.setup_times
    return ctx


@pytest.fixture(scope="module")
def mesh110k():
    return synthetic_mesh(300)


def test_compressed_top_separator_against_the_dense_tiles(mesh110k, monkeypatch):
    """The form saves bytes, the CG it preconditions takes no more iterations than with the dense tiles, and both
    reach rtol 1e-10 at the same solution."""
    n = len(mesh110k.sites)
    assert n >= 100_000
    ctxs = {blr: _precond_ctx(mesh110k, monkeypatch, blr) for blr in (True, False)}
    info = ctxs[True].precond_direct_blr()
    assert info["on"] and not ctxs[False].precond_direct_blr()["on"], info
    assert info["pairs"] > 0 and info["bytes"] < 0.6 * info["dense_bytes"], info
    rhs = np.random.default_rng(3).standard_normal(n)
    rhs -= rhs.mean()
    out = {}
    for blr, ctx in ctxs.items():
        out[blr] = ctx.poisson_solve(rhs)
    for ctx in ctxs.values():
        ctx.close()
    (mu_c, it_c, rel_c), (mu_d, it_d, rel_d) = out[True], out[False]
    assert rel_c <= 1e-10 and rel_d <= 1e-10 and it_c <= it_d + 1, (it_c, it_d, rel_c, rel_d)
    assert np.linalg.norm(mu_c - mu_d) <= 1e-9 * np.linalg.norm(mu_d)


def test_decades_per_application_stay_above_five(mesh110k, monkeypatch):
    ctx = _precond_ctx(mesh110k, monkeypatch, True)
    assert ctx.precond_direct_blr()["on"]
    rng = np.random.default_rng(4)
    for _ in range(12):
        _, its, rel = ctx.poisson_solve(rng.standard_normal(len(mesh110k.sites)))
        assert its <= 3 and rel <= 1e-10
    rate = ctx.precond_direct_stats()["decades_per_application"]
    ctx.close()
    assert rate >= 5.0, rate


def test_fp64_direct_solve_is_untouched(monkeypatch):
    """The fp64 direct solve (the run-ahead loop's, <= 400k sites) keeps its exact dense top separator: bit for bit
    the same with the switch on and off, and never in block low-rank form."""
    from tdgl_amd.hipcore import TDGLContext

    mesh = synthetic_mesh(90)
    monkeypatch.setattr(TDGLContext, "DENSE_MAX_SITES", 0)
    monkeypatch.setattr(TDGLContext, "SUB_MAX_SITES", 200)
    monkeypatch.setattr(TDGLContext, "SUB2_MAX_SITES", 10 ** 6)
    monkeypatch.setattr(TDGLContext, "SUB3_MIN_SITES", 200)
    monkeypatch.setattr(TDGLContext, "SUB3_BIG", 3000)
    rhs = np.random.default_rng(5).standard_normal(len(mesh.sites))
    got = []
    for flag in ("1", "0"):
        monkeypatch.setenv("TDGL_PD_BLR", flag)
        ctx = TDGLContext(mesh, direct_solve=True)
        ctx.build_poisson(rtol=1e-10)
        assert not ctx.precond_direct and not ctx.precond_direct_blr()["on"]
        got.append(ctx.poisson_solve(rhs)[0])
        ctx.close()
    assert np.array_equal(got[0], got[1])
