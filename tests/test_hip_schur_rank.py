"""ONE rank of the rank-level nested dissection (csrc/schur.inc, tdgl_amd/schur_dd.py, `TDGLContext.build_schur_precond`)
on the device, entry by entry against the float64 model of tests/schur_rank_model.py (held on the CPU by
tests/test_schur_rank_host.py): `k_schur_owned_rhs`, `k_schur_scatter` and its r . z partials, `k_schur_column`, the
touched block and the symmetrisation of `tdgl_poisson_schur_complement`, the device-formed ``S^+`` of an order that is
no multiple of 16 or 64, the gauge-free local factors, ranks that own no interface site, ranks whose interior touches
interface sites they do not own, and both storages of `tdgl_poisson_schur_finish`.

One application contains one collective, and the only data a rank receives in it is the sum of |Gamma| doubles.  The
callback transport hands that buffer to Python, so one device rank runs in this process and the model plays every
other rank inside the all-reduce callback: no process group, nothing spawned.  At set-up the callbacks are the identity
(all-reduce) and zeros (ghosts): `precond_calibrate` applies both preconditioners to a zero residual, to which the other
ranks contribute zeros.  The interface complement is summed by `build_schur_precond`'s ``allreduce_sum``, which here
adds the model's shares of the other ranks; ``C_dev`` is read where `tdgl_poisson_schur_complement` returns it
(``A_GG_owned - argument`` of the sum is C only up to a rounding of A_GG's entries, and not symmetrically so: A_GG_owned
holds the owned rows alone).

Per case (`schur_rank_model.CASES`; every test first asserts the shape facts it was chosen for):

1. ``|C_dev - C_model| <= 8 kappa_I u max |C_model|`` entry by entry (kappa_I: condition number of the rank's A_II; the
   error model of tests/dense_reference.py), C_dev symmetric to the bit and exactly zero outside the touched block.
2. fp64 storage: the rank's term t_r of the sum (recorded in the callback) and the returned z within 8 kappa_I u /
   8 kappa u of the exact model's largest entry.
3. fp32 storage: per probe column  d = max |z_dev - z_model| / max |z_model| <= max(F s, 8 kappa u)  against the model of
   exactly what the device stores, s = the storage error of that column on the rank's rows (host only); the rank's term
   t_r of the sum in the same way (floor 8 kappa_I u: S^+ annihilates a constant added to it, z would not show it).  The device
   can differ from the model by the order of its fp64 sums, by the two inverses it forms itself (the local top
   separator's and S^+: float32 roundings of theirs may fall the other way) and by the complement it summed.  Largest
   d / s per case on the MI355X, over 23 to 60 probe columns per rank (F = four times the largest of them; F <= 1 is a
   condition):

       a (2 local levels; ranks 0 / 1 / 2)            4.4e-8 / 5.7e-8 / 2.9e-8
       b (3 local levels; ranks 1 / 2)                3.2e-8 / 4.0e-8
       c (1 local level; rank 1)                      4.2e-8
       d (prescribed sizes 1 .. 257; ranks 0 / 1)     6.1e-8 / 4.8e-8

   d itself is 4e-16 .. 1.6e-15 everywhere: the order of the fp64 sums alone -- at these orders (68 .. 562 on the local
   top separators, 70 and 99 on the interface) every float32 rounding of the device-formed inverses falls as the
   host's.  So F = 4 x 6.1e-8 = 2.5e-7, and the bound in force is the floor 8 kappa u (1e-12 .. 3e-12).  With fp64
   storage (2.): d <= 5.4e-15 for z and t_r; the complement (1.): 1.2e-16 .. 3.9e-16 of max |C|.

4. ``|rz - r_own . z_own| <= n_own u sum |r z|``.
5. The callback saw exactly one all-reduce, of n_gamma doubles, and no halo exchange; `comm_stats` moved by one
   all-reduce of 8 n_gamma bytes; r = 0 with nothing added gives z = 0 exactly.
6. `guess_gram()`, `precond_direct_stats()`, a `poisson_solve` before and after and a second identical application
   (same bits) show that the entry point left the CG's state alone.

Probe columns (global, zero-mean: ``e_i - 1 / n``; the device rank gets its owned rows): the first and the last row of
one part of every distinct size on every local level and of every local separator, an interface site the rank owns, one
it touches but does not own, a site in another rank's interior (the device's r is then the constant alone and
everything arrives through the sum), four standard-normal columns."""

import functools

import numpy as np
import pytest

import dense_reference as D
import schur_rank_model as M

pytestmark = pytest.mark.gpu

F = 2.5e-7  # (four times the largest measured d / s: see the module docstring)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The host side of a case, once per module: every rank's pieces, kappa of the global matrix."""
    h = M.build_case(name)
    return h, D.condition_number(h.A, D.pinv_reference(h.A))


@functools.lru_cache(maxsize=None)
def _rank(name, r):
    """What the model says of device rank ``r``: kappa_I, C, the probe columns and, exact and with the fp32-stored
    factors, (t_r, z_own, sum of the other ranks' terms)."""
    h, _ = _case(name)
    B, what = h.probe_columns(r)
    out = dict(kappa_I=M.condition_number_spd(h.ranks[r].piece.A_II), C=h.complement_share(r), B=B, what=what)
    for rounded in (False, True):
        t_r, z = h.apply_rank(r, B, rounded)
        out[rounded] = (t_r, z, h.others_share(r, B, rounded))
    return out


def teardown_module(module):
    _rank.cache_clear()
    _case.cache_clear()


class DeviceRank:
    """Rank ``r`` of case ``name`` on the device, set up the way `distributed.DistributedTDGL` does it, with the callback
    transport: the all-reduce callback adds ``pending`` (the other ranks' terms of the column in flight) while armed."""

    def __init__(self, name, r, fp32_storage, monkeypatch):
        from tdgl_amd import SolverOptions
        from tdgl_amd.distributed import prepare_payloads_for
        from tdgl_amd.hipcore import TDGLContext
        from tdgl_amd.schur_dd import build_piece

        for var in ("TDGL_PD_SYM", "TDGL_UP_PARTS", "TDGL_PD_TWO_PASS"):
            monkeypatch.delenv(var, raising=False)
        self.h, self.kappa = _case(name)
        h = self.h
        self.r, self.m = r, h.ranks[r]
        blocks, lists = M.CASES[name][3:5]
        pay = prepare_payloads_for(h.mesh, h.world, [r], np.zeros(len(h.mesh.edge_mesh.edges)), schur=True)[0]
        self.lp = lp = pay["lp"]
        assert np.array_equal(lp.local_to_global, self.m.lp.local_to_global) and pay["schur"]["n_gamma"] == h.n_gamma
        with M.prescribed_orders(lists):
            self.piece = piece = build_piece(lp, pay["schur"]["is_gamma"], pay["schur"]["gid"], pay["schur"]["n_gamma"], blocks=blocks)
        assert np.array_equal(piece.interior, self.m.piece.interior) and np.array_equal(piece.gamma_owned_gid, self.m.piece.gamma_owned_gid)
        assert all(np.array_equal(p, q) for p, q in zip(piece.ptrs, self.m.piece.ptrs))
        self.armed, self.pending, self.seen, self.unexpected = False, None, [], []
        opt = SolverOptions(solve_time=1.0)
        self.ctx = ctx = TDGLContext(lp.mesh, n_owned=lp.n_own)
        try:
            ctx.set_halo_plan(lp)
            if pay.get("deep") is not None:
                ctx.set_deep_halo_plan(pay["deep"])
            ctx.comm_init_callbacks(self._halo, self._allreduce)
            if pay.get("deep") is not None:
                ctx.set_poisson_options(rtol=opt.pcg_rtol, max_iter=opt.pcg_max_iter, nu=opt.amg_smoothing_sweeps)
                ctx.set_hierarchy_deep(pay["deep"], pay["coarse"])
            else:
                ctx.set_hierarchy_sliced(pay["level0"], pay["coarse"], lp)
            ctx.set_poisson_options(rtol=opt.pcg_rtol, max_iter=opt.pcg_max_iter, nu=opt.amg_smoothing_sweeps)
            others = sum(h.schur_share(s) for s in range(h.world) if s != r)
            # C as the library returned it.  (``A_GG_owned - argument`` of the sum below is C only to a rounding of
            # A_GG's entries, and A_GG_owned -- the OWNED rows -- is not symmetric: no bit-for-bit statement survives it.)
            complement = ctx._lib.tdgl_poisson_schur_complement

            def spy(c, out):
                status = complement(c, out)
                self.C_dev = np.ctypeslib.as_array(out, shape=(h.n_gamma, h.n_gamma)).copy()
                return status

            monkeypatch.setattr(ctx._lib, "tdgl_poisson_schur_complement", spy)

            def allreduce_sum(a):
                a = np.asarray(a, dtype=float)
                assert a.shape == (h.n_gamma, h.n_gamma) and not hasattr(self, "S_dev")  # the ONE sum of the set-up
                self.S_dev = a.copy()
                return a + others

            self.on = ctx.build_schur_precond(piece, allreduce_sum, lambda a: a, choice=1, fp32_storage=fp32_storage)
        except BaseException:
            ctx.close()
            raise

    def _halo(self, send, send_off, recv, recv_off, ranks):
        recv[:] = 0.0
        if self.armed:
            self.unexpected.append(("halo", len(recv)))

    def _allreduce(self, buf, op):
        if not self.armed:
            return
        if op == 0 and len(buf) == self.h.n_gamma and self.pending is not None:
            self.seen.append(buf.copy())
            buf += self.pending
            self.pending = None
        else:
            self.unexpected.append(("allreduce", op, len(buf)))

    def apply(self, r_own, others):
        """One application with ``others`` added in the all-reduce: ``(t_r as the device formed it, z_own, r . z)``."""
        self.seen, self.pending, self.armed = [], np.array(others, dtype=float), True
        try:
            z, rz = self.ctx.precond_schur_apply(r_own)
        finally:
            self.armed = False
        assert not self.unexpected and len(self.seen) == 1 and self.pending is None, (self.unexpected, len(self.seen))
        return self.seen[0], z, rz


RUNS = [("a", 0, True), ("a", 1, True), ("a", 2, True), ("a", 1, False), ("b", 1, True), ("b", 2, True), ("b", 2, False),
        ("c", 1, True), ("d", 0, True), ("d", 1, True)]


@pytest.mark.parametrize("name, r, fp32_storage", RUNS)
def test_one_rank_of_the_dissection_matches_the_float64_model(name, r, fp32_storage, monkeypatch):
    h, kappa = _case(name)
    _, _, world, _, lists, levels, n_gamma, ranks = M.CASES[name]
    # the shape facts the case was chosen for
    d = h.describe(r)
    owned, touched = ranks[r]
    assert h.world == world and h.n_gamma == n_gamma and n_gamma % 16 != 0 and n_gamma % 64 != 0
    assert d["levels"] == levels and d["owned_interface"] == owned and (touched is None or d["touched_interface"] == touched), d
    assert d["touched_interface"] >= 2 and (owned == 0 or d["touched_interface"] >= owned)
    if lists is not None:
        assert d["part_sizes"][0] == sorted(lists[0]) and d["top_separator"] == (475, 562)[r], d
    model = _rank(name, r)
    B, what, kappa_I = model["B"], model["what"], model["kappa_I"]
    assert "another rank's interior" in what and ("interface, owned" in what) == (owned > 0)
    foreign = np.setdiff1d(h.ranks[r].touched, h.ranks[r].piece.gamma_owned_gid)
    assert ("interface, touched and not owned" in what) == (len(foreign) > 0) and (len(foreign) > 0) == ((name, r) not in (("a", 0), ("d", 0)))
    dev = DeviceRank(name, r, fp32_storage, monkeypatch)
    ctx, m = dev.ctx, dev.m
    try:
        assert dev.on and ctx.precond_direct["storage"] == ("fp32" if fp32_storage else "fp64"), ctx.setup_times
        assert ctx.precond_direct["levels"] == levels and ctx.precond_direct["interface_owned"] == owned
        n_own = m.lp.n_own

        # 1. the interface complement
        C_dev, C = dev.C_dev, model["C"]
        outside = np.ones(C.shape, dtype=bool)
        outside[np.ix_(m.touched, m.touched)] = False
        err_C = np.abs(C_dev - C).max()
        print(f"{name} rank {r}: kappa_I {kappa_I:.4g}, max |C_dev - C| / max |C| = {err_C / np.abs(C).max():.3g} "
              f"(8 kappa_I u = {D.C_TOL * kappa_I * D.U:.3g})")
        assert np.array_equal(dev.S_dev, dev.piece.A_GG_owned.toarray() - C_dev)  # (what went into the sum)
        assert np.array_equal(C_dev, C_dev.T)
        assert np.all(C_dev[outside] == 0.0) and np.all(C[outside] == 0.0)
        assert np.all(np.abs(C_dev - C) <= D.C_TOL * kappa_I * D.U * np.abs(C).max())

        # 6. (before) the CG's state
        rhs = np.random.default_rng(11).standard_normal(ctx.n)
        before = ctx.poisson_solve(rhs)
        gram, stats = ctx.guess_gram(), ctx.precond_direct_stats()
        with pytest.raises(RuntimeError, match="single-GPU contexts only"):
            ctx.precond_apply(np.zeros(ctx.n))

        t_model, z_model, others = model[bool(fp32_storage)]
        z_exact = model[False][1]
        s = M.storage_error(model[True][1], z_exact)
        floor = D.C_TOL * kappa * D.U
        k = B.shape[1]
        d_z, d_t = np.empty(k), np.empty(k)
        for j in range(k):
            r_own = B[m.own, j]
            c0 = ctx.comm_stats()
            t_dev, z, rz = dev.apply(r_own, others[:, j])
            c1 = ctx.comm_stats()
            # 5. one all-reduce of n_gamma doubles, no halo
            assert (c1["allreduces"] - c0["allreduces"], c1["allreduce_bytes"] - c0["allreduce_bytes"]) == (1, 8 * n_gamma)
            assert (c1["halos"], c1["halo_bytes"]) == (c0["halos"], c0["halo_bytes"])
            assert t_dev.shape == (n_gamma,) and z.shape == (n_own,)
            # 4. r . z
            assert abs(rz - r_own @ z) <= n_own * D.U * np.abs(r_own * z).sum(), (j, rz, r_own @ z)
            d_z[j] = np.abs(z - z_model[:, j]).max() / np.abs(z_model[:, j]).max()
            d_t[j] = np.abs(t_dev - t_model[:, j]).max() / np.abs(t_model[:, j]).max()
            if j == k - 1:  # 6. a second identical application: the same bits
                t2, z2, rz2 = dev.apply(r_own, others[:, j])
                assert np.array_equal(t2, t_dev) and np.array_equal(z2, z) and rz2 == rz
        worst = int(np.argmax(d_z / s))
        print(f"{name} rank {r} {'fp32' if fp32_storage else 'fp64'}: kappa {kappa:.4g}, 8 kappa u {floor:.3g}, {k} columns, "
              f"s {s.min():.3g} .. {s.max():.3g}, d {d_z.max():.3g}, largest d / s = {(d_z / s).max():.3g} (column {worst}: "
              f"{what[worst]}; d = {d_z[worst]:.3g}), random columns {(d_z / s)[-4:].max():.3g}; t_r: {d_t.max():.3g}")
        assert np.all(s > 0.0)
        if fp32_storage:  # 3. (and the rank's term of the sum in the same way: on a rank that owns no interface site a
            # constant added to it would not show in z, S^+ annihilates the constants)
            assert F <= 1.0
            assert np.all(d_z <= np.maximum(F * s, floor)), (worst, what[worst], d_z[worst], s[worst])
            s_t = M.storage_error(model[True][0], model[False][0])
            assert np.all(d_t <= np.maximum(F * s_t, D.C_TOL * kappa_I * D.U)), (int(np.argmax(d_t)), d_t.max())
        else:  # 2.
            assert np.all(d_t <= D.C_TOL * kappa_I * D.U), (int(np.argmax(d_t)), d_t.max())
            assert np.all(d_z <= floor), (int(np.argmax(d_z)), what[int(np.argmax(d_z))], d_z.max())

        # 5. nothing in, nothing added: nothing out
        t0, z0, rz0 = dev.apply(np.zeros(n_own), np.zeros(n_gamma))
        assert not t0.any() and not z0.any() and rz0 == 0.0

        # 6. (after)
        assert np.array_equal(ctx.guess_gram(), gram) and ctx.precond_direct_stats() == stats
        after = ctx.poisson_solve(rhs)
        assert before[1] == after[1] and np.array_equal(before[0], after[0]) and before[2] == after[2]
    finally:
        ctx.close()


def test_schur_apply_is_refused_where_the_dissection_is_not_the_preconditioner(substructured_solve):
    from tdgl_amd.hipcore import TDGLContext

    h, _ = _case("c")
    # a rank's context before `build_schur_precond`
    lp = h.ranks[1].lp
    ctx = TDGLContext(lp.mesh, n_owned=lp.n_own)
    try:
        with pytest.raises(RuntimeError, match="not the rank-level dissection"):
            ctx.precond_schur_apply(np.zeros(lp.n_own))
        with pytest.raises(ValueError, match="owned sites"):
            ctx.precond_schur_apply(np.zeros(lp.n_loc + 1))
    finally:
        ctx.close()
    # a single-GPU context, without factors and with the factors as the mu solver (the factors as the single-GPU
    # preconditioner: tests/test_hip_direct.py, next to the refusals of `tdgl_poisson_schur_begin`)
    ctx = TDGLContext(h.mesh)
    try:
        with pytest.raises(RuntimeError, match="not the rank-level dissection"):
            ctx.precond_schur_apply(np.zeros(h.n))
        ctx.build_poisson(rtol=1e-10)
        assert ctx.dense_direct and ctx.substructure, ctx.setup_times
        with pytest.raises(RuntimeError, match="not the rank-level dissection"):
            ctx.precond_schur_apply(np.zeros(h.n))
    finally:
        ctx.close()
