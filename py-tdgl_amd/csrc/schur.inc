// Rank-level nested dissection: the CG's second preconditioner in one-process-per-GPU mode.  Included by tdgl_hip.hip
// (behind dense.inc).  Host side and the mathematics: tdgl_amd/schur_dd.py; reference counterpart: the one sparse LU of
// tdgl/finite_volume/operators.py:305-308 applied at tdgl/solver/solver.py:516.
//
// Gamma = a vertex cover of the edges between ranks.  Every rank holds the explicit multi-level factors of ITS interior
// block A_II (the machinery of dense.inc on a vector of n_local entries; positive definite, so the top separator
// carries a plain inverse and no gauge), its coupling blocks A_GI / A_IG, and -- like every other rank -- the pseudo-
// inverse of the interface complement S = A_GG - sum_r A_GI_r A_II_r^-1 A_I_rG as symmetric fp32 tiles.  One application
//     y_I = A_II^-1 r_I                                  local: gather, the factors' launch sequence (factors.inc)
//     t   = r_G - sum_r A_GI_r y_I                       ONE all-reduce of |Gamma| doubles
//     x_G = S^+ t                                        replicated: the dense pair (factors.inc: launch_dense_sym)
//     x_I = y_I - A_II^-1 (A_IG x_G)                     local: a second pass of the factors
// is a direct solve with the exact factors; with fp32 storage it contracts the residual by ~1e-6, and the CG around it
// (pcg_solve: A p with the fp64 matrix, one exchange of z's ghosts, one sum of 3 x 1024 partials) needs one iteration
// from the projection guess.

namespace tdgl {

// rg[g] = r[owner_local[g]] where this rank owns Gamma site g, else 0
__global__ __launch_bounds__(BLOCK) void k_schur_owned_rhs(int64_t ng, const int32_t *__restrict__ owner_local, const double *__restrict__ r,
                                                           double *__restrict__ rg) {
    const int64_t g = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (g >= ng) return;
    const int32_t l = owner_local[g];
    rg[g] = l >= 0 ? r[l] : 0.0;
}

// z[map[i]] = y[i] - v[i] on the interior, z[go_local[k]] = xg[go_gid[k]] on the owned interface sites, and the partials of
// r . z over the owned rows on the kernel's own fixed grid
__global__ __launch_bounds__(BLOCK) void k_schur_scatter(int64_t nI, const int32_t *__restrict__ map, const double *__restrict__ y,
                                                         const double *__restrict__ v, int64_t ngo, const int32_t *__restrict__ go_local,
                                                         const int32_t *__restrict__ go_gid, const double *__restrict__ xg,
                                                         const double *__restrict__ r, double *__restrict__ z, double *__restrict__ rz_part) {
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < nI + ngo; i += (int64_t)gridDim.x * BLOCK) {
        int j;
        double val;
        if (i < nI) {
            j = map[i];
            val = y[i] - v[i];
        } else {
            j = go_local[i - nI];
            val = xg[go_gid[i - nI]];
        }
        z[j] = val;
        acc += r[j] * val;
    }
    const double t = block_sum(acc);
    if (threadIdx.x == 0) rz_part[blockIdx.x] = t;
}

// dense unit-column right-hand side: b = column j of A_IG = row j of A_GI, scattered into a zeroed vector (set = 1) or
// taken out again (set = 0)
__global__ __launch_bounds__(BLOCK) void k_schur_column(int32_t k0, int32_t k1, const int32_t *__restrict__ idx, const double *__restrict__ val,
                                                        int set, double *__restrict__ b) {
    const int k = k0 + blockIdx.x * BLOCK + threadIdx.x;
    if (k < k1) b[idx[k]] = set ? val[k] : 0.0;
}

}  // namespace tdgl

// Every check comes before the resident factors are touched: a refused description leaves them (and a working
// preconditioner) as they were.  On success a new object holds the interface; the interior's levels follow
// (tdgl_poisson_set_substructure / _inner / _coupling), then _complement and _finish.
extern "C" int tdgl_poisson_schur_begin(tdgl_ctx *ctx, const tdgl_schur_piece *pc) {
    CTX_GUARD(ctx);
    if (!pc || pc->n_interior < 2 || pc->n_gamma < 2 || !pc->interior || !pc->gi_indptr || !pc->ig_indptr ||
        (pc->n_gamma_owned > 0 && (!pc->gamma_owned_local || !pc->gamma_owned_gid)))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_schur_begin: incomplete description");
    if (ctx->levels.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_poisson_schur_begin: set the hierarchy first (its level-0 matrix is the CG's operator)");
    if (pc->n_interior + pc->n_gamma_owned != ctx->n_own)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_schur_begin: interior (%lld) + owned interface sites (%lld) must be the owned sites (%lld)",
                  (long long)pc->n_interior, (long long)pc->n_gamma_owned, (long long)ctx->n_own);
    const int64_t nI = pc->n_interior, ng = pc->n_gamma, ngo = pc->n_gamma_owned;
    std::vector<char> seen((size_t)ctx->n_own, 0);
    for (int64_t i = 0; i < nI; ++i) {
        const int32_t l = pc->interior[i];
        if (l < 0 || l >= ctx->n_own || seen[l]) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_schur_begin: interior is not a set of owned sites");
        seen[l] = 1;
    }
    std::vector<int32_t> owner((size_t)ng, -1);
    for (int64_t k = 0; k < ngo; ++k) {
        const int32_t l = pc->gamma_owned_local[k], g = pc->gamma_owned_gid[k];
        if (l < 0 || l >= ctx->n_own || seen[l] || g < 0 || g >= ng || owner[g] >= 0)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_schur_begin: the owned interface sites must complete the owned sites, each with its own position in Gamma");
        seen[l] = 1;
        owner[g] = l;
    }
    if (!offsets_ok(pc->gi_indptr, ng) || (pc->gi_indptr[ng] > 0 && (!pc->gi_indices || !pc->gi_data)))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_schur_begin: inconsistent A_GI");
    if (!offsets_ok(pc->ig_indptr, nI) || (pc->ig_indptr[nI] > 0 && (!pc->ig_indices || !pc->ig_data)))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_schur_begin: inconsistent A_IG");
    for (int64_t k = 0; k < pc->gi_indptr[ng]; ++k)
        if (pc->gi_indices[k] < 0 || pc->gi_indices[k] >= nI) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_schur_begin: A_GI column out of range");
    for (int64_t k = 0; k < pc->ig_indptr[nI]; ++k)
        if (pc->ig_indices[k] < 0 || pc->ig_indices[k] >= ng) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_schur_begin: A_IG column out of range");
    // `interior` and `gamma_owned_local` are uploaded as device indices: right only where the context's order is the
    // caller's (n_owned < n_sites implies it; a single-process context may carry a site permutation)
    for (int64_t i = 0; i < ctx->n; ++i)
        if (ctx->perm[i] != (int32_t)i)
            TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_poisson_schur_begin: this context has a site permutation; the piece's local sites are device indices (create the context without site_perm)");
    auto f = std::make_unique<DirectFactors>();
    HIP_TRY(ctx, f->map.upload(std::vector<int32_t>(pc->interior, pc->interior + nI)));
    HIP_TRY(ctx, f->owner_local.upload(owner));
    HIP_TRY(ctx, f->go_local.upload(ngo > 0 ? std::vector<int32_t>(pc->gamma_owned_local, pc->gamma_owned_local + ngo) : std::vector<int32_t>(1, 0)));
    HIP_TRY(ctx, f->go_gid.upload(ngo > 0 ? std::vector<int32_t>(pc->gamma_owned_gid, pc->gamma_owned_gid + ngo) : std::vector<int32_t>(1, 0)));
    TDGL_TRY(upload_csr(ctx, ng, nI, pc->gi_indptr, pc->gi_indices, pc->gi_data, f->GI));
    TDGL_TRY(upload_csr(ctx, nI, ng, pc->ig_indptr, pc->ig_indices, pc->ig_data, f->IG));
    HIP_TRY(ctx, f->bp.alloc((size_t)nI));
    HIP_TRY(ctx, f->xp.alloc((size_t)nI));
    HIP_TRY(ctx, f->z.alloc((size_t)ctx->n_pad));
    for (auto *b : {&f->t, &f->rg, &f->xg}) HIP_TRY(ctx, b->alloc((size_t)ng));
    for (auto *b : {&f->y, &f->v, &f->c}) HIP_TRY(ctx, b->alloc((size_t)nI));
    f->ng = ng;
    f->ngo = ngo;
    f->n_local = nI;
    f->stage = DirectFactors::SCHUR_BEGUN;
    ctx->direct = std::move(f);
    return TDGL_OK;
}

// between tdgl_poisson_schur_begin and _finish, with the interior's factors complete
static inline bool schur_factors_ready(const tdgl_ctx *ctx) {
    return ctx->direct && ctx->direct->n_local > 0 && ctx->direct->stage == DirectFactors::READY;
}

// C = A_GI A_II^-1 A_IG restricted to the interface sites this rank's interior touches, column by column with the
// resident (still fp64) factors: out [n_gamma, n_gamma] row major, zero outside the touched block
extern "C" int tdgl_poisson_schur_complement(tdgl_ctx *ctx, double *out) {
    CTX_GUARD(ctx);
    if (!out) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_schur_complement: null output");
    if (!schur_factors_ready(ctx))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_poisson_schur_complement: between tdgl_poisson_schur_begin and _finish, with the interior's factors described");
    DirectFactors &f = *ctx->direct;
    const int64_t ng = f.ng, nI = f.n_local;
    std::vector<int32_t> gp((size_t)ng + 1);
    HIP_TRY(ctx, hipMemcpy(gp.data(), f.GI.indptr.p, gp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> touched;
    for (int64_t g = 0; g < ng; ++g)
        if (gp[g + 1] > gp[g]) touched.push_back(g);
    DevBuf<double> cols;  // [touched, ng]: one result column (a row of the symmetric C) per touched site
    HIP_TRY(ctx, cols.alloc(std::max<size_t>(1, touched.size() * (size_t)ng)));
    HIP_TRY(ctx, hipMemsetAsync(f.bp.p, 0, nI * sizeof(double), ctx->stream));
    for (size_t k = 0; k < touched.size(); ++k) {
        const int64_t g = touched[k];
        const int cnt = gp[g + 1] - gp[g];
        hipLaunchKernelGGL(k_schur_column, dim3(grid_for(cnt)), dim3(BLOCK), 0, ctx->stream, gp[g], gp[g + 1], (const int32_t *)f.GI.indices.p,
                           (const double *)f.GI.data.p, 1, f.bp.p);
        (void)direct_solve_launch(ctx, f.bp.p, f.y.p, false, nullptr, nullptr);
        launch_csr<8, C_AX, 4>(ctx, f.GI, f.y.p, nullptr, nullptr, 0.0, 0.0, nullptr, cols.p + k * (size_t)ng);
        hipLaunchKernelGGL(k_schur_column, dim3(grid_for(cnt)), dim3(BLOCK), 0, ctx->stream, gp[g], gp[g + 1], (const int32_t *)f.GI.indices.p,
                           (const double *)f.GI.data.p, 0, f.bp.p);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<double> h(touched.size() * (size_t)ng);
    if (!h.empty()) HIP_TRY(ctx, hipMemcpy(h.data(), cols.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    memset(out, 0, (size_t)ng * (size_t)ng * sizeof(double));
    for (size_t k = 0; k < touched.size(); ++k)
        for (size_t k2 = 0; k2 < touched.size(); ++k2)  // (symmetrised: both orders were computed)
            out[touched[k] * ng + touched[k2]] = 0.5 * (h[k * (size_t)ng + touched[k2]] + h[k2 * (size_t)ng + touched[k]]);
    return TDGL_OK;
}

static int precond_schur_apply(tdgl_ctx *ctx, const double *r, double *z, double *rz_part) {
    const DirectFactors &f = *ctx->direct;
    const int64_t nI = f.n_local, ng = f.ng;
    launch_pd_gather(ctx, nI, f.map.p, r, f.bp.p);
    (void)direct_solve_launch(ctx, f.bp.p, f.y.p, false, nullptr, nullptr);
    hipLaunchKernelGGL(k_schur_owned_rhs, dim3(grid_for(ng)), dim3(BLOCK), 0, ctx->stream, ng, (const int32_t *)f.owner_local.p, r, f.rg.p);
    launch_csr<8, C_RESID, 4>(ctx, f.GI, f.y.p, f.rg.p, nullptr, 0.0, 0.0, nullptr, f.t.p);
    TDGL_TRY(comm_allreduce(ctx, f.t.p, ng, 0));  // THE collective of an application
    launch_dense_sym(ctx, f.S, (int)ng, (int)((ng + WAVE - 1) / WAVE), f.t.p, finish_product(f.xg.p));
    launch_csr<8, C_AX, 4>(ctx, f.IG, f.xg.p, nullptr, nullptr, 0.0, 0.0, nullptr, f.c.p);
    (void)direct_solve_launch(ctx, f.c.p, f.v.p, false, nullptr, nullptr);
    hipLaunchKernelGGL(k_schur_scatter, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, nI, (const int32_t *)f.map.p, (const double *)f.y.p,
                       (const double *)f.v.p, f.ngo, (const int32_t *)f.go_local.p, (const int32_t *)f.go_gid.p, (const double *)f.xg.p, r, z,
                       rz_part);
    return TDGL_OK;
}

// Per-kernel entry point (tests of the rank-level dissection): ONE application z = M r of this rank's share, COLLECTIVE
// like the application inside the CG -- every rank calls it at the same point, its one all-reduce of n_gamma doubles
// pairs with the other ranks'.  r and z [n_own] in the rank's local site order (ghosts are neither read nor written by
// an application); buffers of its own: the CG's vectors, partials and counters are not touched (the factors' own work
// vectors are: every application overwrites them).  *rz = k_schur_scatter's partials added up in index order.
extern "C" int tdgl_precond_schur_apply(tdgl_ctx *ctx, const double *r, double *z, double *rz) {
    CTX_GUARD(ctx);
    if (!r || !z || !rz) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_precond_schur_apply: null argument");
    if (!ctx->direct || ctx->direct->n_local == 0 || !precond_factors_available(ctx))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_precond_schur_apply: the preconditioner of this context is not the rank-level dissection (tdgl_poisson_schur_begin ... _finish)");
    TDGL_TRY(comm_ready(ctx));
    const size_t bytes = (size_t)ctx->n_own * sizeof(double);
    DevBuf<double> in, out, part;
    HIP_TRY(ctx, in.alloc(ctx->n_pad));
    HIP_TRY(ctx, out.alloc(ctx->n_pad));
    HIP_TRY(ctx, part.alloc((size_t)ctx->npart));
    HIP_TRY(ctx, hipMemcpyAsync(in.p, r, bytes, hipMemcpyHostToDevice, ctx->stream));
    TDGL_TRY(precond_schur_apply(ctx, in.p, out.p, part.p));
    HIP_TRY(ctx, hipGetLastError());
    std::vector<double> h((size_t)ctx->npart);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(z, out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double s = 0.0;
    for (double v : h) s += v;
    *rz = s;
    return TDGL_OK;
}

// S [n_gamma, n_gamma] row major: the interface complement summed over the ranks (the same array on every rank).  The
// interior's factors are converted in place (sub_factors_to_precond): a failure after the checks releases them.
extern "C" int tdgl_poisson_schur_finish(tdgl_ctx *ctx, const double *S, int32_t fp32_storage, double *t_apply_us, double *t_vcycle_us) {
    CTX_GUARD(ctx);
    if (!S) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_schur_finish: the interface complement is required");
    if (!schur_factors_ready(ctx) || sub_laid_out(*ctx->direct))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_poisson_schur_finish: tdgl_poisson_schur_begin and the interior's factors (every level, every coupling block) first");
    DirectFactors &f = *ctx->direct;
    const int64_t m = f.ng;
    // pseudo-inverse on the device (null space: the constants), symmetric tiles
    double s = 0.0;
    for (int64_t i = 0; i < m; ++i) s += S[i * m + i];
    s /= (double)m;
    if (!(s > 0.0) || !std::isfinite(s)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_schur_finish: the interface complement has a non-positive mean diagonal");
    const int64_t N = round_up(m, GB);
    DenseTiles D;
    {
        DevBuf<double> src, M;
        HIP_TRY(ctx, src.alloc((size_t)m * m, false));
        HIP_TRY(ctx, hipMemcpy(src.p, S, (size_t)m * m * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(ctx, M.alloc((size_t)N * N, false));
        hipLaunchKernelGGL(k_dense_from, dim3(grid_for(N * N)), dim3(BLOCK), 0, ctx->stream, m, N, s / (double)m, (const double *)src.p, M.p);
        TDGL_TRY(dense_sweep_pack(ctx, M, m, N, 1.0 / (s * (double)m), D));
    }
    if (fp32_storage) TDGL_TRY(dense_to_fp32(ctx, D));
    f.S = std::move(D);
    TDGL_TRY(sub_factors_to_precond(ctx, fp32_storage != 0, "tdgl_poisson_schur_finish"));
    ctx->choice.enable(false);
    ctx->pcg_epoch += 1;
    return precond_calibrate(ctx, t_apply_us, t_vcycle_us);
}

// the times the solver choice multiplies its predicted iterations with: agreed over the ranks by the host layer (the
// maximum), so that every rank takes the same decision in every solve
extern "C" int tdgl_poisson_set_precond_times(tdgl_ctx *ctx, double t_apply_us, double t_vcycle_us) {
    if (!ctx || !(t_apply_us > 0.0) || !(t_vcycle_us > 0.0)) return TDGL_ERR_ARG;
    ctx->pd_t_apply_us = t_apply_us;
    ctx->pd_t_vcycle_us = t_vcycle_us;
    return TDGL_OK;
}
