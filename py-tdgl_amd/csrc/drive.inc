// The host side of everything that moves with time: the applied vector potential A(t) (FieldDrive, the link setters and
// getters), the tabulated terminal currents mu_b(t) and the separable epsilon(r, t) (MuTable, EpsTable), and the one
// launcher of every kernel that follows a change of them.

// ---- the launchers: each kernel has its one launch site here; an argument is what differs between the callers ----------------
// (go / only_if: a device flag that skips the launch's work when 0 -- the run-ahead loop's "this attempt moves the field" and
// "the links moved"; nullptr: always)

// ceff = cvec + divergence(dadt); either may be null (tdgl_apply_divergence: the bare divergence into its own array)
static void launch_ceff(tdgl_ctx *ctx, const double *dadt, const double *cvec, double *ceff, const int32_t *go = nullptr) {
    hipLaunchKernelGGL(k_ceff, dim3(grid_for((int64_t)ctx->lap_pat.n_slices * WAVE)), dim3(BLOCK), 0, ctx->stream,
                       ctx->lap_pat.n_slices, ctx->lap_pat.n_rows, ctx->lap_pat.slice_off.p, ctx->lap_slot_edge.p,
                       ctx->lap_slot_w.p, ctx->e_inv_len.p, dadt, cvec, ceff, go);
}

static void refresh_ceff(tdgl_ctx *ctx) {
    launch_ceff(ctx, ctx->loop.field.has_dadt ? ctx->e_dAdt.p : (const double *)nullptr, ctx->cvec.p, ctx->ceff.p);
}

// link variables from e_A (+ A2: the induced potential of a screening solve), then the covariant-Laplacian values
static void launch_links(tdgl_ctx *ctx, const double *A2, const int32_t *only_if) {
    hipLaunchKernelGGL(k_link_variables, dim3(grid_for(ctx->m)), dim3(BLOCK), 0, ctx->stream, ctx->m, ctx->e_A.p, A2,
                       ctx->e_dirx.p, ctx->e_diry.p, ctx->e_U.p, only_if);
    hipLaunchKernelGGL(k_fill_laplacian, dim3(grid_for(ctx->lap_pat.n_slots)), dim3(BLOCK), 0, ctx->stream,
                       ctx->lap_pat.n_slots, ctx->lap_slot_edge.p, ctx->lap_slot_w.p, ctx->e_U.p, ctx->lap_vals.p, only_if);
}

// the per-workgroup "did A move" flags of k_dadt / k_field_links and their OR
static int ensure_link_flags(tdgl_ctx *ctx) {
    if (ctx->link_block_changed.n != 0) return TDGL_OK;
    HIP_TRY(ctx, ctx->link_block_changed.alloc(grid_for(ctx->m)));
    HIP_TRY(ctx, ctx->link_changed.alloc(1));
    return TDGL_OK;
}

static void launch_any_flag(tdgl_ctx *ctx, const int32_t *go = nullptr) {
    hipLaunchKernelGGL(k_any_flag, dim3(1), dim3(BLOCK), 0, ctx->stream, grid_for(ctx->m), (const int32_t *)ctx->link_block_changed.p,
                       ctx->link_changed.p, go);
}

// c = mu_boundary_laplacian @ mu_b, added into dst (nb > 0)
static void launch_boundary_term(tdgl_ctx *ctx, const double *mu_b, double *dst) {
    hipLaunchKernelGGL(k_boundary_term, dim3(grid_for(ctx->nb)), dim3(BLOCK), 0, ctx->stream, ctx->nb, ctx->b_s0.p, ctx->b_s1.p,
                       ctx->b_c0.p, ctx->b_c1.p, mu_b, dst);
}

static LoopGeom loop_geom(const FieldDrive &F) {
    LoopGeom g{};
    g.n_loops = F.n_loops, g.z_film = F.zfilm;
    for (int l = 0; l < F.n_loops; ++l) g.radius[l] = F.radius[l];
    return g;
}

// the one launch that forms A, dA/dt, A_prev <- A and the per-workgroup "did it move" of ctx->loop.field: from the values fv
// (ctl == nullptr, the host has decided) or from the run-ahead loop's controller
static void launch_field_links(tdgl_ctx *ctx, const FieldValues &fv, const StepCtl *ctl) {
    const FieldArrays &a = ctx->field;
    const auto kernel = ctx->loop.field.loops() ? k_field_links<true> : k_field_links<false>;
    hipLaunchKernelGGL(kernel, dim3(grid_for(ctx->m)), dim3(BLOCK), 0, ctx->stream, ctx->m, ctx->m_pad, fv, loop_geom(ctx->loop.field),
                       (const double *)a.bases.p, (const double *)a.a0.p, (const double *)a.centres.p, ctx->e_A.p, ctx->e_Aprev.p,
                       (const double *)ctx->e_dirx.p, (const double *)ctx->e_diry.p, (const double *)ctx->e_inv_len.p, ctx->e_dAdt.p,
                       ctx->link_block_changed.p, ctl);
}

// the run-ahead loop's step rule of the moving field, on the device: the values of this attempt into the controller
static void launch_ra_field_begin(tdgl_ctx *ctx) {
    const FieldArrays &fa = ctx->field;
    const double *tab = fa.tab.p;
    hipLaunchKernelGGL(k_ra_field_begin, dim3(1), dim3(64), 0, ctx->stream, ctx->d_ctl.p, (const FieldTerm *)fa.terms.p, tab, tab + fa.tab.n / 2,
                       (const FieldLoop *)fa.loops.p, (const double *)fa.loop_tab.p, (int)(fa.loop_tab.n / 5));
}

// terminal currents at the time of the run-ahead loop's attempt (update_mu_boundary, solver.py:325-345)
static void launch_ra_mu_table(tdgl_ctx *ctx) {
    const MuTable &T = ctx->mu_tab;
    hipLaunchKernelGGL(k_ra_mu_table, dim3(1), dim3(BLOCK), 0, ctx->stream, (int)ctx->nb, (int)ctx->n_b_sites,
                       (const int32_t *)ctx->d_b_sites.p, (const int32_t *)ctx->b_s0.p, (const int32_t *)ctx->b_s1.p,
                       (const double *)ctx->b_c0.p, (const double *)ctx->b_c1.p, ctx->b_mu.p, ctx->cvec.p, ctx->ceff.p, (int)T.t.size(),
                       (const double *)T.d_t.p, (const double *)T.d_dens.p, (const int32_t *)T.d_group.p, (const StepCtl *)ctx->d_ctl.p);
}

// epsilon(r, t) = factor(t) epsilon0(r) at the time of the run-ahead loop's attempt (update_epsilon, solver.py:364-381)
static void launch_ra_eps_table(tdgl_ctx *ctx) {
    const EpsTable &T = ctx->eps_tab;
    hipLaunchKernelGGL(k_ra_eps_table, dim3(grid_for(ctx->n_pad)), dim3(BLOCK), 0, ctx->stream, ctx->n_pad, (const double *)T.eps0.p,
                       ctx->eps.p, (int)T.t.size(), (const double *)T.d_t.p, (const double *)T.d_f.p, (const StepCtl *)ctx->d_ctl.p);
}

// epsilon = epsilon0 - the spots of S, into eps: at the values sv (ctl == nullptr, the host has decided) or at the time of the
// run-ahead loop's attempt.  xy, eps0: the owner's (a replica's lie in its ensemble's arrays)
static void launch_eps_spots(tdgl_ctx *ctx, const EpsSpots &S, const EpsSpotValues &sv, const double2 *xy, const double *eps0, double *eps,
                             const StepCtl *ctl) {
    hipLaunchKernelGGL(k_eps_spots, dim3(grid_for(ctx->n_pad)), dim3(BLOCK), 0, ctx->stream, ctx->n_pad, sv, S.tabs, (const double *)S.d_pool.p, xy,
                       eps0, eps, S.d_applied.p, ctl);
}

// ---- what the setters refuse (the tables are piecewise linear, evaluated inside tdgl_run by table_value, kernels.inc) ----------
static bool table_times_ok(const double *times, int32_t n) {
    for (int32_t k = 0; k < n; ++k)
        if (!std::isfinite(times[k]) || (k > 0 && !(times[k] > times[k - 1]))) return false;
    return true;
}

// what tdgl_set_link_table and tdgl_ensemble_set_link_table refuse
static int check_link_table(tdgl_ctx *ctx, const char *who, int32_t n_nodes, const double *times, const double *values) {
    if (n_nodes < 1 || !times || !values || !table_times_ok(times, n_nodes))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: bad table (times must increase strictly)", who);
    for (int32_t k = 0; k < n_nodes; ++k)
        if (!std::isfinite(values[k])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: non-finite factor", who);
    return TDGL_OK;
}

// what tdgl_set_mu_boundary_table and tdgl_ensemble_set_mu_boundary_table refuse (who: the entry point, for the message)
static int check_mu_table(tdgl_ctx *ctx, const char *who, int32_t n_nodes, const double *times, int32_t n_groups,
                          const int32_t *group_ptr, const int32_t *group_pos, const double *density) {
    if (n_nodes < 1 || n_groups < 1 || !times || !group_ptr || !group_pos || !density || !table_times_ok(times, n_nodes))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: bad table (times must increase strictly)", who);
    if (group_ptr[0] != 0) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: group_ptr must start at 0", who);
    for (int32_t g = 0; g < n_groups; ++g)
        if (group_ptr[g + 1] < group_ptr[g]) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: group_ptr decreases", who);
    for (int32_t k = 0; k < group_ptr[n_groups]; ++k)
        if (group_pos[k] < 0 || group_pos[k] >= ctx->nb)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: boundary position %d out of range", who, group_pos[k]);
    for (int64_t k = 0; k < (int64_t)n_groups * n_nodes; ++k)
        if (!std::isfinite(density[k])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: non-finite density", who);
    return TDGL_OK;
}

// ... and the two epsilon tables
static int check_eps_table(tdgl_ctx *ctx, const char *who, const double *epsilon0, int32_t n_nodes, const double *times, const double *factor) {
    if (!epsilon0) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: bad table (times must increase strictly)", who);
    return check_link_table(ctx, who, n_nodes, times, factor);
}

// a width the kernel can divide by: finite, > 0, and sigma^2 neither 0 nor subnormal (else a site at the centre would get 0 / 0)
static bool eps_sigma_ok(double s) {
    return std::isfinite(s) && s > 0.0 && s * s >= std::numeric_limits<double>::min();
}

// ... and the hot spots of tdgl_set_epsilon_spots and tdgl_ensemble_set_epsilon_spots.  With a >= 0 and epsilon0 <= 1 epsilon
// stays <= 1 at every time (solver.py:215), so nothing is checked per step
static int check_eps_spots(tdgl_ctx *ctx, const char *who, const double *sites, const double *eps0, int32_t n_spots, const int32_t *tab_off,
                           const double *times, const double *cx, const double *cy, const double *amp, const double *sigma) {
    if (n_spots < 1 || n_spots > EPS_SPOTS_MAX) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: n_spots must be in [0, %d]", who, EPS_SPOTS_MAX);
    if (!sites || !eps0 || !tab_off || !times || !cx || !cy || !amp || !sigma) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: null argument", who);
    for (int64_t i = 0; i < 2 * ctx->n; ++i)
        if (!std::isfinite(sites[i])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: sites: non-finite coordinate", who);
    for (int64_t i = 0; i < ctx->n; ++i)
        if (!(std::isfinite(eps0[i]) && eps0[i] <= 1.0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: eps0 must be finite and <= 1", who);
    if (tab_off[0] != 0) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: tab_off must start at 0", who);
    for (int32_t k = 0; k < n_spots; ++k) {
        const int32_t o = tab_off[k], nn = tab_off[k + 1] - o;
        if (nn < 1) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: spot %d has no nodes (tab_off)", who, k);
        if (!table_times_ok(times + o, nn)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: spot %d: tab_times must be finite and increase strictly", who, k);
        for (int32_t i = o; i < o + nn; ++i) {
            if (!std::isfinite(cx[i])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: spot %d: non-finite tab_cx", who, k);
            if (!std::isfinite(cy[i])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: spot %d: non-finite tab_cy", who, k);
            if (!(std::isfinite(amp[i]) && amp[i] >= 0.0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: spot %d: tab_amp must be finite and >= 0", who, k);
            if (!eps_sigma_ok(sigma[i])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: spot %d: tab_sigma must be finite and > 0, with a normal square", who, k);
        }
    }
    return TDGL_OK;
}

// what tdgl_set_link_terms and tdgl_ensemble_set_link_terms refuse: the rules of tdgl_set_link_ramp and check_link_table, term by term
static int check_link_terms(tdgl_ctx *ctx, const char *who, int32_t n_terms, const double *bases, const int32_t *kind, const double *ramp,
                            const int32_t *tab_off, const double *times, const double *values) {
    if (n_terms < 1 || n_terms > FIELD_TERMS_MAX) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: n_terms must be in [1, %d]", who, FIELD_TERMS_MAX);
    if (!bases || !kind) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: null bases or kinds", who);
    for (int32_t k = 0; k < n_terms; ++k) {
        if (kind[k] == TERM_RAMP) {
            if (!ramp) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: term %d is a ramp but there are no ramp parameters", who, k);
            const double *q = ramp + 4 * k;
            if (!(std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]) && std::isfinite(q[3])))
                TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: term %d: the ramp's parameters must be finite", who, k);
            if (!(q[1] > q[0])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: term %d: tmax must be > tmin", who, k);
        } else if (kind[k] == TERM_TABLE) {
            if (!tab_off || !times || !values || tab_off[k] < 0 || tab_off[k + 1] < tab_off[k])
                TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: term %d is a table but its nodes are missing", who, k);
            TDGL_TRY(check_link_table(ctx, who, tab_off[k + 1] - tab_off[k], times + tab_off[k], values + tab_off[k]));
        } else {
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: term %d: kind must be 1 (ramp) or 2 (table)", who, k);
        }
    }
    return TDGL_OK;
}

// ---- the applied vector potential ---------------------------------------------------------------------------------------------
// everything that follows new values in ctx->e_A: dA/dt (dynamic) or A_prev <- A (static), the
// rhs term of dA/dt, link variables, covariant-Laplacian values
// (dadt_done: the caller's own kernel has formed dA/dt, A_prev and the per-workgroup flags already -- k_field_links)
static int finish_links(tdgl_ctx *ctx, bool dynamic, double dt_prev, bool dadt_done = false) {
    const size_t bytes = 2 * ctx->m_pad * sizeof(double);
    const int32_t *only_if = nullptr;
    if (dynamic) {
        TDGL_TRY(ensure_link_flags(ctx));
        if (!dadt_done)
            hipLaunchKernelGGL(k_dadt, dim3(grid_for(ctx->m)), dim3(BLOCK), 0, ctx->stream, ctx->m, 1.0 / dt_prev,
                               ctx->e_A.p, ctx->e_Aprev.p, ctx->e_dirx.p, ctx->e_diry.p, ctx->e_inv_len.p, ctx->e_dAdt.p,
                               ctx->link_block_changed.p);
        launch_any_flag(ctx);
        // (with screening the links are rebuilt from A_applied + A_induced in every screening
        // iteration anyway, solver.py:670-673)
        only_if = ctx->link_changed.p;
        ctx->loop.field.has_dadt = true;
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->e_Aprev.p, ctx->e_A.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        ctx->loop.field.has_dadt = false;
    }
    refresh_ceff(ctx);
    launch_links(ctx, ctx->scr_enabled ? ctx->scr_Aind.p : (const double *)nullptr, only_if);
    HIP_TRY(ctx, hipGetLastError());
    ctx->have_links = true;
    ctx->lap_valid = false;
    ctx->currents.new_links();
    return TDGL_OK;
}

static int upload_edge_vectors(tdgl_ctx *ctx, const double *A, double *dst) {
    std::vector<double> tmp(2 * ctx->m_pad, 0.0);
    for (int64_t k = 0; k < ctx->m; ++k) {
        const int32_t e = ctx->edge_perm[k];
        tmp[2 * k] = A[2 * e];
        tmp[2 * k + 1] = A[2 * e + 1];
    }
    HIP_TRY(ctx, hipMemcpyAsync(dst, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // tmp goes out of scope
    return TDGL_OK;
}

static int set_links_impl(tdgl_ctx *ctx, const double *A, bool dynamic, double dt_prev) {
    CTX_GUARD(ctx);
    if (!A) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_link_exponents: null A");
    TDGL_TRY(upload_edge_vectors(ctx, A, ctx->e_A.p));
    ctx->loop.field.clear();
    TDGL_TRY(finish_links(ctx, dynamic, dt_prev));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

extern "C" int tdgl_set_link_exponents(tdgl_ctx *ctx, const double *A) {
    return set_links_impl(ctx, A, false, 0.0);
}

extern "C" int tdgl_update_link_exponents(tdgl_ctx *ctx, const double *A_new, double dt_prev) {
    if (ctx && !(dt_prev > 0.0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_link_exponents: dt_prev must be > 0");
    if (ctx && !ctx->have_links) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "call tdgl_set_link_exponents first");
    return set_links_impl(ctx, A_new, true, dt_prev);
}

// ---- the moving applied field (FieldDrive ctx->loop.field, its arrays ctx->field) without leaving the device ---------------
// ... from the values the host gives
static int field_links_at(tdgl_ctx *ctx, const double *scales, const double *lp, double inv_dt) {
    TDGL_TRY(ensure_link_flags(ctx));
    const FieldDrive &F = ctx->loop.field;
    FieldValues fv{};
    for (int k = 0; k < F.n_terms; ++k) fv.s[k] = scales[k];
    fv.inv_dt = inv_dt, fv.n_terms = F.n_terms;
    for (int l = 0; l < F.n_loops; ++l)
        for (int j = 0; j < 4; ++j) fv.lp[l][j] = lp[4 * l + j];
    launch_field_links(ctx, fv, nullptr);
    return TDGL_OK;
}

// A = A_prev = the field at the values in force, dA/dt = 0 (the links kernel against A_prev = 0 with 1 / dt = 0), the links,
// the Laplacian values
static int restart_field(tdgl_ctx *ctx) {
    HIP_TRY(ctx, hipMemsetAsync(ctx->e_Aprev.p, 0, 2 * (size_t)ctx->m_pad * sizeof(double), ctx->stream));
    TDGL_TRY(field_links_at(ctx, ctx->loop.field.scale, &ctx->loop.field.loop_par[0][0], 0.0));
    TDGL_TRY(finish_links(ctx, false, 0.0));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

// the descriptors and table pool of the drive's terms as the begin kernel reads them
static int upload_term_tables(tdgl_ctx *ctx, const FieldDrive &F, FieldArrays &a) {
    std::vector<FieldTerm> desc(FIELD_TERMS_MAX);
    std::vector<double> tt, tv;
    F.describe(desc.data(), tt, tv);
    if (tt.empty()) tt.push_back(0.0), tv.push_back(0.0);  // (never read: no term is a table)
    tt.insert(tt.end(), tv.begin(), tv.end());
    HIP_TRY(ctx, a.terms.upload(desc));
    HIP_TRY(ctx, a.tab.upload(tt));
    return TDGL_OK;
}

// the step of the loop with one synchronisation per step: the step rule, then the links where something moves
static int update_field(tdgl_ctx *ctx, const double *scales, const double *lp, double dt_prev) {
    if (!ctx->loop.field.step(scales, lp)) return TDGL_OK;  // (A and dA/dt = 0 are already in place)
    TDGL_TRY(field_links_at(ctx, scales, lp, 1.0 / dt_prev));
    return finish_links(ctx, true, dt_prev, true);
}

// A(t) = scale(t) * A_base: the single product, its factor the caller's until a ramp or a table is switched on
extern "C" int tdgl_set_link_exponents_base(tdgl_ctx *ctx, const double *A_base, double scale) {
    CTX_GUARD(ctx);
    if (!A_base) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_link_exponents_base: null A_base");
    FieldArrays next;
    HIP_TRY(ctx, next.bases.alloc(2 * ctx->m_pad));
    TDGL_TRY(upload_edge_vectors(ctx, A_base, next.bases.p));
    ctx->field.take(next);
    ctx->loop.field.set_product(scale);
    return restart_field(ctx);
}

extern "C" int tdgl_update_link_scale(tdgl_ctx *ctx, double scale, double dt_prev) {
    CTX_GUARD(ctx);
    if (!ctx->loop.field.product()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "call tdgl_set_link_exponents_base first");
    if (!(dt_prev > 0.0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_link_scale: dt_prev must be > 0");
    TDGL_TRY(update_field(ctx, &scale, nullptr, dt_prev));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

extern "C" int tdgl_set_link_ramp(tdgl_ctx *ctx, int32_t on, double tmin, double tmax, double initial, double final_) {
    CTX_GUARD(ctx);
    FieldDrive &F = ctx->loop.field;
    if (on && !F.product()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "call tdgl_set_link_exponents_base first");
    if (on && !(tmax > tmin)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_link_ramp: tmax must be > tmin");
    if (!F.product()) return TDGL_OK;  // (off, and there is no product whose factor could be the caller's again)
    const double q[4] = {tmin, tmax, initial, final_};
    FieldDrive next = F;
    next.set_product_source(on ? TERM_RAMP : TERM_HOST, q, nullptr, nullptr, 0);
    if (on) TDGL_TRY(upload_term_tables(ctx, next, ctx->field));
    F = next;
    return TDGL_OK;
}

// A(t) = table(t) A_base: the factor as a piecewise-linear table (constant outside its nodes) that tdgl_run evaluates itself,
// in the place of the ramp -- a table and a ramp exclude each other, the later call wins
extern "C" int tdgl_set_link_table(tdgl_ctx *ctx, int32_t n_nodes, const double *times, const double *values) {
    CTX_GUARD(ctx);
    FieldDrive &F = ctx->loop.field;
    if (n_nodes == 0) {  // off (a ramp stays)
        if (F.product() && F.term[0].kind == TERM_TABLE) F.set_product_source(TERM_HOST, nullptr, nullptr, nullptr, 0);
        return TDGL_OK;
    }
    if (!F.product()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "call tdgl_set_link_exponents_base first");
    TDGL_TRY(check_link_table(ctx, "tdgl_set_link_table", n_nodes, times, values));
    FieldDrive next = F;
    next.set_product_source(TERM_TABLE, nullptr, times, values, n_nodes);
    TDGL_TRY(upload_term_tables(ctx, next, ctx->field));
    F = next;
    return TDGL_OK;
}

// A(t) = A_0 + f_1(t) A_1 + ... + f_K(t) A_K
extern "C" int tdgl_set_link_terms(tdgl_ctx *ctx, const double *A0, int32_t n_terms, const double *bases, const int32_t *kind,
                                   const double *ramp, const int32_t *tab_off, const double *tab_times, const double *tab_values) {
    CTX_GUARD(ctx);
    TDGL_TRY(check_link_terms(ctx, "tdgl_set_link_terms", n_terms, bases, kind, ramp, tab_off, tab_times, tab_values));
    // (nothing of the state in force has been touched so far; the device's copies are complete before the loop hears of them)
    const size_t slot = 2 * (size_t)ctx->m_pad;
    FieldArrays next;
    HIP_TRY(ctx, next.bases.alloc((size_t)n_terms * slot));
    for (int32_t k = 0; k < n_terms; ++k) TDGL_TRY(upload_edge_vectors(ctx, bases + (size_t)k * 2 * ctx->m, next.bases.p + (size_t)k * slot));
    if (A0) {
        HIP_TRY(ctx, next.a0.alloc(slot));
        TDGL_TRY(upload_edge_vectors(ctx, A0, next.a0.p));
    }
    FieldDrive drive;
    drive.set_terms(n_terms, A0 != nullptr, kind, ramp, tab_off, tab_times, tab_values);
    TDGL_TRY(upload_term_tables(ctx, drive, next));
    ctx->field.take(next);
    ctx->loop.field = drive;
    return restart_field(ctx);
}

extern "C" int tdgl_update_link_terms(tdgl_ctx *ctx, const double *scales, double dt_prev) {
    CTX_GUARD(ctx);
    const FieldDrive &F = ctx->loop.field;
    if (!F.sum()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "call tdgl_set_link_terms first");
    if (F.loops()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "moving loops are set: tdgl_update_link_loops moves the whole sum");
    if (!scales) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_link_terms: null scales");
    for (int k = 0; k < F.n_terms; ++k)
        if (!std::isfinite(scales[k])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_link_terms: non-finite factor");
    if (!(dt_prev > 0.0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_link_terms: dt_prev must be > 0");
    TDGL_TRY(update_field(ctx, scales, nullptr, dt_prev));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

// ... plus moving current loops: A(t) = [that] + sum_l I_l(t) Aloop(r_e - c_l(t); a_l), on a sum or on a static A (which
// becomes the drive's A_0)
extern "C" int tdgl_set_link_loops(tdgl_ctx *ctx, int32_t n_loops, const double *edge_centres, double z_film, const double *radius,
                                   const int32_t *tab_off, const double *tab_times, const double *tab_cx, const double *tab_cy,
                                   const double *tab_cz, const double *tab_current) {
    CTX_GUARD(ctx);
    const char *who = "tdgl_set_link_loops";
    FieldDrive &F = ctx->loop.field;
    if (n_loops == 0) {  // the loops go; what they were added to stays, at the values in force
        if (!F.loops()) return TDGL_OK;
        F.set_loops(0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        TDGL_TRY(restart_field(ctx));
        if (!F.sum()) {  // (they stood on a static A: static links again)
            FieldArrays none;
            ctx->field.take(none);
            F.clear();
        }
        return TDGL_OK;
    }
    // everything is checked before anything in force is touched
    if (n_loops < 1 || n_loops > FIELD_LOOPS_MAX) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: n_loops must be in [0, %d]", who, FIELD_LOOPS_MAX);
    if (!ctx->have_links) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "%s: call tdgl_set_link_exponents or tdgl_set_link_terms first", who);
    if (F.product() && F.moves)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: a single ramped or tabulated product is in force; loops go with a static field or with tdgl_set_link_terms", who);
    if (!edge_centres || !radius || !tab_off || !tab_times || !tab_cx || !tab_cy || !tab_cz || !tab_current)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: null argument", who);
    if (!std::isfinite(z_film)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: z_film must be finite", who);
    for (int64_t i = 0; i < 2 * ctx->m; ++i)
        if (!std::isfinite(edge_centres[i])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: non-finite edge centre", who);
    if (tab_off[0] != 0) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: tab_off must start at 0", who);
    for (int32_t l = 0; l < n_loops; ++l) {
        if (!(std::isfinite(radius[l]) && radius[l] > 0.0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: loop %d: the radius must be finite and > 0", who, l);
        const int32_t n = tab_off[l + 1] - tab_off[l];
        if (n < 1) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: loop %d has no nodes", who, l);
        const double *tabs[4] = {tab_cx, tab_cy, tab_cz, tab_current};
        for (int j = 0; j < 4; ++j) TDGL_TRY(check_link_table(ctx, who, n, tab_times + tab_off[l], tabs[j] + tab_off[l]));
        // the loop's plane stays on one side of the film: between two nodes on the same side the interpolant cannot reach it,
        // so m < 1 strictly at every time
        const double side = tab_cz[tab_off[l]] - z_film;
        for (int32_t i = tab_off[l]; i < tab_off[l + 1]; ++i)
            if (!((tab_cz[i] - z_film) * side > 0.0))
                TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: loop %d: the loop's plane must differ from the film's (cz != z_film, on one side of it) at every node", who, l);
    }
    const size_t slot = 2 * (size_t)ctx->m_pad;
    FieldArrays next;
    HIP_TRY(ctx, next.centres.alloc(slot));
    TDGL_TRY(upload_edge_vectors(ctx, edge_centres, next.centres.p));
    const bool fresh = !F.sum() && !F.loops();  // on a static A: that A becomes A_0, with no products
    if (fresh) {
        HIP_TRY(ctx, next.a0.alloc(slot));
        HIP_TRY(ctx, hipMemcpyAsync(next.a0.p, ctx->e_A.p, slot * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    const int32_t T = tab_off[n_loops];
    std::vector<FieldLoop> desc((size_t)n_loops);
    for (int32_t l = 0; l < n_loops; ++l) desc[l] = FieldLoop{tab_off[l], tab_off[l + 1] - tab_off[l], radius[l]};
    std::vector<double> pool(tab_times, tab_times + T);
    pool.insert(pool.end(), tab_cx, tab_cx + T);
    pool.insert(pool.end(), tab_cy, tab_cy + T);
    pool.insert(pool.end(), tab_cz, tab_cz + T);
    pool.insert(pool.end(), tab_current, tab_current + T);
    HIP_TRY(ctx, next.loops.upload(desc));
    HIP_TRY(ctx, next.loop_tab.upload(pool));
    if (fresh) TDGL_TRY(upload_term_tables(ctx, FieldDrive{}, next));  // (the begin kernel reads no term, but is handed valid pointers)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (fresh) {
        F.clear(), F.a0 = true;
        ctx->field.bases.release(), ctx->field.a0.take(next.a0), ctx->field.terms.take(next.terms), ctx->field.tab.take(next.tab);
    }
    ctx->field.centres.take(next.centres), ctx->field.loops.take(next.loops), ctx->field.loop_tab.take(next.loop_tab);
    F.set_loops(n_loops, z_film, radius, tab_off, tab_times, tab_cx, tab_cy, tab_cz, tab_current);
    return restart_field(ctx);
}

extern "C" int tdgl_update_link_loops(tdgl_ctx *ctx, const double *term_scales, const double *loop_params, double dt_prev) {
    CTX_GUARD(ctx);
    const FieldDrive &F = ctx->loop.field;
    if (!F.loops()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "call tdgl_set_link_loops first");
    if (!loop_params || (F.n_terms > 0 && !term_scales)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_link_loops: null argument");
    for (int k = 0; k < F.n_terms; ++k)
        if (!std::isfinite(term_scales[k])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_link_loops: non-finite factor");
    for (int l = 0; l < F.n_loops; ++l) {
        for (int j = 0; j < 4; ++j)
            if (!std::isfinite(loop_params[4 * l + j])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_link_loops: non-finite loop value");
        if (loop_params[4 * l + 2] == F.zfilm)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_link_loops: loop %d lies in the film's plane", l);
    }
    if (!(dt_prev > 0.0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_link_loops: dt_prev must be > 0");
    TDGL_TRY(update_field(ctx, term_scales, loop_params, dt_prev));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

extern "C" int tdgl_get_link_loop_params(tdgl_ctx *ctx, int32_t *n_loops, double *params) {
    if (!ctx || !n_loops || !params) return TDGL_ERR_ARG;
    *n_loops = ctx->loop.field.n_loops;
    for (int l = 0; l < *n_loops; ++l)
        for (int j = 0; j < 4; ++j) params[4 * l + j] = ctx->loop.field.loop_par[l][j];
    return TDGL_OK;
}

extern "C" int tdgl_get_link_exponents(tdgl_ctx *ctx, double *A) {
    CTX_GUARD(ctx);
    if (!A) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_get_link_exponents: null A");
    if (!ctx->have_links) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_get_link_exponents: no links are set");
    std::vector<double> tmp(2 * (size_t)ctx->m);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(tmp.data(), ctx->e_A.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < ctx->m; ++k) {
        const int32_t e = ctx->edge_perm[k];
        A[2 * e] = tmp[2 * k];
        A[2 * e + 1] = tmp[2 * k + 1];
    }
    return TDGL_OK;
}

extern "C" int tdgl_get_link_term_moves(tdgl_ctx *ctx, int64_t *moves) {
    if (!ctx || !moves) return TDGL_ERR_ARG;
    *moves = ctx->loop.field.sum() || ctx->loop.field.loops() ? ctx->loop.field.n_moves : 0;
    return TDGL_OK;
}

extern "C" int tdgl_get_link_term_scales(tdgl_ctx *ctx, int32_t *n_terms, double *scales) {
    if (!ctx || !n_terms || !scales) return TDGL_ERR_ARG;
    *n_terms = ctx->loop.field.sum() ? ctx->loop.field.n_terms : 0;
    for (int k = 0; k < *n_terms; ++k) scales[k] = ctx->loop.field.scale[k];
    return TDGL_OK;
}

extern "C" int tdgl_get_link_scale(tdgl_ctx *ctx, double *scale) {
    if (!ctx || !scale) return TDGL_ERR_ARG;
    *scale = ctx->loop.field.sum() ? 1.0 : ctx->loop.field.scale[0];  // (the single product's factor)
    return TDGL_OK;
}

extern "C" int tdgl_set_epsilon(tdgl_ctx *ctx, const double *epsilon) {
    CTX_GUARD(ctx);
    if (!epsilon) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_epsilon: null epsilon");
    TDGL_TRY(upload_sites(ctx, epsilon, ctx->eps));
    ctx->eps_tab.clear(), ctx->eps_spots.clear();  // (plain values, a table and spots exclude each other: the later call wins)
    ctx->have_eps = true;
    ctx->choice.reset();
    return TDGL_OK;
}

extern "C" int tdgl_get_epsilon(tdgl_ctx *ctx, double *epsilon) {
    CTX_GUARD(ctx);
    if (!epsilon) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_get_epsilon: null epsilon");
    if (!ctx->have_eps) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_get_epsilon: no epsilon is set");
    return download_sites(ctx, (const double *)ctx->eps.p, epsilon);
}

// mu_boundary -> boundary term of the Poisson right-hand side (everything queued on the stream)
static int apply_mu_boundary(tdgl_ctx *ctx, const double *mu_boundary) {
    HIP_TRY(ctx, hipMemsetAsync(ctx->cvec.p, 0, ctx->n_pad * sizeof(double), ctx->stream));
    if (ctx->nb > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->b_mu.p, mu_boundary, ctx->nb * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        launch_boundary_term(ctx, ctx->b_mu.p, ctx->cvec.p);
    }
    refresh_ceff(ctx);
    HIP_TRY(ctx, hipGetLastError());
    return TDGL_OK;
}

extern "C" int tdgl_set_mu_boundary(tdgl_ctx *ctx, const double *mu_boundary) {
    CTX_GUARD(ctx);
    if (ctx->nb > 0 && !mu_boundary) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_mu_boundary: null array");
    TDGL_TRY(apply_mu_boundary(ctx, mu_boundary));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mu_tab.applied(mu_boundary, ctx->nb);
    ctx->choice.reset();
    return TDGL_OK;
}

// the sites boundary edges touch, once (the table kernels rebuild the boundary term there)
static int ensure_boundary_sites(tdgl_ctx *ctx) {
    if (ctx->d_b_sites.n != 0) return TDGL_OK;
    std::vector<int32_t> s0((size_t)ctx->nb), s1((size_t)ctx->nb);
    HIP_TRY(ctx, hipMemcpy(s0.data(), ctx->b_s0.p, s0.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(s1.data(), ctx->b_s1.p, s1.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    s0.insert(s0.end(), s1.begin(), s1.end());
    std::sort(s0.begin(), s0.end());
    s0.erase(std::unique(s0.begin(), s0.end()), s0.end());
    HIP_TRY(ctx, ctx->d_b_sites.upload(s0));
    ctx->n_b_sites = (int32_t)s0.size();
    return TDGL_OK;
}

// ---- MuTable, EpsTable (tdgl_internal.h) ----------------------------------------------------------------------------------------
namespace tdgl {

void MuTable::clear() {
    t.clear(), dens.clear(), ptr.clear(), pos.clear(), last.clear(), host.clear();
    dev_synced = on_device = false;
}

void MuTable::set(int32_t n_nodes, const double *times, int32_t n_groups, const int32_t *group_ptr, const int32_t *group_pos,
                  const double *density, int64_t nb) {
    clear();
    t.assign(times, times + n_nodes);
    dens.assign(density, density + (size_t)n_groups * n_nodes);
    ptr.assign(group_ptr, group_ptr + n_groups + 1);
    pos.assign(group_pos, group_pos + group_ptr[n_groups]);
    last.assign(n_groups, 0.0);                   // solver.py:323: densities start at 0
    host.assign(std::max<int64_t>(nb, 1), 0.0);  // ... and mu_boundary at 0 (solver.py:289)
}

std::vector<int32_t> MuTable::groups(int64_t nb) const {
    std::vector<int32_t> group((size_t)nb, -1);
    for (size_t g = 0; g + 1 < ptr.size(); ++g)
        for (int32_t k = ptr[g]; k < ptr[g + 1]; ++k) group[(size_t)pos[k]] = (int32_t)g;
    return group;
}

int MuTable::to_device(tdgl_ctx *ctx) {
    HIP_TRY(ctx, d_group.upload(groups(ctx->nb)));
    HIP_TRY(ctx, d_t.upload(t));
    HIP_TRY(ctx, d_dens.upload(dens));
    on_device = true;
    return TDGL_OK;
}

// solver.py:341: a group's positions are rewritten only when its density changed
bool MuTable::step(double time) {
    const size_t nn = t.size();
    bool changed = false;
    for (size_t g = 0; g < last.size(); ++g) {
        const double d = table_value(t.data(), dens.data() + g * nn, (int)nn, time);
        if (d != last[g]) {
            last[g] = d;
            for (int32_t k = ptr[g]; k < ptr[g + 1]; ++k) host[pos[k]] = d;
            changed = true;
        }
    }
    return changed;
}

void MuTable::applied(const double *mu_boundary, int64_t nb) {
    if (on() && nb > 0) host.assign(mu_boundary, mu_boundary + nb);
    dev_synced = on();
}

// The positions no table covers keep the host's values: uploaded once, b_mu then stays resident (the table kernel rewrites
// the tabulated positions only).  The device is about to apply densities the host does not see, so the host's record of
// "what was applied last" is void from here on -- also if the batch fails: the next step of the loop with one
// synchronisation per step re-applies its own (apply_time_tables).
int MuTable::handed_to_device(tdgl_ctx *ctx) {
    if (!dev_synced) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->b_mu.p, host.data(), ctx->nb * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (pageable source: the host array may change after this call)
        dev_synced = true;
    }
    for (double &d : last) d = NAN;
    return TDGL_OK;
}

void EpsTable::clear() {
    t.clear(), f.clear();
    last = NAN, on_device = false;
}

void EpsTable::set(int32_t n_nodes, const double *times, const double *factor) {
    clear();
    t.assign(times, times + n_nodes);
    f.assign(factor, factor + n_nodes);
}

int EpsTable::to_device(tdgl_ctx *ctx) {
    HIP_TRY(ctx, d_t.upload(t));
    HIP_TRY(ctx, d_f.upload(f));
    on_device = true;
    return TDGL_OK;
}

void EpsTable::handed_to_device() { last = NAN; }

bool EpsTable::step(double time) {
    const double now = table_value(t.data(), f.data(), (int)t.size(), time);
    if (now == last) return false;
    last = now;
    return true;
}

void EpsSpots::forget() {
    for (auto &row : last)
        for (double &x : row) x = NAN;
}

void EpsSpots::clear() {
    n_spots = 0;
    pool.clear();
    tabs = EpsSpotTabs{};
    forget();
    xy.release(), eps0.release(), d_pool.release(), d_applied.release();
    on_device = false;
}

void EpsSpots::set(int32_t n, const int32_t *tab_off, const double *times, const double *cx, const double *cy, const double *amp,
                   const double *sigma) {
    n_spots = n;
    const int32_t T = tab_off[n];
    tabs = EpsSpotTabs{};
    tabs.n = n, tabs.T = T, tabs.base = 0;
    for (int32_t k = 0; k <= n; ++k) tabs.off[k] = tab_off[k];
    pool.assign(times, times + T);
    for (const double *q : {cx, cy, amp, sigma}) pool.insert(pool.end(), q, q + T);
    forget();
}

int EpsSpots::to_device(tdgl_ctx *ctx, const double *sites, const double *eps0_ref) {
    HIP_TRY(ctx, xy.alloc(ctx->n_pad));
    TDGL_TRY(upload_sites(ctx, reinterpret_cast<const double2 *>(sites), xy));
    HIP_TRY(ctx, eps0.alloc(ctx->n_pad));
    TDGL_TRY(upload_sites(ctx, eps0_ref, eps0));
    HIP_TRY(ctx, d_pool.upload(pool));
    HIP_TRY(ctx, d_applied.alloc(1));
    on_device = ctx->n_own == ctx->n;  // (the run-ahead loop is the single GPU's)
    return TDGL_OK;
}

EpsSpotValues EpsSpots::values_at(double time) const { return eps_spot_values_at(tabs, pool.data(), time); }

EpsSpotValues EpsSpots::values() const {
    EpsSpotValues sv{};
    sv.n = n_spots;
    for (int k = 0; k < n_spots; ++k)
        for (int j = 0; j < 4; ++j) sv.v[k][j] = last[k][j];
    return sv;
}

void EpsSpots::applied(const EpsSpotValues &sv) {
    for (int k = 0; k < n_spots; ++k)
        for (int j = 0; j < 4; ++j) last[k][j] = sv.v[k][j];
}

// like EpsTable::step: the pass is skipped when all 4 K values equal those applied last
bool EpsSpots::step(double time) {
    const EpsSpotValues now = values_at(time);
    bool changed = false;
    for (int k = 0; k < n_spots; ++k)
        for (int j = 0; j < 4; ++j) changed |= !(now.v[k][j] == last[k][j]);
    if (changed) applied(now);
    return changed;
}

}  // namespace tdgl

extern "C" int tdgl_set_mu_boundary_table(tdgl_ctx *ctx, int32_t n_nodes, const double *times, int32_t n_groups,
                                          const int32_t *group_ptr, const int32_t *group_pos, const double *density) {
    CTX_GUARD(ctx);
    ctx->mu_tab.clear();
    if (n_nodes == 0) return TDGL_OK;  // off
    TDGL_TRY(check_mu_table(ctx, "tdgl_set_mu_boundary_table", n_nodes, times, n_groups, group_ptr, group_pos, density));
    ctx->mu_tab.set(n_nodes, times, n_groups, group_ptr, group_pos, density, ctx->nb);
    // device copy for the run-ahead loop (k_ra_mu_table); single-GPU contexts only, like that loop
    if (ctx->nb > 0 && ctx->n_own == ctx->n) {
        TDGL_TRY(ensure_boundary_sites(ctx));
        TDGL_TRY(ctx->mu_tab.to_device(ctx));
    }
    return TDGL_OK;
}

extern "C" int tdgl_set_epsilon_table(tdgl_ctx *ctx, const double *epsilon0, int32_t n_nodes, const double *times,
                                      const double *factor) {
    CTX_GUARD(ctx);
    EpsTable &T = ctx->eps_tab;
    T.clear();
    if (n_nodes == 0) return TDGL_OK;  // off
    TDGL_TRY(check_eps_table(ctx, "tdgl_set_epsilon_table", epsilon0, n_nodes, times, factor));
    if (T.eps0.n == 0) HIP_TRY(ctx, T.eps0.alloc(ctx->n_pad));
    TDGL_TRY(upload_sites(ctx, epsilon0, T.eps0));
    T.set(n_nodes, times, factor);
    ctx->eps_spots.clear();  // (a table and spots exclude each other: the later call wins)
    if (ctx->n_own == ctx->n) TDGL_TRY(T.to_device(ctx));  // device copy for the run-ahead loop
    return TDGL_OK;
}

// epsilon(r, t) = epsilon0(r) - sum_k a_k(t) exp(-|r - c_k(t)|^2 / (2 sigma_k(t)^2)); sets epsilon = epsilon(r, 0)
extern "C" int tdgl_set_epsilon_spots(tdgl_ctx *ctx, const double *sites, const double *eps0, int32_t n_spots, const int32_t *tab_off,
                                      const double *tab_times, const double *tab_cx, const double *tab_cy, const double *tab_amp,
                                      const double *tab_sigma) {
    CTX_GUARD(ctx);
    if (n_spots == 0) {  // off: epsilon stays as last written
        ctx->eps_spots.clear();
        return TDGL_OK;
    }
    // everything is checked, and the device's copies are complete, before anything in force is touched
    TDGL_TRY(check_eps_spots(ctx, "tdgl_set_epsilon_spots", sites, eps0, n_spots, tab_off, tab_times, tab_cx, tab_cy, tab_amp, tab_sigma));
    EpsSpots next;
    next.set(n_spots, tab_off, tab_times, tab_cx, tab_cy, tab_amp, tab_sigma);
    TDGL_TRY(next.to_device(ctx, sites, eps0));
    (void)next.step(0.0);
    launch_eps_spots(ctx, next, next.values(), next.xy.p, next.eps0.p, ctx->eps.p, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // (only now: a failure above leaves the table or the spots that were in force)
    ctx->eps_tab.clear();
    ctx->eps_spots = std::move(next);
    ctx->have_eps = true;
    ctx->choice.reset();
    return TDGL_OK;
}

// applies cx, cy, a, sigma of every spot now: what the loop with one synchronisation per step does itself
extern "C" int tdgl_update_epsilon_spots(tdgl_ctx *ctx, const double *values) {
    CTX_GUARD(ctx);
    EpsSpots &S = ctx->eps_spots;
    if (!S.on()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "call tdgl_set_epsilon_spots first");
    if (!values) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_epsilon_spots: null values");
    EpsSpotValues sv{};
    sv.n = S.n_spots;
    for (int k = 0; k < S.n_spots; ++k) {
        const double *q = values + 4 * k;
        if (!(std::isfinite(q[0]) && std::isfinite(q[1]))) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_epsilon_spots: spot %d: non-finite centre", k);
        if (!(std::isfinite(q[2]) && q[2] >= 0.0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_epsilon_spots: spot %d: the amplitude must be finite and >= 0", k);
        if (!eps_sigma_ok(q[3])) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_update_epsilon_spots: spot %d: sigma must be finite and > 0, with a normal square", k);
        for (int j = 0; j < 4; ++j) sv.v[k][j] = q[j];
    }
    S.applied(sv);
    launch_eps_spots(ctx, S, sv, S.xy.p, S.eps0.p, ctx->eps.p, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->have_eps = true;
    return TDGL_OK;
}

// the K x 4 values of the epsilon in force (n_spots = 0: no spots are set): the host's record, or -- after a run-ahead batch,
// whose values the host did not see -- what the kernel left
extern "C" int tdgl_get_epsilon_spot_values(tdgl_ctx *ctx, int32_t *n_spots, double *values) {
    CTX_GUARD(ctx);
    if (!n_spots || !values) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_get_epsilon_spot_values: null output");
    const EpsSpots &S = ctx->eps_spots;
    *n_spots = S.n_spots;
    if (!S.on()) return TDGL_OK;
    EpsSpotValues sv = S.values();
    if (std::isnan(sv.v[0][0]) && S.d_applied.p) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(&sv, S.d_applied.p, sizeof(sv), hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < S.n_spots; ++k)
        for (int j = 0; j < 4; ++j) values[4 * k + j] = sv.v[k][j];
    return TDGL_OK;
}

// update_mu_boundary (solver.py:325-345) and update_epsilon (solver.py:364-381) for tabulated inputs,
// at the time of the step about to be taken
static int apply_time_tables(tdgl_ctx *ctx) {
    MuTable &M = ctx->mu_tab;
    if (M.on() && M.step(ctx->loop.time)) {
        // (the copy of the host mirror is asynchronous: wait before it can change again)
        TDGL_TRY(apply_mu_boundary(ctx, M.host.data()));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        M.dev_synced = true;
    }
    EpsTable &E = ctx->eps_tab;
    if (E.on() && E.step(ctx->loop.time)) {
        hipLaunchKernelGGL(k_scale, dim3(grid_for(ctx->n_pad)), dim3(BLOCK), 0, ctx->stream, ctx->n_pad, E.last,
                           (const double *)E.eps0.p, ctx->eps.p);
        ctx->have_eps = true;
    }
    EpsSpots &S = ctx->eps_spots;
    if (S.on() && S.step(ctx->loop.time)) {
        launch_eps_spots(ctx, S, S.values(), S.xy.p, S.eps0.p, ctx->eps.p, nullptr);
        ctx->have_eps = true;
    }
    return TDGL_OK;
}
