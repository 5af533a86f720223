// Application of the mu factors: the dense inverse of the whole matrix, or the nested-dissection levels with the dense /
// block low-rank inverse of the top separator (set-up: dense.inc) -- the direct mu solve in fp64 and, stored in fp32, the
// CG's second preconditioner.  Here: the records its kernels take (DenseFinish, SubMean), one launcher per kernel, the
// launch sequence (direct_solve_launch), the preconditioner's wrapper and the in-loop guard.  Included by tdgl_hip.hip
// behind vcycle.inc (launch_csr, launch_sell, vec_grid, in_storage) and in front of poisson.inc.

static int precond_schur_apply(tdgl_ctx *ctx, const double *r, double *z, double *rz_part);  // schur.inc

// DenseFinish (kernels.inc: finish_product, finish_separator) inside a time step: the flags and maxima of the step's psi
// update, and what workgroup 0 does with them -- the status block (classic loop) or the run-ahead loop's controller ctl
// with this step's record rec.  The whole-matrix inverse writes mu itself: guard = 1, fail_part = the flags in a step,
// else NULL.  Behind a top separator the ways up look at the flags: guard = 0, and fail_part feeds the status block alone.
static DenseFinish finish_in_step(const tdgl_ctx *ctx, DenseFinish fin, int guard, const int32_t *fail_part, bool in_step, StepCtl *ctl,
                                  StepRec *rec) {
    fin.dmax_part = ctx->psi_dmax_part.p, fin.fail_part = fail_part, fin.nfail = ctx->psi_blocks;
    fin.st = (in_step && !ctl) ? ctx->status_dev : nullptr, fin.guard = guard;
    fin.ctl = ctl, fin.rec = rec;
    return fin;
}

// SubMean (kernels.inc: k_sub_up).  Its terms: every level's (G_p 1)^T b_p rows (they sit behind the level's vector:
// w + nI + nS), the shares of u . x_S behind the first level's
static SubMean mean_terms(const DirectFactors &f) {
    SubMean m{};
    int t = 0;
    for (int k = 0; k < f.levels; ++k) {
        const SubLevel &L = f.lv[k];
        m.term[t++] = {L.w.p + L.nI + L.nS, L.parts};
        if (k == 0) m.term[t++] = {f.upart.p, f.nfin};
    }
    return m;
}
// no gauge (the inner levels' ways up) / formed by every workgroup and removed there (one level) / formed by workgroup 0
// of a launch without a gauge of its own and left in f.mean (several levels: the innermost way up) / read from there
static SubMean mean_none() { return SubMean{}; }
static SubMean mean_formed(const DirectFactors &f, double inv_n) { SubMean m = mean_terms(f); m.scale_own = inv_n; return m; }
static SubMean mean_left(const DirectFactors &f, double inv_n) { SubMean m = mean_terms(f); m.scale_out = inv_n, m.out = f.mean.p; return m; }
static SubMean mean_read(const DirectFactors &f) { SubMean m{}; m.in = f.mean.p; return m; }

// One launcher per kernel, as in vcycle.inc: the only place where its hipLaunchKernelGGL stands, the value type deduced
// from the pointer (Stored<VT>::of picks a level's pool or the dense tiles in the storage in force).
template <class VT>
static void launch_dense_sym_tiles(tdgl_ctx *ctx, int n, int nt, const VT *G, const double *b, double *part, const StepCtl *ctl) {
    hipLaunchKernelGGL((k_dense_sym_tiles<VT>), dim3(nt * (nt + 1) / 2), dim3(BLOCK), 0, ctx->stream, n, nt, G, b, part, ctl);
}

// The dense pair, y = G b on n rows with the symmetric tiles of D in the storage they are held in: every tile's
// contributions into D.part, then nfin workgroups of 64 rows add up the slots and do with the sums what `fin` says
// (in the time loop the same launch publishes the step's status block).
static void launch_dense_sym(tdgl_ctx *ctx, const DenseTiles &D, int n, int nfin, const double *b, const DenseFinish &fin) {
    in_storage(D.G32.n > 0, [&](auto S) { launch_dense_sym_tiles(ctx, n, D.tiles, S.of(D.G, D.G32), b, D.part.p, fin.ctl); });
    hipLaunchKernelGGL(k_dense_sym_finish, dim3(nfin), dim3(BLOCK), 0, ctx->stream, n, D.tiles, (const double *)D.part.p, fin);
}

// The two launches of the top separator in block low-rank form (dense.inc: dense_to_blr), y = G b on n rows in nt tiles:
// k_blr_project (the dense tiles into `part`, every column's projection into its twin's slot of Z.coef), then
// k_blr_finish on nfin workgroups of 64 rows with the record k_dense_sym_finish takes (a separator's: guard = 0).  The
// preconditioner's application and tdgl_blr_apply (the kernels alone, for the tests) both come through here.
static void blr_launch(tdgl_ctx *ctx, const BlrTop &Z, int n, int nt, int nfin, const double *b, double *part, const DenseFinish &fin) {
    const BlrArgs a{Z.ndense, Z.nitems, Z.dense_ij.p, Z.Gd.p, Z.F.p, Z.colbase.p, Z.twin.p,
                    reinterpret_cast<const BlrItem *>(Z.items.p), Z.coef.p, Z.dslot_ptr.p, Z.dslot.p};
    hipLaunchKernelGGL(k_blr_project, dim3((unsigned)(Z.ndense + (Z.nitems + BLOCK / WAVE - 1) / (BLOCK / WAVE))), dim3(BLOCK), 0,
                       ctx->stream, n, nt, a, b, part, (const StepCtl *)fin.ctl);
    hipLaunchKernelGGL(k_blr_finish, dim3(nfin), dim3(BLOCK), 0, ctx->stream, n, nt, a, (const double *)part, fin);
}

// the way up of one level: its separator solution L.xs and the way down's L.w -> out
// (R: 64-row chunks per workgroup -- 1, or a whole part of up to 256 rows on the levels stored as symmetric tiles;
// map: row i goes to out[map[i]] -- the first level of a preconditioner application, precond_direct_apply)
template <class VT>
static void launch_sub_up(tdgl_ctx *ctx, const SubLevel &L, const VT *vals, double *out, const SubMean &m, const int32_t *fail, const StepCtl *ctl,
                          const int32_t *map = nullptr) {
    const int nblk_int = L.nI > 0 ? (int)L.up_chunks.n : 0, nblk_sep = grid_for(L.nS);
    auto go = [&](auto R) {
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(nblk_int + nblk_sep), dim3(BLOCK), 0, ctx->stream, L.nI, L.nS, nblk_int,
                               (const SubUpChunk *)L.up_chunks.p, (const int32_t *)L.sep_idx.p, vals, (const double *)L.w.p,
                               (const double *)L.xs.p, m, fail, ctx->psi_blocks, out, ctl, map);
        };
        if (map) launch(k_sub_up<VT, decltype(R)::value, true>);
        else launch(k_sub_up<VT, decltype(R)::value, false>);
    };
    if (L.up_R >= 4) go(std::integral_constant<int, 4>{});
    else if (L.up_R == 3) go(std::integral_constant<int, 3>{});
    else if (L.up_R == 2) go(std::integral_constant<int, 2>{});
    else go(std::integral_constant<int, 1>{});
}

template <class VT> static size_t sym_lds_bytes(int np_lds) {  // k_sub_down_sym: b_p, eight accumulators, eight tiles
    return (size_t)(1 + 2 * (BLOCK / WAVE)) * np_lds * sizeof(double) + (size_t)(2 * (BLOCK / WAVE)) * ST * STP * sizeof(VT);
}

// the way down of one level: b (the level's vector) -> L.w.  `lanes`: the preconditioner's lane-per-row work lists;
// `first`: the first level (its coupling product takes 8 lanes per row, the inner levels' 16); map: entry i of the
// level's vector is b[map[i]] (the first level of a preconditioner application: its work lists are lanes or tiles)
template <class VT>
static void launch_sub_down(tdgl_ctx *ctx, const SubLevel &L, const VT *vals, bool first, bool lanes, const double *b, const StepCtl *ctl,
                            const int32_t *map = nullptr) {
    const int64_t nI = L.nI, nS = L.nS, rows = nI + nS + L.parts;
    const int nblk_dint = nI > 0 ? (int)L.down_chunks.n : 0;
    const int nblk_drest = (int)((rows - nI + BLOCK / WAVE - 1) / (BLOCK / WAVE));
    const SubDownChunk *chunks = L.down_chunks.p;
    const SubDownRow *drows = L.down_rows.p;
    const int32_t *seg_ptr = L.seg_ptr.p, *seg_x = L.seg_x.p, *seg_len = L.seg_len.p;
    const int64_t *seg_val = L.seg_val.p;
    if (lanes || L.sym_lds > 0) {  // (tiles: also a level of the fp64 direct solve, tdgl_poisson_set_substructure_layout)
        const int64_t n_id = L.ident ? nS : 0;
        const int nblk_id = grid_for(n_id) * (n_id > 0), nblk_w = (int)((rows - nI - n_id + BLOCK / WAVE - 1) / (BLOCK / WAVE));
        // (tiles requested one pair ahead: two and three pairs ahead measured the same application time at 1M sites,
        // profiles/EXPERIMENTS.md round 6 -- the kernel is not waiting for its loads)
        const dim3 grid((unsigned)(nblk_dint + nblk_id + nblk_w));
        auto sym = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), sym_lds_bytes<VT>(L.sym_lds), ctx->stream, nI, n_id, rows, nblk_dint, nblk_id, L.sym_lds,
                               chunks, seg_ptr, seg_val, seg_x, seg_len, vals, b, L.w.p, ctl, map);
        };
        auto lane_form = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), 0, ctx->stream, nI, n_id, rows, nblk_dint, nblk_id, chunks, drows, seg_ptr, seg_val, seg_x,
                               seg_len, vals, b, L.w.p, ctl, map);
        };
        if (L.sym_lds > 0) {
            if (map) sym(k_sub_down_sym<VT, 1, true>);
            else sym(k_sub_down_sym<VT, 1, false>);
        } else {
            if (map) lane_form(k_sub_down_lanes<VT, true>);
            else lane_form(k_sub_down_lanes<VT, false>);
        }
    } else
        hipLaunchKernelGGL((k_sub_down<VT>), dim3((unsigned)(nblk_dint + nblk_drest)), dim3(BLOCK), 0, ctx->stream, nI, rows, nblk_dint, chunks,
                           drows, seg_ptr, seg_val, seg_x, seg_len, vals, b, L.w.p, ctl);
    // (optional: the separator rows above were b_S alone; r_S = b_S - A_SI y_I with the sparse coupling block)
    if (L.coupling.nnz > 0) {
        if (first) launch_csr<8, C_RESID, 4>(ctx, L.coupling, L.w.p, L.w.p + nI, nullptr, 0.0, 0.0, nullptr, L.w.p + nI);
        else launch_csr<16, C_RESID, 4>(ctx, L.coupling, L.w.p, L.w.p + nI, nullptr, 0.0, 0.0, nullptr, L.w.p + nI);
    }
}

// the residual into the dissection's order (also the rank-level dissection's interior, schur.inc)
static void launch_pd_gather(tdgl_ctx *ctx, int64_t n, const int32_t *map, const double *r, double *out) {
    hipLaunchKernelGGL(k_pd_gather, dim3(vec_grid(n)), dim3(BLOCK), 0, ctx->stream, n, map, r, out);
}

// The launches of a direct mu solve, x = pinv(A) b (dense inverse or substructured; see the header).
// in_step: inside the time loop -- the kernels that write x hold back when this step's psi update failed and
// the status block is published by k_dense_sym_finish (returns true then).  ctl / rec: the run-ahead loop's
// device-resident controller and the record of this step (run.inc), else NULL.  map (the preconditioner's folded
// application, precond_direct_apply): b and x are in the context's order, entry i of the first level's vector is
// b[map[i]] / goes to x[map[i]]; NULL: both in the dissection's order.
template <class VT>
static bool direct_solve_launch_t(tdgl_ctx *ctx, const double *b, double *x, bool in_step, StepCtl *ctl, StepRec *rec, const int32_t *map) {
    const DirectFactors &f = *ctx->direct;
    const double inv_n = 1.0 / (double)ctx->n_global;
    const int32_t *fail = in_step ? (const int32_t *)ctx->psi_fail_part.p : (const int32_t *)nullptr;
    if (f.levels == 0) {  // the dense inverse of the whole matrix
        launch_dense_sym(ctx, f.dense, (int)ctx->n, (int)((ctx->n + WAVE - 1) / WAVE), b,
                         finish_in_step(ctx, finish_product(x), 1, fail, in_step, ctl, rec));
        return in_step;
    }
    // substructured: the ways down level after level (a level works on the previous level's separator vector), the last
    // level's separator by the dense pair (which also publishes the step's status), the ways up innermost first.  With
    // one level its way up removes the mean; with more the inner ones go without a gauge, and the first of them leaves
    // the mean (all levels' shares of sum x) for the first level's way up.
    const bool lanes = f.stage == DirectFactors::PRECOND;
    const int K = f.levels;
    const double *vec = b;
    for (int k = 0; k < K; ++k) {
        launch_sub_down(ctx, f.lv[k], Stored<VT>::of(f.lv[k].vals, f.lv[k].vals32), k == 0, lanes, vec, ctl, k == 0 ? map : nullptr);
        vec = f.lv[k].w.p + f.lv[k].nI;
    }
    const SubLevel &T = f.lv[K - 1];
    const DenseFinish fin = finish_in_step(ctx, finish_separator(T.xs.p, T.u.p, f.upart.p), 0, ctx->psi_fail_part.p, in_step, ctl, rec);
    if (f.blr.ndense > 0)  // the top separator in block low-rank form (preconditioner, dense.inc: dense_to_blr)
        blr_launch(ctx, f.blr, (int)T.nS, f.dense.tiles, f.nfin, vec, f.dense.part.p, fin);
    else
        launch_dense_sym(ctx, f.dense, (int)T.nS, f.nfin, vec, fin);
    for (int k = K - 1; k >= 1; --k)
        launch_sub_up(ctx, f.lv[k], Stored<VT>::of(f.lv[k].vals, f.lv[k].vals32), f.lv[k - 1].xs.p, k == K - 1 ? mean_left(f, inv_n) : mean_none(), fail, ctl);
    launch_sub_up(ctx, f.lv[0], Stored<VT>::of(f.lv[0].vals, f.lv[0].vals32), x, K == 1 ? mean_formed(f, inv_n) : mean_read(f), fail, ctl, map);
    return in_step;
}

static bool direct_solve_launch(tdgl_ctx *ctx, const double *b, double *x, bool in_step, StepCtl *ctl, StepRec *rec, const int32_t *map = nullptr) {
    return ctx->direct->fp32 ? direct_solve_launch_t<float>(ctx, b, x, in_step, ctl, rec, map)
                             : direct_solve_launch_t<double>(ctx, b, x, in_step, ctl, rec, map);
}

// ---- the factors as preconditioner (tdgl_poisson_set_substructure_precond) ---------------------------------------
// z = M r with M ~ pinv(A): the launch sequence of the direct solve on the fp32-stored factors.  r and z stay in the
// context's order: the first level's way down reads r through the dissection's map and its way up stores z through it --
// the dissection's order exists inside those two kernels only.  The partials of r . z go into rz_part, by k_dot_partial;
// with rz_later the caller's next pass over z forms them instead (cg_step_single: k_sell_axp) and rz_part stays as it is.
// TDGL_PD_TWO_PASS (tdgl_create) keeps the earlier order for comparison: the residual gathered into the dissection's
// order (bp), the sequence on vectors in that order, the result (xp) scattered back together with the partials of r . z
// -- the same values in the same order inside the sweeps, so z is the same bit for bit.
static void precond_direct_apply(tdgl_ctx *ctx, const double *r, double *z, double *rz_part, bool rz_later) {
    const DirectFactors &f = *ctx->direct;
    if (ctx->pd_two_pass) {
        ctx->pd_applies_two_pass += 1;
        launch_pd_gather(ctx, ctx->n, f.map.p, r, f.bp.p);
        (void)direct_solve_launch(ctx, f.bp.p, f.xp.p, false, nullptr, nullptr);
        hipLaunchKernelGGL(k_pd_scatter, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, ctx->n, (const int32_t *)f.map.p, (const double *)f.xp.p, r,
                           z, rz_part);
        return;
    }
    ctx->pd_applies_folded += 1;
    (void)direct_solve_launch(ctx, r, z, false, nullptr, nullptr, f.map.p);
    if (!rz_later)
        hipLaunchKernelGGL(k_dot_partial, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, ctx->n, r, (const double *)z, rz_part);
}

// does an application with rz_later leave r . z to the caller's next pass?  (not on the two-pass order, whose scatter
// forms it, and not in one-process-per-GPU mode)
static inline bool precond_rz_left(const tdgl_ctx *ctx) { return ctx->direct->n_local == 0 && !ctx->pd_two_pass; }

// ... on one GPU the factors of the whole matrix, in one-process-per-GPU mode the rank-level dissection (schur.inc)
static int precond_factors_apply(tdgl_ctx *ctx, const double *r, double *z, double *rz_part, bool rz_later = false) {
    if (ctx->direct->n_local > 0) return precond_schur_apply(ctx, r, z, rz_part);
    precond_direct_apply(ctx, r, z, rz_part, rz_later);
    return TDGL_OK;
}

static inline bool precond_factors_available(const tdgl_ctx *ctx) {
    return ctx->direct && ctx->direct->stage == DirectFactors::PRECOND;
}

// ---- in-loop guard of the direct mu solves ----------------------------------------------------------
// An explicit inverse is checked once at set-up, on one random right-hand side.  In the time loop the
// residual of an accepted step's solve, ||b - A mu|| / ||b|| with the resident level-0 matrix (SELL), is
// measured once per run-ahead batch (classic loop: every DIRECT_GUARD_EVERY steps) -- two small launches
// next to 64 attempts.  Above direct_guard_limit (1e-9; the factors deliver 1e-14) the factors are
// released and AMG-PCG takes over from the next step on; tdgl_get_direct_stats reports it.
constexpr int DIRECT_GUARD_EVERY = 64;
static void direct_guard_launch(tdgl_ctx *ctx) {
    AmgLevel &L0 = *ctx->levels[0];
    hipLaunchKernelGGL(k_dot_partial, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, ctx->n_own, (const double *)ctx->bvec.p,
                       (const double *)ctx->bvec.p, ctx->part_pq.p);
    launch_sell<RESID, DOT_YY>(ctx, L0.A, ctx->mu.p, ctx->bvec.p, nullptr, 0.0, 0.0, nullptr, ctx->pcg_r.p, ctx->part_pair[0].p + NB);
    hipLaunchKernelGGL(k_store_sum, dim3(1), dim3(BLOCK), 0, ctx->stream, (const double *)ctx->part_pq.p, ctx->scal.p, (int)S_BB, 0.0);
    hipLaunchKernelGGL(k_store_sum, dim3(1), dim3(BLOCK), 0, ctx->stream, (const double *)(ctx->part_pair[0].p + NB), ctx->scal.p, (int)S_RR, 0.0);
}
static inline void direct_guard_fetch(tdgl_ctx *ctx) {  // (queued behind everything that writes the status block)
    (void)hipMemcpyAsync(ctx->h_status.p->scal, ctx->scal.p, S_COUNT * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
}
// after the synchronisation; `valid`: mu and b belong to the same, accepted, step
static void direct_guard_read(tdgl_ctx *ctx, bool valid) {
    if (!valid) return;
    const double bb = ctx->h_status.p->scal[S_BB], rr = ctx->h_status.p->scal[S_RR];
    if (!(bb > 0.0)) return;
    const double relres = std::isfinite(rr) ? std::sqrt(rr / bb) : INFINITY;
    ctx->direct_checks += 1;
    if (!(relres <= ctx->direct_relres_max)) ctx->direct_relres_max = relres;
    if (!(relres <= ctx->direct_guard_limit)) {
        ctx->direct.reset();  // run_ahead_ok / dense_on are false from now on: AMG-PCG
        ctx->direct_fell_back = 1;
    }
}

extern "C" int tdgl_get_direct_stats(tdgl_ctx *ctx, double *relres_max, int64_t *checks, int32_t *fell_back) {
    if (!ctx) return TDGL_ERR_ARG;
    if (relres_max) *relres_max = ctx->direct_relres_max;
    if (checks) *checks = ctx->direct_checks;
    if (fell_back) *fell_back = ctx->direct_fell_back;
    return TDGL_OK;
}

// how many applications of the factor preconditioner took the folded order / the two-pass order (TDGL_PD_TWO_PASS)
extern "C" int tdgl_get_precond_apply_stats(tdgl_ctx *ctx, int64_t *folded, int64_t *two_pass) {
    if (!ctx) return TDGL_ERR_ARG;
    if (folded) *folded = ctx->pd_applies_folded;
    if (two_pass) *two_pass = ctx->pd_applies_two_pass;
    return TDGL_OK;
}

extern "C" int tdgl_direct_switching(tdgl_ctx *ctx, int32_t on, int64_t *switches, int32_t *paused) {
    if (!ctx) return TDGL_ERR_ARG;
    if (on >= 0) {
        ctx->choice.enable(on != 0);
    }
    if (switches) *switches = ctx->choice.switches();
    if (paused) *paused = ctx->choice.paused() ? 1 : 0;
    return TDGL_OK;
}

extern "C" int tdgl_set_direct_guard(tdgl_ctx *ctx, double limit) {
    if (!ctx || !(limit > 0.0)) return TDGL_ERR_ARG;
    ctx->direct_guard_limit = limit;
    return TDGL_OK;
}
