// mu Poisson solve: conjugate gradients preconditioned by one smoothed-aggregation AMG
// V-cycle (vcycle.inc), all level operators resident in HBM.  Included by tdgl_hip.hip.  Here: the options and stats, the
// hierarchy setters, sync_status, the direct solve's driver (its launches and guard: factors.inc) and the CG.
//
// Replaces mu = mu_laplacian_lu(rhs) (tdgl/solver/solver.py:516; SuperLU factorisation at
// tdgl/finite_volume/operators.py:305-308).  The reference matrix L_mu is singular (pure
// Neumann); SuperLU returns a solution with a round-off-determined additive constant.  Here
// the symmetrised system A mu = b (A = -diag(a) L_mu, b = -a * rhs) is solved on the
// complement of the constant vector and the zero-mean solution is returned.
//
// Smoother: Chebyshev polynomial of degree `nu` in D^-1 A over [cheb_lo * rho, rho] (default
// degree 2: 13-18 PCG iterations to 1e-10 where one damped-Jacobi sweep needs 23-30), or `nu`
// damped-Jacobi sweeps (smoother = 0).  Both are symmetric in the A inner product, so the
// V-cycle is a valid CG preconditioner.

extern "C" int tdgl_set_poisson_options(tdgl_ctx *ctx, const tdgl_poisson_options *o) {
    if (!ctx || !o) return TDGL_ERR_ARG;
    if (!(o->rtol > 0) || o->max_iter < 1 || o->nu < 1 || o->nu > 8 || o->nu_fine < 0 || o->nu_fine > 8 ||
        o->check_every < 0 || o->extrapolate < 0 || o->extrapolate > 3 || o->guess_window < 0 || o->guess_window > GK ||
        (o->smoother != 0 && o->smoother != 1) || !(o->cheb_lo > 0 && o->cheb_lo < 1))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_poisson_options: invalid options");
    // the storage of the V-cycle's operators (fp64 / fp32 / fp32 + binary16 on level 0) is decided when
    // the reduced-precision copies are made: a change of the option makes them stale
    if (o->precond_fp32 != ctx->popt.precond_fp32) ctx->f32_ready = ctx->coarse32_ready = false;
    ctx->popt = *o;
    ctx->pcg_epoch += 1;  // smoother coefficients / degrees are baked into a captured iteration pair
    return TDGL_OK;
}

extern "C" int tdgl_get_poisson_stats(tdgl_ctx *ctx, int64_t *out3) {
    if (!ctx || !out3) return TDGL_ERR_ARG;
    out3[0] = ctx->f32_fallbacks;
    out3[1] = ctx->last_pcg_iters;
    out3[2] = 0;  // (graph replay of the iteration: removed, slower than plain launches since ROCm 7.2)
    return TDGL_OK;
}

extern "C" int tdgl_get_pcg_prediction_stats(tdgl_ctx *ctx, int64_t *out3, double *rate) {
    if (!ctx || !out3) return TDGL_ERR_ARG;
    out3[0] = ctx->stat_pcg_launched;
    out3[1] = ctx->stat_pcg_needed;
    out3[2] = ctx->stat_pcg_extra_syncs;
    if (rate) *rate = ctx->pcg_rate;
    return TDGL_OK;
}

// how the V-cycle's operators were stored in the last solve: 0 fp64, 1 fp32, 2 fp32 + binary16 on level 0
extern "C" int tdgl_get_precond_storage(tdgl_ctx *ctx, int32_t *mode) {
    if (!ctx || !mode) return TDGL_ERR_ARG;
    *mode = (!ctx->popt.precond_fp32 || !ctx->f32_ready) ? 0 : (ctx->level0_f16 ? 2 : 1);
    return TDGL_OK;
}

extern "C" int tdgl_get_guess_stats(tdgl_ctx *ctx, int32_t *vectors, double *initial_relres) {
    if (!ctx) return TDGL_ERR_ARG;
    if (vectors) *vectors = ctx->last_guess_vectors;
    if (initial_relres) *initial_relres = ctx->last_guess_relres;
    return TDGL_OK;
}

extern "C" int tdgl_get_guess_gram(tdgl_ctx *ctx, int32_t *k, double *G_rowmajor) {
    if (!ctx || !k || !G_rowmajor) return TDGL_ERR_ARG;
    const GuessBasis &g = ctx->guess;
    *k = g.count;
    for (int i = 0; i < g.count; ++i)
        for (int j = 0; j < g.count; ++j) G_rowmajor[i * g.count + j] = g.G[i][j][0] + g.G[i][j][1];
    return TDGL_OK;
}

static int csr_to_sell(tdgl_ctx *ctx, int64_t n_rows, const int32_t *indptr, const int32_t *indices,
                       const double *data, SellF64 &M, bool want16 = false, bool want_off16 = false) {
    return build_sell_f64(ctx, n_rows, indptr, indices, data, M, want16, want_off16);
}

static int upload_csr(tdgl_ctx *ctx, int64_t n_rows, int64_t n_cols, const int32_t *indptr,
                      const int32_t *indices, const double *data, Csr &M) {
    M.n_rows = n_rows;
    M.n_cols = n_cols;
    M.nnz = indptr[n_rows];
    HIP_TRY(ctx, M.indptr.upload(std::vector<int32_t>(indptr, indptr + n_rows + 1)));
    HIP_TRY(ctx, M.indices.upload(std::vector<int32_t>(indices, indices + M.nnz)));
    HIP_TRY(ctx, M.data.upload(std::vector<double>(data, data + M.nnz)));
    return TDGL_OK;
}

extern "C" int tdgl_poisson_set_hierarchy(tdgl_ctx *ctx, const tdgl_amg_level *lv, int32_t n_levels,
                                          const double *coarse_pinv) {
    CTX_GUARD(ctx);
    if (!lv || n_levels < 1 || !coarse_pinv) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_hierarchy: null argument");
    if (lv[0].n != ctx->n_own)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "level 0 has %lld rows, this rank owns %lld sites", (long long)lv[0].n, (long long)ctx->n_own);
    const bool deep = ctx->deep;
    if (deep) {  // two distributed levels: see tdgl_set_deep_halo_plan
        if (n_levels < 3 || lv[0].a_rows != ctx->n || lv[0].p_rows < lv[0].a_rows || lv[0].n_cols != ctx->n_ext ||
            lv[0].p_rows > ctx->n_ext || !lv[1].explicit_only || lv[1].n_cols < lv[1].n)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "two distributed levels: level 0 needs a_rows = %lld, a_rows <= p_rows <= n_cols = %lld,"
                      " level 1 must be explicit_only, and a replicated level must follow", (long long)ctx->n, (long long)ctx->n_ext);
    } else if (lv[0].a_rows || lv[0].p_rows || lv[0].explicit_only || (n_levels > 1 && lv[1].explicit_only)) {
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "a_rows / p_rows / explicit_only need tdgl_set_deep_halo_plan");
    } else if (ctx->n_own < ctx->n && lv[0].n_cols != ctx->n)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "level 0 must have n_cols = %lld (owned + ghost sites)", (long long)ctx->n);
    for (auto *l : ctx->levels) delete l;
    ctx->levels.clear();
    ctx->fusedR.nnz = 0;  // belongs to the previous hierarchy
    ctx->fusedR_off16.release();
    ctx->tail_level = -1;
    ctx->f32_ready = false;
    ctx->coarse32_ready = false;
    ctx->pcg_epoch += 1;
    ctx->direct.reset();  // the explicit inverses belong to the previous operator
    for (int k = 0; k < n_levels; ++k) {
        const tdgl_amg_level &in = lv[k];
        const bool last = (k == n_levels - 1);
        const bool stub = deep && k == 1;  // a distributed level 1 exists through M, Wup, Vneg only
        if (!stub && (!in.A_indptr || !in.A_indices || !in.A_data || !in.dinv))
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "level %d: missing operator", k);
        if (!last && !stub && (!in.P_indptr || (!in.R_indptr && !(deep && k == 0)) || in.n_coarse != lv[k + 1].n))
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "level %d: missing or inconsistent transfer operators", k);
        if (stub && in.n_coarse != lv[k + 1].n) TDGL_FAIL(ctx, TDGL_ERR_ARG, "level 1: n_coarse must be the size of level 2");
        AmgLevel *L = new AmgLevel();
        ctx->levels.push_back(L);
        L->n = in.n;
        L->n_cols = in.n_cols > 0 ? in.n_cols : in.n;
        L->explicit_only = stub;
        L->n_coarse = last ? 0 : in.n_coarse;
        L->rho = in.rho;
        const int64_t a_rows = (deep && k == 0) ? in.a_rows : in.n;
        if (stub) {
            // nothing to upload
        } else if (k == 0) {
            TDGL_TRY(csr_to_sell(ctx, a_rows, in.A_indptr, in.A_indices, in.A_data, L->A, /*want16=*/true));
            ctx->level0_absmax = 0.0;
            for (int64_t e = 0; e < in.A_indptr[a_rows]; ++e)
                ctx->level0_absmax = std::max(ctx->level0_absmax, std::fabs(in.A_data[e]));
        } else
            TDGL_TRY(upload_csr(ctx, in.n, in.n, in.A_indptr, in.A_indices, in.A_data, L->Ac));
        // level-0 vectors carry the ghost entries too (two distributed levels: the whole ghost zone; level 1: the
        // entries b1 is formed on)
        L->n_pad = (k == 0) ? std::max<int64_t>(ctx->n_pad, round_up(L->n_cols, WAVE)) : round_up(std::max<int64_t>(L->n_cols, 1), WAVE);
        if (!stub) {
            std::vector<double> dinv(L->n_pad, 0.0);
            // (distributed level 0: dinv also for the ghost sites, the fused residual gathers it)
            std::copy(in.dinv, in.dinv + ((k == 0 && in.n_cols > 0) ? in.n_cols : in.n), dinv.begin());
            HIP_TRY(ctx, L->dinv.upload(dinv));
        }
        if (!last && !stub) {
            if (k == 0) {  // rows for owned AND ghost sites (two distributed levels: two ghost layers)
                const int64_t p_rows = deep ? in.p_rows : ctx->n;
                TDGL_TRY(csr_to_sell(ctx, p_rows, in.P_indptr, in.P_indices, in.P_data, L->P, false, /*want_off16=*/true));
                for (int64_t e = 0; e < in.P_indptr[p_rows]; ++e)
                    ctx->level0_absmax = std::max(ctx->level0_absmax, std::fabs(in.P_data[e]));
            } else
                TDGL_TRY(upload_csr(ctx, in.n, in.n_coarse, in.P_indptr, in.P_indices, in.P_data, L->Pc));
            if (in.R_indptr) TDGL_TRY(upload_csr(ctx, in.n_coarse, in.n, in.R_indptr, in.R_indices, in.R_data, L->R));
        }
        HIP_TRY(ctx, L->xa.alloc(L->n_pad));
        HIP_TRY(ctx, L->xb.alloc(L->n_pad));
        HIP_TRY(ctx, L->d.alloc(L->n_pad));
        HIP_TRY(ctx, L->r.alloc(L->n_pad));
        if (k > 0) HIP_TRY(ctx, L->b.alloc(L->n_pad + TAIL_Y_MAX));  // (spare room: the tail's y = G b)
    }
    ctx->n_coarsest = lv[n_levels - 1].n;
    HIP_TRY(ctx, ctx->coarse_pinv.upload(
                     std::vector<double>(coarse_pinv, coarse_pinv + ctx->n_coarsest * ctx->n_coarsest)));
    const int64_t n_pad0 = ctx->levels[0]->n_pad;  // (>= ctx->n_pad: the residual lives on the whole ghost zone)
    HIP_TRY(ctx, ctx->pcg_r.alloc(n_pad0));
    HIP_TRY(ctx, ctx->pcg_p.alloc(n_pad0));
    HIP_TRY(ctx, ctx->pcg_q.alloc(n_pad0));
    HIP_TRY(ctx, ctx->pcg_p2.alloc(n_pad0));
    HIP_TRY(ctx, ctx->mu_prev.alloc(ctx->n_pad));
    HIP_TRY(ctx, ctx->mu_prev2.alloc(ctx->n_pad));
    HIP_TRY(ctx, ctx->part_pair[0].alloc(3 * NB));  // [r.z | ||r||^2 | z.w] partials, see pcg_solve
    HIP_TRY(ctx, ctx->part_pair[1].alloc(3 * NB));
    HIP_TRY(ctx, ctx->part_pq.alloc(NB));
    HIP_TRY(ctx, ctx->part_tmp.alloc(NB));
    ctx->prev_dt = ctx->prev_dt2 = 0.0;
    ctx->guess.reset();  // the projection basis belongs to the previous operator
    return TDGL_OK;
}

// Direct solve for small meshes: G = pinv(A) [n, n] dense, row major, level-0 site order (see the header).
// Stored with an even leading dimension (16-byte loads), zero padded.
extern "C" int tdgl_poisson_set_dense_inverse(tdgl_ctx *ctx, const double *G, int64_t n) {
    CTX_GUARD(ctx);
    if (!G) {
        ctx->direct.reset();
        return TDGL_OK;
    }
    if (distributed(ctx)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_dense_inverse: single-GPU contexts only");
    if (ctx->levels.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_poisson_set_dense_inverse: set the hierarchy first");
    if (n != ctx->n) TDGL_FAIL(ctx, TDGL_ERR_ARG, "dense inverse has %lld rows, the mesh %lld sites", (long long)n, (long long)ctx->n);
    if (n > 46000) TDGL_FAIL(ctx, TDGL_ERR_ARG, "dense inverse: %lld sites is beyond what a dense matrix is meant for", (long long)n);
    const int64_t ld = round_up(n, 2);
    {
        // symmetric packed storage: tiles (I, J), J <= I, of DT x DT entries, zero padded
        const int nt = (int)((n + DT - 1) / DT);
        const size_t tiles = (size_t)nt * (nt + 1) / 2;
        std::vector<double> packed(tiles * DT * DT, 0.0);
        double asym = 0.0, gmax = 0.0;
        for (int I = 0; I < nt; ++I)
            for (int J = 0; J <= I; ++J) {
                double *dst = packed.data() + ((size_t)I * (I + 1) / 2 + J) * DT * DT;
                const int64_t rows = std::min<int64_t>(DT, n - (int64_t)I * DT), cols = std::min<int64_t>(DT, n - (int64_t)J * DT);
                for (int64_t r = 0; r < rows; ++r) {
                    const double *src = G + ((int64_t)I * DT + r) * n + (int64_t)J * DT;
                    memcpy(dst + r * DT, src, cols * sizeof(double));
                    if (I != J)  // the mirror entries must agree: the packed form keeps one of the two
                        for (int64_t c = 0; c < cols; ++c) {
                            asym = std::max(asym, std::fabs(src[c] - G[((int64_t)J * DT + c) * n + (int64_t)I * DT + r]));
                            gmax = std::max(gmax, std::fabs(src[c]));
                        }
                }
            }
        if (asym > 1e-12 * gmax)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "dense inverse is not symmetric (max |G - G^T| = %.3e, max |G| = %.3e)", asym, gmax);
        auto f = std::make_unique<DirectFactors>();
        HIP_TRY(ctx, f->dense.G.upload(packed));
        HIP_TRY(ctx, f->dense.part.alloc((size_t)nt * nt * DT));
        f->dense.tiles = nt;
        f->dense.n = n;
        f->ld = ld;
        ctx->direct = std::move(f);
        return TDGL_OK;
    }
}

// a direct solve is set (the explicit inverse of the whole matrix, or the substructured one)
// (not while a description is incomplete -- AMG-PCG meanwhile --, nor when the factors precondition the CG)
static inline bool dense_on(const tdgl_ctx *ctx) {
    if (ctx->choice.paused()) return false;  // (a stationary state: the iterative solve is the cheaper one, see tdgl_direct_switching)
    return ctx->direct && ctx->direct->stage == DirectFactors::READY && !distributed(ctx);
}

// Optional: M = R0 (I - c A0 D0^-1) as one CSR matrix [n_1, n_0].  With degree-1 smoothing on
// level 0 the pre-smoothed residual r1 = (I - c A0 D0^-1) r is only ever restricted, so
// R0 r1 = M r: one pass over ~3.5 nnz per fine row replaces the level-0 residual kernel
// (a full pass over A0) plus the restriction.  Built by the host layer (tdgl_amd/amg.py) for the
// smoothing coefficient c in use; ignored when c does not match or in one-process-per-GPU mode.
extern "C" int tdgl_poisson_set_fused_restriction(tdgl_ctx *ctx, int64_t n_rows, int64_t n_cols,
                                                  const int32_t *indptr, const int32_t *indices,
                                                  const double *data, double c) {
    CTX_GUARD(ctx);
    ctx->pcg_epoch += 1;
    if (!indptr) {  // switch off
        ctx->fusedR.nnz = 0;
        ctx->fusedR_off16.release();
        ctx->f32_ready = false;
        return TDGL_OK;
    }
    if (ctx->levels.size() < 2) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "fused restriction needs a hierarchy with >= 2 levels");
    // (one-process-per-GPU mode: columns = owned + ghost sites, rows = the replicated level 1)
    // (two distributed levels: rows = the level-1 entries this rank forms b1 on, columns = the whole ghost zone)
    if (!indices || !data || n_rows != ctx->levels[1]->n_cols || n_cols != ctx->levels[0]->n_cols || !(c > 0.0))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_fused_restriction: inconsistent operator");
    TDGL_TRY(upload_csr(ctx, n_rows, n_cols, indptr, indices, data, ctx->fusedR));
    for (int64_t e = 0; e < indptr[n_rows]; ++e) ctx->level0_absmax = std::max(ctx->level0_absmax, std::fabs(data[e]));
    // 16-bit column offsets from a per-row base, when every row spans < 65536 indices (k_csr_ax16)
    ctx->fusedR_off16.release();
    ctx->fusedR_base.release();
    {
        std::vector<int32_t> base(std::max<int64_t>(n_rows, 1), 0);
        std::vector<uint16_t> off(std::max<int64_t>(indptr[n_rows], 1), 0);
        bool fits = !env_index32();
        for (int64_t i = 0; i < n_rows && fits; ++i) {
            if (indptr[i + 1] == indptr[i]) continue;
            int32_t lo = indices[indptr[i]], hi = lo;
            for (int32_t k = indptr[i]; k < indptr[i + 1]; ++k) {
                lo = std::min(lo, indices[k]);
                hi = std::max(hi, indices[k]);
            }
            if ((int64_t)hi - lo > 65535) {
                fits = false;
                break;
            }
            base[i] = lo;
            for (int32_t k = indptr[i]; k < indptr[i + 1]; ++k) off[k] = (uint16_t)(indices[k] - lo);
        }
        if (fits) {
            HIP_TRY(ctx, ctx->fusedR_base.upload(base));
            HIP_TRY(ctx, ctx->fusedR_off16.upload(off));
        }
    }
    ctx->fusedR_c = c;
    ctx->f32_ready = false;
    return TDGL_OK;
}

// Optional, levels >= 1: R A and A P (with P stored on A P's pattern).  The restricted residual
// R (b - A x) = R b - (R A) x and the prolongation followed by the first post-smoothing step then
// take one launch each instead of two (k_csr_dual).  Same V-cycle, re-associated.
extern "C" int tdgl_poisson_set_fused_level(tdgl_ctx *ctx, int32_t level, const int32_t *ra_indptr,
                                            const int32_t *ra_indices, const double *ra_data,
                                            const int32_t *ap_indptr, const int32_t *ap_indices,
                                            const double *ap_data, const double *p_on_ap_data) {
    CTX_GUARD(ctx);
    if (level < 1 || level >= (int)ctx->levels.size() - 1)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_fused_level: level %d has no coarse-level transfer", level);
    AmgLevel &L = *ctx->levels[level];
    ctx->pcg_epoch += 1;
    if (!ra_indptr) {
        L.fused = false;
        return TDGL_OK;
    }
    if (!ra_indices || !ra_data || !ap_indptr || !ap_indices || !ap_data || !p_on_ap_data)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_fused_level: null array");
    TDGL_TRY(upload_csr(ctx, L.n_coarse, L.n, ra_indptr, ra_indices, ra_data, L.RA));
    TDGL_TRY(upload_csr(ctx, L.n, L.n_coarse, ap_indptr, ap_indices, ap_data, L.AP));
    std::vector<double> pv(p_on_ap_data, p_on_ap_data + L.AP.nnz);
    if (pv.empty()) pv.push_back(0.0);
    HIP_TRY(ctx, L.APp.upload(pv));
    L.fused = true;
    ctx->coarse32_ready = false;
    return TDGL_OK;
}

// Optional: the collapsed coarse chain (host: tdgl_amd/amg.py collapsed_operators).  The same V-cycle
// re-associated into fewer, denser operators, because the levels below level 0 are bound by kernel
// boundaries and dependent round trips, not by bytes:
//   * tdgl_poisson_set_collapsed_level: M = R (I - A S) [n_coarse x n] of an intermediate level, S the
//     two-step pre-smoothing polynomial -> the next right-hand side no longer waits for x = S b;
//   * tdgl_poisson_set_collapsed_tail: everything from `level` down.  mode 0: e = B b with the dense
//     cycle (or exact pseudo-inverse) B [n, n]; mode 1: y = G b (dense [g_rows, n]), e = W b + V y
//     (W CSR [n, n], V dense [n, g_rows]): two launches replace pre-smoothing, restriction, all
//     coarser levels, prolongation and post-smoothing of that level.
// Both are tied to the smoother settings they were built for and ignored when those differ.
extern "C" int tdgl_poisson_set_collapsed_level(tdgl_ctx *ctx, int32_t level, const int32_t *m_indptr,
                                                const int32_t *m_indices, const double *m_data) {
    CTX_GUARD(ctx);
    if (level < 1 || level >= (int)ctx->levels.size() - 1)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_collapsed_level: level %d has no coarser level", level);
    AmgLevel &L = *ctx->levels[level];
    ctx->pcg_epoch += 1;
    ctx->coarse32_ready = false;
    if (!m_indptr) {
        L.M.nnz = 0;
        return TDGL_OK;
    }
    if (!m_indices || !m_data) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_collapsed_level: null array");
    TDGL_TRY(upload_csr(ctx, L.n_coarse, L.n, m_indptr, m_indices, m_data, L.M));
    return TDGL_OK;
}

// The way up on an intermediate level as explicit operators: e = W b + V e_next with W = T_x S + T_b
// (pre-smoothing, post-smoothing and their interplay as ONE polynomial in A, possibly with its
// smallest entries dropped) and V = T_x P.  With them the level costs two launches -- M b on the way
// down, this on the way up -- instead of three, and its pre-smoothed iterate is never formed.
extern "C" int tdgl_poisson_set_collapsed_up(tdgl_ctx *ctx, int32_t level, const int32_t *w_indptr,
                                             const int32_t *w_indices, const double *w_data, const int32_t *v_indptr,
                                             const int32_t *v_indices, const double *v_data) {
    CTX_GUARD(ctx);
    if (level < 1 || level >= (int)ctx->levels.size() - 1)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_collapsed_up: level %d has no coarser level", level);
    AmgLevel &L = *ctx->levels[level];
    ctx->pcg_epoch += 1;
    ctx->coarse32_ready = false;
    if (!w_indptr) {
        L.Wup.nnz = 0;
        L.Vneg.nnz = 0;
        L.up_woff.release();
        L.up_w16.release();
        return TDGL_OK;
    }
    if (!w_indices || !w_data || !v_indptr || !v_indices || !v_data)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_collapsed_up: null array");
    TDGL_TRY(upload_csr(ctx, L.n, L.n_cols, w_indptr, w_indices, w_data, L.Wup));
    std::vector<double> neg(v_data, v_data + v_indptr[L.n]);
    for (double &v : neg) v = -v;
    if (neg.empty()) neg.push_back(0.0);
    TDGL_TRY(upload_csr(ctx, L.n, L.n_coarse, v_indptr, v_indices, neg.data(), L.Vneg));
    // compact index forms (k_mid_up): all or nothing
    L.up_woff.release();
    L.up_wbase.release();
    L.up_vidx.release();
    if (L.n_coarse < 65536 && !env_index32()) {
        std::vector<int32_t> base(std::max<int64_t>(L.n, 1), 0);
        std::vector<uint16_t> off(std::max<int64_t>(w_indptr[L.n], 1), 0), vidx(std::max<int64_t>(v_indptr[L.n], 1), 0);
        bool fits = true;
        for (int64_t i = 0; i < L.n && fits; ++i) {
            if (w_indptr[i + 1] == w_indptr[i]) continue;
            int32_t lo = w_indices[w_indptr[i]], hi = lo;
            for (int32_t k = w_indptr[i]; k < w_indptr[i + 1]; ++k) {
                lo = std::min(lo, w_indices[k]);
                hi = std::max(hi, w_indices[k]);
            }
            if ((int64_t)hi - lo > 65535) fits = false;
            base[i] = lo;
            for (int32_t k = w_indptr[i]; k < w_indptr[i + 1] && fits; ++k) off[k] = (uint16_t)(w_indices[k] - lo);
        }
        if (fits) {
            for (int64_t k = 0; k < v_indptr[L.n]; ++k) vidx[k] = (uint16_t)v_indices[k];
            HIP_TRY(ctx, L.up_wbase.upload(base));
            HIP_TRY(ctx, L.up_woff.upload(off));
            HIP_TRY(ctx, L.up_vidx.upload(vidx));
        }
    }
    return TDGL_OK;
}

extern "C" int tdgl_poisson_set_collapsed_tail(tdgl_ctx *ctx, const tdgl_collapsed_tail *t) {
    CTX_GUARD(ctx);
    ctx->pcg_epoch += 1;
    ctx->coarse32_ready = false;
    ctx->tail_level = -1;
    if (!t) return TDGL_OK;
    if (t->level < 1 || t->level >= (int)ctx->levels.size() - (t->mode == 1 ? 1 : 0) || (t->mode != 0 && t->mode != 1))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_collapsed_tail: bad level %d / mode %d", t->level, t->mode);
    const int64_t n = ctx->levels[t->level]->n;
    if (!t->G || (t->mode == 1 && (!t->W_indptr || !t->W_indices || !t->W_data || t->g_rows < 1 || t->v_cols < 0 ||
                                   t->v_cols > t->g_rows || (t->v_cols > 0 && !t->V))))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_collapsed_tail: missing operator");
    if (t->mode == 1 && t->g_rows > TAIL_Y_MAX)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_collapsed_tail: g_rows %lld above the limit %d", (long long)t->g_rows,
                  TAIL_Y_MAX);
    const int64_t g = t->mode == 0 ? n : t->g_rows;
    // dense operators are stored with leading dimensions rounded up to 4 entries (16-byte loads in
    // fp32 and fp64), zero padded; the vectors they multiply are padded to a wavefront anyway
    auto padded = [](const double *src, int64_t rows, int64_t cols, int64_t ld) {
        std::vector<double> out((size_t)(rows * ld), 0.0);
        for (int64_t i = 0; i < rows; ++i) std::copy(src + i * cols, src + (i + 1) * cols, out.begin() + i * ld);
        return out;
    };
    ctx->tail_ldg = round_up(n, 4);
    ctx->tail_v_cols = t->mode == 1 ? t->v_cols : 0;
    ctx->tail_ldv = round_up(ctx->tail_v_cols, 4);
    HIP_TRY(ctx, ctx->tailG.upload(padded(t->G, g, n, ctx->tail_ldg)));
    if (t->mode == 1) {
        if (ctx->tail_v_cols > 0)
            HIP_TRY(ctx, ctx->tailV.upload(padded(t->V, n, ctx->tail_v_cols, ctx->tail_ldv)));
        else
            ctx->tailV.release();
        // W acts on [b ; y]: y = G b is written right behind the level's right-hand side (its buffer
        // has TAIL_Y_MAX spare entries), so columns >= n move to n_pad + (col - n)
        const int64_t n_pad_t = ctx->levels[t->level]->n_pad;
        const int32_t nnz = t->W_indptr[n];
        std::vector<int32_t> wi(t->W_indices, t->W_indices + nnz);
        for (int32_t &c : wi) {
            if (c < 0 || c >= n + g) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_collapsed_tail: W column %d out of range", c);
            if (c >= n) c = (int32_t)(n_pad_t + (c - n));
        }
        TDGL_TRY(upload_csr(ctx, n, n_pad_t + g, t->W_indptr, wi.data(), t->W_data, ctx->tailW));
        ctx->tailW_idx16.release();
        if (n_pad_t + g < 65536 && !env_index32()) {
            std::vector<uint16_t> i16(wi.begin(), wi.end());
            if (i16.empty()) i16.push_back(0);
            HIP_TRY(ctx, ctx->tailW_idx16.upload(i16));
        }
    }
    ctx->tail_g_rows = g;
    ctx->tail_mode = t->mode;
    ctx->tail_nu = t->nu;
    ctx->tail_smoother = t->smoother;
    ctx->tail_cheb_lo = t->cheb_lo;
    ctx->tail_level = t->level;
    return TDGL_OK;
}

// The host's look at the stream: the status block travels to the host, which waits for it (stat_wait_ns,
// stat_host_syncs).  guard: the scalars of the direct solve's residual check ride behind the status block.
// shadow: launches on ctx->stream that the step needs whatever the host is about to decide.  They are queued behind
// the copy and run while it lands, the host wakes and does its arithmetic, and its next launch reaches the device:
// the host then waits for an event recorded right behind the copy, not for the stream.
struct NoShadow {
    int operator()() const { return TDGL_OK; }
};
template <class S>
static int sync_status(tdgl_ctx *ctx, bool guard, S shadow) {
    constexpr bool shadowed = !std::is_same<S, NoShadow>::value;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_status.p, ctx->d_status.p, sizeof(StepStatus), hipMemcpyDeviceToHost, ctx->stream));
    if (guard) direct_guard_fetch(ctx);
    if (shadowed) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_status, ctx->stream));
        TDGL_TRY(shadow());
    }
    const int64_t t0 = now_ns();
    const hipError_t e = shadowed ? hipEventSynchronize(ctx->ev_status) : hipStreamSynchronize(ctx->stream);
    ctx->stat_wait_ns += now_ns() - t0;
    ctx->stat_host_syncs += 1;
    HIP_TRY(ctx, e);
    return TDGL_OK;
}
static int sync_status(tdgl_ctx *ctx, bool guard = false) { return sync_status(ctx, guard, NoShadow{}); }

template <class S>
static int fetch_scalars(tdgl_ctx *ctx, bool guess_start, const double *rr_part, S shadow) {
    publish_status(ctx, guess_start, rr_part);
    return sync_status(ctx, false, shadow);
}
static int fetch_scalars(tdgl_ctx *ctx, bool guess_start = false, const double *rr_part = nullptr) {
    return fetch_scalars(ctx, guess_start, rr_part, NoShadow{});
}

// mu = G b in one launch sequence (tdgl_poisson_set_dense_inverse / _substructure).  In the time loop (in_step) the
// kernels themselves hold the result back when the psi update of this step failed, the step driver's edge currents
// follow at once, and the step's only synchronisation comes after them.  after_first_sync / abandoned: see pcg_solve.
template <class F>
static int direct_mu_solve(tdgl_ctx *ctx, MuSolveArgs &args, F after_first_sync, bool *abandoned, bool in_step) {
    const int64_t no = ctx->n_own;
    double *b = ctx->bvec.p, *x = ctx->mu.p;
    if (!in_step) {  // one-off solve: b orthogonal to the constants, so that the residual below means something
        hipLaunchKernelGGL(k_dot_partial, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, no, b, (const double *)nullptr, ctx->part_tmp.p);
        hipLaunchKernelGGL(k_shift_mean, dim3(vec_grid(no)), dim3(BLOCK), 0, ctx->stream, no, ctx->part_tmp.p, 1.0 / (double)ctx->n_global, b);
    }
    const bool status_done = direct_solve_launch(ctx, b, x, in_step, nullptr, nullptr);
    if (args.speculate(in_step)) launch_edge_currents(ctx, ctx->psi[1 - ctx->loop.cur].p, x, ctx->js.p, ctx->jn.p);
    const double *rr_part = nullptr;
    if (!in_step) {  // the true residual, for the caller of tdgl_poisson_solve
        hipLaunchKernelGGL(k_dot_partial, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, no, b, b, ctx->part_pq.p);
        hipLaunchKernelGGL(k_store_sum, dim3(1), dim3(BLOCK), 0, ctx->stream, ctx->part_pq.p, ctx->scal.p, (int)S_BB,
                           ctx->popt.rtol * ctx->popt.rtol);
        launch_sell<RESID, DOT_YY>(ctx, ctx->levels[0]->A, x, b, nullptr, 0.0, 0.0, nullptr, ctx->pcg_r.p, ctx->part_pair[0].p + NB);
        rr_part = ctx->part_pair[0].p + NB;
    }
    bool guard = false;
    if (in_step && status_done && --ctx->direct_guard_countdown <= 0) {
        ctx->direct_guard_countdown = DIRECT_GUARD_EVERY;
        guard = true;
        direct_guard_launch(ctx);
    }
    if (status_done) {  // published by k_dense_sym_finish: only the copy and the step's one synchronisation are left
        ctx->psi_status_pending = false;
        TDGL_TRY(sync_status(ctx, guard));
    } else {
        TDGL_TRY(fetch_scalars(ctx, false, rr_part));
    }
    if (!after_first_sync(ctx->h_status.p)) {
        if (abandoned) *abandoned = true;
        return TDGL_OK;
    }
    ctx->last_pcg_iters = 0;
    ctx->last_guess_vectors = 0;
    if (guard) direct_guard_read(ctx, true);  // (the psi update succeeded: mu = G b was written)
    const double bb = ctx->h_status.p->scal[S_BB];
    ctx->last_relres = (!in_step && bb > 0.0) ? std::sqrt(ctx->h_status.p->scal[S_RR] / bb) : 0.0;
    ctx->last_guess_relres = ctx->last_relres;
    HIP_TRY(ctx, hipGetLastError());
    return TDGL_OK;
}

// ---- the preconditioned CG ---------------------------------------------------------------------------
// Which preconditioner (meshes that carry the substructure factors as one, tdgl_poisson_set_substructure_precond):
// the AMG V-cycle contracts the residual by ~0.3 per iteration at t_V per application, the fp32-stored factors by
// ~1e-5 at t_D (5-6 x t_V at a million sites).  The cost of the rest of a solve from the squared residual rr, either
// way: iterations needed x measured time per iteration.
struct PrecondCost { double amg, pd; double n_amg; };  // predicted time with the V-cycle / the factors; the V-cycle's iterations
static PrecondCost precond_cost(const tdgl_ctx *ctx, double rr, double tol2) {
    const double decades = 0.5 * std::log10(rr / tol2);
    const double n_amg = std::max(1.0, std::ceil(decades / ctx->pcg_rate - 0.25));
    const double n_pd = std::max(1.0, std::ceil(decades / ctx->pd_rate - 0.05));
    const double t_common = 0.55 * ctx->pd_t_vcycle_us;  // (A p + the two recurrences: measured 31 of 85 us at 1M sites)
    return PrecondCost{n_amg * (ctx->pd_t_vcycle_us + t_common), n_pd * (ctx->pd_t_apply_us + t_common), n_amg};
}

// One CG run: what its iterations share.  A solve is one run, or several -- each starts over from the current iterate
// (beta = 0) with another preconditioner, see next_phase and the hand-over in cg_iterate.
struct CgRun {
    tdgl_ctx *ctx;
    double *b, *x, *r, *p, *q;
    // Partials live in two ping-pong buffers [r.z | ||r||^2]: iteration `it` reads r.z and the
    // PREVIOUS residual from pair[it & 1] and writes the new residual into pair[(it + 1) & 1].
    // Keeping both halves adjacent lets the distributed run sum them with ONE all-reduce.
    double *part_rz[2], *part_rr[2];
    bool flex_opt;             // popt.flexible_cg on the path it applies to (pcg_solve)
    bool use_pd;               // the factors precondition, else the V-cycle
    bool f32, coarse32;        // the V-cycle's level 0 / its replicated levels run on the fp32-stored operators
    int it0, budget;           // first iteration of the current run / its limit
    int predicted;             // size of the run's first batch
    bool rr_reduced = true;    // the residual partials the next iteration reads are already global
    bool sum_x_fresh = false;  // part_tmp holds the partials of sum x (left by k_update_xr)
    // The end of the solve (k_finish_solution) rides behind the status copy of every look after a batch, guarded on the
    // device by the scalars that copy carries (pcg_solve sets these three; finish_slot < 0: off)
    int finish_slot = -1;      // the window slot GuessBasis::push will hand out
    double b_mean = 0.0;       // mean of b, still inside it
    bool finish_queued = false;  // a look carried it
    bool finished = false;     // ... and the scalars the host received say that the kernel did its work
    int pd_its = -1;           // iterations taken with the factors before a hand-over to the V-cycle (-1: none)
    double pd_rr_end = 0.0;    // ... and the squared residual they left

    bool f32i() const { return f32 && !use_pd; }   // (the factors deliver an fp64 z)
    bool cg1() const { return f32i() && ctx->deep; }  // (two distributed levels: single-reduction CG on fp32 z, no exchange of z)
    bool flex() const { return flex_opt && f32i(); }
};

// z = M^-1 r and the partials of r.z: into *z (fp64) or *z32 (fp32), whichever the preconditioner delivers
static int cg_precondition(CgRun &run, int it, double **z, const float **z32) {
    tdgl_ctx *ctx = run.ctx;
    double *r = run.r, *rz_new = run.part_rz[it & 1];
    if (run.use_pd) {
        *z = ctx->direct->z.p;
        // (profile mode: every application of the first 64 bracketed by an event pair -> tdgl_profile_read_direct)
        ProfileScope apply;
        TDGL_TRY(profile_begin(ctx, ctx->prof.admit_factor_apply(), apply));
        // (the first iteration of a run: beta = 0, nothing needs r . z before k_sell_axp's pass over z, which forms it --
        // cg_step_single; a further application of the factors in the same run: k_dot_partial behind the sequence)
        TDGL_TRY(precond_factors_apply(ctx, r, *z, rz_new, it == run.it0));
        TDGL_TRY(profile_end(ctx, apply));
    } else if (run.cg1()) {
        *z32 = vcycle0_f32(ctx, r, rz_new, Cycle0Out::ghosts_no_sums());
    } else if (run.f32i() && distributed(ctx)) {
        *z = ctx->levels[0]->xb.p;  // fp64 copy of z: its ghosts travel as doubles
        (void)vcycle0_f32(ctx, r, rz_new, Cycle0Out::f64_rz(*z));
    } else if (run.f32i()) {
        *z32 = vcycle0_f32(ctx, r, rz_new, run.flex() ? Cycle0Out::rz_qz(run.q) : Cycle0Out::rz());
    } else {
        *z = vcycle_level(ctx, 0, r, rz_new, run.coarse32);
    }
    return TDGL_OK;
}

#define TDGL_AXP(ZT, IT, RZ, COLS, Z)                                                                             \
    hipLaunchKernelGGL((k_sell_axp<ZT, IT, RZ>), dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, pat.n_slices, per_xcd, \
                       pat.n_rows, pat.slice_off.p, COLS, L0.A.vals.p, Z, (const double *)p_old,                   \
                       (const double *)rz_new, rz_prev, run.p, run.q, ctx->part_pq.p,                               \
                       flex ? (const double *)(rz_new + 2 * NB) : (const double *)nullptr, (const double *)ctx->scal.p, \
                       (const double *)run.r, rz_new)

// The rest of an iteration on one GPU: the direction update fused into A p (double-buffered p), then x += alpha p,
// r -= alpha q with the partials of the new ||r||^2 -- and of sum x, so that the zero-mean gauge at the end of the
// solve needs no pass over x of its own (valid as soon as one update of this solve has run).
static int cg_step_single(CgRun &run, int it, const double *z, const float *z32) {
    tdgl_ctx *ctx = run.ctx;
    AmgLevel &L0 = *ctx->levels[0];
    const bool flex = run.flex();
    double *rz_new = run.part_rz[it & 1], *rz_old = run.part_rz[(it + 1) & 1];
    double *p_old = run.p;
    run.p = (run.p == ctx->pcg_p.p) ? ctx->pcg_p2.p : ctx->pcg_p.p;
    int per_xcd, grid;
    sell_fixed_grid(L0.A.pat.n_slices, &per_xcd, &grid);
    const double *rz_prev = it == run.it0 ? (const double *)nullptr : (const double *)rz_old;
    const SellPattern &pat = L0.A.pat;
    ProfileScope axp;  // (profile mode: a sample of the launches -> tdgl_profile_read_pcg)
    TDGL_TRY(profile_begin(ctx, ctx->prof.admit_axp(), axp));
    // the factors' first application of a run left z alone: r . z is formed in this pass (k_sell_axp<.., RZ>), in the
    // slots k_update_xr reads; the matrix rows are the sites, so the sum runs over what k_dot_partial's would
    const bool form_rz = run.use_pd && it == run.it0 && precond_rz_left(ctx);
    if (run.f32i()) {
        if (pat.use16) TDGL_AXP(float, int16_t, false, pat.cols16.p, z32); else TDGL_AXP(float, int32_t, false, pat.cols.p, z32);
    } else if (form_rz) {
        if (pat.use16) TDGL_AXP(double, int16_t, true, pat.cols16.p, z); else TDGL_AXP(double, int32_t, true, pat.cols.p, z);
    } else {
        if (pat.use16) TDGL_AXP(double, int16_t, false, pat.cols16.p, z); else TDGL_AXP(double, int32_t, false, pat.cols.p, z);
    }
    TDGL_TRY(profile_end(ctx, axp));
    const XrArgs upd{run.p, run.q, rz_new, ctx->part_pq.p, run.part_rr[it & 1], ctx->scal.p, run.x, run.r, run.part_rr[(it + 1) & 1],
                     ctx->n_own, ctx->npart, ctx->part_tmp.p};
    run.sum_x_fresh = true;
    hipLaunchKernelGGL(k_update_xr, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, upd);
    run.rr_reduced = false;
    return TDGL_OK;
}
#undef TDGL_AXP

// ... in one-process-per-GPU mode: Chronopoulos-Gear recurrences, one all-reduce for the CG sums (the other one of
// the iteration is the coarse right-hand side in the V-cycle).  w = A z lands in the second direction buffer (unused
// in this mode).
static int cg_step_ranks(CgRun &run, int it, double *z, const float *z32) {
    tdgl_ctx *ctx = run.ctx;
    AmgLevel &L0 = *ctx->levels[0];
    const int64_t no = ctx->n_own;
    double *rz_new = run.part_rz[it & 1];
    double *w = ctx->pcg_p2.p, *zw = rz_new + 2 * NB;
    const bool cg1 = run.cg1();
    if (cg1) {
        // z is already valid on the first ghost layer (formed there redundantly): no exchange; r.z and z.w
        // over the owned rows in this one pass
        const SellPattern &pat = L0.A.pat;
        const int n_slices = (int)((no + WAVE - 1) / WAVE), tiles = (n_slices + BLOCK / WAVE - 1) / (BLOCK / WAVE);
        const int per_xcd = std::max(1, (tiles + XCDS - 1) / XCDS);
        if (pat.use16)
            hipLaunchKernelGGL((k_sell_spmv<AX, DOT_BX_XY, int16_t, double, float>), dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream,
                               n_slices, per_xcd, 0, no, pat.slice_off.p, pat.cols16.p, L0.A.vals.p, z32, (const double *)run.r,
                               (const double *)nullptr, 0.0, 0.0, (double *)nullptr, w, rz_new);
        else
            hipLaunchKernelGGL((k_sell_spmv<AX, DOT_BX_XY, int32_t, double, float>), dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream,
                               n_slices, per_xcd, 0, no, pat.slice_off.p, pat.cols.p, L0.A.vals.p, z32, (const double *)run.r,
                               (const double *)nullptr, 0.0, 0.0, (double *)nullptr, w, rz_new);
    } else if (overlap_on(ctx)) {
        TDGL_TRY(comm_halo_start(ctx, z, 1));
        launch_sell<AX, DOT_XY>(ctx, L0.A, z, nullptr, nullptr, 0.0, 0.0, nullptr, w, zw, 1);
        TDGL_TRY(comm_halo_wait(ctx));
        launch_sell<AX, DOT_XY>(ctx, L0.A, z, nullptr, nullptr, 0.0, 0.0, nullptr, w, zw, 2);
    } else {
        TDGL_TRY(comm_halo(ctx, z, 1));
        launch_sell<AX, DOT_XY>(ctx, L0.A, z, nullptr, nullptr, 0.0, 0.0, nullptr, w, zw);
    }
    if (run.rr_reduced) {  // ||r_prev||^2 is already global (first iteration, or just after a check)
        TDGL_TRY(comm_allreduce(ctx, rz_new, NB, 0));
        TDGL_TRY(comm_allreduce(ctx, zw, NB, 0));
    } else {
        TDGL_TRY(comm_allreduce(ctx, rz_new, 3 * NB, 0));
    }
    if (cg1)
        hipLaunchKernelGGL((k_cg_update<float>), dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, no, z32,
                           (const double *)w, (const double *)rz_new, it == run.it0 ? 1 : 0, it & 1, ctx->scal.p, run.p, run.q,
                           run.x, run.r, run.part_rr[(it + 1) & 1]);
    else
        hipLaunchKernelGGL((k_cg_update<double>), dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, no, (const double *)z,
                           (const double *)w, (const double *)rz_new, it == run.it0 ? 1 : 0, it & 1, ctx->scal.p, run.p, run.q,
                           run.x, run.r, run.part_rr[(it + 1) & 1]);
    run.rr_reduced = false;
    return TDGL_OK;
}

// one PCG iteration (all launches on ctx->stream; the only host values in it that change from iteration to iteration are
// the parity of `it` and "is this the first one")
static int cg_iteration(CgRun &run, int it) {
    double *z = nullptr;
    const float *z32 = nullptr;
    TDGL_TRY(cg_precondition(run, it, &z, &z32));
    return (!distributed(run.ctx) && !run.cg1()) ? cg_step_single(run, it, z, z32) : cg_step_ranks(run, it, z, z32);
}

// The iterations of one run, from `it` on until the residual is below the tolerance or the budget is spent.  The host
// looks: with check_every = 0 (auto) after `predicted` iterations (an update that finds the residual already converged
// freezes itself, k_update_xr) and after every iteration from there on; with check_every = k > 0, after every k.
static int cg_iterate(CgRun &run, double tol2, int &it, double &rr) {
    tdgl_ctx *ctx = run.ctx;
    while (rr > tol2 && it < run.budget) {
        int chunk = (ctx->popt.check_every > 0 && !run.use_pd) ? ctx->popt.check_every : (it == run.it0 ? run.predicted : 1);
        chunk = std::min(chunk, run.budget - it);
        for (int c = 0; c < chunk; ++c, ++it) TDGL_TRY(cg_iteration(run, it));
        ctx->stat_pcg_launched += chunk;
        if (it - chunk != run.it0) ctx->stat_pcg_extra_syncs += 1;  // not the first batch of this CG run
        TDGL_TRY(comm_allreduce(ctx, run.part_rr[it & 1], NB, 0));  // the host looks at it now
        run.rr_reduced = true;
        if (run.finish_slot >= 0 && run.sum_x_fresh) {
            // (also scal[S_RR] = sum of the partials, which the guard of the shadow reads)
            TDGL_TRY(fetch_scalars(ctx, false, run.part_rr[it & 1], [&]() {
                hipLaunchKernelGGL(k_finish_solution, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, ctx->n_own,
                                   (const double *)ctx->part_tmp.p, 1.0 / (double)ctx->n_global, run.x, (const double *)run.b, run.b_mean,
                                   (const double *)run.r, ctx->guess.x[run.finish_slot].p, ctx->guess.y[run.finish_slot].p,
                                   (const double *)ctx->scal.p);
                return TDGL_OK;
            }));
            run.finish_queued = true;
            const double *sc = ctx->h_status.p->scal;  // (the kernel's own test, on the copy of the numbers it read)
            run.finished = sc[S_CONV_IT] >= 0.0 || sc[S_RR] <= sc[S_TOL2];
        } else {
            TDGL_TRY(fetch_scalars(ctx, false, run.part_rr[it & 1]));  // also scal[S_RR] = sum of the partials
        }
        rr = ctx->h_status.p->scal[S_RR];
        if (ctx->h_status.p->scal[S_CONV_IT] >= 0.0) {  // converged inside the batch: the rest was frozen
            it = (int)ctx->h_status.p->scal[S_CONV_IT];
            break;
        }
        if (!std::isfinite(rr)) TDGL_FAIL(ctx, TDGL_ERR_PCG, "Poisson solve diverged (non-finite residual) after %d iterations", it);
        // Hand-over: an application of the factors that ends just above the tolerance (a guess at 3e-4 in the long-time
        // regime: 1.4e-10 left) does not need a second one -- 6.5 more decades for 450 us -- when one or two V-cycles (0.5
        // decades, 85 us each) finish the job.  The same cost rule as before the solve, on the residual that is left;
        // the CG starts over from the current iterate (beta = 0) with the other preconditioner.
        if (run.use_pd && rr > tol2 && ctx->pd_choice == 0 && ctx->pd_t_apply_us > 0.0 && ctx->pd_t_vcycle_us > 0.0) {
            const PrecondCost cost = precond_cost(ctx, rr, tol2);
            if (cost.amg < cost.pd) {
                run.pd_its = it - run.it0;
                run.pd_rr_end = rr;
                run.use_pd = false;
                run.it0 = it;
                run.predicted = (int)std::min<double>(cost.n_amg, (double)(run.budget - it));
                ctx->pd_handovers += 1;
            }
        }
    }
    return TDGL_OK;
}

// A run ended above the tolerance with its budget spent: is there another preconditioner to go on with, from the
// current iterate and with a budget of its own?
static bool next_phase(CgRun &run, int it) {
    tdgl_ctx *ctx = run.ctx;
    if (run.use_pd) {
        // (the factors did not get there within the budget -- cannot happen with sound factors: finish with the V-cycle)
        run.use_pd = false;
    } else if (run.f32 && !ctx->deep) {
        // Safety net: the iteration budget ran out with the fp32-stored level-0 operators.  Restart
        // the CG from the current iterate with the fp64 ones before giving up.
        run.f32 = false;
        run.coarse32 = false;
        ctx->f32_fallbacks += 1;
    } else {
        return false;
    }
    run.it0 = it;
    run.budget = it + ctx->popt.max_iter;
    return true;
}

// the bookkeeping behind a solve: counts, the running contraction rates the predictions use, the final error
static int pcg_note_solve(tdgl_ctx *ctx, const CgRun &run, int it, double rr, double bb, double tol2) {
    ctx->last_pcg_iters = it;
    ctx->stat_pcg_iters += it;
    ctx->stat_pcg_needed += it;
    ctx->last_relres = std::sqrt(rr / bb);
    ctx->last_guess_relres = it > 0 ? std::sqrt(std::max(0.0, ctx->h_status.p->scal[S_RR0]) / bb) : ctx->last_relres;
    const int pd_its = run.pd_its;
    if (ctx->pd_last) {
        ctx->pd_solves += 1;
        const int its_f = pd_its >= 0 ? pd_its : it;          // (with the factors; the rest, after a hand-over, with the V-cycle)
        const double rr_f = pd_its >= 0 ? run.pd_rr_end : rr;
        ctx->pd_iters += its_f;
        if (pd_its >= 0) ctx->pd_amg_iters += it - its_f;
        const double rr0 = ctx->h_status.p->scal[S_RR0];
        if (its_f >= 1 && (pd_its >= 0 || !(rr > tol2)) && rr_f > 0.0 && rr0 > rr_f && std::isfinite(rr0)) {
            // (decades per application; a solve that started within a decade of the tolerance says little about it)
            const double seen = 0.5 * std::log10(rr0 / rr_f) / its_f;
            if (rr0 > 100.0 * tol2) ctx->pd_rate = 0.8 * ctx->pd_rate + 0.2 * std::min(8.0, std::max(1.0, seen));
        }
    } else {
        if (precond_factors_available(ctx)) {
            ctx->pd_amg_solves += 1;
            ctx->pd_amg_iters += it;
        }
        if (it >= 2 && !(rr > tol2) && rr > 0.0) {  // contraction per iteration of this solve -> running mean
            const double rr0 = ctx->h_status.p->scal[S_RR0];
            if (rr0 > rr && std::isfinite(rr0)) {
                const double seen = 0.5 * std::log10(rr0 / rr) / it;
                ctx->pcg_rate = 0.8 * ctx->pcg_rate + 0.2 * std::min(1.5, std::max(0.2, seen));
            }
        }
    }
    if (rr > tol2 && ctx->pend_v) (void)comm_halo_wait(ctx);
    if (rr > tol2)
        TDGL_FAIL(ctx, TDGL_ERR_PCG, "Poisson solve did not converge: relative residual %.3e after %d iterations (rtol %.1e)",
                  ctx->last_relres, it, ctx->popt.rtol);
    return TDGL_OK;
}

// Solve A x = b (b = ctx->bvec, x = ctx->mu holds the initial guess).  `args`: what the step driver asks for and hears
// back (a solve outside the time loop passes a default-constructed one).  `after_first_sync` is
// called after the first host synchronisation with the status block filled; it returns false
// to abandon the solve (the step driver retries a failed psi update without finishing a solve
// whose right-hand side is garbage).
// The host synchronises once before the iterations and then as cg_iterate says.
template <class F>
static int pcg_solve(tdgl_ctx *ctx, MuSolveArgs &args, F after_first_sync, bool *abandoned, bool allow_projection = false) {
    if (ctx->levels.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "no AMG hierarchy: call tdgl_poisson_set_hierarchy");
    TDGL_TRY(comm_ready(ctx));
    if (abandoned) *abandoned = false;
    if (dense_on(ctx)) return direct_mu_solve(ctx, args, after_first_sync, abandoned, allow_projection && ctx->psi_status_pending);
    AmgLevel &L0 = *ctx->levels[0];
    GuessBasis &guess = ctx->guess;
    // all pointwise work is on the owned rows; sums are over ranks (comm_allreduce is a no-op
    // on one GPU); the ghost entries of x / p are refreshed before the operator reads them
    const int64_t no = ctx->n_own;
    const double inv_n = 1.0 / (double)ctx->n_global;
    const int gv = vec_grid(no);
    CgRun run{ctx, ctx->bvec.p, ctx->mu.p, ctx->pcg_r.p, ctx->pcg_p.p, ctx->pcg_q.p,
              {ctx->part_pair[0].p, ctx->part_pair[1].p}, {ctx->part_pair[0].p + NB, ctx->part_pair[1].p + NB}};
    double *b = run.b, *x = run.x, *r = run.r;
    run.f32 = precond_f32_on(ctx);
    if (ctx->deep && !distributed(ctx))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "a deep halo plan is set but no transport: call tdgl_comm_init_ipc / _rccl / _callbacks");
    if (ctx->deep && !run.f32)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "two distributed levels need the fp32-stored V-cycle with degree-1 smoothing on"
                  " level 0 and the fused restriction (the default options)");
    if (run.f32) TDGL_TRY(ensure_f32(ctx));
    // Flexible (Polak-Ribiere) beta (tdgl_poisson_options.flexible_cg, off by default -- measured no better than
    // Fletcher-Reeves, see the header) on the path whose preconditioner is not exactly symmetric: the single-GPU recurrence
    // with the fp32 / binary16-stored V-cycle.  The smoothing step that produces z_new also forms z_new . q_old (q still
    // holds A p of the previous iteration); the direction update turns it into beta = -alpha (z_new . q_old) / (r.z)_old.
    run.flex_opt = ctx->popt.flexible_cg != 0 && !distributed(ctx);
    // Initial guess by projection onto the previous solutions: their dot products with the new
    // right-hand side, b.b and sum b go to the host with the status block; x0 and r0 follow the sync.
    const bool proj = allow_projection && ctx->popt.extrapolate >= 3;
    if (proj) {  // (the mean of b is removed arithmetically, see k_multi_dot)
        TDGL_TRY(guess_queue_dots(ctx, b));
    } else {
        // make b orthogonal to the null space (constants); ||b||^2; r = b - A x; ||r||^2
        hipLaunchKernelGGL(k_dot_partial, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, no, b, (const double *)nullptr, ctx->part_tmp.p);
        TDGL_TRY(comm_allreduce(ctx, ctx->part_tmp.p, NB, 0));
        hipLaunchKernelGGL(k_shift_mean, dim3(gv), dim3(BLOCK), 0, ctx->stream, no, ctx->part_tmp.p, inv_n, b);
        hipLaunchKernelGGL(k_dot_partial, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, no, b, b, ctx->part_pq.p);
        launch_sell<RESID, DOT_YY>(ctx, L0.A, x, b, nullptr, 0.0, 0.0, nullptr, r, run.part_rr[0]);
        TDGL_TRY(comm_allreduce(ctx, ctx->part_pq.p, NB, 0));
        TDGL_TRY(comm_allreduce(ctx, run.part_rr[0], NB, 0));
        hipLaunchKernelGGL(k_store_sum, dim3(1), dim3(BLOCK), 0, ctx->stream, ctx->part_pq.p, ctx->scal.p, (int)S_BB,
                           ctx->popt.rtol * ctx->popt.rtol);  // also scal[S_TOL2]
        hipLaunchKernelGGL(k_store_sum, dim3(1), dim3(BLOCK), 0, ctx->stream, run.part_rr[0], ctx->scal.p, (int)S_RR, 0.0);
        static const double init[2] = {-1.0, 0.0};  // S_CONV_IT: "not converged yet"; S_IT: 0
        static_assert(S_IT == S_CONV_IT + 1, "contiguous");
        HIP_TRY(ctx, hipMemcpyAsync(ctx->scal.p + S_CONV_IT, init, 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    if (distributed(ctx)) {  // psi failure flag and max d|psi|^2: identical decisions on all ranks
        hipLaunchKernelGGL(k_status_pack, dim3(1), dim3(BLOCK), 0, ctx->stream, ctx->psi_dmax_part.p,
                           ctx->psi_fail_part.p, ctx->psi_blocks, ctx->d_gstat.p);
        TDGL_TRY(comm_allreduce(ctx, ctx->d_gstat.p, 2, 1));
        hipLaunchKernelGGL(k_status_unpack, dim3(1), dim3(64), 0, ctx->stream, ctx->d_gstat.p, ctx->status_dev);
        ctx->psi_status_pending = false;  // d_status now holds the all-reduced outcome
    }
    // The edge currents the previous step owes (TDGL_CURRENTS_BEHIND_NEXT_LOOK) fill the wait: they read the accepted psi
    // and mu^n, which nothing queued so far has written -- the psi update writes the other buffer, mu changes after this
    // look.
    if (ctx->currents.take_behind_look(args.plan)) {
        TDGL_TRY(fetch_scalars(ctx, proj, nullptr, [&]() {
            launch_edge_currents(ctx, ctx->psi[ctx->loop.cur].p, ctx->mu.p, ctx->js.p, ctx->jn.p);
            return TDGL_OK;
        }));
    } else {
        TDGL_TRY(fetch_scalars(ctx, proj));
    }
    // The Gram row of the window's newest vector arrived with this status block.  Taken BEFORE an abandoned
    // solve returns: a second pcg_solve for the same step (after a psi retry) would compute it again, which
    // is harmless, but a window change in between would not be.
    if (proj) guess.take_gram_row(ctx->h_status.p);
    if (!after_first_sync(ctx->h_status.p)) {
        if (abandoned) *abandoned = true;
        return TDGL_OK;
    }
    const double bb = ctx->h_status.p->scal[S_BB];
    double rr = proj ? INFINITY : ctx->h_status.p->scal[S_RR];
    int it = 0;
    const double b_mean = proj ? ctx->h_status.p->gdot[2 * G_SB] * inv_n : 0.0;  // still inside b
    if (!(bb > 0.0)) {  // b = 0: the zero-mean solution is 0
        HIP_TRY(ctx, hipMemsetAsync(x, 0, ctx->n_pad * sizeof(double), ctx->stream));
        ctx->last_pcg_iters = 0;
        ctx->last_relres = 0.0;
        return TDGL_OK;
    }
    guess.mu_first_saved = false;
    if (proj && guess.count == 0) {  // no basis yet: keep mu^n so that a failed solve can be rolled back (run.inc)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->mu_prev.p, x, ctx->n_pad * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        guess.mu_first_saved = true;
    }
    VecSet vs{};
    const double *c_used = nullptr;  // the guess's coefficients, when it used vectors of the window
    if (proj) {
        // x0 = X c with G c = X^T b (host, K x K); then r0 = b - A x0.  ||r0||^2 stays on the device:
        // the first batch of iterations runs regardless (an update that finds the residual below
        // the tolerance freezes itself), and the first update records it for the statistics.
        TDGL_TRY(guess_apply(ctx, vs, gv, x, &c_used));
        launch_sell<RESID, DOT_YY>(ctx, L0.A, x, b, nullptr, b_mean, 0.0, nullptr, r, run.part_rr[0]);
        // (one process per GPU: ||r0||^2 is not summed over the ranks here -- nobody looks at it before the first
        // iteration, whose one sum of [r.z | ||r||^2 | z.w] takes it along: two sums per step less)
        if (distributed(ctx)) run.rr_reduced = false;
    }
    const double tol2 = ctx->popt.rtol * ctx->popt.rtol * bb;
    // The squared residual the iterations start from is known before anything is queued: with the projection guess
    // ||b - Y c||^2 from the Gram data, which the host already holds.  Both decisions below rest on it.
    const bool predict = proj && ctx->pcg_predict_from_guess && ctx->popt.check_every <= 0;
    const bool choose = precond_factors_available(ctx) && ctx->pd_choice != 2;
    const double est = !proj ? rr : (predict || choose) ? guess.residual_estimate(c_used) : NAN;
    // Size of the first batch.  Iterations queued beyond convergence freeze themselves but still cost their
    // launches (84 us each at 1M sites); a batch that is too short costs one more look per missing iteration
    // (~20 us).  The count of the previous solve is wrong in a third of the steps; the residual of the guess is a
    // much better predictor, divided by the contraction per iteration observed so far.
    run.predicted = std::max(1, ctx->last_pcg_iters);
    if (predict) {
        if (est > tol2 && std::isfinite(est)) {
            const double its = 0.5 * std::log10(est / tol2) / ctx->pcg_rate;
            run.predicted = (int)std::ceil(its - 0.25);  // (an iteration too many costs four times an iteration too few)
        } else {
            run.predicted = 1;
        }
        run.predicted = std::max(1, std::min(run.predicted, ctx->popt.max_iter));
    }
    // Which preconditioner: the cheaper PREDICTED solve (precond_cost).  Stationary / smoothly evolving states (guess
    // good to 1e-9: two or three V-cycles) stay with AMG; transients and the long-time regime (guess at 1e-4 .. 1e-6:
    // 8-13 V-cycles) take ONE application of the factors.
    run.use_pd = false;
    if (choose) {
        if (ctx->pd_choice == 1) {
            run.use_pd = true;
        } else if (std::isfinite(est) && est > tol2 && ctx->pd_t_apply_us > 0.0 && ctx->pd_t_vcycle_us > 0.0) {
            const PrecondCost cost = precond_cost(ctx, est, tol2);
            run.use_pd = cost.pd < cost.amg;
        }
        if (run.use_pd) run.predicted = 1;  // (an application too many costs five V-cycles: look after every one)
    }
    ctx->pd_last = run.use_pd;
    // (one-process-per-GPU mode runs level 0 in fp64 but shares the fp32-stored replicated levels)
    run.coarse32 = ctx->popt.precond_fp32 != 0 && ctx->levels.size() > 2;
    if (run.coarse32) TDGL_TRY(ensure_coarse_f32(ctx));
    run.it0 = 0;
    run.budget = ctx->popt.max_iter;
    // (the finish behind the look: one GPU -- the sums of the gauge and of the residual are complete as they stand)
    if (proj && !distributed(ctx) && !ctx->sync_shadow_disabled) {
        run.finish_slot = guess.next_slot(guess_window(ctx));
        run.b_mean = b_mean;
    }
    do {  // the phases: one CG run each
        TDGL_TRY(cg_iterate(run, tol2, it, rr));
    } while (rr > tol2 && !run.finished && next_phase(run, it));
    // zero-mean gauge, then ghost values of the solution for the edge kernels / next step
    const bool joins = proj && !(rr > tol2);
    if (run.finished != (joins && run.finish_queued))  // (cannot happen: both sides test the same numbers)
        TDGL_FAIL(ctx, TDGL_ERR_PCG, "Poisson solve: the device and the host disagree on convergence (rr %.17g, tol2 %.17g)", rr, tol2);
    if (!run.sum_x_fresh)
        hipLaunchKernelGGL(k_dot_partial, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, no, x, (const double *)nullptr, ctx->part_tmp.p);
    TDGL_TRY(comm_allreduce(ctx, ctx->part_tmp.p, NB, 0));
    if (joins) {
        // the solution joins the projection basis (replacing the oldest vector of a full window): the commit of
        // what the finish behind the last look has already written, or the finish itself
        const int slot = guess.push(guess_window(ctx));
        if (!run.finished)
            hipLaunchKernelGGL(k_finish_solution, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, no, (const double *)ctx->part_tmp.p,
                               inv_n, x, (const double *)b, b_mean, (const double *)r, guess.x[slot].p, guess.y[slot].p,
                               (const double *)nullptr);
    } else {
        hipLaunchKernelGGL(k_shift_mean, dim3(gv), dim3(BLOCK), 0, ctx->stream, no, ctx->part_tmp.p, inv_n, x);
    }
    if (args.mu_halo_pending && overlap_on(ctx))
        TDGL_TRY(comm_halo_start(ctx, x, 1));  // the step driver overlaps it with the interior edges
    else
        TDGL_TRY(comm_halo(ctx, x, 1));
    HIP_TRY(ctx, hipGetLastError());
    return pcg_note_solve(ctx, run, it, rr, bb, tol2);
}

extern "C" int tdgl_poisson_solve(tdgl_ctx *ctx, const double *rhs, double *mu_inout, int32_t *iters,
                                  double *relres) {
    CTX_GUARD(ctx);
    if (!rhs || !mu_inout) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null argument");
    if (ctx->levels.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "no AMG hierarchy: call tdgl_poisson_set_hierarchy");
    // b = -a * rhs in internal order
    std::vector<double> area(ctx->n_pad), b(ctx->n_pad, 0.0);
    HIP_TRY(ctx, hipMemcpy(area.data(), ctx->area.p, ctx->n_pad * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < ctx->n; ++i) b[i] = -area[i] * rhs[ctx->perm[i]];
    HIP_TRY(ctx, hipMemcpy(ctx->bvec.p, b.data(), ctx->n_pad * sizeof(double), hipMemcpyHostToDevice));
    // keep the context's own mu intact
    DevBuf<double> saved;
    HIP_TRY(ctx, saved.alloc(ctx->n_pad));
    HIP_TRY(ctx, hipMemcpy(saved.p, ctx->mu.p, ctx->n_pad * sizeof(double), hipMemcpyDeviceToDevice));
    TDGL_TRY(upload_sites(ctx, mu_inout, ctx->mu));
    const int saved_iters = ctx->last_pcg_iters;
    ctx->last_pcg_iters = 0;  // no prediction for a one-off solve
    MuSolveArgs one_off;
    int st = pcg_solve(ctx, one_off, [](const StepStatus *) { return true; }, nullptr);
    if (iters) *iters = ctx->last_pcg_iters;
    if (relres) *relres = ctx->last_relres;
    ctx->last_pcg_iters = saved_iters;
    int st2 = download_sites(ctx, ctx->mu.p, mu_inout);
    (void)hipMemcpy(ctx->mu.p, saved.p, ctx->n_pad * sizeof(double), hipMemcpyDeviceToDevice);
    return st != TDGL_OK ? st : st2;
}

// Per-kernel entry point (parity tests): the projection guess's dot-product pass on caller-supplied vectors
// (internal order = the caller's; no permutation).  out_pairs[2 a], [2 a + 1] = (hi, lo) of array a in
// {0: b . b, 1: sum b, 2 + j: y_j . b, 2 + 16 + j: y_newest . y_j}.
extern "C" int tdgl_guess_dots(tdgl_ctx *ctx, int32_t k, int64_t n, const double *vectors, const double *b, int32_t newest,
                               double *out_pairs) {
    CTX_GUARD(ctx);
    if (k < 1 || k > GK || n < 1 || !vectors || !b || !out_pairs || newest >= k) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_guess_dots: bad arguments");
    const int64_t n_pad = round_up(n, 2);
    DevBuf<double> dv, db, part;
    HIP_TRY(ctx, dv.alloc((int64_t)k * n_pad));
    HIP_TRY(ctx, db.alloc(n_pad));
    HIP_TRY(ctx, part.alloc(2 * G_ARRAYS * NB));
    for (int j = 0; j < k; ++j)
        HIP_TRY(ctx, hipMemcpy(dv.p + (int64_t)j * n_pad, vectors + (int64_t)j * n, n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(db.p, b, n * sizeof(double), hipMemcpyHostToDevice));
    VecSet vs{};
    vs.k = k;
    for (int j = 0; j < k; ++j) vs.p[j] = dv.p + (int64_t)j * n_pad;
    const int gg = std::min<int>(512, std::max<int64_t>(8, (n / 2 + BLOCK - 1) / BLOCK));
    launch_multi_dot(ctx, gg, n, db.p, vs, newest, part.p);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<double> h((size_t)2 * G_ARRAYS * NB);
    HIP_TRY(ctx, hipMemcpy(h.data(), part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int a = 0; a < G_ARRAYS; ++a) {
        DD t{0.0, 0.0};
        for (int i = 0; i < gg; ++i) t = dd_add(t, DD{h[(size_t)(2 * a) * NB + i], h[(size_t)(2 * a + 1) * NB + i]});
        out_pairs[2 * a] = t.hi;
        out_pairs[2 * a + 1] = t.lo;
    }
    return TDGL_OK;
}

// Per-kernel entry point (tests of the factor sweeps): ONE application of the factor preconditioner, z = M r, on vectors
// in the caller's site order, on buffers of its own -- the CG's vectors, partials and counters are not touched (the
// factors' own work vectors are: every application overwrites them).  *rz = r . z from k_dot_partial's partials (on the
// two-pass order, TDGL_PD_TWO_PASS: k_pd_scatter's), added up in index order.
extern "C" int tdgl_precond_apply(tdgl_ctx *ctx, const double *r, double *z, double *rz) {
    CTX_GUARD(ctx);
    if (!r || !z || !rz) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_precond_apply: null argument");
    // (a rank of a one-process-per-GPU run: its preconditioner is the rank-level dissection, whose application has collectives)
    if (ctx->n_own != ctx->n || distributed(ctx) || (ctx->direct && ctx->direct->n_local > 0))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_precond_apply: single-GPU contexts only (one process per GPU: the rank-level dissection is applied by every rank at once)");
    if (!ctx->direct || ctx->direct->levels == 0)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_precond_apply: no substructure factors (tdgl_poisson_set_substructure_precond)");
    if (!precond_factors_available(ctx))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_precond_apply: the factors are the mu solver, not the CG's preconditioner (tdgl_poisson_solve applies them)");
    DevBuf<double> in, out, part;
    HIP_TRY(ctx, in.alloc(ctx->n_pad));
    HIP_TRY(ctx, out.alloc(ctx->n_pad));
    HIP_TRY(ctx, part.alloc((size_t)ctx->npart));
    TDGL_TRY(upload_sites(ctx, r, in));
    precond_direct_apply(ctx, in.p, out.p, part.p, false);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<double> h((size_t)ctx->npart);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TDGL_TRY(download_sites(ctx, out.p, z));  // (synchronises the stream)
    double s = 0.0;
    for (double v : h) s += v;
    *rz = s;
    return TDGL_OK;
}
