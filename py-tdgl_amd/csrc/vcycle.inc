// The AMG V-cycle, preconditioner of the mu CG (poisson.inc): the launchers of its kernels, the cycle in fp64
// (vcycle_level) and in the stored precisions (vcycle0_f32 over ensure_f32's copies), and the entry points that apply one
// cycle.  Included by tdgl_hip.hip in front of factors.inc and poisson.inc; factors.inc and schur.inc share launch_csr.

// the collapsed chain applies while the smoother settings are the ones it was built for
static inline bool collapsed_on(const tdgl_ctx *ctx) {
    return ctx->tail_level >= 1 && ctx->tail_level < (int)ctx->levels.size() && ctx->popt.nu == ctx->tail_nu &&
           ctx->popt.smoother == ctx->tail_smoother && std::fabs(ctx->popt.cheb_lo - ctx->tail_cheb_lo) <= 1e-15;
}

// ---------------------------------------------------------------------------------------
// fixed-grid launch geometry: at most NB workgroups, a multiple of 8 (one share per XCD)
static inline void sell_fixed_grid(int n_slices, int *per_xcd, int *grid) {
    const int tiles = (n_slices + BLOCK / WAVE - 1) / (BLOCK / WAVE);
    *per_xcd = std::max(1, (tiles + XCDS - 1) / XCDS);
    *grid = std::min(NB, *per_xcd * XCDS);
}

static inline int vec_grid(int64_t n) { return (int)std::min<int64_t>(NB, (n + BLOCK - 1) / BLOCK); }

// grid of the CSR kernels: a multiple of 8 (xcd_tile needs whole rounds over the XCDs)
static inline int csr_grid(int64_t threads) { return (int)round_up(grid_for(threads), XCDS); }

// ---------------------------------------------------------------------------------------
// One launcher per kernel template: the only place where its hipLaunchKernelGGL stands.  Value, index and vector types
// are deduced from the pointers, so a call names the operator's arrays and the kernel's instantiation follows.  (The
// kernels launched from a single place need none: k_dense_matvec, k_dot_partial, k_smooth0, k_to_f32 / k_to_f16.)
template <int MODE, int DOT, class IT, class VT, class XT, class DT, class YT>
static void launch_sell_spmv(tdgl_ctx *ctx, int grid, int slice_end, int per_xcd, int tile_base, int64_t n_rows,
                             const int32_t *slice_off, const IT *cols, const VT *vals, const XT *x, const double *b,
                             const DT *dinv, double c1, double c2, double *d, YT *y, double *partial, const double *b2) {
    hipLaunchKernelGGL((k_sell_spmv<MODE, DOT, IT, VT, XT, YT, DT>), dim3(grid), dim3(BLOCK), 0, ctx->stream, slice_end,
                       per_xcd, tile_base, n_rows, slice_off, cols, vals, x, b, dinv, c1, c2, d, y, partial, b2);
}

template <int TMODE, class IT, class VT, class DT, class YT>
static void launch_sell_transfer(tdgl_ctx *ctx, const SellPattern &pat, const IT *cols, const int32_t *slice_base,
                                 const VT *vals, const double *x, const DT *dinv, const double *b, double c, YT *y) {
    int per_xcd, grid;
    sell_fixed_grid(pat.n_slices, &per_xcd, &grid);
    hipLaunchKernelGGL((k_sell_transfer<TMODE, VT, YT, IT, DT>), dim3(grid), dim3(BLOCK), 0, ctx->stream, pat.n_slices,
                       per_xcd, pat.n_rows, pat.slice_off.p, cols, slice_base, vals, x, dinv, b, c, y);
}

template <int LANES, int OP, int B, class VT>
static void launch_csr_multi(tdgl_ctx *ctx, int64_t n_rows, const int32_t *indptr, const int32_t *indices, const VT *data,
                             const double *x, const double *b, const double *dinv, double c0, double c1, double c2, double *d, double *y) {
    hipLaunchKernelGGL((k_csr_multi<LANES, OP, B, VT>), dim3(csr_grid(n_rows * LANES)), dim3(BLOCK), 0, ctx->stream,
                       n_rows, indptr, indices, data, x, b, dinv, c0, c1, c2, d, y);
}

template <int LANES, int B, class VT>
static void launch_csr_ax16(tdgl_ctx *ctx, int64_t n_rows, const int32_t *indptr, const int32_t *rowbase,
                            const uint16_t *offs, const VT *data, const double *x, double *y) {
    hipLaunchKernelGGL((k_csr_ax16<LANES, B, VT>), dim3(csr_grid(n_rows * LANES)), dim3(BLOCK), 0, ctx->stream, n_rows,
                       indptr, rowbase, offs, data, x, y);
}

// two operators in one launch: M1 on v1, and M2 (val2b: a second value array on its pattern) on v2
template <int LANES, int OP, int B1, int B2, class VT>
static void launch_csr_dual(tdgl_ctx *ctx, int64_t n_rows, const Csr &M1, const VT *val1, const double *v1, const Csr &M2,
                            const VT *val2, const VT *val2b, const double *v2, const double *b, const double *dinv, double c2,
                            double *d, double *y) {
    hipLaunchKernelGGL((k_csr_dual<LANES, OP, B1, B2, VT>), dim3(csr_grid(n_rows * LANES)), dim3(BLOCK), 0, ctx->stream, n_rows,
                       M1.indptr.p, M1.indices.p, val1, v1, M2.indptr.p, M2.indices.p, val2, val2b, v2, b, dinv, c2, d, y);
}

// y2 = M b and the two-step pre-smoothing x = S b with A, side by side
template <int LM, int BM, class VT>
static void launch_csr_down(tdgl_ctx *ctx, const Csr &M, const VT *Mv, const double *b, double *y2, const Csr &A,
                            const VT *Av, const double *dinv, double c0, double c1, double c2, double *d, double *x) {
    const int nbM = csr_grid(M.n_rows * LM), nbA = csr_grid(A.n_rows * 4);
    hipLaunchKernelGGL((k_csr_down<LM, BM, VT>), dim3(nbM + nbA), dim3(BLOCK), 0, ctx->stream, nbM, M.n_rows, M.indptr.p,
                       M.indices.p, Mv, b, y2, A.n_rows, A.indptr.p, A.indices.p, Av, dinv, c0, c1, c2, d, x);
}

// y = Wup b - Vneg e through the level's compact index forms
template <int LANES, int B1, int B2, class VT>
static void launch_mid_up(tdgl_ctx *ctx, const AmgLevel &L, const VT *wv, const VT *vv, const double *b, const double *e, double *y) {
    hipLaunchKernelGGL((k_mid_up<LANES, B1, B2, VT>), dim3(csr_grid(L.n * LANES)), dim3(BLOCK), 0, ctx->stream, L.n,
                       L.Wup.indptr.p, L.up_wbase.p, L.up_woff.p, wv, b, L.Vneg.indptr.p, L.up_vidx.p, vv, e, y);
}

template <int B, class VT, class IT>
static void launch_tail_up(tdgl_ctx *ctx, int64_t n_rows, const Csr &W, const IT *Wi, const VT *Wv, const double *x, int ldv,
                           const VT *V, const double *v, double *y) {
    hipLaunchKernelGGL((k_tail_up<B, VT, IT>), dim3(csr_grid(n_rows * WAVE)), dim3(BLOCK), 0, ctx->stream, n_rows, W.indptr.p,
                       Wi, Wv, x, ldv, V, v, y);
}

template <class VT> static void launch_dense_rows(tdgl_ctx *ctx, int rows, int ld, const VT *G, const double *x, double *y) {
    hipLaunchKernelGGL((k_dense_rows<VT>), dim3(rows), dim3(BLOCK), 0, ctx->stream, ld, G, x, y);
}

// The storage in force as a type: S.vals(M) is a CSR operator's value array in it, S.of(a64, a32) the matching one of the
// two copies of any other array.  in_storage(f32, f) calls the generic lambda f with Stored<float> or Stored<double>: the
// one place where a bool becomes the kernels' value type.
template <class VT> struct Stored {
    static const VT *vals(const Csr &M) { if constexpr (sizeof(VT) == 4) return M.data32.p; else return M.data.p; }
    static const VT *of(const DevBuf<double> &a64, const DevBuf<float> &a32) { if constexpr (sizeof(VT) == 4) return a32.p; else return a64.p; }
    static const VT *none() { return nullptr; }
};
template <class F> static inline void in_storage(bool f32, F &&f) { if (f32) f(Stored<float>{}); else f(Stored<double>{}); }

// ... and a level-0 operator of the stored-precision cycle in the form ensure_f32 chose for it: f(indices, values)
template <class I16, class F>
static inline void in_form(StoredForm form, const I16 *i16, const int32_t *i32, const half_t *v16, const float *v32, F &&f) {
    if (form == StoredForm::F16_I16) f(i16, v16);
    else if (form == StoredForm::F32_I16) f(i16, v32);
    else f(i32, v32);
}

// ---------------------------------------------------------------------------------------
// `part` (tile_range): a DOT kernel split into the ghost-free tiles (1) and the rest (2) gives
// each launch one half of the NB-entry partial array.
template <int MODE, int DOT>
static void launch_sell(tdgl_ctx *ctx, const SellF64 &A, const double *x, const double *b, const double *dinv, double c1,
                        double c2, double *d, double *y, double *partial, int part = 0) {
    int tile_base, slice_end, tiles;
    // (two distributed levels: the level-0 operator also has the rows of the first ghost layer, which only the
    // smoothing pass of the V-cycle uses; every launch through here is about the owned rows)
    const bool own_only = ctx->deep && !ctx->levels.empty() && &A == &ctx->levels[0]->A;
    const int64_t n_rows = own_only ? ctx->n_own : A.pat.n_rows;
    const int n_slices = own_only ? (int)((ctx->n_own + WAVE - 1) / WAVE) : A.pat.n_slices;
    tile_range(ctx, n_slices, part, &tile_base, &slice_end, &tiles);
    const int per_xcd = std::max(1, (tiles + XCDS - 1) / XCDS);
    int grid = std::min(NB, per_xcd * XCDS);
    // every writer of a partial array fills all of its entries (idle workgroups write 0), so
    // kernels with different natural grids can share one array
    if (DOT != DOT_NONE) {
        grid = part == 0 ? ctx->npart : NB / 2;  // (split launches: one-process-per-GPU mode, npart == NB)
        if (part == 2) partial += NB / 2;
    } else if (tiles <= 0) {
        return;
    }
    auto go = [&](auto cols) {
        launch_sell_spmv<MODE, DOT>(ctx, grid, slice_end, per_xcd, tile_base, n_rows, A.pat.slice_off.p, cols, A.vals.p, x, b,
                                    dinv, c1, c2, d, y, partial, nullptr);
    };
    if (A.pat.use16) go((const int16_t *)A.pat.cols16.p);
    else go((const int32_t *)A.pat.cols.p);
}

template <int TMODE>
static void launch_transfer(tdgl_ctx *ctx, const SellF64 &M, const double *x, const double *dinv, const double *b,
                            double c, double *y) {
    launch_sell_transfer<TMODE>(ctx, M.pat, M.pat.cols.p, nullptr, M.vals.p, x, dinv, b, c, y);
}

// a CSR operator in fp64 (also the substructured solve's and the Schur complement's products) ...
template <int LANES, int OP, int B = 2>
static void launch_csr(tdgl_ctx *ctx, const Csr &M, const double *x, const double *b, const double *dinv,
                       double c1, double c2, double *d, double *y) {
    launch_csr_multi<LANES, OP, B>(ctx, M.n_rows, M.indptr.p, M.indices.p, M.data.p, x, b, dinv, 0.0, c1, c2, d, y);
}

// ... and in the storage in force (c0: C_PRE2's first coefficient)
template <int LANES, int OP, int B = 2>
static void launch_csr(tdgl_ctx *ctx, const Csr &M, bool f32, const double *x, const double *b, const double *dinv,
                       double c1, double c2, double *d, double *y, double c0 = 0.0) {
    in_storage(f32, [&](auto S) {
        launch_csr_multi<LANES, OP, B>(ctx, M.n_rows, M.indptr.p, M.indices.p, S.vals(M), x, b, dinv, c0, c1, c2, d, y);
    });
}

// level operator application: SELL on level 0, 8-lane CSR below
static void level_smooth(tdgl_ctx *ctx, int k, AmgLevel &L, const double *x, const double *b, double c1,
                         double c2, double *d, double *y, double *dot_partial) {
    if (k > 0) launch_csr<4, C_SMOOTH, 4>(ctx, L.Ac, x, b, L.dinv.p, c1, c2, d, y);
    else if (dot_partial) launch_sell<SMOOTH, DOT_BY>(ctx, L.A, x, b, L.dinv.p, c1, c2, d, y, dot_partial);
    else launch_sell<SMOOTH, DOT_NONE>(ctx, L.A, x, b, L.dinv.p, c1, c2, d, y, nullptr);
}

static void level_residual(tdgl_ctx *ctx, int k, AmgLevel &L, const double *x, const double *b, double *r) {
    if (k == 0) launch_sell<RESID, DOT_NONE>(ctx, L.A, x, b, nullptr, 0.0, 0.0, nullptr, r, nullptr);
    else launch_csr<4, C_RESID, 4>(ctx, L.Ac, x, b, nullptr, 0.0, 0.0, nullptr, r);
}

static void poisson_spmv_level0(tdgl_ctx *ctx, const double *x, double *y) {
    launch_sell<AX, DOT_NONE>(ctx, ctx->levels[0]->A, x, nullptr, nullptr, 0.0, 0.0, nullptr, y, nullptr);
}

// Smoother coefficients: step k computes d = c1[k] d + c2[k] dinv (b - A x), x += d.
struct SmootherCoef {
    double c1[8], c2[8];
    bool need_d;
};

static inline int level_degree(const tdgl_ctx *ctx, int k) {
    return (k == 0 && ctx->popt.nu_fine > 0) ? ctx->popt.nu_fine : ctx->popt.nu;
}

static SmootherCoef smoother_coef(const tdgl_ctx *ctx, const AmgLevel &L, int nu) {
    SmootherCoef s{};
    if (ctx->popt.smoother == 0) {  // damped Jacobi, omega = (4/3)/rho
        for (int k = 0; k < nu; ++k) {
            s.c1[k] = 0.0;
            s.c2[k] = (4.0 / 3.0) / L.rho;
        }
        s.need_d = false;
        return s;
    }
    const double hi = L.rho, lo = ctx->popt.cheb_lo * L.rho;
    const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = theta / delta;
    double rho_k = 1.0 / sigma;
    s.c1[0] = 0.0;
    s.c2[0] = 1.0 / theta;
    for (int k = 1; k < nu; ++k) {
        const double rho_new = 1.0 / (2.0 * sigma - rho_k);
        s.c1[k] = rho_new * rho_k;
        s.c2[k] = 2.0 * rho_new / delta;
        rho_k = rho_new;
    }
    s.need_d = nu > 1;
    return s;
}

static inline bool fused_restriction_on(const tdgl_ctx *ctx, double c) {
    return ctx->fusedR.nnz > 0 && ctx->fusedR.n_cols == ctx->levels[0]->n_cols && std::fabs(ctx->fusedR_c - c) <= 1e-12 * c;
}

// ---------------------------------------------------------------------------------------
// One V-cycle on level k: returns the level buffer holding the correction for right-hand side b.  With dot_partial
// set, the last level-0 smoothing step also writes the NB partials of sum(b * result) there.  `f32`: the levels below
// level 0 read the reduced-precision copies of their operators where ensure_coarse_f32 has made them.
// vcycle_level (below) chooses among the forms a level can have; each form is one of the functions that follow.
static double *vcycle_level(tdgl_ctx *ctx, int k, const double *b, double *dot_partial, bool f32 = false);

// the coarsest level: dense pseudo-inverse
static double *cycle_coarsest(tdgl_ctx *ctx, AmgLevel &L, const double *b, double *dot_partial) {
    const int nc = (int)L.n;
    hipLaunchKernelGGL(k_dense_matvec, dim3(grid_for((int64_t)nc * WAVE)), dim3(BLOCK), 0, ctx->stream, nc, ctx->coarse_pinv.p, b, L.xa.p);
    if (dot_partial)  // single-level hierarchy
        hipLaunchKernelGGL(k_dot_partial, dim3(ctx->npart), dim3(BLOCK), 0, ctx->stream, L.n_pad, b, L.xa.p, dot_partial);
    return L.xa.p;
}

// the collapsed tail: everything from this level down through explicit operators, one or two launches (G, then W and V)
static double *cycle_tail(tdgl_ctx *ctx, AmgLevel &L, const double *b, bool f32) {
    const bool t32 = f32 && ctx->tailG32.n > 0;
    const int ldv = (int)ctx->tail_ldv;
    // (mode 1: y = G b lands right behind b, where the sparse operator's remapped columns point)
    double *yv = ctx->tail_mode == 0 ? L.xa.p : const_cast<double *>(b) + L.n_pad;
    in_storage(t32, [&](auto S) {
        launch_dense_rows(ctx, (int)ctx->tail_g_rows, (int)ctx->tail_ldg, S.of(ctx->tailG, ctx->tailG32), b, yv);
    });
    if (ctx->tail_mode != 1) return L.xa.p;
    const Csr &W = ctx->tailW;
    if (t32 && ctx->tailW_idx16.n > 0)
        launch_tail_up<8>(ctx, L.n, W, ctx->tailW_idx16.p, W.data32.p, b, ldv, ctx->tailV32.p, yv, L.xa.p);
    else
        in_storage(t32, [&](auto S) {
            launch_tail_up<8>(ctx, L.n, W, W.indices.p, S.vals(W), b, ldv, S.of(ctx->tailV, ctx->tailV32), yv, L.xa.p);
        });
    return L.xa.p;
}

// Level 0 with degree-1 smoothing (default): the pre-smoothed iterate x1 = c dinv b is never stored.
// r = b - A x1 gathers dinv*b directly, the prolongation kernel writes x = c dinv b + P e, one
// smoothing step follows.  Distributed: ONE exchange (ghosts of b) covers the residual; x is then
// valid on the ghost rows too.
static double *cycle_level0_degree1(tdgl_ctx *ctx, AmgLevel &L, const double *b, double c, double *dot_partial, bool f32) {
    AmgLevel &C = *ctx->levels[1];
    if (fused_restriction_on(ctx, c)) {
        // C.b = R (I - c A D^-1) b in one pass (tdgl_poisson_set_fused_restriction); one process
        // per GPU: ghosts of b first, the partial coarse right-hand sides summed after
        if (distributed(ctx)) (void)comm_halo(ctx, const_cast<double *>(b), 1);
        launch_csr<16, C_AX, 4>(ctx, ctx->fusedR, b, nullptr, nullptr, 0.0, 0.0, nullptr, C.b.p);
    } else {
        if (overlap_on(ctx)) {  // ghost-free rows run while the ghosts of b travel
            (void)comm_halo_start(ctx, const_cast<double *>(b), 1);
            launch_sell<RESID0, DOT_NONE>(ctx, L.A, b, nullptr, L.dinv.p, 0.0, c, nullptr, L.r.p, nullptr, 1);
            (void)comm_halo_wait(ctx);
            launch_sell<RESID0, DOT_NONE>(ctx, L.A, b, nullptr, L.dinv.p, 0.0, c, nullptr, L.r.p, nullptr, 2);
        } else {
            if (distributed(ctx)) (void)comm_halo(ctx, const_cast<double *>(b), 1);
            launch_sell<RESID0, DOT_NONE>(ctx, L.A, b, nullptr, L.dinv.p, 0.0, c, nullptr, L.r.p, nullptr);
        }
        launch_csr<16, C_AX>(ctx, L.R, L.r.p, nullptr, nullptr, 0.0, 0.0, nullptr, C.b.p);
    }
    if (distributed(ctx)) (void)comm_allreduce(ctx, C.b.p, C.n, 0);
    const double *xc = vcycle_level(ctx, 1, C.b.p, nullptr, f32);
    launch_transfer<T_BASE>(ctx, L.P, xc, L.dinv.p, b, c, L.xa.p);
    level_smooth(ctx, 0, L, L.xa.p, b, 0.0, c, nullptr, L.xb.p, dot_partial);
    return L.xb.p;
}

// An explicit level of the collapsed chain: M on the way down, W and V on the way up, one launch each -- the level's
// iterate x = S b is not needed at all.
static double *cycle_explicit(tdgl_ctx *ctx, int k, AmgLevel &L, const double *b, bool use32, bool f32) {
    AmgLevel &Cn = *ctx->levels[k + 1];
    launch_csr<32, C_AX, 8>(ctx, L.M, use32, b, nullptr, nullptr, 0.0, 0.0, nullptr, Cn.b.p);
    // two distributed levels: M holds this rank's owned level-1 columns -- the partial level-2 right-hand sides
    // are summed over ranks (fp32 like the operators that consume them: n2 values, 83 KB at 4M sites)
    if (L.explicit_only) (void)comm_allreduce_via_f32(ctx, Cn.b.p, Cn.n);
    const double *xn = vcycle_level(ctx, k + 1, Cn.b.p, nullptr, f32);
    // (8 lanes per row, 8 entries per lane in flight: measured best of 4 / 8 / 16 / 32 lanes and 3 - 8 entries)
    if (use32 && L.up_woff.n > 0 && L.up_w16.n > 0)
        launch_mid_up<8, 8, 2>(ctx, L, L.up_w16.p, L.up_v16.p, b, xn, L.xa.p);
    else if (use32 && L.up_woff.n > 0)
        launch_mid_up<8, 8, 2>(ctx, L, L.Wup.data32.p, L.Vneg.data32.p, b, xn, L.xa.p);
    else
        in_storage(use32, [&](auto S) {
            launch_csr_dual<16, D_RESTRICT, 4, 2>(ctx, L.n, L.Wup, S.vals(L.Wup), b, L.Vneg, S.vals(L.Vneg), S.none(), xn, nullptr,
                                                  nullptr, 0.0, nullptr, L.xa.p);
        });
    return L.xa.p;
}

// The smoothed level: pre-smooth from a zero guess, restrict, recurse, prolong with the first post-smoothing step,
// post-smooth.  `down1` (collapsed chain): the next right-hand side M b and the two-step pre-smoothing in one launch.
static double *cycle_smoothed(tdgl_ctx *ctx, int k, AmgLevel &L, const double *b, const SmootherCoef &sc, int nu, bool use32,
                              bool down1, double *dot_partial, bool f32) {
    AmgLevel &C = *ctx->levels[k + 1];
    double *d = sc.need_d ? L.d.p : nullptr;
    double *x = L.xa.p, *y = L.xb.p;
    // Level 0 is distributed (rows = owned sites): ghost entries of the iterate are refreshed
    // before every operator application.  Levels >= 1 are replicated on every rank.
    const bool dist0 = (k == 0) && distributed(ctx);
    const bool fused = k > 0 && L.fused;
    int s_first = 2;
    if (down1) {
        in_storage(use32, [&](auto S) {
            launch_csr_down<32, 8>(ctx, L.M, S.vals(L.M), b, C.b.p, L.Ac, S.vals(L.Ac), L.dinv.p, sc.c2[0], sc.c1[1], sc.c2[1], d, x);
        });
    } else if (k > 0 && nu >= 2) {  // steps 0 and 1 from a zero guess in one kernel
        launch_csr<4, C_PRE2, 4>(ctx, L.Ac, use32, b, nullptr, L.dinv.p, sc.c1[1], sc.c2[1], d, x, sc.c2[0]);
    } else {
        const int64_t n_rows = (k == 0) ? ctx->n_own : L.n;
        hipLaunchKernelGGL(k_smooth0, dim3(vec_grid(n_rows)), dim3(BLOCK), 0, ctx->stream, n_rows, sc.c2[0], L.dinv.p, b, d, x);
        s_first = 1;
    }
    for (int s = s_first; s < nu; ++s) {
        if (dist0) (void)comm_halo(ctx, x, 1);
        level_smooth(ctx, k, L, x, b, sc.c1[s], sc.c2[s], d, y, nullptr);
        std::swap(x, y);
    }
    if (down1) {
        // C.b is already there
    } else if (use32 || fused) {
        // C.b = R b - (R A) x in one launch
        in_storage(use32, [&](auto S) {
            launch_csr_dual<16, D_RESTRICT, 4, 8>(ctx, C.n, L.R, S.vals(L.R), b, L.RA, S.vals(L.RA), S.none(), x, nullptr, nullptr,
                                                  0.0, nullptr, C.b.p);
        });
    } else {
        if (dist0) (void)comm_halo(ctx, x, 1);
        level_residual(ctx, k, L, x, b, L.r.p);
        // restriction; in distributed mode R holds the owned fine columns only: the partial coarse
        // right-hand sides are summed over ranks
        launch_csr<16, C_AX>(ctx, L.R, L.r.p, nullptr, nullptr, 0.0, 0.0, nullptr, C.b.p);
        if (dist0) (void)comm_allreduce(ctx, C.b.p, C.n, 0);
    }
    const double *xc = vcycle_level(ctx, k + 1, C.b.p, nullptr, f32);
    int s_post = 0;
    if (use32 || fused) {
        // x' = x + P e and the first post-smoothing step in one launch (c1[0] = 0)
        in_storage(use32, [&](auto S) {
            launch_csr_dual<4, D_PSMOOTH, 4, 2>(ctx, L.n, L.Ac, S.vals(L.Ac), x, L.AP, S.vals(L.AP), S.of(L.APp, L.APp32), xc, b,
                                                L.dinv.p, sc.c2[0], d, y);
        });
        std::swap(x, y);
        s_post = 1;
    } else if (k == 0) {
        launch_transfer<T_ADD>(ctx, L.P, xc, nullptr, nullptr, 0.0, x);
    } else {
        launch_csr<4, C_ADD, 1>(ctx, L.Pc, xc, nullptr, nullptr, 0.0, 0.0, nullptr, x);
    }
    // post-smoothing (the polynomial restarts: c1[0] = 0)
    // (the prolongation also updated the ghost rows, so the first step needs no exchange)
    for (int s = s_post; s < nu; ++s) {
        if (dist0 && s > 0) (void)comm_halo(ctx, x, 1);
        if (use32) launch_csr<4, C_SMOOTH, 4>(ctx, L.Ac, true, x, b, L.dinv.p, sc.c1[s], sc.c2[s], d, y);
        else level_smooth(ctx, k, L, x, b, sc.c1[s], sc.c2[s], d, y, (s == nu - 1) ? dot_partial : nullptr);
        std::swap(x, y);
    }
    return x;
}

static double *vcycle_level(tdgl_ctx *ctx, int k, const double *b, double *dot_partial, bool f32) {
    AmgLevel &L = *ctx->levels[k];
    if (k == (int)ctx->levels.size() - 1) return cycle_coarsest(ctx, L, b, dot_partial);
    if (k >= 1 && collapsed_on(ctx) && k == ctx->tail_level) return cycle_tail(ctx, L, b, f32);
    const int nu = level_degree(ctx, k);
    const SmootherCoef sc = smoother_coef(ctx, L, nu);
    if (k == 0 && nu == 1) return cycle_level0_degree1(ctx, L, b, sc.c2[0], dot_partial, f32);
    const bool use32 = f32 && k > 0 && (L.explicit_only ? L.M.data32.n > 0 : (L.fused && L.Ac.data32.n > 0));
    // collapsed chain: the next right-hand side M b and the two-step pre-smoothing in one launch
    const bool down1 = k > 0 && nu == 2 && (L.fused || L.explicit_only) && L.M.nnz > 0 && collapsed_on(ctx) && k < ctx->tail_level &&
                       (!use32 || L.M.data32.n > 0);
    // ... and the way up as one launch too (explicit W, V)
    const bool up1 = down1 && L.Wup.nnz > 0 && (!use32 || L.Wup.data32.n > 0);
    if (up1) return cycle_explicit(ctx, k, L, b, use32, f32);
    return cycle_smoothed(ctx, k, L, b, sc, nu, use32, down1, dot_partial, f32);
}

// ---- mixed-precision preconditioner -----------------------------------------------------
// The V-cycle is an approximation of A^-1 by construction; storing its level-0 operators in
// fp32 perturbs it by ~1e-7 relative, far below its own approximation error, while the CG that
// it preconditions (A p, the residual recurrence, dot products, the convergence test) stays
// fp64 and converges to the same rtol.  What it buys: the three level-0 passes of the cycle
// stream 8 instead of 12 bytes per matrix entry and 4 instead of 8 per vector entry.
static inline bool precond_f32_on(const tdgl_ctx *ctx) {
    if (!ctx->popt.precond_fp32 || ctx->levels.size() < 2 || level_degree(ctx, 0) != 1) return false;
    return fused_restriction_on(ctx, smoother_coef(ctx, *ctx->levels[0], 1).c2[0]);
}

// a copy of n fp64 values in dst's type (float / half_t)
template <class T> static int convert(tdgl_ctx *ctx, const double *src, DevBuf<T> &dst, int64_t n) {
    HIP_TRY(ctx, dst.alloc(std::max<int64_t>(n, 1)));
    if (n <= 0) return TDGL_OK;
    if constexpr (std::is_same<T, float>::value) hipLaunchKernelGGL(k_to_f32, dim3(grid_for(n)), dim3(BLOCK), 0, ctx->stream, n, src, dst.p);
    else hipLaunchKernelGGL(k_to_f16, dim3(grid_for(n)), dim3(BLOCK), 0, ctx->stream, n, src, dst.p);
    return TDGL_OK;
}

// fp32 copies of the intermediate-level operators (any mode, also one-process-per-GPU: these
// levels are replicated on every rank)
static int ensure_coarse_f32(tdgl_ctx *ctx) {
    if (ctx->coarse32_ready) return TDGL_OK;
    ctx->pcg_epoch += 1;
    if (ctx->tail_level >= 1) {
        TDGL_TRY(convert(ctx, ctx->tailG.p, ctx->tailG32, (int64_t)ctx->tailG.n));
        if (ctx->tail_mode == 1) {
            if (ctx->tailV.n > 0) TDGL_TRY(convert(ctx, ctx->tailV.p, ctx->tailV32, (int64_t)ctx->tailV.n));
            else ctx->tailV32.release();
            TDGL_TRY(convert(ctx, ctx->tailW.data.p, ctx->tailW.data32, ctx->tailW.nnz));
        }
    } else {
        ctx->tailG32.release();
    }
    for (size_t k = 1; k + 1 < ctx->levels.size(); ++k) {  // levels with pre-multiplied transfers
        AmgLevel &C = *ctx->levels[k];
        if (!C.fused && !C.explicit_only) continue;
        if (C.M.nnz > 0) TDGL_TRY(convert(ctx, C.M.data.p, C.M.data32, C.M.nnz));
        if (C.Wup.nnz > 0) {
            TDGL_TRY(convert(ctx, C.Wup.data.p, C.Wup.data32, C.Wup.nnz));
            TDGL_TRY(convert(ctx, C.Vneg.data.p, C.Vneg.data32, C.Vneg.nnz));
            C.up_w16.release();
            if (ctx->popt.precond_fp32 >= 2 && C.up_woff.n > 0) {  // (entries are O(1))
                TDGL_TRY(convert(ctx, C.Wup.data.p, C.up_w16, C.Wup.nnz));
                TDGL_TRY(convert(ctx, C.Vneg.data.p, C.up_v16, C.Vneg.nnz));
            }
        }
        if (C.explicit_only) continue;
        for (Csr *M : {&C.Ac, &C.R, &C.RA, &C.AP}) TDGL_TRY(convert(ctx, M->data.p, M->data32, M->nnz));
        TDGL_TRY(convert(ctx, C.APp.p, C.APp32, C.AP.nnz));
    }
    HIP_TRY(ctx, hipGetLastError());
    ctx->coarse32_ready = true;
    return TDGL_OK;
}

// ... and of the level-0 operators; decides the form (value and index types) in which the stored-precision cycle reads
// each of them
static int ensure_f32(tdgl_ctx *ctx) {
    TDGL_TRY(ensure_coarse_f32(ctx));
    if (ctx->f32_ready) return TDGL_OK;
    ctx->pcg_epoch += 1;
    AmgLevel &L = *ctx->levels[0];
    TDGL_TRY(convert(ctx, L.A.vals.p, L.A32, L.A.pat.n_slots));
    TDGL_TRY(convert(ctx, L.P.vals.p, L.P32, L.P.pat.n_slots));
    TDGL_TRY(convert(ctx, L.dinv.p, L.dinv32, L.n_pad));
    TDGL_TRY(convert(ctx, ctx->fusedR.data.p, ctx->fusedR32, ctx->fusedR.nnz));
    // binary16 copies of the three level-0 operator streams
    // (popt.precond_fp32 >= 2; needs the 16-bit index forms, i.e. RCM-numbered single-GPU operators, and
    // entries inside binary16's range: |a| < 3e4 -- entries below 6e-5 lose digits, which a
    // preconditioner does not mind)
    ctx->level0_f16 = ctx->popt.precond_fp32 >= 2 && ctx->fusedR_off16.n > 0 &&
                      L.P.pat.use_off16 && L.A.pat.use16 && ctx->level0_absmax < 3.0e4;
    if (ctx->level0_f16) {
        TDGL_TRY(convert(ctx, L.A.vals.p, L.A16, L.A.pat.n_slots));
        TDGL_TRY(convert(ctx, L.P.vals.p, L.P16, L.P.pat.n_slots));
        TDGL_TRY(convert(ctx, ctx->fusedR.data.p, ctx->fusedR16, ctx->fusedR.nnz));
    }
    auto form = [&](bool idx16) { return ctx->level0_f16 ? StoredForm::F16_I16 : idx16 ? StoredForm::F32_I16 : StoredForm::F32_I32; };
    ctx->form_A = form(L.A.pat.use16);
    ctx->form_P = form(L.P.pat.use_off16);
    ctx->form_R = form(ctx->fusedR_off16.n > 0);
    HIP_TRY(ctx, L.x32a.alloc(L.n_pad));
    HIP_TRY(ctx, L.x32b.alloc(L.n_pad));
    HIP_TRY(ctx, hipGetLastError());
    ctx->f32_ready = true;
    return TDGL_OK;
}

// What vcycle0_f32 delivers besides the fp32 z it returns: the partials of r.z (RZ); those of q.z behind them as well
// (RZ_QZ: DOT_BY2, the flexible CG's z_new . q_old); z on the owned rows AND the first ghost layer (A's rows) without
// sums (GHOSTS_NO_SUMS); r.z and z as an fp64 vector in z64 (F64_RZ: its ghost entries are exchanged as doubles before A z).
struct Cycle0Out {
    enum Kind { RZ, RZ_QZ, GHOSTS_NO_SUMS, F64_RZ } kind;
    double *z64;
    const double *q;
    static Cycle0Out rz() { return {RZ, nullptr, nullptr}; }
    static Cycle0Out rz_qz(const double *q) { return {RZ_QZ, nullptr, q}; }
    static Cycle0Out ghosts_no_sums() { return {GHOSTS_NO_SUMS, nullptr, nullptr}; }
    static Cycle0Out f64_rz(double *z64) { return {F64_RZ, z64, nullptr}; }
};

// the level-0 smoothing pass of the stored-precision cycle: y = x32a + c dinv (r - A x32a), with the sums DOT asks for
template <int DOT, class YT>
static void launch_smooth_stored(tdgl_ctx *ctx, AmgLevel &L, const double *r, double c, YT *y, double *dot_partial, const double *q) {
    const SellPattern &pat = L.A.pat;
    int per_xcd, grid;
    sell_fixed_grid(pat.n_slices, &per_xcd, &grid);
    in_form(ctx->form_A, pat.cols16.p, pat.cols.p, L.A16.p, L.A32.p, [&](auto cols, auto vals) {
        launch_sell_spmv<SMOOTH, DOT>(ctx, ctx->npart, pat.n_slices, per_xcd, 0, pat.n_rows, pat.slice_off.p, cols, vals,
                                      (const float *)L.x32a.p, r, (const float *)L.dinv32.p, 0.0, c, nullptr, y, dot_partial, q);
    });
}

// z = M^-1 r with the level-0 part in fp32 (degree-1 smoothing, fused restriction); writes the
// NB partials of r.z to dot_partial and returns z (fp32, level-0 length); `out`: see Cycle0Out.
// In one-process-per-GPU mode the ghosts of r are refreshed first and the partial coarse right-hand
// sides are summed over ranks.
static const float *vcycle0_f32(tdgl_ctx *ctx, double *r, double *dot_partial, Cycle0Out out) {
    AmgLevel &L = *ctx->levels[0], &C = *ctx->levels[1];
    const double c = smoother_coef(ctx, L, 1).c2[0];
    // rows [r0, r1) of the restriction C.b = F r
    auto restrict_rows = [&](int64_t r0, int64_t r1) {
        const int64_t nr = r1 - r0;
        if (nr <= 0) return;
        const Csr &F = ctx->fusedR;
        if (ctx->form_R == StoredForm::F32_I32)
            launch_csr_multi<16, C_AX, 4>(ctx, nr, F.indptr.p + r0, F.indices.p, ctx->fusedR32.p, r, nullptr, nullptr, 0.0, 0.0, 0.0,
                                          nullptr, C.b.p + r0);
        else if (ctx->form_R == StoredForm::F32_I16)
            launch_csr_ax16<16, 4>(ctx, nr, F.indptr.p + r0, ctx->fusedR_base.p + r0, ctx->fusedR_off16.p, ctx->fusedR32.p, r, C.b.p + r0);
        else
            launch_csr_ax16<16, 4>(ctx, nr, F.indptr.p + r0, ctx->fusedR_base.p + r0, ctx->fusedR_off16.p, ctx->fusedR16.p, r, C.b.p + r0);
    };
    const int64_t nF = ctx->fusedR.n_rows;
    if (ctx->deep && ipc_on(ctx) && ctx->overlap && ctx->l1_interior >= 4096 && !ctx->deep_nbrs.empty()) {
        // the ONE vector exchange of the iteration, hidden: the neighbours' values travel while the level-1 rows whose
        // restriction reads owned entries only are formed (all on this stream: sending launch, ghost-free rows,
        // receiving launch, the rest)
        (void)comm_halo_deep(ctx, r, /*split_phase=*/1);
        restrict_rows(0, ctx->l1_interior);
        (void)comm_halo_deep_wait(ctx, r);
        restrict_rows(ctx->l1_interior, nF);
    } else {
        if (ctx->deep) (void)comm_halo_deep(ctx, r);  // the ONE vector exchange of the iteration
        else if (distributed(ctx)) (void)comm_halo(ctx, r, 1);
        restrict_rows(0, nF);
    }
    // (two distributed levels: b1 is complete on this rank's entries; the sum over ranks happens one level down)
    if (distributed(ctx) && !ctx->deep) (void)comm_allreduce_via_f32(ctx, C.b.p, C.n);
    const double *xc = vcycle_level(ctx, 1, C.b.p, nullptr, /*f32=*/true);
    const SellPattern &pp = L.P.pat;
    in_form(ctx->form_P, pp.offs16.p, pp.cols.p, L.P16.p, L.P32.p, [&](auto cols, auto vals) {
        launch_sell_transfer<T_BASE>(ctx, pp, cols, ctx->form_P == StoredForm::F32_I32 ? nullptr : pp.slice_base.p, vals, xc,
                                     L.dinv32.p, r, c, L.x32a.p);
    });
    // (two distributed levels, or the caller forms its sums later: r.z is formed over the owned rows by the pass that
    // computes w = A z; z stays in fp32 like on one GPU: nothing exchanges it any more)
    if (ctx->deep || out.kind == Cycle0Out::GHOSTS_NO_SUMS) launch_smooth_stored<DOT_NONE>(ctx, L, r, c, L.x32b.p, dot_partial, nullptr);
    else if (out.kind == Cycle0Out::RZ_QZ) launch_smooth_stored<DOT_BY2>(ctx, L, r, c, L.x32b.p, dot_partial, out.q);  // (single GPU)
    else if (out.kind == Cycle0Out::F64_RZ) launch_smooth_stored<DOT_BY>(ctx, L, r, c, out.z64, dot_partial, nullptr);
    else launch_smooth_stored<DOT_BY>(ctx, L, r, c, L.x32b.p, dot_partial, nullptr);
    return L.x32b.p;
}

extern "C" int tdgl_vcycle(tdgl_ctx *ctx, const double *r, double *z) {
    CTX_GUARD(ctx);
    if (!r || !z) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null argument");
    if (ctx->levels.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "no AMG hierarchy");
    DevBuf<double> in;
    HIP_TRY(ctx, in.alloc(ctx->n_pad));
    TDGL_TRY(upload_sites(ctx, r, in));
    const double *res = vcycle_level(ctx, 0, in.p, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    return download_sites(ctx, res, z);
}

// Per-kernel entry point (tests of the stored-precision cycle): ONE application of the V-cycle the CG applies above the
// fp64 one -- vcycle0_f32 with the operators in the storage ensure_f32 gives them -- on vectors in the caller's site
// order.  The residual copy and the dot partials are this call's own: the CG's vectors, partials and counters are not
// touched (the cycle's work vectors are: every application overwrites them).  z = the stored fp32 z widened; *rz (and
// *qz with q, the flexible CG's DOT_BY2 form) = the smoothing pass's partials added up in index order.
extern "C" int tdgl_vcycle_stored(tdgl_ctx *ctx, const double *r, const double *q, double *z, double *rz, double *qz) {
    CTX_GUARD(ctx);
    if (!r || !z || !rz || (q && !qz)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_vcycle_stored: null argument");
    // (a rank of a one-process-per-GPU run: its cycle exchanges ghosts and sums the coarse right-hand sides over ranks)
    if (ctx->n_own != ctx->n || distributed(ctx) || ctx->deep)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_vcycle_stored: single-GPU contexts only (one process per GPU: the cycle has collectives)");
    if (ctx->levels.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_vcycle_stored: no AMG hierarchy");
    if (!precond_f32_on(ctx)) {
        const char *why = !ctx->popt.precond_fp32        ? "the operators are stored in fp64 (precond_fp32 = 0)"
                          : ctx->levels.size() < 2       ? "the hierarchy has a single level"
                          : level_degree(ctx, 0) != 1    ? "the level-0 smoother has a degree other than 1"
                                                         : "no fused restriction for the level-0 coefficient in use";
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_vcycle_stored: the CG applies the fp64 cycle here: %s (tdgl_vcycle)", why);
    }
    TDGL_TRY(ensure_f32(ctx));
    AmgLevel &L = *ctx->levels[0];
    DevBuf<double> in, qin, part;
    HIP_TRY(ctx, in.alloc(L.n_pad));
    HIP_TRY(ctx, part.alloc(3 * NB));
    TDGL_TRY(upload_sites(ctx, r, in));
    if (q) {
        HIP_TRY(ctx, qin.alloc(L.n_pad));
        TDGL_TRY(upload_sites(ctx, q, qin));
    }
    const float *z32 = vcycle0_f32(ctx, in.p, part.p, q ? Cycle0Out::rz_qz(qin.p) : Cycle0Out::rz());
    HIP_TRY(ctx, hipGetLastError());
    std::vector<double> h((size_t)3 * NB);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<float> zf((size_t)ctx->n);
    TDGL_TRY(download_sites(ctx, z32, zf.data()));  // (synchronises the stream)
    for (int64_t i = 0; i < ctx->n; ++i) z[i] = (double)zf[i];
    double s = 0.0, s2 = 0.0;
    for (int i = 0; i < ctx->npart; ++i) {
        s += h[i];
        s2 += h[(size_t)2 * NB + i];
    }
    *rz = s;
    if (q) *qz = s2;
    return TDGL_OK;
}

// Which index form each operator of the stored-precision cycle was built with (read-only; tests assert the path they
// mean to run).  out[TDGL_INDEX_FORMS_LEN]: see include/tdgl_hip.h.
extern "C" int tdgl_get_poisson_index_forms(tdgl_ctx *ctx, int32_t *out) {
    if (!ctx || !out) return TDGL_ERR_ARG;
    for (int i = 0; i < TDGL_INDEX_FORMS_LEN; ++i) out[i] = -1;
    const int nl = (int)ctx->levels.size();
    out[5] = nl;
    out[8] = ctx->lap_pat.use16 ? 1 : 0;
    if (nl == 0) return TDGL_OK;
    const AmgLevel &L = *ctx->levels[0];
    out[0] = L.A.pat.use16 ? 1 : 0;
    if (nl > 1) out[1] = L.P.pat.use_off16 ? 1 : 0;
    if (ctx->fusedR.nnz > 0) out[2] = ctx->fusedR_off16.n > 0 ? 1 : 0;
    if (ctx->tail_level >= 1 && ctx->tail_mode == 1) out[3] = ctx->tailW_idx16.n > 0 ? 1 : 0;
    out[4] = (ctx->f32_ready && ctx->level0_f16) ? 1 : 0;
    out[6] = ctx->tail_level;
    out[7] = ctx->tail_level >= 1 ? ctx->tail_mode : -1;
    for (int k = 1; k + 1 < nl && 8 + k < TDGL_INDEX_FORMS_LEN; ++k) {
        const AmgLevel &M = *ctx->levels[k];
        if (M.Wup.nnz > 0) out[8 + k] = (M.up_woff.n > 0 ? 1 : 0) | (ctx->coarse32_ready && M.up_w16.n > 0 ? 2 : 0);
    }
    return TDGL_OK;
}
