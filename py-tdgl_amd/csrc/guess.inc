// Initial guess of the mu solve by projection onto the previous solutions (popt.extrapolate == 3; kernels.inc "initial
// guess by projection"), the host half: GuessBasis (tdgl_internal.h) owns the window, pcg_solve (poisson.inc) drives it.

constexpr int GUESS_DEFAULT = 12;  // window of the projection guess when the options say 0
static inline int guess_window(const tdgl_ctx *ctx) {
    return std::min(GK, std::max(1, ctx->popt.guess_window > 0 ? ctx->popt.guess_window : GUESS_DEFAULT));
}

// Relative pivot below which a window vector counts as dependent on the newer ones (solve_gram_dd).  The
// Gram entries are double-double sums of stored fp64 vectors (~1e-30 relative); what limits the usable
// depth is how well y_j = b_j - r_j represents A x_j: the CG's recurrence residual follows the true one to
// ~1e-13 ||b||, i.e. components below 1e-13 of a vector are not images of the x_j any more: cut = 1e-24.
// One process per GPU: up to 16 ranks gather each other's totals exactly (k_guess_rank_totals); beyond, hi and
// lo parts are all-reduced separately and the sums are fp64-accurate only.
static inline double guess_cut(const tdgl_ctx *ctx) {
    return (distributed(ctx) && !guess_rank_totals(ctx)) ? 1e-13 : 1e-24;
}

// ---- host double-double arithmetic for the K x K system of the projection guess -------------------
// (hi, lo) pairs with |lo| <= ulp(hi) / 2, ~32 significant digits.  Compiled without -ffast-math; the
// error-free transformations below rely on IEEE semantics (std::fma = one rounding).  None of them has a
// product feeding a sum it must not be fused with (the two-sums are additions only), so the host
// compiler's contraction default is harmless here -- unlike in the device versions (kernels.inc).
struct DD {
    double hi, lo;
};
static inline DD dd_make(double a, double b = 0.0) {
    const double s = a + b;
    return DD{s, b - (s - a)};
}
static inline DD dd_two_sum(double a, double b) {
    const double s = a + b, v = s - a;
    return DD{s, (a - (s - v)) + (b - v)};
}
static inline DD dd_add(DD a, DD b) {
    DD s = dd_two_sum(a.hi, b.hi);
    const DD t = dd_two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = dd_make(s.hi, s.lo);
    s.lo += t.lo;
    return dd_make(s.hi, s.lo);
}
static inline DD dd_neg(DD a) { return DD{-a.hi, -a.lo}; }
static inline DD dd_sub(DD a, DD b) { return dd_add(a, dd_neg(b)); }
static inline DD dd_mul(DD a, DD b) {
    const double p = a.hi * b.hi;
    const double e = std::fma(a.hi, b.hi, -p) + (a.hi * b.lo + a.lo * b.hi);
    return dd_make(p, e);
}
// v - a b with one renormalisation (the inner loop of the factorisation: ~16 flops instead of ~45 for
// dd_sub(v, dd_mul(a, b)); relative error ~1e-31)
static inline DD dd_fms(DD v, DD a, DD b) {
    const double p = a.hi * b.hi;
    const double e = std::fma(a.hi, b.hi, -p) + (a.hi * b.lo + a.lo * b.hi);
    const double s = v.hi - p;
    const double w = s - v.hi;
    const double err = (v.hi - (s - w)) + (-p - w);
    const double l = (v.lo - e) + err;
    const double hi = s + l;
    return DD{hi, l - (hi - s)};
}
static inline DD dd_div(DD a, DD b) {
    const double q1 = a.hi / b.hi;
    DD r = dd_sub(a, dd_mul(b, DD{q1, 0.0}));
    const double q2 = r.hi / b.hi;
    r = dd_sub(r, dd_mul(b, DD{q2, 0.0}));
    const double q3 = r.hi / b.hi;
    return dd_add(dd_make(q1, q2), DD{q3, 0.0});
}

// c = argmin || b - Y c ||_2 from the Gram matrix G = Y^T Y and g = Y^T b (double-double, window order:
// oldest first).  L D L^T WITHOUT pivoting, taken from the NEWEST vector to the oldest; a vector whose
// pivot falls below `cut` times its own squared norm -- it lies in the span of the newer ones to within
// sqrt(cut) -- is left out (c_j = 0).  Returns the number of vectors used, or -1 when the matrix is
// unusable (non-positive diagonal, non-finite entries).
static int solve_gram_dd(int k, const double G[GK][GK][2], const double g[GK][2], double cut, double *c) {
    DD L[GK][GK], d[GK], z[GK];
    int used[GK], nu = 0;
    for (int j = 0; j < k; ++j) {
        c[j] = 0.0;
        if (!(G[j][j][0] > 0.0) || !std::isfinite(G[j][j][0]) || !std::isfinite(g[j][0])) return -1;
    }
    // order: position q in the factorisation <-> window index idx(q) = k - 1 - q
    for (int q = 0; q < k; ++q) {
        const int j = k - 1 - q;
        // row of L against the vectors already taken
        DD piv = DD{G[j][j][0], G[j][j][1]};
        DD row[GK], rowd[GK];  // rowd[t] = row[t] d[t] (the un-normalised entry: no division needed to get it)
        for (int a = 0; a < nu; ++a) {
            const int ja = used[a];
            DD v = DD{G[j][ja][0], G[j][ja][1]};
            for (int t = 0; t < a; ++t) v = dd_fms(v, rowd[t], L[a][t]);
            if (!std::isfinite(v.hi)) return -1;
            rowd[a] = v;
            row[a] = dd_div(v, d[a]);
            piv = dd_fms(piv, row[a], v);
        }
        if (!(piv.hi > cut * G[j][j][0])) continue;  // numerically dependent on the newer vectors
        for (int a = 0; a < nu; ++a) L[nu][a] = row[a];
        d[nu] = piv;
        used[nu++] = j;
    }
    if (nu == 0) return 0;
    // forward substitution L z = g, z /= d, back substitution L^T c = z
    for (int a = 0; a < nu; ++a) {
        DD v = DD{g[used[a]][0], g[used[a]][1]};
        for (int t = 0; t < a; ++t) v = dd_fms(v, L[a][t], z[t]);
        z[a] = v;
    }
    for (int a = 0; a < nu; ++a) z[a] = dd_div(z[a], d[a]);
    for (int a = nu - 1; a >= 0; --a) {
        DD v = z[a];
        for (int t = a + 1; t < nu; ++t) v = dd_fms(v, L[t][a], z[t]);
        z[a] = v;
        c[used[a]] = v.hi;
    }
    for (int j = 0; j < k; ++j)
        if (!std::isfinite(c[j])) return -1;
    return nu;
}

// host-only: the K x K solve behind the projection guess, exported for the CPU tests.  G and g as
// (hi, lo) pairs, row-major [k][k][2] / [k][2]; *used receives the number of vectors kept.
extern "C" int tdgl_host_solve_gram(int32_t k, const double *G_pairs, const double *g_pairs, double cut, double *c,
                                    int32_t *used) {
    if (k < 1 || k > GK || !G_pairs || !g_pairs || !c) return TDGL_ERR_ARG;
    double G[GK][GK][2], g[GK][2];
    for (int i = 0; i < k; ++i) {
        for (int j = 0; j < k; ++j) {
            G[i][j][0] = G_pairs[(i * k + j) * 2];
            G[i][j][1] = G_pairs[(i * k + j) * 2 + 1];
        }
        g[i][0] = g_pairs[2 * i];
        g[i][1] = g_pairs[2 * i + 1];
    }
    const int nu = solve_gram_dd(k, G, g, cut, c);
    if (used) *used = nu;
    return nu >= 0 ? TDGL_OK : TDGL_ERR_ARG;
}

// ---- the window ---------------------------------------------------------------------------------
// the oldest `drop` vectors leave: slots, right-hand sides and Gram entries move down
void GuessBasis::drop_oldest(int drop) {
    for (int i = 0; i + drop < count; ++i) {
        slot[i] = slot[i + drop];
        for (int h = 0; h < 2; ++h) rhs[i][h] = rhs[i + drop][h];
        for (int j = 0; j + drop < count; ++j)
            for (int h = 0; h < 2; ++h) G[i][j][h] = G[i + drop][j + drop][h];
    }
    count -= drop;
}

// buffers for the window the options ask for; a window that shrank keeps the newest vectors
int GuessBasis::ensure(tdgl_ctx *ctx) {
    const int gw = guess_window(ctx);
    for (int j = 0; j < gw; ++j) {
        if (x[j].n == 0) HIP_TRY(ctx, x[j].alloc(ctx->n_pad));
        if (y[j].n == 0) HIP_TRY(ctx, y[j].alloc(ctx->n_pad));
    }
    if (part_dot.n == 0) {
        HIP_TRY(ctx, part_dot.alloc(2 * G_ARRAYS * NB));
        HIP_TRY(ctx, d_dot.alloc(2 * G_ARRAYS));
        HIP_TRY(ctx, part_dot_rank.alloc(2 * G_ARRAYS * G_RANK_STRIDE));  // (zeroed; a rank only ever writes its own position)
    }
    if (count > gw) drop_oldest(count - gw);
    return TDGL_OK;
}

// the Gram row of the window's newest vector, which arrived with the first status block of the solve after its own
void GuessBasis::take_gram_row(const StepStatus *st) {
    if (!row_pending) return;
    const int kn = count - 1;
    for (int j = 0; j < count; ++j)
        for (int h = 0; h < 2; ++h) G[kn][j][h] = G[j][kn][h] = st->gdot[2 * (G_N0 + j) + h];
    row_pending = false;
}

// the new right-hand side against the window: rhs[j] = y_j . b and bb = ||b - mean||^2
void GuessBasis::load_rhs(const StepStatus *st, int64_t n_global) {
    for (int j = 0; j < count; ++j) {
        rhs[j][0] = st->gdot[2 * (G_Y0 + j)];
        rhs[j][1] = st->gdot[2 * (G_Y0 + j) + 1];
    }
    // ||b - mean||^2 = b.b - (sum b)^2 / n in double-double: the diagonal Gram entry if this solve joins the window
    const DD sb = DD{st->gdot[2 * G_SB], st->gdot[2 * G_SB + 1]};
    const DD q = dd_sub(DD{st->gdot[2 * G_BB], st->gdot[2 * G_BB + 1]}, dd_div(dd_mul(sb, sb), DD{(double)n_global, 0.0}));
    bb[0] = q.hi;
    bb[1] = q.lo;
}

// the coefficients of the guess x0 = X c (solve_gram_dd); returns the number of vectors used
int GuessBasis::solve(double cut, double *c) const { return count > 0 ? solve_gram_dd(count, G, rhs, cut, c) : 0; }

// ||b - Y c||^2 = b.b - 2 c.g + c.G c from the Gram data (double-double: it is 8-17 decades below b.b); c == NULL:
// no vector was used, the guess is the iterate as it stands
double GuessBasis::residual_estimate(const double *c) const {
    DD rr0 = DD{bb[0], bb[1]};
    if (c) {
        for (int i = 0; i < count; ++i) {
            if (c[i] == 0.0) continue;
            DD row = dd_mul(DD{-2.0 * c[i], 0.0}, DD{rhs[i][0], rhs[i][1]});
            for (int j = 0; j < count; ++j)
                if (c[j] != 0.0) row = dd_add(row, dd_mul(dd_mul(DD{c[i], 0.0}, DD{c[j], 0.0}), DD{G[i][j][0], G[i][j][1]}));
            rr0 = dd_add(rr0, row);
        }
    }
    return rr0.hi;
}

// The solution of the solve whose right-hand side was loaded joins the window, replacing the oldest vector of a full
// one; returns its slot (x[slot], y[slot] are the caller's to fill).  The Gram row of the new pair
// y_new = (b - mean) - r_final comes with the next solve's dot-product pass: until then the placeholders below --
// y_j . b, off by y_j . r_final -- are never used.
// The slot itself is known beforehand (next_slot): a solution may be written there before the host has decided
// that it joins -- the slot is free, or holds the oldest vector, which the guess of this solve has already used.
int GuessBasis::next_slot(int window) const {
    if (count >= window) return slot[0];
    bool used[GK] = {false};
    for (int i = 0; i < count; ++i) used[slot[i]] = true;
    int s = 0;
    while (used[s]) ++s;
    return s;
}

int GuessBasis::push(int window) {
    const int s = next_slot(window);
    if (count >= window) drop_oldest(1);
    const int k = count;
    slot[k] = s;
    for (int j = 0; j < k; ++j)
        for (int h = 0; h < 2; ++h) G[k][j][h] = G[j][k][h] = rhs[j][h];
    G[k][k][0] = bb[0];
    G[k][k][1] = bb[1];
    row_pending = true;
    count = k + 1;
    return s;
}

// ---- the two kernels of the guess, by window size -------------------------------------------------
static void launch_multi_dot(tdgl_ctx *ctx, int grid, int64_t n, const double *b, const VecSet &vs, int newest, double *out) {
    if (vs.k <= 8) hipLaunchKernelGGL((k_multi_dot<8>), dim3(grid), dim3(BLOCK), 0, ctx->stream, n, b, vs, newest, out);
    else if (vs.k <= 12) hipLaunchKernelGGL((k_multi_dot<12>), dim3(grid), dim3(BLOCK), 0, ctx->stream, n, b, vs, newest, out);
    else hipLaunchKernelGGL((k_multi_dot<GK>), dim3(grid), dim3(BLOCK), 0, ctx->stream, n, b, vs, newest, out);
}

static void launch_combine(tdgl_ctx *ctx, int grid, int64_t n, const VecSet &vs, double *x) {
    if (vs.k <= 8) hipLaunchKernelGGL((k_combine<8>), dim3(grid), dim3(BLOCK), 0, ctx->stream, n, vs, x);
    else if (vs.k <= 12) hipLaunchKernelGGL((k_combine<12>), dim3(grid), dim3(BLOCK), 0, ctx->stream, n, vs, x);
    else hipLaunchKernelGGL((k_combine<GK>), dim3(grid), dim3(BLOCK), 0, ctx->stream, n, vs, x);
}

// The dot products of the new right-hand side with the window's images, b.b and sum b, and the Gram row of the
// window's newest vector: queued here, summed by the status kernel, on the host with the solve's first status block.
static int guess_queue_dots(tdgl_ctx *ctx, const double *b) {
    GuessBasis &g = ctx->guess;
    TDGL_TRY(g.ensure(ctx));
    VecSet vs{};
    vs.k = g.count;
    for (int j = 0; j < g.count; ++j) vs.p[j] = g.y[g.slot[j]].p;
    const int newest = g.row_pending ? g.count - 1 : -1;
    const int gg = guess_grid(ctx);
    launch_multi_dot(ctx, gg, ctx->n_own, b, vs, newest, g.part_dot.p);
    if (guess_rank_totals(ctx)) {  // every rank's double-double totals, gathered exactly (k_guess_rank_totals)
        hipLaunchKernelGGL(k_guess_rank_totals, dim3(1), dim3(BLOCK), 0, ctx->stream, (const double *)g.part_dot.p, gg, vs.k,
                           g.part_dot_rank.p, ctx->rank);
        TDGL_TRY(comm_allreduce(ctx, g.part_dot_rank.p, 2 * G_ARRAYS * G_RANK_STRIDE, 0));
    } else if (distributed(ctx)) {  // (more ranks than that: hi and lo parts summed separately, fp64 accuracy, see guess_cut)
        TDGL_TRY(comm_allreduce(ctx, g.part_dot.p, 2 * (G_Y0 + vs.k) * NB, 0));
        if (newest >= 0) TDGL_TRY(comm_allreduce(ctx, g.part_dot.p + 2 * G_N0 * NB, 2 * vs.k * NB, 0));
    }
    return TDGL_OK;  // (the sums, S_BB / S_TOL2 and the counter reset happen in the status kernel)
}

// x0 = X c with G c = X^T b (host, K x K) into x, ghosts included; *c_used: the coefficients when vectors were used,
// else NULL (x stays as it is).  `vs` keeps them for the caller.
static int guess_apply(tdgl_ctx *ctx, VecSet &vs, int grid, double *x, const double **c_used) {
    GuessBasis &g = ctx->guess;
    g.load_rhs(ctx->h_status.p, ctx->n_global);
    ctx->last_guess_vectors = 0;
    *c_used = nullptr;
    vs.k = g.count;
    for (int j = 0; j < g.count; ++j) vs.p[j] = g.x[g.slot[j]].p;
    const int used = g.solve(guess_cut(ctx), vs.c);
    if (used > 0) {
        launch_combine(ctx, grid, ctx->n_own, vs, x);
        TDGL_TRY(comm_halo(ctx, x, 1));
        ctx->last_guess_vectors = used;
        *c_used = vs.c;
    }
    return TDGL_OK;
}
