// libtdgl_hip: MI355X-native TDGL time-stepping core behind a C ABI (include/tdgl_hip.h).
// Single translation unit: kernels (kernels.inc), the AMG V-cycle (vcycle.inc), the mu factors' application (factors.inc),
// Poisson solver (poisson.inc), the in-run timers (profile.inc), the per-step driver (run.inc).

#include "tdgl_internal.h"

static thread_local std::string g_last_error;

#define TDGL_FAIL(ctx, code, ...)                                   \
    do {                                                            \
        char _buf[512];                                             \
        snprintf(_buf, sizeof(_buf), __VA_ARGS__);                  \
        if (ctx) (ctx)->err = _buf;                                 \
        g_last_error = _buf;                                        \
        return (code);                                              \
    } while (0)

#define HIP_TRY(ctx, expr)                                                               \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess)                                                            \
            TDGL_FAIL(ctx, TDGL_ERR_HIP, "HIP error %s at %s:%d (%s)", hipGetErrorString(_e), \
                      __FILE__, __LINE__, #expr);                                        \
    } while (0)

#define TDGL_TRY(expr)                 \
    do {                               \
        int _s = (expr);               \
        if (_s != TDGL_OK) return _s;  \
    } while (0)

#include "kernels.inc"

using namespace tdgl;

static inline int grid_for(int64_t n, int block = BLOCK) { return (int)((n + block - 1) / block); }

// TDGL_INDEX32=1 (tests): every "do the 16-bit indices fit" question of the set-up is answered no, so that the int32
// forms of the SELL / CSR kernels run on meshes of any size (P's needs > 65,536 coarse rows otherwise).  Read where
// the patterns are built, never on the hot path.
static bool env_index32() {
    const char *env = getenv("TDGL_INDEX32");
    return env && env[0] == '1';
}

// ---------------------------------------------------------------------------------------
// SELL construction from CSR (host)
static int build_sell_pattern(tdgl_ctx *ctx, int64_t n_rows, const int32_t *indptr,
                              const int32_t *indices, SellPattern &pat,
                              std::vector<int64_t> *slot_of_nnz, bool want16 = false, bool want_off16 = false) {
    pat.n_rows = n_rows;
    pat.n_pad = round_up(std::max<int64_t>(n_rows, 1), WAVE);
    pat.n_slices = (int32_t)(pat.n_pad / WAVE);
    std::vector<int32_t> off(pat.n_slices + 1, 0);
    for (int s = 0; s < pat.n_slices; ++s) {
        int w = 0;
        for (int64_t r = (int64_t)s * WAVE; r < std::min<int64_t>(n_rows, (int64_t)(s + 1) * WAVE); ++r)
            w = std::max(w, indptr[r + 1] - indptr[r]);
        off[s + 1] = off[s] + w;
    }
    pat.n_slots = (int64_t)off[pat.n_slices] * WAVE;
    std::vector<int32_t> cols(pat.n_slots);
    if (slot_of_nnz) slot_of_nnz->assign(indptr[n_rows], -1);
    for (int s = 0; s < pat.n_slices; ++s) {
        const int w = off[s + 1] - off[s];
        for (int lane = 0; lane < WAVE; ++lane) {
            const int64_t r = (int64_t)s * WAVE + lane;
            const int deg = (r < n_rows) ? indptr[r + 1] - indptr[r] : 0;
            for (int k = 0; k < w; ++k) {
                const int64_t slot = ((int64_t)off[s] + k) * WAVE + lane;
                if (k < deg) {
                    cols[slot] = indices[indptr[r] + k];
                    if (slot_of_nnz) (*slot_of_nnz)[indptr[r] + k] = slot;
                } else {
                    // padding (value 0): repeat the row's first column -- always a valid
                    // column, also for rectangular operators, and already in cache
                    cols[slot] = deg > 0 ? indices[indptr[r]] : 0;
                }
            }
        }
    }
    HIP_TRY(ctx, pat.slice_off.upload(off));
    HIP_TRY(ctx, pat.cols.upload(cols));
    pat.use16 = false;
    if (want16 && !env_index32()) {
        std::vector<int16_t> d16(pat.n_slots);
        bool fits = true;
        for (int sl = 0; sl < pat.n_slices && fits; ++sl)
            for (int k = off[sl]; k < off[sl + 1] && fits; ++k)
                for (int lane = 0; lane < WAVE; ++lane) {
                    const int64_t slot = (int64_t)k * WAVE + lane, row = (int64_t)sl * WAVE + lane;
                    // padded lanes past n_rows point at column 0: give them delta 0 (own row)
                    const int64_t delta = (row < n_rows) ? (int64_t)cols[slot] - row : 0;
                    if (delta < -32768 || delta > 32767) {
                        fits = false;
                        break;
                    }
                    d16[slot] = (int16_t)delta;
                }
        if (fits) {
            HIP_TRY(ctx, pat.cols16.upload(d16));
            pat.use16 = true;
        }
    }
    pat.use_off16 = false;
    if (want_off16 && !env_index32()) {
        std::vector<uint16_t> o16(std::max<int64_t>(pat.n_slots, 1), 0);
        std::vector<int32_t> sbase(std::max<int32_t>(pat.n_slices, 1), 0);
        bool fits = true;
        for (int sl = 0; sl < pat.n_slices && fits; ++sl) {
            const int64_t rows_here = std::min<int64_t>(WAVE, n_rows - (int64_t)sl * WAVE);  // (padded lanes hold column 0)
            int32_t lo = INT32_MAX, hi = 0;
            for (int k = off[sl]; k < off[sl + 1]; ++k)
                for (int lane = 0; lane < rows_here; ++lane) {
                    lo = std::min(lo, cols[(int64_t)k * WAVE + lane]);
                    hi = std::max(hi, cols[(int64_t)k * WAVE + lane]);
                }
            if (lo == INT32_MAX) lo = 0;
            if ((int64_t)hi - lo > 65535) {
                fits = false;
                break;
            }
            sbase[sl] = lo;
            for (int k = off[sl]; k < off[sl + 1]; ++k)
                for (int lane = 0; lane < WAVE; ++lane)
                    o16[(int64_t)k * WAVE + lane] = lane < rows_here ? (uint16_t)(cols[(int64_t)k * WAVE + lane] - lo) : 0;
        }
        if (fits) {
            HIP_TRY(ctx, pat.offs16.upload(o16));
            HIP_TRY(ctx, pat.slice_base.upload(sbase));
            pat.use_off16 = true;
        }
    }
    return TDGL_OK;
}

static int build_sell_f64(tdgl_ctx *ctx, int64_t n_rows, const int32_t *indptr,
                          const int32_t *indices, const double *data, SellF64 &A, bool want16 = false,
                          bool want_off16 = false) {
    std::vector<int64_t> slot;
    TDGL_TRY(build_sell_pattern(ctx, n_rows, indptr, indices, A.pat, &slot, want16, want_off16));
    std::vector<double> vals(A.pat.n_slots, 0.0);
    for (int64_t k = 0; k < indptr[n_rows]; ++k) vals[slot[k]] = data[k];
    HIP_TRY(ctx, A.vals.upload(vals));
    return TDGL_OK;
}

// ---------------------------------------------------------------------------------------
extern "C" int tdgl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char *tdgl_version(void) { return "tdgl_hip 0.1.0 (gfx950)"; }

extern "C" const char *tdgl_last_error(const tdgl_ctx *ctx) {
    return ctx ? ctx->err.c_str() : g_last_error.c_str();
}

static void ipc_free(tdgl_ctx *ctx);  // ipc.inc

extern "C" void tdgl_destroy(tdgl_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto *lv : ctx->levels) delete lv;
    if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
    ipc_free(ctx);
    delete ctx;  // every member releases what it owns, the stream last (tdgl_internal.h: tdgl_ctx)
}

extern "C" int tdgl_synchronize(tdgl_ctx *ctx) {
    if (!ctx) return TDGL_ERR_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

static int create_impl(tdgl_ctx *ctx, const tdgl_mesh_desc *d) {
    const int64_t n = d->n_sites, m = d->n_edges, nb = d->n_boundary_edges;
    ctx->n = n;
    ctx->m = m;
    ctx->nb = nb;
    ctx->n_pad = round_up(n, WAVE);
    ctx->m_pad = round_up(std::max<int64_t>(m, 1), WAVE);
    ctx->n_own = (d->n_owned > 0) ? d->n_owned : n;
    ctx->n_global = n;
    if (ctx->n_own > n) TDGL_FAIL(ctx, TDGL_ERR_ARG, "n_owned exceeds n_sites");
    if (ctx->n_own < n && d->site_perm) TDGL_FAIL(ctx, TDGL_ERR_ARG, "site_perm must be NULL when n_owned < n_sites");
    ctx->u = d->u;
    ctx->gamma = d->gamma;
    ctx->fix_psi = d->fix_psi != 0;

    // ---- site permutation ----------------------------------------------------------
    ctx->perm.resize(n);
    ctx->iperm.assign(n, -1);
    for (int64_t i = 0; i < n; ++i) ctx->perm[i] = d->site_perm ? d->site_perm[i] : (int32_t)i;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t r = ctx->perm[i];
        if (r < 0 || r >= n || ctx->iperm[r] != -1)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "site_perm is not a permutation of 0..n_sites-1");
        ctx->iperm[r] = (int32_t)i;
    }

    // ---- edges in internal numbering, sorted for gather locality ---------------------
    std::vector<int32_t> p0(m), p1(m);
    for (int64_t e = 0; e < m; ++e) {
        const int32_t i = d->edges[2 * e], j = d->edges[2 * e + 1];
        if (i < 0 || i >= n || j < 0 || j >= n || i == j)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "edge %lld has invalid sites (%d, %d)", (long long)e, i, j);
        p0[e] = ctx->iperm[i];
        p1[e] = ctx->iperm[j];
    }
    ctx->edge_perm.resize(m);
    std::iota(ctx->edge_perm.begin(), ctx->edge_perm.end(), 0);
    // (one-process-per-GPU mode: edges that touch a ghost site go last, so that the edges between
    // owned sites form a prefix the edge kernel can process while ghost values travel)
    std::sort(ctx->edge_perm.begin(), ctx->edge_perm.end(), [&](int32_t a, int32_t b) {
        const int32_t alo = std::min(p0[a], p1[a]), ahi = std::max(p0[a], p1[a]);
        const int32_t blo = std::min(p0[b], p1[b]), bhi = std::max(p0[b], p1[b]);
        const bool ag = ahi >= ctx->n_own, bg = bhi >= ctx->n_own;
        if (ag != bg) return bg;
        return alo != blo ? alo < blo : (ahi != bhi ? ahi < bhi : a < b);
    });
    ctx->m_int = 0;
    for (int64_t e = 0; e < m; ++e) ctx->m_int += std::max(p0[e], p1[e]) < ctx->n_own ? 1 : 0;
    ctx->edge_iperm.resize(m);
    for (int64_t k = 0; k < m; ++k) ctx->edge_iperm[ctx->edge_perm[k]] = (int32_t)k;

    std::vector<int32_t> e0(ctx->m_pad, 0), e1(ctx->m_pad, 0);
    std::vector<double> inv_len(ctx->m_pad, 0.0), dx(ctx->m_pad, 0.0), dy(ctx->m_pad, 0.0), w(m);
    for (int64_t k = 0; k < m; ++k) {
        const int32_t e = ctx->edge_perm[k];
        e0[k] = p0[e];
        e1[k] = p1[e];
        if (!(d->edge_lengths[e] > 0.0) || !(d->dual_edge_lengths[e] >= 0.0))
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "edge %d has non-positive length or negative dual length", e);
        inv_len[k] = 1 / d->edge_lengths[e];                       // operators.py:271
        w[k] = d->dual_edge_lengths[e] / d->edge_lengths[e];       // operators.py:272
        dx[k] = d->directions[2 * e];
        dy[k] = d->directions[2 * e + 1];
    }

    // ---- site graph (CSR, neighbours sorted) -> SELL pattern ------------------------
    std::vector<int32_t> deg(n + 1, 0);
    for (int64_t k = 0; k < m; ++k) {
        deg[e0[k] + 1]++;
        deg[e1[k] + 1]++;
    }
    std::vector<int32_t> indptr(n + 1, 0);
    for (int64_t i = 0; i < n; ++i) indptr[i + 1] = indptr[i] + deg[i + 1];
    std::vector<int32_t> nbr(2 * m), code(2 * m), fill(indptr.begin(), indptr.end() - 1);
    for (int64_t k = 0; k < m; ++k) {  // edges sorted by min site -> rows fill in order
        nbr[fill[e0[k]]] = e1[k];
        code[fill[e0[k]]++] = (int32_t)(k << 1);        // row = tail: U_e
        nbr[fill[e1[k]]] = e0[k];
        code[fill[e1[k]]++] = (int32_t)(k << 1) | 1;    // row = head: conj(U_e)
    }
    for (int64_t i = 0; i < n; ++i) {  // sort each row by neighbour index
        const int b = indptr[i], e = indptr[i + 1];
        std::vector<std::pair<int32_t, int32_t>> row(e - b);
        for (int k = b; k < e; ++k) row[k - b] = {nbr[k], code[k]};
        std::sort(row.begin(), row.end());
        for (int k = b; k < e; ++k) {
            nbr[k] = row[k - b].first;
            code[k] = row[k - b].second;
        }
    }
    // rows exist for owned sites only; ghost sites appear as columns
    const int64_t n_rows = ctx->n_own;
    std::vector<int64_t> slot;
    TDGL_TRY(build_sell_pattern(ctx, n_rows, indptr.data(), nbr.data(), ctx->lap_pat, &slot, /*want16=*/true));
    const int64_t n_slots = ctx->lap_pat.n_slots;
    std::vector<int32_t> slot_edge(n_slots, -1);
    std::vector<double> slot_w(n_slots, 0.0), diag(ctx->n_pad, 0.0), area(ctx->n_pad, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        const double a = d->areas[ctx->perm[i]];
        if (!(a > 0.0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "site %d has non-positive area", ctx->perm[i]);
        area[i] = a;
        if (i >= n_rows) continue;
        double dsum = 0.0;
        for (int k = indptr[i]; k < indptr[i + 1]; ++k) {
            const double wk = w[code[k] >> 1];
            slot_edge[slot[k]] = code[k];
            slot_w[slot[k]] = wk / a;
            dsum += -wk / a;  // operators.py:166-167
        }
        diag[i] = dsum;
    }
    std::vector<uint8_t> fixed(ctx->n_pad, 0);
    if (d->fix_psi)
        for (int64_t k = 0; k < d->n_fixed; ++k) {
            const int32_t s = d->fixed_sites[k];
            if (s < 0 || s >= n) TDGL_FAIL(ctx, TDGL_ERR_ARG, "fixed site %d out of range", s);
            fixed[ctx->iperm[s]] = 1;
        }

    HIP_TRY(ctx, ctx->lap_slot_edge.upload(slot_edge));
    HIP_TRY(ctx, ctx->lap_slot_w.upload(slot_w));
    HIP_TRY(ctx, ctx->lap_vals.alloc(n_slots));
    HIP_TRY(ctx, ctx->lap_diag.upload(diag));
    HIP_TRY(ctx, ctx->fixed_mask.upload(fixed));
    HIP_TRY(ctx, ctx->area.upload(area));
    HIP_TRY(ctx, ctx->e0.upload(e0));
    HIP_TRY(ctx, ctx->e1.upload(e1));
    HIP_TRY(ctx, ctx->e_inv_len.upload(inv_len));
    HIP_TRY(ctx, ctx->e_dirx.upload(dx));
    HIP_TRY(ctx, ctx->e_diry.upload(dy));
    HIP_TRY(ctx, ctx->e_U.alloc(ctx->m_pad));
    HIP_TRY(ctx, ctx->e_A.alloc(2 * ctx->m_pad));
    HIP_TRY(ctx, ctx->e_Aprev.alloc(2 * ctx->m_pad));
    HIP_TRY(ctx, ctx->e_dAdt.alloc(ctx->m_pad));

    // ---- Neumann boundary term (operators.py:188-230) -------------------------------
    std::vector<int32_t> s0(std::max<int64_t>(nb, 1), 0), s1(std::max<int64_t>(nb, 1), 0);
    std::vector<double> c0(std::max<int64_t>(nb, 1), 0.0), c1(std::max<int64_t>(nb, 1), 0.0);
    for (int64_t k = 0; k < nb; ++k) {
        const int32_t e = d->boundary_edge_indices[k];
        if (e < 0 || e >= m) TDGL_FAIL(ctx, TDGL_ERR_ARG, "boundary edge %d out of range", e);
        const int32_t i = d->edges[2 * e], j = d->edges[2 * e + 1];
        s0[k] = ctx->iperm[i];
        s1[k] = ctx->iperm[j];
        c0[k] = d->edge_lengths[e] / (2 * d->areas[i]);
        c1[k] = d->edge_lengths[e] / (2 * d->areas[j]);
    }
    HIP_TRY(ctx, ctx->b_s0.upload(s0));
    HIP_TRY(ctx, ctx->b_s1.upload(s1));
    HIP_TRY(ctx, ctx->b_c0.upload(c0));
    HIP_TRY(ctx, ctx->b_c1.upload(c1));
    HIP_TRY(ctx, ctx->b_mu.alloc(std::max<int64_t>(nb, 1)));
    HIP_TRY(ctx, ctx->cvec.alloc(ctx->n_pad));
    HIP_TRY(ctx, ctx->ceff.alloc(ctx->n_pad));

    // ---- state ------------------------------------------------------------------------
    HIP_TRY(ctx, ctx->psi[0].alloc(ctx->n_pad));
    HIP_TRY(ctx, ctx->psi[1].alloc(ctx->n_pad));
    HIP_TRY(ctx, ctx->lap[0].alloc(ctx->n_pad));
    HIP_TRY(ctx, ctx->lap[1].alloc(ctx->n_pad));
    HIP_TRY(ctx, ctx->mu.alloc(ctx->n_pad));
    HIP_TRY(ctx, ctx->eps.alloc(ctx->n_pad));
    HIP_TRY(ctx, ctx->bvec.alloc(ctx->n_pad));
    HIP_TRY(ctx, ctx->js.alloc(ctx->m_pad));
    HIP_TRY(ctx, ctx->jn.alloc(ctx->m_pad));
    HIP_TRY(ctx, ctx->d_status.alloc(1));
    // The status block is published into device memory and copied to this pinned block at every host
    // synchronisation.
    HIP_TRY(ctx, ctx->h_status.alloc(1));
    // (the environment switches of the library: what the test-suite needs to reach a code path -- DESIGN.md section 5)
    ctx->run_ahead_disabled = getenv("TDGL_NO_RUN_AHEAD") != nullptr;
    ctx->sync_shadow_disabled = getenv("TDGL_NO_SYNC_SHADOW") != nullptr;
    ctx->pd_two_pass = getenv("TDGL_PD_TWO_PASS") != nullptr;
    if (const char *e = getenv("TDGL_PCG_PREDICT")) ctx->pcg_predict_from_guess = strcmp(e, "last") != 0;
    ctx->status_dev = ctx->d_status.p;
    HIP_TRY(ctx, ctx->scal.alloc(S_COUNT));
    HIP_TRY(ctx, ctx->d_ctl.alloc(1));
    HIP_TRY(ctx, ctx->d_rec.alloc(RA_BATCH_MAX));
    HIP_TRY(ctx, ctx->h_ctl.alloc(1));
    HIP_TRY(ctx, ctx->h_rec.alloc(RA_BATCH_MAX));
    HIP_TRY(ctx, ctx->ev0.create());
    HIP_TRY(ctx, ctx->ev1.create());
    ctx->psi_blocks = (int)std::min<int64_t>(std::max<int64_t>(grid_for(ctx->n_own), 1), 2048);
    {
        const int64_t tiles = (ctx->n_own + BLOCK - 1) / BLOCK;
        ctx->npart = (int)std::min<int64_t>(NB, std::max<int64_t>(1, (tiles + XCDS - 1) / XCDS) * XCDS);
        if (ctx->n_own < ctx->n) ctx->npart = NB;
    }
    HIP_TRY(ctx, ctx->psi_dmax_part.alloc(ctx->psi_blocks));
    HIP_TRY(ctx, ctx->psi_fail_part.alloc(ctx->psi_blocks));
    HIP_TRY(ctx, ctx->comm_stream.create(hipStreamNonBlocking));
    HIP_TRY(ctx, ctx->ev_pack.create(/*timing=*/false));
    HIP_TRY(ctx, ctx->ev_halo.create(/*timing=*/false));
    HIP_TRY(ctx, ctx->ev_status.create(/*timing=*/false));
    return TDGL_OK;
}

extern "C" int tdgl_create(tdgl_ctx **out, const tdgl_mesh_desc *d, int device_id) {
    if (!out || !d) TDGL_FAIL((tdgl_ctx *)nullptr, TDGL_ERR_ARG, "tdgl_create: null argument");
    *out = nullptr;
    if (d->n_sites <= 0 || d->n_edges <= 0 || d->n_boundary_edges < 0 || !d->edges || !d->areas ||
        !d->edge_lengths || !d->dual_edge_lengths || !d->directions ||
        (d->n_boundary_edges > 0 && !d->boundary_edge_indices) || (d->n_fixed > 0 && !d->fixed_sites))
        TDGL_FAIL((tdgl_ctx *)nullptr, TDGL_ERR_ARG, "tdgl_create: incomplete mesh description");
    if (d->n_sites >= (1ll << 30) || d->n_edges >= (1ll << 30))
        TDGL_FAIL((tdgl_ctx *)nullptr, TDGL_ERR_ARG, "tdgl_create: mesh too large for int32 indices");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        TDGL_FAIL((tdgl_ctx *)nullptr, TDGL_ERR_HIP,
                  "tdgl_create: no HIP device available (%s); this library has no CPU fallback",
                  hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev)
        TDGL_FAIL((tdgl_ctx *)nullptr, TDGL_ERR_ARG, "tdgl_create: device %d not in [0, %d)", device_id, ndev);
    tdgl_ctx *ctx = new tdgl_ctx();
    ctx->device = device_id;
    int st = TDGL_OK;
    if (hipSetDevice(device_id) != hipSuccess || ctx->stream.create() != hipSuccess) {
        g_last_error = "tdgl_create: cannot select device / create stream";
        st = TDGL_ERR_HIP;
    } else {
        st = create_impl(ctx, d);
    }
    if (st != TDGL_OK) {
        g_last_error = ctx->err.empty() ? g_last_error : ctx->err;
        tdgl_destroy(ctx);
        return st;
    }
    *out = ctx;
    return TDGL_OK;
}

// ---------------------------------------------------------------------------------------
// host <-> device with the site / edge permutation applied
template <class T>
static int upload_sites(tdgl_ctx *ctx, const T *ref, DevBuf<T> &dst) {
    std::vector<T> tmp(ctx->n_pad, T{});
    for (int64_t i = 0; i < ctx->n; ++i) tmp[i] = ref[ctx->perm[i]];
    HIP_TRY(ctx, hipMemcpyAsync(dst.p, tmp.data(), ctx->n_pad * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

template <class T>
static int download_sites(tdgl_ctx *ctx, const T *src, T *ref) {
    std::vector<T> tmp(ctx->n);
    HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), src, ctx->n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < ctx->n; ++i) ref[ctx->perm[i]] = tmp[i];
    return TDGL_OK;
}

static int download_edges(tdgl_ctx *ctx, const double *src, double *ref) {
    std::vector<double> tmp(ctx->m);
    HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), src, ctx->m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t k = 0; k < ctx->m; ++k) ref[ctx->edge_perm[k]] = tmp[k];
    return TDGL_OK;
}

#define CTX_GUARD(ctx)                              \
    do {                                            \
        if (!(ctx)) return TDGL_ERR_ARG;            \
        HIP_TRY(ctx, hipSetDevice((ctx)->device));  \
    } while (0)

// ---------------------------------------------------------------------------------------
// Tile ranges of the SELL kernels whose rows are the owned sites.  part 0: all tiles; 1: the
// leading ghost-free tiles (safe to run while a halo exchange is in flight); 2: the rest.
static inline void tile_range(const tdgl_ctx *ctx, int n_slices, int part, int *tile_base, int *slice_end,
                              int *tiles) {
    const int all = (n_slices + BLOCK / WAVE - 1) / (BLOCK / WAVE);
    const int ni = std::min(ctx->int_tiles, all);
    if (part == 1) {
        *tile_base = 0, *tiles = ni, *slice_end = ni * (BLOCK / WAVE);
    } else if (part == 2) {
        *tile_base = ni, *tiles = all - ni, *slice_end = n_slices;
    } else {
        *tile_base = 0, *tiles = all, *slice_end = n_slices;
    }
}

// (vals: covariant-Laplacian values other than the context's -- an ensemble's replica)
static void launch_psi_laplacian(tdgl_ctx *ctx, bool rhs, const double2 *psi, double2 *lap, int part = 0, const double2 *vals = nullptr) {
    int tile_base, slice_end, tiles;
    tile_range(ctx, ctx->lap_pat.n_slices, part, &tile_base, &slice_end, &tiles);
    if (tiles <= 0) return;
    const int per_xcd = (tiles + XCDS - 1) / XCDS, grid = per_xcd * XCDS;
    const SellPattern &pat = ctx->lap_pat;
    const double *c = rhs ? ctx->ceff.p : ctx->cvec.p;
    if (!vals) vals = ctx->lap_vals.p;
#define TDGL_K1(RHS, IT, COLS)                                                                              \
    hipLaunchKernelGGL((k_psi_laplacian<RHS, IT>), dim3(grid), dim3(BLOCK), 0, ctx->stream, slice_end, per_xcd, \
                       tile_base, pat.n_rows, pat.slice_off.p, COLS, vals, ctx->lap_diag.p,                \
                       ctx->fixed_mask.p, psi, lap, ctx->area.p, c, ctx->bvec.p)
    if (pat.use16) {
        if (rhs) TDGL_K1(true, int16_t, pat.cols16.p); else TDGL_K1(false, int16_t, pat.cols16.p);
    } else {
        if (rhs) TDGL_K1(true, int32_t, pat.cols.p); else TDGL_K1(false, int32_t, pat.cols.p);
    }
#undef TDGL_K1
}

static void launch_psi_update(tdgl_ctx *ctx, const double2 *psi, const double *mu, const double2 *lap,
                              double dt, double2 *psi_new, double *abs_sq, const double *abs_sq_in = nullptr) {
    hipLaunchKernelGGL(k_psi_update, dim3(ctx->psi_blocks), dim3(BLOCK), 0, ctx->stream, ctx->n_own, psi, mu,
                       ctx->eps.p, lap, dt, ctx->u, ctx->gamma, psi_new, abs_sq, ctx->psi_dmax_part.p,
                       ctx->psi_fail_part.p, abs_sq_in);
    ctx->psi_status_pending = true;
}

// ... with the edge currents of the step just accepted in the same launch (k_psi_update_with_currents)
static void launch_psi_update_with_currents(tdgl_ctx *ctx, const double2 *psi, const double *mu, const double2 *lap,
                                            double dt, double2 *psi_new) {
    hipLaunchKernelGGL(k_psi_update_with_currents, dim3(ctx->psi_blocks + grid_for(ctx->m)), dim3(BLOCK), 0, ctx->stream,
                       ctx->psi_blocks, ctx->n_own, psi, mu, ctx->eps.p, lap, dt, ctx->u, ctx->gamma, psi_new,
                       ctx->psi_dmax_part.p, ctx->psi_fail_part.p, ctx->m, ctx->e0.p, ctx->e1.p, ctx->e_inv_len.p,
                       ctx->e_U.p, ctx->js.p, ctx->jn.p);
    ctx->stat_edge_launches += 1;
    ctx->psi_status_pending = true;
}

// one attempt of the run-ahead loop: psi update (+ the owed edge currents) ...
static void launch_ra_psi(tdgl_ctx *ctx, bool with_currents) {
    const int64_t m = with_currents ? ctx->m : 0;
    hipLaunchKernelGGL(k_ra_psi_update, dim3(ctx->psi_blocks + (m > 0 ? grid_for(m) : 0)), dim3(BLOCK), 0, ctx->stream,
                       ctx->psi_blocks, ctx->n_own, ctx->psi[0].p, ctx->psi[1].p, (const double2 *)ctx->lap[0].p,
                       (const double2 *)ctx->lap[1].p, (const double *)ctx->mu.p, (const double *)ctx->eps.p, ctx->u, ctx->gamma,
                       ctx->psi_dmax_part.p, ctx->psi_fail_part.p, m, ctx->e0.p, ctx->e1.p, ctx->e_inv_len.p, ctx->e_U.p,
                       ctx->js.p, ctx->jn.p, ctx->d_ctl.p);
}

// ... then L psi' and the right-hand side
static void launch_ra_laplacian(tdgl_ctx *ctx) {
    const SellPattern &pat = ctx->lap_pat;
    const int tiles = (pat.n_slices + BLOCK / WAVE - 1) / (BLOCK / WAVE);
    const int per_xcd = (tiles + XCDS - 1) / XCDS, grid = per_xcd * XCDS;
#define TDGL_K1RA(IT, COLS)                                                                                          \
    hipLaunchKernelGGL((k_psi_laplacian_ra<IT>), dim3(grid), dim3(BLOCK), 0, ctx->stream, pat.n_slices, per_xcd, pat.n_rows, \
                       pat.slice_off.p, COLS, ctx->lap_vals.p, ctx->lap_diag.p, ctx->fixed_mask.p,                   \
                       (const double2 *)ctx->psi[0].p, (const double2 *)ctx->psi[1].p, ctx->lap[0].p, ctx->lap[1].p, \
                       ctx->area.p, (const double *)ctx->ceff.p, ctx->bvec.p, (const StepCtl *)ctx->d_ctl.p)
    if (pat.use16) TDGL_K1RA(int16_t, pat.cols16.p); else TDGL_K1RA(int32_t, pat.cols.p);
#undef TDGL_K1RA
}

// L psi^n with the links a ramping attempt has just moved (k_psi_laplacian_ra_fresh)
static void launch_ra_laplacian_fresh(tdgl_ctx *ctx) {
    const SellPattern &pat = ctx->lap_pat;
    const int tiles = (pat.n_slices + BLOCK / WAVE - 1) / (BLOCK / WAVE);
    const int per_xcd = (tiles + XCDS - 1) / XCDS, grid = per_xcd * XCDS;
#define TDGL_K1RA(IT, COLS)                                                                                                        \
    hipLaunchKernelGGL((k_psi_laplacian_ra_fresh<IT>), dim3(grid), dim3(BLOCK), 0, ctx->stream, pat.n_slices, per_xcd, pat.n_rows, \
                       pat.slice_off.p, COLS, ctx->lap_vals.p, ctx->lap_diag.p, ctx->fixed_mask.p, (const double2 *)ctx->psi[0].p, \
                       (const double2 *)ctx->psi[1].p, ctx->lap[0].p, ctx->lap[1].p, (const StepCtl *)ctx->d_ctl.p)
    if (pat.use16) TDGL_K1RA(int16_t, pat.cols16.p); else TDGL_K1RA(int32_t, pat.cols.p);
#undef TDGL_K1RA
}

// reduce the outcome of the last psi update into d_status (together with the PCG scalars);
// guess_start: first synchronisation of a solve with the projection guess (sums its partial arrays,
// sets S_BB / S_TOL2, resets the iteration counters); rr_part: residual partials to sum into S_RR
// workgroups of the projection guess's dot-product pass (k_multi_dot): one per CU -- every workgroup ends with
// a reduction of 2 K + 2 double-double sums, and the status kernel (ONE workgroup, on the step's critical
// path) adds that many partials per sum; four waves per CU with 13 16-byte loads per lane in flight keep
// the stream busy.
static inline int guess_grid(const tdgl_ctx *ctx) { return std::min(ctx->npart, 256); }
// one process per GPU with at most G_RANK_STRIDE ranks: the ranks' double-double totals are gathered exactly
static inline bool guess_rank_totals(const tdgl_ctx *ctx) {
    static const bool off = getenv("TDGL_GUESS_NO_GATHER") != nullptr;  // (tests: the path of more than 16 ranks)
    return (ctx->world > 1 || ctx->comm != nullptr || ctx->ipc != nullptr) && ctx->world <= G_RANK_STRIDE && !off;
}

static void publish_status(tdgl_ctx *ctx, bool guess_start = false, const double *rr_part = nullptr) {
    const bool psi = ctx->psi_status_pending;
    const bool rank_totals = guess_rank_totals(ctx);
    hipLaunchKernelGGL(k_publish_status, dim3(1), dim3(BLOCK), 0, ctx->stream, ctx->status_dev, ctx->scal.p,
                       psi ? ctx->psi_dmax_part.p : (const double *)nullptr,
                       psi ? ctx->psi_fail_part.p : (const int32_t *)nullptr, ctx->psi_blocks,
                       ctx->guess.d_dot.n ? ctx->guess.d_dot.p : (double *)nullptr,
                       guess_start ? (rank_totals ? ctx->guess.part_dot_rank.p : ctx->guess.part_dot.p) : (const double *)nullptr,
                       ctx->guess.count,
                       rank_totals ? ctx->world : guess_grid(ctx), rank_totals ? (int)G_RANK_STRIDE : (int)NB, (double)ctx->n_global,
                       ctx->popt.rtol * ctx->popt.rtol, rr_part);
    ctx->psi_status_pending = false;
}

// part 0: all edges; 1: edges between owned sites; 2: edges touching a ghost site
static void launch_edge_currents(tdgl_ctx *ctx, const double2 *psi, const double *mu, double *js,
                                 double *jn, int part = 0) {
    const int64_t base = (part == 2) ? ctx->m_int : 0, end = (part == 1) ? ctx->m_int : ctx->m;
    if (end <= base) return;
    if (part != 2) ctx->stat_edge_launches += 1;  // (parts 1 and 2 together form the currents once)
    const int grid = grid_for(end - base);
    const double *dadt = ctx->loop.field.has_dadt ? ctx->e_dAdt.p : (const double *)nullptr;
    if (js && jn)
        hipLaunchKernelGGL((k_edge_currents<true, true>), dim3(grid), dim3(BLOCK), 0, ctx->stream, end,
                           ctx->e0.p, ctx->e1.p, ctx->e_inv_len.p, ctx->e_U.p, psi, mu, js, jn, dadt, base);
    else if (js)
        hipLaunchKernelGGL((k_edge_currents<true, false>), dim3(grid), dim3(BLOCK), 0, ctx->stream, end,
                           ctx->e0.p, ctx->e1.p, ctx->e_inv_len.p, ctx->e_U.p, psi, mu, js, jn, dadt, base);
    else if (jn)
        hipLaunchKernelGGL((k_edge_currents<false, true>), dim3(grid), dim3(BLOCK), 0, ctx->stream, end,
                           ctx->e0.p, ctx->e1.p, ctx->e_inv_len.p, ctx->e_U.p, psi, mu, js, jn, dadt, base);
}

static inline int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

#include "ipc.inc"
#include "comm.inc"
#include "profile.inc"
#include "loop.inc"
#include "guess.inc"
#include "vcycle.inc"
#include "factors.inc"
#include "poisson.inc"
#include "dense.inc"
#include "schur.inc"
#include "drive.inc"
#include "screening.inc"
#include "screening_tree.inc"
#include "fields.inc"
#include "vortices.inc"
#include "sample.inc"
#include "census.inc"
#include "run.inc"

extern "C" int tdgl_set_state(tdgl_ctx *ctx, const double *psi, const double *mu) {
    CTX_GUARD(ctx);
    if (!psi || !mu) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_state: null array");
    TDGL_TRY(upload_sites(ctx, reinterpret_cast<const double2 *>(psi), ctx->psi[ctx->loop.cur]));
    TDGL_TRY(upload_sites(ctx, mu, ctx->mu));
    ctx->have_state = true;
    ctx->lap_valid = false;
    ctx->currents.new_state();
    ctx->loop.new_state(ctx->loop.cur);
    ctx->prev_dt = ctx->prev_dt2 = 0.0;  // no mu history: the next solve starts from mu itself
    ctx->guess.reset();                   // (nor a projection basis)
    ctx->choice.reset();                  // (nor a history for the loop's solver choice)
    return TDGL_OK;
}

extern "C" int tdgl_set_controller(tdgl_ctx *ctx, const tdgl_controller *c) {
    if (!ctx || !c) return TDGL_ERR_ARG;
    if (c->dt_init > c->dt_max) TDGL_FAIL(ctx, TDGL_ERR_ARG, "dt_init must be less than or equal to dt_max.");
    if (!(c->adaptive_time_step_multiplier > 0 && c->adaptive_time_step_multiplier < 1))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "adaptive_time_step_multiplier must be in (0, 1) (got %g).",
                  c->adaptive_time_step_multiplier);
    if (c->adaptive_window < 0) TDGL_FAIL(ctx, TDGL_ERR_ARG, "adaptive_window must be >= 0 (got %d).", c->adaptive_window);
    ctx->loop.reset(*c);
    return TDGL_OK;
}

extern "C" int tdgl_set_probes(tdgl_ctx *ctx, const int32_t *sites, int32_t n_probe) {
    CTX_GUARD(ctx);
    if (n_probe < 0 || (n_probe > 0 && !sites)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_probes: bad arguments");
    ctx->probes.clear();
    ctx->probe_ring_count = 0;
    for (int k = 0; k < n_probe; ++k) {
        if (sites[k] < 0 || sites[k] >= ctx->n) TDGL_FAIL(ctx, TDGL_ERR_ARG, "probe site %d out of range", sites[k]);
        ctx->probes.push_back(ctx->iperm[sites[k]]);
    }
    ctx->h_probe_out.release();
    if (n_probe > 0) {
        HIP_TRY(ctx, ctx->d_probes.upload(ctx->probes));
        HIP_TRY(ctx, ctx->d_probe_out.alloc((size_t)PROBE_RING_STEPS * 2 * n_probe));
        HIP_TRY(ctx, ctx->h_probe_out.alloc((size_t)PROBE_RING_STEPS * 2 * n_probe, false));
    }
    return TDGL_OK;
}

// ---------------------------------------------------------------------------------------
static int ensure_currents(tdgl_ctx *ctx) {
    if (ctx->currents.formed()) return TDGL_OK;
    if (!ctx->have_links) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "link exponents not set");
    launch_edge_currents(ctx, ctx->psi[ctx->loop.cur].p, ctx->mu.p, ctx->js.p, ctx->jn.p);
    HIP_TRY(ctx, hipGetLastError());
    ctx->currents.request();
    return TDGL_OK;
}

extern "C" int tdgl_get_state(tdgl_ctx *ctx, double *psi, double *mu, double *supercurrent,
                              double *normal_current) {
    CTX_GUARD(ctx);
    if (!ctx->have_state) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_get_state: no state set");
    if (psi) TDGL_TRY(download_sites(ctx, ctx->psi[ctx->loop.cur].p, reinterpret_cast<double2 *>(psi)));
    if (mu) TDGL_TRY(download_sites(ctx, ctx->mu.p, mu));
    if (supercurrent || normal_current) {
        TDGL_TRY(ensure_currents(ctx));
        if (supercurrent) TDGL_TRY(download_edges(ctx, ctx->js.p, supercurrent));
        if (normal_current) TDGL_TRY(download_edges(ctx, ctx->jn.p, normal_current));
    }
    return TDGL_OK;
}

// ---------------------------------------------------------------------------------------
// single-operator entry points (parity tests)
struct Scratch {
    DevBuf<double2> c0, c1;
    DevBuf<double> r0, r1;
};

extern "C" int tdgl_apply_psi_laplacian(tdgl_ctx *ctx, const double *psi, double *out) {
    CTX_GUARD(ctx);
    if (!psi || !out) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null argument");
    if (!ctx->have_links) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "link exponents not set");
    Scratch s;
    HIP_TRY(ctx, s.c0.alloc(ctx->n_pad));
    HIP_TRY(ctx, s.c1.alloc(ctx->n_pad));
    TDGL_TRY(upload_sites(ctx, reinterpret_cast<const double2 *>(psi), s.c0));
    launch_psi_laplacian(ctx, false, s.c0.p, s.c1.p);
    HIP_TRY(ctx, hipGetLastError());
    return download_sites(ctx, s.c1.p, reinterpret_cast<double2 *>(out));
}

extern "C" int tdgl_supercurrent(tdgl_ctx *ctx, const double *psi, double *out) {
    CTX_GUARD(ctx);
    if (!psi || !out) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null argument");
    if (!ctx->have_links) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "link exponents not set");
    Scratch s;
    HIP_TRY(ctx, s.c0.alloc(ctx->n_pad));
    HIP_TRY(ctx, s.r0.alloc(ctx->m_pad));
    TDGL_TRY(upload_sites(ctx, reinterpret_cast<const double2 *>(psi), s.c0));
    launch_edge_currents(ctx, s.c0.p, nullptr, s.r0.p, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    return download_edges(ctx, s.r0.p, out);
}

// psi_gradient @ psi (operators.py:340-344): [n_edges] complex
extern "C" int tdgl_apply_psi_gradient(tdgl_ctx *ctx, const double *psi, double *out) {
    CTX_GUARD(ctx);
    if (!psi || !out) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null argument");
    if (!ctx->have_links) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "link exponents not set");
    Scratch s;
    HIP_TRY(ctx, s.c0.alloc(ctx->n_pad));
    HIP_TRY(ctx, s.c1.alloc(ctx->m_pad));
    TDGL_TRY(upload_sites(ctx, reinterpret_cast<const double2 *>(psi), s.c0));
    hipLaunchKernelGGL(k_edge_gradient, dim3(grid_for(ctx->m)), dim3(BLOCK), 0, ctx->stream, ctx->m, ctx->e0.p,
                       ctx->e1.p, ctx->e_inv_len.p, ctx->e_U.p, s.c0.p, s.c1.p);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<double2> tmp(ctx->m);
    HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), s.c1.p, ctx->m * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double2 *o = reinterpret_cast<double2 *>(out);
    for (int64_t k = 0; k < ctx->m; ++k) o[ctx->edge_perm[k]] = tmp[k];
    return TDGL_OK;
}

// divergence @ edge_field (operators.py:59-84): [n_edges] real -> [n_sites]
extern "C" int tdgl_apply_divergence(tdgl_ctx *ctx, const double *edge_field, double *out) {
    CTX_GUARD(ctx);
    if (!edge_field || !out) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null argument");
    if (ctx->n_own != ctx->n) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_apply_divergence: single-GPU contexts only");
    Scratch s;
    HIP_TRY(ctx, s.r0.alloc(ctx->m_pad));
    HIP_TRY(ctx, s.r1.alloc(ctx->n_pad));
    std::vector<double> tmp(ctx->m_pad, 0.0);
    for (int64_t k = 0; k < ctx->m; ++k) tmp[k] = edge_field[ctx->edge_perm[k]];
    HIP_TRY(ctx, hipMemcpyAsync(s.r0.p, tmp.data(), ctx->m_pad * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_ceff(ctx, s.r0.p, nullptr, s.r1.p);
    HIP_TRY(ctx, hipGetLastError());
    return download_sites(ctx, s.r1.p, out);
}

// mu_laplacian @ mu (operators.py:285)
extern "C" int tdgl_apply_mu_laplacian(tdgl_ctx *ctx, const double *mu, double *out) {
    CTX_GUARD(ctx);
    if (!mu || !out) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null argument");
    if (ctx->n_own != ctx->n) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_apply_mu_laplacian: single-GPU contexts only");
    Scratch s;
    HIP_TRY(ctx, s.r0.alloc(ctx->n_pad));
    HIP_TRY(ctx, s.r1.alloc(ctx->n_pad));
    TDGL_TRY(upload_sites(ctx, mu, s.r0));
    hipLaunchKernelGGL(k_mu_laplacian, dim3(grid_for((int64_t)ctx->lap_pat.n_slices * WAVE)), dim3(BLOCK), 0,
                       ctx->stream, ctx->lap_pat.n_slices, ctx->lap_pat.n_rows, ctx->lap_pat.slice_off.p,
                       ctx->lap_pat.cols.p, ctx->lap_slot_w.p, ctx->lap_diag.p, (const double *)s.r0.p, s.r1.p);
    HIP_TRY(ctx, hipGetLastError());
    return download_sites(ctx, s.r1.p, out);
}

// mu_boundary_laplacian @ mu_boundary (operators.py:188-230, unmasked as built at :286)
extern "C" int tdgl_apply_mu_boundary_laplacian(tdgl_ctx *ctx, const double *mu_boundary, double *out) {
    CTX_GUARD(ctx);
    if ((ctx->nb > 0 && !mu_boundary) || !out) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null argument");
    Scratch s;
    DevBuf<double> mb;
    HIP_TRY(ctx, s.r0.alloc(ctx->n_pad));
    HIP_TRY(ctx, mb.alloc(std::max<int64_t>(ctx->nb, 1)));
    if (ctx->nb > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(mb.p, mu_boundary, ctx->nb * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        launch_boundary_term(ctx, mb.p, s.r0.p);
    }
    HIP_TRY(ctx, hipGetLastError());
    return download_sites(ctx, s.r0.p, out);
}

extern "C" int tdgl_normal_current(tdgl_ctx *ctx, const double *mu, double *out) {
    CTX_GUARD(ctx);
    if (!mu || !out) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null argument");
    Scratch s;
    HIP_TRY(ctx, s.r0.alloc(ctx->n_pad));
    HIP_TRY(ctx, s.r1.alloc(ctx->m_pad));
    TDGL_TRY(upload_sites(ctx, mu, s.r0));
    launch_edge_currents(ctx, nullptr, s.r0.p, nullptr, s.r1.p);
    HIP_TRY(ctx, hipGetLastError());
    return download_edges(ctx, s.r1.p, out);
}

extern "C" int tdgl_psi_update(tdgl_ctx *ctx, const double *psi, const double *mu, double dt,
                               double *psi_out, double *abs_sq_out, int32_t *ok) {
    CTX_GUARD(ctx);
    if (!psi || !mu || !psi_out || !ok) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null argument");
    if (!ctx->have_links || !ctx->have_eps) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "link exponents / epsilon not set");
    Scratch s;
    DevBuf<double2> lap, pnew;
    HIP_TRY(ctx, s.c0.alloc(ctx->n_pad));
    HIP_TRY(ctx, lap.alloc(ctx->n_pad));
    HIP_TRY(ctx, pnew.alloc(ctx->n_pad));
    HIP_TRY(ctx, s.r0.alloc(ctx->n_pad));
    HIP_TRY(ctx, s.r1.alloc(ctx->n_pad));
    TDGL_TRY(upload_sites(ctx, reinterpret_cast<const double2 *>(psi), s.c0));
    TDGL_TRY(upload_sites(ctx, mu, s.r0));
    launch_psi_laplacian(ctx, false, s.c0.p, lap.p);
    launch_psi_update(ctx, s.c0.p, s.r0.p, lap.p, dt, pnew.p, s.r1.p);
    publish_status(ctx);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_status.p, ctx->d_status.p, sizeof(StepStatus), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *ok = ctx->h_status.p->fail_flag ? 0 : 1;
    TDGL_TRY(download_sites(ctx, pnew.p, reinterpret_cast<double2 *>(psi_out)));
    if (abs_sq_out) TDGL_TRY(download_sites(ctx, s.r1.p, abs_sq_out));
    return TDGL_OK;
}

extern "C" int tdgl_poisson_rhs(tdgl_ctx *ctx, const double *psi, double *rhs) {
    CTX_GUARD(ctx);
    if (!psi || !rhs) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null argument");
    if (!ctx->have_links) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "link exponents not set");
    Scratch s;
    HIP_TRY(ctx, s.c0.alloc(ctx->n_pad));
    HIP_TRY(ctx, s.c1.alloc(ctx->n_pad));
    TDGL_TRY(upload_sites(ctx, reinterpret_cast<const double2 *>(psi), s.c0));
    launch_psi_laplacian(ctx, true, s.c0.p, s.c1.p);  // writes ctx->bvec = -a * rhs
    HIP_TRY(ctx, hipGetLastError());
    std::vector<double> b(ctx->n);
    HIP_TRY(ctx, hipMemcpyAsync(b.data(), ctx->bvec.p, ctx->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<double> area(ctx->n);
    HIP_TRY(ctx, hipMemcpyAsync(area.data(), ctx->area.p, ctx->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < ctx->n; ++i) rhs[ctx->perm[i]] = -b[i] / area[i];
    return TDGL_OK;
}

// ---------------------------------------------------------------------------------------
extern "C" int tdgl_time_kernel(tdgl_ctx *ctx, int32_t kernel, int32_t reps, double *avg_ms) {
    CTX_GUARD(ctx);
    if (!avg_ms || reps <= 0) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_time_kernel: bad arguments");
    if (!ctx->have_links || !ctx->have_state || !ctx->have_eps)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_time_kernel: set link exponents, epsilon and state first");
    if ((kernel == 4 || kernel == 5) && ctx->levels.empty())
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_time_kernel: no AMG hierarchy");
    DevBuf<double2> tmp_c;
    DevBuf<double> tmp_r, tmp_r2;
    DevBuf<unsigned> bar_cnt;
    DevBuf<int> bar_err;
    DevBuf<double2> big;
    if (kernel >= 16 && kernel <= 21) HIP_TRY(ctx, big.alloc((size_t)1 << 26));  // 1 GiB
    HIP_TRY(ctx, bar_cnt.alloc(1));
    HIP_TRY(ctx, bar_err.alloc(32));
    HIP_TRY(ctx, tmp_c.alloc(ctx->n_pad));
    HIP_TRY(ctx, tmp_r.alloc(std::max<int64_t>(std::max(ctx->n_pad, ctx->m_pad), 256 * BLOCK)));
    HIP_TRY(ctx, tmp_r2.alloc(std::max(ctx->n_pad, ctx->m_pad)));
    const double2 *psi = ctx->psi[ctx->loop.cur].p;
    auto once = [&]() -> int {
        switch (kernel) {
            case 0: launch_psi_laplacian(ctx, false, psi, tmp_c.p); break;
            case 1: launch_psi_laplacian(ctx, true, psi, tmp_c.p); break;
            case 2: launch_psi_update(ctx, psi, ctx->mu.p, ctx->lap[ctx->loop.cur].p, 1e-4, tmp_c.p, nullptr); break;
            case 3: launch_edge_currents(ctx, psi, ctx->mu.p, tmp_r.p, tmp_r2.p); break;
            case 4: poisson_spmv_level0(ctx, ctx->mu.p, tmp_r.p); break;
            case 5: (void)vcycle_level(ctx, 0, ctx->bvec.p, nullptr); break;
            case 6:
                hipLaunchKernelGGL(k_copy_d2, dim3(grid_for(ctx->n_pad)), dim3(BLOCK), 0, ctx->stream,
                                   ctx->n_pad, psi, tmp_c.p);
                break;
            case 7:
                if (!ctx->scr_enabled) return TDGL_ERR_ARG;
                launch_direct(ctx);
                break;
            case 22:  // one evaluation of the screening treecode
                if (!ctx->scr_enabled || !tree_active(ctx)) return TDGL_ERR_ARG;
                launch_tree(ctx);
                break;
            case 8:  // two trivial kernels, the second on the communication stream and back
                hipLaunchKernelGGL(k_copy_d2, dim3(1), dim3(BLOCK), 0, ctx->stream, 64, psi, tmp_c.p);
                (void)hipEventRecord(ctx->ev_pack, ctx->stream);
                (void)hipStreamWaitEvent(ctx->comm_stream, ctx->ev_pack, 0);
                hipLaunchKernelGGL(k_copy_d2, dim3(1), dim3(BLOCK), 0, ctx->comm_stream, 64, psi, tmp_c.p + 64);
                (void)hipEventRecord(ctx->ev_halo, ctx->comm_stream);
                (void)hipStreamWaitEvent(ctx->stream, ctx->ev_halo, 0);
                break;
            case 9:  // the same two kernels in one stream
                hipLaunchKernelGGL(k_copy_d2, dim3(1), dim3(BLOCK), 0, ctx->stream, 64, psi, tmp_c.p);
                hipLaunchKernelGGL(k_copy_d2, dim3(1), dim3(BLOCK), 0, ctx->stream, 64, psi, tmp_c.p + 64);
                break;
            case 10: case 11: case 12: case 13: case 14: case 15: {
                // 100 device-wide barriers inside one launch (k_barrier_bench): 10 / 11 grid.sync() with 32 /
                // 256 workgroups; 12 / 13 counter + agent-scope fences with 32 / 256; 14 the 32 workgroups
                // of one XCD (every 8th of 256) with agent-scope fences; 15 the same with L2-local fences
                const int mode = kernel <= 11 ? 0 : (kernel <= 14 ? 1 : 2);
                int stride = kernel >= 14 ? 8 : 1;
                const int grid = (kernel == 10 || kernel == 12) ? 32 : 256;
                int iters = 100, workers = grid / stride;
                (void)hipMemsetAsync(bar_cnt.p, 0, sizeof(unsigned), ctx->stream);
                unsigned *cnt = bar_cnt.p;
                double *data = tmp_r.p;
                int *err = bar_err.p;
                if (mode == 0) {
                    void *args[] = {&iters, &stride, &workers, &cnt, &data, &err};
                    if (hipLaunchCooperativeKernel(reinterpret_cast<void *>(k_barrier_bench<0>), dim3(grid), dim3(BLOCK), args, 0,
                                                   ctx->stream) != hipSuccess)
                        return TDGL_ERR_HIP;
                } else if (mode == 1) {
                    hipLaunchKernelGGL(k_barrier_bench<1>, dim3(grid), dim3(BLOCK), 0, ctx->stream, iters, stride, workers, cnt, data, err);
                } else {
                    hipLaunchKernelGGL(k_barrier_bench<2>, dim3(grid), dim3(BLOCK), 0, ctx->stream, iters, stride, workers, cnt, data, err);
                }
                break;
            }
            case 16:  // read-only stream over 1 GiB (HBM-cold: four times the Infinity Cache)
                hipLaunchKernelGGL(k_stream_read<4>, dim3(256 * 8), dim3(BLOCK), 0, ctx->stream, (int64_t)big.n, (const double2 *)big.p,
                                   tmp_r.p);
                break;
            case 18:  // ... 8 loads per lane in flight
                hipLaunchKernelGGL(k_stream_read<8>, dim3(256 * 8), dim3(BLOCK), 0, ctx->stream, (int64_t)big.n, (const double2 *)big.p,
                                   tmp_r.p);
                break;
            case 19:  // ... 16 workgroups per CU
                hipLaunchKernelGGL(k_stream_read<4>, dim3(256 * 16), dim3(BLOCK), 0, ctx->stream, (int64_t)big.n, (const double2 *)big.p,
                                   tmp_r.p);
                break;
            case 20:  // ... one pass, no loop: a workgroup per 256 x 2 entries
                hipLaunchKernelGGL(k_stream_read<2>, dim3((unsigned)(big.n / (BLOCK * 2))), dim3(BLOCK), 0, ctx->stream, (int64_t)big.n,
                                   (const double2 *)big.p, tmp_r.p);
                break;
            case 21:  // one workgroup reading 2 MiB from L2, 50 times
                hipLaunchKernelGGL(k_one_cu_read, dim3(1), dim3(1024), 0, ctx->stream, 50, (int64_t)(1 << 17), (const double2 *)big.p,
                                   tmp_r.p);
                break;
            case 17:  // copy 512 MiB -> 512 MiB
                hipLaunchKernelGGL(k_stream_copy<4>, dim3(256 * 8), dim3(BLOCK), 0, ctx->stream, (int64_t)big.n / 2,
                                   (const double2 *)big.p, big.p + big.n / 2);
                break;
            default: return TDGL_ERR_ARG;
        }
        return TDGL_OK;
    };
    for (int i = 0; i < 3; ++i)
        if (once() != TDGL_OK) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_time_kernel: unknown kernel %d", kernel);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (int i = 0; i < reps; ++i) (void)once();
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
    HIP_TRY(ctx, hipGetLastError());
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *avg_ms = (double)ms / reps;
    if (kernel >= 10 && kernel <= 15) {  // stale reads, block -> XCD mapping: reported through the error string
        int h[17] = {0};
        HIP_TRY(ctx, hipMemcpy(h, bar_err.p, sizeof(h), hipMemcpyDeviceToHost));
        char buf[256];
        int off = snprintf(buf, sizeof(buf), "barrier bench %d: stale reads %d; XCC_ID of blocks 0-15:", kernel, h[0]);
        for (int b = 0; b < 16 && off < (int)sizeof(buf) - 4; ++b) off += snprintf(buf + off, sizeof(buf) - off, " %d", h[1 + b]);
        ctx->err = buf;
    }
    ctx->psi_status_pending = false;  // (the psi-update kernel may have run on scratch data)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

#include "ensemble_sub.inc"
#include "ensemble.inc"
