// Screening: self-consistent induced vector potential inside every step.
// Included by tdgl_hip.hip.
//
// Reference: TDGLSolver.get_induced_vector_potential and the screening loop of update()
// (tdgl/solver/solver.py:522-578, 654-688); the O(n_edges x n_sites) kernel is
// tdgl/solver/screening.py:12-75 (Numba / CuPy JIT in the reference).  This is the one
// compute-bound piece of the path: ~11 fp64 operations per (edge, site) pair, no reuse of HBM
// data beyond the site tile staged in LDS.

namespace tdgl {

__global__ __launch_bounds__(BLOCK) void k_abs_sq(int64_t n, const double2 *__restrict__ psi,
                                                  double *__restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i < n) out[i] = psi[i].x * psi[i].x + psi[i].y * psi[i].y;
}

// Mesh.get_quantity_on_site (tdgl/finite_volume/mesh.py:203-243) of K_e = J_s,e + J_n,e:
// mean over the incident edges of K_e * e_hat (the edge's own direction for both end sites),
// divided by 2.  Gathered through the SELL slots of the site graph.
__global__ __launch_bounds__(BLOCK) void k_site_average(int n_slices, int64_t n_rows,
                                                        const int32_t *__restrict__ slice_off,
                                                        const int32_t *__restrict__ slot_edge,
                                                        const double *__restrict__ js,
                                                        const double *__restrict__ jn,
                                                        const double *__restrict__ dx,
                                                        const double *__restrict__ dy,
                                                        const double *__restrict__ inv_len,
                                                        const double *__restrict__ inv_2deg,
                                                        double *__restrict__ out) {
    const int slice = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
    if (slice >= n_slices) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t row = (int64_t)slice * WAVE + lane;
    if (row >= n_rows) return;
    double ax = 0.0, ay = 0.0;
    int64_t idx = (int64_t)slice_off[slice] * WAVE + lane;
    for (int k = slice_off[slice]; k < slice_off[slice + 1]; ++k, idx += WAVE) {
        const int32_t code = slot_edge[idx];
        if (code < 0) continue;
        const int e = code >> 1;
        const double f = (js[e] + jn[e]) * inv_len[e];
        ax += f * dx[e];
        ay += f * dy[e];
    }
    out[2 * row] = ax * inv_2deg[row];
    out[2 * row + 1] = ay * inv_2deg[row];
}

// owned site currents -> their slots in the global array (zeroed before; summed over ranks after)
__global__ __launch_bounds__(BLOCK) void k_scatter_sites(int64_t n_own, const int64_t *__restrict__ gid,
                                                         const double *__restrict__ J, double *__restrict__ Jg) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i >= n_own) return;
    Jg[2 * gid[i]] = J[2 * i];
    Jg[2 * gid[i] + 1] = J[2 * i + 1];
}

// A_new[e] = sum_j K_site[j] * area_j / |r_e - r_j|   (screening.py:35-42): the one compute-bound
// kernel of the path (fp64 vector units; ~12 flops per (edge, site) pair, no HBM traffic to speak
// of).  Each thread owns EPT edges in registers; the sites stream through LDS in tiles of BLOCK
// as (x, y, area*Kx, area*Ky), read back as wave-wide broadcasts.  1/sqrt is v_rsq_f64 plus one
// cubically convergent correction (full double precision) instead of a sqrt and a divide.
// blockIdx.y splits the site range so that small meshes still fill 256 CUs; the partial sums
// land in Apart[chunk][edge] and k_polyak adds them in chunk order (deterministic).
constexpr int EPT = 2;

__device__ __forceinline__ double rsqrt_f64(double x) {
    const double y0 = __builtin_amdgcn_rsq(x);
    const double e = fma(-x * y0, y0, 1.0);
    return fma(y0 * e, fma(e, 0.375, 0.5), y0);
}

__global__ __launch_bounds__(BLOCK) void k_induced_vector_potential(
    int64_t m, int64_t n, int64_t m_stride, int tiles_per_chunk, const double *__restrict__ edge_xy,
    const double *__restrict__ site_xyw, const double *__restrict__ Jsite, double *__restrict__ Apart) {
    __shared__ double4 tile[BLOCK];
    double ex[EPT], ey[EPT], ax[EPT], ay[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int64_t e = ((int64_t)blockIdx.x * EPT + k) * BLOCK + threadIdx.x;
        ex[k] = (e < m) ? edge_xy[2 * e] : 0.0;
        ey[k] = (e < m) ? edge_xy[2 * e + 1] : 0.0;
        ax[k] = ay[k] = 0.0;
    }
    const int64_t j0 = (int64_t)blockIdx.y * tiles_per_chunk * BLOCK;
    const int64_t j1 = min(n, j0 + (int64_t)tiles_per_chunk * BLOCK);
    for (int64_t base = j0; base < j1; base += BLOCK) {
        const int64_t j = base + threadIdx.x;
        if (j < j1) {
            const double a = site_xyw[3 * j + 2];
            tile[threadIdx.x] = make_double4(site_xyw[3 * j], site_xyw[3 * j + 1], a * Jsite[2 * j], a * Jsite[2 * j + 1]);
        } else {  // padding: zero weight, far from every edge centre
            tile[threadIdx.x] = make_double4(1e150, 1e150, 0.0, 0.0);
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < BLOCK; ++t) {
            const double4 s = tile[t];
#pragma unroll
            for (int k = 0; k < EPT; ++k) {
                const double ddx = ex[k] - s.x, ddy = ey[k] - s.y;
                const double rinv = rsqrt_f64(fma(ddx, ddx, ddy * ddy));
                ax[k] = fma(s.z, rinv, ax[k]);
                ay[k] = fma(s.w, rinv, ay[k]);
            }
        }
        __syncthreads();
    }
    double *out = Apart + (int64_t)blockIdx.y * 2 * m_stride;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int64_t e = ((int64_t)blockIdx.x * EPT + k) * BLOCK + threadIdx.x;
        if (e < m) {
            out[2 * e] = ax[k];
            out[2 * e + 1] = ay[k];
        }
    }
}

// Polyak's heavy-ball update (solver.py:564-575): dA = A_new - A; v = (1 - beta) v + alpha dA;
// A += v; error = max_e |dA_e| / max(|A_e|, 1e-20) with the UPDATED A in the denominator.
__global__ __launch_bounds__(BLOCK) void k_polyak(int64_t m, int64_t m_stride, int n_chunks, double alpha, double beta,
                                                  const double *__restrict__ Apart, double *__restrict__ A,
                                                  double *__restrict__ vel, unsigned long long *__restrict__ err_bits) {
    const int64_t e = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    double ratio = 0.0;
    if (e < m) {
        double nax = 0.0, nay = 0.0;
        for (int c = 0; c < n_chunks; ++c) {
            nax += Apart[(int64_t)c * 2 * m_stride + 2 * e];
            nay += Apart[(int64_t)c * 2 * m_stride + 2 * e + 1];
        }
        const double dax = nax - A[2 * e], day = nay - A[2 * e + 1];
        const double vx = (1.0 - beta) * vel[2 * e] + alpha * dax, vy = (1.0 - beta) * vel[2 * e + 1] + alpha * day;
        vel[2 * e] = vx;
        vel[2 * e + 1] = vy;
        const double nx = A[2 * e] + vx, ny = A[2 * e + 1] + vy;
        A[2 * e] = nx;
        A[2 * e + 1] = ny;
        ratio = sqrt(dax * dax + day * day) / fmax(sqrt(nx * nx + ny * ny), 1e-20);
    }
    const double bm = block_max(ratio);
    if (threadIdx.x == 0 && bm > 0.0) atomicMax(err_bits, (unsigned long long)__double_as_longlong(bm));
}

}  // namespace tdgl

// ---------------------------------------------------------------------------------------
// common set-up; `global`: one-process-per-GPU mode (sites_xy / site_areas are GLOBAL arrays of
// n_global sites in global order, owned_gid the global ids of this rank's owned sites)
static int set_screening_impl(tdgl_ctx *ctx, const tdgl_screening_options *o, const double *sites_xy,
                              const double *edge_centers_xy, const double *site_areas, const int64_t *owned_gid) {
    if (!sites_xy || !edge_centers_xy || !site_areas) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_screening: null array");
    // messages as in tdgl/solver/options.py:107-123
    if (!(o->step_drag > 0 && o->step_drag <= 1)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "screening_step_drag must be in (0, 1] (got %g).", o->step_drag);
    if (!(o->step_size > 0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "screening_step_size must be in > 0 (got %g).", o->step_size);
    if (!(o->tolerance > 0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "screening_tolerance must be in > 0 (got %g).", o->tolerance);
    ctx->scr = *o;
    ctx->scr_tree.reset();  // (new geometry: the all-pairs kernel until tdgl_set_screening_tree is called again)
    const bool global = owned_gid != nullptr;
    const int64_t n = ctx->n, m = ctx->m;
    const int64_t ns = global ? ctx->n_global : n;  // sites of the 1/r sum
    const int64_t ns_pad = round_up(std::max<int64_t>(ns, 1), WAVE);
    std::vector<double> sxyw(3 * ns_pad, 0.0), exy(2 * ctx->m_pad, 0.0), inv2deg(ctx->n_pad, 0.0);
    std::vector<int32_t> deg(n, 0);
    std::vector<int32_t> e0(m), e1(m);
    HIP_TRY(ctx, hipMemcpy(e0.data(), ctx->e0.p, m * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(e1.data(), ctx->e1.p, m * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < m; ++k) {
        deg[e0[k]]++;
        deg[e1[k]]++;
        const int32_t e = ctx->edge_perm[k];
        exy[2 * k] = edge_centers_xy[2 * e];
        exy[2 * k + 1] = edge_centers_xy[2 * e + 1];
    }
    for (int64_t i = 0; i < ns; ++i) {
        const int64_t r = global ? i : ctx->perm[i];
        sxyw[3 * i] = sites_xy[2 * r];
        sxyw[3 * i + 1] = sites_xy[2 * r + 1];
        sxyw[3 * i + 2] = site_areas[r];
    }
    // (owned sites see all their edges, also in one-process-per-GPU mode)
    for (int64_t i = 0; i < n; ++i) inv2deg[i] = deg[i] > 0 ? 1.0 / (2.0 * deg[i]) : 0.0;
    HIP_TRY(ctx, ctx->scr_site_xyw.upload(sxyw));
    HIP_TRY(ctx, ctx->scr_edge_xy.upload(exy));
    HIP_TRY(ctx, ctx->scr_inv_2deg.upload(inv2deg));
    HIP_TRY(ctx, ctx->scr_Jsite.alloc(2 * ctx->n_pad));
    HIP_TRY(ctx, ctx->scr_Aind.alloc(2 * ctx->m_pad));
    HIP_TRY(ctx, ctx->scr_vel.alloc(2 * ctx->m_pad));
    ctx->scr_n_sites = ns;
    if (global) {
        std::vector<int64_t> gid(owned_gid, owned_gid + ctx->n_own);
        for (int64_t g : gid)
            if (g < 0 || g >= ns) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_screening_distributed: bad global site id %lld", (long long)g);
        HIP_TRY(ctx, ctx->scr_owned_gid.upload(gid));
        HIP_TRY(ctx, ctx->scr_Jglobal.alloc(2 * ns_pad));
        if (ctx->d_gstat.n < 2) HIP_TRY(ctx, ctx->d_gstat.alloc(2));
    }
    {   // split the site range over blockIdx.y until the launch has >= ~2048 workgroups.  In
        // one-process-per-GPU mode the split depends on the GLOBAL site count only, so that both
        // owners of a cut edge add the chunks in the same order and get the same bits.
        const int64_t eblocks = (m + (int64_t)EPT * BLOCK - 1) / ((int64_t)EPT * BLOCK);
        const int64_t tiles = (ns + BLOCK - 1) / BLOCK;
        int64_t chunks = global ? std::min<int64_t>(tiles, 16)
                                : std::min<int64_t>(std::min<int64_t>(tiles, 64), std::max<int64_t>(1, 2048 / eblocks));
        ctx->scr_tiles_per_chunk = (int)((tiles + chunks - 1) / chunks);
        ctx->scr_chunks = (int)((tiles + ctx->scr_tiles_per_chunk - 1) / ctx->scr_tiles_per_chunk);
    }
    HIP_TRY(ctx, ctx->scr_Anew.alloc((size_t)ctx->scr_chunks * 2 * ctx->m_pad));
    HIP_TRY(ctx, ctx->abs_sq_old.alloc(ctx->n_pad));
    HIP_TRY(ctx, ctx->scr_err_bits.alloc(1));
    ctx->scr_enabled = true;
    ctx->lap_valid = false;
    return TDGL_OK;
}

extern "C" int tdgl_set_screening(tdgl_ctx *ctx, const tdgl_screening_options *o, const double *sites_xy,
                                  const double *edge_centers_xy, const double *site_areas) {
    CTX_GUARD(ctx);
    if (!o) {
        ctx->scr_enabled = false;
        ctx->scr_tree.reset();
        return TDGL_OK;
    }
    if (distributed(ctx) || ctx->n_own != ctx->n)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "one-process-per-GPU mode: use tdgl_set_screening_distributed");
    return set_screening_impl(ctx, o, sites_xy, edge_centers_xy, site_areas, nullptr);
}

extern "C" int tdgl_set_screening_distributed(tdgl_ctx *ctx, const tdgl_screening_options *o,
                                              const double *global_sites_xy, const double *global_site_areas,
                                              const int64_t *owned_global_ids, const double *edge_centers_xy) {
    CTX_GUARD(ctx);
    if (!o) {
        ctx->scr_enabled = false;
        ctx->scr_tree.reset();
        return TDGL_OK;
    }
    if (ctx->send_ptr.empty() || ctx->n_global < ctx->n_own)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "call tdgl_set_halo_plan first");
    if (!owned_global_ids) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_screening_distributed: null ids");
    return set_screening_impl(ctx, o, global_sites_xy, edge_centers_xy, global_site_areas, owned_global_ids);
}

extern "C" int tdgl_set_induced_vector_potential(tdgl_ctx *ctx, const double *A) {
    CTX_GUARD(ctx);
    if (!ctx->scr_enabled) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "screening is not enabled");
    if (!A) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null array");
    std::vector<double> tmp(2 * ctx->m_pad, 0.0);
    for (int64_t k = 0; k < ctx->m; ++k) {
        tmp[2 * k] = A[2 * ctx->edge_perm[k]];
        tmp[2 * k + 1] = A[2 * ctx->edge_perm[k] + 1];
    }
    HIP_TRY(ctx, hipMemcpy(ctx->scr_Aind.p, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->lap_valid = false;
    return TDGL_OK;
}

extern "C" int tdgl_get_induced_vector_potential(tdgl_ctx *ctx, double *A) {
    CTX_GUARD(ctx);
    if (!A) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null array");
    if (!ctx->scr_enabled) {
        memset(A, 0, 2 * ctx->m * sizeof(double));
        return TDGL_OK;
    }
    std::vector<double> tmp(2 * ctx->m);
    HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), ctx->scr_Aind.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t k = 0; k < ctx->m; ++k) {
        A[2 * ctx->edge_perm[k]] = tmp[2 * k];
        A[2 * ctx->edge_perm[k] + 1] = tmp[2 * k + 1];
    }
    return TDGL_OK;
}

static void launch_direct(tdgl_ctx *ctx) {
    const int gx = (int)((ctx->m + (int64_t)EPT * BLOCK - 1) / ((int64_t)EPT * BLOCK));
    const bool global = ctx->scr_Jglobal.n > 0;
    hipLaunchKernelGGL(k_induced_vector_potential, dim3(gx, ctx->scr_chunks), dim3(BLOCK), 0, ctx->stream, ctx->m,
                       ctx->scr_n_sites, ctx->m_pad, ctx->scr_tiles_per_chunk, ctx->scr_edge_xy.p, ctx->scr_site_xyw.p,
                       global ? ctx->scr_Jglobal.p : ctx->scr_Jsite.p, ctx->scr_Anew.p);
}

static bool tree_active(const tdgl_ctx *ctx);
static void launch_tree(tdgl_ctx *ctx);  // (screening_tree.inc)

// A_new for the site currents in scr_Jsite with the active method: partial sums in the first induced_chunks()
// chunks of scr_Anew (the treecode writes one)
static void launch_induced(tdgl_ctx *ctx) {
    if (tree_active(ctx))
        launch_tree(ctx);
    else
        launch_direct(ctx);
}
static int induced_chunks(const tdgl_ctx *ctx) { return tree_active(ctx) ? 1 : ctx->scr_chunks; }

// Single-operator entry point: A_new = sum_j <K>_j area_j / |r_e - r_j| for an edge current K
// (reference edge order in and out), without the heavy-ball update.
extern "C" int tdgl_induced_vector_potential(tdgl_ctx *ctx, const double *edge_current, double *A_new) {
    CTX_GUARD(ctx);
    if (!ctx->scr_enabled) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "screening is not enabled");
    if (!edge_current || !A_new) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null array");
    const int64_t m = ctx->m;
    std::vector<double> k_int(ctx->m_pad, 0.0);
    for (int64_t k = 0; k < m; ++k) k_int[k] = edge_current[ctx->edge_perm[k]];
    DevBuf<double> dk, zero;
    HIP_TRY(ctx, dk.upload(k_int));
    HIP_TRY(ctx, zero.alloc(ctx->m_pad));
    const int ns = ctx->lap_pat.n_slices;
    hipLaunchKernelGGL(k_site_average, dim3(grid_for((int64_t)ns * WAVE)), dim3(BLOCK), 0, ctx->stream, ns,
                       ctx->lap_pat.n_rows, ctx->lap_pat.slice_off.p, ctx->lap_slot_edge.p, dk.p, zero.p,
                       ctx->e_dirx.p, ctx->e_diry.p, ctx->e_inv_len.p, ctx->scr_inv_2deg.p, ctx->scr_Jsite.p);
    launch_induced(ctx);
    const int chunks = induced_chunks(ctx);
    std::vector<double> part((size_t)chunks * 2 * ctx->m_pad);
    HIP_TRY(ctx, hipMemcpyAsync(part.data(), ctx->scr_Anew.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    for (int64_t k = 0; k < m; ++k) {
        double ax = 0.0, ay = 0.0;
        for (int c = 0; c < chunks; ++c) {  // same order as k_polyak
            ax += part[(size_t)c * 2 * ctx->m_pad + 2 * k];
            ay += part[(size_t)c * 2 * ctx->m_pad + 2 * k + 1];
        }
        A_new[2 * ctx->edge_perm[k]] = ax;
        A_new[2 * ctx->edge_perm[k] + 1] = ay;
    }
    return TDGL_OK;
}

// link variables from A_applied + A_induced, and the covariant Laplacian values (solver.py:670-673)
static void screening_refresh_links(tdgl_ctx *ctx) { launch_links(ctx, ctx->scr_Aind.p, nullptr); }

// get_induced_vector_potential (solver.py:522-578) for the currents in ctx->js / ctx->jn;
// returns the relative change (screening error) through *err.
static int screening_update_A(tdgl_ctx *ctx, double *err) {
    const int ns = ctx->lap_pat.n_slices;
    hipLaunchKernelGGL(k_site_average, dim3(grid_for((int64_t)ns * WAVE)), dim3(BLOCK), 0, ctx->stream, ns,
                       ctx->lap_pat.n_rows, ctx->lap_pat.slice_off.p, ctx->lap_slot_edge.p, ctx->js.p, ctx->jn.p,
                       ctx->e_dirx.p, ctx->e_diry.p, ctx->e_inv_len.p, ctx->scr_inv_2deg.p, ctx->scr_Jsite.p);
    if (ctx->scr_Jglobal.n > 0) {  // one process per GPU: everybody needs the site currents of all sites
        HIP_TRY(ctx, hipMemsetAsync(ctx->scr_Jglobal.p, 0, ctx->scr_Jglobal.n * sizeof(double), ctx->stream));
        hipLaunchKernelGGL(k_scatter_sites, dim3(grid_for(ctx->n_own)), dim3(BLOCK), 0, ctx->stream, ctx->n_own,
                           ctx->scr_owned_gid.p, ctx->scr_Jsite.p, ctx->scr_Jglobal.p);
        TDGL_TRY(comm_allreduce(ctx, ctx->scr_Jglobal.p, 2 * ctx->scr_n_sites, 0));
    }
    launch_induced(ctx);
    HIP_TRY(ctx, hipMemsetAsync(ctx->scr_err_bits.p, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_polyak, dim3(grid_for(ctx->m)), dim3(BLOCK), 0, ctx->stream, ctx->m, ctx->m_pad,
                       induced_chunks(ctx), ctx->scr.step_size, ctx->scr.step_drag, ctx->scr_Anew.p, ctx->scr_Aind.p,
                       ctx->scr_vel.p, ctx->scr_err_bits.p);
    unsigned long long bits = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bits, ctx->scr_err_bits.p, sizeof(bits), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    *err = __builtin_bit_cast(double, bits);
    if (distributed(ctx)) {  // the same decision on every rank: max over ranks
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_gstat.p, err, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        TDGL_TRY(comm_allreduce(ctx, ctx->d_gstat.p, 1, 1));
        HIP_TRY(ctx, hipMemcpyAsync(err, ctx->d_gstat.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return TDGL_OK;
}
