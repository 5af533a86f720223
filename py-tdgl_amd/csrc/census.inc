// Census of the live state: for every accepted step one int32 row (n_plus, n_minus, w_0 .. w_{L-1}) -- the number of
// mesh triangles with charge +1 / -1 and the winding of arg psi around every closed loop of sites -- taken inside the
// time loops from psi in the context's internal (RCM) numbering.  Included by tdgl_hip.hip after vortices.inc, before
// run.inc.  DESIGN.md section 3, "Census in the loop".
//
// The rules are those of the vortex plan (vortex_rules.h: the same device functions), so a row equals what
// tdgl_vortex_plan_find counts on the same psi, and tdgl_amd.vortices.triangle_charges / loop_winding in NumPy.
//
// One launch per attempt.  Workgroups [0, nblk_tri), at most CENSUS_MAX_BLOCKS of them striding over the triangles: one
// lane per triangle, wave ballots of charge > 0 and charge < 0 summed per wavefront, the four wavefronts' sums added in
// LDS, and one integer atomicAdd per workgroup and sign that found any -- at most 2 CENSUS_MAX_BLOCKS per step whatever
// the state (integer sums: the total is the same in any order).  The workgroups behind them: one wavefront per loop,
// which writes the winding itself.  The counter columns of the ring are
// zero before a row is used: the ring is cleared on the stream when tdgl_run begins and behind every flush.
//
//   k_census       classic loop, launched by step_finish next to k_probes: the row of the step just accepted
//   k_ra_census    run-ahead loop, behind the direct solve: predicated on StepCtl like k_ra_probes
//   k_ens_census   ensemble: the replica as grid.y, like k_ens_probes

namespace tdgl {

__device__ inline void census_body(const CensusPlan &c, int blk, const double2 *__restrict__ psi, int32_t *__restrict__ row) {
    __shared__ int wave_plus[BLOCK / WAVE], wave_minus[BLOCK / WAVE];
    const int lane = threadIdx.x & (WAVE - 1);
    if (blk < c.nblk_tri) {  // (uniform in the workgroup, like the loop below: every lane reaches the ballots and the barrier)
        int plus = 0, minus = 0;
        for (int64_t base = (int64_t)blk * BLOCK; base < c.n_tri; base += (int64_t)c.nblk_tri * BLOCK) {
            const int64_t t = base + threadIdx.x;
            int w = 0;
            if (t < c.n_tri) {
                const double2 a = psi[c.elements[t]], b = psi[c.elements[(int64_t)c.n_tri + t]],
                              d = psi[c.elements[2 * (int64_t)c.n_tri + t]];
                w = vortex_triangle_winding(a, b, d) * (int)c.orient[t];
            }
            plus += __popcll(__ballot(w > 0));  // every lane of the wave takes part
            minus += __popcll(__ballot(w < 0));
        }
        if (lane == 0) {
            wave_plus[threadIdx.x / WAVE] = plus;
            wave_minus[threadIdx.x / WAVE] = minus;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int p = 0, m = 0;
            for (int k = 0; k < BLOCK / WAVE; ++k) p += wave_plus[k], m += wave_minus[k];
            if (p) atomicAdd(row, p);
            if (m) atomicAdd(row + 1, m);
        }
        return;
    }
    const int l = (blk - c.nblk_tri) * (BLOCK / WAVE) + threadIdx.x / WAVE;  // uniform in the wave
    if (l >= c.n_loops) return;
    const int w = vortex_loop_winding(psi, c.loop_sites, c.loop_ptr[l], c.loop_ptr[l + 1], lane);
    if (lane == 0) row[2 + l] = w;
}

__global__ __launch_bounds__(BLOCK) void k_census(CensusPlan c, const double2 *__restrict__ psi, int32_t *__restrict__ row) {
    census_body(c, blockIdx.x, psi, row);
}

// an ACCEPTED attempt's census into the slot of its step (the controller has flipped cur: psi^{n+1})
__global__ __launch_bounds__(BLOCK) void k_ra_census(CensusPlan c, const double2 *__restrict__ psi0,
                                                     const double2 *__restrict__ psi1, int32_t *__restrict__ ring,
                                                     int slot_base, const StepCtl *__restrict__ ctl) {
    if (!ctl->live || !ctl->last_ok) return;
    census_body(c, blockIdx.x, ctl->cur != 0 ? psi1 : psi0, ring + (size_t)(slot_base + ctl->n_acc - 1) * c.ncol);
}

// ... per replica blockIdx.y, into slot n_acc - 1 of the replica's RA_BATCH_MAX rows
__global__ __launch_bounds__(BLOCK) void k_ens_census(CensusPlan c, const double2 *__restrict__ psi0,
                                                      const double2 *__restrict__ psi1, int64_t n_pad,
                                                      int32_t *__restrict__ ring, const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    const StepCtl *s = ctl + r;
    if (!s->live || !s->last_ok) return;
    census_body(c, blockIdx.x, (s->cur != 0 ? psi1 : psi0) + (int64_t)r * n_pad,
                ring + ((int64_t)r * RA_BATCH_MAX + s->n_acc - 1) * c.ncol);
}

}  // namespace tdgl

// the step just accepted (classic loop): psi = psi^{n+1}
static void census_launch(tdgl_ctx *ctx, const double2 *psi) {
    Census &c = ctx->census;
    hipLaunchKernelGGL(k_census, dim3(c.grid()), dim3(BLOCK), 0, ctx->stream, c.plan(), psi,
                       c.ring.p + (size_t)c.ring_count * c.ncol());
    c.ring_count += 1;
}

// one attempt of a run-ahead batch whose first accepted step takes row c.ring_count
static void census_launch_ra(tdgl_ctx *ctx) {
    Census &c = ctx->census;
    hipLaunchKernelGGL(k_ra_census, dim3(c.grid()), dim3(BLOCK), 0, ctx->stream, c.plan(), (const double2 *)ctx->psi[0].p,
                       (const double2 *)ctx->psi[1].p, c.ring.p, c.ring_count, (const StepCtl *)ctx->d_ctl.p);
}

// tdgl_run begins: no rows, every counter of the ring zero
static int census_begin_run(tdgl_ctx *ctx) {
    Census &c = ctx->census;
    c.ring_count = 0;
    c.rows.clear();
    if (c.on()) HIP_TRY(ctx, hipMemsetAsync(c.ring.p, 0, c.ring.n * sizeof(int32_t), ctx->stream));
    return TDGL_OK;
}

// the two halves of a flush around the host synchronisation that the probe ring's flush makes (run.inc:
// probe_ring_flush): queue the copy of the rows written and the clearing behind it; afterwards, keep them
static int census_flush_queue(tdgl_ctx *ctx, int *count) {
    Census &c = ctx->census;
    *count = c.ring_count;
    c.ring_count = 0;
    if (*count == 0) return TDGL_OK;
    const size_t bytes = (size_t)*count * c.ncol() * sizeof(int32_t);
    HIP_TRY(ctx, hipMemcpyAsync(c.h_ring.p, c.ring.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(c.ring.p, 0, bytes, ctx->stream));
    return TDGL_OK;
}

static void census_flush_keep(tdgl_ctx *ctx, int count) {
    Census &c = ctx->census;
    c.rows.insert(c.rows.end(), c.h_ring.p, c.h_ring.p + (size_t)count * c.ncol());
}

extern "C" int tdgl_set_census(tdgl_ctx *ctx, const double *sites_xy, int64_t n_tri, const int32_t *elements,
                               int32_t n_loops, const int64_t *loop_ptr, const int32_t *loop_sites) {
    CTX_GUARD(ctx);
    if (n_tri < 0 || n_loops < 0)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_census: negative size (n_tri %lld, n_loops %d)", (long long)n_tri, (int)n_loops);
    static int64_t serial = 0;  // (every call that changes the census gets its own number)
    if (n_tri == 0 && n_loops == 0) {  // off
        ctx->census = Census();
        ctx->census.serial = ++serial;
        return TDGL_OK;
    }
    if (ctx->n_own != ctx->n || distributed(ctx))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_census: not available in one-process-per-GPU mode (a rank holds a part of every loop)");
    const int64_t n = ctx->n;
    if (n_tri > INT32_MAX / 3) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_census: n_tri must be below 2^31 / 3 (got %lld)", (long long)n_tri);
    if ((n_tri > 0 && (!elements || !sites_xy)) || (n_loops > 0 && (!loop_ptr || !loop_sites)))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_census: null array");
    for (int64_t k = 0; k < 3 * n_tri; ++k)
        if (elements[k] < 0 || elements[k] >= n)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_census: element %lld names site %d, out of range for %lld sites",
                      (long long)(k / 3), (int)elements[k], (long long)n);
    if (n_loops > 0 && loop_ptr[0] != 0)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_census: loop_ptr[0] must be 0 (got %lld)", (long long)loop_ptr[0]);
    for (int32_t l = 0; l < n_loops; ++l)
        if (loop_ptr[l + 1] - loop_ptr[l] < 3)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_census: loop %d has %lld sites, a loop needs at least 3", (int)l,
                      (long long)(loop_ptr[l + 1] - loop_ptr[l]));
    const int64_t n_loop_sites = n_loops > 0 ? loop_ptr[n_loops] : 0;
    for (int64_t k = 0; k < n_loop_sites; ++k)
        if (loop_sites[k] < 0 || loop_sites[k] >= n)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_census: loop site %d out of range for %lld sites", (int)loop_sites[k], (long long)n);
    // triangles in the internal numbering, ordered by their lowest site for locality (counts do not depend on the
    // order); the orientation is that of the vertices as given, from the coordinates in the reference numbering
    const std::vector<int32_t> &ip = ctx->iperm;
    std::vector<int64_t> order((size_t)n_tri);
    std::iota(order.begin(), order.end(), (int64_t)0);
    auto lowest = [&](int64_t t) { return std::min({ip[elements[3 * t]], ip[elements[3 * t + 1]], ip[elements[3 * t + 2]]}); };
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return lowest(a) < lowest(b); });
    std::vector<int32_t> el((size_t)(3 * n_tri)), ls((size_t)n_loop_sites);
    std::vector<int8_t> orient((size_t)n_tri);
    for (int64_t k = 0; k < n_tri; ++k) {
        const int32_t *v = elements + 3 * order[k];
        for (int j = 0; j < 3; ++j) el[(size_t)(j * n_tri + k)] = ip[v[j]];
        orient[k] = vortex_orientation(sites_xy + 2 * (int64_t)v[0], sites_xy + 2 * (int64_t)v[1], sites_xy + 2 * (int64_t)v[2]);
    }
    for (int64_t k = 0; k < n_loop_sites; ++k) ls[k] = ip[loop_sites[k]];
    // built aside and moved in whole: a call that fails leaves the previous census in place
    Census c;
    c.n_tri = (int32_t)n_tri;
    c.n_loops = n_loops;
    HIP_TRY(ctx, c.elements.upload(el));
    HIP_TRY(ctx, c.orient.upload(orient));
    HIP_TRY(ctx, c.loop_ptr.upload(std::vector<int64_t>(loop_ptr, loop_ptr + (n_loops > 0 ? n_loops + 1 : 0))));
    HIP_TRY(ctx, c.loop_sites.upload(ls));
    HIP_TRY(ctx, c.ring.alloc((size_t)PROBE_RING_STEPS * c.ncol()));
    HIP_TRY(ctx, c.h_ring.alloc((size_t)PROBE_RING_STEPS * c.ncol(), false));
    c.serial = ++serial;
    ctx->census = std::move(c);
    return TDGL_OK;
}

extern "C" int tdgl_get_census(tdgl_ctx *ctx, int64_t capacity_rows, int32_t *rows, int64_t *n_rows) {
    if (!ctx) return TDGL_ERR_ARG;
    if (capacity_rows < 0 || (capacity_rows > 0 && !rows) || !n_rows) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_get_census: bad arguments");
    const Census &c = ctx->census;
    const int64_t have = c.on() ? (int64_t)(c.rows.size() / c.ncol()) : 0;
    *n_rows = have;
    const int64_t k = std::min(have, capacity_rows);
    if (k > 0) memcpy(rows, c.rows.data(), (size_t)k * c.ncol() * sizeof(int32_t));
    return TDGL_OK;
}
