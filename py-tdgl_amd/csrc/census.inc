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

// REC: the recording variant (tdgl_set_core_records).  In every trip, after the ballots, a wavefront with hits reserves
// popcount(hits) slots of the pool with ONE returning integer atomicAdd on the cursor (lane 0; the base goes to the wave
// by a shuffle), and a hit lane writes its record at base + its rank among the lower hit lanes: the triangle's number as
// the caller gave it, the charge, the position (vortex_rules.h).  A record whose slot is at or beyond the capacity is
// not written, and a wavefront whose plain load of the cursor already shows it there skips the atomic: the host takes
// the counts from the census row, never from the cursor (core_records.h).  `rec` (uniform in the launch): this step
// records.  Nothing here is a barrier, and every lane reaches every ballot and the shuffle.
template <bool REC>
__device__ inline void census_body(const CensusPlan &c, int blk, const double2 *__restrict__ psi, int32_t *__restrict__ row,
                                   const CoresPlan &r, bool rec) {
    __shared__ int wave_plus[BLOCK / WAVE], wave_minus[BLOCK / WAVE];
    const int lane = threadIdx.x & (WAVE - 1);
    if (blk < c.nblk_tri) {  // (uniform in the workgroup, like the loop below: every lane reaches the ballots and the barrier)
        int plus = 0, minus = 0;
        for (int64_t base = (int64_t)blk * BLOCK; base < c.n_tri; base += (int64_t)c.nblk_tri * BLOCK) {
            const int64_t t = base + threadIdx.x;
            int w = 0;
            int32_t i0 = 0, i1 = 0, i2 = 0;
            double2 a = {0.0, 0.0}, b = a, d = a;
            if (t < c.n_tri) {
                i0 = c.elements[t], i1 = c.elements[(int64_t)c.n_tri + t], i2 = c.elements[2 * (int64_t)c.n_tri + t];
                a = psi[i0], b = psi[i1], d = psi[i2];
                w = vortex_triangle_winding(a, b, d) * (int)c.orient[t];
            }
            const unsigned long long hit_plus = __ballot(w > 0), hit_minus = __ballot(w < 0);  // every lane of the wave takes part
            plus += __popcll(hit_plus);
            minus += __popcll(hit_minus);
            if constexpr (REC) {
                const unsigned long long hits = hit_plus | hit_minus;
                if (rec && hits != 0ull) {  // (uniform in the wave)
                    unsigned long long first = r.capacity;
                    if (lane == 0 && __hip_atomic_load(r.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < r.capacity)
                        first = atomicAdd(r.cursor, (unsigned long long)__popcll(hits));
                    first = __shfl(first, 0, WAVE);
                    const unsigned long long pos = first + (unsigned long long)__popcll(hits & ((1ull << lane) - 1ull));
                    if (w != 0 && pos < r.capacity) {
                        const double2 z = vortex_core_position(a, b, d, r.xy[i0], r.xy[i1], r.xy[i2]);
                        tdgl_cores::Record out;
                        out.triangle = r.tri_id[t], out.charge = w, out.x = z.x, out.y = z.y;
                        r.pool[pos] = out;
                    }
                }
            }
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
    census_body<false>(c, blockIdx.x, psi, row, CoresPlan{}, false);
}

// ... of a step that records its cores
__global__ __launch_bounds__(BLOCK) void k_census_cores(CensusPlan c, const double2 *__restrict__ psi, int32_t *__restrict__ row,
                                                        CoresPlan r) {
    census_body<true>(c, blockIdx.x, psi, row, r, true);
}

// an ACCEPTED attempt's census into the slot of its step (the controller has flipped cur: psi^{n+1})
__global__ __launch_bounds__(BLOCK) void k_ra_census(CensusPlan c, const double2 *__restrict__ psi0,
                                                     const double2 *__restrict__ psi1, int32_t *__restrict__ ring,
                                                     int slot_base, const StepCtl *__restrict__ ctl) {
    if (!ctl->live || !ctl->last_ok) return;
    census_body<false>(c, blockIdx.x, ctl->cur != 0 ? psi1 : psi0, ring + (size_t)(slot_base + ctl->n_acc - 1) * c.ncol, CoresPlan{},
                       false);
}

// ... with the cores of the steps whose running index, first + n_acc - 1, is divisible by every (first: the index of
// the batch's first step)
__global__ __launch_bounds__(BLOCK) void k_ra_census_cores(CensusPlan c, const double2 *__restrict__ psi0,
                                                           const double2 *__restrict__ psi1, int32_t *__restrict__ ring,
                                                           int slot_base, const StepCtl *__restrict__ ctl, CoresPlan r,
                                                           int64_t first, int64_t every) {
    if (!ctl->live || !ctl->last_ok) return;
    census_body<true>(c, blockIdx.x, ctl->cur != 0 ? psi1 : psi0, ring + (size_t)(slot_base + ctl->n_acc - 1) * c.ncol, r,
                      (first + ctl->n_acc - 1) % every == 0);
}

// ... per replica blockIdx.y, into slot n_acc - 1 of the replica's RA_BATCH_MAX rows
__global__ __launch_bounds__(BLOCK) void k_ens_census(CensusPlan c, const double2 *__restrict__ psi0,
                                                      const double2 *__restrict__ psi1, int64_t n_pad,
                                                      int32_t *__restrict__ ring, const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    const StepCtl *s = ctl + r;
    if (!s->live || !s->last_ok) return;
    census_body<false>(c, blockIdx.x, (s->cur != 0 ? psi1 : psi0) + (int64_t)r * n_pad,
                       ring + ((int64_t)r * RA_BATCH_MAX + s->n_acc - 1) * c.ncol, CoresPlan{}, false);
}

}  // namespace tdgl

// the step just accepted (classic loop): psi = psi^{n+1}
static void census_launch(tdgl_ctx *ctx, const double2 *psi) {
    Census &c = ctx->census;
    int32_t *row = c.ring.p + (size_t)c.ring_count * c.ncol();
    if (c.cores.on() && c.cores.records_index(c.cores.window_first + c.ring_count))
        hipLaunchKernelGGL(k_census_cores, dim3(c.grid()), dim3(BLOCK), 0, ctx->stream, c.plan(), psi, row, c.cores.plan());
    else
        hipLaunchKernelGGL(k_census, dim3(c.grid()), dim3(BLOCK), 0, ctx->stream, c.plan(), psi, row);
    c.ring_count += 1;
}

// one attempt of a run-ahead batch whose first accepted step takes row c.ring_count
static void census_launch_ra(tdgl_ctx *ctx) {
    Census &c = ctx->census;
    if (c.cores.on())
        hipLaunchKernelGGL(k_ra_census_cores, dim3(c.grid()), dim3(BLOCK), 0, ctx->stream, c.plan(), (const double2 *)ctx->psi[0].p,
                           (const double2 *)ctx->psi[1].p, c.ring.p, c.ring_count, (const StepCtl *)ctx->d_ctl.p, c.cores.plan(),
                           c.cores.window_first + c.ring_count, c.cores.every);
    else
        hipLaunchKernelGGL(k_ra_census, dim3(c.grid()), dim3(BLOCK), 0, ctx->stream, c.plan(), (const double2 *)ctx->psi[0].p,
                           (const double2 *)ctx->psi[1].p, c.ring.p, c.ring_count, (const StepCtl *)ctx->d_ctl.p);
}

// tdgl_run begins: no rows, every counter of the ring zero, an empty pool
static int census_begin_run(tdgl_ctx *ctx) {
    Census &c = ctx->census;
    c.ring_count = 0;
    c.rows.clear();
    c.cores.step.clear(), c.cores.complete.clear(), c.cores.records.clear();
    c.cores.offset.assign(1, 0);
    if (c.on()) HIP_TRY(ctx, hipMemsetAsync(c.ring.p, 0, c.ring.n * sizeof(int32_t), ctx->stream));
    if (c.cores.on()) HIP_TRY(ctx, hipMemsetAsync(c.cores.cursor.p, 0, sizeof(unsigned long long), ctx->stream));
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
    // (the pool itself is read after the synchronisation, once the rows have said how much of it: nothing is queued
    // behind this flush until then, so the records stay where they are)
    if (c.cores.on()) HIP_TRY(ctx, hipMemsetAsync(c.cores.cursor.p, 0, sizeof(unsigned long long), ctx->stream));
    return TDGL_OK;
}

// The rows are on the host.  With records on: the counts of the window's recorded steps say how many records the pool
// holds; exactly those are fetched -- one more host synchronisation, only when there are any -- and put in order.
static int census_flush_keep(tdgl_ctx *ctx, int count) {
    Census &c = ctx->census;
    CoreRecords &k = c.cores;
    if (k.on() && count > 0) {
        const int ncol = c.ncol();
        std::vector<uint8_t> recorded((size_t)count);
        int64_t steps = 0, total = 0;
        for (int r = 0; r < count; ++r) {
            recorded[r] = k.records_index(k.window_first + r) ? 1 : 0;
            if (!recorded[r]) continue;
            ++steps;
            total += (int64_t)c.h_ring.p[(size_t)r * ncol] + (int64_t)c.h_ring.p[(size_t)r * ncol + 1];
        }
        k.window_first += count;
        const int64_t fetch = std::min(total, k.capacity);
        if (fetch > 0) {
            HIP_TRY(ctx, hipMemcpyAsync(k.h_pool.p, k.pool.p, (size_t)fetch * sizeof(tdgl_cores::Record), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            ctx->stat_host_syncs += 1;
        }
        const int64_t run_row = (int64_t)(c.rows.size() / ncol);  // the window's row 0 among the run's steps
        const size_t s0 = k.step.size(), r0 = k.records.size();
        std::vector<int64_t> offset((size_t)steps + 1);
        k.step.resize(s0 + (size_t)steps);
        k.complete.resize(s0 + (size_t)steps);
        k.records.resize(r0 + (size_t)fetch);
        tdgl_cores::assemble(count, ncol, c.h_ring.p, recorded.data(), k.h_pool.p, k.capacity, k.step.data() + s0, offset.data(),
                             k.complete.data() + s0, k.records.data() + r0);
        for (int64_t s = 0; s < steps; ++s) {
            k.step[s0 + s] += run_row;
            k.offset.push_back((int64_t)r0 + offset[s + 1]);
        }
        k.records.resize(r0 + (size_t)offset[steps]);
    }
    c.rows.insert(c.rows.end(), c.h_ring.p, c.h_ring.p + (size_t)count * c.ncol());
    return TDGL_OK;
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
    if (const char *env = getenv("TDGL_CENSUS_MAX_BLOCKS")) {  // (tests: more than one trip through the stride loop on a small mesh)
        const long asked = atol(env);
        if (asked >= 1 && asked <= CENSUS_MAX_BLOCKS) c.max_blocks = (int32_t)asked;
    }
    c.tri_order.assign(order.begin(), order.end());
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

// Records of the cores of every `every`-th accepted step, counted from this call on, at most `capacity` per flush window
// (include/tdgl_hip.h).  Built aside and moved in whole: a call that fails leaves the previous state in place.
extern "C" int tdgl_set_core_records(tdgl_ctx *ctx, const double *sites_xy, int64_t capacity, int64_t every) {
    CTX_GUARD(ctx);
    if (ctx->n_own != ctx->n || distributed(ctx))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_core_records: not available in one-process-per-GPU mode");
    if (capacity < 0) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_core_records: negative capacity (%lld)", (long long)capacity);
    Census &c = ctx->census;
    if (capacity == 0) {  // off
        c.cores = CoreRecords();
        return TDGL_OK;
    }
    if (!c.on() || c.n_tri == 0)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_core_records: needs a census with triangles on the context (tdgl_set_census first)");
    if (every < 1) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_core_records: every must be >= 1 (got %lld)", (long long)every);
    if (!sites_xy) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_core_records: null array");
    const int64_t n = ctx->n;
    std::vector<double2> xy((size_t)n);
    for (int64_t i = 0; i < n; ++i) xy[(size_t)ctx->iperm[i]] = make_double2(sites_xy[2 * i], sites_xy[2 * i + 1]);
    CoreRecords k;
    k.capacity = capacity;
    k.every = every;
    HIP_TRY(ctx, k.tri_id.upload(c.tri_order));
    HIP_TRY(ctx, k.xy.upload(xy));
    HIP_TRY(ctx, k.pool.alloc((size_t)capacity, false));
    HIP_TRY(ctx, k.cursor.alloc(1));
    HIP_TRY(ctx, k.h_pool.alloc((size_t)capacity, false));
    c.cores = std::move(k);
    return TDGL_OK;
}

extern "C" int tdgl_get_core_records(tdgl_ctx *ctx, int64_t capacity_steps, int64_t *step, int64_t *count, int32_t *complete,
                                     int64_t capacity_records, int32_t *triangles, int32_t *charges, double *xy,
                                     int64_t *n_steps, int64_t *n_records) {
    if (!ctx) return TDGL_ERR_ARG;
    if (capacity_steps < 0 || capacity_records < 0 || !n_steps || !n_records || (capacity_steps > 0 && (!step || !count || !complete)) ||
        (capacity_records > 0 && (!triangles || !charges || !xy)))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_get_core_records: bad arguments");
    const CoreRecords &k = ctx->census.cores;
    const int64_t have_steps = k.on() ? (int64_t)k.step.size() : 0, have = k.on() ? (int64_t)k.records.size() : 0;
    *n_steps = have_steps;
    *n_records = have;
    for (int64_t s = 0; s < std::min(have_steps, capacity_steps); ++s) {
        step[s] = k.step[s];
        count[s] = k.offset[s + 1] - k.offset[s];
        complete[s] = k.complete[s];
    }
    for (int64_t g = 0; g < std::min(have, capacity_records); ++g) {
        const tdgl_cores::Record &r = k.records[g];
        triangles[g] = r.triangle, charges[g] = r.charge, xy[2 * g] = r.x, xy[2 * g + 1] = r.y;
    }
    return TDGL_OK;
}

// core_records.h on the host alone, for tests: rows [n_rows][ncol], recorded [n_rows], the pool as three arrays of
// n_pool records (at least min(sum of the recorded counts, capacity)).  Outputs: row, complete [recorded steps], offset
// [recorded steps + 1], and the sorted records (room for min(sum, capacity)).
extern "C" int tdgl_host_core_records_assemble(int64_t n_rows, int32_t ncol, const int32_t *rows, const uint8_t *recorded,
                                               int64_t n_pool, const int32_t *pool_triangles, const int32_t *pool_charges,
                                               const double *pool_xy, int64_t capacity, int64_t *row, int64_t *offset,
                                               uint8_t *complete, int32_t *triangles, int32_t *charges, double *xy,
                                               int64_t *n_steps) {
    tdgl_ctx *const no_ctx = nullptr;
    if (n_rows < 0 || ncol < 2 || n_pool < 0 || capacity < 0 || !offset || !n_steps || (n_rows > 0 && (!rows || !recorded || !row || !complete)) ||
        (n_pool > 0 && (!pool_triangles || !pool_charges || !pool_xy || !triangles || !charges || !xy)))
        TDGL_FAIL(no_ctx, TDGL_ERR_ARG, "tdgl_host_core_records_assemble: bad arguments");
    int64_t total = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        if (rows[r * ncol] < 0 || rows[r * ncol + 1] < 0)
            TDGL_FAIL(no_ctx, TDGL_ERR_ARG, "tdgl_host_core_records_assemble: negative count in row %lld", (long long)r);
        if (recorded[r]) total += (int64_t)rows[r * ncol] + (int64_t)rows[r * ncol + 1];
    }
    if (n_pool < std::min(total, capacity))
        TDGL_FAIL(no_ctx, TDGL_ERR_ARG, "tdgl_host_core_records_assemble: the pool holds %lld records, the rows need %lld",
                  (long long)n_pool, (long long)std::min(total, capacity));
    std::vector<tdgl_cores::Record> pool((size_t)n_pool), out((size_t)n_pool);
    for (int64_t g = 0; g < n_pool; ++g) pool[g] = {pool_triangles[g], pool_charges[g], pool_xy[2 * g], pool_xy[2 * g + 1]};
    *n_steps = tdgl_cores::assemble(n_rows, ncol, rows, recorded, pool.data(), capacity, row, offset, complete, out.data());
    for (int64_t g = 0; g < offset[*n_steps]; ++g)
        triangles[g] = out[g].triangle, charges[g] = out[g].charge, xy[2 * g] = out[g].x, xy[2 * g + 1] = out[g].y;
    return TDGL_OK;
}
