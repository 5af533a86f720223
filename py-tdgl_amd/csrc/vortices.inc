// Vortex cores and loop windings of saved order parameters, away from the time loop: the winding of arg psi around
// every mesh triangle (with the position of the zero of the linear interpolant where it is +-1) and around closed
// loops of sites (the film's and the holes' boundaries).  Included by tdgl_hip.hip after fields.inc.  The definitions
// are DESIGN.md section 3, "Vortex cores and windings"; tests/vortex_model.py restates them in NumPy.
//
// Every sign decision compares two separately rounded products p = u.re v.im and q = u.im v.re and never takes the
// sign of a difference, so a contraction of p - q into an FMA cannot change a decision: charges, triangle numbers,
// their order and the windings equal the NumPy model's bit for bit.  Only the core positions use p - q; they are
// compared within a derived bound.
//
// Three passes over a chunk of frames, one lane per (frame, triangle):
//   k_vortex_charge   charge of every triangle -> int8 [frame][triangle], hits per workgroup (wave ballots)
//   k_vortex_scan     one workgroup per frame: exclusive scan of that frame's workgroup counts, the frame's total
//   k_vortex_write    records at  base[frame] + offset[workgroup] + rank in the workgroup, i.e. in (frame, triangle)
//                     order whatever the scheduling (no atomics); records beyond the capacity are dropped
// and one wavefront per (frame, loop) for the windings (k_vortex_windings).

namespace tdgl {

constexpr int VORTEX_WAVES = BLOCK / WAVE;

__device__ inline int vortex_sign(double p, double q) { return (p > q) - (p < q); }

// +1 / -1 when psi winds once around the triangle (a, b, c) in the order given, 0 otherwise (also for a vertex that
// is zero or NaN: every comparison is then false)
__device__ inline int vortex_triangle_winding(double2 a, double2 b, double2 c) {
    const int sab = vortex_sign(a.x * b.y, a.y * b.x);
    const int sbc = vortex_sign(b.x * c.y, b.y * c.x);
    const int sca = vortex_sign(c.x * a.y, c.y * a.x);
    if (sab > 0 && sbc > 0 && sca > 0) return 1;
    if (sab < 0 && sbc < 0 && sca < 0) return -1;
    return 0;
}

// psi: [frames][n_sites] (re, im); charge: [frames][n_tri]; block_count: [frames][gridDim.x]
__global__ __launch_bounds__(BLOCK) void k_vortex_charge(int64_t n_tri, int64_t n_sites,
                                                         const int32_t *__restrict__ elements,
                                                         const int8_t *__restrict__ orient,
                                                         const double2 *__restrict__ psi, int8_t *__restrict__ charge,
                                                         int32_t *__restrict__ block_count) {
    __shared__ int wave_count[VORTEX_WAVES];
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t f = blockIdx.y;
    int w = 0;
    if (t < n_tri) {
        const double2 *__restrict__ z = psi + f * n_sites;
        const double2 a = z[elements[3 * t]], b = z[elements[3 * t + 1]], c = z[elements[3 * t + 2]];
        w = vortex_triangle_winding(a, b, c) * (int)orient[t];
        charge[f * n_tri + t] = (int8_t)w;
    }
    const unsigned long long hits = __ballot(w != 0);  // every lane of the wave takes part
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_count[threadIdx.x / WAVE] = __popcll(hits);
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int k = 0; k < VORTEX_WAVES; ++k) total += wave_count[k];
        block_count[f * gridDim.x + blockIdx.x] = total;
    }
}

// One workgroup per frame of the chunk: block_count[f][0 .. nb) -> its exclusive scan in place, frame_count[f] = sum.
// Thread k owns the contiguous run [k per, (k + 1) per).
__global__ __launch_bounds__(BLOCK) void k_vortex_scan(int64_t nb, int32_t *__restrict__ block_count,
                                                       int64_t *__restrict__ frame_count) {
    __shared__ int64_t run_sum[BLOCK];
    int32_t *__restrict__ cnt = block_count + (int64_t)blockIdx.x * nb;
    const int64_t per = (nb + BLOCK - 1) / BLOCK;
    const int64_t lo = min(nb, (int64_t)threadIdx.x * per), hi = min(nb, lo + per);
    int64_t sum = 0;
    for (int64_t k = lo; k < hi; ++k) sum += cnt[k];
    run_sum[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int k = 0; k < BLOCK; ++k) {
            const int64_t s = run_sum[k];
            run_sum[k] = acc;
            acc += s;
        }
        frame_count[blockIdx.x] = acc;
    }
    __syncthreads();
    int64_t acc = run_sum[threadIdx.x];  // (a frame has fewer than 2^31 triangles: the offsets fit int32)
    for (int64_t k = lo; k < hi; ++k) {
        const int32_t c = cnt[k];
        cnt[k] = (int32_t)acc;
        acc += c;
    }
}

// frame_base[g0 + k + 1] = frame_base[g0 + k] + frame_count[g0 + k] for the chunk's frames (frame_base[0] = 0 is set
// by the host): where each frame's records start among all records of the call
__global__ void k_vortex_frame_bases(int frames, const int64_t *__restrict__ frame_count, int64_t *__restrict__ frame_base) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t acc = frame_base[0];
    for (int k = 0; k < frames; ++k) {
        acc += frame_count[k];
        frame_base[k + 1] = acc;
    }
}

// block_offset: the scanned block_count; frame_base: [frames] of this chunk.  tri_charge: [capacity][2] = (triangle,
// charge); xy: [capacity][2] the zero of the linear interpolant of psi on the triangle
__global__ __launch_bounds__(BLOCK) void k_vortex_write(int64_t n_tri, int64_t n_sites, int64_t capacity,
                                                        const int32_t *__restrict__ elements,
                                                        const double2 *__restrict__ sites,
                                                        const double2 *__restrict__ psi,
                                                        const int8_t *__restrict__ charge,
                                                        const int32_t *__restrict__ block_offset,
                                                        const int64_t *__restrict__ frame_base,
                                                        int32_t *__restrict__ tri_charge, double *__restrict__ xy) {
    __shared__ int wave_count[VORTEX_WAVES];
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t f = blockIdx.y;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int w = (t < n_tri) ? (int)charge[f * n_tri + t] : 0;
    const unsigned long long hits = __ballot(w != 0);
    if (lane == 0) wave_count[wave] = __popcll(hits);
    __syncthreads();
    if (w == 0) return;  // (no barrier and no cross-lane operation below)
    int64_t pos = frame_base[f] + block_offset[f * gridDim.x + blockIdx.x] + __popcll(hits & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; ++k) pos += wave_count[k];
    if (pos >= capacity) return;
    tri_charge[2 * pos] = (int32_t)t;
    tri_charge[2 * pos + 1] = w;
    const int32_t i0 = elements[3 * t], i1 = elements[3 * t + 1], i2 = elements[3 * t + 2];
    const double2 *__restrict__ z = psi + f * n_sites;
    const double2 a = z[i0], b = z[i1], c = z[i2];
    const double ca = b.x * c.y - b.y * c.x, cb = c.x * a.y - c.y * a.x, cc = a.x * b.y - a.y * b.x;
    const double S = (ca + cb) + cc;
    const double la = ca / S, lb = cb / S, lc = cc / S;
    const double2 ra = sites[i0], rb = sites[i1], rc = sites[i2];
    xy[2 * pos] = (la * ra.x + lb * rb.x) + lc * rc.x;
    xy[2 * pos + 1] = (la * ra.y + lb * rb.y) + lc * rc.y;
}

// One wavefront per (frame, loop): Sunday's crossing rule around the origin over the loop's edges u -> v, lanes
// striding over the edges.  windings: [frames][n_loops]; TDGL_WINDING_UNDEFINED when a vertex is zero or not finite or
// an edge is a segment through the origin.
__global__ __launch_bounds__(BLOCK) void k_vortex_windings(int frames, int n_loops, int64_t n_sites,
                                                           const int64_t *__restrict__ loop_ptr,
                                                           const int32_t *__restrict__ loop_sites,
                                                           const double2 *__restrict__ psi, int32_t *__restrict__ windings) {
    const int64_t item = (int64_t)blockIdx.x * VORTEX_WAVES + threadIdx.x / WAVE;  // uniform in the wave
    if (item >= (int64_t)frames * n_loops) return;
    const int64_t f = item / n_loops;
    const int l = (int)(item % n_loops);
    const int lane = threadIdx.x & (WAVE - 1);
    const double2 *__restrict__ z = psi + f * n_sites;
    const int64_t e0 = loop_ptr[l], e1 = loop_ptr[l + 1];
    int w = 0, undefined = 0;
    for (int64_t e = e0 + lane; e < e1; e += WAVE) {
        const double2 u = z[loop_sites[e]];
        const double2 v = z[loop_sites[e + 1 < e1 ? e + 1 : e0]];
        if ((u.x == 0.0 && u.y == 0.0) || !isfinite(u.x) || !isfinite(u.y)) undefined = 1;
        const double p = u.x * v.y, q = u.y * v.x;
        const double rr = u.x * v.x, ii = u.y * v.y;
        if (p == q && (rr < 0.0 || ii < 0.0)) undefined = 1;
        if (u.y <= 0.0 && v.y > 0.0 && p > q) ++w;
        if (u.y > 0.0 && v.y <= 0.0 && p < q) --w;
    }
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        w += __shfl_xor(w, d, WAVE);
        undefined |= __shfl_xor(undefined, d, WAVE);
    }
    if (lane == 0) windings[f * n_loops + l] = undefined ? TDGL_WINDING_UNDEFINED : w;
}

}  // namespace tdgl

// ---------------------------------------------------------------------------------------
// psi goes up in chunks of frames: at most VORTEX_MAX_CHUNK frames and at most VORTEX_STAGE_BYTES of staging (one
// frame when a single frame is larger).  TDGL_VORTEX_CHUNK=<frames> (tests) fixes the chunk, read at plan creation.
static constexpr int64_t VORTEX_MAX_CHUNK = 32;
static constexpr int64_t VORTEX_STAGE_BYTES = (int64_t)256 << 20;

struct tdgl_vortex_plan {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int64_t n_sites = 0, n_tri = 0, n_loop_sites = 0;
    int32_t n_loops = 0;
    int64_t chunk = 1;  // frames per chunk
    int64_t nb = 0;     // workgroups per frame of the triangle kernels
    DevBuf<double> sites, psi, xy;
    DevBuf<int32_t> elements, loop_sites, block_count, tri_charge, windings;
    DevBuf<int8_t> orient, charge;
    DevBuf<int64_t> loop_ptr, frame_count, frame_base;
    int64_t stats[4] = {0, 0, 0, 0};  // records found, frames, chunks, kernel launches of the last call
    double last_ms = 0.0;
};

static tdgl_ctx *const VORTEX_NO_CTX = nullptr;  // errors go to the global tdgl_last_error(NULL)

extern "C" void tdgl_vortex_plan_destroy(tdgl_vortex_plan *plan) {
    if (!plan) return;
    (void)hipSetDevice(plan->device);
    if (plan->stream) (void)hipStreamSynchronize(plan->stream);
    if (plan->ev0) (void)hipEventDestroy(plan->ev0);
    if (plan->ev1) (void)hipEventDestroy(plan->ev1);
    if (plan->stream) (void)hipStreamDestroy(plan->stream);
    delete plan;
}

// the sign of twice the signed area of (r0, r1, r2), decided like every other sign here: two rounded products compared
static int8_t vortex_orientation(const double *r0, const double *r1, const double *r2) {
    const double p = (r1[0] - r0[0]) * (r2[1] - r0[1]);
    const double q = (r2[0] - r0[0]) * (r1[1] - r0[1]);
    return (int8_t)((p > q) - (p < q));
}

extern "C" int tdgl_vortex_plan_create(tdgl_vortex_plan **out, int device_id, int64_t n_sites, const double *sites_xy,
                                       int64_t n_tri, const int32_t *elements, int32_t n_loops, const int64_t *loop_ptr,
                                       const int32_t *loop_sites) {
    if (!out) TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_create: null output pointer");
    *out = nullptr;
    if (n_sites < 0 || n_tri < 0 || n_loops < 0)
        TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_create: negative size (n_sites %lld, n_tri %lld, n_loops %d)",
                  (long long)n_sites, (long long)n_tri, (int)n_loops);
    if (n_sites < 1 || n_sites > INT32_MAX || n_tri > INT32_MAX)
        TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_create: n_sites must be in 1 .. 2^31 - 1 and n_tri below 2^31 "
                  "(got %lld, %lld)", (long long)n_sites, (long long)n_tri);
    if (!sites_xy || (n_tri > 0 && !elements) || (n_loops > 0 && (!loop_ptr || !loop_sites)))
        TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_create: null array");
    for (int64_t k = 0; k < 3 * n_tri; ++k)
        if (elements[k] < 0 || elements[k] >= n_sites)
            TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_create: element %lld names site %d, out of range for %lld sites",
                      (long long)(k / 3), (int)elements[k], (long long)n_sites);
    if (n_loops > 0 && loop_ptr[0] != 0)
        TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_create: loop_ptr[0] must be 0 (got %lld)", (long long)loop_ptr[0]);
    for (int32_t l = 0; l < n_loops; ++l)
        if (loop_ptr[l + 1] - loop_ptr[l] < 3)
            TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_create: loop %d has %lld sites, a loop needs at least 3",
                      (int)l, (long long)(loop_ptr[l + 1] - loop_ptr[l]));
    const int64_t n_loop_sites = n_loops > 0 ? loop_ptr[n_loops] : 0;
    for (int64_t k = 0; k < n_loop_sites; ++k)
        if (loop_sites[k] < 0 || loop_sites[k] >= n_sites)
            TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_create: loop site %d out of range for %lld sites",
                      (int)loop_sites[k], (long long)n_sites);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count)
        TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_create: no HIP device %d (%d visible)", device_id, count);
    HIP_TRY(VORTEX_NO_CTX, hipSetDevice(device_id));
    std::unique_ptr<tdgl_vortex_plan, void (*)(tdgl_vortex_plan *)> plan(new tdgl_vortex_plan, tdgl_vortex_plan_destroy);
    plan->device = device_id;
    plan->n_sites = n_sites;
    plan->n_tri = n_tri;
    plan->n_loops = n_loops;
    plan->n_loop_sites = n_loop_sites;
    plan->nb = (n_tri + BLOCK - 1) / BLOCK;
    plan->chunk = std::max<int64_t>(1, std::min(VORTEX_MAX_CHUNK, VORTEX_STAGE_BYTES / (16 * n_sites)));
    if (const char *env = getenv("TDGL_VORTEX_CHUNK")) {
        const long asked = atol(env);
        if (asked >= 1 && asked <= VORTEX_MAX_CHUNK) plan->chunk = asked;
    }
    HIP_TRY(VORTEX_NO_CTX, hipStreamCreate(&plan->stream));
    HIP_TRY(VORTEX_NO_CTX, hipEventCreate(&plan->ev0));
    HIP_TRY(VORTEX_NO_CTX, hipEventCreate(&plan->ev1));
    std::vector<int8_t> orient((size_t)n_tri);
    for (int64_t t = 0; t < n_tri; ++t)
        orient[t] = vortex_orientation(sites_xy + 2 * (int64_t)elements[3 * t], sites_xy + 2 * (int64_t)elements[3 * t + 1],
                                       sites_xy + 2 * (int64_t)elements[3 * t + 2]);
    HIP_TRY(VORTEX_NO_CTX, plan->sites.upload(std::vector<double>(sites_xy, sites_xy + 2 * n_sites)));
    HIP_TRY(VORTEX_NO_CTX, plan->elements.upload(std::vector<int32_t>(elements, elements + 3 * n_tri)));
    HIP_TRY(VORTEX_NO_CTX, plan->orient.upload(orient));
    if (n_loops > 0) {
        HIP_TRY(VORTEX_NO_CTX, plan->loop_ptr.upload(std::vector<int64_t>(loop_ptr, loop_ptr + n_loops + 1)));
        HIP_TRY(VORTEX_NO_CTX, plan->loop_sites.upload(std::vector<int32_t>(loop_sites, loop_sites + n_loop_sites)));
    }
    *out = plan.release();
    return TDGL_OK;
}

extern "C" int tdgl_vortex_plan_find(tdgl_vortex_plan *plan, int32_t n_frames, const double *psi, int64_t capacity,
                                     int64_t *counts, int32_t *tri_charge, double *xy, int32_t *windings) {
    if (!plan) TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_find: null plan");
    if (!psi) TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_find: null psi");
    if (n_frames < 1) TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_find: n_frames must be >= 1 (got %d)", (int)n_frames);
    if (capacity < 0) TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_find: negative capacity (%lld)", (long long)capacity);
    const int64_t n = plan->n_sites, n_tri = plan->n_tri, nb = plan->nb, F = n_frames;
    const bool want_records = (tri_charge || xy) && capacity > 0 && n_tri > 0;
    const bool want_triangles = (counts || want_records) && n_tri > 0;
    const bool want_windings = windings && plan->n_loops > 0;
    // the device never holds more records than can exist
    const int64_t cap = want_records ? std::min(capacity, F * n_tri) : 0;
    HIP_TRY(VORTEX_NO_CTX, hipSetDevice(plan->device));
    const int64_t chunk = std::min(plan->chunk, F);
    if (plan->psi.n < (size_t)(2 * chunk * n)) HIP_TRY(VORTEX_NO_CTX, plan->psi.alloc((size_t)(2 * chunk * n), false));
    if (want_triangles) {
        if (plan->charge.n < (size_t)(chunk * n_tri)) HIP_TRY(VORTEX_NO_CTX, plan->charge.alloc((size_t)(chunk * n_tri), false));
        if (plan->block_count.n < (size_t)(chunk * nb)) HIP_TRY(VORTEX_NO_CTX, plan->block_count.alloc((size_t)(chunk * nb), false));
        if (plan->frame_count.n < (size_t)F) HIP_TRY(VORTEX_NO_CTX, plan->frame_count.alloc((size_t)F, false));
        if (plan->frame_base.n < (size_t)(F + 1)) HIP_TRY(VORTEX_NO_CTX, plan->frame_base.alloc((size_t)(F + 1), false));
        HIP_TRY(VORTEX_NO_CTX, hipMemsetAsync(plan->frame_base.p, 0, sizeof(int64_t), plan->stream));
    }
    if (want_records) {
        if (plan->tri_charge.n < (size_t)(2 * cap)) HIP_TRY(VORTEX_NO_CTX, plan->tri_charge.alloc((size_t)(2 * cap), false));
        if (plan->xy.n < (size_t)(2 * cap)) HIP_TRY(VORTEX_NO_CTX, plan->xy.alloc((size_t)(2 * cap), false));
    }
    if (want_windings && plan->windings.n < (size_t)(F * plan->n_loops))
        HIP_TRY(VORTEX_NO_CTX, plan->windings.alloc((size_t)(F * plan->n_loops), false));
    const double2 *d_psi = reinterpret_cast<const double2 *>(plan->psi.p);
    const double2 *d_sites = reinterpret_cast<const double2 *>(plan->sites.p);
    int64_t launches = 0, chunks = 0;
    double total_ms = 0.0;
    for (int64_t g0 = 0; g0 < F; g0 += chunk, ++chunks) {
        const int fc = (int)std::min(chunk, F - g0);
        HIP_TRY(VORTEX_NO_CTX, hipMemcpyAsync(plan->psi.p, psi + 2 * g0 * n, (size_t)fc * 2 * n * sizeof(double),
                                             hipMemcpyHostToDevice, plan->stream));
        HIP_TRY(VORTEX_NO_CTX, hipEventRecord(plan->ev0, plan->stream));
        if (want_triangles) {
            hipLaunchKernelGGL(k_vortex_charge, dim3((unsigned)nb, fc), dim3(BLOCK), 0, plan->stream, n_tri, n,
                               plan->elements.p, plan->orient.p, d_psi, plan->charge.p, plan->block_count.p);
            hipLaunchKernelGGL(k_vortex_scan, dim3(fc), dim3(BLOCK), 0, plan->stream, nb, plan->block_count.p,
                               plan->frame_count.p + g0);
            hipLaunchKernelGGL(k_vortex_frame_bases, dim3(1), dim3(WAVE), 0, plan->stream, fc, plan->frame_count.p + g0,
                               plan->frame_base.p + g0);
            launches += 3;
            if (want_records) {
                hipLaunchKernelGGL(k_vortex_write, dim3((unsigned)nb, fc), dim3(BLOCK), 0, plan->stream, n_tri, n, cap,
                                   plan->elements.p, d_sites, d_psi, plan->charge.p, plan->block_count.p,
                                   plan->frame_base.p + g0, plan->tri_charge.p, plan->xy.p);
                ++launches;
            }
        }
        if (want_windings) {
            const int64_t items = (int64_t)fc * plan->n_loops;
            hipLaunchKernelGGL(k_vortex_windings, dim3((unsigned)((items + VORTEX_WAVES - 1) / VORTEX_WAVES)), dim3(BLOCK), 0,
                               plan->stream, fc, (int)plan->n_loops, n, plan->loop_ptr.p, plan->loop_sites.p, d_psi,
                               plan->windings.p + g0 * plan->n_loops);
            ++launches;
        }
        HIP_TRY(VORTEX_NO_CTX, hipEventRecord(plan->ev1, plan->stream));
        // the staging buffer is reused by the next chunk: wait, and add this chunk's device time
        HIP_TRY(VORTEX_NO_CTX, hipStreamSynchronize(plan->stream));
        HIP_TRY(VORTEX_NO_CTX, hipGetLastError());
        float ms = 0.f;
        HIP_TRY(VORTEX_NO_CTX, hipEventElapsedTime(&ms, plan->ev0, plan->ev1));
        total_ms += ms;
    }
    int64_t found = 0;
    if (want_triangles) {
        std::vector<int64_t> host_counts((size_t)F);
        HIP_TRY(VORTEX_NO_CTX, hipMemcpy(host_counts.data(), plan->frame_count.p, (size_t)F * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (int64_t f = 0; f < F; ++f) found += host_counts[f];
        if (counts) memcpy(counts, host_counts.data(), (size_t)F * sizeof(int64_t));
        const int64_t written = std::min(found, cap);
        if (want_records && tri_charge && written > 0)
            HIP_TRY(VORTEX_NO_CTX, hipMemcpy(tri_charge, plan->tri_charge.p, (size_t)(2 * written) * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (want_records && xy && written > 0)
            HIP_TRY(VORTEX_NO_CTX, hipMemcpy(xy, plan->xy.p, (size_t)(2 * written) * sizeof(double), hipMemcpyDeviceToHost));
    } else if (counts) {
        memset(counts, 0, (size_t)F * sizeof(int64_t));  // a plan without triangles
    }
    if (want_windings)
        HIP_TRY(VORTEX_NO_CTX, hipMemcpy(windings, plan->windings.p, (size_t)(F * plan->n_loops) * sizeof(int32_t), hipMemcpyDeviceToHost));
    plan->last_ms = total_ms;
    plan->stats[0] = found;
    plan->stats[1] = F;
    plan->stats[2] = chunks;
    plan->stats[3] = launches;
    return TDGL_OK;
}

extern "C" int tdgl_vortex_plan_stats(tdgl_vortex_plan *plan, int64_t *out4, double *last_ms) {
    if (!plan) TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_stats: null plan");
    if (out4) memcpy(out4, plan->stats, sizeof(plan->stats));
    if (last_ms) *last_ms = plan->last_ms;
    return TDGL_OK;
}
