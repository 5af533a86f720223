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
//
// tdgl_vortex_plan_link links the cores of consecutive frames into tracks: k_vortex_nearest, k_vortex_mutual and
// k_vortex_event_keys, further down.

#include "vortex_rules.h"  // vortex_triangle_winding, vortex_loop_winding, vortex_core_position: shared with census.inc

namespace tdgl {

constexpr int VORTEX_WAVES = BLOCK / WAVE;

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
    const double2 r = vortex_core_position(a, b, c, sites[i0], sites[i1], sites[i2]);
    xy[2 * pos] = r.x;
    xy[2 * pos + 1] = r.y;
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
    const int w = vortex_loop_winding(z, loop_sites, loop_ptr[l], loop_ptr[l + 1], lane);
    if (lane == 0) windings[f * n_loops + l] = w;
}

// ---------------------------------------------------------------------------------------
// Tracks: cores of consecutive frames linked by mutual keyed nearest neighbour, loose ends paired with the nearest
// loose end of the opposite charge, every core given its nearest loop site (DESIGN.md section 3, "Tracks";
// tdgl_amd.vortices.link_frames and tests/track_model.py restate the rule).  All three are k_vortex_nearest with another
// target segment and other keys, followed by k_vortex_mutual.  Every decision compares identically rounded doubles
// (fp contraction is off), so the indices equal the NumPy model's exactly.

// a source and a target segment of the concatenated records: sources [src0, src1), targets [tgt0, tgt1)
struct VortexJob {
    int64_t src0, src1, tgt0, tgt1;
};

__device__ inline double vortex_d2(double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
    const double dx = bx - ax, dy = by - ay;
    return (dx * dx) + (dy * dy);
}

// One lane per source of job blockIdx.y; the job's targets go through LDS in tiles of BLOCK (x, y, key), every lane
// reading the same address per step (a broadcast).  A source takes the lowest target index among those whose key
// equals its own, with d2 <= r2 and d2 minimal: a scan in index order with a strict <, from best = +inf, so a d2
// that is NaN or +inf is never taken.  out_idx: the index within the target segment or -1; out_d2 (may be NULL): that
// d2 or +inf.  A NULL key array stands for all keys 0.  Workgroups beyond the job's sources leave as a whole; in the
// others every lane reaches every barrier and lanes past the end only skip the store.
__global__ __launch_bounds__(BLOCK) void k_vortex_nearest(const VortexJob *__restrict__ jobs,
                                                          const double2 *__restrict__ src_xy,
                                                          const int32_t *__restrict__ src_key,
                                                          const double2 *__restrict__ tgt_xy,
                                                          const int32_t *__restrict__ tgt_key, double r2,
                                                          int32_t *__restrict__ out_idx, double *__restrict__ out_d2) {
#pragma clang fp contract(off)
    __shared__ double tile_x[BLOCK], tile_y[BLOCK];
    __shared__ int32_t tile_key[BLOCK];
    const VortexJob job = jobs[blockIdx.y];
    const int64_t first = job.src0 + (int64_t)blockIdx.x * BLOCK;
    if (first >= job.src1) return;  // (uniform in the workgroup)
    const int64_t s = first + threadIdx.x;
    const bool live = s < job.src1;
    double ax = 0.0, ay = 0.0;
    int32_t want = 0;
    if (live) {
        const double2 a = src_xy[s];
        ax = a.x;
        ay = a.y;
        if (src_key) want = src_key[s];
    }
    double best = INFINITY;
    int32_t arg = -1;
    for (int64_t t0 = job.tgt0; t0 < job.tgt1; t0 += BLOCK) {
        const int64_t t = t0 + threadIdx.x;
        if (t < job.tgt1) {
            const double2 b = tgt_xy[t];
            tile_x[threadIdx.x] = b.x;
            tile_y[threadIdx.x] = b.y;
            tile_key[threadIdx.x] = tgt_key ? tgt_key[t] : 0;
        }
        __syncthreads();
        const int m = (int)min((int64_t)BLOCK, job.tgt1 - t0);
        const int32_t base = (int32_t)(t0 - job.tgt0);
        for (int k = 0; k < m; ++k) {
            const double d2 = vortex_d2(ax, ay, tile_x[k], tile_y[k]);
            if (tile_key[k] == want && d2 <= r2 && d2 < best) {
                best = d2;
                arg = base + k;
            }
        }
        __syncthreads();  // the tile is overwritten next
    }
    if (live) {
        out_idx[s] = arg;
        if (out_d2) out_d2[s] = best;
    }
}

// out[g] = mine[g] when the core it names (number mine[g] of frame frame[g] + shift) names g back in `theirs`, else -1.
// offset: [frames + 1], where each frame's cores start.  mine[g] is -1 wherever frame[g] + shift is no frame.
__global__ __launch_bounds__(BLOCK) void k_vortex_mutual(int64_t n, int shift, const int32_t *__restrict__ frame,
                                                         const int32_t *__restrict__ offset,
                                                         const int32_t *__restrict__ mine,
                                                         const int32_t *__restrict__ theirs, int32_t *__restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n) return;
    const int32_t f = frame[g], c = mine[g];
    int32_t r = -1;
    if (c >= 0 && theirs[(int64_t)offset[f + shift] + c] == (int32_t)(g - offset[f])) r = c;
    out[g] = r;
}

// The keys of the pair search among loose ends: a core with link[g] == -1 outside frame `skip` looks for the opposite
// charge (src_key = -charge) and offers its own (tgt_key = charge); every other core looks for 2, which nobody offers,
// and offers 0, which nobody looks for.
__global__ __launch_bounds__(BLOCK) void k_vortex_event_keys(int64_t n, int32_t skip, const int32_t *__restrict__ frame,
                                                             const int32_t *__restrict__ charge,
                                                             const int32_t *__restrict__ link,
                                                             int32_t *__restrict__ src_key, int32_t *__restrict__ tgt_key) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n) return;
    const bool loose = link[g] < 0 && frame[g] != skip;
    src_key[g] = loose ? -charge[g] : 2;
    tgt_key[g] = loose ? charge[g] : 0;
}

}  // namespace tdgl

// ---------------------------------------------------------------------------------------
// psi goes up in chunks of frames: at most VORTEX_MAX_CHUNK frames and at most VORTEX_STAGE_BYTES of staging (one
// frame when a single frame is larger).  TDGL_VORTEX_CHUNK=<frames> (tests) fixes the chunk, read at plan creation.
static constexpr int64_t VORTEX_MAX_CHUNK = 32;
static constexpr int64_t VORTEX_STAGE_BYTES = (int64_t)256 << 20;
// tdgl_vortex_plan_link launches k_vortex_nearest with one job per blockIdx.y: at most this many per launch (the
// grid's y limit is 65,535).  TDGL_VORTEX_LINK_JOBS=<jobs> (tests) lowers it, read at plan creation.
static constexpr int64_t VORTEX_LINK_MAX_JOBS = 32768;

struct tdgl_vortex_plan : tdgl::TimedStream {  // (stream, ev0, ev1)
    int device = 0;
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
    // tdgl_vortex_plan_link: the loops' coordinates in the order of loop_sites, the call's records and its results
    int64_t link_max_jobs = VORTEX_LINK_MAX_JOBS;  // jobs (blockIdx.y) per launch of k_vortex_nearest
    DevBuf<double> loop_xy, l_xy, l_near_d2;
    DevBuf<int32_t> l_charge, l_frame, l_offset, l_fwd, l_bwd, l_next, l_prev, l_src_key, l_tgt_key, l_choice, l_end,
        l_start, l_near;
    DevBuf<tdgl::VortexJob> l_jobs;
    int64_t link_stats[4] = {0, 0, 0, 0};  // links, frames, pairs evaluated, kernel launches of the last link
    double link_ms = 0.0;
};

static tdgl_ctx *const VORTEX_NO_CTX = nullptr;  // errors go to the global tdgl_last_error(NULL)

extern "C" void tdgl_vortex_plan_destroy(tdgl_vortex_plan *plan) {
    if (!plan) return;
    (void)hipSetDevice(plan->device);
    if (plan->stream) (void)hipStreamSynchronize(plan->stream);
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
    if (const char *env = getenv("TDGL_VORTEX_LINK_JOBS")) {
        const long asked = atol(env);
        if (asked >= 1 && asked <= VORTEX_LINK_MAX_JOBS) plan->link_max_jobs = asked;
    }
    HIP_TRY(VORTEX_NO_CTX, plan->create());
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
        std::vector<double> loop_xy((size_t)(2 * n_loop_sites));
        for (int64_t q = 0; q < n_loop_sites; ++q) {
            loop_xy[2 * q] = sites_xy[2 * (int64_t)loop_sites[q]];
            loop_xy[2 * q + 1] = sites_xy[2 * (int64_t)loop_sites[q] + 1];
        }
        HIP_TRY(VORTEX_NO_CTX, plan->loop_xy.upload(loop_xy));
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

// ---------------------------------------------------------------------------------------
// k_vortex_nearest over jobs[j0 .. j0 + count) of the device's job list, at most plan->link_max_jobs per launch; the
// grid's x covers the longest source segment of each launch (the host's copy of the jobs says which)
static void vortex_launch_nearest(tdgl_vortex_plan *plan, const std::vector<tdgl::VortexJob> &jobs, int64_t j0, int64_t count,
                                  const double *src_xy, const int32_t *src_key, const double *tgt_xy,
                                  const int32_t *tgt_key, double r2, int32_t *out_idx, double *out_d2, int64_t *launches,
                                  int64_t *pairs) {
    for (int64_t c0 = j0; c0 < j0 + count; c0 += plan->link_max_jobs) {
        const int64_t c1 = std::min(j0 + count, c0 + plan->link_max_jobs);
        int64_t longest = 0;
        for (int64_t j = c0; j < c1; ++j) {
            longest = std::max(longest, jobs[j].src1 - jobs[j].src0);
            *pairs += (jobs[j].src1 - jobs[j].src0) * (jobs[j].tgt1 - jobs[j].tgt0);
        }
        hipLaunchKernelGGL(k_vortex_nearest, dim3((unsigned)((longest + BLOCK - 1) / BLOCK), (unsigned)(c1 - c0)), dim3(BLOCK),
                           0, plan->stream, plan->l_jobs.p + c0, reinterpret_cast<const double2 *>(src_xy), src_key,
                           reinterpret_cast<const double2 *>(tgt_xy), tgt_key, r2, out_idx, out_d2);
        ++*launches;
    }
}

template <class T>
static hipError_t vortex_room(DevBuf<T> &buf, int64_t count) {
    return buf.n < (size_t)count ? buf.alloc((size_t)count, false) : hipSuccess;
}

extern "C" int tdgl_vortex_plan_link(tdgl_vortex_plan *plan, int32_t n_frames, const int64_t *counts, const double *xy,
                                     const int32_t *charges, double max_distance, int32_t *next, int32_t *prev,
                                     int32_t *end_partner, int32_t *start_partner, int32_t *near, double *near_d2) {
    if (!plan) TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_link: null plan");
    if (n_frames < 1) TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_link: n_frames must be >= 1 (got %d)", (int)n_frames);
    if (!counts) TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_link: null counts");
    if (!(max_distance >= 0.0) || !std::isfinite(max_distance))
        TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_link: max_distance must be finite and >= 0 (got %g)", max_distance);
    const int64_t F = n_frames;
    std::vector<int32_t> offset((size_t)F + 1, 0);
    int64_t total = 0;
    for (int64_t f = 0; f < F; ++f) {
        if (counts[f] < 0)
            TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_link: negative count (%lld) in frame %lld", (long long)counts[f],
                      (long long)f);
        if (counts[f] > INT32_MAX || (total += counts[f]) > INT32_MAX)
            TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_link: the frames hold 2^31 cores or more (frame %lld)", (long long)f);
        offset[f + 1] = (int32_t)total;
    }
    const int64_t N = total;
    if (N > 0 && (!xy || !charges)) TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_link: null xy or charges with %lld cores", (long long)N);
    for (int64_t g = 0; g < N; ++g)
        if (charges[g] != 1 && charges[g] != -1)
            TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_link: charge %d of core %lld is neither +1 nor -1", (int)charges[g], (long long)g);
    const int64_t n_targets = plan->n_loop_sites;
    const bool want_near = (near || near_d2) && N > 0;
    if (want_near && n_targets > INT32_MAX)
        TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_link: the loops hold 2^31 sites or more");
    const double r2 = max_distance * max_distance;
    const bool want_ends = end_partner && F > 1 && N > 0, want_starts = start_partner && F > 1 && N > 0;
    const bool want_links = (next || prev || want_ends || want_starts) && F > 1 && N > 0;

    // the jobs: [forward | backward | ends | starts | loop sites]; a job with an empty side writes nothing new
    std::vector<tdgl::VortexJob> jobs;
    int64_t n_pair_jobs = 0, n_end_jobs = 0, n_start_jobs = 0;
    if (want_links) {
        for (int64_t f = 0; f + 1 < F; ++f)
            if (counts[f] > 0 && counts[f + 1] > 0) jobs.push_back({offset[f], offset[f + 1], offset[f + 1], offset[f + 2]});
        n_pair_jobs = (int64_t)jobs.size();
        for (int64_t j = 0; j < n_pair_jobs; ++j) jobs.push_back({jobs[j].tgt0, jobs[j].tgt1, jobs[j].src0, jobs[j].src1});
    }
    if (want_ends)
        for (int64_t f = 0; f + 1 < F; ++f)
            if (counts[f] > 1) {
                jobs.push_back({offset[f], offset[f + 1], offset[f], offset[f + 1]});
                ++n_end_jobs;
            }
    if (want_starts)
        for (int64_t f = 1; f < F; ++f)
            if (counts[f] > 1) {
                jobs.push_back({offset[f], offset[f + 1], offset[f], offset[f + 1]});
                ++n_start_jobs;
            }
    const int64_t near_job = (int64_t)jobs.size();
    const bool run_near = want_near && n_targets > 0;
    if (run_near) jobs.push_back({0, N, 0, n_targets});

    HIP_TRY(VORTEX_NO_CTX, hipSetDevice(plan->device));
    int64_t launches = 0, pairs = 0, links = 0;
    float ms = 0.f;
    std::vector<int32_t> host_next;
    if (want_links || run_near) {
        std::vector<int32_t> frame((size_t)N);
        for (int64_t f = 0; f < F; ++f) std::fill(frame.begin() + offset[f], frame.begin() + offset[f + 1], (int32_t)f);
        HIP_TRY(VORTEX_NO_CTX, vortex_room(plan->l_xy, 2 * N));
        HIP_TRY(VORTEX_NO_CTX, vortex_room(plan->l_charge, N));
        HIP_TRY(VORTEX_NO_CTX, vortex_room(plan->l_frame, N));
        HIP_TRY(VORTEX_NO_CTX, vortex_room(plan->l_offset, F + 1));
        HIP_TRY(VORTEX_NO_CTX, vortex_room(plan->l_jobs, (int64_t)jobs.size()));
        if (want_links)
            for (DevBuf<int32_t> *buf : {&plan->l_fwd, &plan->l_bwd, &plan->l_next, &plan->l_prev}) HIP_TRY(VORTEX_NO_CTX, vortex_room(*buf, N));
        if (want_ends || want_starts)
            for (DevBuf<int32_t> *buf : {&plan->l_src_key, &plan->l_tgt_key, &plan->l_choice, &plan->l_end, &plan->l_start})
                HIP_TRY(VORTEX_NO_CTX, vortex_room(*buf, N));
        if (run_near) {
            HIP_TRY(VORTEX_NO_CTX, vortex_room(plan->l_near, N));
            HIP_TRY(VORTEX_NO_CTX, vortex_room(plan->l_near_d2, N));
        }
        hipStream_t st = plan->stream;
        HIP_TRY(VORTEX_NO_CTX, hipMemcpyAsync(plan->l_xy.p, xy, (size_t)(2 * N) * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(VORTEX_NO_CTX, hipMemcpyAsync(plan->l_charge.p, charges, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(VORTEX_NO_CTX, hipMemcpyAsync(plan->l_frame.p, frame.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(VORTEX_NO_CTX, hipMemcpyAsync(plan->l_offset.p, offset.data(), (size_t)(F + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (!jobs.empty())
            HIP_TRY(VORTEX_NO_CTX, hipMemcpyAsync(plan->l_jobs.p, jobs.data(), jobs.size() * sizeof(tdgl::VortexJob), hipMemcpyHostToDevice, st));
        HIP_TRY(VORTEX_NO_CTX, hipEventRecord(plan->ev0, st));
        const dim3 cores((unsigned)((N + BLOCK - 1) / BLOCK));
        const size_t ibytes = (size_t)N * sizeof(int32_t);
        if (want_links) {
            // -1 wherever no job writes: the last frame's forward choice, the first frame's backward one, empty neighbours
            HIP_TRY(VORTEX_NO_CTX, hipMemsetAsync(plan->l_fwd.p, 0xFF, ibytes, st));
            HIP_TRY(VORTEX_NO_CTX, hipMemsetAsync(plan->l_bwd.p, 0xFF, ibytes, st));
            vortex_launch_nearest(plan, jobs, 0, n_pair_jobs, plan->l_xy.p, plan->l_charge.p, plan->l_xy.p, plan->l_charge.p, r2,
                                  plan->l_fwd.p, nullptr, &launches, &pairs);
            vortex_launch_nearest(plan, jobs, n_pair_jobs, n_pair_jobs, plan->l_xy.p, plan->l_charge.p, plan->l_xy.p,
                                  plan->l_charge.p, r2, plan->l_bwd.p, nullptr, &launches, &pairs);
            hipLaunchKernelGGL(k_vortex_mutual, cores, dim3(BLOCK), 0, st, N, 1, plan->l_frame.p, plan->l_offset.p, plan->l_fwd.p,
                               plan->l_bwd.p, plan->l_next.p);
            hipLaunchKernelGGL(k_vortex_mutual, cores, dim3(BLOCK), 0, st, N, -1, plan->l_frame.p, plan->l_offset.p, plan->l_bwd.p,
                               plan->l_fwd.p, plan->l_prev.p);
            launches += 2;
        }
        // loose ends of every frame but the last, then loose starts of every frame but the first: the same three steps
        int64_t j0 = 2 * n_pair_jobs;
        for (int side = 0; side < 2; ++side) {
            const bool wanted = side == 0 ? want_ends : want_starts;
            const int64_t n_jobs = side == 0 ? n_end_jobs : n_start_jobs;
            if (!wanted) continue;
            int32_t *out = side == 0 ? plan->l_end.p : plan->l_start.p;
            HIP_TRY(VORTEX_NO_CTX, hipMemsetAsync(plan->l_choice.p, 0xFF, ibytes, st));
            hipLaunchKernelGGL(k_vortex_event_keys, cores, dim3(BLOCK), 0, st, N, (int32_t)(side == 0 ? F - 1 : 0), plan->l_frame.p,
                               plan->l_charge.p, side == 0 ? plan->l_next.p : plan->l_prev.p, plan->l_src_key.p, plan->l_tgt_key.p);
            vortex_launch_nearest(plan, jobs, j0, n_jobs, plan->l_xy.p, plan->l_src_key.p, plan->l_xy.p, plan->l_tgt_key.p, r2,
                                  plan->l_choice.p, nullptr, &launches, &pairs);
            hipLaunchKernelGGL(k_vortex_mutual, cores, dim3(BLOCK), 0, st, N, 0, plan->l_frame.p, plan->l_offset.p, plan->l_choice.p,
                               plan->l_choice.p, out);
            launches += 2;
            j0 += n_jobs;
        }
        if (run_near)
            vortex_launch_nearest(plan, jobs, near_job, 1, plan->l_xy.p, nullptr, plan->loop_xy.p, nullptr, (double)INFINITY,
                                  plan->l_near.p, plan->l_near_d2.p, &launches, &pairs);
        HIP_TRY(VORTEX_NO_CTX, hipEventRecord(plan->ev1, st));
        HIP_TRY(VORTEX_NO_CTX, hipStreamSynchronize(st));
        HIP_TRY(VORTEX_NO_CTX, hipGetLastError());
        HIP_TRY(VORTEX_NO_CTX, hipEventElapsedTime(&ms, plan->ev0, plan->ev1));
        if (want_links) {
            host_next.resize((size_t)N);
            HIP_TRY(VORTEX_NO_CTX, hipMemcpy(host_next.data(), plan->l_next.p, ibytes, hipMemcpyDeviceToHost));
            for (int64_t g = 0; g < N; ++g) links += host_next[g] >= 0;
        }
    }
    // what no kernel ran for is known without one: a single frame links nothing, a plan without loops is nowhere near one
    const size_t ibytes = (size_t)N * sizeof(int32_t);
    if (N > 0) {
        if (next) {
            if (want_links) memcpy(next, host_next.data(), ibytes);
            else memset(next, 0xFF, ibytes);
        }
        if (prev) {
            if (want_links) HIP_TRY(VORTEX_NO_CTX, hipMemcpy(prev, plan->l_prev.p, ibytes, hipMemcpyDeviceToHost));
            else memset(prev, 0xFF, ibytes);
        }
        if (end_partner) {
            if (want_ends) HIP_TRY(VORTEX_NO_CTX, hipMemcpy(end_partner, plan->l_end.p, ibytes, hipMemcpyDeviceToHost));
            else memset(end_partner, 0xFF, ibytes);
        }
        if (start_partner) {
            if (want_starts) HIP_TRY(VORTEX_NO_CTX, hipMemcpy(start_partner, plan->l_start.p, ibytes, hipMemcpyDeviceToHost));
            else memset(start_partner, 0xFF, ibytes);
        }
        if (n_targets > 0) {
            if (near) HIP_TRY(VORTEX_NO_CTX, hipMemcpy(near, plan->l_near.p, ibytes, hipMemcpyDeviceToHost));
            if (near_d2) HIP_TRY(VORTEX_NO_CTX, hipMemcpy(near_d2, plan->l_near_d2.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
        } else {
            if (near) memset(near, 0xFF, ibytes);
            if (near_d2) std::fill(near_d2, near_d2 + N, (double)INFINITY);
        }
    }
    plan->link_ms = ms;
    plan->link_stats[0] = links;
    plan->link_stats[1] = F;
    plan->link_stats[2] = pairs;
    plan->link_stats[3] = launches;
    return TDGL_OK;
}

extern "C" int tdgl_vortex_plan_link_stats(tdgl_vortex_plan *plan, int64_t *out4, double *last_ms) {
    if (!plan) TDGL_FAIL(VORTEX_NO_CTX, TDGL_ERR_ARG, "tdgl_vortex_plan_link_stats: null plan");
    if (out4) memcpy(out4, plan->link_stats, sizeof(plan->link_stats));
    if (last_ms) *last_ms = plan->link_stats[3] > 0 ? plan->link_ms : 0.0;
    return TDGL_OK;
}
