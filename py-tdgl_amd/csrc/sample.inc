// Sheet current densities on the sites and values between the sites of saved steps, away from the time loop: the
// edge -> site average of Mesh.get_quantity_on_site, the piecewise-linear interpolant of triinterp.py at fixed points, and
// the dipole moment of the site densities, for many saved frames in one call.  Included by tdgl_hip.hip after
// vortices.inc.  The definitions are DESIGN.md section 3, "Currents between the sites"; tests/sample_model.py restates
// them in NumPy.
//
// Every result is a fixed sequence of separately rounded operations (fp contraction is off in every device function
// here), so the site densities, the location and the sampled values equal the NumPy model's bit for bit; the moment is
// a sum in a fixed order, the same bytes on every call and for every chunk length.  No atomics.
//
//   k_sample_locate   once, at create: one lane per point -> triangle (-1: in none) and weights (csrc/sample_grid.h)
//   k_sample_sites    one lane per site: its incidence row and direction cosines once per tile of SAMPLE_TILE
//                     (frame, field) pairs -> g [frame][field][site] (x, y)
//   k_sample_points   one lane per (point, frame, field): (w0 v0 + w1 v1) + w2 v2 per component, NaN where in no triangle
//   k_sample_moment   per (frame, field): workgroup partials of 1/2 ((x - cx) g_y - (y - cy) g_x) weight in site order,
//   k_sample_moment_finish   then one workgroup per (frame, field) over the partials

#include "sample_grid.h"

namespace tdgl {

constexpr int SAMPLE_TILE = 8;  // (frame, field) pairs a lane of k_sample_sites accumulates at once

__global__ __launch_bounds__(BLOCK) void k_sample_locate(tdgl_sample::GridView grid, int64_t m,
                                                         const double2 *__restrict__ points, int32_t *__restrict__ triangle,
                                                         double *__restrict__ weights) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= m) return;
    const double2 r = points[p];
    double w[3];
    triangle[p] = tdgl_sample::locate_point(grid, r.x, r.y, w);
    weights[3 * p] = w[0], weights[3 * p + 1] = w[1], weights[3 * p + 2] = w[2];
}

// values: [pairs][n_edges] (pair = frame * n_fields + field of the chunk); g: [pairs][n_sites].  Row i of the incidence
// CSR lists the edges with edges[e][0] == i in ascending order, then those with edges[e][1] == i: np.bincount's order.
__global__ __launch_bounds__(BLOCK) void k_sample_sites(int64_t n_sites, int64_t n_edges, int pairs,
                                                        const int64_t *__restrict__ row_ptr,
                                                        const int32_t *__restrict__ row_edge,
                                                        const double2 *__restrict__ edge_dir,
                                                        const double *__restrict__ values, double2 *__restrict__ g) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_sites) return;
    const int64_t k0 = row_ptr[i], k1 = row_ptr[i + 1];
    const double count = (double)(k1 - k0);
    for (int p0 = 0; p0 < pairs; p0 += SAMPLE_TILE) {
        const int np = min(SAMPLE_TILE, pairs - p0);
        double sx[SAMPLE_TILE], sy[SAMPLE_TILE];
#pragma unroll
        for (int q = 0; q < SAMPLE_TILE; ++q) sx[q] = sy[q] = 0.0;
        for (int64_t k = k0; k < k1; ++k) {
            const int32_t e = row_edge[k];
            const double2 d = edge_dir[e];
            const double *__restrict__ v = values + (int64_t)p0 * n_edges + e;
#pragma unroll
            for (int q = 0; q < SAMPLE_TILE; ++q) {
                if (q < np) {
                    const double f = v[(int64_t)q * n_edges];
                    sx[q] += f * d.x;
                    sy[q] += f * d.y;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < SAMPLE_TILE; ++q)
            if (q < np) g[(int64_t)(p0 + q) * n_sites + i] = make_double2(sx[q] / count / 2.0, sy[q] / count / 2.0);
    }
}

// values: [pairs][n_sites] (x, y) or (re, im); out: [pairs][m]
__global__ __launch_bounds__(BLOCK) void k_sample_points(int64_t m, int64_t n_sites, int64_t items,
                                                         const int32_t *__restrict__ triangle,
                                                         const double *__restrict__ weights,
                                                         const int32_t *__restrict__ elements,
                                                         const double2 *__restrict__ values, double2 *__restrict__ out) {
#pragma clang fp contract(off)
    const int64_t item = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (item >= items) return;
    const int64_t pair = item / m, p = item - pair * m;
    const int32_t t = triangle[p];
    if (t < 0) {
        const double nan = __builtin_nan("");
        out[item] = make_double2(nan, nan);
        return;
    }
    const double w0 = weights[3 * p], w1 = weights[3 * p + 1], w2 = weights[3 * p + 2];
    const double2 *__restrict__ v = values + pair * n_sites;
    const double2 a = v[elements[3 * (int64_t)t]], b = v[elements[3 * (int64_t)t + 1]], c = v[elements[3 * (int64_t)t + 2]];
    out[item] = make_double2((w0 * a.x + w1 * b.x) + w2 * c.x, (w0 * a.y + w1 * b.y) + w2 * c.y);
}

// the workgroup's sum in a fixed order: a tree over shared memory
__device__ inline double sample_block_sum(double v, double *scratch) {
#pragma clang fp contract(off)
    scratch[threadIdx.x] = v;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) scratch[threadIdx.x] += scratch[threadIdx.x + s];
        __syncthreads();
    }
    return scratch[0];
}

// grid (nb, pairs): partial[pair][block]
__global__ __launch_bounds__(BLOCK) void k_sample_moment(int64_t n_sites, double cx, double cy,
                                                         const double2 *__restrict__ sites,
                                                         const double *__restrict__ weight,
                                                         const double2 *__restrict__ g, double *__restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double scratch[BLOCK];
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    double term = 0.0;
    if (i < n_sites) {
        const double2 r = sites[i];
        const double2 k = g[(int64_t)blockIdx.y * n_sites + i];
        term = 0.5 * ((r.x - cx) * k.y - (r.y - cy) * k.x) * weight[i];
    }
    const double sum = sample_block_sum(term, scratch);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// one workgroup per pair: lane k adds partials k, k + BLOCK, ... in that order, then the tree
__global__ __launch_bounds__(BLOCK) void k_sample_moment_finish(int64_t nb, const double *__restrict__ partial,
                                                                double *__restrict__ moment) {
#pragma clang fp contract(off)
    __shared__ double scratch[BLOCK];
    const double *__restrict__ row = partial + (int64_t)blockIdx.x * nb;
    double acc = 0.0;
    for (int64_t k = threadIdx.x; k < nb; k += BLOCK) acc += row[k];
    const double sum = sample_block_sum(acc, scratch);
    if (threadIdx.x == 0) moment[blockIdx.x] = sum;
}

}  // namespace tdgl

// ---------------------------------------------------------------------------------------
// Frames go up in chunks: at most SAMPLE_MAX_CHUNK frames and at most SAMPLE_STAGE_BYTES of inputs and results on the
// device (one frame when a single frame is larger).  TDGL_SAMPLE_CHUNK=<frames> (tests) fixes the chunk, read at plan
// creation.
static constexpr int64_t SAMPLE_MAX_CHUNK = 32;
static constexpr int64_t SAMPLE_STAGE_BYTES = (int64_t)512 << 20;

struct tdgl_sample_plan : tdgl::TimedStream {  // (stream, ev0, ev1)
    int device = 0;
    int64_t n_sites = 0, n_edges = 0, n_tri = 0, m = 0;
    int64_t nb = 0;         // workgroups over the sites
    int64_t chunk_env = 0;  // TDGL_SAMPLE_CHUNK, 0: not set
    int64_t located = 0;    // points in a triangle
    bool has_weight = false;
    double cx = 0.0, cy = 0.0;
    tdgl_sample::GridView grid;  // device pointers
    DevBuf<double> sites, weight, edge_dir, tri_geom, points, loc_w;
    DevBuf<int32_t> elements, row_edge, cell_tri, loc_tri;
    DevBuf<int64_t> row_ptr, cell_ptr;
    DevBuf<double> values, psi, g, point_g, point_psi, partial, moment;  // per chunk
    int64_t stats[4] = {0, 0, 0, 0};  // points located, frames, chunks, kernel launches of the last call
    double last_ms = 0.0;
};

static tdgl_ctx *const SAMPLE_NO_CTX = nullptr;  // errors go to the global tdgl_last_error(NULL)

extern "C" void tdgl_sample_plan_destroy(tdgl_sample_plan *plan) {
    if (!plan) return;
    (void)hipSetDevice(plan->device);
    if (plan->stream) (void)hipStreamSynchronize(plan->stream);
    delete plan;
}

// the checks the plan and the host entry point share: sizes, the sites, the elements, the points
static int sample_check_mesh(const char *who, int64_t n_sites, const double *sites_xy, int64_t n_tri, const int32_t *elements,
                             int64_t m, const double *points_xy) {
    if (n_sites < 0 || n_tri < 0 || m < 0)
        TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: negative size (n_sites %lld, n_tri %lld, m %lld)", who, (long long)n_sites,
                  (long long)n_tri, (long long)m);
    if (n_sites < 1 || n_sites > INT32_MAX || n_tri > INT32_MAX / 3 || m > INT32_MAX)
        TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: n_sites must be in 1 .. 2^31 - 1, 3 n_tri and m below 2^31 (got %lld, %lld, %lld)",
                  who, (long long)n_sites, (long long)n_tri, (long long)m);
    if (!sites_xy) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: null sites_xy", who);
    if (n_tri > 0 && !elements) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: null elements", who);
    if (m > 0 && !points_xy) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: null points_xy", who);
    for (int64_t k = 0; k < 2 * n_sites; ++k)
        if (!std::isfinite(sites_xy[k]))
            TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: sites_xy: site %lld is not finite", who, (long long)(k / 2));
    for (int64_t k = 0; k < 3 * n_tri; ++k)
        if (elements[k] < 0 || elements[k] >= n_sites)
            TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: elements: element %lld names site %d, out of range for %lld sites", who,
                      (long long)(k / 3), (int)elements[k], (long long)n_sites);
    for (int64_t k = 0; k < 2 * m; ++k)
        if (!std::isfinite(points_xy[k]))
            TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: points_xy: point %lld is not finite", who, (long long)(k / 2));
    return TDGL_OK;
}

extern "C" int tdgl_host_sample_locate(int64_t n_sites, const double *sites_xy, int64_t n_tri, const int32_t *elements,
                                       int64_t m, const double *points_xy, int32_t *triangle, double *weights) {
    const int status = sample_check_mesh("tdgl_host_sample_locate", n_sites, sites_xy, n_tri, elements, m, points_xy);
    if (status != TDGL_OK) return status;
    if (m > 0 && (!triangle || !weights))
        TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "tdgl_host_sample_locate: null triangle or weights");
    const tdgl_sample::Grid grid = tdgl_sample::build_grid(n_sites, sites_xy, n_tri, elements);
    const tdgl_sample::GridView view = grid.view();
    for (int64_t p = 0; p < m; ++p)
        triangle[p] = tdgl_sample::locate_point(view, points_xy[2 * p], points_xy[2 * p + 1], weights + 3 * p);
    return TDGL_OK;
}

extern "C" int tdgl_sample_plan_create(tdgl_sample_plan **out, int device_id, int64_t n_sites, const double *sites_xy,
                                       const double *site_weight, const double *centre_xy, int64_t n_edges,
                                       const int32_t *edges, const double *edge_dir, int64_t n_tri, const int32_t *elements,
                                       int64_t m, const double *points_xy) {
    const char *who = "tdgl_sample_plan_create";
    if (!out) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: null output pointer", who);
    *out = nullptr;
    if (n_edges < 0) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: negative size (n_edges %lld)", who, (long long)n_edges);
    if (n_edges > INT32_MAX / 2) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: 2 n_edges must be below 2^31 (got %lld)", who, (long long)n_edges);
    const int status = sample_check_mesh(who, n_sites, sites_xy, n_tri, elements, m, points_xy);
    if (status != TDGL_OK) return status;
    if (n_edges > 0 && !edges) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: null edges", who);
    if (n_edges > 0 && !edge_dir) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: null edge_dir", who);
    if (site_weight && !centre_xy) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: null centre_xy (needed with site_weight)", who);
    if (site_weight) {
        for (int64_t i = 0; i < n_sites; ++i)
            if (!std::isfinite(site_weight[i]))
                TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: site_weight: the weight of site %lld is not finite", who, (long long)i);
        if (!std::isfinite(centre_xy[0]) || !std::isfinite(centre_xy[1]))
            TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: centre_xy is not finite", who);
    }
    for (int64_t k = 0; k < 2 * n_edges; ++k) {
        if (edges[k] < 0 || edges[k] >= n_sites)
            TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: edges: edge %lld names site %d, out of range for %lld sites", who,
                      (long long)(k / 2), (int)edges[k], (long long)n_sites);
        if (!std::isfinite(edge_dir[k]))
            TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: edge_dir: the direction of edge %lld is not finite", who, (long long)(k / 2));
    }
    // the incidence CSR in np.bincount's order: per site the edges that start there (ascending), then those that end there
    std::vector<int64_t> row_ptr((size_t)n_sites + 1, 0), starts((size_t)n_sites, 0);
    for (int64_t e = 0; e < n_edges; ++e) {
        ++row_ptr[(size_t)edges[2 * e] + 1];
        ++row_ptr[(size_t)edges[2 * e + 1] + 1];
        ++starts[(size_t)edges[2 * e]];
    }
    for (int64_t i = 0; i < n_sites; ++i) {
        if (row_ptr[i + 1] == 0)
            TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: edges: site %lld has no edge", who, (long long)i);
        row_ptr[i + 1] += row_ptr[i];
    }
    std::vector<int32_t> row_edge((size_t)(2 * n_edges));
    {
        std::vector<int64_t> first(row_ptr.begin(), row_ptr.end() - 1), second((size_t)n_sites);
        for (int64_t i = 0; i < n_sites; ++i) second[i] = row_ptr[i] + starts[i];
        for (int64_t e = 0; e < n_edges; ++e) {
            row_edge[(size_t)first[edges[2 * e]]++] = (int32_t)e;
            row_edge[(size_t)second[edges[2 * e + 1]]++] = (int32_t)e;
        }
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count)
        TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: no HIP device %d (%d visible)", who, device_id, count);
    HIP_TRY(SAMPLE_NO_CTX, hipSetDevice(device_id));
    std::unique_ptr<tdgl_sample_plan, void (*)(tdgl_sample_plan *)> plan(new tdgl_sample_plan, tdgl_sample_plan_destroy);
    plan->device = device_id;
    plan->n_sites = n_sites, plan->n_edges = n_edges, plan->n_tri = n_tri, plan->m = m;
    plan->nb = (n_sites + BLOCK - 1) / BLOCK;
    if (const char *env = getenv("TDGL_SAMPLE_CHUNK")) {
        const long asked = atol(env);
        if (asked >= 1 && asked <= SAMPLE_MAX_CHUNK) plan->chunk_env = asked;
    }
    HIP_TRY(SAMPLE_NO_CTX, plan->create());
    HIP_TRY(SAMPLE_NO_CTX, plan->sites.upload(std::vector<double>(sites_xy, sites_xy + 2 * n_sites)));
    HIP_TRY(SAMPLE_NO_CTX, plan->row_ptr.upload(row_ptr));
    HIP_TRY(SAMPLE_NO_CTX, plan->row_edge.upload(row_edge));
    HIP_TRY(SAMPLE_NO_CTX, plan->edge_dir.upload(std::vector<double>(edge_dir, edge_dir + 2 * n_edges)));
    HIP_TRY(SAMPLE_NO_CTX, plan->elements.upload(std::vector<int32_t>(elements, elements + 3 * n_tri)));
    if (site_weight) {
        plan->has_weight = true;
        plan->cx = centre_xy[0], plan->cy = centre_xy[1];
        HIP_TRY(SAMPLE_NO_CTX, plan->weight.upload(std::vector<double>(site_weight, site_weight + n_sites)));
    }
    if (m > 0) {
        const tdgl_sample::Grid grid = tdgl_sample::build_grid(n_sites, sites_xy, n_tri, elements);
        HIP_TRY(SAMPLE_NO_CTX, plan->cell_ptr.upload(grid.cell_ptr));
        HIP_TRY(SAMPLE_NO_CTX, plan->cell_tri.upload(grid.cell_tri));
        HIP_TRY(SAMPLE_NO_CTX, plan->tri_geom.upload(grid.tri));
        HIP_TRY(SAMPLE_NO_CTX, plan->points.upload(std::vector<double>(points_xy, points_xy + 2 * m)));
        HIP_TRY(SAMPLE_NO_CTX, plan->loc_tri.alloc((size_t)m, false));
        HIP_TRY(SAMPLE_NO_CTX, plan->loc_w.alloc((size_t)(3 * m), false));
        plan->grid = grid.view();
        plan->grid.cell_ptr = plan->cell_ptr.p, plan->grid.cell_tri = plan->cell_tri.p, plan->grid.tri = plan->tri_geom.p;
        hipLaunchKernelGGL(k_sample_locate, dim3((unsigned)((m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, plan->stream, plan->grid, m,
                           reinterpret_cast<const double2 *>(plan->points.p), plan->loc_tri.p, plan->loc_w.p);
        HIP_TRY(SAMPLE_NO_CTX, hipGetLastError());
        std::vector<int32_t> tri((size_t)m);
        HIP_TRY(SAMPLE_NO_CTX, hipMemcpyAsync(tri.data(), plan->loc_tri.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, plan->stream));
        HIP_TRY(SAMPLE_NO_CTX, hipStreamSynchronize(plan->stream));
        for (int64_t p = 0; p < m; ++p) plan->located += tri[p] >= 0;
        plan->stats[0] = plan->located;
    }
    *out = plan.release();
    return TDGL_OK;
}

extern "C" int tdgl_sample_plan_location(tdgl_sample_plan *plan, int32_t *triangle, double *weights) {
    if (!plan) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "tdgl_sample_plan_location: null plan");
    if (plan->m == 0) return TDGL_OK;
    HIP_TRY(SAMPLE_NO_CTX, hipSetDevice(plan->device));
    if (triangle)
        HIP_TRY(SAMPLE_NO_CTX, hipMemcpy(triangle, plan->loc_tri.p, (size_t)plan->m * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (weights)
        HIP_TRY(SAMPLE_NO_CTX, hipMemcpy(weights, plan->loc_w.p, (size_t)(3 * plan->m) * sizeof(double), hipMemcpyDeviceToHost));
    return TDGL_OK;
}

extern "C" int tdgl_sample_plan_eval(tdgl_sample_plan *plan, int32_t n_frames, int32_t n_fields, const double *edge_values,
                                     const double *psi, double *site_density, double *point_density, double *point_psi,
                                     double *moment) {
    const char *who = "tdgl_sample_plan_eval";
    if (n_fields < 0 || n_fields > 2) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: n_fields must be 0, 1 or 2 (got %d)", who, (int)n_fields);
    if (n_frames < 1) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: n_frames must be >= 1 (got %d)", who, (int)n_frames);
    if (!plan) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: null plan", who);
    if (n_fields > 0 && !edge_values) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: null edge_values with n_fields %d", who, (int)n_fields);
    if (n_fields == 0 && (site_density || point_density || moment))
        TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: %s needs edge_values (n_fields is 0)", who,
                  site_density ? "site_density" : point_density ? "point_density" : "moment");
    if (moment && !plan->has_weight)
        TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: moment needs the plan's site_weight (created without)", who);
    if (point_density && plan->m == 0) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: point_density needs points (the plan has m = 0)", who);
    if (point_psi && plan->m == 0) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: point_psi needs points (the plan has m = 0)", who);
    if (point_psi && !psi) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "%s: point_psi needs psi (null)", who);
    const int64_t n = plan->n_sites, E = plan->n_edges, m = plan->m, nb = plan->nb, F = n_frames, nf = n_fields;
    const bool want_sites = nf > 0 && (site_density || point_density || moment);
    const bool want_psi = point_psi != nullptr;
    int64_t chunk = plan->chunk_env;
    if (chunk == 0) {
        const int64_t per_frame = 8 * ((want_sites ? nf * (E + 2 * n + 2 * m) : 0) + (want_psi ? 2 * n + 2 * m : 0));
        chunk = std::max<int64_t>(1, std::min(SAMPLE_MAX_CHUNK, SAMPLE_STAGE_BYTES / std::max<int64_t>(per_frame, 1)));
    }
    chunk = std::min(chunk, F);
    HIP_TRY(SAMPLE_NO_CTX, hipSetDevice(plan->device));
    auto room = [](DevBuf<double> &buf, int64_t count) -> hipError_t {
        return buf.n < (size_t)count ? buf.alloc((size_t)count, false) : hipSuccess;
    };
    if (want_sites) {
        HIP_TRY(SAMPLE_NO_CTX, room(plan->values, chunk * nf * E));
        HIP_TRY(SAMPLE_NO_CTX, room(plan->g, chunk * nf * n * 2));
        if (point_density) HIP_TRY(SAMPLE_NO_CTX, room(plan->point_g, chunk * nf * m * 2));
        if (moment) {
            HIP_TRY(SAMPLE_NO_CTX, room(plan->partial, chunk * nf * nb));
            HIP_TRY(SAMPLE_NO_CTX, room(plan->moment, chunk * nf));
        }
    }
    if (want_psi) {
        HIP_TRY(SAMPLE_NO_CTX, room(plan->psi, chunk * n * 2));
        HIP_TRY(SAMPLE_NO_CTX, room(plan->point_psi, chunk * m * 2));
    }
    const double2 *d_sites = reinterpret_cast<const double2 *>(plan->sites.p);
    int64_t launches = 0, chunks = 0;
    double total_ms = 0.0;
    auto grid_of = [](int64_t items) { return dim3((unsigned)((items + BLOCK - 1) / BLOCK)); };
    for (int64_t g0 = 0; g0 < F && (want_sites || want_psi); g0 += chunk, ++chunks) {
        const int64_t fc = std::min(chunk, F - g0);
        const int pairs = (int)(fc * nf);
        if (want_sites)
            HIP_TRY(SAMPLE_NO_CTX, hipMemcpyAsync(plan->values.p, edge_values + g0 * nf * E, (size_t)(fc * nf * E) * sizeof(double),
                                                 hipMemcpyHostToDevice, plan->stream));
        if (want_psi)
            HIP_TRY(SAMPLE_NO_CTX, hipMemcpyAsync(plan->psi.p, psi + g0 * 2 * n, (size_t)(fc * 2 * n) * sizeof(double),
                                                 hipMemcpyHostToDevice, plan->stream));
        HIP_TRY(SAMPLE_NO_CTX, hipEventRecord(plan->ev0, plan->stream));
        if (want_sites) {
            double2 *d_g = reinterpret_cast<double2 *>(plan->g.p);
            hipLaunchKernelGGL(k_sample_sites, dim3((unsigned)nb), dim3(BLOCK), 0, plan->stream, n, E, pairs, plan->row_ptr.p,
                               plan->row_edge.p, reinterpret_cast<const double2 *>(plan->edge_dir.p), plan->values.p, d_g);
            ++launches;
            if (point_density) {
                hipLaunchKernelGGL(k_sample_points, grid_of(pairs * m), dim3(BLOCK), 0, plan->stream, m, n, (int64_t)pairs * m,
                                   plan->loc_tri.p, plan->loc_w.p, plan->elements.p, d_g,
                                   reinterpret_cast<double2 *>(plan->point_g.p));
                ++launches;
            }
            if (moment) {
                hipLaunchKernelGGL(k_sample_moment, dim3((unsigned)nb, (unsigned)pairs), dim3(BLOCK), 0, plan->stream, n, plan->cx,
                                   plan->cy, d_sites, plan->weight.p, d_g, plan->partial.p);
                hipLaunchKernelGGL(k_sample_moment_finish, dim3((unsigned)pairs), dim3(BLOCK), 0, plan->stream, nb,
                                   plan->partial.p, plan->moment.p);
                launches += 2;
            }
        }
        if (want_psi) {
            hipLaunchKernelGGL(k_sample_points, grid_of(fc * m), dim3(BLOCK), 0, plan->stream, m, n, fc * m, plan->loc_tri.p,
                               plan->loc_w.p, plan->elements.p, reinterpret_cast<const double2 *>(plan->psi.p),
                               reinterpret_cast<double2 *>(plan->point_psi.p));
            ++launches;
        }
        HIP_TRY(SAMPLE_NO_CTX, hipEventRecord(plan->ev1, plan->stream));
        if (site_density)
            HIP_TRY(SAMPLE_NO_CTX, hipMemcpyAsync(site_density + g0 * nf * n * 2, plan->g.p, (size_t)(fc * nf * n * 2) * sizeof(double),
                                                 hipMemcpyDeviceToHost, plan->stream));
        if (point_density)
            HIP_TRY(SAMPLE_NO_CTX, hipMemcpyAsync(point_density + g0 * nf * m * 2, plan->point_g.p,
                                                 (size_t)(fc * nf * m * 2) * sizeof(double), hipMemcpyDeviceToHost, plan->stream));
        if (moment)
            HIP_TRY(SAMPLE_NO_CTX, hipMemcpyAsync(moment + g0 * nf, plan->moment.p, (size_t)(fc * nf) * sizeof(double),
                                                 hipMemcpyDeviceToHost, plan->stream));
        if (want_psi)
            HIP_TRY(SAMPLE_NO_CTX, hipMemcpyAsync(point_psi + g0 * m * 2, plan->point_psi.p, (size_t)(fc * m * 2) * sizeof(double),
                                                 hipMemcpyDeviceToHost, plan->stream));
        // the staging buffers are reused by the next chunk: wait, and add this chunk's device time
        HIP_TRY(SAMPLE_NO_CTX, hipStreamSynchronize(plan->stream));
        HIP_TRY(SAMPLE_NO_CTX, hipGetLastError());
        float ms = 0.f;
        HIP_TRY(SAMPLE_NO_CTX, hipEventElapsedTime(&ms, plan->ev0, plan->ev1));
        total_ms += ms;
    }
    plan->last_ms = total_ms;
    plan->stats[0] = plan->located;
    plan->stats[1] = F;
    plan->stats[2] = chunks;
    plan->stats[3] = launches;
    return TDGL_OK;
}

extern "C" int tdgl_sample_plan_stats(tdgl_sample_plan *plan, int64_t *out4, double *last_ms) {
    if (!plan) TDGL_FAIL(SAMPLE_NO_CTX, TDGL_ERR_ARG, "tdgl_sample_plan_stats: null plan");
    if (out4) memcpy(out4, plan->stats, sizeof(plan->stats));
    if (last_ms) *last_ms = plan->last_ms;
    return TDGL_OK;
}
