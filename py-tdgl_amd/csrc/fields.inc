// Fields of the sheet currents away from the time loop: vector potential and magnetic field of n sites'
// currents at m arbitrary points (x, y, z).  Included by tdgl_hip.hip (after screening.inc: rsqrt_f64).
//
// Reference: tdgl/em.py:_biot_savart_2d_z / _biot_savart_2d_vector (Numba parallel loops) and the 1/r sum of
// Solution.vector_potential_at_position (tdgl/solution/solution.py:768-872).  Post-processing: the plan below owns
// its buffers and its stream and needs no tdgl_ctx.
//
// The same shape as k_induced_vector_potential: each thread keeps FIELD_TPT targets in registers, the sources stream
// through LDS in tiles of BLOCK as (x, y, a Kx, a Ky) per current field, read back as wave-wide broadcasts.  One
// corrected v_rsq_f64 per (target, source) pair serves everything asked for: 1/r for the vector potential, its cube
// for the field, both current fields.  dz is a property of the target (all sources lie in the plane z = z0), so the
// in-plane field components are two plain sums of w / r^3 that k_field_reduce multiplies by dz.
// blockIdx.y splits the source range; the partial sums land in part[chunk][component][target] and k_field_reduce adds
// them in chunk order (deterministic, no atomics).

namespace tdgl {

constexpr int FIELD_TPT = 2;  // targets per thread
constexpr int FIELD_A = 1, FIELD_Z = 2, FIELD_XY = 4;
// Padding sources sit at (FIELD_FAR, FIELD_FAR) with zero weight; user coordinates are limited to +-FIELD_COORD_MAX,
// so that every squared distance is finite (<= 2 (1e150 + 1e100)^2 + 4e200 < 1.8e308), 1/r is a normal number and
// 1/r^3 underflows to zero for the padding: a zero weight never meets an infinity.
constexpr double FIELD_FAR = 1e150;
constexpr double FIELD_COORD_MAX = 1e100;

__host__ __device__ constexpr int field_components(int what, int n_fields) {
    return n_fields * (((what & FIELD_A) ? 2 : 0) + ((what & FIELD_Z) ? 1 : 0) + ((what & FIELD_XY) ? 2 : 0));
}

// tgt: [m][3] = (x, y, z - z0) of this batch; src_xyw: [n][3] = (x, y, area); K: [NF][n][2];
// part: [chunks][components][m_stride], components per current field in the order (A_x, A_y), S_z, (sum w_y / r^3,
// sum w_x / r^3).
template <int WHAT, int NF>
__global__ __launch_bounds__(BLOCK) void k_field_sums(int64_t m, int64_t n, int64_t m_stride, int tiles_per_chunk,
                                                      const double *__restrict__ tgt,
                                                      const double *__restrict__ src_xyw,
                                                      const double *__restrict__ K, double *__restrict__ part) {
    constexpr bool WANT_A = (WHAT & FIELD_A) != 0, WANT_Z = (WHAT & FIELD_Z) != 0, WANT_XY = (WHAT & FIELD_XY) != 0;
    constexpr int NC = field_components(WHAT, 1);  // per current field
    __shared__ double4 tile[BLOCK];
    __shared__ double2 tile2[NF == 2 ? BLOCK : 1];
    double tx[FIELD_TPT], ty[FIELD_TPT], tz2[FIELD_TPT], acc[FIELD_TPT][NF][NC];
#pragma unroll
    for (int k = 0; k < FIELD_TPT; ++k) {
        const int64_t i = ((int64_t)blockIdx.x * FIELD_TPT + k) * BLOCK + threadIdx.x;
        tx[k] = (i < m) ? tgt[3 * i] : 0.0;
        ty[k] = (i < m) ? tgt[3 * i + 1] : 0.0;
        const double dz = (i < m) ? tgt[3 * i + 2] : 0.0;
        tz2[k] = dz * dz;
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[k][f][c] = 0.0;
    }
    const int64_t j0 = (int64_t)blockIdx.y * tiles_per_chunk * BLOCK;
    const int64_t j1 = min(n, j0 + (int64_t)tiles_per_chunk * BLOCK);
    for (int64_t base = j0; base < j1; base += BLOCK) {
        const int64_t j = base + threadIdx.x;
        if (j < j1) {
            const double a = src_xyw[3 * j + 2];
            tile[threadIdx.x] = make_double4(src_xyw[3 * j], src_xyw[3 * j + 1], a * K[2 * j], a * K[2 * j + 1]);
            if (NF == 2) tile2[threadIdx.x] = make_double2(a * K[2 * (n + j)], a * K[2 * (n + j) + 1]);
        } else {  // padding: zero weight, far from every target
            tile[threadIdx.x] = make_double4(FIELD_FAR, FIELD_FAR, 0.0, 0.0);
            if (NF == 2) tile2[threadIdx.x] = make_double2(0.0, 0.0);
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < BLOCK; ++t) {
            const double4 s = tile[t];
            double wx[NF], wy[NF];
            wx[0] = s.z;
            wy[0] = s.w;
            if (NF == 2) {
                const double2 s2 = tile2[t];
                wx[NF - 1] = s2.x;
                wy[NF - 1] = s2.y;
            }
#pragma unroll
            for (int k = 0; k < FIELD_TPT; ++k) {
                const double ddx = tx[k] - s.x, ddy = ty[k] - s.y;
                const double rinv = rsqrt_f64(fma(ddx, ddx, fma(ddy, ddy, tz2[k])));
                const double rinv3 = rinv * rinv * rinv;
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    int c = 0;
                    if (WANT_A) {
                        acc[k][f][c] = fma(wx[f], rinv, acc[k][f][c]);
                        acc[k][f][c + 1] = fma(wy[f], rinv, acc[k][f][c + 1]);
                        c += 2;
                    }
                    if (WANT_Z) {
                        acc[k][f][c] = fma(fma(wx[f], ddy, -(wy[f] * ddx)), rinv3, acc[k][f][c]);
                        c += 1;
                    }
                    if (WANT_XY) {
                        acc[k][f][c] = fma(wy[f], rinv3, acc[k][f][c]);
                        acc[k][f][c + 1] = fma(wx[f], rinv3, acc[k][f][c + 1]);
                    }
                }
            }
        }
        __syncthreads();
    }
    double *out = part + (int64_t)blockIdx.y * (NF * NC) * m_stride;
#pragma unroll
    for (int k = 0; k < FIELD_TPT; ++k) {
        const int64_t i = ((int64_t)blockIdx.x * FIELD_TPT + k) * BLOCK + threadIdx.x;
        if (i < m) {
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int c = 0; c < NC; ++c) out[(int64_t)(f * NC + c) * m_stride + i] = acc[k][f][c];
        }
    }
}

// Adds the chunk partials of one target batch in chunk order and writes the caller's layouts: S_A [nf][m_total][2],
// S_z [nf][m_total], S_xy [nf][m_total][2] = (dz sum w_y / r^3, -dz sum w_x / r^3); first target of the batch: b0.
// One thread per (target, component), blockIdx.y = component: a polygon's few hundred targets against a million
// sources have ~2,000 chunks to add, which one thread per target alone would do in a single workgroup.
__global__ __launch_bounds__(BLOCK) void k_field_reduce(int64_t mb, int64_t m_stride, int n_chunks, int what, int nf,
                                                        int64_t m_total, int64_t b0, const double *__restrict__ tgt,
                                                        const double *__restrict__ part, double *__restrict__ S_A,
                                                        double *__restrict__ S_z, double *__restrict__ S_xy) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i >= mb) return;
    const int nc = field_components(what, 1), total = nc * nf;
    const int comp = blockIdx.y, f = comp / nc;
    int c = comp % nc;
    const double *p = part + (int64_t)comp * m_stride + i;
    const int64_t step = (int64_t)total * m_stride;
    double sum = 0.0;
#pragma unroll 8
    for (int ch = 0; ch < n_chunks; ++ch) sum += p[ch * step];
    const int64_t row = (int64_t)f * m_total + b0 + i;
    if (what & FIELD_A) {
        if (c < 2) {
            S_A[2 * row + c] = sum;
            return;
        }
        c -= 2;
    }
    if (what & FIELD_Z) {
        if (c == 0) {
            S_z[row] = sum;
            return;
        }
        c -= 1;
    }
    const double dz = tgt[3 * i + 2];
    S_xy[2 * row + c] = c == 0 ? dz * sum : -(dz * sum);
}

}  // namespace tdgl

// ---------------------------------------------------------------------------------------
// A launch covers at most FIELD_MAX_PAIRS (target, source) pairs, so that no single launch runs for long and the
// partial-sum buffer stays bounded: larger m x n is cut into target batches (multiples of one workgroup's targets).
// Measured launch times: DESIGN.md section 3, "Fields of the currents".
static constexpr int64_t FIELD_MAX_PAIRS = (int64_t)1 << 35;
static constexpr int64_t FIELD_MAX_BATCH = (int64_t)1 << 20;  // targets per launch, whatever n
static constexpr int64_t FIELD_MIN_GROUPS = 2048;             // workgroups a launch should have (the source range is split to get there)
static constexpr int64_t FIELD_GROUP_TARGETS = (int64_t)FIELD_TPT * BLOCK;

struct tdgl_field_plan : tdgl::TimedStream {  // (stream, ev0, ev1)
    int device = 0;
    int64_t n = 0, m = 0;
    int64_t batch = 0;  // targets per launch
    DevBuf<double> src_xyw, tgt, K, part, S_A, S_z, S_xy;
    int64_t stats[4] = {0, 0, 0, 0};  // pairs, launches, source chunks (first batch), target batches of the last evaluation
    double last_ms = 0.0;
};

static tdgl_ctx *const FIELD_NO_CTX = nullptr;  // errors go to the global tdgl_last_error(NULL)

static bool field_coords_ok(const double *a, int64_t count) {
    for (int64_t i = 0; i < count; ++i)
        if (!(std::fabs(a[i]) <= FIELD_COORD_MAX)) return false;  // (NaN fails the comparison too)
    return true;
}

extern "C" void tdgl_field_plan_destroy(tdgl_field_plan *plan) {
    if (!plan) return;
    (void)hipSetDevice(plan->device);
    if (plan->stream) (void)hipStreamSynchronize(plan->stream);
    delete plan;
}

extern "C" int tdgl_field_plan_create(tdgl_field_plan **out, int device_id, int64_t n, const double *src_xy,
                                      const double *src_area, double z0, int64_t m, const double *target_xyz) {
    if (!out) TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_create: null output pointer");
    *out = nullptr;
    if (!src_xy || !src_area || !target_xyz) TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_create: null array");
    if (n < 1) TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_create: n must be >= 1 (got %lld)", (long long)n);
    if (m < 1) TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_create: m must be >= 1 (got %lld)", (long long)m);
    if (!field_coords_ok(src_xy, 2 * n) || !field_coords_ok(target_xyz, 3 * m) || !field_coords_ok(&z0, 1))
        TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG,
                  "tdgl_field_plan_create: coordinates must be finite and within +-%g", FIELD_COORD_MAX);
    for (int64_t j = 0; j < n; ++j)
        if (!std::isfinite(src_area[j])) TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_create: non-finite area");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count)
        TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_create: no HIP device %d (%d visible)", device_id, count);
    HIP_TRY(FIELD_NO_CTX, hipSetDevice(device_id));
    std::unique_ptr<tdgl_field_plan, void (*)(tdgl_field_plan *)> plan(new tdgl_field_plan, tdgl_field_plan_destroy);
    plan->device = device_id;
    plan->n = n;
    plan->m = m;
    HIP_TRY(FIELD_NO_CTX, plan->create());
    std::vector<double> sxyw(3 * n), t(3 * m);
    for (int64_t j = 0; j < n; ++j) {
        sxyw[3 * j] = src_xy[2 * j];
        sxyw[3 * j + 1] = src_xy[2 * j + 1];
        sxyw[3 * j + 2] = src_area[j];
    }
    for (int64_t i = 0; i < m; ++i) {
        t[3 * i] = target_xyz[3 * i];
        t[3 * i + 1] = target_xyz[3 * i + 1];
        t[3 * i + 2] = target_xyz[3 * i + 2] - z0;
    }
    HIP_TRY(FIELD_NO_CTX, plan->src_xyw.upload(sxyw));
    HIP_TRY(FIELD_NO_CTX, plan->tgt.upload(t));
    HIP_TRY(FIELD_NO_CTX, plan->K.alloc(2 * 2 * (size_t)n));
    const int64_t by_pairs = FIELD_MAX_PAIRS / n / FIELD_GROUP_TARGETS * FIELD_GROUP_TARGETS;
    plan->batch = std::min(FIELD_MAX_BATCH, std::max(FIELD_GROUP_TARGETS, by_pairs));
    *out = plan.release();
    return TDGL_OK;
}

// the split of the source range for a batch of mb targets: enough chunks for FIELD_MIN_GROUPS workgroups
static void field_split(int64_t n, int64_t mb, int *tiles_per_chunk, int *chunks) {
    const int64_t groups = (mb + FIELD_GROUP_TARGETS - 1) / FIELD_GROUP_TARGETS;
    const int64_t tiles = (n + BLOCK - 1) / BLOCK;
    const int64_t want = std::min<int64_t>(tiles, std::max<int64_t>(1, FIELD_MIN_GROUPS / groups));
    *tiles_per_chunk = (int)((tiles + want - 1) / want);
    *chunks = (int)((tiles + *tiles_per_chunk - 1) / *tiles_per_chunk);
}

template <int WHAT, int NF>
static void field_launch(tdgl_field_plan *p, int64_t b0, int64_t mb, int64_t m_stride, int tiles_per_chunk, int chunks) {
    const int gx = (int)((mb + FIELD_GROUP_TARGETS - 1) / FIELD_GROUP_TARGETS);
    hipLaunchKernelGGL((k_field_sums<WHAT, NF>), dim3(gx, chunks), dim3(BLOCK), 0, p->stream, mb, p->n, m_stride,
                       tiles_per_chunk, p->tgt.p + 3 * b0, p->src_xyw.p, p->K.p, p->part.p);
}

template <int NF>
static void field_launch_what(tdgl_field_plan *p, int what, int64_t b0, int64_t mb, int64_t m_stride, int tpc, int chunks) {
    switch (what) {
        case 1: field_launch<1, NF>(p, b0, mb, m_stride, tpc, chunks); break;
        case 2: field_launch<2, NF>(p, b0, mb, m_stride, tpc, chunks); break;
        case 3: field_launch<3, NF>(p, b0, mb, m_stride, tpc, chunks); break;
        case 4: field_launch<4, NF>(p, b0, mb, m_stride, tpc, chunks); break;
        case 5: field_launch<5, NF>(p, b0, mb, m_stride, tpc, chunks); break;
        case 6: field_launch<6, NF>(p, b0, mb, m_stride, tpc, chunks); break;
        default: field_launch<7, NF>(p, b0, mb, m_stride, tpc, chunks); break;
    }
}

extern "C" int tdgl_field_plan_eval(tdgl_field_plan *plan, int32_t n_fields, const double *K, int32_t what,
                                    double *S_A, double *S_z, double *S_xy) {
    if (!plan) TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_eval: null plan");
    if (!K) TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_eval: null current array");
    if (n_fields != 1 && n_fields != 2)
        TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_eval: n_fields must be 1 or 2 (got %d)", n_fields);
    if (what < 1 || what > 7)
        TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_eval: what must be a non-zero combination of bits 0-2 (got %d)", what);
    if (((what & FIELD_A) && !S_A) || ((what & FIELD_Z) && !S_z) || ((what & FIELD_XY) && !S_xy))
        TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_eval: null output array for a sum that was asked for");
    const int64_t n = plan->n, m = plan->m;
    HIP_TRY(FIELD_NO_CTX, hipSetDevice(plan->device));
    // buffers: the outputs asked for (kept between calls), the partial sums of the largest batch
    const size_t rows = (size_t)n_fields * m;
    if ((what & FIELD_A) && plan->S_A.n < 2 * rows) HIP_TRY(FIELD_NO_CTX, plan->S_A.alloc(2 * rows, false));
    if ((what & FIELD_Z) && plan->S_z.n < rows) HIP_TRY(FIELD_NO_CTX, plan->S_z.alloc(rows, false));
    if ((what & FIELD_XY) && plan->S_xy.n < 2 * rows) HIP_TRY(FIELD_NO_CTX, plan->S_xy.alloc(2 * rows, false));
    const int total = field_components(what, n_fields);
    size_t need = 0;
    for (const int64_t mb : {std::min(plan->batch, m), m - (m - 1) / plan->batch * plan->batch}) {  // full and last batch
        int tpc, chunks;
        field_split(n, mb, &tpc, &chunks);
        need = std::max(need, (size_t)chunks * total * (size_t)round_up(mb, BLOCK));
    }
    if (plan->part.n < need) HIP_TRY(FIELD_NO_CTX, plan->part.alloc(need, false));
    HIP_TRY(FIELD_NO_CTX, hipMemcpyAsync(plan->K.p, K, (size_t)n_fields * 2 * n * sizeof(double), hipMemcpyHostToDevice, plan->stream));
    HIP_TRY(FIELD_NO_CTX, hipEventRecord(plan->ev0, plan->stream));
    int64_t launches = 0, batches = 0, first_chunks = 0;
    for (int64_t b0 = 0; b0 < m; b0 += plan->batch, ++batches) {
        const int64_t mb = std::min(plan->batch, m - b0);
        const int64_t m_stride = round_up(mb, BLOCK);
        int tpc, chunks;
        field_split(n, mb, &tpc, &chunks);
        if (batches == 0) first_chunks = chunks;
        if (n_fields == 1)
            field_launch_what<1>(plan, what, b0, mb, m_stride, tpc, chunks);
        else
            field_launch_what<2>(plan, what, b0, mb, m_stride, tpc, chunks);
        ++launches;
        hipLaunchKernelGGL(k_field_reduce, dim3(grid_for(mb), total), dim3(BLOCK), 0, plan->stream, mb, m_stride, chunks, what,
                           n_fields, m, b0, plan->tgt.p + 3 * b0, plan->part.p, plan->S_A.p, plan->S_z.p, plan->S_xy.p);
    }
    HIP_TRY(FIELD_NO_CTX, hipEventRecord(plan->ev1, plan->stream));
    if (what & FIELD_A)
        HIP_TRY(FIELD_NO_CTX, hipMemcpyAsync(S_A, plan->S_A.p, 2 * rows * sizeof(double), hipMemcpyDeviceToHost, plan->stream));
    if (what & FIELD_Z)
        HIP_TRY(FIELD_NO_CTX, hipMemcpyAsync(S_z, plan->S_z.p, rows * sizeof(double), hipMemcpyDeviceToHost, plan->stream));
    if (what & FIELD_XY)
        HIP_TRY(FIELD_NO_CTX, hipMemcpyAsync(S_xy, plan->S_xy.p, 2 * rows * sizeof(double), hipMemcpyDeviceToHost, plan->stream));
    HIP_TRY(FIELD_NO_CTX, hipStreamSynchronize(plan->stream));
    HIP_TRY(FIELD_NO_CTX, hipGetLastError());
    float ms = 0.f;
    HIP_TRY(FIELD_NO_CTX, hipEventElapsedTime(&ms, plan->ev0, plan->ev1));
    plan->last_ms = ms;
    plan->stats[0] = m * n;
    plan->stats[1] = launches;
    plan->stats[2] = first_chunks;
    plan->stats[3] = batches;
    return TDGL_OK;
}

extern "C" int tdgl_field_plan_stats(tdgl_field_plan *plan, int64_t *out4, double *last_ms) {
    if (!plan) TDGL_FAIL(FIELD_NO_CTX, TDGL_ERR_ARG, "tdgl_field_plan_stats: null plan");
    if (out4) memcpy(out4, plan->stats, sizeof(plan->stats));
    if (last_ms) *last_ms = plan->last_ms;
    return TDGL_OK;
}
