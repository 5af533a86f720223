// Device kernels of libtdgl_hip (gfx950, wave64).  Included by tdgl_hip.hip.
//
// Everything here is bandwidth bound (fp64 sparse gathers, < 1 flop/byte): no MFMA.  The
// layout rules that matter are (1) SELL-64: a wavefront reads 64 consecutive values /
// column indices per instruction, (2) 16-byte accesses for complex data, (3) the
// blockIdx -> slice mapping gives every XCD a contiguous range of rows so that the gathered
// psi / p entries of neighbouring rows are re-used from that XCD's private L2.

namespace tdgl {

// ------------------------------------------------------------------ helpers
// Workgroups are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8).  Map block
// b to logical tile (b % 8) * per_xcd + b / 8 so that one XCD walks a contiguous row range.
// Performance only: any other placement gives the same result.
__device__ __forceinline__ int xcd_tile(int b, int per_xcd) {
    return (b % XCDS) * per_xcd + b / XCDS;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, WAVE));
    return v;
}

// Sum over a 256-thread workgroup; result valid in thread 0.  Fixed order -> deterministic.
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double sh[BLOCK / WAVE];
    v = wave_sum(v);
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < BLOCK / WAVE; ++i) t += sh[i];
    }
    return t;
}

__device__ __forceinline__ double block_max(double v) {
    __shared__ double shm[BLOCK / WAVE];
    v = wave_max(v);
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    __syncthreads();
    if (lane == 0) shm[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < BLOCK / WAVE; ++i) t = fmax(t, shm[i]);
    }
    return t;
}

// ------------------------------------------------------------------ link variables
// U_e = exp(-i A_e . d_e)   (operators.py:109-111, 153-155)
// (A2, if given, is added: applied + induced vector potential, solver.py:673)
__device__ __forceinline__ void link_variable_body(int64_t e, const double *__restrict__ A, const double *__restrict__ A2,
                                                   const double *__restrict__ dx, const double *__restrict__ dy,
                                                   double2 *__restrict__ U) {
    double ax = A[2 * e], ay = A[2 * e + 1];
    if (A2) {
        ax += A2[2 * e];
        ay += A2[2 * e + 1];
    }
    double theta = ax * dx[e] + ay * dy[e];
    double s, c;
    sincos(theta, &s, &c);
    U[e] = make_double2(c, -s);
}

__global__ __launch_bounds__(BLOCK) void k_link_variables(int64_t m, const double *__restrict__ A,
                                                          const double *__restrict__ A2,
                                                          const double *__restrict__ dx,
                                                          const double *__restrict__ dy,
                                                          double2 *__restrict__ U,
                                                          const int32_t *__restrict__ only_if) {
    int64_t e = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (e >= m || (only_if && !only_if[0])) return;
    link_variable_body(e, A, A2, dx, dy, U);
}

// out = scale * base (epsilon = factor(t) * epsilon0 of the loop with one synchronisation per step: apply_time_tables)
__global__ __launch_bounds__(BLOCK) void k_scale(int64_t n, double scale, const double *__restrict__ base,
                                                 double *__restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i < n) out[i] = scale * base[i];
}

// dA/dt along each edge: ((A_new - A_prev) / dt) . e_hat  (solver.py:630-634); A_prev <- A_new.
// Also evaluates the reference's test `not np.allclose(new_A, current_A)` (solver.py:636-637,
// |new - old| <= 1e-8 + 1e-5 |old| elementwise): per-workgroup flags, reduced by k_any_flag.  The
// reference refreshes the link variables only when that test fires -- with a very small dt a ramp
// moves A by less than the tolerance per step and the links lag; reproduced.
__device__ __forceinline__ int dadt_body(int64_t e, int64_t m, double inv_dt, double ax, double ay, double *__restrict__ Aprev,
                                         const double *__restrict__ dx, const double *__restrict__ dy,
                                         const double *__restrict__ inv_len, double *__restrict__ dadt) {
    if (e >= m) return 0;
    const double px = Aprev[2 * e], py = Aprev[2 * e + 1];
    const double il = inv_len[e];
    dadt[e] = ((ax - px) * inv_dt) * (dx[e] * il) + ((ay - py) * inv_dt) * (dy[e] * il);
    Aprev[2 * e] = ax;
    Aprev[2 * e + 1] = ay;
    return !(fabs(ax - px) <= 1e-8 + 1e-5 * fabs(px)) || !(fabs(ay - py) <= 1e-8 + 1e-5 * fabs(py));
}

__global__ __launch_bounds__(BLOCK) void k_dadt(int64_t m, double inv_dt, const double *__restrict__ A,
                                                double *__restrict__ Aprev, const double *__restrict__ dx,
                                                const double *__restrict__ dy,
                                                const double *__restrict__ inv_len,
                                                double *__restrict__ dadt, int32_t *__restrict__ block_changed) {
    const int64_t e = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    const int changed = e < m ? dadt_body(e, m, inv_dt, A[2 * e], A[2 * e + 1], Aprev, dx, dy, inv_len, dadt) : 0;
    const int any = __syncthreads_or(changed);
    if (threadIdx.x == 0) block_changed[blockIdx.x] = any;
}

// flag[0] = OR of the per-workgroup flags (one workgroup)
// (only_if, run-ahead loop with a field ramp: 0 there means "nothing moved in this attempt" -> flag = 0)
__global__ __launch_bounds__(BLOCK) void k_any_flag(int n, const int32_t *__restrict__ block_flags,
                                                    int32_t *__restrict__ flag, const int32_t *__restrict__ only_if = nullptr) {
    int v = 0;
    if (!only_if || *only_if)
        for (int i = threadIdx.x; i < n; i += BLOCK) v |= block_flags[i];
    const int any = __syncthreads_or(v);
    if (threadIdx.x == 0) flag[0] = any;
}

// ceff = cvec + divergence(dA/dt)  (operators.py:59-84 applied to the edge field dA/dt), gathered
// over the row's incident edges through the SELL slots of the site graph.
// (body: one row of `slice`; the row must be < n_rows)
__device__ __forceinline__ void ceff_body(int slice, int lane, int64_t row, const int32_t *__restrict__ slice_off,
                                          const int32_t *__restrict__ slot_edge, const double *__restrict__ slot_w,
                                          const double *__restrict__ inv_len, const double *__restrict__ dadt,
                                          const double *__restrict__ cvec, double *__restrict__ ceff) {
    double acc = 0.0;
    if (dadt) {
        int64_t idx = (int64_t)slice_off[slice] * WAVE + lane;
        for (int k = slice_off[slice]; k < slice_off[slice + 1]; ++k, idx += WAVE) {
            const int32_t code = slot_edge[idx];
            if (code < 0) continue;
            const int e = code >> 1;
            const double v = slot_w[idx] / inv_len[e] * dadt[e];  // (s_e / a_i) dA/dt_e
            acc += (code & 1) ? -v : v;
        }
    }
    ceff[row] = (cvec ? cvec[row] : 0.0) + acc;
}

__global__ __launch_bounds__(BLOCK) void k_ceff(int n_slices, int64_t n_rows, const int32_t *__restrict__ slice_off,
                                                const int32_t *__restrict__ slot_edge,
                                                const double *__restrict__ slot_w,
                                                const double *__restrict__ inv_len,
                                                const double *__restrict__ dadt,
                                                const double *__restrict__ cvec, double *__restrict__ ceff,
                                                const int32_t *__restrict__ only_if = nullptr) {
    if (only_if && !*only_if) return;
    const int slice = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
    if (slice >= n_slices) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t row = (int64_t)slice * WAVE + lane;
    if (row >= n_rows) return;
    ceff_body(slice, lane, row, slice_off, slot_edge, slot_w, inv_len, dadt, cvec, ceff);
}

// Covariant-Laplacian values per SELL slot: (w_e / a_i) * U_e for the edge's own
// orientation, conj(U_e) for the reversed one (operators.py:162-168).
__device__ __forceinline__ void fill_laplacian_body(int64_t s, const int32_t *__restrict__ slot_edge,
                                                    const double *__restrict__ slot_w, const double2 *__restrict__ U,
                                                    double2 *__restrict__ vals) {
    int32_t code = slot_edge[s];
    double2 v = make_double2(0.0, 0.0);
    if (code >= 0) {
        double2 u = U[code >> 1];
        double w = slot_w[s];
        v = make_double2(w * u.x, (code & 1) ? -(w * u.y) : w * u.y);
    }
    vals[s] = v;
}

__global__ __launch_bounds__(BLOCK) void k_fill_laplacian(int64_t n_slots,
                                                          const int32_t *__restrict__ slot_edge,
                                                          const double *__restrict__ slot_w,
                                                          const double2 *__restrict__ U,
                                                          double2 *__restrict__ vals,
                                                          const int32_t *__restrict__ only_if) {
    int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (s >= n_slots || (only_if && !only_if[0])) return;
    fill_laplacian_body(s, slot_edge, slot_w, U, vals);
}

constexpr int SELL_BATCH = 8;

// column index of a SELL slot: absolute (int32) or relative to the row (int16, SellPattern::cols16)
template <class IT>
__device__ __forceinline__ int col_at(const IT *__restrict__ cols, int64_t idx, int64_t row);
template <>
__device__ __forceinline__ int col_at<int32_t>(const int32_t *__restrict__ cols, int64_t idx, int64_t) {
    return cols[idx];
}
template <>
__device__ __forceinline__ int col_at<int16_t>(const int16_t *__restrict__ cols, int64_t idx, int64_t row) {
    return (int)row + (int)cols[idx];
}

// ------------------------------------------------------------------ K1: psi Laplacian
// lap_i = diag_i psi_i + sum_k val_ik psi_{col_ik}          (operators.py:120-185)
// Rows flagged `fixed` are identity rows (operators.py:170-181).  With RHS = true the
// kernel also emits the right-hand side of the SPD mu system,
//     b_i = -a_i * ( Im(conj(psi_i) S_i) - c_i ),
// where S_i is the UNMASKED row sum: Im(conj(psi_i) S_i) = (divergence @ J_s)_i
// (solver.py:507-510; DESIGN.md "rhs without forming J_s").
template <bool RHS, class IT>
__device__ __forceinline__ void psi_laplacian_body(
    int n_slices, int per_xcd, int tile_base, int64_t n_rows, const int32_t *__restrict__ slice_off,
    const IT *__restrict__ cols, const double2 *__restrict__ vals,
    const double *__restrict__ diag, const uint8_t *__restrict__ fixed,
    const double2 *__restrict__ psi, double2 *__restrict__ lap, const double *__restrict__ area,
    const double *__restrict__ cvec, double *__restrict__ bvec) {
    // (tile_base / n_slices bound a tile range: one-process-per-GPU mode runs the ghost-free
    // rows while the halo exchange is in flight and the remaining rows after it, comm.inc)
    const int tile = tile_base + xcd_tile(blockIdx.x, per_xcd);
    // (the slice index is wave-uniform: telling the compiler makes slice_off a scalar load and
    // the entry count a scalar, so the batches below are straight-line code)
    const int slice = __builtin_amdgcn_readfirstlane(tile * (BLOCK / WAVE) + (threadIdx.x / WAVE));
    if (slice >= n_slices) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t row = (int64_t)slice * WAVE + lane;
    if (row >= n_rows) return;  // (distributed: entries past the owned rows are ghost sites)
    const int beg = slice_off[slice], cnt = slice_off[slice + 1] - beg;
    // every row-indexed operand is requested before the first wait
    const double2 pi = psi[row];
    const double d = diag[row];
    const uint8_t fx = fixed[row];
    double a = 0.0, cv = 0.0;
    if (RHS) {
        a = area[row];
        cv = cvec[row];
    }
    double sr = d * pi.x, si = d * pi.y;
    const int64_t idx0 = (int64_t)beg * WAVE + lane;
    // (Measured in round 3, profiles/KAB_r03f.txt / KAB_r03g.txt: a software-pipelined persistent variant
    // -- next slice's operator stream requested behind the current gathers -- and chunked / plain
    // block -> tile mappings all run in the same 33-34 us: 176 MB at 5.2 TB/s is what an HBM-cold
    // read stream delivers on this chip, 5.36 TB/s for a plain grid-stride sum, tools/bench_barrier.py.)
    // Memory-level parallelism: the operator is HBM-cold in the step, so the number of DEPENDENT
    // round trips per wave is what bounds the kernel.  All column indices and values of a batch of
    // SELL_BATCH entries are requested at once, then all gathers: three round trips for a row of
    // <= 8 entries.  Entries past the slice width re-read the last one (a cache hit, no HBM
    // traffic) with the value forced to 0.
    for (int base = 0; base < cnt; base += SELL_BATCH) {
        int c[SELL_BATCH];
        double2 v[SELL_BATCH];
#pragma unroll
        for (int k = 0; k < SELL_BATCH; ++k) {
            const int kk = min(base + k, cnt - 1);
            c[k] = col_at<IT>(cols, idx0 + (int64_t)kk * WAVE, row);
            v[k] = vals[idx0 + (int64_t)kk * WAVE];
        }
#pragma unroll
        for (int k = 0; k < SELL_BATCH; ++k) {
            const double2 pj = psi[c[k]];
            const double w = (base + k < cnt) ? 1.0 : 0.0;
            const double vx = w * v[k].x, vy = w * v[k].y;
            sr += vx * pj.x - vy * pj.y;
            si += vx * pj.y + vy * pj.x;
        }
    }
    if (RHS) {
        const double div_js = pi.x * si - pi.y * sr;
        bvec[row] = -a * (div_js - cv);
    }
    lap[row] = fx ? pi : make_double2(sr, si);
}

template <bool RHS, class IT>
__global__ __launch_bounds__(BLOCK) void k_psi_laplacian(
    int n_slices, int per_xcd, int tile_base, int64_t n_rows, const int32_t *__restrict__ slice_off,
    const IT *__restrict__ cols, const double2 *__restrict__ vals,
    const double *__restrict__ diag, const uint8_t *__restrict__ fixed,
    const double2 *__restrict__ psi, double2 *__restrict__ lap, const double *__restrict__ area,
    const double *__restrict__ cvec, double *__restrict__ bvec) {
    psi_laplacian_body<RHS, IT>(n_slices, per_xcd, tile_base, n_rows, slice_off, cols, vals, diag, fixed, psi, lap, area, cvec, bvec);
}

// ... in the run-ahead time loop (run.inc): which of the two psi / L psi buffers holds the attempt's psi' is
// decided on the device (ctl->cur: 0 -> the attempt wrote buffer 1), and a dead step does nothing
template <class IT>
__global__ __launch_bounds__(BLOCK) void k_psi_laplacian_ra(
    int n_slices, int per_xcd, int64_t n_rows, const int32_t *__restrict__ slice_off,
    const IT *__restrict__ cols, const double2 *__restrict__ vals,
    const double *__restrict__ diag, const uint8_t *__restrict__ fixed,
    const double2 *__restrict__ psi0, const double2 *__restrict__ psi1, double2 *__restrict__ lap0, double2 *__restrict__ lap1,
    const double *__restrict__ area, const double *__restrict__ cvec, double *__restrict__ bvec,
    const StepCtl *__restrict__ ctl) {
    if (!ctl->live) return;
    const bool to1 = ctl->cur == 0;
    psi_laplacian_body<true, IT>(n_slices, per_xcd, 0, n_rows, slice_off, cols, vals, diag, fixed, to1 ? psi1 : psi0,
                                 to1 ? lap1 : lap0, area, cvec, bvec);
}

// ------------------------------------------------------------------ K2: pointwise psi update
// TDGLSolver.solve_for_psi_squared (solver.py:383-439, docs/background.rst:273-353).
// Writes psi' to a separate buffer so a failed step can be retried with a smaller dt.
// status->fail_flag is raised where the reference returns None (negative discriminant or a
// floating point exception); status->dmax_bits receives max | |psi'|^2 - |psi|^2 |
// (solver.py:701) as an ordered bit pattern (non-negative doubles compare like uint64).
// (body: `nblk` workgroups numbered `blk` share the sites; the fused variant below runs other work in the
// remaining workgroups of its launch)
__device__ __forceinline__ void psi_update_body(
    int blk, int nblk, int64_t n, const double2 *__restrict__ psi, const double *__restrict__ mu,
    const double *__restrict__ eps, const double2 *__restrict__ lap, double dt, double u,
    double gamma, double2 *__restrict__ psi_new, double *__restrict__ abs_sq_out,
    double *__restrict__ dmax_part, int32_t *__restrict__ fail_part, const double *__restrict__ abs_sq_in) {
    const double g2 = gamma * gamma;
    const double half_g2 = g2 / 2;
    const double dt_u = dt / u;
    double dmax = 0.0;
    int bad = 0;
    for (int64_t i = blk * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)nblk * BLOCK) {
        const double2 p = psi[i];
        const double2 l = lap[i];
        // (screening iterations pass |psi|^2 of the step's STARTING psi: solver.py:676-678)
        const double a2 = abs_sq_in ? abs_sq_in[i] : p.x * p.x + p.y * p.y;
        double s, c;
        sincos(mu[i] * dt, &s, &c);
        const double ur = c, ui = -s;  // U = exp(-i mu dt)
        // z = U * gamma^2/2 * psi
        const double zr = half_g2 * (ur * p.x - ui * p.y);
        const double zi = half_g2 * (ur * p.y + ui * p.x);
        // t = psi + (dt/u) sqrt(1 + gamma^2 |psi|^2) ((eps - |psi|^2) psi + lap)
        const double f = dt_u * sqrt(1.0 + g2 * a2);
        const double ea = eps[i] - a2;
        const double tr = p.x + f * (ea * p.x + l.x);
        const double ti = p.y + f * (ea * p.y + l.y);
        // w = z |psi|^2 + U t
        const double wr = zr * a2 + (ur * tr - ui * ti);
        const double wi = zi * a2 + (ur * ti + ui * tr);
        const double cc = wr * zr + wi * zi;
        const double b = 2.0 * cc + 1.0;
        const double w2 = wr * wr + wi * wi;
        const double z2 = zr * zr + zi * zi;
        const double disc = b * b - 4.0 * z2 * w2;
        if (!(disc >= 0.0) || !isfinite(w2) || !isfinite(disc)) bad = 1;
        const double nsq = (2.0 * w2) / (b + sqrt(fmax(disc, 0.0)));
        psi_new[i] = make_double2(wr - zr * nsq, wi - zi * nsq);
        if (abs_sq_out) abs_sq_out[i] = nsq;
        dmax = fmax(dmax, fabs(nsq - a2));
    }
    const double bm = block_max(dmax);
    const int anybad = __syncthreads_or(bad);
    // one plain store per workgroup; k_publish_status / k_status_pack reduce the <= 2048 entries.
    // (Atomics on a shared status word serialise: 2048 same-line atomicMax cost more than the
    // whole rest of this kernel.)
    if (threadIdx.x == 0) {
        dmax_part[blk] = bm;
        fail_part[blk] = anybad ? 1 : 0;
    }
}

__global__ __launch_bounds__(BLOCK) void k_psi_update(
    int64_t n, const double2 *__restrict__ psi, const double *__restrict__ mu,
    const double *__restrict__ eps, const double2 *__restrict__ lap, double dt, double u,
    double gamma, double2 *__restrict__ psi_new, double *__restrict__ abs_sq_out,
    double *__restrict__ dmax_part, int32_t *__restrict__ fail_part, const double *__restrict__ abs_sq_in) {
    psi_update_body(blockIdx.x, gridDim.x, n, psi, mu, eps, lap, dt, u, gamma, psi_new, abs_sq_out, dmax_part, fail_part,
                    abs_sq_in);
}

// ------------------------------------------------------------------ K3 + K6: edge currents
// J_s,e = Im(conj(psi_i) (U_e psi_j - psi_i) / l_e)     (operators.py:87-117, 385-394)
// J_n,e = -(mu_j - mu_i) / l_e                          (solver.py:519)
template <bool JS, bool JN>
__device__ __forceinline__ void edge_currents_body(
    int64_t e, int64_t m, const int32_t *__restrict__ e0, const int32_t *__restrict__ e1,
    const double *__restrict__ inv_len, const double2 *__restrict__ U,
    const double2 *__restrict__ psi, const double *__restrict__ mu, double *__restrict__ js,
    double *__restrict__ jn, const double *__restrict__ dadt) {
    if (e >= m) return;
    const int i = e0[e], j = e1[e];
    const double il = inv_len[e];
    if (JS) {
        const double2 pi = psi[i], pj = psi[j], ue = U[e];
        const double gr = (ue.x * il) * pj.x - (ue.y * il) * pj.y - il * pi.x;
        const double gi = (ue.x * il) * pj.y + (ue.y * il) * pj.x - il * pi.y;
        js[e] = pi.x * gi - pi.y * gr;
    }
    if (JN) jn[e] = -(il * mu[j] - il * mu[i]) - (dadt ? dadt[e] : 0.0);
}

template <bool JS, bool JN>
__global__ __launch_bounds__(BLOCK) void k_edge_currents(
    int64_t m, const int32_t *__restrict__ e0, const int32_t *__restrict__ e1,
    const double *__restrict__ inv_len, const double2 *__restrict__ U,
    const double2 *__restrict__ psi, const double *__restrict__ mu, double *__restrict__ js,
    double *__restrict__ jn, const double *__restrict__ dadt, int64_t e_base) {
    // edges [e_base, m): one-process-per-GPU mode computes the edges between owned sites while
    // the ghost values of mu travel, the cut edges after (edges touching a ghost are numbered last)
    edge_currents_body<JS, JN>(e_base + blockIdx.x * (int64_t)BLOCK + threadIdx.x, m, e0, e1, inv_len, U, psi, mu, js, jn, dadt);
}

// Launch-bound (small-mesh) time loop: the psi update of step n + 1 and the edge currents of step n in
// ONE launch.  Both read psi^{n+1}... of the accepted step (`psi`) and mu only, the currents feed nothing
// back into the time loop, and a step of the direct solve is five launches, so one launch less is ~8 %.
// Workgroups [0, nblk_psi) update psi, the others take 256 edges each.  Used only while the link
// variables are static (loop.inc: currents_plan, TDGL_CURRENTS_WITH_NEXT_PSI).
__global__ __launch_bounds__(BLOCK) void k_psi_update_with_currents(
    int nblk_psi, int64_t n, const double2 *__restrict__ psi, const double *__restrict__ mu,
    const double *__restrict__ eps, const double2 *__restrict__ lap, double dt, double u, double gamma,
    double2 *__restrict__ psi_new, double *__restrict__ dmax_part, int32_t *__restrict__ fail_part,
    int64_t m, const int32_t *__restrict__ e0, const int32_t *__restrict__ e1, const double *__restrict__ inv_len,
    const double2 *__restrict__ U, double *__restrict__ js, double *__restrict__ jn) {
    if ((int)blockIdx.x < nblk_psi)  // (workgroup-uniform)
        psi_update_body(blockIdx.x, nblk_psi, n, psi, mu, eps, lap, dt, u, gamma, psi_new, nullptr, dmax_part, fail_part,
                        nullptr);
    else
        edge_currents_body<true, true>((blockIdx.x - nblk_psi) * (int64_t)BLOCK + threadIdx.x, m, e0, e1, inv_len, U, psi,
                                       mu, js, jn, nullptr);
}

// ---- the moving applied field inside the run-ahead loop (run.inc; FieldDrive in tdgl_internal.h) ----------------------
// A factor such as LinearRamp(t) (tdgl/sources/scaling.py:4-14) evaluated on the device at the time the device's loop
// has reached; what TDGLSolver.update does before the psi update of a step (solver.py:626-642), once per STEP: the
// first attempt of a step moves the links, retries and dead attempts skip everything.  The arithmetic is the host's,
// operation for operation (no contraction), so that this loop and the one with one synchronisation per step agree
// to the last bit.
// tdgl/sources/scaling.py:4-14, branch for branch and operation for operation (`initial` before tmin, `final` from
// tmax on -- exactly, whatever the two values are --, Python's left-to-right product and quotient in between); host
// and device evaluate THIS, so the two time loops agree to the last bit and `FieldDrive::settled` can test equality
__host__ __device__ inline double linear_ramp_value(double t, double tmin, double tmax, double initial, double final_) {
#pragma clang fp contract(off)
    if (t < tmin) return initial;
    if (t < tmax) return initial + (final_ - initial) * (t - tmin) / (tmax - tmin);
    return final_;
}

// Value at time t of the piecewise-linear table (times[k], v[k]), n >= 1 nodes, constant outside the node range.  Like the
// ramp: host and device evaluate THIS, with no contraction into fused multiply-adds.
__host__ __device__ inline double table_value(const double *__restrict__ times, const double *__restrict__ v, int n, double t) {
#pragma clang fp contract(off)
    if (t <= times[0]) return v[0];
    if (t >= times[n - 1]) return v[n - 1];
    int lo = 0, hi = n - 1;  // first node with times[node] > t (std::upper_bound)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (times[mid] > t) hi = mid;
        else lo = mid;
    }
    const double t0 = times[hi - 1], t1 = times[hi];
    return v[hi - 1] + (v[hi] - v[hi - 1]) * ((t - t0) / (t1 - t0));
}

// L psi^n with the links of this step (the cached one belongs to the links of the previous step)
template <class IT>
__global__ __launch_bounds__(BLOCK) void k_psi_laplacian_ra_fresh(
    int n_slices, int per_xcd, int64_t n_rows, const int32_t *__restrict__ slice_off, const IT *__restrict__ cols,
    const double2 *__restrict__ vals, const double *__restrict__ diag, const uint8_t *__restrict__ fixed,
    const double2 *__restrict__ psi0, const double2 *__restrict__ psi1, double2 *__restrict__ lap0, double2 *__restrict__ lap1,
    const StepCtl *__restrict__ ctl) {
    if (!ctl->ramp_do) return;
    const bool c1 = ctl->cur != 0;
    psi_laplacian_body<false, IT>(n_slices, per_xcd, 0, n_rows, slice_off, cols, vals, diag, fixed, c1 ? psi1 : psi0,
                                  c1 ? lap1 : lap0, nullptr, nullptr, nullptr);
}

// the edge currents of psi^n the previous attempt owes, with the links and dA/dt they belong to (before the ramp moves on)
__global__ __launch_bounds__(BLOCK) void k_ra_edge_currents(int64_t m, const int32_t *__restrict__ e0, const int32_t *__restrict__ e1,
                                                            const double *__restrict__ inv_len, const double2 *__restrict__ U,
                                                            const double2 *__restrict__ psi0, const double2 *__restrict__ psi1,
                                                            const double *__restrict__ mu, double *__restrict__ js,
                                                            double *__restrict__ jn, const double *__restrict__ dadt,
                                                            const StepCtl *__restrict__ ctl) {
    if (ctl->poisoned) return;
    edge_currents_body<true, true>(blockIdx.x * (int64_t)BLOCK + threadIdx.x, m, e0, e1, inv_len, U, ctl->cur != 0 ? psi1 : psi0, mu,
                                   js, jn, dadt);
}

// The same launch in the run-ahead time loop (run.inc): dt (attempt_dt) and the buffer that holds psi^n
// (ctl->cur) live on the device; nothing runs once the loop is poisoned (end of the run reached, retry budget
// spent).  m == 0: no edge currents are owed.  An attempt that repeats a failed one forms the same currents again.
__global__ __launch_bounds__(BLOCK) void k_ra_psi_update(
    int nblk_psi, int64_t n, double2 *__restrict__ psi0, double2 *__restrict__ psi1, const double2 *__restrict__ lap0,
    const double2 *__restrict__ lap1, const double *__restrict__ mu, const double *__restrict__ eps, double u, double gamma,
    double *__restrict__ dmax_part, int32_t *__restrict__ fail_part, int64_t m, const int32_t *__restrict__ e0,
    const int32_t *__restrict__ e1, const double *__restrict__ inv_len, const double2 *__restrict__ U, double *__restrict__ js,
    double *__restrict__ jn, StepCtl *__restrict__ ctl) {
    if (ctl->poisoned) {  // (uniform over the launch: `poisoned` only changes in the controller, a different launch)
        if (blockIdx.x == 0 && threadIdx.x == 0) ctl->live = 0;
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->live = 1;
    const bool c1 = ctl->cur != 0;
    const double2 *__restrict__ psi = c1 ? psi1 : psi0;
    if ((int)blockIdx.x < nblk_psi)
        psi_update_body(blockIdx.x, nblk_psi, n, psi, mu, eps, c1 ? lap1 : lap0, ctl->attempt_dt, u, gamma, c1 ? psi0 : psi1,
                        nullptr, dmax_part, fail_part, nullptr);
    else
        edge_currents_body<true, true>((blockIdx.x - nblk_psi) * (int64_t)BLOCK + threadIdx.x, m, e0, e1, inv_len, U, psi,
                                       mu, js, jn, nullptr);
}

// probe read-outs of an ACCEPTED attempt into the slot of its step (run-ahead loop)
__global__ void k_ra_probes(int n_probe, const int32_t *__restrict__ sites, const double2 *__restrict__ psi0,
                            const double2 *__restrict__ psi1, const double *__restrict__ mu, double *__restrict__ ring,
                            int slot_base, const StepCtl *__restrict__ ctl) {
    if (!ctl->live || !ctl->last_ok) return;
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_probe) return;
    const int s = sites[k];
    const double2 *__restrict__ psi = ctl->cur != 0 ? psi1 : psi0;  // (the controller has flipped cur: psi^{n+1})
    double *__restrict__ out = ring + (size_t)(slot_base + ctl->n_acc - 1) * 2 * n_probe;
    out[k] = mu[s];
    out[n_probe + k] = atan2(psi[s].y, psi[s].x);
}

// (grad psi)_e = (U_e psi_j - psi_i) / l_e  -- psi_gradient @ psi (operators.py:87-117 with link
// variables, :340-344); complex, one edge per lane
__global__ __launch_bounds__(BLOCK) void k_edge_gradient(int64_t m, const int32_t *__restrict__ e0,
                                                         const int32_t *__restrict__ e1,
                                                         const double *__restrict__ inv_len,
                                                         const double2 *__restrict__ U,
                                                         const double2 *__restrict__ psi,
                                                         double2 *__restrict__ out) {
    const int64_t e = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (e >= m) return;
    const double2 pi = psi[e0[e]], pj = psi[e1[e]], ue = U[e];
    const double il = inv_len[e];
    out[e] = make_double2((ue.x * il) * pj.x - (ue.y * il) * pj.y - il * pi.x,
                          (ue.x * il) * pj.y + (ue.y * il) * pj.x - il * pi.y);
}

// mu_laplacian @ x (operators.py:120-185 with U = 1 and no fixed rows, :285): real SpMV on the
// site-graph SELL pattern, row i: sum_k (w_e / a_i) x_j + diag_i x_i
__global__ __launch_bounds__(BLOCK) void k_mu_laplacian(int n_slices, int64_t n_rows,
                                                        const int32_t *__restrict__ slice_off,
                                                        const int32_t *__restrict__ cols,
                                                        const double *__restrict__ slot_w,
                                                        const double *__restrict__ diag,
                                                        const double *__restrict__ x, double *__restrict__ y) {
    const int slice = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
    if (slice >= n_slices) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t row = (int64_t)slice * WAVE + lane;
    if (row >= n_rows) return;
    double acc = diag[row] * x[row];
    int64_t idx = (int64_t)slice_off[slice] * WAVE + lane;
    for (int k = slice_off[slice]; k < slice_off[slice + 1]; ++k, idx += WAVE) acc += slot_w[idx] * x[cols[idx]];
    y[row] = acc;
}

// c = mu_boundary_laplacian @ mu_boundary  (operators.py:188-230): every boundary site
// receives exactly two contributions, so the float atomics commute -> deterministic.
__global__ __launch_bounds__(BLOCK) void k_boundary_term(int64_t nb, const int32_t *__restrict__ s0,
                                                         const int32_t *__restrict__ s1,
                                                         const double *__restrict__ c0,
                                                         const double *__restrict__ c1,
                                                         const double *__restrict__ mu_b,
                                                         double *__restrict__ cvec) {
    int64_t k = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (k >= nb) return;
    const double v = mu_b[k];
    if (v != 0.0) {
        atomicAdd(&cvec[s0[k]], c0[k] * v);
        atomicAdd(&cvec[s1[k]], c1[k] * v);
    }
}

// ---- the moving applied field A(t) = A_0 + f_1(t) A_1 + ... + f_K(t) A_K + loops (FieldDrive; tdgl_set_link_exponents_base,
// tdgl_set_link_terms, tdgl_set_link_loops) ----------------------------------------------------------------------------------
// The step rule (FieldDrive::step on the host): the K factors and every loop's four values are evaluated at the controller's
// time with the evaluators above (linear_ramp_value, table_value); nothing moves only when EVERY value equals its last
// two evaluations and a dynamic update has run -- so a plateau inside a table skips the link launches as a finished ramp
// does.  `term`: the K = ctl->n_terms descriptors of THIS controller; a table term's nodes are times[off .. off + n),
// values[off .. off + n).  A factor the caller supplies (TERM_HOST) never comes here: the loop does not evaluate such a field.
// the K factors at time t into s[]; false when one of them differs from its last two evaluations
__device__ __forceinline__ bool terms_eval(const StepCtl *__restrict__ ctl, const FieldTerm *__restrict__ term,
                                           const double *__restrict__ times, const double *__restrict__ values, double t, double *s) {
#pragma clang fp contract(off)
    const int K = ctl->n_terms;
    bool same = true;
#pragma unroll
    for (int k = 0; k < FIELD_TERMS_MAX; ++k) {
        s[k] = 0.0;
        if (k >= K) continue;
        const FieldTerm d = term[k];
        s[k] = d.kind == TERM_TABLE ? table_value(times + d.off, values + d.off, d.n, t)
                                    : linear_ramp_value(t, d.ramp[0], d.ramp[1], d.ramp[2], d.ramp[3]);
        same = same && s[k] == ctl->term_scale[k] && s[k] == ctl->term_scale_prev[k];
    }
    return same;
}

// ... taken over as the factors of the current A
__device__ __forceinline__ void terms_take(StepCtl *__restrict__ ctl, const double *s) {
#pragma unroll
    for (int k = 0; k < FIELD_TERMS_MAX; ++k)
        if (k < ctl->n_terms) {
            ctl->term_scale_prev[k] = ctl->term_scale[k];
            ctl->term_scale[k] = s[k];
        }
}

// ---- moving current loops in that field (tdgl_set_link_loops) -------------------------------------------------------------
// A(t) = [A_0 + sum_k f_k(t) A_k] + sum_l I_l(t) Aloop(r_e - c_l(t); a_l): a circular loop of radius a in a plane parallel to
// the film, its centre and current piecewise linear in t.  Six numbers per step and one closed form per edge.
//
// The loop's potential without cancellation.  With rho the in-plane distance from the axis, z the height of the film above
// the loop's plane, d^2 = (a + rho)^2 + z^2 and m = 4 a rho / d^2, A_phi = I G with G = ((2 - m) K(m) - 2 E(m)) d / (4 pi rho)
// (I: the current with mu_0 and the units folded in).  That textbook form subtracts two numbers that agree to O(m^2) and
// has no correct digit below m ~ 1e-6.  Here
// (2 - m) K - 2 E = K sum_{n >= 1} 2^n c_n^2 with c_n the differences of the arithmetic-geometric mean: every term positive.
// b0 = sqrt(1 - m) is formed as sqrt(((a - rho)^2 + z^2) / d^2), never from 1 - m; c_0 / rho = 2 a / (d^2 (1 + b0)) is carried
// next to c_0, so H = G / rho needs no division by rho and A = I H (-dy, dx) is exactly zero on the axis.  LOOP_AGM_STEPS
// halvings reach double precision down to 1 - m = 2e-9 (z != 0 is the caller's to guarantee); a fixed count, every lane the
// same work: per loop and edge 3 + LOOP_AGM_STEPS square roots and 3 + LOOP_AGM_STEPS divisions in fp64.
constexpr int LOOP_AGM_STEPS = 6;
__device__ __forceinline__ void loop_potential_add(double ex, double ey, double cx, double cy, double z, double a, double cur, double &ax,
                                                   double &ay) {
#pragma clang fp contract(off)
    const double dx = ex - cx, dy = ey - cy;
    const double rho = sqrt(dx * dx + dy * dy);
    const double z2 = z * z, sp = a + rho, sm = a - rho;
    const double d2 = sp * sp + z2;
    const double b0 = sqrt((sm * sm + z2) / d2);
    const double ob = 1.0 + b0;
    double cr = (2.0 * a) / (d2 * ob);  // c / rho
    double c = cr * rho;
    double an = 0.5 * ob, bn = sqrt(b0), sr = 2.0 * (cr * cr), p = 4.0;  // sr = S / rho^2
#pragma unroll
    for (int n = 0; n < LOOP_AGM_STEPS; ++n) {
        const double a1 = 0.5 * (an + bn);
        bn = sqrt(an * bn);
        const double q = c / (4.0 * a1);
        cr = cr * q;
        c = c * q;
        sr = sr + p * (cr * cr);
        p = p * 2.0;
        an = a1;
    }
    const double h = cur * ((sr * sqrt(d2)) / (8.0 * an));
    double lx = -(dy * h), ly = dx * h;
    asm volatile("" : "+v"(lx), "+v"(ly));
    ax = ax + lx;
    ay = ay + ly;
}

// (body: one thread per controller)  loop[l]: nodes off .. off + n of the pools tab[0 .. T) (times), tab[T ..) centre x, then
// y, z and the current, T nodes each (read only when ctl->n_loops > 0).  Leaves has_dadt = 1 and ramp_do = 1 where the field
// moves, ramp_do = 0 on retries, dead attempts and where nothing moves.
__device__ __forceinline__ void field_begin_body(StepCtl *__restrict__ ctl, const FieldTerm *__restrict__ term,
                                                 const double *__restrict__ times, const double *__restrict__ values,
                                                 const FieldLoop *__restrict__ loop, const double *__restrict__ tab, int T) {
    int go = 0;
    if (!ctl->poisoned && ctl->retries == 0) {
        const double t = ctl->time;
        double s[FIELD_TERMS_MAX], lp[FIELD_LOOPS_MAX][4];
        bool same = terms_eval(ctl, term, times, values, t, s) && ctl->has_dadt != 0;
        const int L = ctl->n_loops;
#pragma unroll
        for (int l = 0; l < FIELD_LOOPS_MAX; ++l) {
            if (l >= L) continue;
            const FieldLoop d = loop[l];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lp[l][j] = table_value(tab + d.off, tab + (int64_t)(j + 1) * T + d.off, d.n, t);
                same = same && lp[l][j] == ctl->loop_par[l][j] && lp[l][j] == ctl->loop_par_prev[l][j];
            }
        }
        if (!same) {
            terms_take(ctl, s);
#pragma unroll
            for (int l = 0; l < FIELD_LOOPS_MAX; ++l)
                if (l < L) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        ctl->loop_par_prev[l][j] = ctl->loop_par[l][j];
                        ctl->loop_par[l][j] = lp[l][j];
                    }
                }
            ctl->has_dadt = 1;
            ctl->n_term_moves += 1;
            go = 1;
        }
    }
    ctl->ramp_do = go;
}

__global__ void k_ra_field_begin(StepCtl *__restrict__ ctl, const FieldTerm *__restrict__ term, const double *__restrict__ times,
                                 const double *__restrict__ values, const FieldLoop *__restrict__ loop, const double *__restrict__ tab,
                                 int T) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    field_begin_body(ctl, term, times, values, loop, tab, T);
}

// the values of a step, by value: the loop with one synchronisation per step evaluates them on the host (update_field) and
// hands them to the kernel the run-ahead loop feeds from its controller
struct FieldValues {
    double s[FIELD_TERMS_MAX];
    double lp[FIELD_LOOPS_MAX][4];  // centre x, y, z and current
    double inv_dt;
    int n_terms, pad;
};
// what does not move: the loops' radii, the film's height and how many there are
struct LoopGeom {
    double radius[FIELD_LOOPS_MAX];
    double z_film;
    int n_loops, pad;
};

// A = ((A_0 + s_1 A_1) + s_2 A_2) + ... per edge and component, terms added in term order, every product rounded before
// it is added (no contraction: the pragma, and the empty asm between a product and the sum or difference that takes it --
// __dmul_rn is a plain product to the compiler, which would contract it into the A - A_prev of dadt_body); without A_0
// (a0 == nullptr) the sum starts from the first product, without products it is A_0.  `bases`: slot k the (k + 1)-th
// base, `stride` double2 apart; a pure stream, 16 bytes per lane and array.
__device__ __forceinline__ void terms_sum(int64_t e, const FieldValues &fv, const double2 *__restrict__ bases, int64_t stride,
                                          const double2 *__restrict__ a0, double &ax, double &ay) {
#pragma clang fp contract(off)
    if (fv.n_terms == 0) {
        const double2 a = a0[e];
        ax = a.x, ay = a.y;
        return;
    }
    const double2 b1 = bases[e];
    ax = fv.s[0] * b1.x, ay = fv.s[0] * b1.y;
    asm volatile("" : "+v"(ax), "+v"(ay));
    if (a0) {
        const double2 a = a0[e];
        ax = a.x + ax;
        ay = a.y + ay;
    }
#pragma unroll
    for (int k = 1; k < FIELD_TERMS_MAX; ++k) {
        if (k >= fv.n_terms) break;
        const double2 b = bases[k * stride + e];
        double px = fv.s[k] * b.x, py = fv.s[k] * b.y;
        asm volatile("" : "+v"(px), "+v"(py));
        ax = ax + px;
        ay = ay + py;
    }
    asm volatile("" : "+v"(ax), "+v"(ay));
}

// One lane per edge: the sum of terms, the loops added in loop order (LOOPS; else the instantiation carries neither the
// registers of the arithmetic-geometric mean nor the centre's 16 bytes), A stored, then dA/dt along the edge with the previous
// accepted step's dt, A_prev <- A and "did it move" (dadt_body).  No LDS, no atomics.
template <bool LOOPS>
__device__ __forceinline__ int field_link_body(int64_t e, int64_t m, const FieldValues &fv, const LoopGeom &geom,
                                               const double2 *__restrict__ bases, int64_t stride, const double2 *__restrict__ a0,
                                               const double2 *__restrict__ centres, double *__restrict__ A, double *__restrict__ Aprev,
                                               const double *__restrict__ dx, const double *__restrict__ dy,
                                               const double *__restrict__ inv_len, double *__restrict__ dadt) {
    double ax, ay;
    terms_sum(e, fv, bases, stride, a0, ax, ay);
    if (LOOPS) {
        const double2 ce = centres[e];
#pragma unroll
        for (int l = 0; l < FIELD_LOOPS_MAX; ++l) {
            if (l >= geom.n_loops) break;
            loop_potential_add(ce.x, ce.y, fv.lp[l][0], fv.lp[l][1], geom.z_film - fv.lp[l][2], geom.radius[l], fv.lp[l][3], ax, ay);
        }
    }
    reinterpret_cast<double2 *>(A)[e] = make_double2(ax, ay);
    return dadt_body(e, m, fv.inv_dt, ax, ay, Aprev, dx, dy, inv_len, dadt);
}

// the values of this attempt from its controller
__device__ __forceinline__ FieldValues field_values_of(const StepCtl *__restrict__ c) {
    FieldValues fv;
#pragma unroll
    for (int k = 0; k < FIELD_TERMS_MAX; ++k) fv.s[k] = c->term_scale[k];
#pragma unroll
    for (int l = 0; l < FIELD_LOOPS_MAX; ++l)
#pragma unroll
        for (int j = 0; j < 4; ++j) fv.lp[l][j] = c->loop_par[l][j];
    fv.inv_dt = 1.0 / c->runner_dt;
    fv.n_terms = c->n_terms;
    fv.pad = 0;
    return fv;
}

// ... per workgroup: "did it move".  ctl: the run-ahead loop's controller, which says whether the attempt moves anything and
// with which values; nullptr: the host has decided, the values are `host`'s
template <bool LOOPS>
__global__ __launch_bounds__(BLOCK) void k_field_links(int64_t m, int64_t m_pad, FieldValues host, LoopGeom geom,
                                                       const double *__restrict__ bases, const double *__restrict__ a0,
                                                       const double *__restrict__ centres, double *__restrict__ A,
                                                       double *__restrict__ Aprev, const double *__restrict__ dx,
                                                       const double *__restrict__ dy, const double *__restrict__ inv_len,
                                                       double *__restrict__ dadt, int32_t *__restrict__ block_changed,
                                                       const StepCtl *__restrict__ ctl) {
    if (ctl && !ctl->ramp_do) return;
    const FieldValues fv = ctl ? field_values_of(ctl) : host;
    const int64_t e = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    const int changed = e < m ? field_link_body<LOOPS>(e, m, fv, geom, reinterpret_cast<const double2 *>(bases), m_pad,
                                                       reinterpret_cast<const double2 *>(a0), reinterpret_cast<const double2 *>(centres),
                                                       A, Aprev, dx, dy, inv_len, dadt)
                              : 0;
    const int any = __syncthreads_or(changed);
    if (threadIdx.x == 0) block_changed[blockIdx.x] = any;
}

// Run-ahead loop with tabulated terminal currents (update_mu_boundary, solver.py:325-345, at the time of the step
// about to be attempted -- which only the device knows): ONE workgroup evaluates the piecewise-linear tables at
// ctl->time, rewrites mu_boundary at the tabulated positions, and rebuilds c = mu_boundary_laplacian @ mu_boundary
// on the sites boundary edges touch (every such site receives exactly two contributions: the atomics commute) and
// ceff = c (no dA/dt term in this loop).  The same table_value as the host's, then the arithmetic of
// k_boundary_term + k_ceff, operation for operation: the run-ahead loop stays bit-identical to the loop with one synchronisation per step.
// (body: one whole workgroup)
__device__ __forceinline__ void mu_table_body(int nb, int n_sites, const int32_t *__restrict__ b_sites, const int32_t *__restrict__ s0,
                                              const int32_t *__restrict__ s1, const double *__restrict__ c0,
                                              const double *__restrict__ c1, double *__restrict__ mu_b, double *__restrict__ cvec,
                                              double *__restrict__ ceff, int n_nodes, const double *__restrict__ times,
                                              const double *__restrict__ dens, const int32_t *__restrict__ group, double time) {
#pragma clang fp contract(off)
    for (int k = threadIdx.x; k < nb; k += BLOCK) {
        const int g = group[k];
        if (g >= 0) mu_b[k] = table_value(times, dens + (int64_t)g * n_nodes, n_nodes, time);
    }
    for (int j = threadIdx.x; j < n_sites; j += BLOCK) cvec[b_sites[j]] = 0.0;
    __threadfence();
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += BLOCK) {
        const double v = mu_b[k];
        if (v != 0.0) {
            atomicAdd(&cvec[s0[k]], c0[k] * v);
            atomicAdd(&cvec[s1[k]], c1[k] * v);
        }
    }
    __threadfence();
    __syncthreads();
    for (int j = threadIdx.x; j < n_sites; j += BLOCK) {
        const int i = b_sites[j];
        ceff[i] = __hip_atomic_load(&cvec[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 0.0;
    }
}

__global__ __launch_bounds__(BLOCK) void k_ra_mu_table(int nb, int n_sites, const int32_t *__restrict__ b_sites,
                                                       const int32_t *__restrict__ s0, const int32_t *__restrict__ s1,
                                                       const double *__restrict__ c0, const double *__restrict__ c1,
                                                       double *__restrict__ mu_b, double *__restrict__ cvec,
                                                       double *__restrict__ ceff, int n_nodes,
                                                       const double *__restrict__ times, const double *__restrict__ dens,
                                                       const int32_t *__restrict__ group, const StepCtl *__restrict__ ctl) {
    mu_table_body(nb, n_sites, b_sites, s0, s1, c0, c1, mu_b, cvec, ceff, n_nodes, times, dens, group, ctl->time);
}

// ... and with a separable disorder parameter epsilon(r, t) = factor(t) * epsilon0(r) (update_epsilon,
// solver.py:364-381): the host's table_value + k_scale at the device's time.
__device__ __forceinline__ void eps_table_body(int64_t i, const double *__restrict__ eps0, double *__restrict__ eps, int n_nodes,
                                               const double *__restrict__ times, const double *__restrict__ factor, double time) {
#pragma clang fp contract(off)
    const double f = table_value(times, factor, n_nodes, time);
    eps[i] = f * eps0[i];
}

__global__ __launch_bounds__(BLOCK) void k_ra_eps_table(int64_t n, const double *__restrict__ eps0, double *__restrict__ eps,
                                                        int n_nodes, const double *__restrict__ times,
                                                        const double *__restrict__ factor, const StepCtl *__restrict__ ctl) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i >= n) return;
    eps_table_body(i, eps0, eps, n_nodes, times, factor, ctl->time);
}

// ---- Gaussian hot spots in epsilon (EpsSpots, tdgl_set_epsilon_spots) --------------------------------------------------------
// epsilon(r, t) = epsilon0(r) - sum_k a_k(t) exp(-|r - c_k(t)|^2 / (2 sigma_k(t)^2)), K <= EPS_SPOTS_MAX spots whose centre x, y,
// amplitude and width are piecewise-linear tables over the spot's own nodes.
// The four values of every spot at `time`: the host's step rule and every lane of the kernels evaluate THIS (table_value), so
// the values are the same bits wherever they are formed.  pool: the nodes' times, then cx, cy, a, sigma, tabs.T apart, from tabs.base
__host__ __device__ inline EpsSpotValues eps_spot_values_at(const EpsSpotTabs &tabs, const double *__restrict__ pool, double time) {
    EpsSpotValues sv{};
    sv.n = tabs.n;
    const double *p = pool + tabs.base;
    for (int k = 0; k < EPS_SPOTS_MAX; ++k) {
        if (k >= tabs.n) break;
        const int32_t off = tabs.off[k], nn = tabs.off[k + 1] - off;
        for (int j = 0; j < 4; ++j) sv.v[k][j] = table_value(p + off, p + (int64_t)(j + 1) * tabs.T + off, nn, time);
    }
    return sv;
}

// One lane per site, spots in spot order; every operation rounded on its own (no contraction: the pragma, and the empty asm
// between a product and the sum or difference that takes it), so that NumPy restates it operation for operation -- all but
// exp.  32 bytes per site: the coordinates as one double2, epsilon0 read, epsilon written.  (s*s is a normal number -- the
// setters check it --, so den > 0 and a site at a spot's centre gets g = exp(-0) = 1, never 0 / 0.)
__device__ __forceinline__ void eps_spots_body(int64_t i, const EpsSpotValues &sv, const double2 *__restrict__ xy,
                                               const double *__restrict__ eps0, double *__restrict__ eps) {
#pragma clang fp contract(off)
    const double2 r = xy[i];
    double acc = eps0[i];
#pragma unroll
    for (int k = 0; k < EPS_SPOTS_MAX; ++k) {
        if (k >= sv.n) break;
        const double dx = r.x - sv.v[k][0], dy = r.y - sv.v[k][1], s = sv.v[k][3];
        double xx = dx * dx, yy = dy * dy, ss = s * s;
        asm volatile("" : "+v"(xx), "+v"(yy), "+v"(ss));
        const double d2 = xx + yy, den = 2.0 * ss;
        const double g = exp(-(d2 / den));
        double p = sv.v[k][2] * g;
        asm volatile("" : "+v"(p));
        acc = acc - p;
    }
    eps[i] = acc;
}

// ctl: the run-ahead loop's controller -- every lane evaluates the tables at ctl->time, uniformly across the wavefront, and a
// poisoned attempt returns at once; nullptr: the host has decided, the values are `host`'s.  The first lane leaves the values it
// applied in `applied` (what tdgl_get_epsilon_spot_values reports after a batch the host did not see).
__global__ __launch_bounds__(BLOCK) void k_eps_spots(int64_t n, EpsSpotValues host, EpsSpotTabs tabs, const double *__restrict__ pool,
                                                     const double2 *__restrict__ xy, const double *__restrict__ eps0,
                                                     double *__restrict__ eps, EpsSpotValues *__restrict__ applied,
                                                     const StepCtl *__restrict__ ctl) {
    if (ctl && ctl->poisoned) return;
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i >= n) return;
    const EpsSpotValues sv = ctl ? eps_spot_values_at(tabs, pool, ctl->time) : host;
    if (i == 0 && applied) *applied = sv;
    eps_spots_body(i, sv, xy, eps0, eps);
}

__global__ void k_probes(int n_probe, const int32_t *__restrict__ sites,
                         const double2 *__restrict__ psi, const double *__restrict__ mu,
                         double *__restrict__ out) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_probe) return;
    const int s = sites[k];
    out[k] = mu[s];
    out[n_probe + k] = atan2(psi[s].y, psi[s].x);  // np.angle
}

// ------------------------------------------------------------------ Poisson: SELL SpMV family
// Level-0 PCG kernels run on a FIXED grid of at most NB workgroups (4 per CU) that stride over
// their work, and every dot product is written as NB per-workgroup partials.  A consumer kernel
// sums the NB partials itself (fixed order, identical in every workgroup), so no separate
// reduction launch and no floating-point atomics are needed and results are bit-reproducible.
constexpr int NB = 1024;

// The number of partials actually WRITTEN is a property of the context, npart <= NB: the number of
// 256-row tiles rounded up to a multiple of 8, capped at NB -- the grid of every kernel that produces
// them (a 5.8k-site mesh has 24 tiles: 1024 workgroups that mostly write zeros cost more than the
// work).  The arrays keep the stride NB and are zero beyond npart (allocated zeroed, never written
// there), so consumers simply sum all NB entries: NB / BLOCK independent loads per thread, one round
// trip whatever npart is.
//
// Sum of the NB partials, returned to every thread of the workgroup.
__device__ __forceinline__ double sum_partials(const double *__restrict__ part) {
    __shared__ double shp[BLOCK / WAVE];
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < NB / BLOCK; ++i) v += part[threadIdx.x + i * BLOCK];
    v = wave_sum(v);
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    __syncthreads();
    if (lane == 0) shp[w] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < BLOCK / WAVE; ++i) t += shp[i];
    return t;
}

// Up to three NB-entry partial arrays summed with ONE round trip and one pair of barriers (the
// loads of all arrays are in flight together); results valid in every thread.  Same fixed
// summation order per array as sum_partials.
__device__ __forceinline__ void sum_partials3(const double *__restrict__ a, const double *__restrict__ b,
                                              const double *__restrict__ c, double *sa, double *sb, double *sc) {
    __shared__ double shq[3][BLOCK / WAVE];
    double va = 0.0, vb = 0.0, vc = 0.0;
#pragma unroll
    for (int i = 0; i < NB / BLOCK; ++i) {
        va += a[threadIdx.x + i * BLOCK];
        if (b) vb += b[threadIdx.x + i * BLOCK];
        if (c) vc += c[threadIdx.x + i * BLOCK];
    }
    va = wave_sum(va);
    vb = wave_sum(vb);
    vc = wave_sum(vc);
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    __syncthreads();
    if (lane == 0) {
        shq[0][w] = va;
        shq[1][w] = vb;
        shq[2][w] = vc;
    }
    __syncthreads();
    double ta = 0.0, tb = 0.0, tc = 0.0;
#pragma unroll
    for (int i = 0; i < BLOCK / WAVE; ++i) {
        ta += shq[0][i];
        tb += shq[1][i];
        tc += shq[2][i];
    }
    *sa = ta;
    *sb = tb;
    *sc = tc;
}

// ---- the CG update x += alpha p, r -= alpha q ----------------------------------------------------
// alpha = (r.z)/(p.q) from the partial arrays.  The host launches iterations in batches without
// looking at the residual in between.  Once the residual of the PREVIOUS iteration (part_rr_in,
// complete because it was written by an earlier launch) is below tol2 the update freezes
// (alpha = 0): iterating CG past convergence divides round-off by round-off and destroys the
// solution.  Every kernel that needs alpha computes it with this function from the same arrays in
// the same order, so they all get the same bits.
// (struct XrArgs: tdgl_internal.h)
__device__ __forceinline__ double cg_alpha(const XrArgs &a, bool *converged, double *rr_prev) {
    double rz, pq;
    sum_partials3(a.part_rz, a.part_pq, a.part_rr_in, &rz, &pq, rr_prev);
    *converged = *rr_prev <= a.scal[S_TOL2];
    return (*converged || !(pq > 0.0)) ? 0.0 : rz / pq;
}

// x += alpha p ; r -= alpha q ; part_rr_out[vblock] = sum r^2 over the rows of virtual workgroup
// `vblock` of NB.  The first frozen iteration records its index so the host learns how many
// iterations were really needed.  (vblock: the update can ride in another kernel's launch, see
// k_csr_down / k_dense_rows.)
__device__ __forceinline__ void xr_update_body(int vblock, const XrArgs &a) {
    // The operands of the first grid-stride iteration do not depend on alpha: request them BEFORE the
    // partial sums (two barriers and a dependent round trip), so that the stream is already in
    // flight while alpha is being formed.
    const int64_t n_pairs = a.n / 2;
    const int64_t i0 = vblock * (int64_t)BLOCK + threadIdx.x;
    const bool have0 = i0 < n_pairs;
    double2 pv0 = make_double2(0.0, 0.0), qv0 = pv0, xv0 = pv0, rv0 = pv0;
    if (have0) {
        pv0 = reinterpret_cast<const double2 *>(a.p)[i0];
        qv0 = reinterpret_cast<const double2 *>(a.q)[i0];
        xv0 = reinterpret_cast<const double2 *>(a.x)[i0];
        rv0 = reinterpret_cast<const double2 *>(a.r)[i0];
    }
    bool converged;
    double rr_prev;
    const double alpha = cg_alpha(a, &converged, &rr_prev);
    if (vblock == 0 && threadIdx.x == 0) {  // iteration counter / first frozen iteration
        const double it = a.scal[S_IT];
        if (converged && a.scal[S_CONV_IT] < 0.0) a.scal[S_CONV_IT] = it;
        if (it == 0.0) a.scal[S_RR0] = rr_prev;
        a.scal[S_IT] = it + 1.0;
        a.scal[S_ALPHA] = alpha;
    }
    double rr = 0.0, sx = 0.0;
    // 16-byte accesses: two rows per lane; an odd last row is done by one thread
    const int64_t n = a.n, n2 = n / 2;
    const double2 *__restrict__ p2 = reinterpret_cast<const double2 *>(a.p);
    const double2 *__restrict__ q2 = reinterpret_cast<const double2 *>(a.q);
    double2 *__restrict__ x2 = reinterpret_cast<double2 *>(a.x);
    double2 *__restrict__ r2 = reinterpret_cast<double2 *>(a.r);
    if (have0) {
        xv0.x += alpha * pv0.x;
        xv0.y += alpha * pv0.y;
        rv0.x -= alpha * qv0.x;
        rv0.y -= alpha * qv0.y;
        x2[i0] = xv0;
        r2[i0] = rv0;
        rr += rv0.x * rv0.x + rv0.y * rv0.y;
        sx += xv0.x + xv0.y;
    }
    for (int64_t i = i0 + (int64_t)a.npart * BLOCK; i < n2; i += (int64_t)a.npart * BLOCK) {
        const double2 pv = p2[i], qv = q2[i];
        double2 xv = x2[i], rv = r2[i];
        xv.x += alpha * pv.x;
        xv.y += alpha * pv.y;
        rv.x -= alpha * qv.x;
        rv.y -= alpha * qv.y;
        x2[i] = xv;
        r2[i] = rv;
        rr += rv.x * rv.x + rv.y * rv.y;
        sx += xv.x + xv.y;
    }
    if ((n & 1) && vblock == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        const double xi = a.x[i] + alpha * a.p[i];
        a.x[i] = xi;
        const double ri = a.r[i] - alpha * a.q[i];
        a.r[i] = ri;
        rr += ri * ri;
        sx += xi;
    }
    // both sums through one pass over LDS (same fixed order as block_sum)
    __shared__ double shx[2][BLOCK / WAVE];
    rr = wave_sum(rr);
    sx = wave_sum(sx);
    __syncthreads();
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        shx[0][threadIdx.x / WAVE] = rr;
        shx[1][threadIdx.x / WAVE] = sx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0, u = 0.0;
#pragma unroll
        for (int i = 0; i < BLOCK / WAVE; ++i) {
            t += shx[0][i];
            u += shx[1][i];
        }
        a.part_rr_out[vblock] = t;
        if (a.part_sx) a.part_sx[vblock] = u;
    }
}

__global__ __launch_bounds__(BLOCK) void k_update_xr(XrArgs a) { xr_update_body(blockIdx.x, a); }

enum SpmvMode { AX = 0, RESID = 1, SMOOTH = 2, RESID0 = 3 };
// DOT_BY2: b.y into partial[0, NB) and b2.y into partial[2 NB, 3 NB) (the flexible CG's z.q next to r.z)
// DOT_BX_XY: b.x into partial[0, NB) and x.y into partial[2 NB, 3 NB) (one-process-per-GPU mode with two distributed
//   levels: r.z and z.w from the pass that forms w = A z over the OWNED rows -- the smoothing pass before it also
//   forms z on ghost rows, which must not enter a sum)
enum DotMode { DOT_NONE = 0, DOT_XY = 1, DOT_BY = 2, DOT_YY = 3, DOT_BY2 = 4, DOT_BX_XY = 5 };

// y = A x                                             (AX)
// y = (b - c1) - A x                                  (RESID)
// d = c1 d + c2 dinv (b - A x);  y = x + d            (SMOOTH: damped Jacobi when c1 = 0 and
//                                                      d == nullptr, else one Chebyshev step)
// y = x - c2 A (dinv * x)                            (RESID0: residual of the right-hand side x
//                                                      after ONE smoothing step x1 = c2 dinv x
//                                                      from a zero guess, without storing x1)
// optionally with per-workgroup partials of x.y, b.y or y.y.
// Grid: `grid` workgroups (a multiple of 8); workgroup g serves XCD g % 8 and walks the tiles
// [xcd * per_xcd, (xcd + 1) * per_xcd) with stride grid / 8.
// VT / XT / YT: storage types of the matrix values (and dinv), of the gathered vector and of the
// result.  The mixed-precision preconditioner (fp32 V-cycle operators on level 0 inside the fp64
// CG) instantiates them with float; all arithmetic is fp64 either way.
template <int MODE, int DOT, class IT, class VT = double, class XT = double, class YT = double, class DT = VT>
__global__ __launch_bounds__(BLOCK) void k_sell_spmv(
    int n_slices, int per_xcd, int tile_base, int64_t n_rows, const int32_t *__restrict__ slice_off,
    const IT *__restrict__ cols, const VT *__restrict__ vals,
    const XT *__restrict__ x, const double *__restrict__ b, const DT *__restrict__ dinv,
    double c1, double c2, double *__restrict__ d, YT *__restrict__ y,
    double *__restrict__ partial, const double *__restrict__ b2 = nullptr) {
    const int xcd = blockIdx.x % XCDS, local = blockIdx.x / XCDS, stride = gridDim.x / XCDS;
    const int lane = threadIdx.x & (WAVE - 1);
    double dot = 0.0, dot2 = 0.0;
    for (int t = local; t < per_xcd; t += stride) {
        const int slice =
            __builtin_amdgcn_readfirstlane((tile_base + xcd * per_xcd + t) * (BLOCK / WAVE) + (threadIdx.x / WAVE));
        if (slice >= n_slices) continue;
        const int64_t row = (int64_t)slice * WAVE + lane;
        // lanes past the last row own nothing: in distributed mode those vector entries are
        // ghost sites with live data, so they must neither be written nor enter a dot product
        if (row >= n_rows) continue;
        const int beg = slice_off[slice], cnt = slice_off[slice + 1] - beg;
        // row-indexed operands are requested up front, together with the first batch
        constexpr bool NEED_X = (MODE == RESID0 || MODE == SMOOTH || DOT == DOT_XY || DOT == DOT_BX_XY);
        constexpr bool NEED_B = (MODE == RESID || MODE == SMOOTH || DOT == DOT_BY || DOT == DOT_BY2 || DOT == DOT_BX_XY);
        const double xr = NEED_X ? (double)x[row] : 0.0;
        const double br = NEED_B ? b[row] : 0.0;
        const double b2r = (DOT == DOT_BY2) ? b2[row] : 0.0;
        const double dr = (MODE == SMOOTH) ? (double)dinv[row] : 0.0;
        const double dold = (MODE == SMOOTH && d) ? d[row] : 0.0;
        double acc = 0.0;
        const int64_t idx0 = (int64_t)beg * WAVE + lane;
        // batched requests as in k_psi_laplacian: indices + values, then the gathers
        for (int base = 0; base < cnt; base += SELL_BATCH) {
            int c[SELL_BATCH];
            VT v[SELL_BATCH];
#pragma unroll
            for (int k = 0; k < SELL_BATCH; ++k) {
                const int kk = min(base + k, cnt - 1);
                c[k] = col_at<IT>(cols, idx0 + (int64_t)kk * WAVE, row);
                v[k] = vals[idx0 + (int64_t)kk * WAVE];
            }
            double g[SELL_BATCH];
#pragma unroll
            for (int k = 0; k < SELL_BATCH; ++k)
                g[k] = (MODE == RESID0) ? (double)dinv[c[k]] * (double)x[c[k]] : (double)x[c[k]];
#pragma unroll
            for (int k = 0; k < SELL_BATCH; ++k) acc += ((base + k < cnt) ? (double)v[k] : 0.0) * g[k];
        }
        double out;
        if (MODE == AX) {
            out = acc;
        } else if (MODE == RESID0) {
            out = xr - c2 * acc;
        } else if (MODE == RESID) {
            out = (br - c1) - acc;  // (c1: mean of b still to be removed, else 0)
        } else {
            double inc = c2 * dr * (br - acc);
            if (d) {
                inc += c1 * dold;
                d[row] = inc;
            }
            out = xr + inc;
        }
        y[row] = (YT)out;
        // (sums with y use the STORED value: with an fp32 y the CG's r.z must belong to the z it goes on with --
        // the unrounded one is a different vector at the 6e-8 level, which costs iterations near convergence)
        const double outs = (double)(YT)out;
        if (DOT == DOT_XY) dot += xr * out;
        if (DOT == DOT_BY || DOT == DOT_BY2) dot += br * outs;
        if (DOT == DOT_BY2) dot2 += b2r * outs;
        if (DOT == DOT_BX_XY) {
            dot += br * xr;
            dot2 += xr * out;
        }
        if (DOT == DOT_YY) dot += out * out;
    }
    if (DOT != DOT_NONE) {
        const double s = block_sum(dot);
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
    }
    if (DOT == DOT_BY2 || DOT == DOT_BX_XY) {
        const double s2 = block_sum(dot2);
        if (threadIdx.x == 0) partial[2 * NB + blockIdx.x] = s2;
    }
}

// CG direction update fused into the operator application (single GPU):
//   beta = (r.z) / (r.z)_previous  (0 when part_rz_old == nullptr, the first iteration), or, with
//   part_zq given (flexible CG): beta = z_new.(r_new - r_old) / (r.z)_previous = -alpha (z_new.q) /
//   (r.z)_previous, since r_new - r_old = -alpha q exactly (alpha of the last update: scal[S_ALPHA])
//   p_new = z + beta p_old   (written for the row; gathered on the fly for the columns)
//   q = A p_new,  partial[block] = sum p_new q
// p is double-buffered by the caller: other rows gather p_old while this row's p_new is written.
// Saves the separate direction-update pass (24 bytes per row and one launch per iteration).
// RZ (the first iteration of a run with the factors, whose application leaves z and no sums): r . z is formed here as
// well, from the z[row] the pass reads anyway -- part_rz_out[block], the slots and the fixed order k_update_xr expects.
template <class ZT, class IT, bool RZ = false>
__global__ __launch_bounds__(BLOCK) void k_sell_axp(
    int n_slices, int per_xcd, int64_t n_rows, const int32_t *__restrict__ slice_off,
    const IT *__restrict__ cols, const double *__restrict__ vals, const ZT *__restrict__ z,
    const double *__restrict__ p_old, const double *__restrict__ part_rz_new,
    const double *__restrict__ part_rz_old, double *__restrict__ p_new, double *__restrict__ q,
    double *__restrict__ partial, const double *__restrict__ part_zq, const double *__restrict__ scal,
    const double *__restrict__ r, double *__restrict__ part_rz_out) {
    const int xcd = blockIdx.x % XCDS, local = blockIdx.x / XCDS, stride = gridDim.x / XCDS;
    const int lane = threadIdx.x & (WAVE - 1);
    double beta = 0.0;
    if (part_rz_old) {
        double num, den, unused;
        sum_partials3(part_zq ? part_zq : part_rz_new, part_rz_old, nullptr, &num, &den, &unused);
        beta = part_zq ? -scal[S_ALPHA] * num / den : num / den;
    }
    double dot = 0.0;
    [[maybe_unused]] double rz = 0.0;
    for (int t = local; t < per_xcd; t += stride) {
        const int slice = __builtin_amdgcn_readfirstlane((xcd * per_xcd + t) * (BLOCK / WAVE) + (threadIdx.x / WAVE));
        if (slice >= n_slices) continue;
        const int64_t row = (int64_t)slice * WAVE + lane;
        if (row >= n_rows) continue;
        const int beg = slice_off[slice], cnt = slice_off[slice + 1] - beg;
        const double zr = (double)z[row], pr = part_rz_old ? p_old[row] : 0.0;
        const double pn = zr + beta * pr;
        if constexpr (RZ) rz += r[row] * zr;
        double acc = 0.0;
        const int64_t idx0 = (int64_t)beg * WAVE + lane;
        for (int base = 0; base < cnt; base += SELL_BATCH) {
            int c[SELL_BATCH];
            double v[SELL_BATCH], gz[SELL_BATCH], gp[SELL_BATCH];
#pragma unroll
            for (int k = 0; k < SELL_BATCH; ++k) {
                const int kk = min(base + k, cnt - 1);
                c[k] = col_at<IT>(cols, idx0 + (int64_t)kk * WAVE, row);
                v[k] = vals[idx0 + (int64_t)kk * WAVE];
            }
#pragma unroll
            for (int k = 0; k < SELL_BATCH; ++k) {
                gz[k] = (double)z[c[k]];
                gp[k] = part_rz_old ? p_old[c[k]] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < SELL_BATCH; ++k) acc += ((base + k < cnt) ? v[k] : 0.0) * (gz[k] + beta * gp[k]);
        }
        p_new[row] = pn;
        q[row] = acc;
        dot += pn * acc;
    }
    const double s = block_sum(dot);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
    if constexpr (RZ) {
        const double srz = block_sum(rz);
        if (threadIdx.x == 0) part_rz_out[blockIdx.x] = srz;
    }
}

// Row-per-lane SELL SpMV for the level-0 prolongation: y = A x (T_SET), y += A x (T_ADD) or
// y = c dinv b + A x (T_BASE: adds the coarse correction to the one-step pre-smoothed iterate
// c dinv b, which is recomputed here instead of having been stored).
enum TransferMode { T_SET = 0, T_ADD = 1, T_BASE = 2 };

// IT = uint16_t: `cols` holds offsets from slice_base[slice] (SellPattern::offs16).
template <int TMODE, class VT = double, class YT = double, class IT = int32_t, class DT = VT>
__global__ __launch_bounds__(BLOCK) void k_sell_transfer(int n_slices, int per_xcd, int64_t n_rows,
                                                         const int32_t *__restrict__ slice_off,
                                                         const IT *__restrict__ cols,
                                                         const int32_t *__restrict__ slice_base,
                                                         const VT *__restrict__ vals,
                                                         const double *__restrict__ x,
                                                         const DT *__restrict__ dinv,
                                                         const double *__restrict__ b, double c,
                                                         YT *__restrict__ y) {
    const int xcd = blockIdx.x % XCDS, local = blockIdx.x / XCDS, stride = gridDim.x / XCDS;
    const int lane = threadIdx.x & (WAVE - 1);
    for (int t = local; t < per_xcd; t += stride) {
        const int slice = __builtin_amdgcn_readfirstlane((xcd * per_xcd + t) * (BLOCK / WAVE) + (threadIdx.x / WAVE));
        if (slice >= n_slices) continue;
        const int64_t row = (int64_t)slice * WAVE + lane;
        if (row >= n_rows) continue;
        const int beg = slice_off[slice], cnt = slice_off[slice + 1] - beg;
        const int sb = sizeof(IT) == 2 ? slice_base[slice] : 0;
        const double base_val =
            (TMODE == T_BASE) ? c * (double)dinv[row] * b[row] : (TMODE == T_ADD ? (double)y[row] : 0.0);
        double acc = 0.0;
        const int64_t idx0 = (int64_t)beg * WAVE + lane;
        // batched requests (k_psi_laplacian): a prolongation row has 1-4 entries
        constexpr int TB = 4;
        for (int base = 0; base < cnt; base += TB) {
            int cc[TB];
            VT v[TB];
#pragma unroll
            for (int k = 0; k < TB; ++k) {
                const int kk = min(base + k, cnt - 1);
                cc[k] = sb + (int)cols[idx0 + (int64_t)kk * WAVE];
                v[k] = vals[idx0 + (int64_t)kk * WAVE];
            }
            double g[TB];
#pragma unroll
            for (int k = 0; k < TB; ++k) g[k] = x[cc[k]];
#pragma unroll
            for (int k = 0; k < TB; ++k) acc += ((base + k < cnt) ? (double)v[k] : 0.0) * g[k];
        }
        y[row] = (YT)(base_val + acc);
    }
}

// CSR operator with LANES lanes per row (coarse levels, restriction, coarse prolongation):
//   C_AX: y = A x | C_RESID: y = b - A x | C_SMOOTH: d = c1 d + c2 dinv (b - A x), y = x + d
//   C_ADD: y += A x
//   C_PRE2: the first TWO smoothing steps from a zero guess in one pass (x = b holds the
//           right-hand side): d0 = c0 dinv b, d = c1 d0 + c2 dinv (b - A d0), y = d0 + d
enum CsrOp { C_AX = 0, C_RESID = 1, C_SMOOTH = 2, C_ADD = 3, C_PRE2 = 4 };

// B = entries per lane requested together (indices + values, then the gathers): LANES * B should
// cover a typical row so that a row costs three dependent round trips (indptr, entries, gathers);
// these kernels are latency bound, not bandwidth bound.  Entries past the row end re-read the
// last one with the value forced to 0.
template <int LANES, int OP, int B, class VT>
__device__ __forceinline__ void csr_multi_body(int vblock, int vgrid, int64_t n_rows, const int32_t *__restrict__ indptr,
                                                     const int32_t *__restrict__ indices,
                                                     const VT *__restrict__ data,
                                                     const double *__restrict__ x,
                                                     const double *__restrict__ b,
                                                     const double *__restrict__ dinv, double c0, double c1,
                                                     double c2, double *__restrict__ d, double *__restrict__ y) {
    // XCD-aware: consecutive row blocks stay on one XCD (the grid is a multiple of 8), so the
    // gathered vector entries shared by neighbouring rows are fetched into ONE L2, not eight
    // (vblock / vgrid: position in a virtual grid -- several operators can share one launch, k_csr_down)
    const int64_t gid = xcd_tile(vblock, vgrid / XCDS) * (int64_t)BLOCK + threadIdx.x;
    const int64_t row = gid / LANES;
    const int sub = (int)(gid % LANES);
    const bool lead = row < n_rows && sub == 0;
    double acc = 0.0;
    // the row's own operands (lane 0 of the row) travel with the entries
    double xr = 0.0, br = 0.0, dr = 0.0, dold = 0.0, yold = 0.0;
    if (lead) {
        if (OP == C_PRE2 || OP == C_SMOOTH) xr = x[row];
        if (OP == C_RESID || OP == C_SMOOTH) br = b[row];
        if (OP == C_PRE2 || OP == C_SMOOTH) dr = dinv[row];
        if (OP == C_SMOOTH && d) dold = d[row];
        if (OP == C_ADD) yold = y[row];
    }
    if (row < n_rows) {
        const int beg = indptr[row], end = indptr[row + 1];
        for (int base = beg + sub; base < end; base += LANES * B) {
            int c[B];
            double v[B], g[B];
#pragma unroll
            for (int k = 0; k < B; ++k) {
                const int kk = min(base + k * LANES, end - 1);
                c[k] = indices[kk];
                v[k] = (double)data[kk];
            }
#pragma unroll
            for (int k = 0; k < B; ++k) g[k] = (OP == C_PRE2) ? dinv[c[k]] * x[c[k]] : x[c[k]];
#pragma unroll
            for (int k = 0; k < B; ++k) acc += ((base + k * LANES < end) ? v[k] : 0.0) * g[k];
        }
    }
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, LANES);
    if (lead) {
        if (OP == C_AX) {
            y[row] = acc;
        } else if (OP == C_ADD) {
            y[row] = yold + acc;
        } else if (OP == C_RESID) {
            y[row] = br - acc;
        } else if (OP == C_PRE2) {
            const double d0 = c0 * dr * xr;
            const double d1 = c1 * d0 + c2 * dr * (xr - c0 * acc);
            d[row] = d1;
            y[row] = d0 + d1;
        } else {
            double inc = c2 * dr * (br - acc);
            if (d) {
                inc += c1 * dold;
                d[row] = inc;
            }
            y[row] = xr + inc;
        }
    }
}

template <int LANES, int OP, int B, class VT = double>
__global__ __launch_bounds__(BLOCK) void k_csr_multi(int64_t n_rows, const int32_t *__restrict__ indptr,
                                                     const int32_t *__restrict__ indices,
                                                     const VT *__restrict__ data,
                                                     const double *__restrict__ x,
                                                     const double *__restrict__ b,
                                                     const double *__restrict__ dinv, double c0, double c1,
                                                     double c2, double *__restrict__ d, double *__restrict__ y) {
    csr_multi_body<LANES, OP, B, VT>(blockIdx.x, gridDim.x, n_rows, indptr, indices, data, x, b, dinv, c0, c1, c2, d, y);
}

// y = M x for a CSR operator whose column indices are stored as 16-bit offsets from a per-row base
// (the level-0 fused restriction: with RCM numbering the fine sites a coarse row touches lie within
// a few thousand indices of each other -- 2 bytes less per entry on a 46 MB stream).  Same lane /
// batch scheme as csr_multi_body.
template <int LANES, int B, class VT>
__global__ __launch_bounds__(BLOCK) void k_csr_ax16(int64_t n_rows, const int32_t *__restrict__ indptr,
                                                    const int32_t *__restrict__ rowbase,
                                                    const uint16_t *__restrict__ offs, const VT *__restrict__ data,
                                                    const double *__restrict__ x, double *__restrict__ y) {
    const int64_t gid = xcd_tile(blockIdx.x, gridDim.x / XCDS) * (int64_t)BLOCK + threadIdx.x;
    const int64_t row = gid / LANES;
    const int sub = (int)(gid % LANES);
    double acc = 0.0;
    if (row < n_rows) {
        const int beg = indptr[row], end = indptr[row + 1], rb = rowbase[row];
        for (int base = beg + sub; base < end; base += LANES * B) {
            int c[B];
            double v[B], g[B];
#pragma unroll
            for (int k = 0; k < B; ++k) {
                const int kk = min(base + k * LANES, end - 1);
                c[k] = rb + (int)offs[kk];
                v[k] = (double)data[kk];
            }
#pragma unroll
            for (int k = 0; k < B; ++k) g[k] = x[c[k]];
#pragma unroll
            for (int k = 0; k < B; ++k) acc += ((base + k * LANES < end) ? v[k] : 0.0) * g[k];
        }
    }
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, LANES);
    if (row < n_rows && sub == 0) y[row] = acc;
}

// The way up on an intermediate level of the collapsed chain in ONE launch: y = W b - Vn e with the
// explicit W = T_x S + T_b (columns as 16-bit offsets from a per-row base: the level's numbering
// follows the fine one, a row reaches a few hundred indices) and Vn = -T_x P (columns of the next
// level, fewer than 65536 rows: plain 16-bit indices).  Values in VT (binary16 / fp32).
template <int LANES, int B1, int B2, class VT>
__global__ __launch_bounds__(BLOCK) void k_mid_up(int64_t n_rows, const int32_t *__restrict__ wp,
                                                  const int32_t *__restrict__ wbase, const uint16_t *__restrict__ woff,
                                                  const VT *__restrict__ wv, const double *__restrict__ b,
                                                  const int32_t *__restrict__ vp, const uint16_t *__restrict__ vi,
                                                  const VT *__restrict__ vv, const double *__restrict__ e,
                                                  double *__restrict__ y) {
    const int64_t gid = xcd_tile(blockIdx.x, gridDim.x / XCDS) * (int64_t)BLOCK + threadIdx.x;
    const int64_t row = gid / LANES;
    const int sub = (int)(gid % LANES);
    double acc = 0.0;
    if (row < n_rows) {
        const int beg1 = wp[row], end1 = wp[row + 1], rb = wbase[row], beg2 = vp[row], end2 = vp[row + 1];
        // the (short) V part is requested first: its gathers hit a 40 KB vector
        for (int base = beg2 + sub; base < end2; base += LANES * B2) {
            int c[B2];
            double v[B2], g[B2];
#pragma unroll
            for (int k = 0; k < B2; ++k) {
                const int kk = min(base + k * LANES, end2 - 1);
                c[k] = (int)vi[kk];
                v[k] = (double)vv[kk];
            }
#pragma unroll
            for (int k = 0; k < B2; ++k) g[k] = e[c[k]];
#pragma unroll
            for (int k = 0; k < B2; ++k) acc -= ((base + k * LANES < end2) ? v[k] : 0.0) * g[k];
        }
        for (int base = beg1 + sub; base < end1; base += LANES * B1) {
            int c[B1];
            double v[B1], g[B1];
#pragma unroll
            for (int k = 0; k < B1; ++k) {
                const int kk = min(base + k * LANES, end1 - 1);
                c[k] = rb + (int)woff[kk];
                v[k] = (double)wv[kk];
            }
#pragma unroll
            for (int k = 0; k < B1; ++k) g[k] = b[c[k]];
#pragma unroll
            for (int k = 0; k < B1; ++k) acc += ((base + k * LANES < end1) ? v[k] : 0.0) * g[k];
        }
    }
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, LANES);
    if (row < n_rows && sub == 0) y[row] = acc;
}

// The way down on an intermediate level in ONE launch (collapsed coarse chain, tdgl_amd/amg.py
// collapsed_operators): the first nbM workgroups form the next level's right-hand side
// y2 = M b with the explicit M = R (I - A S), the others the fused two-step pre-smoothing x = S b.
// Neither waits for the other; the critical path (y2) gets the lowest block ids.
template <int LM, int BM, class VT>
__global__ __launch_bounds__(BLOCK) void k_csr_down(int nbM, int64_t nM, const int32_t *__restrict__ Mp,
                                                    const int32_t *__restrict__ Mi, const VT *__restrict__ Mv,
                                                    const double *__restrict__ b, double *__restrict__ y2, int64_t nA,
                                                    const int32_t *__restrict__ Ap, const int32_t *__restrict__ Ai,
                                                    const VT *__restrict__ Av, const double *__restrict__ dinv,
                                                    double c0, double c1, double c2, double *__restrict__ d,
                                                    double *__restrict__ x) {
    if ((int)blockIdx.x < nbM)
        csr_multi_body<LM, C_AX, BM, VT>(blockIdx.x, nbM, nM, Mp, Mi, Mv, b, nullptr, nullptr, 0.0, 0.0, 0.0, nullptr, y2);
    else
        csr_multi_body<4, C_PRE2, 4, VT>(blockIdx.x - nbM, gridDim.x - nbM, nA, Ap, Ai, Av, b, nullptr, dinv, c0, c1, c2,
                                        d, x);
}

// 16-byte vectors of the storage type (4 floats / 2 doubles) and the matching slice of a double vector
template <class VT> struct Vec16;
template <> struct Vec16<float> {
    typedef float4 type;
    static constexpr int W = 4;
    static __device__ __forceinline__ double dot(const float4 g, const double *__restrict__ x) {
        const double2 a = *reinterpret_cast<const double2 *>(x), b = *reinterpret_cast<const double2 *>(x + 2);
        return (double)g.x * a.x + (double)g.y * a.y + (double)g.z * b.x + (double)g.w * b.y;
    }
};
template <> struct Vec16<double> {
    typedef double2 type;
    static constexpr int W = 2;
    static __device__ __forceinline__ double dot(const double2 g, const double *__restrict__ x) {
        const double2 a = *reinterpret_cast<const double2 *>(x);
        return g.x * a.x + g.y * a.y;
    }
};

// y = G x with a dense row-major G [gridDim.x rows, ld] (ld = the column count rounded up to a
// 16-byte multiple, zero padded; x padded alike): one workgroup per row, 16-byte loads, every
// load of a thread independent of the others (the tail of the collapsed coarse chain: a few hundred
// rows of a few thousand entries -- every CU gets a row or two, no index stream, one round trip).
template <class VT>
__device__ __forceinline__ void dense_row_body(int row, int ld, const VT *__restrict__ G, const double *__restrict__ x,
                                               double *__restrict__ y) {
    typedef typename Vec16<VT>::type V;
    constexpr int W = Vec16<VT>::W;
    const V *__restrict__ g = reinterpret_cast<const V *>(G + (int64_t)row * ld);
    const int nv = ld / W;
    double acc = 0.0;
    constexpr int U = 8;  // vectors requested per thread before the first use
    for (int base = threadIdx.x; base < nv; base += BLOCK * U) {
        V v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int c = min(base + k * BLOCK, nv - 1);
            v[k] = g[c];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int c = base + k * BLOCK;
            if (c < nv) acc += Vec16<VT>::dot(v[k], x + (int64_t)c * W);
        }
    }
    const double t = block_sum(acc);
    if (threadIdx.x == 0) y[row] = t;
}

template <class VT>
__global__ __launch_bounds__(BLOCK) void k_dense_rows(int ld, const VT *__restrict__ G, const double *__restrict__ x,
                                                      double *__restrict__ y) {
    dense_row_body<VT>(blockIdx.x, ld, G, x, y);
}

// The mu solve of a SMALL mesh: mu = G b with G = pinv(A) dense, fp64 (tdgl_poisson_set_dense_inverse).  Below
// ~10^4 sites a step of the iterative solver is ~60 dependent launches of a few microseconds each; streaming the
// matrix once is cheaper than that, needs no initial guess, no convergence test and no host decision.  The result
// is written only if the psi update of this step succeeded (fail_part: the per-workgroup flags of k_psi_update), so
// that a step that will be repeated with a smaller dt leaves mu^n intact without the host having looked yet.
// G is stored ONCE per symmetric pair: G = G^T, so only the tiles (I, J), J <= I, of
// DT x DT entries are kept (packed by tile, row major inside a tile, zero padded: 138 MB instead of
// 268 MB at 5.8k sites -- half the stream, and small enough to stay in the 256 MB Infinity Cache from
// one step to the next).  One workgroup per tile: wave w owns 32 of its rows, lane l the columns
// 2l, 2l + 1.  Every entry is used twice: g_rc b_c towards y_r (a sum over the lanes of a row: the
// per-lane products of 16 rows are reduced together by a transposing butterfly, 17 shuffles for 16 rows) and
// g_rc b_r towards y_c (a lane-local sum over the rows; the four waves meet in LDS).  The tile's two
// contributions go to fixed slots of `part` ([nt][nt * DT]: slot J of row block I and slot I of row
// block J), summed in a fixed order by k_dense_sym_finish -- no atomics, bit-reproducible.
constexpr int DT = 128;

// one step of the transposing butterfly: 2H per-lane values -> H, lanes 4H apart exchange the half they give up
template <int H>
__device__ __forceinline__ void butterfly_step(double *acc, int lane) {
    const bool upper = (lane & (4 * H)) != 0;
#pragma unroll
    for (int k = 0; k < H; ++k) {
        const double keep = upper ? acc[k + H] : acc[k];
        const double send = upper ? acc[k] : acc[k + H];
        acc[k] = keep + __shfl_xor(send, 4 * H, WAVE);
    }
}

// (VT: storage type of the tiles -- double, or float when the factors are the CG's PRECONDITIONER,
// tdgl_poisson_set_substructure_precond: every entry is widened on load, all arithmetic is fp64)
template <class VT> struct Pair2;
template <> struct Pair2<double> { typedef double2 type; };
template <> struct Pair2<float> { typedef float2 type; };

// (body: tile (I, J) at `tile`; k_blr_project runs it on the tiles the block low-rank form keeps dense)
template <class VT>
__device__ __forceinline__ void dense_sym_tile_body(int I, int J, int n, int nt, const VT *__restrict__ tile,
                                                    const double *__restrict__ b, double *__restrict__ part) {
    typedef typename Pair2<VT>::type V2;
    __shared__ double shc[BLOCK / WAVE][DT];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const V2 *__restrict__ g = reinterpret_cast<const V2 *>(tile) + (w * 32) * (DT / 2) + lane;
    const int cj = J * DT + 2 * lane;
    const double bjx = cj < n ? b[cj] : 0.0, bjy = cj + 1 < n ? b[cj + 1] : 0.0;
    double cx = 0.0, cy = 0.0;
    const int64_t ldp = (int64_t)nt * DT;
#pragma unroll 1
    for (int r0 = 0; r0 < 32; r0 += 16) {  // (not unrolled: 16 rows = 16 KB per wave in flight, <= 128 VGPRs)
        V2 raw[16];
        double2 v[16];
        double acc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) raw[k] = g[(r0 + k) * (DT / 2)];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = make_double2((double)raw[k].x, (double)raw[k].y);
        const int ri = I * DT + w * 32 + r0 + (lane & 15);
        const double bi = ri < n ? b[ri] : 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            acc[k] = v[k].x * bjx + v[k].y * bjy;
            // (b_r of row r0 + k sits in lane k: a scalar read, no cross-lane traffic)
            const double s = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(bi), k),
                                              __builtin_amdgcn_readlane(__double2loint(bi), k));
            cx += v[k].x * s;
            cy += v[k].y * s;
        }
        // transposing butterfly over 16 rows: afterwards lanes 4r .. 4r + 3 hold the sum of row r over the 64 lanes
        butterfly_step<8>(acc, lane);
        butterfly_step<4>(acc, lane);
        butterfly_step<2>(acc, lane);
        butterfly_step<1>(acc, lane);
        acc[0] += __shfl_xor(acc[0], 2, WAVE);
        acc[0] += __shfl_xor(acc[0], 1, WAVE);
        if ((lane & 3) == 0) part[(int64_t)J * ldp + I * DT + w * 32 + r0 + (lane >> 2)] = acc[0];
    }
    if (I != J) {  // (workgroup-uniform)
        shc[w][2 * lane] = cx;
        shc[w][2 * lane + 1] = cy;
        __syncthreads();
        if (threadIdx.x < DT) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < BLOCK / WAVE; ++i) s += shc[i][threadIdx.x];
            part[(int64_t)I * ldp + J * DT + threadIdx.x] = s;
        }
    }
}

template <class VT>
__global__ __launch_bounds__(BLOCK, 4) void k_dense_sym_tiles(int n, int nt, const VT *__restrict__ Gp,
                                                           const double *__restrict__ b, double *__restrict__ part,
                                                           const StepCtl *__restrict__ ctl) {
    if (ctl && !ctl->live) return;  // run-ahead: dead step
    const int t = blockIdx.x;
    int I = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    while (I * (I + 1) / 2 > t) --I;
    const int J = t - I * (I + 1) / 2;
    dense_sym_tile_body<VT>(I, J, n, nt, Gp + (int64_t)t * DT * DT, b, part);
}

// y = W x + V v: sparse W (CSR) plus dense row-major V [n_rows, ldv] (zero padded to a 16-byte
// multiple like v), one wavefront per row (tail of the collapsed coarse chain: the post-smoothed
// correction of the tail level from its right-hand side and the dense part's result).  The dense
// part needs no indices and is requested first; a sparse row of up to 64 * B entries costs two
// dependent round trips.
template <int B, class VT, class IT>
__global__ __launch_bounds__(BLOCK) void k_tail_up(int64_t n_rows, const int32_t *__restrict__ Wp,
                                                   const IT *__restrict__ Wi, const VT *__restrict__ Wv,
                                                   const double *__restrict__ x, int ldv, const VT *__restrict__ V,
                                                   const double *__restrict__ v, double *__restrict__ y) {
    typedef typename Vec16<VT>::type V16;
    constexpr int VW = Vec16<VT>::W;
    const int64_t row = xcd_tile(blockIdx.x, gridDim.x / XCDS) * (int64_t)(BLOCK / WAVE) + threadIdx.x / WAVE;
    const int sub = threadIdx.x & (WAVE - 1);
    if (row >= n_rows) return;  // (wave-uniform)
    const int beg = Wp[row], end = Wp[row + 1];
    const V16 *__restrict__ vr = reinterpret_cast<const V16 *>(V + row * (int64_t)ldv);
    const int nv = ldv / VW;
    double acc = 0.0;
    for (int c0 = sub; c0 < nv; c0 += 2 * WAVE) {
        const int c1 = c0 + WAVE;
        const V16 a = vr[c0], b2 = vr[min(c1, nv - 1)];
        acc += Vec16<VT>::dot(a, v + (int64_t)c0 * VW);
        if (c1 < nv) acc += Vec16<VT>::dot(b2, v + (int64_t)c1 * VW);
    }
    for (int base = beg + sub; base < end; base += WAVE * B) {
        int c[B];
        double w[B], g[B];
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const int kk = min(base + k * WAVE, end - 1);
            c[k] = (int)Wi[kk];  // (IT = uint16_t: the tail level has fewer than 65536 rows)
            w[k] = (double)Wv[kk];
        }
#pragma unroll
        for (int k = 0; k < B; ++k) g[k] = x[c[k]];
#pragma unroll
        for (int k = 0; k < B; ++k) acc += ((base + k * WAVE < end) ? w[k] : 0.0) * g[k];
    }
    acc = wave_sum(acc);
    if (sub == 0) y[row] = acc;
}

// Two CSR operators over the same rows in one launch (coarse levels; saves a launch per level on
// the way down and one on the way up -- these levels are launch/latency bound):
//   D_RESTRICT: y = M1 v1 - M2 v2                 (M1 = R, v1 = b, M2 = R A, v2 = x:
//                                                   the restricted residual R (b - A x))
//   D_PSMOOTH:  x' = x + P e;  inc = c2 dinv (b - A x');  d = inc;  y = x' + inc
//               with M1 = A (gathers v1 = x), M2 = pattern of A P (gathers v2 = e) carrying two
//               value arrays: A P (val2) and P padded to the same pattern (val2b)
enum DualOp { D_RESTRICT = 0, D_PSMOOTH = 1 };

template <int LANES, int OP, int B1, int B2, class VT = double>
__global__ __launch_bounds__(BLOCK) void k_csr_dual(
    int64_t n_rows, const int32_t *__restrict__ ip1, const int32_t *__restrict__ ix1,
    const VT *__restrict__ val1, const double *__restrict__ v1, const int32_t *__restrict__ ip2,
    const int32_t *__restrict__ ix2, const VT *__restrict__ val2, const VT *__restrict__ val2b,
    const double *__restrict__ v2, const double *__restrict__ b, const double *__restrict__ dinv, double c2,
    double *__restrict__ d, double *__restrict__ y) {
    const int64_t gid = xcd_tile(blockIdx.x, gridDim.x / XCDS) * (int64_t)BLOCK + threadIdx.x;
    const int64_t row = gid / LANES;
    const int sub = (int)(gid % LANES);
    const bool lead = row < n_rows && sub == 0;
    double xr = 0.0, br = 0.0, dr = 0.0;
    if (lead && OP == D_PSMOOTH) {
        xr = v1[row];
        br = b[row];
        dr = dinv[row];
    }
    double acc1 = 0.0, acc2 = 0.0;
    if (row < n_rows) {
        const int beg1 = ip1[row], end1 = ip1[row + 1], beg2 = ip2[row], end2 = ip2[row + 1];
        for (int base = beg1 + sub; base < end1; base += LANES * B1) {
            int c[B1];
            double v[B1], g[B1];
#pragma unroll
            for (int k = 0; k < B1; ++k) {
                const int kk = min(base + k * LANES, end1 - 1);
                c[k] = ix1[kk];
                v[k] = (double)val1[kk];
            }
#pragma unroll
            for (int k = 0; k < B1; ++k) g[k] = v1[c[k]];
#pragma unroll
            for (int k = 0; k < B1; ++k) acc1 += ((base + k * LANES < end1) ? v[k] : 0.0) * g[k];
        }
        for (int base = beg2 + sub; base < end2; base += LANES * B2) {
            int c[B2];
            double v[B2], w[B2], g[B2];
#pragma unroll
            for (int k = 0; k < B2; ++k) {
                const int kk = min(base + k * LANES, end2 - 1);
                c[k] = ix2[kk];
                v[k] = (double)val2[kk];
                w[k] = (OP == D_PSMOOTH) ? (double)val2b[kk] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < B2; ++k) g[k] = v2[c[k]];
#pragma unroll
            for (int k = 0; k < B2; ++k) {
                const bool ok = base + k * LANES < end2;
                if (OP == D_RESTRICT) {
                    acc1 -= (ok ? v[k] : 0.0) * g[k];
                } else {
                    acc1 += (ok ? v[k] : 0.0) * g[k];
                    acc2 += (ok ? w[k] : 0.0) * g[k];
                }
            }
        }
    }
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) {
        acc1 += __shfl_down(acc1, off, LANES);
        if (OP == D_PSMOOTH) acc2 += __shfl_down(acc2, off, LANES);
    }
    if (lead) {
        if (OP == D_RESTRICT) {
            y[row] = acc1;
        } else {
            const double xp = xr + acc2;
            const double inc = c2 * dr * (br - acc1);
            if (d) d[row] = inc;
            y[row] = xp + inc;
        }
    }
}

// First smoothing step from a zero initial guess: d = c2 dinv b, x = d.
__global__ __launch_bounds__(BLOCK) void k_smooth0(int64_t n, double c2,
                                                   const double *__restrict__ dinv,
                                                   const double *__restrict__ b,
                                                   double *__restrict__ d, double *__restrict__ x) {
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const double v = c2 * dinv[i] * b[i];
        if (d) d[i] = v;
        x[i] = v;
    }
}

// dense coarse solve: x = pinv * b, one wavefront per row
__global__ __launch_bounds__(BLOCK) void k_dense_matvec(int n, const double *__restrict__ M,
                                                        const double *__restrict__ b,
                                                        double *__restrict__ x) {
    const int row = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    if (row >= n) return;
    double acc = 0.0;
    for (int k = lane; k < n; k += WAVE) acc += M[(int64_t)row * n + k] * b[k];
    acc = wave_sum(acc);
    if (lane == 0) x[row] = acc;
}

// ------------------------------------------------------------------ Poisson: vector kernels
// partial[block] = sum a_i * b_i (b == nullptr: sum a_i), fixed grid of NB workgroups
__global__ __launch_bounds__(BLOCK) void k_dot_partial(int64_t n, const double *__restrict__ a,
                                                       const double *__restrict__ b,
                                                       double *__restrict__ partial) {
    double v = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK)
        v += a[i] * (b ? b[i] : 1.0);
    const double t = block_sum(v);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// scal[slot] = sum of the NB partials (only used where the HOST needs the number)
__global__ __launch_bounds__(BLOCK) void k_store_sum(const double *__restrict__ partial,
                                                     double *__restrict__ scal, int slot, double tol_factor) {
    const double s = sum_partials(partial);
    if (threadIdx.x == 0) {
        scal[slot] = s;
        if (tol_factor > 0.0) scal[S_TOL2] = tol_factor * s;  // rtol^2 ||b||^2 with slot = S_BB
    }
}

// One-reduction CG step (Chronopoulos & Gear): with z = M^-1 r and w = A z already formed and the
// three sums r.z, ||r_prev||^2, z.w available (one all-reduce in one-process-per-GPU mode),
//   beta = (r.z)/(r.z)_old,  alpha = (r.z) / (z.w - beta (r.z)/alpha_old)      (beta = 0 first)
//   p = z + beta p;  q = w + beta q  (= A p);  x += alpha p;  r -= alpha q;  partials of ||r||^2.
// Saves the classic recurrence's second global reduction (p.q).  `part` = [r.z | ||r_prev||^2 | z.w],
// NB entries each.  (r.z)_old / alpha_old live in scal[] in two slots alternating with the parity
// of the iteration, so that no workgroup reads a value another one has already replaced.
template <class ZT>
__global__ __launch_bounds__(BLOCK) void k_cg_update(int64_t n, const ZT *__restrict__ z,
                                                     const double *__restrict__ w,
                                                     const double *__restrict__ part, int first, int parity,
                                                     double *__restrict__ scal, double *__restrict__ p,
                                                     double *__restrict__ q, double *__restrict__ x,
                                                     double *__restrict__ r, double *__restrict__ part_rr) {
    double rz, rr_prev, zw;
    sum_partials3(part, part + NB, part + 2 * NB, &rz, &rr_prev, &zw);
    const bool converged = rr_prev <= scal[S_TOL2];
    double beta = 0.0, alpha = 0.0;
    if (!converged) {
        const double rz_old = scal[S_CG_RZ0 + (parity ^ 1)], alpha_old = scal[S_CG_ALPHA0 + (parity ^ 1)];
        beta = first ? 0.0 : rz / rz_old;
        const double denom = first ? zw : zw - beta * rz / alpha_old;
        alpha = (denom > 0.0) ? rz / denom : 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double it = scal[S_IT];
        if (converged && scal[S_CONV_IT] < 0.0) scal[S_CONV_IT] = it;
        if (it == 0.0) scal[S_RR0] = rr_prev;
        scal[S_IT] = it + 1.0;
        scal[S_CG_RZ0 + parity] = rz;
        scal[S_CG_ALPHA0 + parity] = alpha;
    }
    double rr = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        if (!converged) {
            const double zi = (double)z[i];
            const double pn = first ? zi : zi + beta * p[i], qn = first ? w[i] : w[i] + beta * q[i];
            p[i] = pn;
            q[i] = qn;
            x[i] += alpha * pn;
            r[i] -= alpha * qn;
        }
        rr += r[i] * r[i];
    }
    const double t = block_sum(rr);
    if (threadIdx.x == 0) part_rr[blockIdx.x] = t;
}

// v[i] -= (sum of partials) / count  for i < n_real  (remove the constant null-space component)
__global__ __launch_bounds__(BLOCK) void k_shift_mean(int64_t n_real, const double *__restrict__ partial,
                                                      double inv_count, double *__restrict__ v) {
    const double mean = sum_partials(partial) * inv_count;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n_real; i += (int64_t)gridDim.x * BLOCK)
        v[i] -= mean;
}

// ---- initial guess by projection onto previous solutions ---------------------------------------
// The mu system has the same matrix every step; only the right-hand side moves.  The window keeps the
// last K solutions x_j together with their images y_j = A x_j, and the guess is the combination whose
// RESIDUAL is smallest: x0 = X c with c = argmin ||b - Y c||_2, i.e. (Y^T Y) c = Y^T b (cf. P. Fischer,
// "Projection techniques for iterative solution of Ax = b with successive right-hand sides", 1998,
// in the residual norm).  y_j costs no operator application: the CG recurrence ends with
// r_j = b_j - A x_j to round-off, so y_j = b_j - r_j (k_finish_solution).  Because y_j is the image of
// x_j whatever the solver tolerance was, nothing about the window is inexact except round-off.
//
// Consecutive solutions are nearly parallel: with a smooth trajectory the k-th difference of the
// window is (dt/T)^k small, the Gram matrix Y^T Y has a condition number of (T/dt)^(2K), and in fp64
// everything beyond the first ~6 directions drowns in the rounding of the dot products (rounds 2-3: a
// window of 8 gained nothing over 6; guess residual 3e-5 of ||b|| whatever the window).  So the dot
// products are accumulated as DOUBLE-DOUBLE numbers (error-free products and sums, ~1e-32 relative: these
// passes are bandwidth bound, the extra flops are free), the K x K system is solved on the host in
// double-double arithmetic (poisson.inc: solve_gram_dd), and a window of 12 lowers the guess residual to
// 2e-6..4e-6 in the transient regime and by two to three orders in quasi-stationary states.
// Device work per step: one pass over b and the window's y_j (k_multi_dot) gives the K + 2 dot products
// with the new right-hand side AND the Gram row of the window's newest vector, y_new . y_j -- it joined
// the window at the end of the previous solve, after that step's pass; all vectors are in registers
// anyway, so the row costs flops only -- then one linear combination (k_combine).
constexpr int GK = GUESS_MAX;  // maximal window
constexpr int TAIL_Y_MAX = 4096;  // spare entries behind a coarse level's right-hand side (collapsed tail)

struct VecSet {
    const double *p[GK];
    double c[GK];
    int k;
};

// Partial arrays of the guess: array a in {0: b . b, 1: sum b, 2 + j: y_j . b, 2 + GK + j: y_newest . y_j}
// has its NB hi parts at (2 a) NB and its NB lo parts at (2 a + 1) NB.
constexpr int G_BB = 0, G_SB = 1, G_Y0 = 2, G_N0 = 2 + GK, G_ARRAYS = 2 * GK + 2;

// Double-double accumulation (Dekker / Knuth).  The error-free transformations need every operation
// rounded on its own, and HIP compiles device code with -ffp-contract=fast: `hi + a * b` becomes one fma,
// s is no longer fl(hi + p), and the sums are good to 1e-19 instead of 1e-32 (measured).  Contraction is
// switched off inside these functions, and they use plain operators: HIP's __dadd_rn / __dmul_rn are
// header inlines compiled WITH the contract flag, which the pragma of the calling function does not reach.
// (hi, lo) += a * b
__device__ __forceinline__ void dd_fma(double &hi, double &lo, double a, double b) {
#pragma clang fp contract(off)
    const double p = a * b;
    const double e = __builtin_fma(a, b, -p);
    const double s = hi + p;
    const double v = s - hi;
    const double err = (hi - (s - v)) + (p - v);
    hi = s;
    lo = lo + (err + e);
}
// (hi, lo) += (a, b)
__device__ __forceinline__ void dd_add(double &hi, double &lo, double a, double b) {
#pragma clang fp contract(off)
    const double s = hi + a;
    const double v = s - hi;
    const double err = (hi - (s - v)) + (a - v);
    const double l = (lo + b) + err;
    hi = s + l;  // renormalise: |lo| <= ulp(hi) / 2
    lo = l - (hi - s);
}
__device__ __forceinline__ void dd_wave_sum(double &hi, double &lo) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double a = __shfl_down(hi, off, WAVE), b = __shfl_down(lo, off, WAVE);
        dd_add(hi, lo, a, b);
    }
}

// Sums of N double-double accumulators over the wavefront by a TRANSPOSING butterfly: at the step with
// lane distance `off` a lane keeps one half of its values and hands the other half to its partner, so the
// values per lane halve while the lanes summed double -- N' - 1 + log2(64 / N') exchanges (N' = N rounded
// up to a power of two <= 64) instead of 6 N for N separate reductions (with 26-34 accumulators of ~25
// instructions per exchange the separate reductions cost more than the streaming loop they follow).
// Afterwards lane L holds, in hi[0] / lo[0], the wave total of accumulator dd_wave_owner<N>(L)
// (-1: none -- a duplicate or padding).
template <int N> struct DdPad { static constexpr int M = N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : N <= 8 ? 8 : N <= 16 ? 16 : N <= 32 ? 32 : 64; };
template <int N>
__device__ __forceinline__ int dd_wave_owner(int lane) {
    constexpr int M = DdPad<N>::M;
    // the M values are spread over the lanes' HIGH bits; the remaining low bits hold duplicates
    constexpr int dup = WAVE / M;  // lanes per value after the exchange steps
    const int idx = lane / dup;
    return ((lane % dup) == 0 && idx < N) ? idx : -1;
}
template <int N>
__device__ __forceinline__ void dd_wave_transpose_sum(double (&hi)[N], double (&lo)[N]) {
    constexpr int M = DdPad<N>::M;
    static_assert(N >= 1 && N <= 64, "at most one value per lane");
    // halving steps: width W values per lane -> W / 2, partner at distance off = 32, 16, ...
    int off = 32;
#pragma unroll
    for (int W = M; W > 1; W >>= 1, off >>= 1) {
        const bool upper = (threadIdx.x & off) != 0;
#pragma unroll
        for (int j = 0; j < W / 2; ++j) {  // (j < W / 2 <= M / 2 < N; indices are compile-time)
            const bool has_up = j + W / 2 < N;  // values at index >= N do not exist and read as zero
            const double up_h = has_up ? hi[has_up ? j + W / 2 : 0] : 0.0, up_l = has_up ? lo[has_up ? j + W / 2 : 0] : 0.0;
            const double keep_h = upper ? up_h : hi[j], keep_l = upper ? up_l : lo[j];
            const double send_h = upper ? hi[j] : up_h, send_l = upper ? lo[j] : up_l;
            const double rh = __shfl_xor(send_h, off, WAVE), rl = __shfl_xor(send_l, off, WAVE);
            hi[j] = keep_h;
            lo[j] = keep_l;
            dd_add(hi[j], lo[j], rh, rl);
        }
    }
    // remaining steps: both partners hold the same accumulator
#pragma unroll
    for (; off > 0; off >>= 1) {
        const double rh = __shfl_xor(hi[0], off, WAVE), rl = __shfl_xor(lo[0], off, WAVE);
        dd_add(hi[0], lo[0], rh, rl);
    }
}

// partial[(2 (2 + j)) NB + block] (+ NB: lo) = sum_i y_j[i] b[i]  (j < vs.k; zero for the unused j), the
// partials of b . b and sum b, and -- `newest` >= 0 -- those of y_newest . y_j at array 2 + GK + j.  b is
// the RAW right-hand side: its mean is removed arithmetically afterwards (the y_j have zero mean, so
// y_j . b does not see it; ||b - m||^2 = b.b - n m^2).
// KT: compiled window (8 or 16) -- registers only.
template <int KT>
__global__ __launch_bounds__(BLOCK) void k_multi_dot(int64_t n, const double *__restrict__ b, VecSet vs, int newest,
                                                     double *__restrict__ partial) {
    double hi[2 * KT + 2], lo[2 * KT + 2];  // [0, 2): b.b, sum b; [2, 2 + KT): y_j . b; [2 + KT, 2 + 2 KT): y_newest . y_j
#pragma unroll
    for (int j = 0; j < 2 * KT + 2; ++j) hi[j] = lo[j] = 0.0;
    // 16-byte accesses: two entries per lane and stream; an odd last entry is done by one thread
    const int64_t n2 = n / 2;
    const double2 *__restrict__ b2 = reinterpret_cast<const double2 *>(b);
    // Software-pipelined over two register sets: the loads of the NEXT grid-stride iteration are in flight during
    // the ~600 dependent double-double operations of the current one -- with one workgroup per CU (one wave per
    // SIMD) nothing else would hide the memory latency behind the arithmetic.  No divergent control flow: every
    // lane runs the same number of iterations, indices past the end are clamped and their values zeroed (adding
    // an exact zero leaves a double-double sum unchanged); unused window slots read b and are zeroed at the end.
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    const int64_t iters = (n2 + stride - 1) / stride;
    const double2 *pj[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) pj[j] = j < vs.k ? reinterpret_cast<const double2 *>(vs.p[j]) : b2;
    int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    double2 bA, yA[KT], bB, yB[KT];
    auto fetch = [&](int64_t idx, double2 &bv, double2(&y)[KT]) {
        const int64_t ic = idx < n2 ? idx : 0;
        bv = b2[ic];
#pragma unroll
        for (int j = 0; j < KT; ++j) y[j] = pj[j][ic];
    };
    auto accumulate = [&](int64_t idx, double2 bv, double2(&y)[KT]) {
        const bool ok = idx < n2;
        if (!ok) bv = make_double2(0.0, 0.0);
        double2 yn = make_double2(0.0, 0.0);
#pragma unroll
        for (int j = 0; j < KT; ++j) {
            if (!ok) y[j] = make_double2(0.0, 0.0);
            if (j == newest) yn = y[j];
        }
#pragma unroll
        for (int j = 0; j < KT; ++j) {
            dd_fma(hi[2 + j], lo[2 + j], y[j].x, bv.x);
            dd_fma(hi[2 + j], lo[2 + j], y[j].y, bv.y);
            dd_fma(hi[2 + KT + j], lo[2 + KT + j], y[j].x, yn.x);
            dd_fma(hi[2 + KT + j], lo[2 + KT + j], y[j].y, yn.y);
        }
        dd_fma(hi[G_BB], lo[G_BB], bv.x, bv.x);
        dd_fma(hi[G_BB], lo[G_BB], bv.y, bv.y);
        dd_add(hi[G_SB], lo[G_SB], bv.x, 0.0);
        dd_add(hi[G_SB], lo[G_SB], bv.y, 0.0);
    };
    if (iters > 0) fetch(i, bA, yA);
    for (int64_t it = 0; it < iters; it += 2) {
        fetch(i + stride, bB, yB);
        accumulate(i, bA, yA);
        fetch(i + 2 * stride, bA, yA);
        accumulate(i + stride, bB, yB);
        i += 2 * stride;
    }
#pragma unroll
    for (int j = 0; j < KT; ++j)
        if (j >= vs.k) hi[2 + j] = lo[2 + j] = hi[2 + KT + j] = lo[2 + KT + j] = 0.0;
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double bi = b[n - 1];
        const double yn = newest >= 0 ? vs.p[newest][n - 1] : 0.0;
#pragma unroll
        for (int j = 0; j < KT; ++j)
            if (j < vs.k) {
                dd_fma(hi[2 + j], lo[2 + j], vs.p[j][n - 1], bi);
                dd_fma(hi[2 + KT + j], lo[2 + KT + j], vs.p[j][n - 1], yn);
            }
        dd_fma(hi[G_BB], lo[G_BB], bi, bi);
        dd_add(hi[G_SB], lo[G_SB], bi, 0.0);
    }
    __shared__ double sh[2 * KT + 2][2][BLOCK / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    dd_wave_transpose_sum<2 * KT + 2>(hi, lo);
    const int own = dd_wave_owner<2 * KT + 2>(lane);
    if (own >= 0) {
        sh[own][0][w] = hi[0];
        sh[own][1][w] = lo[0];
    }
    __syncthreads();
    if (threadIdx.x < 2 * KT + 2) {
        double th = 0.0, tl = 0.0;
#pragma unroll
        for (int i = 0; i < BLOCK / WAVE; ++i) dd_add(th, tl, sh[threadIdx.x][0][i], sh[threadIdx.x][1][i]);
        const int arr = threadIdx.x < 2 + KT ? threadIdx.x : G_N0 + (threadIdx.x - 2 - KT);
        partial[(2 * arr) * NB + blockIdx.x] = th;
        partial[(2 * arr + 1) * NB + blockIdx.x] = tl;
    }
}

// x = sum_j c_j x_j
template <int KT>
__global__ __launch_bounds__(BLOCK) void k_combine(int64_t n, VecSet vs, double *__restrict__ x) {
    const int64_t n2 = n / 2;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n2; i += (int64_t)gridDim.x * BLOCK) {
        double2 xv[KT];
#pragma unroll
        for (int j = 0; j < KT; ++j)
            xv[j] = (j < vs.k) ? reinterpret_cast<const double2 *>(vs.p[j])[i] : make_double2(0.0, 0.0);
        double2 v = make_double2(0.0, 0.0);
#pragma unroll
        for (int j = 0; j < KT; ++j) {
            const double cj = (j < vs.k) ? vs.c[j] : 0.0;
            v.x += cj * xv[j].x;
            v.y += cj * xv[j].y;
        }
        reinterpret_cast<double2 *>(x)[i] = v;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < KT; ++j)
            if (j < vs.k) v += vs.c[j] * vs.p[j][n - 1];
        x[n - 1] = v;
    }
}

// End of a solve: zero-mean gauge (as k_shift_mean), copy into the window slot, and the image of the
// solution y = A x = (b - mean b) - r  (r: the residual the CG recurrence ended with) into its slot.
// guard (the PCG scalars, or NULL): queued before the host has seen the residual -- the kernel holds back unless the
// scalars the status kernel has just written say what the host is about to read from their copy: converged
// (poisson.inc: cg_iterate takes the same decision from the same numbers).
__global__ __launch_bounds__(BLOCK) void k_finish_solution(int64_t n_real, const double *__restrict__ partial_mean,
                                                           double inv_count, double *__restrict__ x,
                                                           const double *__restrict__ b, double b_mean,
                                                           const double *__restrict__ r, double *__restrict__ slot_x,
                                                           double *__restrict__ slot_y, const double *__restrict__ guard) {
    if (guard && !(guard[S_CONV_IT] >= 0.0 || guard[S_RR] <= guard[S_TOL2])) return;
    const double mean = sum_partials(partial_mean) * inv_count;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n_real; i += (int64_t)gridDim.x * BLOCK) {
        const double v = x[i] - mean;
        x[i] = v;
        slot_x[i] = v;
        slot_y[i] = (b[i] - b_mean) - r[i];
    }
}

// Polynomial extrapolation of mu in time as the initial guess of the next solve:
// guess = l0 mu^n + l1 mu^{n-1} + l2 mu^{n-2} (Lagrange weights for the variable steps, from the
// host; l2 = 0 -> linear, l1 = l2 = 0 -> none);  history shifts: prev2 <- prev, prev <- mu, mu <- guess.
__global__ __launch_bounds__(BLOCK) void k_extrapolate(int64_t n, double l0, double l1, double l2,
                                                       double *__restrict__ mu, double *__restrict__ mu_prev,
                                                       double *__restrict__ mu_prev2) {
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const double m = mu[i], mp = mu_prev[i], mpp = mu_prev2[i];
        mu_prev2[i] = mp;
        mu_prev[i] = m;
        mu[i] = l0 * m + l1 * mp + l2 * mpp;
    }
}

// ---- measurement only (tdgl_time_kernel ids 10-15): what a device-wide barrier costs inside ONE launch,
// against the ~3 us of a kernel boundary.  `workers` workgroups (those with blockIdx.x % stride == 0)
// write a value, synchronise, read their neighbour's value and check it, `iters` times.
//   MODE 0: cooperative-groups grid.sync() (cooperative launch)
//   MODE 1: monotonic counter, agent-scope release / acquire fences around it
//   MODE 2: the same with the fences replaced by what suffices when all workers share one XCD's L2
//           (stores drained with s_waitcnt, L1 invalidated): only valid for stride == 8
// err[0] counts stale reads; err[1 + b] = XCC_ID of workgroup b (b < 16): the block -> XCD mapping.
template <int MODE>
__global__ __launch_bounds__(BLOCK) void k_barrier_bench(int iters, int stride, int workers, unsigned *cnt,
                                                         double *data, int *err) {
    if (blockIdx.x < 16 && threadIdx.x == 0) err[1 + blockIdx.x] = (int)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));
    if (blockIdx.x % stride != 0) return;
    const int w = blockIdx.x / stride;
    int bad = 0;
    for (int it = 1; it <= iters; ++it) {
        data[w * BLOCK + threadIdx.x] = (double)it;
        if (MODE == 0) {
            cooperative_groups::this_grid().sync();
        } else {
            __syncthreads();
            if (threadIdx.x == 0) {
                if (MODE == 1) __threadfence();
                else __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
                atomicAdd(cnt, 1u);
                const unsigned target = (unsigned)it * (unsigned)workers;
                while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) __builtin_amdgcn_s_sleep(1);
                if (MODE == 1) __threadfence();
            }
            __syncthreads();
            if (MODE == 2) __asm__ volatile("buffer_inv sc0\n s_waitcnt vmcnt(0)" ::: "memory");
        }
        const double v = data[((w + 1) % workers) * BLOCK + threadIdx.x];
        if (v != (double)it && v != (double)(it + 1)) bad = 1;  // (the neighbour may already have written the next value)
        if (MODE == 0) cooperative_groups::this_grid().sync();  // (keep the neighbour from running two values ahead)
    }
    if (bad) atomicAdd(err, 1);
}

// measurement only (tdgl_time_kernel 16 / 17): HBM-cold streaming ceilings on buffers far larger than the
// 256 MB Infinity Cache -- read-only (sum of a double2 stream, U independent 16-byte loads per lane in
// flight) and copy
template <int U>
__global__ __launch_bounds__(BLOCK) void k_stream_read(int64_t n2, const double2 *__restrict__ a, double *__restrict__ out) {
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n2; i += stride * U) {
        double2 v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) v[k] = a[min(i + k * stride, n2 - 1)];
#pragma unroll
        for (int k = 0; k < U; ++k) acc += v[k].x + v[k].y;
    }
    if (acc == 1.2345e-300) out[0] = acc;  // (keeps the loads alive)
}

// measurement only (tdgl_time_kernel 21): what ONE workgroup of 1024 threads (one CU) reads per second from
// an L2-resident 2 MiB buffer -- the budget of a single-workgroup persistent solver for small meshes
__global__ __launch_bounds__(1024) void k_one_cu_read(int reps, int64_t n2, const double2 *__restrict__ a, double *__restrict__ out) {
    double acc = 0.0;
    for (int r = 0; r < reps; ++r) {
        for (int64_t i = threadIdx.x; i < n2; i += 1024 * 4) {
            double2 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = a[min(i + k * 1024, n2 - 1)];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += v[k].x + v[k].y;
        }
        __syncthreads();
    }
    if (acc == 1.2345e-300) out[0] = acc;
}

template <int U>
__global__ __launch_bounds__(BLOCK) void k_stream_copy(int64_t n2, const double2 *__restrict__ a, double2 *__restrict__ b) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n2; i += stride * U) {
        double2 v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) v[k] = a[min(i + k * stride, n2 - 1)];
#pragma unroll
        for (int k = 0; k < U; ++k)
            if (i + k * stride < n2) b[i + k * stride] = v[k];
    }
}

__global__ __launch_bounds__(BLOCK) void k_copy_d2(int64_t n, const double2 *__restrict__ a,
                                                   double2 *__restrict__ b) {
    int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i < n) b[i] = a[i];
}

__global__ __launch_bounds__(BLOCK) void k_from_f32(int64_t n, const float *__restrict__ a, double *__restrict__ b) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i < n) b[i] = (double)a[i];
}

__global__ __launch_bounds__(BLOCK) void k_to_f16(int64_t n, const double *__restrict__ a, half_t *__restrict__ b) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i < n) b[i] = (half_t)a[i];
}

__global__ __launch_bounds__(BLOCK) void k_to_f32(int64_t n, const double *__restrict__ a, float *__restrict__ b) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i < n) b[i] = (float)a[i];
}

// Sums of the projection guess's partial arrays (layout of k_multi_dot with stride `stride` between arrays,
// `nparts` entries each): 8 threads per array (32 arrays per round), each over every 8th entry, then three
// exchanges among the 8 -- fixed order, double-double.  Arrays the window does not use (gk vectors) give
// zero.  out[(2 a) ostride + opos] = hi, out[(2 a + 1) ostride + opos] = lo.  One workgroup of BLOCK threads.
__device__ __forceinline__ void guess_sum_arrays(const double *__restrict__ part, int stride, int nparts, int gk,
                                                 double *__restrict__ out, int ostride, int opos) {
    for (int base = 0; base < G_ARRAYS; base += BLOCK / 8) {
        const int j = base + threadIdx.x / 8, sub = threadIdx.x % 8;
        const bool live = j < G_Y0 + gk || (j >= G_N0 && j < G_N0 + gk);
        double vh = 0.0, vl = 0.0;
        if (j < G_ARRAYS && live) {
            // up to 32 entries per thread (256 partials: all of them) requested together, then added in index order:
            // one round trip for the whole array instead of one per few entries -- this kernel is ONE workgroup on
            // the step's critical path
            const double *__restrict__ ph = part + (size_t)(2 * j) * stride, *__restrict__ pl = part + (size_t)(2 * j + 1) * stride;
            constexpr int GB_ = 32;
            for (int i = sub; i < nparts; i += 8 * GB_) {
                double hb[GB_], lb[GB_];
#pragma unroll
                for (int k = 0; k < GB_; ++k) {
                    const int ii = i + 8 * k;
                    hb[k] = ii < nparts ? ph[ii] : 0.0;
                    lb[k] = ii < nparts ? pl[ii] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < GB_; ++k) dd_add(vh, vl, hb[k], lb[k]);
            }
        }
#pragma unroll
        for (int off = 4; off > 0; off >>= 1) {
            const double oh = __shfl_xor(vh, off, WAVE), ol = __shfl_xor(vl, off, WAVE);
            dd_add(vh, vl, oh, ol);
        }
        if (j < G_ARRAYS && sub == 0) {
            out[(size_t)(2 * j) * ostride + opos] = vh;
            out[(size_t)(2 * j + 1) * ostride + opos] = vl;
        }
    }
}

// One process per GPU: this rank's double-double totals go to position `rank` of arrays with stride
// G_RANK_STRIDE whose other positions stay zero on this rank, so that the all-reduce (a sum with zeros is
// exact) hands every rank all ranks' totals -- an all-gather through the transport the library has; the
// status kernel then adds them in rank order, in double-double.
constexpr int G_RANK_STRIDE = 16;
__global__ __launch_bounds__(BLOCK) void k_guess_rank_totals(const double *__restrict__ part, int nparts, int gk,
                                                             double *__restrict__ out, int rank) {
    // (the all-reduce leaves every rank's totals of the LAST step in the buffer: clear the others' first)
    for (int i = threadIdx.x; i < 2 * G_ARRAYS * G_RANK_STRIDE; i += BLOCK)
        if (i % G_RANK_STRIDE != rank) out[i] = 0.0;
    guess_sum_arrays(part, NB, nparts, gk, out, G_RANK_STRIDE, rank);
}

// max / any over the per-workgroup results of k_psi_update (one workgroup of BLOCK threads);
// valid in thread 0
__device__ __forceinline__ void reduce_psi_status(const double *__restrict__ dmax_part,
                                                  const int32_t *__restrict__ fail_part, int nblk, double *dmax,
                                                  int *fail) {
    double m = 0.0;
    int f = 0;
    for (int i = threadIdx.x; i < nblk; i += BLOCK) {
        m = fmax(m, dmax_part[i]);
        f |= fail_part[i];
    }
    *dmax = block_max(m);
    *fail = __syncthreads_or(f);
}

// Status block the host reads -- ONE workgroup does everything the host synchronisation needs:
//   * gdot_part given (start of a solve with the projection guess): sums the G_ARRAYS partial arrays
//     into gdot[], removes the mean of b arithmetically (scal[S_BB] = b.b - n m^2, S_TOL2 = rtol^2 of
//     it) and resets the iteration counters (S_CONV_IT = -1, S_IT = 0);
//   * rr_part given (convergence check): scal[S_RR] = sum of the NB residual partials;
//   * copies the PCG scalars and gdot[] into the status block;
//   * dmax_part given: reduces the outcome of the last psi update (failure flag, max d|psi|^2).
__global__ __launch_bounds__(BLOCK) void k_publish_status(StepStatus *__restrict__ st, double *__restrict__ scal,
                                                          const double *__restrict__ dmax_part,
                                                          const int32_t *__restrict__ fail_part, int nblk,
                                                          double *__restrict__ gdot,
                                                          const double *__restrict__ gdot_part, int gk, int gparts, int gstride, double n_global,
                                                          double rtol2, const double *__restrict__ rr_part) {
    if (gdot_part) {
        guess_sum_arrays(gdot_part, gstride, gparts, gk, gdot, 1, 0);
        __syncthreads();
        if (threadIdx.x == 0) {
            const double m = gdot[2 * G_SB] / n_global;
            const double bb = fmax(gdot[2 * G_BB] - n_global * m * m, 0.0);
            scal[S_BB] = bb;
            scal[S_TOL2] = rtol2 * bb;
            scal[S_CONV_IT] = -1.0;
            scal[S_IT] = 0.0;
        }
        __syncthreads();
    }
    if (rr_part) {
        const double s = sum_partials(rr_part);
        if (threadIdx.x == 0) scal[S_RR] = s;
        __syncthreads();
    }
    if (threadIdx.x < S_COUNT) st->scal[threadIdx.x] = scal[threadIdx.x];
    if (gdot && threadIdx.x < 2 * G_ARRAYS) st->gdot[threadIdx.x] = gdot[threadIdx.x];
    if (dmax_part) {
        double m;
        int f;
        reduce_psi_status(dmax_part, fail_part, nblk, &m, &f);
        if (threadIdx.x == 0) {
            st->fail_flag = f ? 1 : 0;
            st->dmax_bits[0] = (unsigned long long)__double_as_longlong(m);
        }
        if (threadIdx.x > 0 && threadIdx.x < XCDS) st->dmax_bits[threadIdx.x] = 0ull;
    }
}

// numpy's pairwise summation for fewer than 129 terms (loop.inc: numpy_pairwise_sum), on the device and in the host replay
__host__ __device__ __forceinline__ double numpy_sum_le128(const double *a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r[8];
    for (int k = 0; k < 8; ++k) r[k] = a[k];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int k = 0; k < 8; ++k) r[k] += a[i + k];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

// The scalar fields of StepCtl in front of `hist`, as one block: the controller reads them in ONE batch of wide loads
// (read field by field between its stores and branches they were a dozen dependent round trips -- 4 of the 8 us the
// launch that carries the controller took at 5.8k sites, where a whole step is 31 us).
struct StepCtlHead {
    double tentative_dt, attempt_dt, time, end_time, dt_init, dt_cap, multiplier;
    long long stage_step;
    int adaptive, window, max_retries, cur, retries, poisoned, live, last_ok, reached_end, error, n_done, n_acc, hist_count, pad;
};
static_assert(offsetof(StepCtl, hist) == sizeof(StepCtlHead), "StepCtlHead mirrors the fields of StepCtl in front of hist");

// One thread: the bookkeeping of an attempt in the run-ahead time loop -- what step_once's retry loop,
// step_finish and tdgl_run do on the host in the classic loop (solver.py:475-485, 698-707,
// runner.py:429-433), in the same arithmetic and order.
__host__ __device__ __forceinline__ void step_controller(StepCtl *__restrict__ ctl, StepRec *__restrict__ rec, double dmax, int fail) {
    const StepCtlHead h = *reinterpret_cast<const StepCtlHead *>(ctl);
    if (!h.live) return;
    if (h.n_done >= RA_BATCH_MAX) {  // (the host never queues more: the record array has RA_BATCH_MAX slots)
        ctl->poisoned = 1;
        return;
    }
    const double dt = h.attempt_dt;
    StepRec r;
    r.dt = dt;
    r.dmax = dmax;
    r.ok = fail ? 0 : 1;
    r.pad = 0;
    rec[h.n_done] = r;
    ctl->n_done = h.n_done + 1;
    ctl->last_ok = fail ? 0 : 1;
    if (fail) {
        // solver.py:475-485: repeat the step with a smaller dt -- the next queued attempt does, the state did not move
        if (!h.adaptive || h.retries > h.max_retries) {
            ctl->error = 1;  // retry budget spent: the host raises the reference's error
            ctl->poisoned = 1;
        } else {
            ctl->attempt_dt = dt * h.multiplier;
            ctl->retries = h.retries + 1;
        }
        return;
    }
    ctl->cur = h.cur ^ 1;  // accept: psi' becomes psi^n
    ctl->retries = 0;
    ctl->n_acc = h.n_acc + 1;
    double tentative = h.tentative_dt;
    if (h.adaptive) {
        const int w = h.window;
        int cnt = h.hist_count;
        if (cnt < w) {
            ctl->hist[cnt++] = dmax;
            ctl->hist_count = cnt;
        } else {
            for (int i = 0; i + 1 < w; ++i) ctl->hist[i] = ctl->hist[i + 1];
            ctl->hist[w - 1] = dmax;
        }
        if (h.stage_step > w) {
            const double mean = numpy_sum_le128(ctl->hist, cnt) / (double)cnt;
            const double new_dt = h.dt_init / fmax(1e-10, mean);
            tentative = fmin(fmax(0.5 * (new_dt + dt), 0.0), h.dt_cap);
            ctl->tentative_dt = tentative;
        }
    }
    ctl->attempt_dt = tentative;
    if (h.time >= h.end_time) {  // runner.py:429-430: tested before time advances
        ctl->reached_end = 1;
        ctl->poisoned = 1;
    } else {
        ctl->runner_dt = dt;  // runner.py:431
        ctl->time = h.time + dt;
        ctl->stage_step = h.stage_step + 1;
    }
}

// What the last launch of a dense product (k_dense_sym_finish, k_blr_finish, the ensemble's k_ens_finish / k_ens_sub_top)
// does with its 64 sums per workgroup.  Built by finish_product / finish_separator below and, inside a time step, by
// finish_in_step (factors.inc); the ensemble's kernels fill one per replica.
struct DenseFinish {
    const double *__restrict__ dmax_part;   // the step's psi update per workgroup: max d|psi|^2 ...
    const int32_t *__restrict__ fail_part;  // ... and its failure flags (NULL: none to look at)
    int nfail;                              // entries of either
    StepStatus *__restrict__ st;            // classic loop: workgroup 0 publishes the step's status block from them
    int guard;                              // != 0: a raised flag holds back the write of y
    double *__restrict__ y;                 // the product
    const double *__restrict__ u;           // separator solve: the workgroup's share of u . y goes to ...
    double *__restrict__ upart;             // ... upart[workgroup]
    StepCtl *__restrict__ ctl;              // run-ahead loop: a dead step does nothing, workgroup 0 runs the controller ...
    StepRec *__restrict__ rec;              // ... which records the step here
};

// the bare product (y and nothing else) / the solve of a top separator (x_S and the shares of u . x_S the way up removes
// the mean with)
__host__ __device__ inline DenseFinish finish_product(double *y) { DenseFinish f{}; f.y = y; return f; }
__host__ __device__ inline DenseFinish finish_separator(double *xs, const double *u, double *upart) { DenseFinish f = finish_product(xs); f.u = u, f.upart = upart; return f; }

// What the second launch of a dense solve does with its 64 sums v (lane = row; wave 0 writes them): the held-back write
// of y, the workgroup's share of u . x_S, and (workgroup 0) the step's status block / the run-ahead controller
__device__ __forceinline__ void dense_finish_tail(int blk, int n, double v, int anybad, const DenseFinish &fin) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int i = blk * WAVE + lane;
    if (w == 0) {
        if (i < n && !anybad) fin.y[i] = v;
        if (fin.u) {  // substructured solve: this workgroup's share of u . x_S (k_sub_up removes the mean with it)
            const double c = wave_sum(i < n ? fin.u[i] * v : 0.0);
            if (lane == 0) fin.upart[blk] = c;
        }
    }
    if ((fin.st || fin.ctl) && blk == 0) {  // (workgroup-uniform)
        double m;
        int f;
        reduce_psi_status(fin.dmax_part, fin.fail_part, fin.nfail, &m, &f);
        if (threadIdx.x == 0) {
            if (fin.st) {
                fin.st->fail_flag = f ? 1 : 0;
                fin.st->dmax_bits[0] = (unsigned long long)__double_as_longlong(m);
            }
            // run-ahead: the step's bookkeeping (every workgroup of this launch has read ctl->live by now or
            // reads the value this thread leaves unchanged: only `poisoned` and the counters move)
            if (fin.ctl) step_controller(fin.ctl, fin.rec, m, f);
        }
        if (fin.st && threadIdx.x > 0 && threadIdx.x < XCDS) fin.st->dmax_bits[threadIdx.x] = 0ull;
    }
}

// Second half of the symmetric dense solve: y_i = sum over the nt slots of `part`, in slot order; 64 outputs
// per workgroup, wave w takes the slots w, w + 4, ... (all loads independent), the four waves meet in LDS
// in a fixed order.  Held back when the psi update of this step failed.  In the time
// loop workgroup 0 also publishes the step's status block (failure flag, max d|psi|^2: what
// k_publish_status does on the iterative path) -- one launch less per step.
// (body: workgroup `blk` of the launch; the ensemble's launch, ensemble.inc, runs one per replica)
__device__ __forceinline__ void dense_sym_finish_body(int blk, int n, int nt, const double *__restrict__ part, const DenseFinish &fin) {
    __shared__ double sh[BLOCK / WAVE][WAVE];
    if (fin.ctl && !fin.ctl->live) return;  // run-ahead: a dead step (behind a failed one / the end) does nothing
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int i = blk * WAVE + lane;
    const int64_t ldp = (int64_t)nt * DT;
    int bad = 0;
    if (fin.guard && fin.fail_part)
        for (int k = threadIdx.x; k < fin.nfail; k += BLOCK) bad |= fin.fail_part[k];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        // sixteen slots per batch, all requested before the first is added (unconditional requests on a clamped slot: a
        // conditional load is a branch and a wait, profiles/EXPERIMENTS.md round 6) -- a top separator of up to 8,192 sites
        // is ONE batch per wavefront where the loop of four used to take four to six round trips
        for (int k0 = w; k0 < nt; k0 += 64) {
            double v[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) v[t] = part[(int64_t)min(k0 + 4 * t, nt - 1) * ldp + i];
#pragma unroll
            for (int t = 0; t < 16; ++t) s[t & 3] += k0 + 4 * t < nt ? v[t] : 0.0;
        }
    }
    sh[w][lane] = (s[0] + s[1]) + (s[2] + s[3]);
    const int anybad = __syncthreads_or(bad);
    const double v = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
    dense_finish_tail(blk, n, v, anybad, fin);
}

__global__ __launch_bounds__(BLOCK) void k_dense_sym_finish(int n, int nt, const double *__restrict__ part, DenseFinish fin) {
    dense_sym_finish_body(blockIdx.x, n, nt, part, fin);
}

// The preconditioner's top separator in block low-rank form (dense.inc: dense_to_blr).  The tile pairs (I, J), I > J,
// whose fp64 block is numerically of low rank are kept as G_IJ ~ U_IJ W_IJ^T (fp32 factors of r columns); the
// diagonal tiles and the blocks that do not pay stay dense tiles.  Row block K of DT rows owns the columns F_K = every
// U_KJ (J < K) and every W_IK (I > K) in pair order: y_K = sum over K's dense tiles + F_K c_K, where the coefficient
// of a U_KJ column is the matching W_KJ column's projection onto x_J and vice versa -- so both launches stream the
// same columns, once as projections (c = F^T x, written to the twin column's slot) and once back into y.  Storage of
// F_K: its columns padded to a multiple of 4, row half h (64 rows) of column c at F + DT * colbase[K] + (h * R + c) * 64:
// four columns of one half are one contiguous kilobyte, what a wavefront reads in one request (float4 per lane).
struct BlrItem {
    int32_t K, g0, g1, pad;  // a wavefront's groups [g0, g1) of four columns of row block K
};

struct BlrArgs {
    int ndense;                          // dense tiles: the first workgroups of k_blr_project
    int nitems;                          // wavefront items of the projections
    const int32_t *__restrict__ dense_ij;  // [ndense] I << 16 | J
    const float *__restrict__ Gd;        // [ndense][DT * DT] the dense tiles, as k_dense_sym_tiles stores them
    const float *__restrict__ F;         // the columns
    const int64_t *__restrict__ colbase;  // [nt + 1] first column of row block K (multiples of 4)
    const int32_t *__restrict__ twin;    // [columns] the slot of coef the column's projection goes to (-1: padding)
    const BlrItem *__restrict__ items;   // [nitems]
    double *__restrict__ coef;           // [columns] (padding: 0, never written)
    const int32_t *__restrict__ dslot_ptr;  // [nt + 1] the dense slots of part row block K sums ...
    const int32_t *__restrict__ dslot;   // ... (the J of its dense tiles, the diagonal included)
};

constexpr int BLR_ITEM_GROUPS = 8;  // groups of four columns per wavefront item of k_blr_project

// Launch 1: the dense tiles (k_dense_sym_tiles' body, slots of `part`) and every column's projection c = F_K^T x_K.
// A wavefront takes BLR_ITEM_GROUPS groups of four columns; lane l reads rows 4 (l & 15) .. + 3 of column 4 g + l / 16
// in both halves (two 1-KB requests per group and wavefront), the 16 lanes of a column are summed by a butterfly.
__global__ __launch_bounds__(BLOCK, 4) void k_blr_project(int n, int nt, BlrArgs a, const double *__restrict__ b,
                                                       double *__restrict__ part, const StepCtl *__restrict__ ctl) {
    if (ctl && !ctl->live) return;  // run-ahead: dead step
    if ((int)blockIdx.x < a.ndense) {  // (workgroup-uniform)
        const int ij = a.dense_ij[blockIdx.x];
        dense_sym_tile_body<float>(ij >> 16, ij & 0xffff, n, nt, a.Gd + (int64_t)blockIdx.x * DT * DT, b, part);
        return;
    }
    const int item = ((int)blockIdx.x - a.ndense) * (BLOCK / WAVE) + (int)(threadIdx.x / WAVE);
    if (item >= a.nitems) return;  // (wave-uniform)
    const BlrItem it = a.items[item];
    const int lane = threadIdx.x & (WAVE - 1), rr = 4 * (lane & 15), cl = lane >> 4;
    const int64_t cb = a.colbase[it.K];
    const int R = (int)(a.colbase[it.K + 1] - cb);
    const float *__restrict__ Fk = a.F + cb * DT;
    double xv[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = it.K * DT + h * WAVE + rr + j;
            xv[h][j] = row < n ? b[row] : 0.0;
        }
    float4 f[BLR_ITEM_GROUPS][2];
#pragma unroll
    for (int u = 0; u < BLR_ITEM_GROUPS; ++u) {  // (every request first: groups past the item's end repeat its last)
        const int col = 4 * min(it.g0 + u, it.g1 - 1) + cl;
#pragma unroll
        for (int h = 0; h < 2; ++h) f[u][h] = *reinterpret_cast<const float4 *>(Fk + ((int64_t)h * R + col) * WAVE + rr);
    }
#pragma unroll
    for (int u = 0; u < BLR_ITEM_GROUPS; ++u) {
        double s = 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            s += ((double)f[u][h].x * xv[h][0] + (double)f[u][h].y * xv[h][1]) + ((double)f[u][h].z * xv[h][2] + (double)f[u][h].w * xv[h][3]);
        s += __shfl_xor(s, 1, WAVE);
        s += __shfl_xor(s, 2, WAVE);
        s += __shfl_xor(s, 4, WAVE);
        s += __shfl_xor(s, 8, WAVE);
        if ((lane & 15) == 0 && it.g0 + u < it.g1) {
            const int32_t t = a.twin[cb + 4 * (it.g0 + u) + cl];
            if (t >= 0) a.coef[t] = s;
        }
    }
}

// Launch 2: y of 64 rows (half h of row block K = blk / 2) = its dense slots of `part` + F_K c_K, then everything
// k_dense_sym_finish does (dense_finish_tail).  Wave w takes the groups w, w + 4, ... (eight requests of a kilobyte in
// flight per lane), lanes l, l + 16, l + 32, l + 48 are summed by shuffles, the four waves meet in LDS in a fixed order.
__global__ __launch_bounds__(BLOCK) void k_blr_finish(int n, int nt, BlrArgs a, const double *__restrict__ part, DenseFinish fin) {
    __shared__ double shl[BLOCK / WAVE][WAVE];
    __shared__ double shd[BLOCK / WAVE][WAVE];
    if (fin.ctl && !fin.ctl->live) return;  // run-ahead: a dead step does nothing
    const int blk = blockIdx.x, K = blk >> 1, h = blk & 1;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int rr = 4 * (lane & 15), cl = lane >> 4;
    const int i = blk * WAVE + lane;
    const int64_t ldp = (int64_t)nt * DT;
    int bad = 0;
    if (fin.guard && fin.fail_part)
        for (int k = threadIdx.x; k < fin.nfail; k += BLOCK) bad |= fin.fail_part[k];
    const int64_t cb = a.colbase[K];
    const int R = (int)(a.colbase[K + 1] - cb), ng = R / 4;
    const float *__restrict__ Fh = a.F + cb * DT + (int64_t)h * R * WAVE + rr;
    const double *__restrict__ ck = a.coef + cb;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    constexpr int U = 8;
    for (int g0 = w; g0 < ng; g0 += U * (BLOCK / WAVE)) {
        float4 f[U];
        double c[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int g = g0 + k * (BLOCK / WAVE), col = 4 * min(g, ng - 1) + cl;
            f[k] = *reinterpret_cast<const float4 *>(Fh + (int64_t)col * WAVE);
            c[k] = ck[col];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const double cc = g0 + k * (BLOCK / WAVE) < ng ? c[k] : 0.0;
            acc[0] += (double)f[k].x * cc;
            acc[1] += (double)f[k].y * cc;
            acc[2] += (double)f[k].z * cc;
            acc[3] += (double)f[k].w * cc;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[j] += __shfl_xor(acc[j], 16, WAVE);
        acc[j] += __shfl_xor(acc[j], 32, WAVE);
    }
    if (lane < 16)
#pragma unroll
        for (int j = 0; j < 4; ++j) shl[w][rr + j] = acc[j];
    double ds = 0.0;
    if (i < n)
        for (int k = a.dslot_ptr[K] + w; k < a.dslot_ptr[K + 1]; k += BLOCK / WAVE) ds += part[(int64_t)a.dslot[k] * ldp + i];
    shd[w][lane] = ds;
    const int anybad = __syncthreads_or(bad);
    const double v = ((shd[0][lane] + shl[0][lane]) + (shd[1][lane] + shl[1][lane])) +
                     ((shd[2][lane] + shl[2][lane]) + (shd[3][lane] + shl[3][lane]));
    dense_finish_tail(blk, n, v, anybad, fin);
}

// ------------------------------------------------------------------ substructured direct solve
// (tdgl_poisson_set_substructure; host set-up: tdgl_amd/substructure.py)
// Where entry i of a level's vector sits.  MAP, the first level of a preconditioner application (factors.inc:
// precond_direct_apply): at map[i] -- the vector is in the context's order, map[i] = the context's index of the site at
// dissection position i; the values, the products and their order are what they are on a vector in the dissection's order.
template <bool MAP>
__device__ __forceinline__ int64_t vec_at(const int32_t *__restrict__ map, int64_t i) {
    if constexpr (MAP) return map[i];
    else return i;
}
// Way down: out[row] = sum over the row's segments of vals[seg_val ..) . b[seg_x ..): one wavefront per
// row, 8-byte loads (segments start at arbitrary offsets), four independent pairs in flight per lane.
// (MAP: vec_at -- b read through the map, the indices of a batch requested first)
template <class VT, bool MAP = false>
__device__ __forceinline__ void sub_down_row(int64_t row, int lane, const int32_t *__restrict__ seg_ptr,
                                             const int64_t *__restrict__ seg_val, const int32_t *__restrict__ seg_x,
                                             const int32_t *__restrict__ seg_len, const VT *__restrict__ vals,
                                             const double *__restrict__ b, double *__restrict__ out,
                                             const int32_t *__restrict__ map = nullptr) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if constexpr (MAP) {
        for (int k = seg_ptr[row]; k < seg_ptr[row + 1]; ++k) {
            const VT *__restrict__ v = vals + seg_val[k];
            const int32_t *__restrict__ mx = map + seg_x[k];
            const int len = seg_len[k];
            int c = lane;
            for (; c + 3 * WAVE < len; c += 4 * WAVE) {
                const int m0 = mx[c], m1 = mx[c + WAVE], m2 = mx[c + 2 * WAVE], m3 = mx[c + 3 * WAVE];
                const VT v0 = v[c], v1 = v[c + WAVE], v2 = v[c + 2 * WAVE], v3 = v[c + 3 * WAVE];
                const double x0 = b[m0], x1 = b[m1], x2 = b[m2], x3 = b[m3];
                a0 += (double)v0 * x0;
                a1 += (double)v1 * x1;
                a2 += (double)v2 * x2;
                a3 += (double)v3 * x3;
            }
            for (; c < len; c += WAVE) a0 += (double)v[c] * b[mx[c]];
        }
        const double t = wave_sum((a0 + a1) + (a2 + a3));
        if (lane == 0) out[row] = t;
        return;
    }
    for (int k = seg_ptr[row]; k < seg_ptr[row + 1]; ++k) {
        const VT *__restrict__ v = vals + seg_val[k];
        const double *__restrict__ x = b + seg_x[k];
        const int len = seg_len[k];
        int c = lane;
        for (; c + 3 * WAVE < len; c += 4 * WAVE) {
            const VT v0 = v[c], v1 = v[c + WAVE], v2 = v[c + 2 * WAVE], v3 = v[c + 3 * WAVE];
            const double x0 = x[c], x1 = x[c + WAVE], x2 = x[c + 2 * WAVE], x3 = x[c + 3 * WAVE];
            a0 += (double)v0 * x0;
            a1 += (double)v1 * x1;
            a2 += (double)v2 * x2;
            a3 += (double)v3 * x3;
        }
        for (; c < len; c += WAVE) a0 += (double)v[c] * x[c];
    }
    const double t = wave_sum((a0 + a1) + (a2 + a3));
    if (lane == 0) out[row] = t;
}

// The interior rows (G_p b_p: the bulk of the bytes): a workgroup takes a chunk of up to 32 consecutive rows of ONE
// part (SubDownChunk, one 24-byte load instead of the chain row -> part -> offsets), eight rows per wavefront -- the
// rows share the entries of b_p they multiply, and eight rows' worth of loads are in flight per lane.  The other rows
// (separator rows, (G_p 1)^T) follow behind them, one wavefront each, with up to four segments described in ONE
// record (SubDownRow) so that all their loads are requested together; rows with more segments walk the lists.
// A workgroup's life is then two dependent round trips with nothing but the record in flight during the first.
template <class VT>
__device__ __forceinline__ void sub_down_chunk(const SubDownChunk ch, int wv, int lane, const VT *__restrict__ vals,
                                               const double *__restrict__ b, double *__restrict__ out) {
    constexpr int R = 8;
    const int r0 = wv * R;
    if (r0 >= ch.n_rows) return;  // (wave-uniform)
    const int nc = ch.ncols;
    const double *__restrict__ x = b + ch.x0;
    const VT *g[R];
#pragma unroll
    for (int r = 0; r < R; ++r) g[r] = vals + ch.g + (int64_t)min(r0 + r, ch.n_rows - 1) * nc;  // (rows past the end: repeated, not stored)
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    int c = lane;
    for (; c + WAVE < nc; c += 2 * WAVE) {
        const double x0 = x[c], x1 = x[c + WAVE];
        VT u[R], v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            u[r] = g[r][c];
            v[r] = g[r][c + WAVE];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] += (double)u[r] * x0 + (double)v[r] * x1;
    }
    if (c < nc) {
        const double x0 = x[c];
        VT u[R];
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = g[r][c];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] += (double)u[r] * x0;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r0 + r < ch.n_rows) out[ch.row0 + r0 + r] = acc[r];
    }
}

template <class VT>
__global__ __launch_bounds__(BLOCK) void k_sub_down(int64_t nI, int64_t n_rows, int nblk_int, const SubDownChunk *__restrict__ chunks,
                                                    const SubDownRow *__restrict__ rest,
                                                    const int32_t *__restrict__ seg_ptr, const int64_t *__restrict__ seg_val,
                                                    const int32_t *__restrict__ seg_x, const int32_t *__restrict__ seg_len,
                                                    const VT *__restrict__ vals, const double *__restrict__ b,
                                                    double *__restrict__ out, const StepCtl *__restrict__ ctl) {
    if (ctl && !ctl->live) return;  // run-ahead: dead step
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    if ((int)blockIdx.x < nblk_int) {
        sub_down_chunk(chunks[blockIdx.x], wv, lane, vals, b, out);
        return;
    }
    const int64_t row = nI + (blockIdx.x - nblk_int) * (int64_t)(BLOCK / WAVE) + wv;
    if (row >= n_rows) return;
    const SubDownRow d = rest[row - nI];
    if (d.nseg < 0) {  // more than four segments
        sub_down_row(row, lane, seg_ptr, seg_val, seg_x, seg_len, vals, b, out);
        return;
    }
    // the first two tiles of every segment are requested at once (a separator row of the first level: two or three
    // segments of ~100 entries, done with that); longer segments go on in pairs of tiles
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    double pv[4][2], px[4][2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const VT *__restrict__ v = vals + d.val[k];
        const double *__restrict__ x = b + d.x[k];
        const int len = k < d.nseg ? d.len[k] : 0;
        pv[k][0] = lane < len ? (double)v[lane] : 0.0;
        px[k][0] = lane < len ? x[lane] : 0.0;
        pv[k][1] = lane + WAVE < len ? (double)v[lane + WAVE] : 0.0;
        px[k][1] = lane + WAVE < len ? x[lane + WAVE] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a0 += pv[k][0] * px[k][0];
        a1 += pv[k][1] * px[k][1];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int len = k < d.nseg ? d.len[k] : 0;
        if (len <= 2 * WAVE) continue;  // (wave-uniform)
        const VT *__restrict__ v = vals + d.val[k];
        const double *__restrict__ x = b + d.x[k];
        int c = lane + 2 * WAVE;
        for (; c + 3 * WAVE < len; c += 4 * WAVE) {
            const VT v0 = v[c], v1 = v[c + WAVE], v2 = v[c + 2 * WAVE], v3 = v[c + 3 * WAVE];
            const double x0 = x[c], x1 = x[c + WAVE], x2 = x[c + 2 * WAVE], x3 = x[c + 3 * WAVE];
            a0 += (double)v0 * x0;
            a1 += (double)v1 * x1;
            a2 += (double)v2 * x2;
            a3 += (double)v3 * x3;
        }
        for (; c < len; c += WAVE) a2 += (double)v[c] * x[c];
    }
    const double t = wave_sum((a0 + a1) + (a2 + a3));
    if (lane == 0) out[row] = t;
}

// Way up: x_p = w_p - E_p x_S[sep_idx_p] - mean;  x_S = xs - mean (256 separator sites per workgroup, behind the
// interior workgroups).  Nothing is written when the psi update of the step failed.
// E_p is read where the way down reads it: the -E_p^T block of the value pool, [s_p, n_p] row major.  A wavefront takes
// up to 64 consecutive rows of ONE part (SubUpChunk), a LANE per row: for every separator site j the part touches the
// 64 lanes read 64 consecutive entries of row j of -E_p^T -- one contiguous 512-byte request, no reduction across lanes
// -- and multiply by x_S[j], which the wavefront gathered ONCE into LDS.  (History, profiles/EXPERIMENTS.md: gathering
// x_S per row of E_p -- 8 bytes out of a 128-byte line, 10^7 times per solve at 250k sites -- ran into the L2's request
// rate, 41 us for 77 MB; rows of 66 entries read by 16 lanes each, 528-byte rows against 128-byte lines: 33 us for 88 MB.)
// The mean, SubMean: either read from `in` (one number, left there by an earlier launch), or formed here as
// scale_own * (the sum of the terms, one after the other) -- every workgroup adds the few hundred numbers itself, in a
// fixed order (the terms: the first level's (G_p 1)^T b_p rows of the way down, the shares of u . x_S, then the
// (G_p 1)^T b_p rows of every further level; unused terms have n = 0).  Several levels: the inner levels' ways up run
// without a gauge (scale_own = 0) and workgroup 0 of the innermost leaves scale_out * (the sum over ALL levels' shares)
// in `out` for the first level's way up: ~2,000 parts there, too many for every workgroup to add up again.  (factors.inc: mean_*)
constexpr int SUB_MEAN_TERMS = 4;
static_assert(SUB_MEAN_TERMS == SUB_LEVELS_MAX + 1, "a term per level and one for the shares of u . x_S");
struct SubMean {
    struct Term { const double *p; int n; } term[SUB_MEAN_TERMS];
    double scale_own, scale_out;
    double *out;
    const double *in;
};

// sum over j = first, first + NW, ... (j < end) of g[j * stride] * sh[j], a lane per output: every load is one contiguous
// request of the wavefront.  Software-pipelined by hand: the caller requests the FIRST batch of U entries before the
// barrier that makes `sh` valid (strided_prefetch), the loop requests batch k + 1 before it consumes batch k -- the
// chain "descriptor -> values staged in LDS -> barrier -> loads" would otherwise leave the memory pipe idle for a round
// trip per batch (the kernels that use this live for five dependent round trips with ~40 KB in flight per workgroup).
// Indices past the end re-read the last entry (a cache hit) and count as zero.
template <class VT, int U>
__device__ __forceinline__ void strided_prefetch(VT (&cur)[U], const VT *__restrict__ g, int64_t stride, int first, int end) {
    constexpr int NW = BLOCK / WAVE;
    const int last = max(end - 1, 0);
    // (unconditional requests: with `end > 0 ? load : 0` the compiler branched around every pair of loads and waited for
    // them at the joins -- four dependent round trips where one was meant; entry 0 of the block exists for end = 0 too)
#pragma unroll
    for (int t = 0; t < U; ++t) cur[t] = g[(int64_t)min(first + t * NW, last) * stride];
}

template <class VT, int U>
__device__ __forceinline__ double strided_dot(VT (&cur)[U], const VT *__restrict__ g, int64_t stride, int first, int end,
                                              const double *__restrict__ sh) {
    constexpr int NW = BLOCK / WAVE;
    const int last = end - 1;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = first; j < end; j += U * NW) {
        VT nxt[U];
        const int jn = j + U * NW;
        if (jn < end) {  // (wave-uniform)
#pragma unroll
            for (int t = 0; t < U; ++t) nxt[t] = g[(int64_t)min(jn + t * NW, last) * stride];
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {  // (a select, not a branch around the LDS read: sh[last] is always there)
            const int jj = j + t * NW;
            const double w = sh[min(jj, last)];
            a[t & 3] += jj < end ? (double)cur[t] * w : 0.0;
        }
        if (jn < end) {
#pragma unroll
            for (int t = 0; t < U; ++t) cur[t] = nxt[t];
        }
    }
    return (a[0] + a[1]) + (a[2] + a[3]);
}

// ... the same for R chunks of 64 outputs at once (a whole part of up to 64 R rows per workgroup: k_sub_up<VT, R>): entry
// (j, 64 r + lane) for r < R in one batch, so that a wavefront's requests for one j cover the block's row j end to end.
template <class VT, int U, int R>
__device__ __forceinline__ void strided_prefetch_rows(VT (&cur)[R][U], const VT *const (&g)[R], int64_t stride, int first, int end) {
    constexpr int NW = BLOCK / WAVE;
    const int last = max(end - 1, 0);
#pragma unroll
    for (int t = 0; t < U; ++t) {
        const int64_t o = (int64_t)min(first + t * NW, last) * stride;
#pragma unroll
        for (int r = 0; r < R; ++r) cur[r][t] = g[r][o];
    }
}
template <class VT, int U, int R>
__device__ __forceinline__ void strided_dot_rows(double (&acc)[R], VT (&cur)[R][U], const VT *const (&g)[R], int64_t stride, int first,
                                                 int end, const double *__restrict__ sh) {
    constexpr int NW = BLOCK / WAVE;
    const int last = max(end - 1, 0);
    double a[R][2];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r][0] = a[r][1] = 0.0;
    for (int j = first; j < end; j += U * NW) {
        VT nxt[R][U];
        const int jn = j + U * NW;
        if (jn < end) {  // (wave-uniform)
#pragma unroll
            for (int t = 0; t < U; ++t) {
                const int64_t o = (int64_t)min(jn + t * NW, last) * stride;
#pragma unroll
                for (int r = 0; r < R; ++r) nxt[r][t] = g[r][o];
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int jj = j + t * NW;
            const double wgt = jj < end ? sh[min(jj, last)] : 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) a[r][t & 1] += (double)cur[r][t] * wgt;
        }
        if (jn < end) {
#pragma unroll
            for (int t = 0; t < U; ++t)
#pragma unroll
                for (int r = 0; r < R; ++r) cur[r][t] = nxt[r][t];
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = a[r][0] + a[r][1];
}

constexpr int SUB_UP_MAX_SEP = 1024;  // separator sites a part may touch (LDS: 1,024 doubles)
// (R > 1: a chunk is a whole PART of up to 64 R rows -- the levels stored as symmetric tiles, sub_level_to_precond --, its
// separator values gathered once for all of them)
// (MAP: vec_at -- row i is stored at x[map[i]]; every entry of the result is written exactly once, so x needs no other pass)
template <class VT, int R, bool MAP = false>
__global__ __launch_bounds__(BLOCK) void k_sub_up(int64_t nI, int64_t nS, int nblk_int,
                                                  const SubUpChunk *__restrict__ chunks, const int32_t *__restrict__ sep_idx,
                                                  const VT *__restrict__ vals, const double *__restrict__ w,
                                                  const double *__restrict__ xs, SubMean m, const int32_t *__restrict__ fail_part,
                                                  int nfail, double *__restrict__ x, const StepCtl *__restrict__ ctl,
                                                  const int32_t *__restrict__ map) {
    __shared__ double sh_mean;
    __shared__ double sh_xs[SUB_UP_MAX_SEP];
    __shared__ double sh_acc[BLOCK / WAVE][R * WAVE];
    // run-ahead: `live` was decided by this step's psi-update kernel; `poisoned` may have been raised since by
    // this very step's controller (failure: the flags below catch it; end reached: the step itself is accepted)
    if (ctl && !ctl->live) return;
    const bool interior = (int)blockIdx.x < nblk_int;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    // requested before the mean / the failure flags are looked at: the chunk (one per workgroup: its four wavefronts
    // share the chunk's rows and split the part's separator sites among themselves -- a part of 100 rows is two
    // chunks, and at 60k sites the 900 chunks would not even give every CU a wavefront), the separator values
    SubUpChunk ch{0, 0, 0, 0, 0, 0};
    constexpr int U = R == 1 ? 8 : (sizeof(VT) == 4 ? 8 : 4);  // entries requested per lane, row chunk and batch (two batches in flight)
    VT cur[R][U];
    const VT *et[R];
#pragma unroll
    for (int r = 0; r < R; ++r) et[r] = vals;
    double w_row = 0.0;
    [[maybe_unused]] int at = 0;
    if (interior) {
        ch = chunks[blockIdx.x];
        // (the first batch of -E^T entries and w of the row are requested before the separator values are gathered)
#pragma unroll
        for (int r = 0; r < R; ++r) et[r] = vals + ch.et + min(r * WAVE + lane, max(ch.n_rows - 1, 0));  // (-E_p^T)[0][this row]
        strided_prefetch_rows<VT, U, R>(cur, et, ch.np, wv, ch.cnt);
        if ((int)threadIdx.x < ch.n_rows) w_row = w[ch.row0 + threadIdx.x];  // (R * 64 <= BLOCK: thread t finishes row t)
        if constexpr (MAP)
            if ((int)threadIdx.x < ch.n_rows) at = map[ch.row0 + threadIdx.x];  // (... and where it goes, requested with it)
        for (int j = threadIdx.x; j < ch.cnt; j += BLOCK) sh_xs[j] = xs[sep_idx[ch.s0 + j]];
    }
    const bool leader = m.out && blockIdx.x == 0;
    if (!m.in && (m.scale_own != 0.0 || leader)) {  // (workgroup-uniform)
        double v = 0.0;
#pragma unroll
        for (int t = 0; t < SUB_MEAN_TERMS; ++t)
            for (int i = threadIdx.x; i < m.term[t].n; i += BLOCK) v += m.term[t].p[i];
        const double tot = block_sum(v);
        if (threadIdx.x == 0) {
            sh_mean = tot * m.scale_own;
            if (leader) *m.out = tot * m.scale_out;
        }
    } else if (threadIdx.x == 0) {
        sh_mean = m.in ? *m.in : 0.0;
    }
    int bad = 0;
    if (fail_part)
        for (int i = threadIdx.x; i < nfail; i += BLOCK) bad |= fail_part[i];
    const int anybad = __syncthreads_or(bad);  // (also orders sh_xs and sh_mean)
    if (anybad) return;
    const double mean = sh_mean;
    if (!interior) {
        const int64_t i = (blockIdx.x - nblk_int) * (int64_t)BLOCK + threadIdx.x;
        if (i < nS) x[vec_at<MAP>(map, nI + i)] = xs[i] - mean;
        return;
    }
    // wavefront wv: the separator sites wv, wv + 4, ... of the part; lane = row 64 r + lane of the chunk
    double acc_r[R];
    strided_dot_rows<VT, U, R>(acc_r, cur, et, ch.np, wv, ch.cnt, sh_xs);
#pragma unroll
    for (int r = 0; r < R; ++r) sh_acc[wv][r * WAVE + lane] = acc_r[r];
    __syncthreads();
    if ((int)threadIdx.x < ch.n_rows) {
        const int t = threadIdx.x;
        const double acc = (sh_acc[0][t] + sh_acc[1][t]) + (sh_acc[2][t] + sh_acc[3][t]);
        if constexpr (MAP) x[at] = w_row + acc - mean;
        else x[ch.row0 + t] = w_row + acc - mean;  // (the pool holds -E^T)
    }
}

// The way down, a LANE per row (the form the fp32-stored factors use; chunk lists rebuilt by
// tdgl_poisson_set_substructure_precond).  G_p is symmetric, so column r of G_p is row r: for every c the 64 lanes of
// a wavefront read 64 consecutive entries of row c -- one contiguous request, entry (c, r0 + lane) -- and multiply by
// b_p[c], which the workgroup staged in LDS once.  No reduction across lanes (the row-per-wavefront form pays eight
// six-step shuffle reductions for every 8 x 160 entries -- at four bytes per entry they cost more than the loads),
// the four wavefronts of a workgroup split the rows c among themselves and meet in LDS in a fixed order.  Behind the
// chunks: the separator rows that are their identity segment alone (sparse coupling form: out = b, a thread per row),
// then whatever rows are left ((G_p 1)^T: one wavefront each, as in k_sub_down).
constexpr int SUB_DOWN_MAX_COLS = 2048;  // rows of a part's G block the lane form stages b_p for (LDS: 16 KB)
// (MAP: vec_at)
template <class VT, bool MAP = false>
__global__ __launch_bounds__(BLOCK) void k_sub_down_lanes(int64_t nI, int64_t n_ident, int64_t n_rows, int nblk_int, int nblk_ident,
                                                          const SubDownChunk *__restrict__ chunks, const SubDownRow *__restrict__ rest,
                                                          const int32_t *__restrict__ seg_ptr, const int64_t *__restrict__ seg_val,
                                                          const int32_t *__restrict__ seg_x, const int32_t *__restrict__ seg_len,
                                                          const VT *__restrict__ vals, const double *__restrict__ b,
                                                          double *__restrict__ out, const StepCtl *__restrict__ ctl,
                                                          const int32_t *__restrict__ map) {
    __shared__ double sh_b[SUB_DOWN_MAX_COLS];
    __shared__ double sh_acc[BLOCK / WAVE][WAVE];
    if (ctl && !ctl->live) return;  // run-ahead: dead step
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    if ((int)blockIdx.x < nblk_int) {
        const SubDownChunk ch = chunks[blockIdx.x];  // here: g = where entry (0, first row of the chunk) of G_p sits
        const int nc = ch.ncols;
        const bool has_row = lane < ch.n_rows;
        const VT *__restrict__ g = vals + ch.g + (has_row ? lane : 0);
        constexpr int U = 8;
        VT cur[U];
        strided_prefetch<VT, U>(cur, g, ch.ld, wv, nc);  // (before b_p is staged: the two chains run side by side)
        for (int j = threadIdx.x; j < nc; j += BLOCK) sh_b[j] = b[vec_at<MAP>(map, ch.x0 + j)];
        __syncthreads();
        sh_acc[wv][lane] = strided_dot<VT, U>(cur, g, ch.ld, wv, nc, sh_b);
        __syncthreads();
        if (wv == 0 && has_row) out[ch.row0 + lane] = (sh_acc[0][lane] + sh_acc[1][lane]) + (sh_acc[2][lane] + sh_acc[3][lane]);
        return;
    }
    if ((int)blockIdx.x < nblk_int + nblk_ident) {
        const int64_t i = (blockIdx.x - nblk_int) * (int64_t)BLOCK + threadIdx.x;
        if (i < n_ident) out[nI + i] = b[vec_at<MAP>(map, nI + i)];
        return;
    }
    const int64_t row = nI + n_ident + (blockIdx.x - nblk_int - nblk_ident) * (int64_t)(BLOCK / WAVE) + wv;
    if (row >= n_rows) return;
    sub_down_row<VT, MAP>(row, lane, seg_ptr, seg_val, seg_x, seg_len, vals, b, out, map);
}

// The way down on SYMMETRIC storage (round 6; fp32 factors as preconditioner, parts of at most SYM_MAX_ROWS rows): only
// the 16 x 16 tiles on or below the diagonal of G_p are stored (k_sub_repack), 60 % of the block at 140 rows.  One
// workgroup per part.  Its four wavefronts take the tiles pair by pair, one tile per 32-lane half: the half's 32 lanes
// request the tile (8 entries each, requested an iteration ahead), lay it out in LDS with a row stride of 17 (every
// access pattern below is then free of bank conflicts), and use every entry TWICE without any traffic across lanes:
// lanes 0-15 own a ROW r of the tile, y_I[r] += sum_c T[r][c] b_J[c]; lanes 16-31 own a COLUMN c, y_J[c] += sum_r
// T[r][c] b_I[r] (not on the diagonal tiles: they are stored whole).  Every half-wavefront accumulates into an LDS
// array of its own; the eight arrays are added in a fixed order at the end.  b_p sits in LDS.
constexpr int ST = 16;  // edge of a symmetric tile
constexpr int STP = ST + 1;
constexpr int SYM_MAX_ROWS = 256;  // (LDS: 27 KB at most -- eight workgroups a CU)
// LDS written by some lanes of a wavefront and read by others of the SAME wavefront: the hardware keeps a wavefront's LDS
// operations in order; the compiler must not move them across this point
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// (MAP: vec_at)
template <class VT, int D, bool MAP = false>
__global__ __launch_bounds__(BLOCK) void k_sub_down_sym(int64_t nI, int64_t n_ident, int64_t n_rows, int nblk_int, int nblk_ident, int np_lds,
                                                        const SubDownChunk *__restrict__ parts, const int32_t *__restrict__ seg_ptr,
                                                        const int64_t *__restrict__ seg_val, const int32_t *__restrict__ seg_x,
                                                        const int32_t *__restrict__ seg_len, const VT *__restrict__ vals,
                                                        const double *__restrict__ b, double *__restrict__ out,
                                                        const StepCtl *__restrict__ ctl, const int32_t *__restrict__ map) {
    extern __shared__ __align__(16) unsigned char sym_lds[];
    if (ctl && !ctl->live) return;  // run-ahead: dead step
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    if ((int)blockIdx.x < nblk_int) {
        constexpr int NW = BLOCK / WAVE, NH = 2 * NW;  // wavefronts, half-wavefronts
        double *sh_b = reinterpret_cast<double *>(sym_lds);      // [np_lds]
        double *sh_y = sh_b + np_lds;                            // [NH][np_lds]
        VT *sh_t = reinterpret_cast<VT *>(sh_y + NH * np_lds);   // [NH][ST * STP]
        const SubDownChunk ch = parts[blockIdx.x];  // (g: where the part's tiles start, ncols: its rows)
        const int np = ch.ncols, nt = (np + ST - 1) / ST, ntiles = nt * (nt + 1) / 2, npairs = (ntiles + 1) / 2;
        const int half = lane >> 5, l = lane & 31;
        auto tile_of = [&](int t, int &I, int &J) {
            I = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f);
            while ((I + 1) * (I + 2) / 2 <= t) ++I;
            while (I * (I + 1) / 2 > t) --I;
            J = t - I * (I + 1) / 2;
        };
        // the first D pairs' entries are requested before b_p is staged; afterwards pair k + D as soon as pair k sits in LDS
        VT buf[D][8];
        auto request = [&](VT(&dst)[8], int pr) {
            const VT *__restrict__ src = vals + ch.g + (int64_t)min(2 * pr + half, ntiles - 1) * (ST * ST) + 8 * l;
#pragma unroll
            for (int i = 0; i < 8; ++i) dst[i] = src[i];
        };
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (wv + d * NW < npairs) request(buf[d], wv + d * NW);  // (wave-uniform)
        for (int j = threadIdx.x; j < np_lds; j += BLOCK) sh_b[j] = j < np ? b[vec_at<MAP>(map, ch.x0 + j)] : 0.0;
        for (int j = threadIdx.x; j < NH * np_lds; j += BLOCK) sh_y[j] = 0.0;
        __syncthreads();
        double *my_y = sh_y + (size_t)(wv * 2 + half) * np_lds;
        VT *my_t = sh_t + (size_t)(wv * 2 + half) * (ST * STP);
        const bool is_row = l < ST;  // lanes 0-15: row l of the tile against b_J; lanes 16-31: column l - 16 against b_I
        const VT *tp = my_t + (is_row ? l * STP : l - ST);
        const int stride = is_row ? 1 : STP;
        VT *stage = my_t + (l >> 1) * STP + 8 * (l & 1);  // entries 8 l .. 8 l + 7 of a tile: row l / 2, columns 8 (l % 2) ...
        for (int pr0 = wv; pr0 < npairs; pr0 += D * NW) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int pr = pr0 + d * NW;
                if (pr >= npairs) break;  // (wave-uniform)
                const int t = 2 * pr + half;
                const bool valid = t < ntiles;
                int I = 0, J = 0;
                tile_of(valid ? t : 0, I, J);
#pragma unroll
                for (int i = 0; i < 8; ++i) stage[i] = buf[d][i];
                if (pr + D * NW < npairs) request(buf[d], pr + D * NW);
                wave_lds_sync();  // (the tile was written by other lanes of this wavefront)
                const double *bp = sh_b + (is_row ? J : I) * ST;
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < ST; ++k) acc += (double)tp[k * stride] * bp[k];
                if (valid && (is_row || I != J)) my_y[(is_row ? I : J) * ST + (l & (ST - 1))] += acc;
                wave_lds_sync();  // (before the next tile overwrites this one)
            }
        }
        __syncthreads();
        for (int r = threadIdx.x; r < np; r += BLOCK) {
            double v = 0.0;
#pragma unroll
            for (int h = 0; h < NH; ++h) v += sh_y[(size_t)h * np_lds + r];
            out[ch.row0 + r] = v;
        }
        return;
    }
    if ((int)blockIdx.x < nblk_int + nblk_ident) {
        const int64_t i = (blockIdx.x - nblk_int) * (int64_t)BLOCK + threadIdx.x;
        if (i < n_ident) out[nI + i] = b[vec_at<MAP>(map, nI + i)];
        return;
    }
    const int64_t row = nI + n_ident + (blockIdx.x - nblk_int - nblk_ident) * (int64_t)(BLOCK / WAVE) + wv;
    if (row >= n_rows) return;
    sub_down_row<VT, MAP>(row, lane, seg_ptr, seg_val, seg_x, seg_len, vals, b, out, map);
}

// fp64 pool -> fp32 pool with every row of every G_p / -E_p^T block starting on a 64-byte line (row stride ld = np rounded
// up to 16 floats, block bases multiples of 16): the lane-per-row kernels read a chunk of a row per request, and with
// rows of 160 floats packed back to back (and the pool's leading 1.0 shifting everything by four bytes) every request
// ended inside a line that the neighbouring chunk's workgroup fetched again -- 1.34 x the algorithmic bytes on the way
// down, 1.6 x on the way up (PMC, profiles/r08g_pmc_hbm_traffic_1M.txt).  One workgroup per part.
// (d.pad != 0: the G block goes out as the 16 x 16 tiles on or below its diagonal instead -- k_sub_down_sym --, tile
// (I, J) at new_g + (I (I + 1) / 2 + J) * 256, row major, zero beyond the block)
template <class DT>
__global__ __launch_bounds__(BLOCK) void k_sub_repack(const SubRepack *__restrict__ parts, const double *__restrict__ src, DT *__restrict__ dst) {
    const SubRepack d = parts[blockIdx.x];
    const int64_t ng = (int64_t)d.np * d.np, ne = (int64_t)d.sp * d.np;
    if (d.pad) {
        const int nt = (d.np + ST - 1) / ST;
        const int64_t total = (int64_t)nt * (nt + 1) / 2 * ST * ST;
        for (int64_t i = threadIdx.x; i < total; i += BLOCK) {
            const int t = (int)(i / (ST * ST)), e = (int)(i % (ST * ST));
            int I = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f);
            while ((I + 1) * (I + 2) / 2 <= t) ++I;
            while (I * (I + 1) / 2 > t) --I;
            const int J = t - I * (I + 1) / 2;
            const int r = I * ST + e / ST, c = J * ST + e % ST;
            dst[d.new_g + i] = (r < d.np && c < d.np) ? (DT)src[d.old_g + (int64_t)r * d.np + c] : (DT)0;
        }
    } else
    for (int64_t i = threadIdx.x; i < ng; i += BLOCK) {
        const int64_t r = i / d.np, c = i % d.np;
        dst[d.new_g + r * d.ld + c] = (DT)src[d.old_g + i];
    }
    for (int64_t i = threadIdx.x; i < ne; i += BLOCK) {
        const int64_t r = i / d.np, c = i % d.np;
        dst[d.new_et + r * d.ld + c] = (DT)src[d.old_et + i];
    }
}

// ------------------------------------------------------------------ the substructure factors as the CG's preconditioner
// (tdgl_poisson_set_substructure_precond; factors.inc: precond_direct_apply).  The context keeps its reverse
// Cuthill-McKee site order -- the order the stencil kernels and the AMG hierarchy are fastest in --, the dissection's
// order exists inside the solve only: `map[i]` = the context's index of the site at dissection position i.
__global__ __launch_bounds__(BLOCK) void k_pd_gather(int64_t n, const int32_t *__restrict__ map, const double *__restrict__ r,
                                                     double *__restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) out[i] = r[map[i]];
}

// z[map[i]] = x[i], and the partials of r . z on the kernel's own fixed grid (summed by the consumer in a fixed order)
__global__ __launch_bounds__(BLOCK) void k_pd_scatter(int64_t n, const int32_t *__restrict__ map, const double *__restrict__ x,
                                                      const double *__restrict__ r, double *__restrict__ z,
                                                      double *__restrict__ rz_part) {
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const int j = map[i];
        const double v = x[i];
        z[j] = v;
        acc += r[j] * v;
    }
    const double t = block_sum(acc);
    if (threadIdx.x == 0) rz_part[blockIdx.x] = t;
}

__global__ __launch_bounds__(BLOCK) void k_to_float(int64_t n, const double *__restrict__ src, float *__restrict__ dst) {
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) dst[i] = (float)src[i];
}

}  // namespace tdgl
