// Set-up of the direct mu solve on the device (tdgl_poisson_build_dense_inverse).  Included by tdgl_hip.hip
// after poisson.inc (the application of what it sets up: factors.inc).
//
// The counterpart of the reference's one-off LU factorisation (tdgl/finite_volume/operators.py:305-308)
// for meshes small enough for the explicit pseudo-inverse (see tdgl_poisson_set_dense_inverse).  The
// dense matrix M = A + (s / n) 1 1^T (A = the level-0 Poisson matrix already resident as SELL-64,
// s = its mean diagonal) is assembled on the device and inverted in place by a blocked symmetric sweep
// (Gauss-Jordan without pivoting, which a positive definite matrix does not need), then packed into the
// symmetric tile layout k_dense_sym_tiles streams, with the rank-one term removed again on the way:
//   (A + (s/n) 1 1^T)^-1 = pinv(A) + 1 1^T / (s n)      (A symmetric, A 1 = 0).
//
// Symmetric sweep on the pivot block K (GB = 64 rows): with P = M[:, K] and D = M[K, K]^-1,
//   M[K, K] <- -D,   M[i, K] <- W = P D,   M[i, j] <- M[i, j] - W_i P_j^T   (i, j outside K);
// every intermediate matrix is symmetric (only tiles on or below the diagonal are kept), the part not yet
// swept is the Schur complement (positive definite), and after all blocks M = -(M_0)^-1.  Two launches
// per block: k_gj_panel (every workgroup inverts the 64 x 64 pivot block in LDS for itself -- 64
// dependent steps, cheaper than a separate launch -- and forms its 64 rows of W) and k_gj_update (one
// 64 x 64 tile per workgroup, both panels staged transposed in LDS, 4 x 4 outputs per thread: plain fp64
// FMAs -- the matrix cores of gfx950 run fp64 at the vector rate).  2 n^3 / 2 flops and n / 64 passes over
// the lower triangle: ~0.1 s at 5.8k sites, ~1 s at 16k, nothing leaves the device.  (The ROCm
// library route, rocSOLVER dpotrf + dpotri, was measured too: 0.03-0.1 s per matrix once loaded, but
// loading its 0.9 GB shared object takes seconds to minutes on a cold file cache -- not acceptable for
// a set-up step of a 5k-site simulation.)

namespace tdgl {

constexpr int GB = 64;        // pivot block / tile edge of the sweep
constexpr int GLD = GB + 2;   // leading dimension of the transposed panels in LDS (even: 16-byte reads)

// M[r][c] = shift for r, c < n; identity on the padding [n, N)
__global__ __launch_bounds__(BLOCK) void k_dense_fill(int64_t n, int64_t N, double shift, double *__restrict__ M) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i >= N * N) return;
    const int64_t r = i / N, c = i % N;
    M[i] = (r < n && c < n) ? shift : (r == c ? 1.0 : 0.0);
}

// M[r][c] += A_rc from the SELL-64 matrix: one lane per row, so every entry of M has one writer
// (padding slots repeat a column of the row with value 0)
__global__ __launch_bounds__(BLOCK) void k_dense_scatter_sell(int n_slices, int64_t n_rows, const int32_t *__restrict__ slice_off,
                                                              const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                              int64_t ld, double *__restrict__ M) {
    const int slice = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
    if (slice >= n_slices) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t row = (int64_t)slice * WAVE + lane;
    if (row >= n_rows) return;
    int64_t idx = (int64_t)slice_off[slice] * WAVE + lane;
    for (int k = slice_off[slice]; k < slice_off[slice + 1]; ++k, idx += WAVE) M[row * ld + cols[idx]] += vals[idx];
}

// the mean diagonal comes from dinv (1 / A_ii)
__global__ __launch_bounds__(BLOCK) void k_sum_inverse(int64_t n, const double *__restrict__ dinv, double *__restrict__ out) {
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += BLOCK) v += 1.0 / dinv[i];
    const double t = block_sum(v);
    if (threadIdx.x == 0) out[0] = t;
}

// Panel of sweep step k: workgroup r owns the rows of block r.  P = M[r-block, K] (read from the lower
// triangle: directly for r > k, transposed from M[K, r-block] for r < k), W = P D with D = M[K, K]^-1
// inverted here in LDS by an unblocked symmetric sweep.  Writes Pbuf / Wbuf [N][GB]; workgroup r == k
// writes D to Dbuf instead.  flag[0] is raised when a pivot is not positive (not positive definite).
__device__ __forceinline__ void gj_panel_body(int r, int64_t N, int k, const double *__restrict__ M, double *__restrict__ Pbuf,
                                              double *__restrict__ Wbuf, double *__restrict__ Dbuf,
                                              int32_t *__restrict__ flag) {
    __shared__ double D[GB][GB + 1];
    __shared__ double Ps[GB / 2][GB];  // (rows of P in two halves: static LDS is limited to 64 KB)
    __shared__ double colp[GB];
    const int t = threadIdx.x;
    const int64_t k0 = (int64_t)k * GB, r0 = (int64_t)r * GB;
    // pivot block: lower triangle of M[K, K], mirrored
    for (int e = t; e < GB * GB; e += BLOCK) {
        const int i = e / GB, j = e % GB;
        D[i][j] = M[(k0 + (i > j ? i : j)) * N + k0 + (i > j ? j : i)];
    }
    __syncthreads();
    // symmetric sweep of all 64 pivots: D <- -D^-1
    int bad = 0;
    for (int p = 0; p < GB; ++p) {
        const double d = D[p][p];
        if (!(d > 0.0)) bad = 1;
        if (t < GB) colp[t] = D[t][p];
        __syncthreads();
        const double inv = 1.0 / d;
        for (int e = t; e < GB * GB; e += BLOCK) {
            const int i = e / GB, j = e % GB;
            double v;
            if (i == p && j == p) v = -inv;
            else if (i == p) v = colp[j] * inv;
            else if (j == p) v = colp[i] * inv;
            else v = D[i][j] - colp[i] * colp[j] * inv;
            D[i][j] = v;
        }
        __syncthreads();
    }
    if (bad && t == 0) flag[0] = 1;
    if (r == k) {
        for (int e = t; e < GB * GB; e += BLOCK) Dbuf[e] = -D[e / GB][e % GB];  // + M[K, K]^-1
        return;
    }
    // W = P * (M[K, K]^-1) = -P * D, 32 rows at a time; 8 outputs per thread and half
    for (int h = 0; h < 2; ++h) {
        __syncthreads();
        for (int e = t; e < GB * GB / 2; e += BLOCK) {
            const int i = e / GB, j = e % GB, gi = h * (GB / 2) + i;  // P[gi][j] = M[r0 + gi][k0 + j]
            Ps[i][j] = r > k ? M[(r0 + gi) * N + k0 + j] : M[(k0 + j) * N + r0 + gi];
        }
        __syncthreads();
        for (int e = t; e < GB * GB / 2; e += BLOCK) {
            const int i = e / GB, j = e % GB, gi = h * (GB / 2) + i;
            double acc = 0.0;
#pragma unroll 8
            for (int b = 0; b < GB; ++b) acc += Ps[i][b] * D[b][j];
            Wbuf[(r0 + gi) * GB + j] = -acc;
            Pbuf[(r0 + gi) * GB + j] = Ps[i][j];
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_gj_panel(int64_t N, int k, const double *__restrict__ M, double *__restrict__ Pbuf,
                                                    double *__restrict__ Wbuf, double *__restrict__ Dbuf,
                                                    int32_t *__restrict__ flag) {
    gj_panel_body(blockIdx.x, N, k, M, Pbuf, Wbuf, Dbuf, flag);
}

// Update of sweep step k on tile (I, J), J <= I (one workgroup each):
//   I == J == k: -D;   J == k: W_I;   I == k: W_J^T;   otherwise M_IJ -= W_I P_J^T.
__device__ __forceinline__ void gj_update_body(int tt, int64_t N, int k, double *__restrict__ M, const double *__restrict__ Pbuf,
                                               const double *__restrict__ Wbuf, const double *__restrict__ Dbuf) {
    __shared__ double Ws[GB / 2][GLD];  // [b][i], b in halves of 32 (static LDS: 64 KB)
    __shared__ double Pt[GB / 2][GLD];  // [b][j]
    int I = (int)((sqrt(8.0 * tt + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= tt) ++I;
    while (I * (I + 1) / 2 > tt) --I;
    const int J = tt - I * (I + 1) / 2;
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)I * GB, j0 = (int64_t)J * GB;
    if (I == k || J == k) {  // (workgroup-uniform)
        for (int e = t; e < GB * GB; e += BLOCK) {
            const int i = e / GB, j = e % GB;
            double v;
            if (I == k && J == k) v = -Dbuf[e];
            else if (J == k) v = Wbuf[(i0 + i) * GB + j];
            else v = Wbuf[(j0 + j) * GB + i];
            M[(i0 + i) * N + j0 + j] = v;
        }
        return;
    }
    const double2 *__restrict__ w2 = reinterpret_cast<const double2 *>(Wbuf + i0 * GB);
    const double2 *__restrict__ p2 = reinterpret_cast<const double2 *>(Pbuf + j0 * GB);
    const int ty = t / 16, tx = t % 16;  // rows 4 ty .. 4 ty + 3, columns 4 tx .. 4 tx + 3
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;
    for (int h = 0; h < 2; ++h) {
        __syncthreads();
        // stage both panels transposed: a thread reads 16-byte pieces along b and stores [b][row]
#pragma unroll
        for (int q = 0; q < GB * GB / 4 / BLOCK; ++q) {
            const int e = t + q * BLOCK, row = e / (GB / 4), b = 2 * (e % (GB / 4));
            const double2 a = w2[row * (GB / 2) + h * (GB / 4) + e % (GB / 4)], c = p2[row * (GB / 2) + h * (GB / 4) + e % (GB / 4)];
            Ws[b][row] = a.x;
            Ws[b + 1][row] = a.y;
            Pt[b][row] = c.x;
            Pt[b + 1][row] = c.y;
        }
        __syncthreads();
#pragma unroll 4
        for (int b = 0; b < GB / 2; ++b) {
            const double2 wa = *reinterpret_cast<const double2 *>(&Ws[b][4 * ty]), wb = *reinterpret_cast<const double2 *>(&Ws[b][4 * ty + 2]);
            const double2 pa = *reinterpret_cast<const double2 *>(&Pt[b][4 * tx]), pb = *reinterpret_cast<const double2 *>(&Pt[b][4 * tx + 2]);
            const double w[4] = {wa.x, wa.y, wb.x, wb.y}, p[4] = {pa.x, pa.y, pb.x, pb.y};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] += w[a] * p[c];
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        double2 *__restrict__ dst = reinterpret_cast<double2 *>(M + (i0 + 4 * ty + a) * N + j0 + 4 * tx);
        double2 u = dst[0], v = dst[1];
        u.x -= acc[a][0];
        u.y -= acc[a][1];
        v.x -= acc[a][2];
        v.y -= acc[a][3];
        dst[0] = u;
        dst[1] = v;
    }
}

__global__ __launch_bounds__(BLOCK) void k_gj_update(int64_t N, int k, double *__restrict__ M, const double *__restrict__ Pbuf,
                                                     const double *__restrict__ Wbuf, const double *__restrict__ Dbuf) {
    gj_update_body(blockIdx.x, N, k, M, Pbuf, Wbuf, Dbuf);
}

// The same two steps for a BATCH of independent matrices (the interior blocks of the substructured solve):
// blockIdx.y = matrix; matrix q has nbq[q] pivot blocks and lives at M + moff[q], its panels at
// P/Wbuf + poff[q], its pivot inverse at Dbuf + q * GB * GB.  Workgroups beyond a matrix's size leave.
__global__ __launch_bounds__(BLOCK) void k_gj_panel_batch(int k, const int32_t *__restrict__ nbq, const int64_t *__restrict__ moff,
                                                          const int64_t *__restrict__ poff, const double *__restrict__ M,
                                                          double *__restrict__ Pbuf, double *__restrict__ Wbuf,
                                                          double *__restrict__ Dbuf, int32_t *__restrict__ flag) {
    const int q = blockIdx.y, nb = nbq[q];
    if (k >= nb || (int)blockIdx.x >= nb) return;
    gj_panel_body(blockIdx.x, (int64_t)nb * GB, k, M + moff[q], Pbuf + poff[q], Wbuf + poff[q], Dbuf + (int64_t)q * GB * GB, flag);
}

__global__ __launch_bounds__(BLOCK) void k_gj_update_batch(int k, const int32_t *__restrict__ nbq, const int64_t *__restrict__ moff,
                                                           const int64_t *__restrict__ poff, double *__restrict__ M,
                                                           const double *__restrict__ Pbuf, const double *__restrict__ Wbuf,
                                                           const double *__restrict__ Dbuf) {
    const int q = blockIdx.y, nb = nbq[q];
    if (k >= nb || (int)blockIdx.x >= nb * (nb + 1) / 2) return;
    gj_update_body(blockIdx.x, (int64_t)nb * GB, k, M + moff[q], Pbuf + poff[q], Wbuf + poff[q], Dbuf + (int64_t)q * GB * GB);
}

// Symmetric tile packing for k_dense_sym_tiles: tile (I, J), J <= I, of DT x DT entries; entry (r, c) =
// -Msw[max(r, c)][min(r, c)] - shift_out (Msw = the swept matrix = -(M_0)^-1, lower triangle valid), zero beyond n.
__global__ __launch_bounds__(BLOCK) void k_dense_pack_sym(int64_t n, int64_t N, const double *__restrict__ Msw,
                                                          double shift_out, double *__restrict__ Gp) {
    const int t = blockIdx.x;
    int I = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    while (I * (I + 1) / 2 > t) --I;
    const int J = t - I * (I + 1) / 2;
    double *__restrict__ dst = Gp + (int64_t)t * DT * DT;
    for (int e = threadIdx.x; e < DT * DT; e += BLOCK) {
        const int64_t r = (int64_t)I * DT + e / DT, c = (int64_t)J * DT + e % DT;
        double v = 0.0;
        if (r < n && c < n) v = -Msw[(r > c ? r : c) * N + (r > c ? c : r)] - shift_out;
        dst[e] = v;
    }
}

}  // namespace tdgl

// M [N x N] (N = a multiple of GB, identity on the padding) -> symmetric tiles of -(swept M)[:n, :n] - shift_out
// in D, with the work array of k_dense_sym_tiles / _finish
static int dense_sweep_pack(tdgl_ctx *ctx, DevBuf<double> &M, int64_t n, int64_t N, double shift_out, DenseTiles &D) {
    const int nb = (int)(N / GB);
    DevBuf<double> Pbuf, Wbuf, Dbuf;
    DevBuf<int32_t> d_flag;
    HIP_TRY(ctx, Pbuf.alloc((size_t)N * GB, false));
    HIP_TRY(ctx, Wbuf.alloc((size_t)N * GB, false));
    HIP_TRY(ctx, Dbuf.alloc((size_t)GB * GB, false));
    HIP_TRY(ctx, d_flag.alloc(1));
    const unsigned tri = (unsigned)((int64_t)nb * (nb + 1) / 2);
    for (int k = 0; k < nb; ++k) {
        hipLaunchKernelGGL(k_gj_panel, dim3(nb), dim3(BLOCK), 0, ctx->stream, N, k, (const double *)M.p, Pbuf.p, Wbuf.p, Dbuf.p, d_flag.p);
        hipLaunchKernelGGL(k_gj_update, dim3(tri), dim3(BLOCK), 0, ctx->stream, N, k, M.p, (const double *)Pbuf.p,
                           (const double *)Wbuf.p, (const double *)Dbuf.p);
    }
    HIP_TRY(ctx, hipGetLastError());
    int32_t flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, d_flag.p, sizeof(flag), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flag)
        TDGL_FAIL(ctx, TDGL_ERR_ARG,
                  "dense inverse: the matrix is not positive definite on the complement of the constants"
                  " (a mesh in several pieces?)");
    const int nt = (int)((n + DT - 1) / DT);
    const size_t tiles = (size_t)nt * (nt + 1) / 2;
    HIP_TRY(ctx, D.G.alloc(tiles * DT * DT, false));
    hipLaunchKernelGGL(k_dense_pack_sym, dim3((unsigned)tiles), dim3(BLOCK), 0, ctx->stream, n, N, (const double *)M.p, shift_out,
                       D.G.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, D.part.alloc((size_t)nt * nt * DT));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    D.tiles = nt;
    D.n = n;
    return TDGL_OK;
}

// the tiles in fp32 (G released)
static int dense_to_fp32(tdgl_ctx *ctx, DenseTiles &D) {
    HIP_TRY(ctx, D.G32.alloc(std::max<size_t>(D.G.n, 1), false));
    if (D.G.n > 0)
        hipLaunchKernelGGL(k_to_float, dim3(vec_grid((int64_t)D.G.n)), dim3(BLOCK), 0, ctx->stream, (int64_t)D.G.n, (const double *)D.G.p,
                           D.G32.p);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    D.G.release();
    return TDGL_OK;
}

extern "C" int tdgl_poisson_build_dense_inverse(tdgl_ctx *ctx, double *seconds) {
    CTX_GUARD(ctx);
    if (distributed(ctx)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_dense_inverse: single-GPU contexts only");
    if (ctx->levels.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_poisson_build_dense_inverse: set the hierarchy first");
    const int64_t n = ctx->n;
    if (n < 2 || n > 46000) TDGL_FAIL(ctx, TDGL_ERR_ARG, "dense inverse: %lld sites is outside what a dense matrix is meant for", (long long)n);
    const int64_t t_begin = now_ns();
    AmgLevel &L0 = *ctx->levels[0];
    // s = mean diagonal of A: the added eigenvalue sits inside the spectrum
    DevBuf<double> d_s;
    HIP_TRY(ctx, d_s.alloc(1));
    hipLaunchKernelGGL(k_sum_inverse, dim3(1), dim3(BLOCK), 0, ctx->stream, n, (const double *)L0.dinv.p, d_s.p);
    double s = 0.0;
    HIP_TRY(ctx, hipMemcpyAsync(&s, d_s.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    s /= (double)n;
    if (!(s > 0.0) || !std::isfinite(s)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "dense inverse: the Poisson matrix has a non-positive mean diagonal");
    const int64_t N = round_up(n, GB);
    DevBuf<double> M;
    HIP_TRY(ctx, M.alloc((size_t)N * N, false));
    hipLaunchKernelGGL(k_dense_fill, dim3(grid_for(N * N)), dim3(BLOCK), 0, ctx->stream, n, N, s / (double)n, M.p);
    const SellPattern &pat = L0.A.pat;
    hipLaunchKernelGGL(k_dense_scatter_sell, dim3(grid_for((int64_t)pat.n_slices * WAVE)), dim3(BLOCK), 0, ctx->stream,
                       pat.n_slices, n, pat.slice_off.p, pat.cols.p, L0.A.vals.p, N, M.p);
    auto f = std::make_unique<DirectFactors>();
    TDGL_TRY(dense_sweep_pack(ctx, M, n, N, 1.0 / (s * (double)n), f->dense));
    f->ld = round_up(n, 2);
    ctx->direct = std::move(f);
    if (seconds) *seconds = (double)(now_ns() - t_begin) * 1e-9;
    return TDGL_OK;
}

// ---------------------------------------------------------------------------------------------------
// Substructured direct solve (include/tdgl_hip.h: tdgl_substructure)
namespace tdgl {
// M[r][c] = src[r][c] + shift for r, c < n (src row major [n, n]); identity on the padding
__global__ __launch_bounds__(BLOCK) void k_dense_from(int64_t n, int64_t N, double shift, const double *__restrict__ src,
                                                      double *__restrict__ M) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i >= N * N) return;
    const int64_t r = i / N, c = i % N;
    M[i] = (r < n && c < n) ? src[r * n + c] + shift : (r == c ? 1.0 : 0.0);
}
}  // namespace tdgl

// a CSR-like offset array of n entries (n + 1 offsets): from 0, never decreasing
static bool offsets_ok(const int32_t *ptr, int64_t n) {
    if (ptr[0] != 0) return false;
    for (int64_t i = 0; i < n; ++i)
        if (ptr[i + 1] < ptr[i]) return false;
    return true;
}

// The way up's work list (k_sub_up): chunks of <= 64 rows of one part, a wavefront each, reading the part's -E_p^T
// block of the value pool (et_off[p]: [s_p, n_p] row major).
static int sub_upload_chunks(tdgl_ctx *ctx, int P, const int32_t *part_ptr, const int32_t *sep_ptr, const int64_t *et_off,
                             tdgl::DevBuf<tdgl::SubUpChunk> &dst, const char *who) {
    std::vector<tdgl::SubUpChunk> chunks;
    for (int p = 0; p < P; ++p) {
        const int32_t cnt = sep_ptr[p + 1] - sep_ptr[p], np_ = part_ptr[p + 1] - part_ptr[p];
        if (cnt > tdgl::SUB_UP_MAX_SEP)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: part %d touches %d separator sites (at most %d are supported: use smaller parts)", who, p,
                      (int)cnt, tdgl::SUB_UP_MAX_SEP);
        for (int32_t r = part_ptr[p]; r < part_ptr[p + 1]; r += WAVE)
            chunks.push_back(tdgl::SubUpChunk{et_off[p] + (r - part_ptr[p]), np_, sep_ptr[p], cnt, r,
                                              std::min<int32_t>(WAVE, part_ptr[p + 1] - r)});
    }
    if (chunks.empty()) chunks.push_back(tdgl::SubUpChunk{0, 0, 0, 0, 0, 0});
    HIP_TRY(ctx, dst.upload(chunks));
    return TDGL_OK;
}

// The way down's work lists (k_sub_down): chunks of <= 32 interior rows of one part, and the remaining rows with
// their (up to four) segments inline.
static int sub_upload_down_lists(tdgl_ctx *ctx, int P, int64_t n_rows, const int32_t *part_ptr, const int64_t *g_off,
                                 const int32_t *seg_ptr, const int64_t *seg_val, const int32_t *seg_x, const int32_t *seg_len,
                                 tdgl::DevBuf<tdgl::SubDownChunk> &chunks, tdgl::DevBuf<tdgl::SubDownRow> &rows) {
    std::vector<tdgl::SubDownChunk> ch;
    for (int p = 0; p < P; ++p) {
        const int32_t np_ = part_ptr[p + 1] - part_ptr[p];
        for (int32_t r = part_ptr[p]; r < part_ptr[p + 1]; r += 32)
            ch.push_back(tdgl::SubDownChunk{g_off[p] + (int64_t)(r - part_ptr[p]) * np_, part_ptr[p], np_, r,
                                            std::min<int32_t>(32, part_ptr[p + 1] - r), np_, 0});
    }
    if (ch.empty()) ch.push_back(tdgl::SubDownChunk{0, 0, 0, 0, 0, 0, 0});
    const int64_t nI = part_ptr[P];
    std::vector<tdgl::SubDownRow> rr((size_t)std::max<int64_t>(n_rows - nI, 1));
    for (int64_t row = nI; row < n_rows; ++row) {
        tdgl::SubDownRow d{};
        const int k0 = seg_ptr[row], ns = seg_ptr[row + 1] - k0;
        d.nseg = ns <= 4 ? ns : -1;
        for (int k = 0; k < 4; ++k) {
            const bool in = k < ns && ns <= 4;
            d.val[k] = in ? seg_val[k0 + k] : 0;
            d.x[k] = in ? seg_x[k0 + k] : 0;
            d.len[k] = in ? seg_len[k0 + k] : 0;
        }
        rr[(size_t)(row - nI)] = d;
    }
    HIP_TRY(ctx, chunks.upload(ch));
    HIP_TRY(ctx, rows.upload(rr));
    return TDGL_OK;
}

// Everything of one level except the dense matrix: checks, index arrays, value pools, into a level under construction.
// `n` = length of the vector the level works on (the site count, a rank's interior, or the previous level's separator).
static int sub_upload_level(tdgl_ctx *ctx, const tdgl_substructure *sub, int64_t n, SubLevel &d, const char *who) {
    const int64_t nI = sub->n_interior, nS = sub->n_sep;
    const int P = sub->n_parts;
    if (nI + nS != n || P < 1 || nS < 2 || !sub->part_ptr || !sub->seg_ptr || !sub->seg_val || !sub->seg_x ||
        !sub->seg_len || !sub->vals || !sub->sep_ptr || !sub->sep_idx || !sub->e_off || !sub->e_vals || !sub->u)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: inconsistent description (n_interior + n_sep must be the length of the level's vector)", who);
    if (sub->part_ptr[0] != 0 || sub->part_ptr[P] != nI)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: part_ptr must run from 0 to n_interior", who);
    const int64_t n_rows = n + P;
    if (!offsets_ok(sub->seg_ptr, n_rows) || !offsets_ok(sub->sep_ptr, P))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: seg_ptr and sep_ptr must run from 0 and not decrease", who);
    const int64_t n_seg = sub->seg_ptr[n_rows];
    for (int64_t k = 0; k < n_seg; ++k)
        if (sub->seg_len[k] < 0 || sub->seg_val[k] < 0 || sub->seg_val[k] + sub->seg_len[k] > sub->n_vals || sub->seg_x[k] < 0 ||
            (int64_t)sub->seg_x[k] + sub->seg_len[k] > n)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: segment %lld out of range", who, (long long)k);
    std::vector<int32_t> row_part(nI);
    for (int p = 0; p < P; ++p) {
        if (sub->part_ptr[p + 1] < sub->part_ptr[p]) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: part_ptr must not decrease", who);
        for (int64_t r = sub->part_ptr[p]; r < sub->part_ptr[p + 1]; ++r) row_part[r] = p;
        const int64_t cnt = sub->sep_ptr[p + 1] - sub->sep_ptr[p], rows = sub->part_ptr[p + 1] - sub->part_ptr[p];
        if (cnt < 0 || sub->e_off[p] < 0 || sub->e_off[p] + rows * cnt > sub->n_e)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: E block of part %d out of range", who, p);
    }
    const int64_t n_sidx = sub->sep_ptr[P];
    for (int64_t k = 0; k < n_sidx; ++k)
        if (sub->sep_idx[k] < 0 || sub->sep_idx[k] >= nS) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: separator index out of range", who);
    // the G_p blocks open the value pool (behind the leading 1.0), row major, part after part: where
    // k_sub_down's four-rows-per-wavefront path reads them; the row segments must say the same
    std::vector<int64_t> g_off(P);
    {
        int64_t off = 1;
        for (int p = 0; p < P; ++p) {
            g_off[p] = off;
            const int64_t rows = sub->part_ptr[p + 1] - sub->part_ptr[p];
            for (int64_t r = 0; r < rows; ++r) {
                const int64_t row = sub->part_ptr[p] + r, k = sub->seg_ptr[row];
                if (sub->seg_ptr[row + 1] != k + 1 || sub->seg_val[k] != off + r * rows || sub->seg_x[k] != sub->part_ptr[p] || sub->seg_len[k] != rows)
                    TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: interior row %lld is not a row of its part's G block", who, (long long)row);
            }
            off += rows * rows;
        }
    }
    HIP_TRY(ctx, d.part_ptr.upload(std::vector<int32_t>(sub->part_ptr, sub->part_ptr + P + 1)));
    HIP_TRY(ctx, d.seg_ptr.upload(std::vector<int32_t>(sub->seg_ptr, sub->seg_ptr + n_rows + 1)));
    HIP_TRY(ctx, d.seg_val.upload(std::vector<int64_t>(sub->seg_val, sub->seg_val + n_seg)));
    HIP_TRY(ctx, d.seg_x.upload(std::vector<int32_t>(sub->seg_x, sub->seg_x + n_seg)));
    HIP_TRY(ctx, d.seg_len.upload(std::vector<int32_t>(sub->seg_len, sub->seg_len + n_seg)));
    HIP_TRY(ctx, d.sep_ptr.upload(std::vector<int32_t>(sub->sep_ptr, sub->sep_ptr + P + 1)));
    HIP_TRY(ctx, d.sep_idx.upload(std::vector<int32_t>(sub->sep_idx, sub->sep_idx + n_sidx)));
    HIP_TRY(ctx, d.row_part.upload(row_part));
    {
        // the -E_p^T blocks follow the G blocks in the pool, [s_p, n_p] row major, part after part: where the way up
        // reads them; the separator rows' segments must say the same
        // (every separator row its identity segment alone: the form that goes with tdgl_poisson_set_substructure_coupling)
        bool sparse_sep = n_sidx > 0;
        for (int64_t row = nI; row < n && sparse_sep; ++row) sparse_sep = sub->seg_ptr[row + 1] - sub->seg_ptr[row] == 1;
        d.need_coupling = sparse_sep;
        // ... and that one segment the unit entry on the row itself (what pack_for_device writes): the row is a copy
        bool ident = sparse_sep;
        for (int64_t row = nI; row < n && ident; ++row) {
            const int64_t k = sub->seg_ptr[row];
            ident = sub->seg_len[k] == 1 && sub->seg_x[k] == row && sub->vals[sub->seg_val[k]] == 1.0;
        }
        d.ident = ident;
        std::vector<int64_t> et_off(P);
        int64_t off = 1;
        for (int p = 0; p < P; ++p) off += (int64_t)(sub->part_ptr[p + 1] - sub->part_ptr[p]) * (sub->part_ptr[p + 1] - sub->part_ptr[p]);
        for (int p = 0; p < P; ++p) {
            et_off[p] = off;
            const int64_t rows = sub->part_ptr[p + 1] - sub->part_ptr[p];
            const int32_t s0 = sub->sep_ptr[p], cnt = sub->sep_ptr[p + 1] - s0;
            for (int32_t j = 0; j < cnt && !sparse_sep; ++j) {
                const int64_t row = nI + sub->sep_idx[s0 + j];
                bool found = false;
                for (int32_t k = sub->seg_ptr[row]; k < sub->seg_ptr[row + 1] && !found; ++k)
                    found = sub->seg_x[k] == sub->part_ptr[p] && sub->seg_val[k] == off + (int64_t)j * rows && sub->seg_len[k] == rows;
                if (!found && rows > 0)
                    TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: separator row %lld has no segment that is row %d of part %d's -E^T block", who,
                              (long long)row, (int)j, p);
            }
            off += rows * cnt;
        }
        if (off > sub->n_vals) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: the value pool is shorter than its G and -E^T blocks", who);
        TDGL_TRY(sub_upload_chunks(ctx, P, sub->part_ptr, sub->sep_ptr, et_off.data(), d.up_chunks, who));
    }
    TDGL_TRY(sub_upload_down_lists(ctx, P, n_rows, sub->part_ptr, g_off.data(), sub->seg_ptr, sub->seg_val, sub->seg_x, sub->seg_len,
                                   d.down_chunks, d.down_rows));
    HIP_TRY(ctx, d.g_off.upload(g_off));
    HIP_TRY(ctx, d.vals.alloc((size_t)sub->n_vals, false));
    HIP_TRY(ctx, hipMemcpy(d.vals.p, sub->vals, (size_t)sub->n_vals * sizeof(double), hipMemcpyHostToDevice));
    // (e_vals, the row-major copy of the E_p blocks, is not uploaded: the way up reads the pool's -E_p^T blocks)
    HIP_TRY(ctx, d.u.upload(std::vector<double>(sub->u, sub->u + nS)));
    HIP_TRY(ctx, d.w.alloc((size_t)n_rows));
    HIP_TRY(ctx, d.xs.alloc((size_t)nS));
    d.parts = P;
    d.nI = nI;
    d.nS = nS;
    return TDGL_OK;
}

// pseudo-inverse of a singular Schur complement [m, m] (null space: the constants) on the device, into
// D: (S + (s / m) 1 1^T)^-1 - 1 1^T / (s m)
// (plain -- the factors of a rank's interior block, tdgl_poisson_schur_begin: the plain inverse)
static int sub_schur_pinv(tdgl_ctx *ctx, const double *schur, int64_t m, bool plain, DenseTiles &D, const char *who) {
    double s = 0.0;
    for (int64_t i = 0; i < m; ++i) s += schur[i * m + i];
    s /= (double)m;
    if (!(s > 0.0) || !std::isfinite(s)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: the Schur complement has a non-positive mean diagonal", who);
    const int64_t N = round_up(m, GB);
    DevBuf<double> src, M;
    HIP_TRY(ctx, src.alloc((size_t)m * m, false));
    HIP_TRY(ctx, hipMemcpy(src.p, schur, (size_t)m * m * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, M.alloc((size_t)N * N, false));
    hipLaunchKernelGGL(k_dense_from, dim3(grid_for(N * N)), dim3(BLOCK), 0, ctx->stream, m, N, plain ? 0.0 : s / (double)m, (const double *)src.p, M.p);
    TDGL_TRY(dense_sweep_pack(ctx, M, m, N, plain ? 0.0 : 1.0 / (s * (double)m), D));
    return TDGL_OK;
}

// the last level's separator: its dense pseudo-inverse and the partials of its finish, staged in f (a new object, or the
// commit of an inner level)
static int sub_top(tdgl_ctx *ctx, DirectFactors &f, const double *schur, int64_t nS, const char *who) {
    f.nfin = (int)((nS + WAVE - 1) / WAVE);
    HIP_TRY(ctx, f.upart.alloc((size_t)f.nfin));
    if (f.levels > 1) HIP_TRY(ctx, f.mean.alloc(1));
    return sub_schur_pinv(ctx, schur, nS, f.n_local > 0, f.dense, who);
}

extern "C" int tdgl_poisson_set_substructure(tdgl_ctx *ctx, const tdgl_substructure *sub, double *seconds) {
    CTX_GUARD(ctx);
    if (!sub) {
        ctx->direct.reset();
        return TDGL_OK;
    }
    // (between tdgl_poisson_schur_begin and _finish: this rank's interior; otherwise the whole matrix)
    DirectFactors *cur = ctx->direct.get();
    const bool schur = cur && cur->in_schur_setup();
    if (distributed(ctx) && !schur)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_substructure: single-GPU contexts only (one process per GPU: inside tdgl_poisson_schur_begin / _finish)");
    if (ctx->levels.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_poisson_set_substructure: set the hierarchy first");
    // (schur == NULL: the Schur system is solved by further levels, tdgl_poisson_set_substructure_inner)
    if (sub->schur && sub->n_sep > 46000)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_substructure: a separator of %lld sites is outside what a dense matrix is meant for",
                  (long long)sub->n_sep);
    const int64_t t_begin = now_ns();
    auto f = std::make_unique<DirectFactors>();
    f->n_local = schur ? cur->n_local : 0;
    TDGL_TRY(sub_upload_level(ctx, sub, schur ? cur->n_local : ctx->n, f->lv[0], "tdgl_poisson_set_substructure"));
    f->levels = 1;
    if (sub->schur) TDGL_TRY(sub_top(ctx, *f, sub->schur, sub->n_sep, "tdgl_poisson_set_substructure"));
    f->stage = sub->schur ? f->settled() : DirectFactors::INNER_PENDING;
    if (schur) {  // the interface and the work vectors of tdgl_poisson_schur_begin stay
        f->ng = cur->ng;
        f->ngo = cur->ngo;
        f->owner_local = std::move(cur->owner_local);
        f->go_local = std::move(cur->go_local);
        f->go_gid = std::move(cur->go_gid);
        f->GI = std::move(cur->GI);
        f->IG = std::move(cur->IG);
        f->map = std::move(cur->map);
        for (auto b : {&DirectFactors::bp, &DirectFactors::xp, &DirectFactors::z, &DirectFactors::t, &DirectFactors::rg, &DirectFactors::xg,
                       &DirectFactors::y, &DirectFactors::v, &DirectFactors::c})
            (*f).*b = std::move((*cur).*b);
    }
    ctx->direct = std::move(f);
    if (seconds) *seconds = (double)(now_ns() - t_begin) * 1e-9;
    return TDGL_OK;
}

extern "C" int tdgl_poisson_set_substructure_coupling(tdgl_ctx *ctx, int32_t level, const int32_t *indptr, const int32_t *indices,
                                                      const double *data) {
    CTX_GUARD(ctx);
    if (level < 0 || level > 2) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_substructure_coupling: level must be 0, 1 or 2");
    DirectFactors *f = ctx->direct.get();
    if (!f || level >= f->levels || f->stage == DirectFactors::PRECOND)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_poisson_set_substructure_coupling: set that level's factors first (and before they precondition the CG)");
    SubLevel &L = f->lv[level];
    if (!indptr)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_substructure_coupling: the operator is required (a level described WITH its -E^T rows "
                  "needs no coupling block; one described without cannot do without)");
    const int64_t rows = L.nS, cols = L.nI;
    if (!offsets_ok(indptr, rows) || (indptr[rows] > 0 && (!indices || !data)))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_substructure_coupling: inconsistent operator");
    for (int64_t k = 0; k < indptr[rows]; ++k)
        if (indices[k] < 0 || indices[k] >= cols) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_substructure_coupling: column out of range");
    // the separator rows of that level's way down must then be their identity segment alone
    Csr M;
    TDGL_TRY(upload_csr(ctx, rows, cols, indptr, indices, data, M));
    L.coupling = std::move(M);
    L.need_coupling = false;
    if (f->stage == DirectFactors::COUPLING_PENDING) f->stage = f->settled();
    return TDGL_OK;
}

extern "C" int tdgl_poisson_set_substructure_inner(tdgl_ctx *ctx, const tdgl_substructure *sub, double *seconds) {
    CTX_GUARD(ctx);
    if (!sub) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_substructure_inner: a description is required");
    DirectFactors *f = ctx->direct.get();
    if (!f || f->stage != DirectFactors::INNER_PENDING)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_poisson_set_substructure_inner: set the first level without a Schur complement first");
    const int k = f->levels;  // this call describes level k (the second level of the solve is k = 1)
    if (k >= 3 || (k == 2 && !sub->schur))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_substructure_inner: at most two inner levels, and the last one carries the Schur complement");
    if (sub->schur && sub->n_sep > 46000)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_set_substructure_inner: a top separator of %lld sites is outside what a dense matrix is meant for",
                  (long long)sub->n_sep);
    const int64_t t_begin = now_ns();
    // built aside: the level (the previous level's separator vector is its vector) and, with the Schur complement, the top
    SubLevel L;
    TDGL_TRY(sub_upload_level(ctx, sub, f->lv[k - 1].nS, L, "tdgl_poisson_set_substructure_inner"));
    DirectFactors top;
    top.levels = k + 1;
    top.n_local = f->n_local;
    if (sub->schur) TDGL_TRY(sub_top(ctx, top, sub->schur, L.nS, "tdgl_poisson_set_substructure_inner"));
    f->lv[k] = std::move(L);
    f->levels = k + 1;
    if (sub->schur) {  // the last level: the dense top separator, and the solve is complete
        f->dense = std::move(top.dense);
        f->nfin = top.nfin;
        f->upart = std::move(top.upart);
        f->mean = std::move(top.mean);
        f->stage = f->settled();
    }
    if (seconds) *seconds = (double)(now_ns() - t_begin) * 1e-9;
    return TDGL_OK;
}

// fp32 storage of the resident factors (value pools, the top separator's tiles) and the lane-per-row work lists of
// the ways down: shared by the single-GPU preconditioner and the rank-level dissection.  With fp32 storage the pools are
// REPACKED on the way (k_sub_repack): every row of every block on its own 64-byte lines, chunks cut at multiples of 16
// rows, so that no request of the lane-per-row kernels shares a line with another workgroup's.
static bool env_force_sym() {  // TDGL_PD_SYM=2: symmetric tiles also on levels of a few parts (tests of small meshes)
    const char *env = getenv("TDGL_PD_SYM");
    return env && env[0] == '2';
}

// fp64_tiles: the direct SOLVE's form (tdgl_poisson_set_substructure_layout) -- a level that qualifies for symmetric tiles
// is repacked into a new fp64 pool (tiles, padded -E^T rows) and gets the tile kernel's work list; any other level is left
// exactly as it was uploaded (k_sub_down / k_sub_up on the original pool).
// Sets L.sym_lds (rows of b_p the symmetric way down stages, 0: the level keeps whole blocks) and L.up_R (chunks of 64
// rows per workgroup of the way up, > 1: a whole part each on the levels stored as tiles).
static int sub_level_to_precond(tdgl_ctx *ctx, SubLevel &L, bool fp32_storage, bool allow_sym, const char *who, bool fp64_tiles = false) {
    const int P = L.parts;
    L.sym_lds = 0;
    L.up_R = 1;
    std::vector<int32_t> pp((size_t)P + 1), sp((size_t)P + 1);
    std::vector<int64_t> go((size_t)P);
    HIP_TRY(ctx, hipMemcpy(pp.data(), L.part_ptr.p, pp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(sp.data(), L.sep_ptr.p, sp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(go.data(), L.g_off.p, go.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    std::vector<int32_t> ld((size_t)P);
    std::vector<int64_t> new_g((size_t)P), old_et((size_t)P), new_et((size_t)P);
    int64_t old_gvec = 0, new_gvec = 0, n_new = 0;
    const bool repack = (fp32_storage || fp64_tiles) && L.vals.n > 0;
    // symmetric tiles (k_sub_down_sym) where every part of the level is small enough for one workgroup each
    int32_t np_max = 0;
    for (int p = 0; p < P; ++p) np_max = std::max(np_max, pp[p + 1] - pp[p]);
    const bool sym = repack && allow_sym && np_max > 0 && np_max <= SYM_MAX_ROWS && (P >= 256 || (env_force_sym()));
    if (fp64_tiles && !sym) return TDGL_OK;
    if (repack) {
        int64_t off_old = 1, off_new = 16;
        for (int p = 0; p < P; ++p) off_old += (int64_t)(pp[p + 1] - pp[p]) * (pp[p + 1] - pp[p]);
        for (int p = 0; p < P; ++p) {
            const int32_t np_ = pp[p + 1] - pp[p];
            ld[p] = (int32_t)round_up(std::max<int32_t>(np_, 1), 16);
            new_g[p] = off_new;
            const int64_t nt_ = ld[p] / ST;
            off_new += sym ? nt_ * (nt_ + 1) / 2 * (ST * ST) : (int64_t)np_ * ld[p];
        }
        for (int p = 0; p < P; ++p) {
            const int32_t np_ = pp[p + 1] - pp[p], cnt = sp[p + 1] - sp[p];
            old_et[p] = off_old;
            new_et[p] = off_new;
            off_old += (int64_t)np_ * cnt;
            off_new += (int64_t)cnt * ld[p];
        }
        old_gvec = off_old;
        new_gvec = off_new;
        n_new = new_gvec + L.nI + 16;
        if (old_gvec + L.nI > (int64_t)L.vals.n) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: the value pool is shorter than its blocks", who);
        std::vector<SubRepack> desc((size_t)P);
        for (int p = 0; p < P; ++p)
            desc[p] = SubRepack{go[p], new_g[p], old_et[p], new_et[p], pp[p + 1] - pp[p], sp[p + 1] - sp[p], ld[p], sym ? 1 : 0};
        DevBuf<SubRepack> d_desc;
        HIP_TRY(ctx, d_desc.upload(desc));
        DevBuf<double> fresh;  // (fp64_tiles: the level's new pool)
        if (fp64_tiles) {
            HIP_TRY(ctx, fresh.alloc((size_t)n_new));  // (zeroed: the padding)
            const double one = 1.0;
            HIP_TRY(ctx, hipMemcpyAsync(fresh.p, &one, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL((k_sub_repack<double>), dim3(P), dim3(BLOCK), 0, ctx->stream, (const SubRepack *)d_desc.p, (const double *)L.vals.p,
                               fresh.p);
            if (L.nI > 0)
                HIP_TRY(ctx, hipMemcpyAsync(fresh.p + new_gvec, L.vals.p + old_gvec, (size_t)L.nI * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            HIP_TRY(ctx, L.vals32.alloc((size_t)n_new));  // (zeroed: the padding)
            const float one = 1.0f;
            HIP_TRY(ctx, hipMemcpyAsync(L.vals32.p, &one, sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL((k_sub_repack<float>), dim3(P), dim3(BLOCK), 0, ctx->stream, (const SubRepack *)d_desc.p, (const double *)L.vals.p,
                               L.vals32.p);
            if (L.nI > 0)
                hipLaunchKernelGGL(k_to_float, dim3(vec_grid(L.nI)), dim3(BLOCK), 0, ctx->stream, L.nI, (const double *)(L.vals.p + old_gvec),
                                   L.vals32.p + new_gvec);
        }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        // the segment lists (the rows the lane form leaves to a wavefront each: (G_p 1)^T, separator rows with -E^T segments)
        const int64_t n_rows = L.nI + L.nS + P;
        std::vector<int32_t> segp((size_t)n_rows + 1);
        HIP_TRY(ctx, hipMemcpy(segp.data(), L.seg_ptr.p, segp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<int64_t> sv((size_t)segp[n_rows]);
        if (!sv.empty()) HIP_TRY(ctx, hipMemcpy(sv.data(), L.seg_val.p, sv.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        const int64_t g_end = P > 0 ? old_et[0] : 1;
        for (int64_t &o : sv) {
            if (o == 0) continue;  // the leading 1.0
            if (o >= old_gvec) {
                o = new_gvec + (o - old_gvec);
            } else if (o >= g_end) {  // a row of a -E^T block
                const int p = (int)(std::upper_bound(old_et.begin(), old_et.end(), o) - old_et.begin()) - 1;
                const int64_t np_ = pp[p + 1] - pp[p], local = o - old_et[p];
                o = new_et[p] + (local / np_) * ld[p] + local % np_;
            } else {  // a row of a G block
                if (sym) {  // (the interior rows' own segments: the row form's, which neither the lane nor the tile form reads)
                    o = 0;
                    continue;
                }
                const int p = (int)(std::upper_bound(go.begin(), go.end(), o) - go.begin()) - 1;
                const int64_t np_ = pp[p + 1] - pp[p], local = o - go[p];
                o = new_g[p] + (local / np_) * ld[p] + local % np_;
            }
        }
        if (!sv.empty()) HIP_TRY(ctx, hipMemcpy(L.seg_val.p, sv.data(), sv.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        if (fp64_tiles) L.vals.take(fresh);
        else L.vals.release();
    } else {
        for (int p = 0; p < P; ++p) {
            ld[p] = pp[p + 1] - pp[p];
            new_g[p] = go[p];
        }
    }
    // the way down as a lane per row (k_sub_down_lanes): chunks of at most 64 rows cut at multiples of 16; g = where entry
    // (0, first row of the chunk) of the part's G block sits in the pool
    std::vector<SubDownChunk> ch;
    std::vector<SubUpChunk> up;
    // (TDGL_UP_PARTS=0: 64-row chunks on the way up everywhere -- for A/B measurements)
    const char *env_up = getenv("TDGL_UP_PARTS");
    const bool up_parts = sym && np_max > WAVE && !(env_up && env_up[0] == '0');
    int64_t et_run = 0;
    if (!repack) {  // (the -E^T blocks of the fp64 pool: behind the G blocks, back to back)
        et_run = 1;
        for (int p = 0; p < P; ++p) et_run += (int64_t)(pp[p + 1] - pp[p]) * (pp[p + 1] - pp[p]);
    }
    for (int p = 0; p < P; ++p) {
        const int32_t np_ = pp[p + 1] - pp[p], cnt = sp[p + 1] - sp[p];
        if (np_ > SUB_DOWN_MAX_COLS) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: a part of %d rows (at most %d are supported)", who, (int)np_, SUB_DOWN_MAX_COLS);
        const int64_t et_p = repack ? new_et[p] : et_run;
        if (!repack) et_run += (int64_t)np_ * cnt;
        if (np_ <= 0) continue;
        if (sym) {  // one workgroup per part: g = where its tiles start
            ch.push_back(SubDownChunk{new_g[p], pp[p], np_, pp[p], np_, 0, 0});
        } else {
        const int pieces = (np_ + WAVE - 1) / WAVE;
        const int32_t per = (int32_t)std::min<int64_t>(WAVE, round_up((np_ + pieces - 1) / pieces, 16));
        for (int32_t r0 = 0; r0 < np_; r0 += per)
            ch.push_back(SubDownChunk{new_g[p] + r0, pp[p], np_, pp[p] + r0, std::min<int32_t>(per, np_ - r0), ld[p], 0});
        }
        if (up_parts) {  // the whole part: its separator values are gathered once, a request covers a row of the block end to end
            up.push_back(SubUpChunk{et_p, ld[p], sp[p], cnt, pp[p], np_});
            continue;
        }
        for (int32_t r0 = 0; r0 < np_; r0 += WAVE)
            up.push_back(SubUpChunk{et_p + r0, ld[p], sp[p], cnt, pp[p] + r0, std::min<int32_t>(WAVE, np_ - r0)});
    }
    if (ch.empty()) ch.push_back(SubDownChunk{0, 0, 0, 0, 0, 0, 0});
    if (up.empty()) up.push_back(SubUpChunk{0, 0, 0, 0, 0, 0});
    HIP_TRY(ctx, L.down_chunks.upload(ch));
    HIP_TRY(ctx, L.up_chunks.upload(up));
    if (sym) L.sym_lds = (int)round_up(np_max, ST);
    L.up_R = up_parts ? (np_max + WAVE - 1) / WAVE : 1;
    return TDGL_OK;
}

// ------------------------------------------------------------------ the preconditioner's top separator, block low-rank
// Away from its diagonal the inverse of a separator's Schur complement is smooth (a discrete Green's function on the
// separator curves): its off-diagonal tiles are numerically of low rank.  One tile A = G_IJ (DT x DT, row major) is
// compressed by Gram-Schmidt with column pivoting (a rank-revealing QR, reorthogonalised): columns are taken until the
// Frobenius norm of the remainder (I - Q Q^T) A -- a bound on its 2-norm -- is at most tol; then A ~ Q (A^T Q)^T.
// Returns the rank (Q, W = A^T Q: column j at [j * B]), or -1 when kmax columns do not reach tol (the tile stays dense).
static int blr_compress_block(const double *A, int B, double tol, int kmax, std::vector<double> &Q, std::vector<double> &W) {
    std::vector<double> R(A, A + (size_t)B * B), cn((size_t)B), w((size_t)B);
    Q.assign((size_t)B * kmax, 0.0);
    const double tol2 = tol * tol;
    int k = 0;
    for (;;) {
        double tot = 0.0, best = -1.0;
        int piv = 0;
        for (int c = 0; c < B; ++c) cn[c] = 0.0;
        for (int r = 0; r < B; ++r)
            for (int c = 0; c < B; ++c) cn[c] += R[(size_t)r * B + c] * R[(size_t)r * B + c];
        for (int c = 0; c < B; ++c) {
            tot += cn[c];
            if (cn[c] > best) best = cn[c], piv = c;
        }
        if (tot <= tol2) break;
        if (k == kmax) return -1;
        double *q = &Q[(size_t)k * B];
        for (int r = 0; r < B; ++r) q[r] = R[(size_t)r * B + piv];
        for (int pass = 0; pass < 2; ++pass)  // (against the earlier columns, twice: orthogonal to working precision)
            for (int j = 0; j < k; ++j) {
                const double *qj = &Q[(size_t)j * B];
                double d = 0.0;
                for (int r = 0; r < B; ++r) d += qj[r] * q[r];
                for (int r = 0; r < B; ++r) q[r] -= d * qj[r];
            }
        double nrm = 0.0;
        for (int r = 0; r < B; ++r) nrm += q[r] * q[r];
        nrm = std::sqrt(nrm);
        if (!(nrm > 0.0)) break;
        for (int r = 0; r < B; ++r) q[r] /= nrm;
        for (int c = 0; c < B; ++c) w[c] = 0.0;
        for (int r = 0; r < B; ++r)
            for (int c = 0; c < B; ++c) w[c] += q[r] * R[(size_t)r * B + c];
        for (int r = 0; r < B; ++r)
            for (int c = 0; c < B; ++c) R[(size_t)r * B + c] -= q[r] * w[c];
        ++k;
    }
    Q.resize((size_t)k * B);
    W.assign((size_t)k * B, 0.0);
    for (int j = 0; j < k; ++j)
        for (int r = 0; r < B; ++r) {
            const double qr = Q[(size_t)j * B + r];
            for (int c = 0; c < B; ++c) W[(size_t)j * B + c] += A[(size_t)r * B + c] * qr;
        }
    return k;
}

// (the compression of one block, for the host tests: Q and W [kmax * B] column by column; returns the rank or -1)
extern "C" int32_t tdgl_host_blr_compress(const double *A, int32_t B, double tol, int32_t kmax, double *Q, double *W) {
    if (!A || !Q || !W || B <= 0 || kmax < 0) return -2;
    std::vector<double> q, w;
    const int k = blr_compress_block(A, B, tol, kmax, q, w);
    if (k > 0) {
        std::copy(q.begin(), q.end(), Q);
        std::copy(w.begin(), w.end(), W);
    }
    return k;
}

static double env_double(const char *name, double dflt) {
    const char *env = getenv(name);
    if (!env || !env[0]) return dflt;
    char *end = nullptr;
    const double v = strtod(env, &end);
    return (end && end != env && v > 0.0) ? v : dflt;
}

// The block low-rank form of a symmetric matrix, on the host: everything dense_to_blr uploads and reports.  The arrays
// are the ones kernels.inc documents (BlrArgs) at their true lengths: `items` is empty when no row block has a column,
// `F` and `twin` when there is no column at all (blr_upload puts a placeholder element in their place on the device).
struct BlrForm {
    std::vector<int32_t> dense_ij;         // [ndense] I << 16 | J, in tile order
    std::vector<float> Gd;                 // [ndense][DT * DT]
    std::vector<float> F;                  // [cols * DT]
    std::vector<int64_t> colbase;          // [nt + 1]
    std::vector<int32_t> twin;             // [cols]
    std::vector<int32_t> items;            // [nitems][4] BlrItem
    std::vector<int32_t> dslot_ptr, dslot;  // [nt + 1], [dslot_ptr[nt]]
    int ndense = 0, nitems = 0;
    int64_t cols = 0, pairs = 0, rank_max = 0, bytes = 0, dense_bytes = 0;
};

// The fp64 tiles hG (tile t = I (I + 1) / 2 + J, J <= I, DT x DT row major, zero beyond n) of a symmetric matrix of order
// n in nt tiles per side -> its block low-rank form: every off-diagonal tile compressed to the absolute tolerance
// tol_abs (blr_compress_block, at most DT / 4 columns: else the tile stays dense), the columns placed, the wavefront
// items, the dense slots, the byte counts.  A pure function of its arguments (the tiles are padded: n itself is not
// needed); the compression runs on up to 16 host threads.
static BlrForm blr_form_host(const double *hG, int64_t n, int nt, double tol_abs) {
    (void)n;
    BlrForm Z;
    const int64_t ntile = (int64_t)nt * (nt + 1) / 2, T2 = (int64_t)DT * DT;
    // every off-diagonal tile, on up to 16 host threads (tile order: t = I (I + 1) / 2 + J)
    const int kmax = DT / 4;
    std::vector<int> rank((size_t)ntile, -1);
    std::vector<std::vector<double>> Qs((size_t)ntile), Ws((size_t)ntile);
    std::atomic<int64_t> next{0};
    auto work = [&]() {
        for (int64_t t; (t = next.fetch_add(1)) < ntile;) {
            int I = (int)((std::sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
            while ((int64_t)(I + 1) * (I + 2) / 2 <= t) ++I;
            while ((int64_t)I * (I + 1) / 2 > t) --I;
            if (t - (int64_t)I * (I + 1) / 2 == I) continue;  // (diagonal tile: dense)
            rank[t] = blr_compress_block(&hG[(size_t)t * T2], DT, tol_abs, kmax, Qs[t], Ws[t]);
        }
    };
    {
        const int nth = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::vector<std::thread> pool;
        for (int k = 1; k < nth; ++k) pool.emplace_back(work);
        work();
        for (auto &th : pool) th.join();
    }
    // columns per row block, in pair order: U_IJ in block I, W_IJ in block J
    std::vector<int64_t> R((size_t)nt, 0), posU((size_t)ntile, 0), posW((size_t)ntile, 0);
    std::vector<int32_t> &dense_ij = Z.dense_ij;
    std::vector<char> is_dense((size_t)ntile, 0);
    for (int I = 0; I < nt; ++I)
        for (int J = 0; J <= I; ++J) {
            const int64_t t = (int64_t)I * (I + 1) / 2 + J;
            if (rank[t] < 0) {
                is_dense[t] = 1;
                dense_ij.push_back((I << 16) | J);
                continue;
            }
            posU[t] = R[I];
            R[I] += rank[t];
            posW[t] = R[J];
            R[J] += rank[t];
            Z.pairs += 1;
            Z.rank_max = std::max<int64_t>(Z.rank_max, rank[t]);
        }
    std::vector<int64_t> &colbase = Z.colbase;
    colbase.assign((size_t)nt + 1, 0);
    for (int K = 0; K < nt; ++K) colbase[K + 1] = colbase[K] + round_up(R[K], 4);
    Z.cols = colbase[nt];
    Z.ndense = (int)dense_ij.size();
    Z.dense_bytes = ntile * T2 * (int64_t)sizeof(float);
    Z.bytes = (int64_t)Z.ndense * T2 * (int64_t)sizeof(float) + 2 * Z.cols * DT * (int64_t)sizeof(float);
    std::vector<float> &F = Z.F, &Gd = Z.Gd;
    std::vector<int32_t> &twin = Z.twin;
    F.assign((size_t)(Z.cols * DT), 0.0f);
    Gd.assign((size_t)Z.ndense * T2, 0.0f);
    twin.assign((size_t)Z.cols, -1);
    for (int I = 0, d = 0; I < nt; ++I)
        for (int J = 0; J <= I; ++J) {
            const int64_t t = (int64_t)I * (I + 1) / 2 + J;
            if (is_dense[t]) {
                for (int64_t e = 0; e < T2; ++e) Gd[(size_t)d * T2 + e] = (float)hG[(size_t)t * T2 + e];
                ++d;
                continue;
            }
            const int r = rank[t];
            for (int c = 0; c < r; ++c) {
                const int64_t cu = posU[t] + c, cw = posW[t] + c;
                for (int row = 0; row < DT; ++row) {
                    const int h = row / WAVE, rl = row % WAVE;
                    F[(size_t)(DT * colbase[I] + ((int64_t)h * (colbase[I + 1] - colbase[I]) + cu) * WAVE + rl)] = (float)Qs[t][(size_t)c * DT + row];
                    F[(size_t)(DT * colbase[J] + ((int64_t)h * (colbase[J + 1] - colbase[J]) + cw) * WAVE + rl)] = (float)Ws[t][(size_t)c * DT + row];
                }
                twin[(size_t)(colbase[I] + cu)] = (int32_t)(colbase[J] + cw);
                twin[(size_t)(colbase[J] + cw)] = (int32_t)(colbase[I] + cu);
            }
        }
    std::vector<int32_t> &items = Z.items, &dslot_ptr = Z.dslot_ptr, &dslot = Z.dslot;
    dslot_ptr.assign((size_t)nt + 1, 0);
    for (int K = 0; K < nt; ++K) {
        const int32_t ng = (int32_t)((colbase[K + 1] - colbase[K]) / 4);
        for (int32_t g0 = 0; g0 < ng; g0 += BLR_ITEM_GROUPS) {
            items.insert(items.end(), {K, g0, std::min<int32_t>(g0 + BLR_ITEM_GROUPS, ng), 0});
        }
        for (int J = 0; J < nt; ++J) {
            const int I = std::max(K, J), Jm = std::min(K, J);
            if (is_dense[(size_t)((int64_t)I * (I + 1) / 2 + Jm)]) dslot.push_back(J);
        }
        dslot_ptr[K + 1] = (int32_t)dslot.size();
    }
    Z.nitems = (int)(items.size() / 4);
    return Z;
}

// The form's arrays onto the device and its counts into Z (coef zeroed; Z.tol and Z.norm are the caller's).  Arrays that
// may be empty get one placeholder element (four for F and the items): the kernels are handed no null pointer.
static int blr_upload(tdgl_ctx *ctx, BlrForm &S, BlrTop &Z) {
    Z.ndense = S.ndense;
    Z.nitems = S.nitems;
    Z.cols = S.cols;
    Z.pairs = S.pairs;
    Z.rank_max = S.rank_max;
    Z.bytes = S.bytes;
    Z.dense_bytes = S.dense_bytes;
    std::vector<int32_t> &items = S.items, &twin = S.twin, &dslot = S.dslot;
    std::vector<float> &F = S.F;
    if (items.empty()) items.assign(4, 0);
    HIP_TRY(ctx, Z.Gd.upload(S.Gd));
    HIP_TRY(ctx, Z.dense_ij.upload(S.dense_ij));
    if (F.empty()) F.assign(4, 0.0f);
    if (twin.empty()) twin.assign(1, -1);
    HIP_TRY(ctx, Z.F.upload(F));
    HIP_TRY(ctx, Z.colbase.upload(S.colbase));
    HIP_TRY(ctx, Z.twin.upload(twin));
    HIP_TRY(ctx, Z.items.upload(items));
    HIP_TRY(ctx, Z.coef.alloc((size_t)std::max<int64_t>(Z.cols, 1)));  // (zeroed: the padding columns)
    HIP_TRY(ctx, Z.dslot_ptr.upload(S.dslot_ptr));
    if (dslot.empty()) dslot.push_back(0);
    HIP_TRY(ctx, Z.dslot.upload(dslot));
    return TDGL_OK;
}

// The fp64 tiles of the top separator (f.dense.G) -> the block low-rank form f.blr (fp32), the fp64 tiles released.
// Truncation tau * ||G||_2 per tile pair (||G||_2 by power iteration on the device, on the tiles as they are); tiles
// whose rank would exceed DT / 4 stay dense.  If the form does not save at least 40 % of the bytes the dense fp32 tiles
// are kept (dense_to_fp32).  (TDGL_PD_BLR=0: the dense tiles always -- for A/B measurements; TDGL_PD_BLR_TOL: tau.)
constexpr double BLR_TOL = 3e-9;
constexpr int BLR_MIN_TILES = 8;

static int dense_to_blr(tdgl_ctx *ctx, DirectFactors &f) {
    DenseTiles &D = f.dense;
    BlrTop &Z = f.blr;
    Z = BlrTop();
    const int nt = D.tiles;
    const int64_t n = D.n;
    const double tau = env_double("TDGL_PD_BLR_TOL", BLR_TOL);
    // ||G||_2: power iteration on a deterministic start vector of mean zero (G 1 = 0)
    {
        DevBuf<double> xv, yv;
        HIP_TRY(ctx, xv.alloc((size_t)n, false));
        HIP_TRY(ctx, yv.alloc((size_t)n));
        std::vector<double> hx((size_t)n);
        uint64_t st = 0x9e3779b97f4a7c15ull;
        double mean = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            hx[i] = (double)(st >> 11) * 0x1.0p-53 - 0.5;
            mean += hx[i];
        }
        mean /= (double)n;
        for (auto &v : hx) v -= mean;
        double lam = 0.0;
        for (int it = 0; it < 30; ++it) {
            double nx = 0.0;
            for (double v : hx) nx += v * v;
            nx = std::sqrt(nx);
            if (!(nx > 0.0)) break;
            for (auto &v : hx) v /= nx;
            HIP_TRY(ctx, hipMemcpyAsync(xv.p, hx.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            launch_dense_sym(ctx, D, (int)n, (int)((n + WAVE - 1) / WAVE), xv.p, finish_product(yv.p));
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(hx.data(), yv.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            double ny = 0.0;
            for (double v : hx) ny += v * v;
            lam = std::sqrt(ny);
        }
        Z.norm = lam;
    }
    if (!(Z.norm > 0.0) || !std::isfinite(Z.norm)) return dense_to_fp32(ctx, D);
    Z.tol = tau;
    std::vector<double> hG((size_t)D.G.n);
    HIP_TRY(ctx, hipMemcpy(hG.data(), D.G.p, hG.size() * sizeof(double), hipMemcpyDeviceToHost));
    BlrForm S = blr_form_host(hG.data(), n, nt, tau * Z.norm);
    if (S.bytes > S.dense_bytes * 6 / 10) {  // (does not pay)
        Z = BlrTop();
        return dense_to_fp32(ctx, D);
    }
    TDGL_TRY(blr_upload(ctx, S, Z));
    D.G.release();
    return TDGL_OK;
}

static bool blr_wanted(const DirectFactors &f) {
    const char *env = getenv("TDGL_PD_BLR");
    if (env && env[0] == '0') return false;
    return f.n_local == 0 && f.levels > 0 && f.dense.tiles >= BLR_MIN_TILES && f.dense.G.n > 0;
}

// The resident factors, READY and not laid out for the direct solve (checked by the callers), become the preconditioner's:
// lane-per-row work lists, fp32 storage if asked.  The levels are converted in place: if that fails part way, the factors
// are released (the CG goes on with the AMG V-cycle alone).
static int sub_factors_to_precond(tdgl_ctx *ctx, bool fp32_storage, const char *who) {
    DirectFactors &f = *ctx->direct;
    // (TDGL_PD_SYM=0: whole G blocks on every level, the form of the earlier rounds -- for A/B measurements)
    const char *env = getenv("TDGL_PD_SYM");
    const bool allow_sym = !(env && env[0] == '0');
    int rc = TDGL_OK;
    for (int k = 0; k < f.levels && rc == TDGL_OK; ++k) rc = sub_level_to_precond(ctx, f.lv[k], fp32_storage, allow_sym, who);
    if (rc == TDGL_OK && fp32_storage) rc = blr_wanted(f) ? dense_to_blr(ctx, f) : dense_to_fp32(ctx, f.dense);
    if (rc != TDGL_OK) {
        ctx->direct.reset();
        return rc;
    }
    f.fp32 = fp32_storage;
    f.stage = DirectFactors::PRECOND;
    return TDGL_OK;
}

// What one application of either preconditioner costs on THIS device (the solver choice of pcg_solve multiplies them by
// the iterations it predicts): every application bracketed on its own, the MEDIAN of seven after two untimed ones -- one
// slow sample (another tenant's burst, a clock ramp) must not tilt every later choice.  On a zero residual.  In
// one-process-per-GPU mode both applications contain collectives: every rank calls this at the same point.
static int precond_calibrate(tdgl_ctx *ctx, double *t_apply_us, double *t_vcycle_us) {
    if (precond_f32_on(ctx)) TDGL_TRY(ensure_f32(ctx));
    HIP_TRY(ctx, hipMemsetAsync(ctx->pcg_r.p, 0, ctx->n_pad * sizeof(double), ctx->stream));
    std::vector<Event> ev(18);
    for (auto &e : ev) HIP_TRY(ctx, e.create());
    auto median_us = [&](auto &&apply, double *out) -> int {
        for (int rep = 0; rep < 9; ++rep) {
            HIP_TRY(ctx, hipEventRecord(ev[2 * rep], ctx->stream));
            TDGL_TRY(apply());
            HIP_TRY(ctx, hipEventRecord(ev[2 * rep + 1], ctx->stream));
        }
        HIP_TRY(ctx, hipEventSynchronize(ev[17]));
        std::vector<double> t;
        for (int rep = 2; rep < 9; ++rep) {
            float ms = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, ev[2 * rep], ev[2 * rep + 1]));
            t.push_back(1e3 * ms);
        }
        std::sort(t.begin(), t.end());
        *out = t[t.size() / 2];
        return TDGL_OK;
    };
    // (the application as the first iteration of a run launches it: r . z left to k_sell_axp where that is the order)
    TDGL_TRY(median_us([&]() -> int { return precond_factors_apply(ctx, ctx->pcg_r.p, ctx->direct->z.p, ctx->part_pair[0].p, true); }, &ctx->pd_t_apply_us));
    TDGL_TRY(median_us(
        [&]() -> int {
            if (precond_f32_on(ctx) && ctx->deep) {
                (void)vcycle0_f32(ctx, ctx->pcg_r.p, ctx->part_pair[0].p, Cycle0Out::ghosts_no_sums());
            } else if (precond_f32_on(ctx)) {
                (void)vcycle0_f32(ctx, ctx->pcg_r.p, ctx->part_pair[0].p, distributed(ctx) ? Cycle0Out::f64_rz(ctx->levels[0]->xb.p) : Cycle0Out::rz());
            } else {
                (void)vcycle_level(ctx, 0, ctx->pcg_r.p, ctx->part_pair[0].p, false);
            }
            return TDGL_OK;
        },
        &ctx->pd_t_vcycle_us));
    HIP_TRY(ctx, hipGetLastError());
    if (t_apply_us) *t_apply_us = ctx->pd_t_apply_us;
    if (t_vcycle_us) *t_vcycle_us = ctx->pd_t_vcycle_us;
    return TDGL_OK;
}

// factors laid out for the fp64 direct solve (tdgl_poisson_set_substructure_layout) cannot be converted
static bool sub_laid_out(const DirectFactors &f) {
    for (int k = 0; k < f.levels; ++k)
        if (f.lv[k].sym_lds > 0) return true;
    return false;
}

// The resident substructure factors become the CG's PRECONDITIONER instead of the solver (include/tdgl_hip.h).
extern "C" int tdgl_poisson_set_substructure_precond(tdgl_ctx *ctx, const int32_t *site_map, int32_t fp32_storage, double *t_apply_us,
                                                     double *t_vcycle_us) {
    CTX_GUARD(ctx);
    const char *who = "tdgl_poisson_set_substructure_precond";
    if (!site_map) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: the site map is required", who);
    DirectFactors *f = ctx->direct.get();
    if (!f || f->levels == 0 || f->stage != DirectFactors::READY)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "%s: describe the factors first (every level, every coupling block); once converted, describe them again", who);
    if (distributed(ctx) || ctx->levels.empty() || f->n_local > 0)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "%s: single-GPU contexts with a hierarchy only (one process per GPU: tdgl_poisson_schur_begin / _finish)", who);
    if (sub_laid_out(*f))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "%s: the fp64 pools were laid out for the direct solve (tdgl_poisson_set_substructure_layout); describe the factors again", who);
    const int64_t n = ctx->n;
    // dissection position -> the caller's site -> the context's index; must be a permutation
    std::vector<int32_t> map(n);
    std::vector<char> seen(n, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t s = site_map[i];
        if (s < 0 || s >= n || seen[s]) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: site_map is not a permutation of the sites", who);
        seen[s] = 1;
        map[i] = ctx->iperm[s];
    }
    DevBuf<int32_t> d_map;
    DevBuf<double> bp, xp, z;
    HIP_TRY(ctx, d_map.upload(map));
    if (ctx->pd_two_pass) {  // (the folded application reads r and writes z through the map: no vectors in the dissection's order)
        HIP_TRY(ctx, bp.alloc((size_t)n));
        HIP_TRY(ctx, xp.alloc((size_t)n));
    }
    HIP_TRY(ctx, z.alloc((size_t)ctx->n_pad));
    f->map = std::move(d_map);
    f->bp = std::move(bp);
    f->xp = std::move(xp);
    f->z = std::move(z);
    TDGL_TRY(sub_factors_to_precond(ctx, fp32_storage != 0, who));
    ctx->choice.enable(false);
    ctx->pcg_epoch += 1;
    return precond_calibrate(ctx, t_apply_us, t_vcycle_us);
}

extern "C" int tdgl_poisson_precond_choice(tdgl_ctx *ctx, int32_t mode) {
    if (!ctx || mode < 0 || mode > 2) return TDGL_ERR_ARG;
    ctx->pd_choice = mode;
    return TDGL_OK;
}

extern "C" int tdgl_get_precond_direct_stats(tdgl_ctx *ctx, int64_t *out4, double *out4d, int32_t reset) {
    double *out3 = out4d;
    if (!ctx) return TDGL_ERR_ARG;
    if (out4) {
        out4[0] = ctx->pd_solves;
        out4[1] = ctx->pd_iters;
        out4[2] = ctx->pd_amg_solves;
        out4[3] = ctx->pd_amg_iters;
    }
    if (out3) {
        out3[0] = ctx->pd_t_apply_us;
        out3[1] = ctx->pd_t_vcycle_us;
        out3[2] = ctx->pd_rate;
        out3[3] = (double)ctx->pd_handovers;
    }
    if (reset) ctx->pd_solves = ctx->pd_iters = ctx->pd_amg_solves = ctx->pd_amg_iters = ctx->pd_handovers = 0;
    return TDGL_OK;
}

extern "C" int tdgl_get_precond_direct_layout(tdgl_ctx *ctx, int32_t *sym_rows3) {
    if (!ctx || !sym_rows3) return TDGL_ERR_ARG;
    for (int k = 0; k < 3; ++k) sym_rows3[k] = ctx->direct ? ctx->direct->lv[k].sym_lds : 0;
    return TDGL_OK;
}

extern "C" int tdgl_get_precond_direct_blr(tdgl_ctx *ctx, int64_t *out6, double *out2) {
    if (!ctx || !out6 || !out2) return TDGL_ERR_ARG;
    const BlrTop *Z = ctx->direct ? &ctx->direct->blr : nullptr;
    const bool on = Z && Z->ndense > 0;
    out6[0] = on ? 1 : 0;
    out6[1] = on ? Z->pairs : 0;
    out6[2] = on ? Z->ndense : 0;
    out6[3] = on ? Z->rank_max : 0;
    out6[4] = on ? Z->bytes : 0;
    out6[5] = on ? Z->dense_bytes : 0;
    out2[0] = on ? Z->tol : 0.0;
    out2[1] = on ? Z->norm : 0.0;
    return TDGL_OK;
}

// ---- the block low-rank form through the C interface (include/tdgl_hip.h: tdgl_blr_form) -- for the tests of the form
// A form into the caller's struct: the counts on the sizing call (every array NULL), the arrays on the second call
// (every array given, the counts as the sizing call left them).  Returns a message, or NULL when all is well.
static const char *blr_form_out(const BlrForm &S, int64_t n, int nt, tdgl_blr_form *o) {
    const int given = (o->dense_ij != nullptr) + (o->Gd != nullptr) + (o->F != nullptr) + (o->colbase != nullptr) + (o->twin != nullptr) +
                      (o->items != nullptr) + (o->dslot_ptr != nullptr) + (o->dslot != nullptr);
    if (given != 0 && given != 8) return "every array of the form, or none (the sizing call)";
    const int64_t ndslot = (int64_t)S.dslot.size();
    if (given == 8 && (o->n != n || o->nt != nt || o->ndense != S.ndense || o->nitems != S.nitems || o->cols != S.cols || o->ndslot != ndslot))
        return "the counts are not those of the sizing call for this matrix";
    o->n = n;
    o->nt = nt;
    o->ndense = S.ndense;
    o->nitems = S.nitems;
    o->cols = S.cols;
    o->ndslot = ndslot;
    o->pairs = S.pairs;
    o->rank_max = S.rank_max;
    o->bytes = S.bytes;
    o->dense_bytes = S.dense_bytes;
    if (given == 0) return nullptr;
    std::copy(S.dense_ij.begin(), S.dense_ij.end(), o->dense_ij);
    std::copy(S.Gd.begin(), S.Gd.end(), o->Gd);
    std::copy(S.F.begin(), S.F.end(), o->F);
    std::copy(S.colbase.begin(), S.colbase.end(), o->colbase);
    std::copy(S.twin.begin(), S.twin.end(), o->twin);
    std::copy(S.items.begin(), S.items.end(), o->items);
    std::copy(S.dslot_ptr.begin(), S.dslot_ptr.end(), o->dslot_ptr);
    std::copy(S.dslot.begin(), S.dslot.end(), o->dslot);
    return nullptr;
}

// G [n x n] row major, symmetric (its lower triangle is read) -> the fp64 tiles as k_dense_pack_sym leaves them
static std::vector<double> blr_pack_tiles(const double *G, int64_t n, int nt) {
    const int64_t ntile = (int64_t)nt * (nt + 1) / 2, T2 = (int64_t)DT * DT;
    std::vector<double> hG((size_t)(ntile * T2), 0.0);
    for (int I = 0; I < nt; ++I)
        for (int J = 0; J <= I; ++J) {
            double *dst = &hG[(size_t)(((int64_t)I * (I + 1) / 2 + J) * T2)];
            for (int e = 0; e < DT * DT; ++e) {
                const int64_t r = (int64_t)I * DT + e / DT, c = (int64_t)J * DT + e % DT;
                if (r < n && c < n) dst[e] = G[(r > c ? r : c) * n + (r > c ? c : r)];
            }
        }
    return hG;
}

constexpr int64_t BLR_TEST_MAX_N = 32767 * (int64_t)DT;  // (dense_ij keeps I in 15 bits)

extern "C" int tdgl_host_blr_form(int64_t n, const double *G, double tol_abs, tdgl_blr_form *form) {
    if (!G || !form || n < 1 || n > BLR_TEST_MAX_N || !(tol_abs >= 0.0))
        TDGL_FAIL((tdgl_ctx *)nullptr, TDGL_ERR_ARG, "tdgl_host_blr_form: G and form are required, n in 1 .. %lld, tol_abs >= 0", (long long)BLR_TEST_MAX_N);
    const int nt = (int)((n + DT - 1) / DT);
    const std::vector<double> hG = blr_pack_tiles(G, n, nt);
    const BlrForm S = blr_form_host(hG.data(), n, nt, tol_abs);
    const char *msg = blr_form_out(S, n, nt, form);
    if (msg) TDGL_FAIL((tdgl_ctx *)nullptr, TDGL_ERR_ARG, "tdgl_host_blr_form: %s", msg);
    return TDGL_OK;
}

extern "C" int tdgl_get_precond_direct_blr_form(tdgl_ctx *ctx, tdgl_blr_form *form) {
    CTX_GUARD(ctx);
    const char *who = "tdgl_get_precond_direct_blr_form";
    if (!form) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: null argument", who);
    if (!ctx->direct || ctx->direct->blr.ndense == 0)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "%s: the top separator is not in block low-rank form (tdgl_get_precond_direct_blr)", who);
    const BlrTop &Z = ctx->direct->blr;
    const int nt = ctx->direct->dense.tiles;
    BlrForm S;
    S.ndense = Z.ndense;
    S.nitems = Z.nitems;
    S.cols = Z.cols;
    S.pairs = Z.pairs;
    S.rank_max = Z.rank_max;
    S.bytes = Z.bytes;
    S.dense_bytes = Z.dense_bytes;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    auto fetch = [&](auto &dst, const auto &src, size_t count) -> hipError_t {
        dst.resize(count);
        if (count == 0) return hipSuccess;
        return hipMemcpy(dst.data(), src.p, count * sizeof(dst[0]), hipMemcpyDeviceToHost);
    };
    HIP_TRY(ctx, fetch(S.dslot_ptr, Z.dslot_ptr, (size_t)nt + 1));
    HIP_TRY(ctx, fetch(S.dslot, Z.dslot, (size_t)S.dslot_ptr[(size_t)nt]));
    HIP_TRY(ctx, fetch(S.dense_ij, Z.dense_ij, (size_t)Z.ndense));
    HIP_TRY(ctx, fetch(S.Gd, Z.Gd, (size_t)Z.ndense * DT * DT));
    HIP_TRY(ctx, fetch(S.F, Z.F, (size_t)(Z.cols * DT)));
    HIP_TRY(ctx, fetch(S.colbase, Z.colbase, (size_t)nt + 1));
    HIP_TRY(ctx, fetch(S.twin, Z.twin, (size_t)Z.cols));
    HIP_TRY(ctx, fetch(S.items, Z.items, (size_t)Z.nitems * 4));
    const char *msg = blr_form_out(S, ctx->direct->dense.n, nt, form);
    if (msg) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: %s", who, msg);
    return TDGL_OK;
}

// The two kernels of the form alone: the form of G built by blr_form_host, uploaded into buffers of this call, applied
// to the n_vec vectors of X ([n_vec][n]) one after the other through blr_launch -- the launches of the preconditioner,
// without status block, controller or u; Y [n_vec][n].  coef is zeroed once and then lives through the applications, as
// in the product.  The context lends its device and stream: its factors and the CG's state are not touched.
extern "C" int tdgl_blr_apply(tdgl_ctx *ctx, int64_t n, const double *G, double tol_abs, int64_t n_vec, const double *X, double *Y,
                              tdgl_blr_form *form) {
    CTX_GUARD(ctx);
    const char *who = "tdgl_blr_apply";
    if (!G || !X || !Y) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: null argument", who);
    if (n < 1 || n > BLR_TEST_MAX_N) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: n must be in 1 .. %lld", who, (long long)BLR_TEST_MAX_N);
    if (n_vec < 1) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: no vectors", who);
    if (!(tol_abs >= 0.0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: the tolerance must be >= 0", who);
    const int nt = (int)((n + DT - 1) / DT), nfin = (int)((n + WAVE - 1) / WAVE);
    BlrForm S;
    {
        const std::vector<double> hG = blr_pack_tiles(G, n, nt);
        S = blr_form_host(hG.data(), n, nt, tol_abs);
    }
    if (form) {
        const char *msg = blr_form_out(S, n, nt, form);
        if (msg) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: %s", who, msg);
    }
    BlrTop Z;
    TDGL_TRY(blr_upload(ctx, S, Z));
    DevBuf<double> part, x, y;
    HIP_TRY(ctx, part.alloc((size_t)nt * nt * DT));
    HIP_TRY(ctx, x.alloc((size_t)(n * n_vec), false));
    HIP_TRY(ctx, y.alloc((size_t)(n * n_vec)));
    HIP_TRY(ctx, hipMemcpy(x.p, X, (size_t)(n * n_vec) * sizeof(double), hipMemcpyHostToDevice));
    for (int64_t v = 0; v < n_vec; ++v)
        blr_launch(ctx, Z, (int)n, nt, nfin, x.p + v * n, part.p, finish_product(y.p + v * n));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(Y, y.p, (size_t)(n * n_vec) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

// The direct SOLVE (fp64 factors, run-ahead loop): levels of many small parts keep only the tiles on or below the diagonal
// of their symmetric G blocks and run the tile kernel on the way down; everything else stays as uploaded.  The levels are
// repacked in place: if that fails part way, the factors are released (AMG-PCG).
extern "C" int tdgl_poisson_set_substructure_layout(tdgl_ctx *ctx, int32_t symmetric_tiles) {
    CTX_GUARD(ctx);
    const char *who = "tdgl_poisson_set_substructure_layout";
    DirectFactors *f = ctx->direct.get();
    if (!f || f->levels == 0 || f->stage < DirectFactors::COUPLING_PENDING)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "%s: describe the factors first (every level)", who);
    if (f->stage == DirectFactors::PRECOND)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: the factors already precondition the CG (their layout is set there)", who);
    const char *env = getenv("TDGL_PD_SYM");
    if (!symmetric_tiles || (env && env[0] == '0')) return TDGL_OK;
    for (int k = 0; k < f->levels; ++k) {
        if (f->lv[k].sym_lds > 0) continue;
        const int rc = sub_level_to_precond(ctx, f->lv[k], false, true, who, true);
        if (rc != TDGL_OK) {
            ctx->direct.reset();
            return rc;
        }
    }
    return TDGL_OK;
}

// ---------------------------------------------------------------------------------------------------
// ... with the factors formed on the device (include/tdgl_hip.h: tdgl_substructure_plan)
namespace tdgl {

// padded interior blocks: zero, identity on the padding
__global__ __launch_bounds__(BLOCK) void k_sub_blocks_init(const int32_t *__restrict__ nbq, const int64_t *__restrict__ moff,
                                                           const int32_t *__restrict__ part_ptr, double *__restrict__ Mp) {
    const int q = blockIdx.y;
    const int64_t N = (int64_t)nbq[q] * GB, np_ = part_ptr[q + 1] - part_ptr[q];
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i >= N * N) return;
    const int64_t r = i / N, c = i % N;
    Mp[moff[q] + i] = (r == c && r >= np_) ? 1.0 : 0.0;
}

// A_pp from the SELL level-0 matrix: one lane per interior row
__global__ __launch_bounds__(BLOCK) void k_sub_blocks_scatter(int n_slices, int64_t nI, const int32_t *__restrict__ slice_off,
                                                              const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                              const int32_t *__restrict__ row_part, const int32_t *__restrict__ part_ptr,
                                                              const int32_t *__restrict__ nbq, const int64_t *__restrict__ moff,
                                                              double *__restrict__ Mp) {
    const int slice = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
    if (slice >= n_slices) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t row = (int64_t)slice * WAVE + lane;
    if (row >= nI) return;
    const int p = row_part[row], a = part_ptr[p], b = part_ptr[p + 1];
    double *__restrict__ M = Mp + moff[p] + (row - a) * (int64_t)nbq[p] * GB;
    int64_t idx = (int64_t)slice_off[slice] * WAVE + lane;
    for (int k = slice_off[slice]; k < slice_off[slice + 1]; ++k, idx += WAVE) {
        const int c = cols[idx];
        if (c >= a && c < b) M[c - a] += vals[idx];
    }
}

// G_p = -(swept block), row by row into the value pool; its row sums (G_p 1) behind them: one wavefront per row
__global__ __launch_bounds__(BLOCK) void k_sub_unpack_G(int64_t nI, const int32_t *__restrict__ row_part,
                                                        const int32_t *__restrict__ part_ptr, const int32_t *__restrict__ nbq,
                                                        const int64_t *__restrict__ moff, const double *__restrict__ Mp,
                                                        const int64_t *__restrict__ g_off, int64_t gvec_off, double *__restrict__ pool) {
    const int64_t row = blockIdx.x * (int64_t)(BLOCK / WAVE) + threadIdx.x / WAVE;
    if (row >= nI) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int p = row_part[row], a = part_ptr[p], np_ = part_ptr[p + 1] - a, lr = (int)(row - a);
    const int64_t N = (int64_t)nbq[p] * GB;
    const double *__restrict__ M = Mp + moff[p];
    double *__restrict__ dst = pool + g_off[p] + (int64_t)lr * np_;
    double acc = 0.0;
    for (int c = lane; c < np_; c += WAVE) {
        const double v = -M[(int64_t)(lr > c ? lr : c) * N + (lr > c ? c : lr)];
        dst[c] = v;
        acc += v;
    }
    acc = wave_sum(acc);
    if (lane == 0) pool[gvec_off + row] = acc;
}

// E_p[:, j] = sum over the entries (r', v) of A_pS[:, j] of v G_p[r', :]  (one workgroup per (part, site) pair);
// written as E_p (row major, the way up), as -E_p^T (value pool, the way down), and its column sum
__global__ __launch_bounds__(BLOCK) void k_sub_E(const int32_t *__restrict__ pair_part, const int32_t *__restrict__ part_ptr,
                                                 const int32_t *__restrict__ sep_ptr, const int32_t *__restrict__ ent_ptr,
                                                 const int32_t *__restrict__ ent_row, const double *__restrict__ ent_val,
                                                 const int64_t *__restrict__ g_off, const int64_t *__restrict__ et_off,
                                                 const int64_t *__restrict__ e_off, double *__restrict__ pool,
                                                 double *__restrict__ e_vals, double *__restrict__ colsum) {
    const int q = blockIdx.x, p = pair_part[q], a = part_ptr[p], np_ = part_ptr[p + 1] - a;
    const int sp = sep_ptr[p + 1] - sep_ptr[p], jl = q - sep_ptr[p];
    const int k0 = ent_ptr[q], k1 = ent_ptr[q + 1];
    const double *__restrict__ G = pool + g_off[p];
    double acc = 0.0;
    for (int r = threadIdx.x; r < np_; r += BLOCK) {
        double e = 0.0;
        for (int k = k0; k < k1; ++k) e += ent_val[k] * G[(int64_t)(ent_row[k] - a) * np_ + r];
        e_vals[e_off[p] + (int64_t)r * sp + jl] = e;
        pool[et_off[p] + (int64_t)jl * np_ + r] = -e;
        acc += e;
    }
    const double t = block_sum(acc);
    if (threadIdx.x == 0) colsum[q] = t;
}

// C_p[i, :] = sum over the entries (r', v) of A_pS[:, i] of v E_p[r', :]  (one workgroup per pair)
__global__ __launch_bounds__(BLOCK) void k_sub_C(const int32_t *__restrict__ pair_part, const int32_t *__restrict__ part_ptr,
                                                 const int32_t *__restrict__ sep_ptr, const int32_t *__restrict__ ent_ptr,
                                                 const int32_t *__restrict__ ent_row, const double *__restrict__ ent_val,
                                                 const int64_t *__restrict__ e_off, const double *__restrict__ e_vals,
                                                 const int64_t *__restrict__ c_off, double *__restrict__ Cpool) {
    const int q = blockIdx.x, p = pair_part[q], a = part_ptr[p];
    const int sp = sep_ptr[p + 1] - sep_ptr[p], il = q - sep_ptr[p];
    const int k0 = ent_ptr[q], k1 = ent_ptr[q + 1];
    for (int j = threadIdx.x; j < sp; j += BLOCK) {
        double c = 0.0;
        for (int k = k0; k < k1; ++k) c += ent_val[k] * e_vals[e_off[p] + (int64_t)(ent_row[k] - a) * sp + j];
        Cpool[c_off[p] + (int64_t)il * sp + j] = c;
    }
}

// Row i of the padded matrix the sweep inverts: S_c[i, :] + shift = A_SS[i, :] - sum over the pairs that
// touch site i (ascending pair id) of their C_p row, + shift; identity on the padding.  One workgroup owns
// the row, so the three phases need no atomics.  Also u_i = -sum of the pairs' column sums of E.
__global__ __launch_bounds__(BLOCK) void k_sub_schur_row(int64_t nS, int64_t N, double shift, const int32_t *__restrict__ ass_indptr,
                                                         const int32_t *__restrict__ ass_indices, const double *__restrict__ ass_data,
                                                         const int32_t *__restrict__ node_ptr, const int32_t *__restrict__ node_pair,
                                                         const int32_t *__restrict__ pair_part, const int32_t *__restrict__ sep_ptr,
                                                         const int32_t *__restrict__ sep_idx, const int64_t *__restrict__ c_off,
                                                         const double *__restrict__ Cpool, const double *__restrict__ colsum,
                                                         double *__restrict__ M, double *__restrict__ u) {
    const int64_t i = blockIdx.x;
    double *__restrict__ row = M + i * N;
    for (int64_t c = threadIdx.x; c < N; c += BLOCK) row[c] = (i < nS && c < nS) ? shift : (c == i ? 1.0 : 0.0);
    if (i >= nS) return;  // (workgroup-uniform)
    __syncthreads();
    for (int k = ass_indptr[i] + threadIdx.x; k < ass_indptr[i + 1]; k += BLOCK) row[ass_indices[k]] += ass_data[k];
    double usum = 0.0;
    for (int t = node_ptr[i]; t < node_ptr[i + 1]; ++t) {
        __syncthreads();
        const int q = node_pair[t], p = pair_part[q], s0 = sep_ptr[p], sp = sep_ptr[p + 1] - s0, il = q - s0;
        const double *__restrict__ C = Cpool + c_off[p] + (int64_t)il * sp;
        for (int j = threadIdx.x; j < sp; j += BLOCK) row[sep_idx[s0 + j]] -= C[j];
        usum -= colsum[q];
    }
    if (threadIdx.x == 0) u[i] = usum;
}

}  // namespace tdgl

extern "C" int tdgl_poisson_build_substructure(tdgl_ctx *ctx, const tdgl_substructure_plan *pl, double *seconds) {
    CTX_GUARD(ctx);
    if (!pl) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: null plan");
    if (distributed(ctx)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: single-GPU contexts only");
    if (ctx->levels.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_poisson_build_substructure: set the hierarchy first");
    const int64_t nI = pl->n_interior, nS = pl->n_sep, n = ctx->n;
    const int P = pl->n_parts;
    if (nI + nS != n || P < 1 || nS < 2 || nS > 46000 || !pl->part_ptr || !pl->sep_ptr || !pl->sep_idx || !pl->ent_ptr || !pl->ent_row ||
        !pl->ent_val || !pl->node_ptr || !pl->node_pair || !pl->ass_indptr || !pl->ass_indices || !pl->ass_data || !pl->seg_ptr ||
        !pl->seg_val || !pl->seg_x || !pl->seg_len || !pl->g_off || !pl->et_off || !pl->e_off)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: inconsistent plan (n_interior + n_sep must be the site count)");
    if (pl->part_ptr[0] != 0 || pl->part_ptr[P] != nI) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: part_ptr must run from 0 to n_interior");
    const int64_t t_begin = now_ns();
    const int64_t n_rows = n + P;
    if (!offsets_ok(pl->seg_ptr, n_rows) || !offsets_ok(pl->sep_ptr, P) || !offsets_ok(pl->ent_ptr, pl->sep_ptr[P]) ||
        !offsets_ok(pl->node_ptr, nS) || !offsets_ok(pl->ass_indptr, nS))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: an offset array does not run from 0 or decreases");
    const int64_t n_seg = pl->seg_ptr[n_rows], Q = pl->sep_ptr[P], n_ent = pl->ent_ptr[Q];
    if (pl->node_ptr[nS] != Q) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: node_ptr must cover every pair");
    // host-side index checks and derived tables
    std::vector<int32_t> row_part(nI), pair_part(Q), nbq(P);
    std::vector<int64_t> moff(P), poff(P), c_off(P);
    int64_t m_total = 0, p_total = 0, c_total = 0;
    int max_nb = 0;
    for (int p = 0; p < P; ++p) {
        const int64_t rows = pl->part_ptr[p + 1] - pl->part_ptr[p], cnt = pl->sep_ptr[p + 1] - pl->sep_ptr[p];
        if (rows < 1 || cnt < 0) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: empty part %d", p);
        for (int64_t r = pl->part_ptr[p]; r < pl->part_ptr[p + 1]; ++r) row_part[r] = p;
        for (int64_t q = pl->sep_ptr[p]; q < pl->sep_ptr[p + 1]; ++q) pair_part[q] = p;
        nbq[p] = (int)((rows + GB - 1) / GB);
        max_nb = std::max(max_nb, nbq[p]);
        moff[p] = m_total;
        m_total += (int64_t)nbq[p] * GB * nbq[p] * GB;
        poff[p] = p_total;
        p_total += (int64_t)nbq[p] * GB * GB;
        c_off[p] = c_total;
        c_total += cnt * cnt;
        if (pl->g_off[p] < 1 || pl->g_off[p] + rows * rows > pl->n_vals || pl->et_off[p] < 1 || pl->et_off[p] + rows * cnt > pl->n_vals ||
            pl->e_off[p] < 0 || pl->e_off[p] + rows * cnt > pl->n_e)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: pool offsets of part %d out of range", p);
    }
    for (int p = 0; p < P; ++p) {  // interior rows = the rows of their part's G block (k_sub_down's fast path reads them there)
        const int64_t rows = pl->part_ptr[p + 1] - pl->part_ptr[p];
        for (int64_t r = 0; r < rows; ++r) {
            const int64_t row = pl->part_ptr[p] + r, k = pl->seg_ptr[row];
            if (pl->seg_ptr[row + 1] != k + 1 || pl->seg_val[k] != pl->g_off[p] + r * rows || pl->seg_x[k] != pl->part_ptr[p] || pl->seg_len[k] != rows)
                TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: interior row %lld is not a row of its part's G block", (long long)row);
        }
    }
    if (pl->gvec_off < 1 || pl->gvec_off + nI > pl->n_vals) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: gvec_off out of range");
    for (int64_t q = 0; q < Q; ++q) {
        if (pl->sep_idx[q] < 0 || pl->sep_idx[q] >= nS) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: separator index out of range");
        const int p = pair_part[q];
        for (int k = pl->ent_ptr[q]; k < pl->ent_ptr[q + 1]; ++k)
            if (pl->ent_row[k] < pl->part_ptr[p] || pl->ent_row[k] >= pl->part_ptr[p + 1])
                TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: entry %d lies outside its part", k);
    }
    for (int64_t t = 0; t < Q; ++t)
        if (pl->node_pair[t] < 0 || pl->node_pair[t] >= Q) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: pair id out of range");
    for (int64_t k = 0; k < n_seg; ++k)
        if (pl->seg_len[k] < 0 || pl->seg_val[k] < 0 || pl->seg_val[k] + pl->seg_len[k] > pl->n_vals || pl->seg_x[k] < 0 ||
            (int64_t)pl->seg_x[k] + pl->seg_len[k] > n)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: segment %lld out of range", (long long)k);
    const int64_t ass_nnz = pl->ass_indptr[nS];
    double s = 0.0;
    for (int64_t i = 0; i < nS; ++i)
        for (int k = pl->ass_indptr[i]; k < pl->ass_indptr[i + 1]; ++k) {
            if (pl->ass_indices[k] < 0 || pl->ass_indices[k] >= nS) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: A_SS column out of range");
            if (pl->ass_indices[k] == i) s += pl->ass_data[k];
        }
    s /= (double)nS;
    if (!(s > 0.0) || !std::isfinite(s)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: A_SS has a non-positive mean diagonal");
    // built aside, moved in once complete
    auto f = std::make_unique<DirectFactors>();
    SubLevel &L = f->lv[0];
    // index arrays of the solve
    HIP_TRY(ctx, L.part_ptr.upload(std::vector<int32_t>(pl->part_ptr, pl->part_ptr + P + 1)));
    HIP_TRY(ctx, L.seg_ptr.upload(std::vector<int32_t>(pl->seg_ptr, pl->seg_ptr + n_rows + 1)));
    HIP_TRY(ctx, L.seg_val.upload(std::vector<int64_t>(pl->seg_val, pl->seg_val + n_seg)));
    HIP_TRY(ctx, L.seg_x.upload(std::vector<int32_t>(pl->seg_x, pl->seg_x + n_seg)));
    HIP_TRY(ctx, L.seg_len.upload(std::vector<int32_t>(pl->seg_len, pl->seg_len + n_seg)));
    HIP_TRY(ctx, L.sep_ptr.upload(std::vector<int32_t>(pl->sep_ptr, pl->sep_ptr + P + 1)));
    HIP_TRY(ctx, L.sep_idx.upload(std::vector<int32_t>(pl->sep_idx, pl->sep_idx + Q)));
    HIP_TRY(ctx, L.row_part.upload(row_part));
    TDGL_TRY(sub_upload_chunks(ctx, P, pl->part_ptr, pl->sep_ptr, pl->et_off, L.up_chunks, "tdgl_poisson_build_substructure"));
    TDGL_TRY(sub_upload_down_lists(ctx, P, n_rows, pl->part_ptr, pl->g_off, pl->seg_ptr, pl->seg_val, pl->seg_x, pl->seg_len,
                                   L.down_chunks, L.down_rows));
    HIP_TRY(ctx, L.vals.alloc((size_t)pl->n_vals, false));
    HIP_TRY(ctx, L.u.alloc((size_t)nS));
    HIP_TRY(ctx, L.w.alloc((size_t)n_rows));
    HIP_TRY(ctx, L.xs.alloc((size_t)nS));
    f->nfin = (int)((nS + WAVE - 1) / WAVE);
    HIP_TRY(ctx, f->upart.alloc((size_t)f->nfin));
    // set-up-only tables
    DevBuf<int32_t> d_pair_part, d_nbq, d_ent_ptr, d_ent_row, d_node_ptr, d_node_pair, d_ass_p, d_ass_i, d_flag;
    DevBuf<int64_t> d_moff, d_poff, d_coff, d_goff, d_etoff, d_eoff;
    DevBuf<double> d_ent_val, d_ass_v, Mp, Pb, Wb, Db, Cpool, colsum, E;  // (E: the row-major E_p blocks, which only the build reads)
    HIP_TRY(ctx, d_pair_part.upload(pair_part));
    HIP_TRY(ctx, d_nbq.upload(nbq));
    HIP_TRY(ctx, d_moff.upload(moff));
    HIP_TRY(ctx, d_poff.upload(poff));
    HIP_TRY(ctx, d_coff.upload(c_off));
    HIP_TRY(ctx, d_goff.upload(std::vector<int64_t>(pl->g_off, pl->g_off + P)));
    HIP_TRY(ctx, L.g_off.upload(std::vector<int64_t>(pl->g_off, pl->g_off + P)));
    HIP_TRY(ctx, d_etoff.upload(std::vector<int64_t>(pl->et_off, pl->et_off + P)));
    HIP_TRY(ctx, d_eoff.upload(std::vector<int64_t>(pl->e_off, pl->e_off + P)));
    HIP_TRY(ctx, E.alloc((size_t)std::max<int64_t>(pl->n_e, 1), false));
    HIP_TRY(ctx, d_ent_ptr.upload(std::vector<int32_t>(pl->ent_ptr, pl->ent_ptr + Q + 1)));
    HIP_TRY(ctx, d_ent_row.upload(std::vector<int32_t>(pl->ent_row, pl->ent_row + n_ent)));
    HIP_TRY(ctx, d_ent_val.upload(std::vector<double>(pl->ent_val, pl->ent_val + n_ent)));
    HIP_TRY(ctx, d_node_ptr.upload(std::vector<int32_t>(pl->node_ptr, pl->node_ptr + nS + 1)));
    HIP_TRY(ctx, d_node_pair.upload(std::vector<int32_t>(pl->node_pair, pl->node_pair + Q)));
    HIP_TRY(ctx, d_ass_p.upload(std::vector<int32_t>(pl->ass_indptr, pl->ass_indptr + nS + 1)));
    HIP_TRY(ctx, d_ass_i.upload(std::vector<int32_t>(pl->ass_indices, pl->ass_indices + ass_nnz)));
    HIP_TRY(ctx, d_ass_v.upload(std::vector<double>(pl->ass_data, pl->ass_data + ass_nnz)));
    HIP_TRY(ctx, d_flag.alloc(1));
    HIP_TRY(ctx, Mp.alloc((size_t)m_total, false));
    HIP_TRY(ctx, Pb.alloc((size_t)p_total, false));
    HIP_TRY(ctx, Wb.alloc((size_t)p_total, false));
    HIP_TRY(ctx, Db.alloc((size_t)P * GB * GB, false));
    HIP_TRY(ctx, Cpool.alloc((size_t)std::max<int64_t>(c_total, 1), false));
    HIP_TRY(ctx, colsum.alloc((size_t)std::max<int64_t>(Q, 1), false));
    // 1. interior blocks, inverted all at once
    const int64_t Nmax = (int64_t)max_nb * GB;
    hipLaunchKernelGGL(k_sub_blocks_init, dim3((unsigned)grid_for(Nmax * Nmax), (unsigned)P), dim3(BLOCK), 0, ctx->stream,
                       (const int32_t *)d_nbq.p, (const int64_t *)d_moff.p, (const int32_t *)L.part_ptr.p, Mp.p);
    AmgLevel &L0 = *ctx->levels[0];
    const SellPattern &pat = L0.A.pat;
    hipLaunchKernelGGL(k_sub_blocks_scatter, dim3(grid_for((int64_t)pat.n_slices * WAVE)), dim3(BLOCK), 0, ctx->stream, pat.n_slices, nI,
                       (const int32_t *)pat.slice_off.p, (const int32_t *)pat.cols.p, (const double *)L0.A.vals.p,
                       (const int32_t *)L.row_part.p, (const int32_t *)L.part_ptr.p, (const int32_t *)d_nbq.p,
                       (const int64_t *)d_moff.p, Mp.p);
    for (int k = 0; k < max_nb; ++k) {
        hipLaunchKernelGGL(k_gj_panel_batch, dim3((unsigned)max_nb, (unsigned)P), dim3(BLOCK), 0, ctx->stream, k, (const int32_t *)d_nbq.p,
                           (const int64_t *)d_moff.p, (const int64_t *)d_poff.p, (const double *)Mp.p, Pb.p, Wb.p, Db.p, d_flag.p);
        hipLaunchKernelGGL(k_gj_update_batch, dim3((unsigned)(max_nb * (max_nb + 1) / 2), (unsigned)P), dim3(BLOCK), 0, ctx->stream, k,
                           (const int32_t *)d_nbq.p, (const int64_t *)d_moff.p, (const int64_t *)d_poff.p, Mp.p, (const double *)Pb.p,
                           (const double *)Wb.p, (const double *)Db.p);
    }
    // 2. value pool: 1.0, G_p rows and row sums; E_p, -E_p^T, column sums; C_p
    const double one = 1.0;
    HIP_TRY(ctx, hipMemcpyAsync(L.vals.p, &one, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_sub_unpack_G, dim3((unsigned)((nI + BLOCK / WAVE - 1) / (BLOCK / WAVE))), dim3(BLOCK), 0, ctx->stream, nI,
                       (const int32_t *)L.row_part.p, (const int32_t *)L.part_ptr.p, (const int32_t *)d_nbq.p,
                       (const int64_t *)d_moff.p, (const double *)Mp.p, (const int64_t *)d_goff.p, pl->gvec_off, L.vals.p);
    hipLaunchKernelGGL(k_sub_E, dim3((unsigned)Q), dim3(BLOCK), 0, ctx->stream, (const int32_t *)d_pair_part.p,
                       (const int32_t *)L.part_ptr.p, (const int32_t *)L.sep_ptr.p, (const int32_t *)d_ent_ptr.p,
                       (const int32_t *)d_ent_row.p, (const double *)d_ent_val.p, (const int64_t *)d_goff.p, (const int64_t *)d_etoff.p,
                       (const int64_t *)d_eoff.p, L.vals.p, E.p, colsum.p);
    hipLaunchKernelGGL(k_sub_C, dim3((unsigned)Q), dim3(BLOCK), 0, ctx->stream, (const int32_t *)d_pair_part.p,
                       (const int32_t *)L.part_ptr.p, (const int32_t *)L.sep_ptr.p, (const int32_t *)d_ent_ptr.p,
                       (const int32_t *)d_ent_row.p, (const double *)d_ent_val.p, (const int64_t *)d_eoff.p,
                       (const double *)E.p, (const int64_t *)d_coff.p, Cpool.p);
    // 3. Schur complement (+ shift) assembled into the padded matrix, u; pseudo-inverse by the sweep
    {
        const int64_t N = round_up(nS, GB);
        DevBuf<double> M;
        HIP_TRY(ctx, M.alloc((size_t)N * N, false));
        hipLaunchKernelGGL(k_sub_schur_row, dim3((unsigned)N), dim3(BLOCK), 0, ctx->stream, nS, N, s / (double)nS,
                           (const int32_t *)d_ass_p.p, (const int32_t *)d_ass_i.p, (const double *)d_ass_v.p,
                           (const int32_t *)d_node_ptr.p, (const int32_t *)d_node_pair.p, (const int32_t *)d_pair_part.p,
                           (const int32_t *)L.sep_ptr.p, (const int32_t *)L.sep_idx.p, (const int64_t *)d_coff.p,
                           (const double *)Cpool.p, (const double *)colsum.p, M.p, L.u.p);
        HIP_TRY(ctx, hipGetLastError());
        int32_t flag = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&flag, d_flag.p, sizeof(flag), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (flag) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_poisson_build_substructure: an interior block is not positive definite");
        TDGL_TRY(dense_sweep_pack(ctx, M, nS, N, 1.0 / (s * (double)nS), f->dense));
    }
    L.parts = P;
    L.nI = nI;
    L.nS = nS;
    f->levels = 1;
    ctx->direct = std::move(f);
    if (seconds) *seconds = (double)(now_ns() - t_begin) * 1e-9;
    return TDGL_OK;
}
