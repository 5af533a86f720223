// The ensemble's mu solve on the substructured factors (ensemble.inc; the single run's: factors.inc,
// direct_solve_launch_t).  Included from tdgl_hip.hip in front of ensemble.inc.
//
// For R right-hand sides b_r (K2's bvec) mu_r = pinv(A) b_r with the single run's factors and gauge, one or two levels
// of fp64 factors, whole G_p blocks or the 16 x 16 tiles on or below their diagonal.  A workgroup takes a group of
// ENS_SG replicas, so every block of the factors is read from memory once per group and round:
//   S1 k_ens_sub_down       per level: G_p b_p, a LANE per row (G_p is symmetric: column r is row r, one contiguous
//                           request per entry j of the row for the wavefront), the group's b_p in LDS; then the
//                           separator rows and the (G_p 1)^T rows (segment lists), a wavefront per row
//   S2 k_ens_dense_tiles    the last separator's pseudo-inverse (ensemble.inc, K3), and
//   S3 k_ens_sub_top        its slot sums with each replica's share of u . x_S (dense_sym_finish_body)
//   S4 k_ens_sub_mean       the mean of each replica's solution, from the (G_p 1)^T rows of every level and u . x_S
//   S5 k_ens_sub_up         per level, innermost first: x_p = w_p - E_p x_S - mean, x_S = xs - mean, a lane per row,
//                           the group's x_S values gathered into LDS; the inner level leaves the mean alone, the first
//                           removes it and writes mu only for replicas that are live and whose psi update succeeded
//   S6 k_ens_sub_control    the controller per replica, with mu final (step_controller)
// Per replica the arithmetic is the single run's up to the order of the sums inside each product.

namespace tdgl {

constexpr int ENS_SG = 8;    // replicas per workgroup of the substructured solve
constexpr int ENS_SB = 256;  // entries of the group's vectors staged in LDS at a time

// Up to 64 consecutive output rows of one part: out[row0 + l] = sum_j M(j, l) v[j], j < ncol, M as below.
//   ld > 0: M(j, l) = vals[m + j ld + l]      (a whole row-major G_p block, m = entry (0, first row), ld = its rows --
//                                               by symmetry its column; or a -E_p^T block of the way up)
//   ld = 0: M(j, l) = G_p(j, lr0 + l)         (the part's tiles on or below the diagonal start at m)
// The way down reads v = b[x0 ..), the way up v = xs[sep_idx[x0 + j]].
struct EnsSubChunk {
    int64_t m;
    int32_t ld, ncol, x0, row0, n_rows, lr0;
};

__device__ __forceinline__ int64_t ens_sub_at(const EnsSubChunk &ch, int j, int l) {
    if (ch.ld > 0) return ch.m + (int64_t)j * ch.ld + l;
    const int r = ch.lr0 + l, I = j >> 4, J = r >> 4;  // (tile (I, J) holds rows 16 I .., columns 16 J ..; J <= I stored)
    return I >= J ? ch.m + (int64_t)(I * (I + 1) / 2 + J) * 256 + (j & 15) * 16 + (r & 15)
                  : ch.m + (int64_t)(J * (J + 1) / 2 + I) * 256 + (r & 15) * 16 + (j & 15);
}

// The group's replicas that run this round (in LDS); false: every one of them is dead, the workgroup returns.
__device__ __forceinline__ bool ens_group_live(int g0, int R, const StepCtl *__restrict__ ctl, int *sh_live) {
    int live = 0;
    if ((int)threadIdx.x < ENS_SG) {
        live = g0 + (int)threadIdx.x < R ? ctl[g0 + threadIdx.x].live : 0;
        sh_live[threadIdx.x] = live;
    }
    return __syncthreads_or(live) != 0;
}

// acc_out[q][l] (q < ENS_SG, l < 64, in LDS) = the chunk's product for replica g0 + q.  `vec(q, j)` reads entry j of
// replica g0 + q's vector (q clamped to a replica that exists).  The four wavefronts split j; a lane = a row.
template <class V>
__device__ __forceinline__ void ens_sub_product(const EnsSubChunk &ch, const double *__restrict__ vals, V vec,
                                                double (*sh_v)[ENS_SG], double (*sh_acc)[ENS_SG][WAVE]) {
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    const int l = min(lane, ch.n_rows - 1);  // (lanes past the chunk re-read its last row; not stored)
    double acc[ENS_SG];
#pragma unroll
    for (int q = 0; q < ENS_SG; ++q) acc[q] = 0.0;
    for (int j0 = 0; j0 < ch.ncol; j0 += ENS_SB) {
        const int nj = min(ENS_SB, ch.ncol - j0);
        __syncthreads();  // (the previous block has been read by everyone)
        for (int f = threadIdx.x; f < ENS_SG * ENS_SB; f += BLOCK) {
            const int q = f / ENS_SB, j = f % ENS_SB;
            if (j < nj) sh_v[j][q] = vec(q, j0 + j);
        }
        __syncthreads();
        int j = wv;
        for (; j + 3 * (BLOCK / WAVE) < nj; j += 4 * (BLOCK / WAVE)) {  // four entries of the row requested at once
            double g[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] = vals[ens_sub_at(ch, j0 + j + u * (BLOCK / WAVE), l)];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double2 *bv = reinterpret_cast<const double2 *>(sh_v[j + u * (BLOCK / WAVE)]);
#pragma unroll
                for (int q = 0; q < ENS_SG / 2; ++q) {
                    const double2 b = bv[q];
                    acc[2 * q] += g[u] * b.x;
                    acc[2 * q + 1] += g[u] * b.y;
                }
            }
        }
        for (; j < nj; j += BLOCK / WAVE) {
            const double g = vals[ens_sub_at(ch, j0 + j, l)];
            const double2 *bv = reinterpret_cast<const double2 *>(sh_v[j]);
#pragma unroll
            for (int q = 0; q < ENS_SG / 2; ++q) {
                const double2 b = bv[q];
                acc[2 * q] += g * b.x;
                acc[2 * q + 1] += g * b.y;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < ENS_SG; ++q) sh_acc[wv][q][lane] = acc[q];
    __syncthreads();
}

// S1: the way down of one level for the group of replicas blockIdx.y: workgroups [0, nchunk) the interior rows (a chunk
// each), then four rows of the rest per workgroup.  b: the level's vectors (replica stride ldb); out: w (stride ldw).
__global__ __launch_bounds__(BLOCK) void k_ens_sub_down(int nchunk, const EnsSubChunk *__restrict__ chunks, int64_t nI, int64_t n_rows,
                                                        const int32_t *__restrict__ seg_ptr, const int64_t *__restrict__ seg_val,
                                                        const int32_t *__restrict__ seg_x, const int32_t *__restrict__ seg_len,
                                                        const double *__restrict__ vals, const double *__restrict__ b, int64_t ldb,
                                                        double *__restrict__ out, int64_t ldw, int R, const StepCtl *__restrict__ ctl) {
    __shared__ __align__(16) double sh_v[ENS_SB][ENS_SG];
    __shared__ double sh_acc[BLOCK / WAVE][ENS_SG][WAVE];
    __shared__ int sh_live[ENS_SG];
    const int g0 = blockIdx.y * ENS_SG;
    if (!ens_group_live(g0, R, ctl, sh_live)) return;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    if ((int)blockIdx.x < nchunk) {
        const EnsSubChunk ch = chunks[blockIdx.x];
        ens_sub_product(ch, vals, [&](int q, int j) { return b[(int64_t)min(g0 + q, R - 1) * ldb + ch.x0 + j]; }, sh_v, sh_acc);
        for (int o = threadIdx.x; o < ENS_SG * WAVE; o += BLOCK) {
            const int q = o / WAVE, l = o % WAVE;
            if (l < ch.n_rows && g0 + q < R)
                out[(int64_t)(g0 + q) * ldw + ch.row0 + l] = (sh_acc[0][q][l] + sh_acc[1][q][l]) + (sh_acc[2][q][l] + sh_acc[3][q][l]);
        }
        return;
    }
    const int64_t row = nI + (int64_t)(blockIdx.x - nchunk) * (BLOCK / WAVE) + wv;
    if (row >= n_rows) return;
    const double *bq[ENS_SG];
#pragma unroll
    for (int q = 0; q < ENS_SG; ++q) bq[q] = b + (int64_t)min(g0 + q, R - 1) * ldb;
    double acc[ENS_SG];
#pragma unroll
    for (int q = 0; q < ENS_SG; ++q) acc[q] = 0.0;
    for (int k = seg_ptr[row]; k < seg_ptr[row + 1]; ++k) {
        const double *__restrict__ v = vals + seg_val[k];
        const int x = seg_x[k], len = seg_len[k];
        for (int c = lane; c < len; c += WAVE) {
            const double a = v[c];
#pragma unroll
            for (int q = 0; q < ENS_SG; ++q) acc[q] += a * bq[q][x + c];
        }
    }
#pragma unroll
    for (int q = 0; q < ENS_SG; ++q) acc[q] = wave_sum(acc[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < ENS_SG; ++q)
            if (g0 + q < R) out[(int64_t)(g0 + q) * ldw + row] = acc[q];
    }
}

// S3: x_S of every live replica = the slot sums of S2, and its workgroup's share of u . x_S
__global__ __launch_bounds__(BLOCK) void k_ens_sub_top(int n, int nt, const double *__restrict__ part, int64_t ldpart,
                                                       double *__restrict__ xs, const double *__restrict__ u, double *__restrict__ upart,
                                                       int nfin, const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    if (!ctl[r].live) return;
    dense_sym_finish_body(blockIdx.x, n, nt, part + (int64_t)r * ldpart, finish_separator(xs + (int64_t)r * n, u, upart + (int64_t)r * nfin));
}

// S4: mean[r] = inv_n (sum of the (G_p 1)^T rows of every level + sum of the shares of u . x_S), a workgroup per replica
// (SubMean of the single run: there the first level's way up forms it, or the inner level's leaves it behind)
__global__ __launch_bounds__(BLOCK) void k_ens_sub_mean(const double *__restrict__ a, int na, int64_t lda, const double *__restrict__ c,
                                                        int nc, int64_t ldc, const double *__restrict__ upart, int nfin, double inv_n,
                                                        double *__restrict__ mean, const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.x;
    if (!ctl[r].live) return;
    double v = 0.0;
    for (int i = threadIdx.x; i < na; i += BLOCK) v += a[(int64_t)r * lda + i];
    for (int i = threadIdx.x; i < nfin; i += BLOCK) v += upart[(int64_t)r * nfin + i];
    for (int i = threadIdx.x; i < nc; i += BLOCK) v += c[(int64_t)r * ldc + i];
    const double tot = block_sum(v);
    if (threadIdx.x == 0) mean[r] = tot * inv_n;
}

// S5: the way up of one level for the group blockIdx.y: workgroups [0, nchunk) the interior rows, then the separator
// rows (BLOCK each).  out = w + (-E^T)^T x_S - mean per replica; mean = NULL: none (an inner level).  fail_part != NULL
// (the first level, out = mu): nothing is written for a replica that is not live or whose psi update failed this round.
__global__ __launch_bounds__(BLOCK) void k_ens_sub_up(int nchunk, const EnsSubChunk *__restrict__ chunks, int64_t nI, int64_t nS,
                                                      const int32_t *__restrict__ sep_idx, const double *__restrict__ vals,
                                                      const double *__restrict__ w, int64_t ldw, const double *__restrict__ xs,
                                                      int64_t ldxs, const double *__restrict__ mean, const int32_t *__restrict__ fail_part,
                                                      int nfail, double *__restrict__ out, int64_t ldo, int R,
                                                      const StepCtl *__restrict__ ctl) {
    __shared__ __align__(16) double sh_v[ENS_SB][ENS_SG];
    __shared__ double sh_acc[BLOCK / WAVE][ENS_SG][WAVE];
    __shared__ int sh_live[ENS_SG];
    __shared__ int sh_bad[ENS_SG];
    __shared__ double sh_mean[ENS_SG];
    const int g0 = blockIdx.y * ENS_SG;
    if ((int)threadIdx.x < ENS_SG) sh_bad[threadIdx.x] = 0;
    if (!ens_group_live(g0, R, ctl, sh_live)) return;  // (its barrier also orders sh_bad)
    if ((int)threadIdx.x < ENS_SG) sh_mean[threadIdx.x] = mean && sh_live[threadIdx.x] ? mean[g0 + threadIdx.x] : 0.0;
    if (fail_part && nfail > 0)
        for (int f = threadIdx.x; f < ENS_SG * nfail; f += BLOCK) {
            const int q = f / nfail;
            if (g0 + q < R && fail_part[(int64_t)(g0 + q) * nfail + f % nfail]) sh_bad[q] = 1;  // (every writer writes 1)
        }
    __syncthreads();
    if ((int)blockIdx.x < nchunk) {
        const EnsSubChunk ch = chunks[blockIdx.x];
        ens_sub_product(ch, vals, [&](int q, int j) { return xs[(int64_t)min(g0 + q, R - 1) * ldxs + sep_idx[ch.x0 + j]]; }, sh_v, sh_acc);
        for (int o = threadIdx.x; o < ENS_SG * WAVE; o += BLOCK) {
            const int q = o / WAVE, l = o % WAVE;
            if (l < ch.n_rows && g0 + q < R && sh_live[q] && !sh_bad[q]) {
                const int64_t row = ch.row0 + l;
                const double acc = (sh_acc[0][q][l] + sh_acc[1][q][l]) + (sh_acc[2][q][l] + sh_acc[3][q][l]);
                out[(int64_t)(g0 + q) * ldo + row] = w[(int64_t)(g0 + q) * ldw + row] + acc - sh_mean[q];  // (the pool holds -E^T)
            }
        }
        return;
    }
    const int64_t i = (int64_t)(blockIdx.x - nchunk) * BLOCK + threadIdx.x;
    if (i >= nS) return;
#pragma unroll
    for (int q = 0; q < ENS_SG; ++q)
        if (g0 + q < R && sh_live[q] && !sh_bad[q]) out[(int64_t)(g0 + q) * ldo + nI + i] = xs[(int64_t)(g0 + q) * ldxs + i] - sh_mean[q];
}

// S6: the controller of every live replica (k_ens_finish's second half), a workgroup per replica
__global__ __launch_bounds__(BLOCK) void k_ens_sub_control(const double *__restrict__ dmax_part, const int32_t *__restrict__ fail_part,
                                                           int nfail, StepCtl *__restrict__ ctl, StepRec *__restrict__ rec,
                                                           const int32_t *__restrict__ limit) {
    const int r = blockIdx.x;
    StepCtl *c = ctl + r;
    if (!c->live) return;
    double m;
    int f;
    reduce_psi_status(dmax_part + (int64_t)r * nfail, fail_part + (int64_t)r * nfail, nfail, &m, &f);
    if (threadIdx.x == 0) {
        step_controller(c, rec + (int64_t)r * RA_BATCH_MAX, m, f);
        if (!c->poisoned && c->n_acc >= limit[r]) c->poisoned = 1;
    }
}

}  // namespace tdgl
