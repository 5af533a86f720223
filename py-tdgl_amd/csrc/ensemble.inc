// Ensemble of R independent replicas of one device in one batched time loop (include/tdgl_hip.h:
// tdgl_ensemble_*).  Included at the end of tdgl_hip.hip.
//
// The replicas share the context's mesh, SELL-64 pattern and dense inverse G (tdgl_poisson_build_dense_inverse);
// each has its own link variables (and covariant-Laplacian values), boundary term of the Poisson right-hand side,
// epsilon, state (psi, L psi double-buffered, mu) and controller (a StepCtl in device memory).  The loop is the
// run-ahead loop of run.inc with the replica as a grid dimension: one ROUND is one attempt per live replica, five
// launches over all replicas,
//   K1 k_ens_psi_update      psi update (psi_update_body) per replica
//   K2 k_ens_laplacian       L psi' and the Poisson right-hand side (psi_laplacian_body<true>) per replica
//   K3 k_ens_dense_tiles     G [b_1 .. b_R]: each symmetric tile read once per 16 replicas, used for its block
//                            and its transpose
//   K4 k_ens_finish          slot sums of K3 (dense_sym_finish_body) and the controller (step_controller) per replica
//   K5 k_ens_probes          probe read-outs of the accepted attempts
// (above the dense inverse's cap K3 / K4 become the substructured solve's S1 - S6, ensemble_sub.inc)
// and the host synchronises once per batch of rounds.  A failed psi update is that replica's next attempt, with
// the smaller dt, in the next round; a replica that has reached its end time, spent its retry budget or taken the
// steps asked of this call is poisoned and its launches return at once.  Per replica the arithmetic is that of the
// run-ahead loop, operation for operation, except for the order of the sums inside the dense product.
//
// Per-replica inputs are formed by the context's own entry points (tdgl_set_link_exponents, tdgl_set_mu_boundary,
// tdgl_set_epsilon, tdgl_set_state: the site / edge permutations, the link variables, the boundary term) and copied
// from the context's buffers into the replica's; the context's own run state is scratch for the ensemble.

#include <memory>

namespace tdgl {

constexpr int ENS_RG = 16;  // replicas per workgroup of the dense product
constexpr int ENS_CH = 16;  // tile rows per LDS chunk

__global__ __launch_bounds__(BLOCK) void k_ens_psi_update(int64_t n, int64_t n_pad, double2 *__restrict__ psi0, double2 *__restrict__ psi1,
                                                          const double2 *__restrict__ lap0, const double2 *__restrict__ lap1,
                                                          const double *__restrict__ mu, const double *__restrict__ eps, double u,
                                                          double gamma, double *__restrict__ dmax_part, int32_t *__restrict__ fail_part,
                                                          StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    StepCtl *c = ctl + r;
    if (c->poisoned) {  // (uniform over the replica's workgroups: `poisoned` only changes in K4)
        if (blockIdx.x == 0 && threadIdx.x == 0) c->live = 0;
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) c->live = 1;
    const int64_t o = (int64_t)r * n_pad;
    const bool c1 = c->cur != 0;
    psi_update_body(blockIdx.x, gridDim.x, n, (c1 ? psi1 : psi0) + o, mu + o, eps + o, (c1 ? lap1 : lap0) + o, c->attempt_dt, u, gamma,
                    (c1 ? psi0 : psi1) + o, nullptr, dmax_part + (int64_t)r * gridDim.x, fail_part + (int64_t)r * gridDim.x, nullptr);
}

template <class IT>
__global__ __launch_bounds__(BLOCK) void k_ens_laplacian(int n_slices, int per_xcd, int64_t n_rows, const int32_t *__restrict__ slice_off,
                                                         const IT *__restrict__ cols, const double2 *__restrict__ vals, int64_t n_slots,
                                                         const double *__restrict__ diag, const uint8_t *__restrict__ fixed,
                                                         const double2 *__restrict__ psi0, const double2 *__restrict__ psi1,
                                                         double2 *__restrict__ lap0, double2 *__restrict__ lap1, const double *__restrict__ area,
                                                         const double *__restrict__ ceff, double *__restrict__ bvec, int64_t n_pad,
                                                         const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    const StepCtl *c = ctl + r;
    if (!c->live) return;
    const bool to1 = c->cur == 0;
    const int64_t o = (int64_t)r * n_pad;
    psi_laplacian_body<true, IT>(n_slices, per_xcd, 0, n_rows, slice_off, cols, vals + (int64_t)r * n_slots, diag, fixed,
                                 (to1 ? psi1 : psi0) + o, (to1 ? lap1 : lap0) + o, area, ceff + o, bvec + o);
}

// Y = G B on the symmetric tiles of k_dense_sym_tiles (tile (I, J), J <= I, DT x DT, row major), B = [b_1 .. b_R] with
// replica r's vector at b + r * ldb.  Workgroup (t, g): tile t for the replicas 16 g .. 16 g + 15.  The tile streams
// through LDS in chunks of ENS_CH rows; both b blocks of the 16 replicas sit in LDS for the whole tile.
//   transpose part  y_J[c][q] += sum_r T[r][c] b_I[r][q]: thread = 4 columns (c0 + 32 k) x 2 replicas, summed over
//                   the tile's rows in registers; 8 FMAs per 6 LDS reads;
//   block part      y_I[r][q] += sum_c T[r][c] b_J[c][q]: per chunk, thread = 4 rows x 4 replicas x 1/16 of the
//                   columns (16 FMAs per 8 LDS reads), the 16 column slices summed by a butterfly over 16 lanes.
// The two contributions go to the fixed slots of `part` the single-vector kernel uses (slot J of row block I, slot I
// of row block J), per replica at part + r * ldpart: no atomics, the result does not depend on the schedule.
// Plain fp64 FMAs: gfx950's fp64 matrix instructions run at the vector rate (78.6 TF either way, spec), so they
// buy nothing here, and the kernel is bound by LDS and the stream of G, not by the FMA rate.
__global__ __launch_bounds__(BLOCK) void k_ens_dense_tiles(int n, int nt, const double *__restrict__ Gp, const double *__restrict__ b,
                                                           int64_t ldb, double *__restrict__ part, int64_t ldpart, int R,
                                                           const StepCtl *__restrict__ ctl) {
    __shared__ double sT[ENS_CH][DT];
    __shared__ double sBI[DT][ENS_RG + 1];  // (+1: the block part's reads of 16 rows x 4 replicas spread over the banks)
    __shared__ double sBJ[DT][ENS_RG + 1];
    const int tid = threadIdx.x;
    const int g0 = blockIdx.y * ENS_RG;
    int live = 0;
    if (tid < ENS_RG && g0 + tid < R) live = ctl[g0 + tid].live;
    if (!__syncthreads_or(live)) return;  // (every replica of the group is dead this round)
    const int t = blockIdx.x;
    int I = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    while (I * (I + 1) / 2 > t) --I;
    const int J = t - I * (I + 1) / 2;
    for (int f = tid; f < ENS_RG * DT; f += BLOCK) {
        const int q = f / DT, c = f % DT;
        const bool okq = g0 + q < R;
        const int ri = I * DT + c, cj = J * DT + c;
        sBI[c][q] = okq && ri < n ? b[(int64_t)(g0 + q) * ldb + ri] : 0.0;
        sBJ[c][q] = okq && cj < n ? b[(int64_t)(g0 + q) * ldb + cj] : 0.0;
    }
    const double2 *__restrict__ g = reinterpret_cast<const double2 *>(Gp + (int64_t)t * DT * DT);
    // transpose part: columns cg + 32 k, replicas 2 gp, 2 gp + 1
    const int cg = tid & 31, gp = tid >> 5;
    double accT[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    // block part: rows 4 rq .. 4 rq + 3 of the chunk (rq = the wave), replicas 4 gq .. 4 gq + 3, columns ks + 16 j
    const int rq = tid >> 6, gq = (tid >> 4) & 3, ks = tid & 15;
    const int64_t ldp = (int64_t)nt * DT;
    constexpr int PER = ENS_CH * DT / 2 / BLOCK;  // double2 loads per thread and chunk
    for (int r0 = 0; r0 < DT; r0 += ENS_CH) {
        double2 v[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) v[k] = g[(int64_t)r0 * (DT / 2) + tid + k * BLOCK];
        __syncthreads();  // (the previous chunk has been read by everyone; the first time: the b blocks are in place)
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int f = 2 * (tid + k * BLOCK);
            sT[f / DT][f % DT] = v[k].x;
            sT[f / DT][f % DT + 1] = v[k].y;
        }
        __syncthreads();
        if (I != J) {  // (workgroup-uniform; a diagonal tile holds its whole block: the block part alone covers it)
#pragma unroll 4
            for (int k = 0; k < ENS_CH; ++k) {
                const double bi0 = sBI[r0 + k][2 * gp], bi1 = sBI[r0 + k][2 * gp + 1];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double tv = sT[k][cg + 32 * q];
                    accT[q][0] += tv * bi0;
                    accT[q][1] += tv * bi1;
                }
            }
        }
        double acc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0.0;
#pragma unroll
        for (int j = 0; j < DT / 16; ++j) {
            const int c = ks + 16 * j;
            double tv[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) tv[i] = sT[4 * rq + i][c];
#pragma unroll
            for (int q = 0; q < 4; ++q) bv[q] = sBJ[c][4 * gq + q];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[4 * i + q] += tv[i] * bv[q];
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] += __shfl_xor(acc[k], off, WAVE);
        {  // lane ks stores entry ks = 4 i + q
            double mine = acc[0];
#pragma unroll
            for (int k = 1; k < 16; ++k) mine = ks == k ? acc[k] : mine;
            const int i = ks >> 2, q = g0 + 4 * gq + (ks & 3);
            if (q < R) part[(int64_t)q * ldpart + (int64_t)J * ldp + I * DT + r0 + 4 * rq + i] = mine;
        }
    }
    if (I != J) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int q = g0 + 2 * gp + e;
            if (q >= R) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) part[(int64_t)q * ldpart + (int64_t)I * ldp + J * DT + cg + 32 * k] = accT[k][e];
        }
    }
}

// mu of every replica whose psi update succeeded = the slot sums of K3; the replica's controller.  A replica that has
// taken the steps asked of this call (limit) is poisoned like one that reached its end time.
__global__ __launch_bounds__(BLOCK) void k_ens_finish(int n, int nt, const double *__restrict__ part, int64_t ldpart,
                                                      const double *__restrict__ dmax_part, const int32_t *__restrict__ fail_part,
                                                      int nfail, double *__restrict__ mu, int64_t n_pad, StepCtl *__restrict__ ctl,
                                                      StepRec *__restrict__ rec, const int32_t *__restrict__ limit) {
    const int r = blockIdx.y;
    StepCtl *c = ctl + r;
    DenseFinish fin = finish_product(mu + (int64_t)r * n_pad);  // (the whole-matrix inverse inside a step: factors.inc)
    fin.dmax_part = dmax_part + (int64_t)r * nfail, fin.fail_part = fail_part + (int64_t)r * nfail, fin.nfail = nfail, fin.guard = 1;
    fin.ctl = c, fin.rec = rec + (int64_t)r * RA_BATCH_MAX;
    dense_sym_finish_body(blockIdx.x, n, nt, part + (int64_t)r * ldpart, fin);
    if (blockIdx.x == 0 && threadIdx.x == 0 && c->live && !c->poisoned && c->n_acc >= limit[r]) c->poisoned = 1;
}

// probe read-outs of an accepted attempt into slot n_acc - 1 of the replica's records (k_ra_probes per replica)
__global__ void k_ens_probes(int n_probe, const int32_t *__restrict__ sites, const double2 *__restrict__ psi0,
                             const double2 *__restrict__ psi1, const double *__restrict__ mu, int64_t n_pad, double *__restrict__ ring,
                             const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    const StepCtl *c = ctl + r;
    if (!c->live || !c->last_ok) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_probe) return;
    const int s = sites[k];
    const int64_t o = (int64_t)r * n_pad;
    const double2 p = (c->cur != 0 ? psi1 : psi0)[o + s];  // (the controller has flipped cur: psi^{n+1})
    double *__restrict__ out = ring + ((int64_t)r * RA_BATCH_MAX + c->n_acc - 1) * 2 * n_probe;
    out[k] = mu[o + s];
    out[n_probe + k] = atan2(p.y, p.x);
}

// ---- time-dependent inputs per replica, queued in front of K1 (run.inc's run-ahead loop, the replica as grid.y) ----
// A replica's moving applied field (FieldDrive: a single ramped or tabulated product, or a sum of terms) moves in three
// launches over the replicas -- R1 the step rule (field_begin_body), R2 A, A_prev, dA/dt and "did it move" (field_link_body),
// R3 ceff with the dA/dt term and
// the link variables (ceff_body, link_variable_body) -- and two more rebuild what depends on the links: R4 the
// covariant-Laplacian values (fill_laplacian_body) and R5 L psi^n with them (psi_laplacian_body).  Retries, dead
// replicas and replicas whose field does not move this step return at once (ramp_do, moved).  Tabulated terminal
// currents (T1, mu_table_body: one workgroup per replica) and separable epsilon (T2, eps_table_body) are evaluated at
// the replica's own time.  Every body is the single run's, so each replica's arithmetic is its run-ahead loop's.

// R1: one thread per replica.  move[r]: the replica's field moves in this batch (else ramp_do = 0, as the single run that
// queues no field launch at all).  term: FIELD_TERMS_MAX descriptors per replica whose table nodes are offsets into the pools
__global__ void k_ens_field_begin(int R, StepCtl *__restrict__ ctl, const int32_t *__restrict__ move, const FieldTerm *__restrict__ term,
                                  const double *__restrict__ times, const double *__restrict__ values, int32_t *__restrict__ moved) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    if (move[r])
        field_begin_body(ctl + r, term + (int64_t)r * FIELD_TERMS_MAX, times, values, nullptr, nullptr, 0);
    else
        ctl[r].ramp_do = 0;
    moved[r] = 0;
}

// R2: moved[r] = OR over the replica's workgroups (k_field_links + k_any_flag).  bases[r], a0[r]: the replica's own bases
// (slots of 2 m_pad) and static part (or nullptr)
__global__ __launch_bounds__(BLOCK) void k_ens_field_links(int64_t m, int64_t m_pad, const double *const *__restrict__ bases,
                                                           const double *const *__restrict__ a0, double *__restrict__ A,
                                                           double *__restrict__ Aprev, const double *__restrict__ dx,
                                                           const double *__restrict__ dy, const double *__restrict__ inv_len,
                                                           double *__restrict__ dadt, int32_t *__restrict__ moved,
                                                           const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    const StepCtl *c = ctl + r;
    if (!c->ramp_do) return;
    const int64_t e = blockIdx.x * (int64_t)BLOCK + threadIdx.x, o2 = 2 * (int64_t)r * m_pad;
    const int changed = e < m ? field_link_body<false>(e, m, field_values_of(c), LoopGeom{}, reinterpret_cast<const double2 *>(bases[r]), m_pad,
                                                       reinterpret_cast<const double2 *>(a0[r]), nullptr, A + o2, Aprev + o2, dx, dy, inv_len,
                                                       dadt + (int64_t)r * m_pad)
                              : 0;
    const int any = __syncthreads_or(changed);
    if (threadIdx.x == 0 && any) atomicOr(moved + r, 1);
}

// R3: workgroups [0, nblk_ceff): ceff = cvec + div dA/dt (k_ceff); the rest: the link variables where A moved
// (k_link_variables)
__global__ __launch_bounds__(BLOCK) void k_ens_ceff_links(int nblk_ceff, int n_slices, int64_t n_rows, const int32_t *__restrict__ slice_off,
                                                          const int32_t *__restrict__ slot_edge, const double *__restrict__ slot_w,
                                                          const double *__restrict__ inv_len, const double *__restrict__ dadt,
                                                          const double *__restrict__ cvec, double *__restrict__ ceff, int64_t n_pad,
                                                          int64_t m, int64_t m_pad, const double *__restrict__ A, const double *__restrict__ dx,
                                                          const double *__restrict__ dy, double2 *__restrict__ U,
                                                          const int32_t *__restrict__ moved, const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    if (!ctl[r].ramp_do) return;
    if ((int)blockIdx.x < nblk_ceff) {
        const int slice = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
        if (slice >= n_slices) return;
        const int lane = threadIdx.x & (WAVE - 1);
        const int64_t row = (int64_t)slice * WAVE + lane;
        if (row >= n_rows) return;
        const int64_t o = (int64_t)r * n_pad;
        ceff_body(slice, lane, row, slice_off, slot_edge, slot_w, inv_len, dadt + (int64_t)r * m_pad, cvec + o, ceff + o);
        return;
    }
    if (!moved[r]) return;
    const int64_t e = (blockIdx.x - nblk_ceff) * (int64_t)BLOCK + threadIdx.x;
    if (e < m) link_variable_body(e, A + 2 * (int64_t)r * m_pad, nullptr, dx, dy, U + (int64_t)r * m_pad);
}

// R4: covariant-Laplacian values of the replicas whose links moved (k_fill_laplacian)
__global__ __launch_bounds__(BLOCK) void k_ens_fill_laplacian(int64_t n_slots, const int32_t *__restrict__ slot_edge,
                                                              const double *__restrict__ slot_w, const double2 *__restrict__ U,
                                                              int64_t m_pad, double2 *__restrict__ vals, const int32_t *__restrict__ moved) {
    const int r = blockIdx.y;
    const int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (s >= n_slots || !moved[r]) return;
    fill_laplacian_body(s, slot_edge, slot_w, U + (int64_t)r * m_pad, vals + (int64_t)r * n_slots);
}

// R5: L psi^n with the links of this step (k_psi_laplacian_ra_fresh)
template <class IT>
__global__ __launch_bounds__(BLOCK) void k_ens_laplacian_fresh(int n_slices, int per_xcd, int64_t n_rows, const int32_t *__restrict__ slice_off,
                                                               const IT *__restrict__ cols, const double2 *__restrict__ vals, int64_t n_slots,
                                                               const double *__restrict__ diag, const uint8_t *__restrict__ fixed,
                                                               const double2 *__restrict__ psi0, const double2 *__restrict__ psi1,
                                                               double2 *__restrict__ lap0, double2 *__restrict__ lap1, int64_t n_pad,
                                                               const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    const StepCtl *c = ctl + r;
    if (!c->ramp_do) return;
    const bool c1 = c->cur != 0;
    const int64_t o = (int64_t)r * n_pad;
    psi_laplacian_body<false, IT>(n_slices, per_xcd, 0, n_rows, slice_off, cols, vals + (int64_t)r * n_slots, diag, fixed,
                                  (c1 ? psi1 : psi0) + o, (c1 ? lap1 : lap0) + o, nullptr, nullptr, nullptr);
}

// T1: replica r's current table (nodes t_off[r] .. t_off[r + 1] of the pool, densities from d_off[r]) at its time
// (k_ra_mu_table); replicas without a table and dead replicas return
__global__ __launch_bounds__(BLOCK) void k_ens_mu_table(int nb, int n_sites, const int32_t *__restrict__ b_sites,
                                                        const int32_t *__restrict__ s0, const int32_t *__restrict__ s1,
                                                        const double *__restrict__ c0, const double *__restrict__ c1,
                                                        double *__restrict__ mu_b, double *__restrict__ cvec, double *__restrict__ ceff,
                                                        int64_t n_pad, const int32_t *__restrict__ t_off, const int64_t *__restrict__ d_off,
                                                        const double *__restrict__ times, const double *__restrict__ dens,
                                                        const int32_t *__restrict__ group, const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    const StepCtl *c = ctl + r;
    const int t0 = t_off[r], nn = t_off[r + 1] - t0;
    if (nn == 0 || c->poisoned) return;
    const int64_t o = (int64_t)r * n_pad;
    mu_table_body(nb, n_sites, b_sites, s0, s1, c0, c1, mu_b + (int64_t)r * nb, cvec + o, ceff + o, nn, times + t0, dens + d_off[r],
                  group + (int64_t)r * nb, c->time);
}

// T2: epsilon = factor_r(t) epsilon0_r (k_ra_eps_table); nodes e_off[r] .. e_off[r + 1] of the pools
__global__ __launch_bounds__(BLOCK) void k_ens_eps_table(int64_t n_pad, const double *__restrict__ eps0, double *__restrict__ eps,
                                                         const int32_t *__restrict__ e_off, const double *__restrict__ times,
                                                         const double *__restrict__ factor, const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    const StepCtl *c = ctl + r;
    const int t0 = e_off[r], nn = e_off[r + 1] - t0;
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (nn == 0 || c->poisoned || i >= n_pad) return;
    const int64_t o = (int64_t)r * n_pad;
    eps_table_body(i, eps0 + o, eps + o, nn, times + t0, factor + t0, c->time);
}

// T3: epsilon = epsilon0_r - replica r's hot spots (k_eps_spots) at its own time; tabs[r]: where its nodes lie in the pool
// (n = 0: the replica has no spots and returns at once).  xy: the ensemble's site coordinates
__global__ __launch_bounds__(BLOCK) void k_ens_eps_spots(int64_t n_pad, const double2 *__restrict__ xy, const double *__restrict__ eps0,
                                                         double *__restrict__ eps, const EpsSpotTabs *__restrict__ tabs,
                                                         const double *__restrict__ pool, const StepCtl *__restrict__ ctl) {
    const int r = blockIdx.y;
    const StepCtl *c = ctl + r;
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (tabs[r].n == 0 || c->poisoned || i >= n_pad) return;
    const int64_t o = (int64_t)r * n_pad;
    eps_spots_body(i, eps_spot_values_at(tabs[r], pool, c->time), xy, eps0 + o, eps + o);
}

}  // namespace tdgl

struct EnsReplica {
    LoopState loop;  // controller, loop, retry and field state: the host's mirror of the replica's StepCtl
    bool have_ctl = false, have_links = false, have_eps = false, have_state = false, lap_valid = false;
    FieldArrays field;  // a moving field: the replica's own bases and A_0 (its descriptors and tables live in the ensemble's pools)
    MuTable mu_tab;    // tabulated terminal currents / separable epsilon: the host's nodes (their device copy is the ensemble's pools)
    EpsTable eps_tab;
    EpsSpots eps_spots;  // hot spots in epsilon: likewise (and the site coordinates are the ensemble's)
};

struct tdgl_ensemble {
    tdgl_ctx *ctx = nullptr;
    int R = 0, nt = 0, np_ = 0;
    int64_t n = 0, n_pad = 0, m_pad = 0, n_slots = 0, ldpart = 0;
    int batch = 4;  // rounds per synchronisation: doubles up to RA_BATCH_MAX
    DevBuf<double2> U, lapv, psi0, psi1, lap0, lap1;
    DevBuf<double> ceff, eps, mu, bvec, part, dmax_part, probe;
    DevBuf<int32_t> fail_part, limit, d_probes;
    DevBuf<StepCtl> d_ctl;
    DevBuf<StepRec> d_rec;
    // time-dependent inputs (allocated when the first replica asks): per replica A, A_prev (2 m_pad), dA/dt
    // (m_pad), the boundary term before dA/dt (n_pad), mu_boundary (nb), epsilon0 (n_pad); the tables as pools
    DevBuf<double> A, Aprev, dadt, cvec, mu_b, eps0;
    DevBuf<double> mu_t, mu_dens, eps_t, eps_f;
    DevBuf<double2> spot_xy;            // hot spots: the site coordinates [n_pad], stored once ...
    DevBuf<double> spot_pool;           // ... and every replica's nodes
    DevBuf<EpsSpotTabs> spot_tabs;      // [R]
    DevBuf<int32_t> mu_toff, mu_group, eps_off, ramping, moved;  // ramping[r]: the replica's field moves in this batch
    DevBuf<int64_t> mu_doff;
    // the moving fields: per replica FIELD_TERMS_MAX descriptors, the pools of their tables' nodes, the replicas' bases and A_0
    DevBuf<FieldTerm> term_desc;
    DevBuf<double> tab_term_t, tab_term_v;
    DevBuf<const double *> term_bases, term_a0;
    bool tables_dirty = true, any_mu_table = false, any_eps_table = false, any_eps_spots = false;  // (dirty: the pools and their offsets exist from the first run on)
    std::vector<int32_t> h_ramping;
    std::vector<StepCtl> h_ctl;
    std::vector<StepRec> h_rec;
    std::vector<double> h_probe;
    // the census of every replica (census.inc; tdgl_ensemble_set_census): the batch's rows [R][RA_BATCH_MAX][ncol] with
    // zero counters before every batch, and per replica the rows of the last tdgl_ensemble_run
    bool census_on = false;
    int64_t census_serial = 0;  // Census::serial of the context's census that was taken over
    DevBuf<int32_t> census;
    std::vector<int32_t> h_census;
    std::vector<std::vector<int32_t>> census_rows;
    std::vector<int32_t> h_limit;
    std::vector<EnsReplica> rep;
    int64_t stat_rounds = 0, stat_batches = 0;
    // the mu solve on the substructured factors (levels > 0; ensemble_sub.inc): the factors it was set up for, per level
    // the work lists of the ways down and up and the replicas' w [R][ldw] and x_S [R][nS]; the shares of u . x_S, the means
    int levels = 0;
    const DirectFactors *fac = nullptr;
    int64_t factor_bytes = 0;  // bytes of the factors one round reads (every block once per group of replicas)
    DevBuf<EnsSubChunk> sub_down[2], sub_up[2];
    int n_down[2] = {0, 0}, n_up[2] = {0, 0};
    DevBuf<double> sub_w[2], sub_xs[2], upart, mean;
    int64_t ldw[2] = {0, 0};
};

// The ensemble's work lists of one level (EnsSubChunk: chunks of at most 64 rows) from the single run's: whole G_p blocks
// (k_sub_down's chunks of 32 rows, the first of a part at its first row) or a part's tiles (k_sub_down_sym: one chunk
// per part), and the way up's chunks (of 64 rows, or whole parts).  Every chunk is checked against the level's arrays.
static int ens_sub_lists(tdgl_ctx *ctx, const SubLevel &L, int64_t n, DevBuf<EnsSubChunk> &down, int &n_down, DevBuf<EnsSubChunk> &up,
                         int &n_up) {
    const char *who = "tdgl_ensemble_create";
    std::vector<SubDownChunk> dc(L.down_chunks.n);
    std::vector<SubUpChunk> uc(L.up_chunks.n);
    if (!dc.empty()) HIP_TRY(ctx, hipMemcpy(dc.data(), L.down_chunks.p, dc.size() * sizeof(SubDownChunk), hipMemcpyDeviceToHost));
    if (!uc.empty()) HIP_TRY(ctx, hipMemcpy(uc.data(), L.up_chunks.p, uc.size() * sizeof(SubUpChunk), hipMemcpyDeviceToHost));
    const bool tiles = L.sym_lds > 0;
    const int64_t nv = (int64_t)L.vals.n;
    std::vector<EnsSubChunk> d, u;
    for (const SubDownChunk &c : dc) {
        if (c.n_rows <= 0 || (!tiles && c.row0 != c.x0)) continue;  // (whole blocks: a part once, from its first chunk)
        const int32_t np_ = c.ncols;
        const int64_t nt = (np_ + ST - 1) / ST;
        const bool ok = np_ > 0 && c.x0 >= 0 && c.x0 + (int64_t)np_ <= L.nI && c.g >= 0 &&
                        (tiles ? c.g + nt * (nt + 1) / 2 * (ST * ST) <= nv : c.g + (int64_t)np_ * np_ <= nv);
        if (!ok) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: the factors' way-down work list is inconsistent", who);
        for (int32_t r0 = 0; r0 < np_; r0 += WAVE)
            d.push_back(EnsSubChunk{tiles ? c.g : c.g + r0, tiles ? 0 : np_, np_, c.x0, c.x0 + r0, std::min<int32_t>(WAVE, np_ - r0), r0});
    }
    for (const SubUpChunk &c : uc) {
        if (c.n_rows <= 0) continue;
        const bool ok = c.np >= c.n_rows && c.cnt >= 0 && c.s0 >= 0 && c.s0 + (int64_t)c.cnt <= (int64_t)L.sep_idx.n && c.row0 >= 0 &&
                        c.row0 + (int64_t)c.n_rows <= L.nI && c.et >= 0 &&
                        (c.cnt == 0 || c.et + (int64_t)(c.cnt - 1) * c.np + c.n_rows <= nv);
        if (!ok) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: the factors' way-up work list is inconsistent", who);
        for (int32_t r0 = 0; r0 < c.n_rows; r0 += WAVE)
            u.push_back(EnsSubChunk{c.et + r0, c.np, c.cnt, c.s0, c.row0 + r0, std::min<int32_t>(WAVE, c.n_rows - r0), 0});
    }
    int64_t rows = 0;
    for (const EnsSubChunk &c : d) rows += c.n_rows;
    if (rows != L.nI || L.nI + L.nS != n) TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: the factors' work lists do not cover the level", who);
    n_down = (int)d.size();
    n_up = (int)u.size();
    if (d.empty()) d.push_back(EnsSubChunk{0, 0, 0, 0, 0, 0, 0});
    if (u.empty()) u.push_back(EnsSubChunk{0, 0, 0, 0, 0, 0, 0});
    HIP_TRY(ctx, down.upload(d));
    HIP_TRY(ctx, up.upload(u));
    return TDGL_OK;
}

// The substructured factors the ensemble applies: a READY fp64 direct solve of one or two levels whose separator
// right-hand sides come from the -E^T rows (no sparse coupling blocks).  Anything else is refused with TDGL_ERR_ARG.
static int ens_sub_check(tdgl_ctx *ctx, const DirectFactors &f) {
    const char *who = "tdgl_ensemble_create";
    if (f.stage != DirectFactors::READY || f.fp32)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: the substructured factors precondition the CG (fp32 / preconditioner form): the ensemble "
                  "needs the fp64 direct solve", who);
    if (f.levels > 2)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: substructured factors of %d levels are not supported (one or two)", who, f.levels);
    for (int k = 0; k < f.levels; ++k)
        if (f.lv[k].coupling.nnz > 0 || f.lv[k].need_coupling || f.lv[k].ident || f.lv[k].vals.n == 0)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: substructured factors with sparse coupling blocks are not supported", who);
    if (f.dense.n != f.lv[f.levels - 1].nS || f.dense.tiles <= 0 || f.dense.G.n == 0 || f.nfin != (int)((f.dense.n + WAVE - 1) / WAVE))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "%s: the substructured factors have no fp64 top separator", who);
    return TDGL_OK;
}

static int ens_check(tdgl_ensemble *e, int32_t r) {
    if (!e) return TDGL_ERR_ARG;
    if (r < 0 || r >= e->R) TDGL_FAIL(e->ctx, TDGL_ERR_ARG, "ensemble: replica %d out of range [0, %d)", r, e->R);
    HIP_TRY(e->ctx, hipSetDevice(e->ctx->device));
    return TDGL_OK;
}

template <class T>
static int ens_copy(tdgl_ctx *ctx, T *dst, const T *src, int64_t count) {
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, (size_t)count * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_create(tdgl_ensemble **out, tdgl_ctx *ctx, int32_t n_replicas) {
    if (!out) return TDGL_ERR_ARG;
    *out = nullptr;
    CTX_GUARD(ctx);
    if (distributed(ctx)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_ensemble_create: single-GPU contexts only");
    if (n_replicas < 1 || n_replicas > TDGL_ENSEMBLE_MAX_REPLICAS)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_ensemble_create: n_replicas must be in [1, %d] (got %d)", TDGL_ENSEMBLE_MAX_REPLICAS, n_replicas);
    const DirectFactors *fac = ctx->direct.get();
    const bool dense = fac && fac->ld > 0 && fac->dense.n == ctx->n;
    if (!dense && !(fac && fac->levels > 0 && fac->n_local == 0))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_ensemble_create: the context has no dense inverse (tdgl_poisson_build_dense_inverse) "
                  "and no substructured direct solve");
    if (!dense) TDGL_TRY(ens_sub_check(ctx, *fac));
    if (ctx->scr_enabled) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_ensemble_create: screening is not supported");
    std::unique_ptr<tdgl_ensemble> e(new tdgl_ensemble());
    e->ctx = ctx;
    e->R = n_replicas;
    e->n = ctx->n;
    e->n_pad = ctx->n_pad;
    e->m_pad = ctx->m_pad;
    e->n_slots = ctx->lap_pat.n_slots;
    e->nt = fac->dense.tiles;
    e->ldpart = (int64_t)e->nt * e->nt * DT;
    e->fac = fac;
    const size_t R = (size_t)n_replicas;
    e->factor_bytes = (int64_t)fac->dense.G.n * (int64_t)sizeof(double) * (int64_t)((R + ENS_RG - 1) / ENS_RG);
    if (!dense) {
        e->levels = fac->levels;
        int64_t len = ctx->n;  // (the length of the vector a level works on)
        for (int k = 0; k < e->levels; ++k) {
            const SubLevel &L = fac->lv[k];
            TDGL_TRY(ens_sub_lists(ctx, L, len, e->sub_down[k], e->n_down[k], e->sub_up[k], e->n_up[k]));
            e->ldw[k] = L.nI + L.nS + L.parts;
            HIP_TRY(ctx, e->sub_w[k].alloc(R * e->ldw[k]));
            HIP_TRY(ctx, e->sub_xs[k].alloc(R * L.nS));
            e->factor_bytes += (int64_t)L.vals.n * (int64_t)sizeof(double) * (int64_t)((R + ENS_SG - 1) / ENS_SG);
            len = L.nS;
        }
        HIP_TRY(ctx, e->upart.alloc(R * fac->nfin));
        HIP_TRY(ctx, e->mean.alloc(R));
    }
    HIP_TRY(ctx, e->U.alloc(R * e->m_pad));
    HIP_TRY(ctx, e->lapv.alloc(R * std::max<int64_t>(e->n_slots, 1)));
    HIP_TRY(ctx, e->psi0.alloc(R * e->n_pad));
    HIP_TRY(ctx, e->psi1.alloc(R * e->n_pad));
    HIP_TRY(ctx, e->lap0.alloc(R * e->n_pad));
    HIP_TRY(ctx, e->lap1.alloc(R * e->n_pad));
    HIP_TRY(ctx, e->ceff.alloc(R * e->n_pad));
    HIP_TRY(ctx, e->eps.alloc(R * e->n_pad));
    HIP_TRY(ctx, e->mu.alloc(R * e->n_pad));
    HIP_TRY(ctx, e->bvec.alloc(R * e->n_pad));
    HIP_TRY(ctx, e->part.alloc(R * e->ldpart));
    HIP_TRY(ctx, e->dmax_part.alloc(R * ctx->psi_blocks));
    HIP_TRY(ctx, e->fail_part.alloc(R * ctx->psi_blocks));
    HIP_TRY(ctx, e->limit.alloc(R));
    HIP_TRY(ctx, e->d_ctl.alloc(R));
    HIP_TRY(ctx, e->d_rec.alloc(R * RA_BATCH_MAX));
    HIP_TRY(ctx, e->cvec.alloc(R * e->n_pad));
    HIP_TRY(ctx, e->ramping.alloc(R));
    HIP_TRY(ctx, e->moved.alloc(R));
    e->h_ramping.assign(R, 0);
    e->h_ctl.resize(R);
    e->h_rec.resize(R * RA_BATCH_MAX);
    e->h_limit.resize(R);
    e->rep.resize(R);
    *out = e.release();
    return TDGL_OK;
}

extern "C" void tdgl_ensemble_destroy(tdgl_ensemble *e) {
    if (!e) return;
    (void)hipSetDevice(e->ctx->device);
    (void)hipStreamSynchronize(e->ctx->stream);
    delete e;
}

extern "C" int tdgl_ensemble_size(tdgl_ensemble *e, int32_t *n_replicas) {
    if (!e || !n_replicas) return TDGL_ERR_ARG;
    *n_replicas = e->R;
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_set_link_exponents(tdgl_ensemble *e, int32_t r, const double *A) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    TDGL_TRY(tdgl_set_link_exponents(ctx, A));  // (link variables and covariant-Laplacian values, in the context's buffers)
    TDGL_TRY(ens_copy(ctx, e->U.p + r * e->m_pad, ctx->e_U.p, e->m_pad));
    TDGL_TRY(ens_copy(ctx, e->lapv.p + r * e->n_slots, ctx->lap_vals.p, e->n_slots));
    EnsReplica &p = e->rep[r];
    p.have_links = true;
    p.lap_valid = false;
    FieldArrays none;
    p.field.take(none);
    p.loop.field.clear();
    p.loop.field.has_dadt = false;
    e->tables_dirty = true;
    return TDGL_OK;
}

// Replica r is about to be given a moving field: it is without links until ens_take_field has completed it.  The arrays every
// replica with moving links has a share of are allocated when the first replica asks
static int ens_begin_field(tdgl_ensemble *e, int32_t r) {
    e->rep[r].have_links = false;
    e->tables_dirty = true;
    if (e->A.n != 0) return TDGL_OK;
    tdgl_ctx *ctx = e->ctx;
    const size_t R = (size_t)e->R;
    DevBuf<double> a, prev, dadt;
    HIP_TRY(ctx, a.alloc(R * 2 * e->m_pad));
    HIP_TRY(ctx, prev.alloc(R * 2 * e->m_pad));
    HIP_TRY(ctx, dadt.alloc(R * e->m_pad));
    e->A.take(a);
    e->Aprev.take(prev);
    e->dadt.take(dadt);
    return TDGL_OK;
}

// A replica whose links move inside tdgl_ensemble_run takes over the field the context has just been given by one of its own
// setters (A = A_prev = A(0), the links and the Laplacian values in the context's buffers): the drive, its arrays -- moved,
// not copied: the context's own links do not stay a moving field, they are the ensemble's scratch --, and copies of A,
// A_prev, the links and the Laplacian values; dA/dt = 0.
static int ens_take_field(tdgl_ensemble *e, int32_t r) {
    tdgl_ctx *ctx = e->ctx;
    EnsReplica &p = e->rep[r];
    p.field.take(ctx->field);
    p.loop.field = ctx->loop.field;
    ctx->loop.field.clear();
    const int64_t o2 = 2 * (int64_t)r * e->m_pad;
    TDGL_TRY(ens_copy(ctx, e->A.p + o2, ctx->e_A.p, 2 * e->m_pad));
    TDGL_TRY(ens_copy(ctx, e->Aprev.p + o2, ctx->e_Aprev.p, 2 * e->m_pad));
    HIP_TRY(ctx, hipMemset(e->dadt.p + r * e->m_pad, 0, e->m_pad * sizeof(double)));
    TDGL_TRY(ens_copy(ctx, e->U.p + r * e->m_pad, ctx->e_U.p, e->m_pad));
    TDGL_TRY(ens_copy(ctx, e->lapv.p + r * e->n_slots, ctx->lap_vals.p, e->n_slots));
    p.loop.field.has_dadt = false;
    p.lap_valid = false;
    p.have_links = true;
    return TDGL_OK;
}

// A(t) = LinearRamp(t) A_base for replica r (tdgl_set_link_exponents_base + tdgl_set_link_ramp of the context): the
// links start at the ramp's value at t = 0 and move inside tdgl_ensemble_run
extern "C" int tdgl_ensemble_set_link_ramp(tdgl_ensemble *e, int32_t r, const double *A_base, double tmin, double tmax, double initial,
                                           double final_) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    if (!A_base) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_ensemble_set_link_ramp: null A_base");
    if (!(std::isfinite(tmin) && std::isfinite(tmax) && std::isfinite(initial) && std::isfinite(final_)))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_ensemble_set_link_ramp: the ramp's parameters must be finite");
    if (!(tmax > tmin)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_link_ramp: tmax must be > tmin");
    TDGL_TRY(ens_begin_field(e, r));
    TDGL_TRY(tdgl_set_link_exponents_base(ctx, A_base, linear_ramp_value(0.0, tmin, tmax, initial, final_)));
    TDGL_TRY(ens_take_field(e, r));
    const double q[4] = {tmin, tmax, initial, final_};
    e->rep[r].loop.field.set_product_source(TERM_RAMP, q, nullptr, nullptr, 0);
    return TDGL_OK;
}

// A(t) = table(t) A_base for replica r (tdgl_set_link_exponents_base + tdgl_set_link_table of the context), with the
// failure rules of tdgl_ensemble_set_link_ramp: the links start at the table's value at t = 0
extern "C" int tdgl_ensemble_set_link_table(tdgl_ensemble *e, int32_t r, const double *A_base, int32_t n_nodes, const double *times,
                                            const double *values) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    if (!A_base) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_ensemble_set_link_table: null A_base");
    TDGL_TRY(check_link_table(ctx, "tdgl_ensemble_set_link_table", n_nodes, times, values));
    TDGL_TRY(ens_begin_field(e, r));
    TDGL_TRY(tdgl_set_link_exponents_base(ctx, A_base, table_value(times, values, n_nodes, 0.0)));
    TDGL_TRY(ens_take_field(e, r));
    e->rep[r].loop.field.set_product_source(TERM_TABLE, nullptr, times, values, n_nodes);
    return TDGL_OK;
}

// A(t) = A_0 + f_1(t) A_1 + ... + f_K(t) A_K for replica r (tdgl_set_link_terms of the context, whose arguments and rules
// these are), with the failure rules of tdgl_ensemble_set_link_table: a refused argument leaves the replica as it was, a
// failure behind that leaves it without links.
extern "C" int tdgl_ensemble_set_link_terms(tdgl_ensemble *e, int32_t r, const double *A0, int32_t n_terms, const double *bases,
                                            const int32_t *kind, const double *ramp, const int32_t *tab_off, const double *tab_times,
                                            const double *tab_values) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    TDGL_TRY(check_link_terms(ctx, "tdgl_ensemble_set_link_terms", n_terms, bases, kind, ramp, tab_off, tab_times, tab_values));
    TDGL_TRY(ens_begin_field(e, r));
    TDGL_TRY(tdgl_set_link_terms(ctx, A0, n_terms, bases, kind, ramp, tab_off, tab_times, tab_values));
    return ens_take_field(e, r);
}

extern "C" int tdgl_ensemble_get_link_term_scales(tdgl_ensemble *e, int32_t r, int32_t *n_terms, double *scales) {
    TDGL_TRY(ens_check(e, r));
    if (!n_terms || !scales) TDGL_FAIL(e->ctx, TDGL_ERR_ARG, "tdgl_ensemble_get_link_term_scales: null output");
    const LoopState &L = e->rep[r].loop;
    *n_terms = L.field.sum() ? L.field.n_terms : 0;
    for (int k = 0; k < *n_terms; ++k) scales[k] = L.field.scale[k];
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_get_link_scale(tdgl_ensemble *e, int32_t r, double *scale) {
    TDGL_TRY(ens_check(e, r));
    if (!scale) TDGL_FAIL(e->ctx, TDGL_ERR_ARG, "tdgl_ensemble_get_link_scale: null scale");
    const FieldDrive &F = e->rep[r].loop.field;
    *scale = F.sum() ? 1.0 : F.scale[0];
    return TDGL_OK;
}

// replica r's terminal currents as tables (tdgl_set_mu_boundary_table's arguments and rules); n_nodes = 0: off
extern "C" int tdgl_ensemble_set_mu_boundary_table(tdgl_ensemble *e, int32_t r, int32_t n_nodes, const double *times, int32_t n_groups,
                                                   const int32_t *group_ptr, const int32_t *group_pos, const double *density) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    EnsReplica &p = e->rep[r];
    if (n_nodes != 0) {
        TDGL_TRY(check_mu_table(ctx, "tdgl_ensemble_set_mu_boundary_table", n_nodes, times, n_groups, group_ptr, group_pos, density));
        TDGL_TRY(ensure_boundary_sites(ctx));
        if (e->mu_b.n == 0) HIP_TRY(ctx, e->mu_b.alloc((size_t)e->R * std::max<int64_t>(ctx->nb, 1)));
        // solver.py:289, 323: mu_boundary and the densities start at 0; the table rewrites its positions
        HIP_TRY(ctx, hipMemset(e->mu_b.p + (int64_t)r * ctx->nb, 0, ctx->nb * sizeof(double)));
    }
    if (n_nodes != 0) p.mu_tab.set(n_nodes, times, n_groups, group_ptr, group_pos, density, ctx->nb);
    else p.mu_tab.clear();
    e->tables_dirty = true;
    return TDGL_OK;
}

// replica r's epsilon(r, t) = factor(t) epsilon0(r) (tdgl_set_epsilon_table's arguments and rules); n_nodes = 0: off
extern "C" int tdgl_ensemble_set_epsilon_table(tdgl_ensemble *e, int32_t r, const double *epsilon0, int32_t n_nodes, const double *times,
                                               const double *factor) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    EnsReplica &p = e->rep[r];
    if (n_nodes != 0) {
        TDGL_TRY(check_eps_table(ctx, "tdgl_ensemble_set_epsilon_table", epsilon0, n_nodes, times, factor));
        if (e->eps0.n == 0) HIP_TRY(ctx, e->eps0.alloc((size_t)e->R * e->n_pad));
        DevBuf<double> tmp;
        HIP_TRY(ctx, tmp.alloc(e->n_pad));
        TDGL_TRY(upload_sites(ctx, epsilon0, tmp));
        TDGL_TRY(ens_copy(ctx, e->eps0.p + r * e->n_pad, tmp.p, e->n_pad));
    }
    if (n_nodes != 0) p.eps_tab.set(n_nodes, times, factor), p.eps_spots.clear();
    else p.eps_tab.clear();
    e->tables_dirty = true;
    return TDGL_OK;
}

// replica r's epsilon(r, t) = epsilon0(r) - its hot spots (tdgl_set_epsilon_spots' arguments and rules); n_spots = 0: off.
// The site coordinates are the ensemble's: stored at the first call
extern "C" int tdgl_ensemble_set_epsilon_spots(tdgl_ensemble *e, int32_t r, const double *sites, const double *eps0, int32_t n_spots,
                                               const int32_t *tab_off, const double *tab_times, const double *tab_cx, const double *tab_cy,
                                               const double *tab_amp, const double *tab_sigma) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    EnsReplica &p = e->rep[r];
    if (n_spots == 0) {
        p.eps_spots.clear();
        e->tables_dirty = true;
        return TDGL_OK;
    }
    TDGL_TRY(check_eps_spots(ctx, "tdgl_ensemble_set_epsilon_spots", sites, eps0, n_spots, tab_off, tab_times, tab_cx, tab_cy, tab_amp, tab_sigma));
    if (e->eps0.n == 0) HIP_TRY(ctx, e->eps0.alloc((size_t)e->R * e->n_pad));
    if (e->spot_xy.n == 0) {
        DevBuf<double2> xy;
        HIP_TRY(ctx, xy.alloc(e->n_pad));
        TDGL_TRY(upload_sites(ctx, reinterpret_cast<const double2 *>(sites), xy));
        e->spot_xy.take(xy);
    }
    DevBuf<double> tmp;
    HIP_TRY(ctx, tmp.alloc(e->n_pad));
    TDGL_TRY(upload_sites(ctx, eps0, tmp));
    TDGL_TRY(ens_copy(ctx, e->eps0.p + r * e->n_pad, tmp.p, e->n_pad));
    p.eps_tab.clear();
    EpsSpots &S = p.eps_spots;
    S.clear();
    S.set(n_spots, tab_off, tab_times, tab_cx, tab_cy, tab_amp, tab_sigma);
    // epsilon = epsilon(r, 0), by the single run's kernel at the host's values
    launch_eps_spots(ctx, S, S.values_at(0.0), e->spot_xy.p, e->eps0.p + r * e->n_pad, e->eps.p + r * e->n_pad, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    p.have_eps = true;
    e->tables_dirty = true;
    return TDGL_OK;
}

// replica r's epsilon in force, in the caller's site order, whatever set it
extern "C" int tdgl_ensemble_get_epsilon(tdgl_ensemble *e, int32_t r, double *epsilon) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    if (!epsilon) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_ensemble_get_epsilon: null epsilon");
    if (!e->rep[r].have_eps) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_ensemble_get_epsilon: replica %d has no epsilon", r);
    return download_sites(ctx, (const double *)(e->eps.p + r * e->n_pad), epsilon);
}

// the replicas' tables as pools on the device
static int ens_upload_tables(tdgl_ensemble *e) {
    tdgl_ctx *ctx = e->ctx;
    const int R = e->R;
    const int64_t nb = std::max<int64_t>(ctx->nb, 1);
    std::vector<int32_t> toff(R + 1, 0), eoff(R + 1, 0), group((size_t)R * nb, -1);
    std::vector<int64_t> doff(R, 0);
    std::vector<double> mt, md, et, ef;
    e->any_mu_table = e->any_eps_table = e->any_eps_spots = false;
    std::vector<EpsSpotTabs> stabs((size_t)R, EpsSpotTabs{});
    std::vector<double> spool;
    for (int r = 0; r < R; ++r) {
        const EnsReplica &p = e->rep[r];
        doff[r] = (int64_t)md.size();
        const MuTable &M = p.mu_tab;
        const EpsTable &E = p.eps_tab;
        const std::vector<int32_t> g = M.on() ? M.groups(ctx->nb) : std::vector<int32_t>();
        mt.insert(mt.end(), M.t.begin(), M.t.end());
        md.insert(md.end(), M.dens.begin(), M.dens.end());
        std::copy(g.begin(), g.end(), group.begin() + (size_t)r * nb);
        toff[r + 1] = (int32_t)mt.size();
        et.insert(et.end(), E.t.begin(), E.t.end());
        ef.insert(ef.end(), E.f.begin(), E.f.end());
        eoff[r + 1] = (int32_t)et.size();
        e->any_mu_table |= M.on();
        e->any_eps_table |= E.on();
        if (p.eps_spots.on()) {
            stabs[r] = p.eps_spots.tabs;
            stabs[r].base = (int64_t)spool.size();
            spool.insert(spool.end(), p.eps_spots.pool.begin(), p.eps_spots.pool.end());
            e->any_eps_spots = true;
        }
    }
    if (e->any_eps_spots) {  // (an ensemble without spots allocates nothing for them)
        HIP_TRY(ctx, e->spot_tabs.upload(stabs));
        HIP_TRY(ctx, e->spot_pool.upload(spool));
    }
    std::vector<FieldTerm> desc((size_t)R * FIELD_TERMS_MAX, FieldTerm{});
    std::vector<const double *> bases((size_t)R, nullptr), a0s((size_t)R, nullptr);
    std::vector<double> kt, kv;
    for (int r = 0; r < R; ++r) {
        const EnsReplica &p = e->rep[r];
        if (!p.loop.field.moves) continue;
        bases[r] = p.field.bases.p, a0s[r] = p.field.a0.p;
        p.loop.field.describe(desc.data() + (size_t)r * FIELD_TERMS_MAX, kt, kv);  // (its nodes in the ensemble's pools)
    }
    if (kt.empty()) kt.push_back(0.0), kv.push_back(0.0);
    HIP_TRY(ctx, e->term_desc.upload(desc));
    HIP_TRY(ctx, e->term_bases.upload(bases));
    HIP_TRY(ctx, e->term_a0.upload(a0s));
    HIP_TRY(ctx, e->tab_term_t.upload(kt));
    HIP_TRY(ctx, e->tab_term_v.upload(kv));
    if (mt.empty()) mt.push_back(0.0), md.push_back(0.0);  // (never read: every replica's node count is 0)
    if (et.empty()) et.push_back(0.0), ef.push_back(0.0);
    HIP_TRY(ctx, e->mu_toff.upload(toff));
    HIP_TRY(ctx, e->mu_doff.upload(doff));
    HIP_TRY(ctx, e->mu_group.upload(group));
    HIP_TRY(ctx, e->mu_t.upload(mt));
    HIP_TRY(ctx, e->mu_dens.upload(md));
    HIP_TRY(ctx, e->eps_off.upload(eoff));
    HIP_TRY(ctx, e->eps_t.upload(et));
    HIP_TRY(ctx, e->eps_f.upload(ef));
    e->tables_dirty = false;
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_set_mu_boundary(tdgl_ensemble *e, int32_t r, const double *mu_boundary) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    if (ctx->loop.field.has_dadt) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_ensemble_set_mu_boundary: the context's links are time dependent");
    TDGL_TRY(tdgl_set_mu_boundary(ctx, mu_boundary));  // (static links: the boundary term as the run-ahead loop reads it)
    TDGL_TRY(ens_copy(ctx, e->ceff.p + r * e->n_pad, ctx->ceff.p, e->n_pad));
    TDGL_TRY(ens_copy(ctx, e->cvec.p + r * e->n_pad, ctx->cvec.p, e->n_pad));  // (a ramp adds its dA/dt term to this)
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_set_epsilon(tdgl_ensemble *e, int32_t r, const double *epsilon) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    TDGL_TRY(tdgl_set_epsilon(ctx, epsilon));
    TDGL_TRY(ens_copy(ctx, e->eps.p + r * e->n_pad, ctx->eps.p, e->n_pad));
    EnsReplica &p = e->rep[r];
    if (p.eps_tab.on() || p.eps_spots.on()) {  // (plain values, a table and spots exclude each other: the later call wins)
        p.eps_tab.clear(), p.eps_spots.clear();
        e->tables_dirty = true;
    }
    p.have_eps = true;
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_set_state(tdgl_ensemble *e, int32_t r, const double *psi, const double *mu) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    TDGL_TRY(tdgl_set_state(ctx, psi, mu));
    EnsReplica &p = e->rep[r];
    p.loop.new_state(0);
    TDGL_TRY(ens_copy(ctx, e->psi0.p + r * e->n_pad, ctx->psi[ctx->loop.cur].p, e->n_pad));
    TDGL_TRY(ens_copy(ctx, e->mu.p + r * e->n_pad, ctx->mu.p, e->n_pad));
    p.have_state = true;
    p.lap_valid = false;
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_set_controller(tdgl_ensemble *e, int32_t r, const tdgl_controller *c) {
    TDGL_TRY(ens_check(e, r));
    if (!c) TDGL_FAIL(e->ctx, TDGL_ERR_ARG, "tdgl_ensemble_set_controller: null controller");
    if (c->dt_init > c->dt_max) TDGL_FAIL(e->ctx, TDGL_ERR_ARG, "dt_init must be less than or equal to dt_max.");
    if (!(c->adaptive_time_step_multiplier > 0 && c->adaptive_time_step_multiplier < 1))
        TDGL_FAIL(e->ctx, TDGL_ERR_ARG, "adaptive_time_step_multiplier must be in (0, 1) (got %g).", c->adaptive_time_step_multiplier);
    if (c->adaptive && (c->adaptive_window < 1 || c->adaptive_window > RA_HIST_MAX))
        TDGL_FAIL(e->ctx, TDGL_ERR_ARG, "ensemble: adaptive_window must be in [1, %d] (got %d)", RA_HIST_MAX, c->adaptive_window);
    e->rep[r].loop.reset(*c);
    e->rep[r].have_ctl = true;
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_set_probes(tdgl_ensemble *e, const int32_t *sites, int32_t n_probe) {
    if (!e) return TDGL_ERR_ARG;
    tdgl_ctx *ctx = e->ctx;
    TDGL_TRY(tdgl_set_probes(ctx, sites, n_probe));  // (validation and the site permutation)
    std::vector<int32_t> internal(ctx->probes.begin(), ctx->probes.end());
    HIP_TRY(ctx, e->d_probes.alloc(std::max<size_t>(internal.size(), 1)));
    HIP_TRY(ctx, e->probe.alloc((size_t)e->R * RA_BATCH_MAX * 2 * std::max<int32_t>(n_probe, 1)));
    if (!internal.empty())
        HIP_TRY(ctx, hipMemcpy(e->d_probes.p, internal.data(), internal.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    e->np_ = n_probe;
    e->h_probe.assign((size_t)e->R * RA_BATCH_MAX * 2 * std::max<int32_t>(n_probe, 1), 0.0);
    return TDGL_OK;
}

// Takes over the context's census (tdgl_set_census, whose triangles and loops it keeps reading) for every replica; a
// context without one switches the ensemble's off.
extern "C" int tdgl_ensemble_set_census(tdgl_ensemble *e) {
    if (!e) return TDGL_ERR_ARG;
    tdgl_ctx *ctx = e->ctx;
    CTX_GUARD(ctx);
    e->census_on = false;
    e->census.release();
    e->h_census.clear();
    e->census_rows.assign((size_t)e->R, std::vector<int32_t>());
    if (!ctx->census.on()) return TDGL_OK;
    const size_t count = (size_t)e->R * RA_BATCH_MAX * ctx->census.ncol();
    HIP_TRY(ctx, e->census.alloc(count));
    e->h_census.assign(count, 0);
    e->census_serial = ctx->census.serial;
    e->census_on = true;
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_get_census(tdgl_ensemble *e, int32_t r, int64_t capacity_rows, int32_t *rows, int64_t *n_rows) {
    TDGL_TRY(ens_check(e, r));
    if (capacity_rows < 0 || (capacity_rows > 0 && !rows) || !n_rows) TDGL_FAIL(e->ctx, TDGL_ERR_ARG, "tdgl_ensemble_get_census: bad arguments");
    const int ncol = e->ctx->census.ncol();
    const bool on = e->census_on && e->ctx->census.on() && e->census_serial == e->ctx->census.serial;
    const int64_t have = on ? (int64_t)(e->census_rows[r].size() / ncol) : 0;
    *n_rows = have;
    const int64_t k = std::min(have, capacity_rows);
    if (k > 0) memcpy(rows, e->census_rows[r].data(), (size_t)k * ncol * sizeof(int32_t));
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_begin_stage(tdgl_ensemble *e, int32_t r) {
    TDGL_TRY(ens_check(e, r));
    e->rep[r].loop.begin_stage();
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_get_loop_state(tdgl_ensemble *e, int32_t r, int64_t *step, double *time, double *runner_dt,
                                            double *tentative_dt) {
    TDGL_TRY(ens_check(e, r));
    e->rep[r].loop.report(step, time, runner_dt, tentative_dt);
    return TDGL_OK;
}

// psi, mu of replica r and the currents formed from them: the replica's state goes through the context, whose
// tdgl_get_state forms J_s, J_n with the replica's link variables (the arithmetic of the single run)
extern "C" int tdgl_ensemble_get_state(tdgl_ensemble *e, int32_t r, double *psi, double *mu, double *supercurrent,
                                       double *normal_current) {
    TDGL_TRY(ens_check(e, r));
    tdgl_ctx *ctx = e->ctx;
    const EnsReplica &p = e->rep[r];
    if (!p.have_state || !p.have_links) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_ensemble_get_state: replica %d has no state or links", r);
    if (ctx->loop.field.has_dadt) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_ensemble_get_state: the context's links are time dependent");
    TDGL_TRY(ens_copy(ctx, ctx->psi[ctx->loop.cur].p, (p.loop.cur ? e->psi1.p : e->psi0.p) + r * e->n_pad, e->n_pad));
    TDGL_TRY(ens_copy(ctx, ctx->mu.p, e->mu.p + r * e->n_pad, e->n_pad));
    TDGL_TRY(ens_copy(ctx, ctx->e_U.p, e->U.p + r * e->m_pad, e->m_pad));
    // a ramping replica: J_n with its dA/dt -- that of the step that produced psi (the next step's ramp moves at the
    // start of its first attempt, in the next tdgl_ensemble_run)
    const bool dadt = p.loop.field.moves && p.loop.field.has_dadt;
    if (dadt) TDGL_TRY(ens_copy(ctx, ctx->e_dAdt.p, e->dadt.p + r * e->m_pad, e->m_pad));
    ctx->have_state = true;
    ctx->lap_valid = false;  // (the context's Laplacian values belong to whatever links it was last given)
    ctx->currents.new_state();
    ctx->loop.field.has_dadt = dadt;
    const int status = tdgl_get_state(ctx, psi, mu, supercurrent, normal_current);
    ctx->loop.field.has_dadt = false;  // (the context's own links are static)
    return status;
}

static void ens_launch_laplacian_cache(tdgl_ensemble *e, int r) {
    const bool c1 = e->rep[r].loop.cur != 0;
    launch_psi_laplacian(e->ctx, false, (c1 ? e->psi1.p : e->psi0.p) + r * e->n_pad, (c1 ? e->lap1.p : e->lap0.p) + r * e->n_pad, 0,
                         e->lapv.p + r * e->n_slots);
}

// the time-dependent inputs of the round's attempts (T1, T2, R1 - R5), in the single run's order (run.inc: run_ahead)
static void ens_queue_drives(tdgl_ensemble *e, bool ramping) {
    tdgl_ctx *ctx = e->ctx;
    const unsigned R = (unsigned)e->R;
    if (e->any_mu_table)
        hipLaunchKernelGGL(k_ens_mu_table, dim3(1, R), dim3(BLOCK), 0, ctx->stream, (int)ctx->nb, (int)ctx->n_b_sites,
                           (const int32_t *)ctx->d_b_sites.p, (const int32_t *)ctx->b_s0.p, (const int32_t *)ctx->b_s1.p,
                           (const double *)ctx->b_c0.p, (const double *)ctx->b_c1.p, e->mu_b.p, e->cvec.p, e->ceff.p, e->n_pad,
                           (const int32_t *)e->mu_toff.p, (const int64_t *)e->mu_doff.p, (const double *)e->mu_t.p,
                           (const double *)e->mu_dens.p, (const int32_t *)e->mu_group.p, (const StepCtl *)e->d_ctl.p);
    if (e->any_eps_table)
        hipLaunchKernelGGL(k_ens_eps_table, dim3(grid_for(e->n_pad), R), dim3(BLOCK), 0, ctx->stream, e->n_pad, (const double *)e->eps0.p,
                           e->eps.p, (const int32_t *)e->eps_off.p, (const double *)e->eps_t.p, (const double *)e->eps_f.p,
                           (const StepCtl *)e->d_ctl.p);
    if (e->any_eps_spots)
        hipLaunchKernelGGL(k_ens_eps_spots, dim3(grid_for(e->n_pad), R), dim3(BLOCK), 0, ctx->stream, e->n_pad, (const double2 *)e->spot_xy.p,
                           (const double *)e->eps0.p, e->eps.p, (const EpsSpotTabs *)e->spot_tabs.p, (const double *)e->spot_pool.p,
                           (const StepCtl *)e->d_ctl.p);
    if (!ramping) return;
    const SellPattern &pat = ctx->lap_pat;
    hipLaunchKernelGGL(k_ens_field_begin, dim3((R + 63) / 64), dim3(64), 0, ctx->stream, (int)R, e->d_ctl.p, (const int32_t *)e->ramping.p,
                       (const FieldTerm *)e->term_desc.p, (const double *)e->tab_term_t.p, (const double *)e->tab_term_v.p, e->moved.p);
    const int nblk = grid_for(ctx->m);
    hipLaunchKernelGGL(k_ens_field_links, dim3(nblk, R), dim3(BLOCK), 0, ctx->stream, ctx->m, e->m_pad, (const double *const *)e->term_bases.p,
                       (const double *const *)e->term_a0.p, e->A.p, e->Aprev.p, (const double *)ctx->e_dirx.p, (const double *)ctx->e_diry.p,
                       (const double *)ctx->e_inv_len.p, e->dadt.p, e->moved.p, (const StepCtl *)e->d_ctl.p);
    const int nblk_ceff = grid_for((int64_t)pat.n_slices * WAVE);
    hipLaunchKernelGGL(k_ens_ceff_links, dim3(nblk_ceff + nblk, R), dim3(BLOCK), 0, ctx->stream, nblk_ceff, pat.n_slices, pat.n_rows,
                       (const int32_t *)pat.slice_off.p, (const int32_t *)ctx->lap_slot_edge.p, (const double *)ctx->lap_slot_w.p,
                       (const double *)ctx->e_inv_len.p, (const double *)e->dadt.p, (const double *)e->cvec.p, e->ceff.p, e->n_pad, ctx->m,
                       e->m_pad, (const double *)e->A.p, (const double *)ctx->e_dirx.p, (const double *)ctx->e_diry.p, e->U.p,
                       (const int32_t *)e->moved.p, (const StepCtl *)e->d_ctl.p);
    hipLaunchKernelGGL(k_ens_fill_laplacian, dim3(grid_for(pat.n_slots), R), dim3(BLOCK), 0, ctx->stream, pat.n_slots,
                       (const int32_t *)ctx->lap_slot_edge.p, (const double *)ctx->lap_slot_w.p, (const double2 *)e->U.p, e->m_pad,
                       e->lapv.p, (const int32_t *)e->moved.p);
    const int tiles = (pat.n_slices + BLOCK / WAVE - 1) / (BLOCK / WAVE);
    const int per_xcd = (tiles + XCDS - 1) / XCDS, grid = per_xcd * XCDS;
#define TDGL_KENS(IT, COLS)                                                                                                      \
    hipLaunchKernelGGL((k_ens_laplacian_fresh<IT>), dim3(grid, R), dim3(BLOCK), 0, ctx->stream, pat.n_slices, per_xcd, pat.n_rows, \
                       pat.slice_off.p, COLS, (const double2 *)e->lapv.p, e->n_slots, ctx->lap_diag.p, ctx->fixed_mask.p,        \
                       (const double2 *)e->psi0.p, (const double2 *)e->psi1.p, e->lap0.p, e->lap1.p, e->n_pad,                  \
                       (const StepCtl *)e->d_ctl.p)
    if (pat.use16) TDGL_KENS(int16_t, pat.cols16.p); else TDGL_KENS(int32_t, pat.cols.p);
#undef TDGL_KENS
}

// mu = pinv(A) bvec of every live replica on the substructured factors, then the controllers (S1 - S6, ensemble_sub.inc):
// the ways down level after level, the top separator, the means, the ways up innermost first
static void ens_queue_sub_solve(tdgl_ensemble *e) {
    tdgl_ctx *ctx = e->ctx;
    const DirectFactors &f = *e->fac;
    const int R = e->R, K = e->levels, nt = e->nt;
    const unsigned groups = (unsigned)((R + ENS_SG - 1) / ENS_SG);
    const StepCtl *ctl = e->d_ctl.p;
    const double *vec = e->bvec.p;
    int64_t ldv = e->n_pad;
    for (int k = 0; k < K; ++k) {
        const SubLevel &L = f.lv[k];
        const int64_t rows = L.nI + L.nS + L.parts;
        const int nblk_rest = (int)((rows - L.nI + BLOCK / WAVE - 1) / (BLOCK / WAVE));
        hipLaunchKernelGGL(k_ens_sub_down, dim3((unsigned)(e->n_down[k] + nblk_rest), groups), dim3(BLOCK), 0, ctx->stream, e->n_down[k],
                           (const EnsSubChunk *)e->sub_down[k].p, L.nI, rows, (const int32_t *)L.seg_ptr.p, (const int64_t *)L.seg_val.p,
                           (const int32_t *)L.seg_x.p, (const int32_t *)L.seg_len.p, (const double *)L.vals.p, vec, ldv, e->sub_w[k].p,
                           e->ldw[k], R, ctl);
        vec = e->sub_w[k].p + L.nI;  // (the separator rows of the way down: the next level's vector)
        ldv = e->ldw[k];
    }
    const SubLevel &L0 = f.lv[0], &T = f.lv[K - 1];
    hipLaunchKernelGGL(k_ens_dense_tiles, dim3(nt * (nt + 1) / 2, (R + ENS_RG - 1) / ENS_RG), dim3(BLOCK), 0, ctx->stream, (int)T.nS, nt,
                       (const double *)f.dense.G.p, vec, ldv, e->part.p, e->ldpart, R, ctl);
    hipLaunchKernelGGL(k_ens_sub_top, dim3(f.nfin, R), dim3(BLOCK), 0, ctx->stream, (int)T.nS, nt, (const double *)e->part.p, e->ldpart,
                       e->sub_xs[K - 1].p, (const double *)T.u.p, e->upart.p, f.nfin, ctl);
    const SubLevel &L1 = f.lv[1];
    hipLaunchKernelGGL(k_ens_sub_mean, dim3(R), dim3(BLOCK), 0, ctx->stream, (const double *)(e->sub_w[0].p + L0.nI + L0.nS), L0.parts,
                       e->ldw[0], K > 1 ? (const double *)(e->sub_w[1].p + L1.nI + L1.nS) : (const double *)nullptr, K > 1 ? L1.parts : 0,
                       e->ldw[1], (const double *)e->upart.p, f.nfin, 1.0 / (double)ctx->n_global, e->mean.p, ctl);
    for (int k = K - 1; k >= 0; --k) {
        const SubLevel &L = f.lv[k];
        double *out = k == 0 ? e->mu.p : e->sub_xs[k - 1].p;
        const int64_t ldo = k == 0 ? e->n_pad : f.lv[k - 1].nS;
        hipLaunchKernelGGL(k_ens_sub_up, dim3((unsigned)(e->n_up[k] + grid_for(L.nS)), groups), dim3(BLOCK), 0, ctx->stream, e->n_up[k],
                           (const EnsSubChunk *)e->sub_up[k].p, L.nI, L.nS, (const int32_t *)L.sep_idx.p, (const double *)L.vals.p,
                           (const double *)e->sub_w[k].p, e->ldw[k], (const double *)e->sub_xs[k].p, L.nS,
                           k == 0 ? (const double *)e->mean.p : (const double *)nullptr,
                           k == 0 ? (const int32_t *)e->fail_part.p : (const int32_t *)nullptr, ctx->psi_blocks, out, ldo, R, ctl);
    }
    hipLaunchKernelGGL(k_ens_sub_control, dim3(R), dim3(BLOCK), 0, ctx->stream, (const double *)e->dmax_part.p,
                       (const int32_t *)e->fail_part.p, ctx->psi_blocks, e->d_ctl.p, e->d_rec.p, (const int32_t *)e->limit.p);
}

static void ens_queue_round(tdgl_ensemble *e, bool ramping) {
    tdgl_ctx *ctx = e->ctx;
    const unsigned R = (unsigned)e->R;
    ens_queue_drives(e, ramping);
    hipLaunchKernelGGL(k_ens_psi_update, dim3(ctx->psi_blocks, R), dim3(BLOCK), 0, ctx->stream, ctx->n_own, e->n_pad, e->psi0.p, e->psi1.p,
                       (const double2 *)e->lap0.p, (const double2 *)e->lap1.p, (const double *)e->mu.p, (const double *)e->eps.p, ctx->u,
                       ctx->gamma, e->dmax_part.p, e->fail_part.p, e->d_ctl.p);
    const SellPattern &pat = ctx->lap_pat;
    const int tiles = (pat.n_slices + BLOCK / WAVE - 1) / (BLOCK / WAVE);
    const int per_xcd = (tiles + XCDS - 1) / XCDS, grid = per_xcd * XCDS;
#define TDGL_KENS(IT, COLS)                                                                                                       \
    hipLaunchKernelGGL((k_ens_laplacian<IT>), dim3(grid, R), dim3(BLOCK), 0, ctx->stream, pat.n_slices, per_xcd, pat.n_rows,       \
                       pat.slice_off.p, COLS, (const double2 *)e->lapv.p, e->n_slots, ctx->lap_diag.p, ctx->fixed_mask.p,         \
                       (const double2 *)e->psi0.p, (const double2 *)e->psi1.p, e->lap0.p, e->lap1.p, ctx->area.p,                 \
                       (const double *)e->ceff.p, e->bvec.p, e->n_pad, (const StepCtl *)e->d_ctl.p)
    if (pat.use16) TDGL_KENS(int16_t, pat.cols16.p); else TDGL_KENS(int32_t, pat.cols.p);
#undef TDGL_KENS
    const int nt = e->nt;
    if (e->levels > 0) {
        ens_queue_sub_solve(e);
    } else {
        hipLaunchKernelGGL(k_ens_dense_tiles, dim3(nt * (nt + 1) / 2, (R + ENS_RG - 1) / ENS_RG), dim3(BLOCK), 0, ctx->stream, (int)e->n, nt,
                           (const double *)ctx->direct->dense.G.p, (const double *)e->bvec.p, e->n_pad, e->part.p, e->ldpart, (int)R,
                           (const StepCtl *)e->d_ctl.p);
        hipLaunchKernelGGL(k_ens_finish, dim3((unsigned)((e->n + WAVE - 1) / WAVE), R), dim3(BLOCK), 0, ctx->stream, (int)e->n, nt,
                           (const double *)e->part.p, e->ldpart, (const double *)e->dmax_part.p, (const int32_t *)e->fail_part.p,
                           ctx->psi_blocks, e->mu.p, e->n_pad, e->d_ctl.p, e->d_rec.p, (const int32_t *)e->limit.p);
    }
    if (e->np_ > 0)
        hipLaunchKernelGGL(k_ens_probes, dim3((e->np_ + 63) / 64, R), dim3(64), 0, ctx->stream, e->np_, (const int32_t *)e->d_probes.p,
                           (const double2 *)e->psi0.p, (const double2 *)e->psi1.p, (const double *)e->mu.p, e->n_pad, e->probe.p,
                           (const StepCtl *)e->d_ctl.p);
    if (e->census_on)
        hipLaunchKernelGGL(k_ens_census, dim3(ctx->census.grid(), R), dim3(BLOCK), 0, ctx->stream, ctx->census.plan(),
                           (const double2 *)e->psi0.p, (const double2 *)e->psi1.p, e->n_pad, e->census.p, (const StepCtl *)e->d_ctl.p);
}

// Up to max_steps[r] accepted steps of every replica (the loop of tdgl_run per replica: runner.py:379-433), stopping
// a replica at end_time[r].  Outputs per replica r: out_dt[r * capacity + k], out_mu_probe / out_theta_probe
// [r * capacity + k][n_probe], steps_done[r], reached_end[r].  A replica that spends its retry budget stops the call
// after the batch it happened in: TDGL_ERR_PSI_RETRIES with the reference's message prefixed by the replica index
// (the first such replica); the steps before it are delivered.
extern "C" int tdgl_ensemble_run(tdgl_ensemble *e, const int64_t *max_steps, const double *end_time, int64_t capacity,
                                 double *out_dt, double *out_mu_probe, double *out_theta_probe, int64_t *steps_done,
                                 int32_t *reached_end, int32_t *failed) {
    if (!e) return TDGL_ERR_ARG;
    tdgl_ctx *ctx = e->ctx;
    CTX_GUARD(ctx);
    if (!max_steps || !end_time || capacity < 0 || !out_dt || !steps_done || !reached_end)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_ensemble_run: bad arguments");
    if (e->levels == 0 && !(ctx->direct && ctx->direct->ld > 0 && ctx->direct->dense.tiles == e->nt))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_ensemble_run: the context's dense inverse has been released");
    if (e->levels > 0 && !(ctx->direct.get() == e->fac && e->fac->levels == e->levels && e->fac->stage == DirectFactors::READY &&
                           e->fac->dense.tiles == e->nt))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_ensemble_run: the context's substructured factors have been released or replaced");
    const int R = e->R, np_ = e->np_;
    // (a census set on the context after tdgl_ensemble_set_census, or taken off it: the ensemble's rows no longer fit)
    if (e->census_on && (!ctx->census.on() || e->census_serial != ctx->census.serial))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_ensemble_run: the context's census changed; call tdgl_ensemble_set_census again");
    const int ncen = e->census_on ? ctx->census.ncol() : 0;
    for (auto &rows : e->census_rows) rows.clear();
    for (int r = 0; r < R; ++r) {
        const EnsReplica &p = e->rep[r];
        if (max_steps[r] < 0 || max_steps[r] > capacity) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_ensemble_run: max_steps[%d] outside [0, capacity]", r);
        if (max_steps[r] > 0 && (!p.have_links || !p.have_eps || !p.have_state || !p.have_ctl))
            TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_ensemble_run: replica %d needs link exponents, epsilon, state and controller", r);
        steps_done[r] = 0;
        reached_end[r] = 0;
        if (failed) failed[r] = 0;
    }
    if (e->tables_dirty) TDGL_TRY(ens_upload_tables(e));
    for (int r = 0; r < R; ++r)
        if (!e->rep[r].lap_valid && max_steps[r] > 0) {
            ens_launch_laplacian_cache(e, r);
            e->rep[r].lap_valid = true;
        }
    HIP_TRY(ctx, hipGetLastError());
    int err_replica = -1;
    double err_dt = 0.0;
    for (;;) {
        int active = 0, n_ramping = 0;
        for (int r = 0; r < R; ++r) {
            EnsReplica &p = e->rep[r];
            const bool on = !reached_end[r] && steps_done[r] < max_steps[r];
            active += on;
            // a ramp that has reached its end: dA/dt is identically zero from here on, and a replica whose ramp has
            // settled costs what a static one does (as in tdgl_run)
            if (p.loop.ramp_settled()) p.loop.field.has_dadt = false;
            e->h_ramping[r] = on && p.loop.ramping();
            n_ramping += e->h_ramping[r];
            p.loop.fill(e->h_ctl[r], end_time[r], on);
            e->h_limit[r] = on ? (int32_t)std::min<int64_t>(max_steps[r] - steps_done[r], RA_BATCH_MAX) : 0;
        }
        if (active == 0 || err_replica >= 0) break;
        const int batch = std::min(e->batch, RA_BATCH_MAX);
        HIP_TRY(ctx, hipMemcpyAsync(e->d_ctl.p, e->h_ctl.data(), (size_t)R * sizeof(StepCtl), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(e->limit.p, e->h_limit.data(), (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        if (n_ramping > 0)
            HIP_TRY(ctx, hipMemcpyAsync(e->ramping.p, e->h_ramping.data(), (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        if (ncen > 0) HIP_TRY(ctx, hipMemsetAsync(e->census.p, 0, e->census.n * sizeof(int32_t), ctx->stream));
        for (int s = 0; s < batch; ++s) ens_queue_round(e, n_ramping > 0);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(e->h_ctl.data(), e->d_ctl.p, (size_t)R * sizeof(StepCtl), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(e->h_rec.data(), e->d_rec.p, (size_t)R * RA_BATCH_MAX * sizeof(StepRec), hipMemcpyDeviceToHost, ctx->stream));
        if (np_ > 0)
            HIP_TRY(ctx, hipMemcpyAsync(e->h_probe.data(), e->probe.p, e->h_probe.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (ncen > 0)
            HIP_TRY(ctx, hipMemcpyAsync(e->h_census.data(), e->census.p, e->h_census.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        e->stat_rounds += batch;
        e->stat_batches += 1;
        for (int r = 0; r < R; ++r) {
            if (reached_end[r] || steps_done[r] >= max_steps[r]) continue;  // (was poisoned for the whole batch)
            EnsReplica &p = e->rep[r];
            const StepCtl &h = e->h_ctl[r];
            const StepRec *rec = e->h_rec.data() + (size_t)r * RA_BATCH_MAX;
            const LoopState::Batch b = p.loop.absorb(h, rec, batch, e->h_limit[r], e->h_ramping[r] != 0,
                                                     out_dt + (size_t)r * capacity + steps_done[r]);
            if (b.corrupt)
                TDGL_FAIL(ctx, TDGL_ERR_HIP, "ensemble: corrupt attempt records of replica %d (%d processed, %d accepted of %d; check %d)", r,
                          h.n_done, h.n_acc, batch, b.corrupt);
            const int acc = b.accepted;
            if (np_ > 0)
                for (int k = 0; k < acc; ++k) {
                    const double *row = e->h_probe.data() + ((size_t)r * RA_BATCH_MAX + k) * 2 * np_;
                    const size_t at = ((size_t)r * capacity + steps_done[r] + k) * np_;
                    if (out_mu_probe) memcpy(out_mu_probe + at, row, np_ * sizeof(double));
                    if (out_theta_probe) memcpy(out_theta_probe + at, row + np_, np_ * sizeof(double));
                }
            if (ncen > 0) {
                const int32_t *rows = e->h_census.data() + (size_t)r * RA_BATCH_MAX * ncen;
                e->census_rows[r].insert(e->census_rows[r].end(), rows, rows + (size_t)acc * ncen);
            }
            steps_done[r] += acc;
            if (b.reached) reached_end[r] = 1;
            if (b.error) {
                if (failed) failed[r] = 1;
                if (err_replica < 0) {
                    err_replica = r;
                    err_dt = b.last_fail_dt;
                }
            }
        }
        e->batch = std::min(2 * batch, RA_BATCH_MAX);
    }
    if (err_replica >= 0)  // (the replica has stopped at the step that failed)
        TDGL_FAIL(ctx, TDGL_ERR_PSI_RETRIES, "%s", e->rep[err_replica].loop.budget_message(err_replica, err_dt).c_str());
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_get_mu_path(tdgl_ensemble *e, int32_t *levels, int64_t *factor_bytes) {
    if (!e) return TDGL_ERR_ARG;
    if (levels) *levels = e->levels;
    if (factor_bytes) *factor_bytes = e->factor_bytes;
    return TDGL_OK;
}

extern "C" int tdgl_ensemble_get_stats(tdgl_ensemble *e, int64_t *rounds, int64_t *batches) {
    if (!e) return TDGL_ERR_ARG;
    if (rounds) *rounds = e->stat_rounds;
    if (batches) *batches = e->stat_batches;
    return TDGL_OK;
}
