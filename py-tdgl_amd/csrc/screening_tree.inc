// Screening on large meshes: a barycentric Lagrange treecode (BLTC) for the 1/r sum of screening.inc.
// Included by tdgl_hip.hip after screening.inc.
//
//   A_new[e] = sum_j w_j / |r_e - r_j|,   w_j = area_j K_site[j]   (two components)
//
// L. Wang, R. Krasny, S. Tlupova, Commun. Comput. Phys. 28 (2020); N. Vaughn, L. Wilson, R. Krasny, IPDPSW 2020.
// The sources (sites) are clustered by a tree of tight bounding boxes.  A cluster far enough from a batch of targets
// (edge centres) is replaced by its (p+1)^2 Chebyshev points of the second kind on a tensor grid over its box, which
// carry the proxy charges q_kl = sum_j L_k(x_j) L_l(y_j) w_j (barycentric Lagrange basis of the box).  Every
// interaction, near or far, is the same w / |r - s| direct sum.  The geometry never changes during a run, so the tree,
// the proxies, the transfer matrices and the interaction lists are built once, on the host; an evaluation is
//   1. gather: (x, y, w) in tree order                                            (k_tree_gather)
//   2. upward pass: the leaves from their sources, then one launch per level,
//      parents from their children through the transfer matrices                 (k_tree_leaf_charges, k_tree_upward)
//   3. one wavefront per target batch: the far list on proxies, the near list on sources   (k_tree_eval<P>)
// Every sum runs in a fixed order, without atomics: the same inputs give the same bits.  tests/bltc_model.py restates
// the algorithm in NumPy.

namespace tdgl {

constexpr int BLTC_PMAX = 17;                                         // proxies per axis: degree <= 16
constexpr int BLTC_RMAX = (BLTC_PMAX * BLTC_PMAX + WAVE - 1) / WAVE;  // proxy-grid entries per lane
constexpr int BLTC_BATCH = WAVE;                                      // targets per batch: one wavefront

struct ScrTree {
    int P = 0;  // proxies per axis, degree + 1
    double theta = 0.0;
    int32_t n_nodes = 0, n_levels = 0, n_batches = 0;
    int64_t n_src = 0, far_pairs = 0, near_pairs = 0, setup_us = 0;
    DevBuf<int32_t> src_perm;  // tree order -> internal site
    DevBuf<double4> src;       // (x, y, w_x, w_y) in tree order, written by k_tree_gather
    DevBuf<int32_t> node_begin, node_end, node_child0, node_nchild;
    DevBuf<double> node_px, node_py;  // [n_nodes][P] proxy coordinates
    DevBuf<double> tx, ty;            // [n_nodes][P][P] this node -> its parent: tx[c][k'][k] = L_parent,k'(px_c[k])
    DevBuf<double2> node_q;           // [n_nodes][P][P] proxy charges
    DevBuf<int32_t> leaves;           // leaf node ids
    std::vector<int32_t> level_off;   // internal nodes by level, deepest first: inner[level_off[i] .. level_off[i + 1])
    DevBuf<int32_t> inner;
    DevBuf<double2> tgt_xy;           // targets (edge centres) in batch order
    DevBuf<int32_t> tgt_perm;         // batch order -> internal edge
    DevBuf<int32_t> batch_off, far_off, far_list, near_off;
    DevBuf<int2> near_list;           // contiguous source ranges [x, y) in tree order
};

// ---------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(BLOCK) void k_tree_gather(int64_t n, const int32_t *__restrict__ perm,
                                                       const double *__restrict__ site_xyw, const double *__restrict__ Jsite,
                                                       double4 *__restrict__ src) {
    const int64_t t = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (t >= n) return;
    const int64_t i = perm[t];
    const double a = site_xyw[3 * i + 2];  // (the weights of k_induced_vector_potential, bit for bit)
    src[t] = make_double4(site_xyw[3 * i], site_xyw[3 * i + 1], a * Jsite[2 * i], a * Jsite[2 * i + 1]);
}

// barycentric Lagrange basis of the P Chebyshev points s[] at x into out[0..P): (w_k / (x - s_k)) / sum_l (w_l / (x - s_l));
// x on a node gives that node's unit vector
__device__ __forceinline__ void bary_basis(int P, double x, const double *s, double *out) {
    int hit = -1;
    double sum = 0.0;
    for (int k = 0; k < P; ++k) {
        const double d = x - s[k];
        if (d == 0.0 && hit < 0) hit = k;
        const double wk = ((k & 1) ? -1.0 : 1.0) * ((k == 0 || k == P - 1) ? 0.5 : 1.0);
        const double t = (d == 0.0) ? 0.0 : wk / d;
        out[k] = t;
        sum += t;
    }
    if (hit >= 0) {
        for (int k = 0; k < P; ++k) out[k] = (k == hit) ? 1.0 : 0.0;
    } else {
        const double inv = 1.0 / sum;
        for (int k = 0; k < P; ++k) out[k] *= inv;
    }
}

// One wavefront per leaf: q_kl = sum_j L_k(x_j) L_l(y_j) w_j.  A lane owns the grid entries lane, lane + 64, ... and
// sums the leaf's sources in order; the basis values of 64 sources at a time are staged in LDS.
__global__ __launch_bounds__(WAVE) void k_tree_leaf_charges(int P, const int32_t *__restrict__ leaves,
                                                            const int32_t *__restrict__ node_begin,
                                                            const int32_t *__restrict__ node_end,
                                                            const double *__restrict__ node_px,
                                                            const double *__restrict__ node_py,
                                                            const double4 *__restrict__ src, double2 *__restrict__ node_q) {
    __shared__ double lx[WAVE][BLTC_PMAX], ly[WAVE][BLTC_PMAX];
    __shared__ double2 wt[WAVE];
    __shared__ double spx[BLTC_PMAX], spy[BLTC_PMAX];
    const int lane = threadIdx.x;
    const int64_t node = leaves[blockIdx.x];
    const int b = node_begin[node], e = node_end[node];
    const int PP = P * P;
    if (lane < P) {
        spx[lane] = node_px[node * P + lane];
        spy[lane] = node_py[node * P + lane];
    }
    int kk[BLTC_RMAX], ll[BLTC_RMAX];
    double qx[BLTC_RMAX], qy[BLTC_RMAX];
#pragma unroll
    for (int r = 0; r < BLTC_RMAX; ++r) {
        const int idx = min(lane + WAVE * r, PP - 1);
        kk[r] = idx / P;
        ll[r] = idx % P;
        qx[r] = qy[r] = 0.0;
    }
    __syncthreads();
    for (int base = b; base < e; base += WAVE) {
        const int j = base + lane;
        if (j < e) {
            const double4 s = src[j];
            bary_basis(P, s.x, spx, lx[lane]);
            bary_basis(P, s.y, spy, ly[lane]);
            wt[lane] = make_double2(s.z, s.w);
        }
        __syncthreads();
        const int cnt = min(WAVE, e - base);
        for (int t = 0; t < cnt; ++t) {
            const double2 w = wt[t];
#pragma unroll
            for (int r = 0; r < BLTC_RMAX; ++r) {
                const double f = lx[t][kk[r]] * ly[t][ll[r]];
                qx[r] = fma(f, w.x, qx[r]);
                qy[r] = fma(f, w.y, qy[r]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < BLTC_RMAX; ++r) {
        const int idx = lane + WAVE * r;
        if (idx < PP) node_q[node * PP + idx] = make_double2(qx[r], qy[r]);
    }
}

// One wavefront per internal node of one level: Q = sum over the children c, in order, of Tx_c q_c Ty_c^T.
__global__ __launch_bounds__(WAVE) void k_tree_upward(int P, const int32_t *__restrict__ nodes,
                                                      const int32_t *__restrict__ node_child0,
                                                      const int32_t *__restrict__ node_nchild,
                                                      const double *__restrict__ tx, const double *__restrict__ ty,
                                                      double2 *__restrict__ node_q) {
    __shared__ double2 qs[BLTC_PMAX * BLTC_PMAX], tmp[BLTC_PMAX * BLTC_PMAX];
    const int lane = threadIdx.x;
    const int64_t node = nodes[blockIdx.x];
    const int PP = P * P;
    const int c0 = node_child0[node], nc = node_nchild[node];
    double2 acc[BLTC_RMAX];
#pragma unroll
    for (int r = 0; r < BLTC_RMAX; ++r) acc[r] = make_double2(0.0, 0.0);
    for (int c = c0; c < c0 + nc; ++c) {
        const double2 *qc = node_q + (int64_t)c * PP;
        const double *txc = tx + (int64_t)c * PP, *tyc = ty + (int64_t)c * PP;
#pragma unroll
        for (int r = 0; r < BLTC_RMAX; ++r) {
            const int idx = lane + WAVE * r;
            if (idx < PP) qs[idx] = qc[idx];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < BLTC_RMAX; ++r) {  // tmp[k'][l] = sum_k Tx[k'][k] q[k][l]
            const int idx = lane + WAVE * r;
            if (idx < PP) {
                const int kp = idx / P, l = idx % P;
                double sx = 0.0, sy = 0.0;
                for (int k = 0; k < P; ++k) {
                    const double f = txc[kp * P + k];
                    sx = fma(f, qs[k * P + l].x, sx);
                    sy = fma(f, qs[k * P + l].y, sy);
                }
                tmp[idx] = make_double2(sx, sy);
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < BLTC_RMAX; ++r) {  // Q[k'][l'] += sum_l Ty[l'][l] tmp[k'][l]
            const int idx = lane + WAVE * r;
            if (idx < PP) {
                const int kp = idx / P, lp = idx % P;
                double sx = acc[r].x, sy = acc[r].y;
                for (int l = 0; l < P; ++l) {
                    const double f = tyc[lp * P + l];
                    sx = fma(f, tmp[kp * P + l].x, sx);
                    sy = fma(f, tmp[kp * P + l].y, sy);
                }
                acc[r] = make_double2(sx, sy);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < BLTC_RMAX; ++r) {
        const int idx = lane + WAVE * r;
        if (idx < PP) node_q[node * PP + idx] = acc[r];
    }
}

// One wavefront per target batch (<= 64 targets, one per lane): the far list on the clusters' proxies, then the near
// list on the sources.  A far cluster's charges and proxy coordinates are staged in LDS and read back as broadcasts;
// the proxies are a tensor grid, so a lane keeps (y - py_l)^2 in registers and pays one add, one rsqrt_f64 and two FMAs
// per proxy.  The near sources stream through LDS in tiles of 64 as in k_induced_vector_potential.  The result goes to
// the target's slot in the context's edge order (one chunk of scr_Anew, which k_polyak reads).
template <int P>
__global__ __launch_bounds__(WAVE) void k_tree_eval(const int32_t *__restrict__ batch_off, const double2 *__restrict__ tgt_xy,
                                                    const int32_t *__restrict__ tgt_perm, const int32_t *__restrict__ far_off,
                                                    const int32_t *__restrict__ far_list, const int32_t *__restrict__ near_off,
                                                    const int2 *__restrict__ near_list, const double *__restrict__ node_px,
                                                    const double *__restrict__ node_py, const double2 *__restrict__ node_q,
                                                    const double4 *__restrict__ src, double *__restrict__ A) {
    constexpr int PP = P * P;
    __shared__ double2 sq[PP];
    __shared__ double spx[P], spy[P];
    __shared__ double4 tile[WAVE];
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const int t0 = batch_off[b], t1 = batch_off[b + 1];
    const int t = t0 + lane;
    const bool active = t < t1;
    const double2 me = tgt_xy[active ? t : t0];  // (idle lanes shadow the first target; their sums are dropped)
    double ax = 0.0, ay = 0.0;
    const int f1 = far_off[b + 1];
    for (int i = far_off[b]; i < f1; ++i) {
        const int64_t node = far_list[i];
        for (int idx = lane; idx < PP; idx += WAVE) sq[idx] = node_q[node * PP + idx];
        if (lane < P) {
            spx[lane] = node_px[node * P + lane];
            spy[lane] = node_py[node * P + lane];
        }
        __syncthreads();
        double dy2[P];
#pragma unroll
        for (int l = 0; l < P; ++l) {
            const double d = me.y - spy[l];
            dy2[l] = d * d;
        }
#pragma unroll 1
        for (int k = 0; k < P; ++k) {
            const double d = me.x - spx[k];
            const double dx2 = d * d;
#pragma unroll
            for (int l = 0; l < P; ++l) {
                const double rinv = rsqrt_f64(dx2 + dy2[l]);
                const double2 q = sq[k * P + l];
                ax = fma(q.x, rinv, ax);
                ay = fma(q.y, rinv, ay);
            }
        }
        __syncthreads();
    }
    const int n1 = near_off[b + 1];
    for (int i = near_off[b]; i < n1; ++i) {
        const int2 rg = near_list[i];
        for (int base = rg.x; base < rg.y; base += WAVE) {
            const int j = base + lane;
            tile[lane] = (j < rg.y) ? src[j] : make_double4(1e150, 1e150, 0.0, 0.0);
            __syncthreads();
            const int cnt = min(WAVE, rg.y - base);
            for (int s = 0; s < cnt; ++s) {
                const double4 v = tile[s];
                const double ddx = me.x - v.x, ddy = me.y - v.y;
                const double rinv = rsqrt_f64(fma(ddx, ddx, ddy * ddy));
                ax = fma(v.z, rinv, ax);
                ay = fma(v.w, rinv, ay);
            }
            __syncthreads();
        }
    }
    if (active) {
        const int64_t e = tgt_perm[t];
        A[2 * e] = ax;
        A[2 * e + 1] = ay;
    }
}

}  // namespace tdgl

// ---------------------------------------------------------------------------------------------- host set-up
namespace {

struct TreeNode {
    double x0, x1, y0, y1;
    int32_t begin, end, level, child0, nchild, parent;
};

// Split idx[begin, end) of node `id` recursively over tight bounding boxes (exact min / max): a node of at most
// leaf_max points is a leaf; otherwise the box is split at its midpoint in two along each axis (quad) or, when the
// aspect ratio exceeds sqrt(2) or !quad, along its long axis only.  The points keep their relative order inside each
// child, the children are appended in the order of their code (x bit + 2 * y bit) and each is one contiguous range.
// tests/bltc_model.py: build_tree is the same function.
void bltc_split(std::vector<TreeNode> &nodes, int32_t id, std::vector<int32_t> &idx, std::vector<int32_t> &scratch,
                const double *x, const double *y, int leaf_max, bool quad) {
#pragma clang fp contract(off)
    TreeNode nd = nodes[id];
    double x0 = x[idx[nd.begin]], x1 = x0, y0 = y[idx[nd.begin]], y1 = y0;
    for (int32_t i = nd.begin; i < nd.end; ++i) {
        const int32_t j = idx[i];
        x0 = std::min(x0, x[j]);
        x1 = std::max(x1, x[j]);
        y0 = std::min(y0, y[j]);
        y1 = std::max(y1, y[j]);
    }
    nd.x0 = x0, nd.x1 = x1, nd.y0 = y0, nd.y1 = y1;
    nd.child0 = -1, nd.nchild = 0;
    nodes[id] = nd;
    const double w = x1 - x0, h = y1 - y0;
    if (nd.end - nd.begin <= leaf_max || (w == 0.0 && h == 0.0)) return;
    const double sqrt2 = std::sqrt(2.0);
    bool sx, sy;
    if (quad && !(w > sqrt2 * h) && !(h > sqrt2 * w)) {
        sx = sy = true;
    } else {
        sx = w >= h;
        sy = !sx;
    }
    const double xm = 0.5 * (x0 + x1), ym = 0.5 * (y0 + y1);
    auto code = [&](int32_t j) { return ((sx && x[j] >= xm) ? 1 : 0) + ((sy && y[j] >= ym) ? 2 : 0); };
    int32_t count[4] = {0, 0, 0, 0};
    for (int32_t i = nd.begin; i < nd.end; ++i) count[code(idx[i])]++;
    int nonempty = 0;
    for (int c = 0; c < 4; ++c) nonempty += count[c] > 0;
    if (nonempty < 2) return;  // (a box a few ulps wide: its midpoint separates nothing)
    int32_t start[4], pos[4];
    start[0] = nd.begin;
    for (int c = 1; c < 4; ++c) start[c] = start[c - 1] + count[c - 1];
    for (int c = 0; c < 4; ++c) pos[c] = start[c];
    for (int32_t i = nd.begin; i < nd.end; ++i) scratch[pos[code(idx[i])]++] = idx[i];
    std::copy(scratch.begin() + nd.begin, scratch.begin() + nd.end, idx.begin() + nd.begin);
    const int32_t c0 = (int32_t)nodes.size();
    for (int c = 0; c < 4; ++c)
        if (count[c] > 0) nodes.push_back(TreeNode{0, 0, 0, 0, start[c], start[c] + count[c], nd.level + 1, -1, 0, id});
    nodes[id].child0 = c0;
    nodes[id].nchild = nonempty;
    for (int c = 0; c < nonempty; ++c) bltc_split(nodes, c0 + c, idx, scratch, x, y, leaf_max, quad);
}

std::vector<TreeNode> bltc_tree(int64_t n, const double *x, const double *y, int leaf_max, bool quad,
                                std::vector<int32_t> &idx) {
    idx.resize(n);
    std::iota(idx.begin(), idx.end(), 0);
    std::vector<int32_t> scratch(n);
    std::vector<TreeNode> nodes;
    nodes.push_back(TreeNode{0, 0, 0, 0, 0, (int32_t)n, 0, -1, 0, -1});
    bltc_split(nodes, 0, idx, scratch, x, y, leaf_max, quad);
    return nodes;
}

// P Chebyshev points of the second kind over [a, b]: (a + b) / 2 + (b - a) / 2 cos(k pi / (P - 1))
void bltc_cheb(double a, double b, int P, double *out) {
#pragma clang fp contract(off)
    const double pi = 3.141592653589793;
    const double c = 0.5 * (a + b), r = 0.5 * (b - a);
    for (int k = 0; k < P; ++k) out[k] = c + r * std::cos(pi * k / (P - 1));
}

// the host form of bary_basis
void bltc_basis(int P, double x, const double *s, double *out) {
#pragma clang fp contract(off)
    int hit = -1;
    double sum = 0.0;
    for (int k = 0; k < P; ++k) {
        const double d = x - s[k];
        if (d == 0.0 && hit < 0) hit = k;
        const double wk = ((k & 1) ? -1.0 : 1.0) * ((k == 0 || k == P - 1) ? 0.5 : 1.0);
        out[k] = (d == 0.0) ? 0.0 : wk / d;
        sum += out[k];
    }
    for (int k = 0; k < P; ++k) out[k] = hit >= 0 ? (k == hit ? 1.0 : 0.0) : out[k] / sum;
}

}  // namespace

static int build_screening_tree(tdgl_ctx *ctx, int P, double theta, tdgl::ScrTree &T) {
#pragma clang fp contract(off)
    const auto t_start = std::chrono::steady_clock::now();
    const int64_t ns = ctx->scr_n_sites, m = ctx->m;
    const int PP = P * P;
    std::vector<double> sxyw(3 * ns), exy(2 * m);
    HIP_TRY(ctx, hipMemcpy(sxyw.data(), ctx->scr_site_xyw.p, sxyw.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(exy.data(), ctx->scr_edge_xy.p, exy.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<double> sx(ns), sy(ns), ex(m), ey(m);
    for (int64_t i = 0; i < ns; ++i) sx[i] = sxyw[3 * i], sy[i] = sxyw[3 * i + 1];
    for (int64_t k = 0; k < m; ++k) ex[k] = exy[2 * k], ey[k] = exy[2 * k + 1];
    // ---- the source tree: leaves of at most (p + 1)^2 sites, so that every internal node holds more sources than proxies
    std::vector<int32_t> sperm, tperm;
    const std::vector<TreeNode> nodes = bltc_tree(ns, sx.data(), sy.data(), PP, true, sperm);
    // ---- the target batches: leaves of at most 64 edge centres.  Split along the long axis only, which keeps a leaf
    //      between 32 and 64 targets (fuller wavefronts than four-way splits give)
    const std::vector<TreeNode> tnodes = bltc_tree(m, ex.data(), ey.data(), BLTC_BATCH, false, tperm);
    const int32_t nn = (int32_t)nodes.size();
    // ---- proxies, transfer matrices, levels
    std::vector<double> px((size_t)nn * P), py((size_t)nn * P), tx((size_t)nn * PP, 0.0), ty((size_t)nn * PP, 0.0);
    std::vector<double> cx(nn), cy(nn), rad(nn);
    std::vector<int32_t> leaves, begin(nn), end(nn), child0(nn), nchild(nn);
    int32_t levels = 0;
    for (int32_t i = 0; i < nn; ++i) {
        const TreeNode &nd = nodes[i];
        bltc_cheb(nd.x0, nd.x1, P, &px[(size_t)i * P]);
        bltc_cheb(nd.y0, nd.y1, P, &py[(size_t)i * P]);
        cx[i] = 0.5 * (nd.x0 + nd.x1);
        cy[i] = 0.5 * (nd.y0 + nd.y1);
        const double w = nd.x1 - nd.x0, h = nd.y1 - nd.y0;
        rad[i] = 0.5 * std::sqrt(w * w + h * h);
        levels = std::max(levels, nd.level + 1);
        begin[i] = nd.begin, end[i] = nd.end, child0[i] = std::max(nd.child0, 0), nchild[i] = nd.nchild;
        if (nd.nchild == 0) leaves.push_back(i);
    }
    for (int32_t c = 1; c < nn; ++c) {  // exact up to round-off: the parent's basis has degree <= p in x and in y
        const int32_t p = nodes[c].parent;
        for (int k = 0; k < P; ++k) {
            double Lx[BLTC_PMAX], Ly[BLTC_PMAX];
            bltc_basis(P, px[(size_t)c * P + k], &px[(size_t)p * P], Lx);
            bltc_basis(P, py[(size_t)c * P + k], &py[(size_t)p * P], Ly);
            for (int kp = 0; kp < P; ++kp) {
                tx[(size_t)c * PP + kp * P + k] = Lx[kp];
                ty[(size_t)c * PP + kp * P + k] = Ly[kp];
            }
        }
    }
    std::vector<int32_t> inner, level_off(1, 0);
    for (int32_t lv = levels - 1; lv >= 0; --lv) {
        for (int32_t i = 0; i < nn; ++i)
            if (nodes[i].level == lv && nodes[i].nchild > 0) inner.push_back(i);
        level_off.push_back((int32_t)inner.size());
    }
    // ---- batches in target-tree order and their interaction lists: one traversal per batch, children in order.
    //      Accepted, (r_cluster + r_batch) < theta |c_cluster - c_batch|, with more sources than proxies: far list;
    //      accepted with fewer, or a leaf that fails: near list (adjacent source ranges merged)
    std::vector<int32_t> batches;
    for (int32_t i = 0; i < (int32_t)tnodes.size(); ++i)
        if (tnodes[i].nchild == 0) batches.push_back(i);
    std::sort(batches.begin(), batches.end(), [&](int32_t a, int32_t b) { return tnodes[a].begin < tnodes[b].begin; });
    const int32_t nb = (int32_t)batches.size();
    std::vector<std::vector<int32_t>> far(nb);
    std::vector<std::vector<int2>> near(nb);
    auto traverse = [&](int32_t b0, int32_t b1) {
#pragma clang fp contract(off)
        std::vector<int32_t> stack;
        for (int32_t bi = b0; bi < b1; ++bi) {
            const TreeNode &bt = tnodes[batches[bi]];
            const double bx = 0.5 * (bt.x0 + bt.x1), by = 0.5 * (bt.y0 + bt.y1);
            const double bw = bt.x1 - bt.x0, bh = bt.y1 - bt.y0;
            const double br = 0.5 * std::sqrt(bw * bw + bh * bh);
            stack.assign(1, 0);
            while (!stack.empty()) {
                const int32_t c = stack.back();
                stack.pop_back();
                const double dx = cx[c] - bx, dy = cy[c] - by;
                const bool accept = (rad[c] + br) < theta * std::sqrt(dx * dx + dy * dy);
                if (accept && end[c] - begin[c] > PP) {
                    far[bi].push_back(c);
                } else if (accept || nchild[c] == 0) {
                    if (!near[bi].empty() && near[bi].back().y == begin[c])
                        near[bi].back().y = end[c];
                    else
                        near[bi].push_back(make_int2(begin[c], end[c]));
                } else {
                    for (int32_t k = nchild[c] - 1; k >= 0; --k) stack.push_back(child0[c] + k);
                }
            }
        }
    };
    {
        const int64_t hw = std::max<int64_t>(1, (int64_t)std::thread::hardware_concurrency());
        const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, hw), nb / 256));
        std::vector<std::thread> pool;
        for (int k = 0; k < nt; ++k)
            pool.emplace_back(traverse, (int32_t)((int64_t)nb * k / nt), (int32_t)((int64_t)nb * (k + 1) / nt));
        for (auto &th : pool) th.join();
    }
    std::vector<int32_t> batch_off(nb + 1, 0), far_off(nb + 1, 0), near_off(nb + 1, 0), far_list, tgt_perm(m);
    std::vector<int2> near_list;
    std::vector<double2> tgt_xy(m);
    int64_t far_pairs = 0, near_pairs = 0;
    for (int32_t bi = 0; bi < nb; ++bi) {
        const TreeNode &bt = tnodes[batches[bi]];
        const int64_t nt = bt.end - bt.begin;
        batch_off[bi + 1] = bt.end;
        far_list.insert(far_list.end(), far[bi].begin(), far[bi].end());
        near_list.insert(near_list.end(), near[bi].begin(), near[bi].end());
        far_off[bi + 1] = (int32_t)far_list.size();
        near_off[bi + 1] = (int32_t)near_list.size();
        far_pairs += nt * (int64_t)far[bi].size() * PP;
        for (const int2 &r : near[bi]) near_pairs += nt * (int64_t)(r.y - r.x);
    }
    for (int64_t k = 0; k < m; ++k) {
        tgt_perm[k] = tperm[k];
        tgt_xy[k] = make_double2(ex[tperm[k]], ey[tperm[k]]);
    }
    if (far_list.empty()) far_list.push_back(0);  // (valid pointers; no batch reads them)
    if (near_list.empty()) near_list.push_back(make_int2(0, 0));
    // ---- upload
    HIP_TRY(ctx, T.src_perm.upload(sperm));
    HIP_TRY(ctx, T.src.alloc(ns));
    HIP_TRY(ctx, T.node_begin.upload(begin));
    HIP_TRY(ctx, T.node_end.upload(end));
    HIP_TRY(ctx, T.node_child0.upload(child0));
    HIP_TRY(ctx, T.node_nchild.upload(nchild));
    HIP_TRY(ctx, T.node_px.upload(px));
    HIP_TRY(ctx, T.node_py.upload(py));
    HIP_TRY(ctx, T.tx.upload(tx));
    HIP_TRY(ctx, T.ty.upload(ty));
    HIP_TRY(ctx, T.node_q.alloc((size_t)nn * PP));
    HIP_TRY(ctx, T.leaves.upload(leaves));
    HIP_TRY(ctx, T.inner.upload(inner.empty() ? std::vector<int32_t>(1, 0) : inner));
    HIP_TRY(ctx, T.tgt_xy.upload(tgt_xy));
    HIP_TRY(ctx, T.tgt_perm.upload(tgt_perm));
    HIP_TRY(ctx, T.batch_off.upload(batch_off));
    HIP_TRY(ctx, T.far_off.upload(far_off));
    HIP_TRY(ctx, T.near_off.upload(near_off));
    HIP_TRY(ctx, T.far_list.upload(far_list));
    HIP_TRY(ctx, T.near_list.upload(near_list));
    T.P = P;
    T.theta = theta;
    T.n_src = ns;
    T.n_nodes = nn;
    T.n_levels = levels;
    T.n_batches = nb;
    T.level_off = level_off;
    T.far_pairs = far_pairs;
    T.near_pairs = near_pairs;
    T.setup_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_start).count();
    return TDGL_OK;
}

template <int P>
static void launch_tree_eval(tdgl_ctx *ctx, const tdgl::ScrTree &T) {
    hipLaunchKernelGGL(k_tree_eval<P>, dim3(T.n_batches), dim3(WAVE), 0, ctx->stream, T.batch_off.p, T.tgt_xy.p,
                       T.tgt_perm.p, T.far_off.p, T.far_list.p, T.near_off.p, T.near_list.p, T.node_px.p, T.node_py.p,
                       T.node_q.p, T.src.p, ctx->scr_Anew.p);
}

// one tree evaluation for the site currents in ctx->scr_Jsite: the result lands in chunk 0 of scr_Anew
static void launch_tree(tdgl_ctx *ctx) {
    const tdgl::ScrTree &T = *ctx->scr_tree;
    hipLaunchKernelGGL(k_tree_gather, dim3(grid_for(T.n_src)), dim3(BLOCK), 0, ctx->stream, T.n_src, T.src_perm.p,
                       ctx->scr_site_xyw.p, ctx->scr_Jsite.p, T.src.p);
    hipLaunchKernelGGL(k_tree_leaf_charges, dim3((unsigned)T.leaves.n), dim3(WAVE), 0, ctx->stream, T.P, T.leaves.p,
                       T.node_begin.p, T.node_end.p, T.node_px.p, T.node_py.p, T.src.p, T.node_q.p);
    for (size_t lv = 0; lv + 1 < T.level_off.size(); ++lv) {
        const int32_t a = T.level_off[lv], b = T.level_off[lv + 1];
        if (b > a)
            hipLaunchKernelGGL(k_tree_upward, dim3(b - a), dim3(WAVE), 0, ctx->stream, T.P, T.inner.p + a,
                               T.node_child0.p, T.node_nchild.p, T.tx.p, T.ty.p, T.node_q.p);
    }
    switch (T.P) {
#define BLTC_CASE(p) \
    case p: launch_tree_eval<p>(ctx, T); break;
        BLTC_CASE(3) BLTC_CASE(4) BLTC_CASE(5) BLTC_CASE(6) BLTC_CASE(7) BLTC_CASE(8) BLTC_CASE(9) BLTC_CASE(10)
        BLTC_CASE(11) BLTC_CASE(12) BLTC_CASE(13) BLTC_CASE(14) BLTC_CASE(15) BLTC_CASE(16) BLTC_CASE(17)
#undef BLTC_CASE
        default: break;  // (tdgl_set_screening_tree admits degrees 2 ... 16 only)
    }
}

static bool tree_active(const tdgl_ctx *ctx) { return ctx->scr_tree != nullptr; }

extern "C" int tdgl_set_screening_tree(tdgl_ctx *ctx, int32_t degree, double theta) {
    CTX_GUARD(ctx);
    if (!ctx->scr_enabled) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_set_screening_tree: call tdgl_set_screening first");
    if (distributed(ctx) || ctx->scr_Jglobal.n > 0)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_screening_tree: tree screening is not supported in one-process-per-GPU mode");
    // validate first, then commit: a refused call leaves the previous method in place
    if (degree != 0 && (degree < 2 || degree > BLTC_PMAX - 1))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "screening_tree_degree must be in [2, %d] (got %d).", BLTC_PMAX - 1, degree);
    if (degree != 0 && !(theta > 0 && theta < 1))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "screening_tree_theta must be in (0, 1) (got %g).", theta);
    if (degree == 0) {
        ctx->scr_tree.reset();
        return TDGL_OK;
    }
    auto T = std::make_shared<tdgl::ScrTree>();
    TDGL_TRY(build_screening_tree(ctx, degree + 1, theta, *T));
    ctx->scr_tree = std::move(T);
    return TDGL_OK;
}

extern "C" int tdgl_get_screening_tree_stats(tdgl_ctx *ctx, int64_t *out) {
    CTX_GUARD(ctx);
    if (!out) TDGL_FAIL(ctx, TDGL_ERR_ARG, "null array");
    for (int k = 0; k < 6; ++k) out[k] = 0;
    if (!ctx->scr_tree) return TDGL_OK;
    const tdgl::ScrTree &T = *ctx->scr_tree;
    out[0] = T.n_nodes;
    out[1] = T.n_levels;
    out[2] = T.n_batches;
    out[3] = T.far_pairs;
    out[4] = T.near_pairs;
    out[5] = T.setup_us;
    return TDGL_OK;
}
