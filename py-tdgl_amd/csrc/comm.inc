// One-process-per-GPU communication: neighbour halo exchange and small all-reduces.
// Included by tdgl_hip.hip.
//
// Two transports behind the same three calls (comm_halo, comm_allreduce, comm ready check):
//   * RCCL over xGMI (production): ncclSend/ncclRecv grouped per exchange, ncclAllReduce; all
//     enqueued on the context's stream, so no host synchronisation is added;
//   * host callbacks (tests): the library stages through pinned host buffers and hands them to
//     two caller-provided functions (the test suite implements them with torch.distributed /
//     gloo so that two ranks can share the single GPU of a test box, which RCCL refuses).
// The reference has no communication layer at all (SURVEY.md §2: "NCCL / MPI / any collective:
// none exist").

__global__ __launch_bounds__(BLOCK) void k_halo_pack(int64_t n_send, int width,
                                                     const int32_t *__restrict__ send_idx,
                                                     const double *__restrict__ v,
                                                     double *__restrict__ buf) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i >= n_send * width) return;
    const int64_t k = i / width;
    const int c = (int)(i % width);
    buf[i] = v[(int64_t)send_idx[k] * width + c];
}

// ghost entries of v <- the values received (the deep exchange: neighbours' values arrive grouped by sender, the
// ghost zone is ordered by layer)
__global__ __launch_bounds__(BLOCK) void k_halo_unpack(int64_t n_recv, const int32_t *__restrict__ recv_idx,
                                                       const double *__restrict__ buf, double *__restrict__ v) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i < n_recv) v[recv_idx[i]] = buf[i];
}

// outcome of the psi update <-> 2-double vector {fail flag, max d|psi|^2} for the MAX all-reduce
__global__ void k_status_pack(const double *__restrict__ dmax_part, const int32_t *__restrict__ fail_part,
                              int nblk, double *__restrict__ g) {
    double m;
    int f;
    reduce_psi_status(dmax_part, fail_part, nblk, &m, &f);
    if (threadIdx.x == 0) {
        g[0] = f ? 1.0 : 0.0;
        g[1] = m;
    }
}

__global__ void k_status_unpack(const double *__restrict__ g, StepStatus *__restrict__ st) {
    if (threadIdx.x == 0) {
        st->fail_flag = g[0] > 0.0 ? 1 : 0;
        st->dmax_bits[0] = (unsigned long long)__double_as_longlong(g[1]);
    }
    if (threadIdx.x > 0 && threadIdx.x < 8) st->dmax_bits[threadIdx.x] = 0ull;
}

#define NCCL_TRY(ctx, expr)                                                                    \
    do {                                                                                       \
        ncclResult_t _r = (expr);                                                              \
        if (_r != ncclSuccess)                                                                 \
            TDGL_FAIL(ctx, TDGL_ERR_HIP, "RCCL error %s at %s:%d (%s)", ncclGetErrorString(_r), \
                      __FILE__, __LINE__, #expr);                                              \
    } while (0)

static inline bool ipc_on(const tdgl_ctx *ctx) { return ctx->ipc && ctx->ipc->on; }

// (a communicator / a set of inboxes on a single rank is allowed: it exercises the decomposed sequence with world = 1)
static inline bool distributed(const tdgl_ctx *ctx) { return ctx->world > 1 || ctx->comm != nullptr || ipc_on(ctx); }

extern "C" int tdgl_comm_unique_id(char *out128) {
    if (!out128) return TDGL_ERR_ARG;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) {
        g_last_error = "ncclGetUniqueId failed";
        return TDGL_ERR_HIP;
    }
    memcpy(out128, id.internal, NCCL_UNIQUE_ID_BYTES);
    return TDGL_OK;
}

extern "C" int tdgl_set_halo_plan(tdgl_ctx *ctx, const tdgl_halo_plan *p) {
    CTX_GUARD(ctx);
    if (!p || p->world < 1 || p->rank < 0 || p->rank >= p->world || p->n_neighbors < 0 || p->n_global < ctx->n_own)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_halo_plan: invalid plan");
    if (p->n_neighbors > 0 && (!p->neighbor_ranks || !p->send_ptr || !p->send_idx || !p->recv_ptr))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_halo_plan: missing arrays");
    ctx->rank = p->rank;
    ctx->world = p->world;
    ctx->n_global = p->n_global;
    ctx->npart = NB;        // partial arrays are summed over ranks whose tile counts differ: all NB entries
    ctx->pcg_epoch += 1;
    ctx->nbr_ranks.assign(p->neighbor_ranks, p->neighbor_ranks + p->n_neighbors);
    ctx->send_ptr.assign(1, 0);
    ctx->recv_ptr.assign(1, 0);
    if (p->n_neighbors > 0) {
        ctx->send_ptr.assign(p->send_ptr, p->send_ptr + p->n_neighbors + 1);
        ctx->recv_ptr.assign(p->recv_ptr, p->recv_ptr + p->n_neighbors + 1);
    }
    const int64_t n_send = ctx->send_ptr.back(), n_recv = ctx->recv_ptr.back();
    if (n_recv != ctx->n - ctx->n_own)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "halo plan receives %lld values but the mesh has %lld ghost sites",
                  (long long)n_recv, (long long)(ctx->n - ctx->n_own));
    std::vector<int32_t> idx(p->send_idx, p->send_idx + n_send);
    for (int32_t s : idx)
        if (s < 0 || s >= ctx->n_own) TDGL_FAIL(ctx, TDGL_ERR_ARG, "halo plan sends non-owned site %d", s);
    for (size_t k = 0; k < ctx->nbr_ranks.size(); ++k)
        if (ctx->nbr_ranks[k] < 0 || ctx->nbr_ranks[k] >= p->world || ctx->nbr_ranks[k] == p->rank)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "halo plan: bad neighbour rank %d", ctx->nbr_ranks[k]);
    HIP_TRY(ctx, ctx->d_send_idx.upload(idx.empty() ? std::vector<int32_t>(1, 0) : idx));
    HIP_TRY(ctx, ctx->d_sendbuf.alloc(std::max<int64_t>(2 * n_send, 2)));
    HIP_TRY(ctx, ctx->d_gstat.alloc(2));
    const size_t hdoubles = (size_t)std::max<int64_t>({2 * n_send, 2 * n_recv, (int64_t)NB, 16});
    HIP_TRY(ctx, ctx->h_sendbuf.alloc(hdoubles, false));
    HIP_TRY(ctx, ctx->h_recvbuf.alloc(hdoubles, false));
    // Longest prefix of owned rows without a ghost neighbour (partition.py numbers the interior
    // sites first): those rows can be processed while a halo exchange is in flight.
    {
        std::vector<int32_t> e0(ctx->m), e1(ctx->m);
        HIP_TRY(ctx, hipMemcpy(e0.data(), ctx->e0.p, ctx->m * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(e1.data(), ctx->e1.p, ctx->m * sizeof(int32_t), hipMemcpyDeviceToHost));
        int64_t first = ctx->n_own;
        for (int64_t k = 0; k < ctx->m; ++k)
            if (std::max(e0[k], e1[k]) >= ctx->n_own) first = std::min<int64_t>(first, std::min(e0[k], e1[k]));
        ctx->int_tiles = (int)(first / BLOCK);
    }
    return TDGL_OK;
}

// Every overlapped exchange costs two cross-stream dependencies (compute -> communication stream
// and back).  Measured on MI355X / ROCm 7.2 (tdgl_time_kernel ids 8 / 9): two trivial dependent
// kernels take 5.8 us in one stream and 27 us across two streams, i.e. ~21 us per overlapped
// exchange -- more than the ghost-free rows of a small partition take to process.  Mode 1 (default)
// therefore overlaps only when the ghost-free part is large, mode 2 always, mode 0 never.
constexpr int64_t OVERLAP_MIN_ROWS = 750000;

static inline bool overlap_on(const tdgl_ctx *ctx) {
    if (!ctx->overlap || !distributed(ctx) || ctx->nbr_ranks.empty() || ctx->int_tiles <= 0) return false;
    // peer-mapped transport: sending and receiving are two launches on the compute stream; queueing the ghost-free
    // tiles between them costs one kernel boundary, whatever the size of the partition
    if (ipc_on(ctx)) return true;
    return ctx->overlap == 2 || (int64_t)ctx->int_tiles * BLOCK >= OVERLAP_MIN_ROWS;
}

extern "C" int tdgl_set_comm_overlap(tdgl_ctx *ctx, int32_t mode) {
    if (!ctx || mode < 0 || mode > 2) return TDGL_ERR_ARG;
    ctx->overlap = mode;
    return TDGL_OK;
}

extern "C" int tdgl_get_comm_stats(tdgl_ctx *ctx, int64_t *out4, int32_t reset) {
    if (!ctx || !out4) return TDGL_ERR_ARG;
    out4[0] = ctx->stat_halos;
    out4[1] = ctx->stat_halo_bytes;
    out4[2] = ctx->stat_allreduces;
    out4[3] = ctx->stat_allreduce_bytes;
    if (reset) ctx->stat_halos = ctx->stat_halo_bytes = ctx->stat_allreduces = ctx->stat_allreduce_bytes = 0;
    return TDGL_OK;
}

extern "C" int tdgl_get_comm_overlap(tdgl_ctx *ctx, int32_t *enabled, int64_t *interior_rows) {
    if (!ctx) return TDGL_ERR_ARG;
    if (enabled) *enabled = overlap_on(ctx) ? 1 : 0;
    if (interior_rows) *interior_rows = (int64_t)ctx->int_tiles * BLOCK;
    return TDGL_OK;
}

extern "C" int tdgl_comm_init_rccl(tdgl_ctx *ctx, const char *id128) {
    CTX_GUARD(ctx);
    if (!id128) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_comm_init_rccl: null id");
    if (ctx->world < 1 || ctx->send_ptr.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "call tdgl_set_halo_plan first");
    ncclUniqueId id;
    memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    if (ctx->comm) {
        (void)ncclCommDestroy(ctx->comm);
        ctx->comm = nullptr;
    }
    NCCL_TRY(ctx, ncclCommInitRank(&ctx->comm, ctx->world, id, ctx->rank));
    ctx->cb_halo = nullptr;
    ctx->cb_allreduce = nullptr;
    return TDGL_OK;
}

extern "C" int tdgl_comm_init_callbacks(tdgl_ctx *ctx, tdgl_halo_fn halo, tdgl_allreduce_fn allreduce, void *user) {
    if (!ctx || !halo || !allreduce) return TDGL_ERR_ARG;
    if (ctx->send_ptr.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "call tdgl_set_halo_plan first");
    ctx->cb_halo = halo;
    ctx->cb_allreduce = allreduce;
    ctx->cb_user = user;
    return TDGL_OK;
}

static int comm_ready(tdgl_ctx *ctx) {
    if (!distributed(ctx)) return TDGL_OK;
    if (!ctx->comm && !ctx->cb_halo && !ipc_on(ctx))
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "distributed context without a communicator: call tdgl_comm_init_rccl / _ipc / _callbacks");
    return TDGL_OK;
}

extern "C" int tdgl_set_deep_halo_plan(tdgl_ctx *ctx, const tdgl_deep_halo_plan *p) {
    CTX_GUARD(ctx);
    if (ctx->send_ptr.empty()) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "call tdgl_set_halo_plan first");
    if (!p) {  // off
        ctx->deep = false;
        ctx->n_ext = 0;
        return TDGL_OK;
    }
    if (p->n_ext < ctx->n || p->n_neighbors < 0 || (p->n_neighbors > 0 && (!p->neighbor_ranks || !p->send_ptr || !p->recv_ptr)))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_deep_halo_plan: invalid plan");
    ctx->deep_nbrs.assign(p->neighbor_ranks, p->neighbor_ranks + p->n_neighbors);
    ctx->deep_send_ptr.assign(1, 0);
    ctx->deep_recv_ptr.assign(1, 0);
    if (p->n_neighbors > 0) {
        ctx->deep_send_ptr.assign(p->send_ptr, p->send_ptr + p->n_neighbors + 1);
        ctx->deep_recv_ptr.assign(p->recv_ptr, p->recv_ptr + p->n_neighbors + 1);
    }
    const int64_t n_send = ctx->deep_send_ptr.back(), n_recv = ctx->deep_recv_ptr.back();
    if (n_recv != p->n_ext - ctx->n_own)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "deep halo plan receives %lld values for %lld ghost entries", (long long)n_recv,
                  (long long)(p->n_ext - ctx->n_own));
    if ((n_send > 0 && !p->send_idx) || (n_recv > 0 && !p->recv_idx)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "deep halo plan: missing index arrays");
    std::vector<int32_t> si(p->send_idx, p->send_idx + n_send), ri(p->recv_idx, p->recv_idx + n_recv);
    for (int32_t s : si)
        if (s < 0 || s >= ctx->n_own) TDGL_FAIL(ctx, TDGL_ERR_ARG, "deep halo plan sends non-owned entry %d", s);
    {
        std::vector<uint8_t> hit((size_t)(p->n_ext - ctx->n_own), 0);
        for (int32_t g : ri) {
            if (g < ctx->n_own || g >= p->n_ext || hit[(size_t)(g - ctx->n_own)])
                TDGL_FAIL(ctx, TDGL_ERR_ARG, "deep halo plan: ghost entry %d out of range or filled twice", g);
            hit[(size_t)(g - ctx->n_own)] = 1;
        }
    }
    for (size_t k = 0; k < ctx->deep_nbrs.size(); ++k)
        if (ctx->deep_nbrs[k] < 0 || ctx->deep_nbrs[k] >= ctx->world || ctx->deep_nbrs[k] == ctx->rank)
            TDGL_FAIL(ctx, TDGL_ERR_ARG, "deep halo plan: bad neighbour rank %d", ctx->deep_nbrs[k]);
    if (si.empty()) si.push_back(0);
    if (ri.empty()) ri.push_back(0);
    HIP_TRY(ctx, ctx->d_deep_send_idx.upload(si));
    HIP_TRY(ctx, ctx->d_deep_recv_idx.upload(ri));
    HIP_TRY(ctx, ctx->d_deep_sendbuf.alloc(std::max<int64_t>(n_send, 2)));
    HIP_TRY(ctx, ctx->d_deep_recvbuf.alloc(std::max<int64_t>(n_recv, 2)));
    HIP_TRY(ctx, ctx->h_deep_send.alloc((size_t)std::max<int64_t>(n_send, 2), false));
    HIP_TRY(ctx, ctx->h_deep_recv.alloc((size_t)std::max<int64_t>(n_recv, 2), false));
    ctx->n_ext = p->n_ext;
    ctx->l1_interior = std::max<int64_t>(0, p->l1_interior);
    ctx->deep = true;
    ctx->pcg_epoch += 1;
    return TDGL_OK;
}

// Refresh ALL ghost entries v[n_own .. n_ext) of a level-0 vector of the PCG (the residual): pack, exchange, unpack.
// split_phase 1: only what can be queued before the ghost-free work (peer-mapped transport: the sending launch; the other
// transports: the whole exchange, they have nothing to hide it behind on one stream)
static int comm_halo_deep(tdgl_ctx *ctx, double *v, int split_phase = 0) {
    if (!ctx->deep) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "comm_halo_deep without tdgl_set_deep_halo_plan");
    if (ctx->deep_nbrs.empty()) return TDGL_OK;
    const int64_t n_send = ctx->deep_send_ptr.back(), n_recv = ctx->deep_recv_ptr.back();
    ctx->stat_halos += 1;
    ctx->stat_deep_halos += 1;
    ctx->stat_halo_bytes += n_send * (int64_t)sizeof(double);
    if (ipc_on(ctx)) {  // two launches, no staging: the values go straight into the neighbours' inboxes
        TDGL_TRY(ipc_halo_send(ctx, ctx->ipc->deep, v, 1));
        if (split_phase == 1) return TDGL_OK;  // (the caller queues ghost-free work, then comm_halo_deep_wait)
        return ipc_halo_recv(ctx, ctx->ipc->deep, v, 1, /*indexed=*/true);
    }
    if (n_send > 0)
        hipLaunchKernelGGL(k_halo_pack, dim3(grid_for(n_send)), dim3(BLOCK), 0, ctx->stream, n_send, 1, ctx->d_deep_send_idx.p,
                           (const double *)v, ctx->d_deep_sendbuf.p);
    if (ctx->comm) {
        NCCL_TRY(ctx, ncclGroupStart());
        for (size_t k = 0; k < ctx->deep_nbrs.size(); ++k) {
            const int peer = ctx->deep_nbrs[k];
            const int64_t so = ctx->deep_send_ptr[k], sc = ctx->deep_send_ptr[k + 1] - so;
            const int64_t ro = ctx->deep_recv_ptr[k], rc = ctx->deep_recv_ptr[k + 1] - ro;
            // (an empty list on this side is an empty list on the other: both skip the call)
            if (sc > 0) NCCL_TRY(ctx, ncclSend(ctx->d_deep_sendbuf.p + so, sc, ncclDouble, peer, ctx->comm, ctx->stream));
            if (rc > 0) NCCL_TRY(ctx, ncclRecv(ctx->d_deep_recvbuf.p + ro, rc, ncclDouble, peer, ctx->comm, ctx->stream));
        }
        NCCL_TRY(ctx, ncclGroupEnd());
    } else {
        if (n_send > 0)
            HIP_TRY(ctx, hipMemcpyAsync(ctx->h_deep_send.p, ctx->d_deep_sendbuf.p, n_send * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<int64_t> so(ctx->deep_send_ptr.begin(), ctx->deep_send_ptr.end()), ro(ctx->deep_recv_ptr.begin(), ctx->deep_recv_ptr.end());
        if (ctx->cb_halo(ctx->cb_user, ctx->h_deep_send.p, so.data(), ctx->h_deep_recv.p, ro.data(), (int32_t)ctx->deep_nbrs.size(),
                         ctx->deep_nbrs.data()) != 0)
            TDGL_FAIL(ctx, TDGL_ERR_HIP, "halo exchange callback failed");
        if (n_recv > 0)
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_deep_recvbuf.p, ctx->h_deep_recv.p, n_recv * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    if (n_recv > 0)
        hipLaunchKernelGGL(k_halo_unpack, dim3(grid_for(n_recv)), dim3(BLOCK), 0, ctx->stream, n_recv, (const int32_t *)ctx->d_deep_recv_idx.p,
                           (const double *)ctx->d_deep_recvbuf.p, v);
    return TDGL_OK;
}

static int comm_halo_deep_wait(tdgl_ctx *ctx, double *v) {
    if (ipc_on(ctx) && !ctx->deep_nbrs.empty()) return ipc_halo_recv(ctx, ctx->ipc->deep, v, 1, /*indexed=*/true);
    return TDGL_OK;
}

// Refresh the ghost entries v[n_own .. n) (width doubles per site) from their owners.
static int comm_halo(tdgl_ctx *ctx, double *v, int width) {
    if (!distributed(ctx) || ctx->nbr_ranks.empty()) return TDGL_OK;
    const int64_t n_send = ctx->send_ptr.back(), n_recv = ctx->recv_ptr.back();
    ctx->stat_halos += 1;
    ctx->stat_halo_bytes += n_send * width * (int64_t)sizeof(double);
    if (ipc_on(ctx)) {
        TDGL_TRY(ipc_halo_send(ctx, ctx->ipc->thin, v, width));
        return ipc_halo_recv(ctx, ctx->ipc->thin, v, width, /*indexed=*/false);
    }
    hipLaunchKernelGGL(k_halo_pack, dim3(grid_for(n_send * width)), dim3(BLOCK), 0, ctx->stream, n_send, width,
                       ctx->d_send_idx.p, v, ctx->d_sendbuf.p);
    double *ghost = v + ctx->n_own * (int64_t)width;
    if (ctx->comm) {
        NCCL_TRY(ctx, ncclGroupStart());
        for (size_t k = 0; k < ctx->nbr_ranks.size(); ++k) {
            const int peer = ctx->nbr_ranks[k];
            const int64_t so = ctx->send_ptr[k], sc = ctx->send_ptr[k + 1] - so;
            const int64_t ro = ctx->recv_ptr[k], rc = ctx->recv_ptr[k + 1] - ro;
            NCCL_TRY(ctx, ncclSend(ctx->d_sendbuf.p + so * width, sc * width, ncclDouble, peer, ctx->comm, ctx->stream));
            NCCL_TRY(ctx, ncclRecv(ghost + ro * width, rc * width, ncclDouble, peer, ctx->comm, ctx->stream));
        }
        NCCL_TRY(ctx, ncclGroupEnd());
        return TDGL_OK;
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_sendbuf.p, ctx->d_sendbuf.p, n_send * width * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int64_t> so(ctx->send_ptr.size()), ro(ctx->recv_ptr.size());
    for (size_t k = 0; k < so.size(); ++k) {
        so[k] = (int64_t)ctx->send_ptr[k] * width;
        ro[k] = (int64_t)ctx->recv_ptr[k] * width;
    }
    if (ctx->cb_halo(ctx->cb_user, ctx->h_sendbuf.p, so.data(), ctx->h_recvbuf.p, ro.data(), (int32_t)ctx->nbr_ranks.size(),
                     ctx->nbr_ranks.data()) != 0)
        TDGL_FAIL(ctx, TDGL_ERR_HIP, "halo exchange callback failed");
    HIP_TRY(ctx, hipMemcpyAsync(ghost, ctx->h_recvbuf.p, n_recv * width * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

// The same exchange split in two so that work which does not read ghost entries can be queued in
// between (north_star: "halo exchange ... overlapped with interior updates on a second HIP
// stream").  RCCL: the pack kernel runs on the compute stream, the grouped send/recv on
// ctx->comm_stream behind an event; comm_halo_wait makes the compute stream wait for them.
// Callback transport (tests): the host exchange happens inside comm_halo_wait, after the caller
// has queued the ghost-free work.
static int comm_halo_start(tdgl_ctx *ctx, double *v, int width) {
    const int64_t n_send = ctx->send_ptr.back();
    ctx->stat_halos += 1;
    ctx->stat_halo_bytes += n_send * width * (int64_t)sizeof(double);
    ctx->pend_v = v;
    ctx->pend_width = width;
    if (ipc_on(ctx)) return ipc_halo_send(ctx, ctx->ipc->thin, v, width);  // (comm_halo_wait queues the receiving launch)
    hipLaunchKernelGGL(k_halo_pack, dim3(grid_for(n_send * width)), dim3(BLOCK), 0, ctx->stream, n_send, width,
                       ctx->d_send_idx.p, v, ctx->d_sendbuf.p);
    if (ctx->comm) {
        double *ghost = v + ctx->n_own * (int64_t)width;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_pack, ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->comm_stream, ctx->ev_pack, 0));
        NCCL_TRY(ctx, ncclGroupStart());
        for (size_t k = 0; k < ctx->nbr_ranks.size(); ++k) {
            const int peer = ctx->nbr_ranks[k];
            const int64_t so = ctx->send_ptr[k], sc = ctx->send_ptr[k + 1] - so;
            const int64_t ro = ctx->recv_ptr[k], rc = ctx->recv_ptr[k + 1] - ro;
            NCCL_TRY(ctx, ncclSend(ctx->d_sendbuf.p + so * width, sc * width, ncclDouble, peer, ctx->comm, ctx->comm_stream));
            NCCL_TRY(ctx, ncclRecv(ghost + ro * width, rc * width, ncclDouble, peer, ctx->comm, ctx->comm_stream));
        }
        NCCL_TRY(ctx, ncclGroupEnd());
        HIP_TRY(ctx, hipEventRecord(ctx->ev_halo, ctx->comm_stream));
        return TDGL_OK;
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_sendbuf.p, ctx->d_sendbuf.p, n_send * width * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_pack, ctx->stream));
    return TDGL_OK;
}

static int comm_halo_wait(tdgl_ctx *ctx) {
    double *v = ctx->pend_v;
    const int width = ctx->pend_width;
    ctx->pend_v = nullptr;
    if (!v) TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "comm_halo_wait without comm_halo_start");
    if (ipc_on(ctx)) return ipc_halo_recv(ctx, ctx->ipc->thin, v, width, /*indexed=*/false);
    if (ctx->comm) {
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_halo, 0));
        return TDGL_OK;
    }
    const int64_t n_recv = ctx->recv_ptr.back();
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_pack));
    std::vector<int64_t> so(ctx->send_ptr.size()), ro(ctx->recv_ptr.size());
    for (size_t k = 0; k < so.size(); ++k) {
        so[k] = (int64_t)ctx->send_ptr[k] * width;
        ro[k] = (int64_t)ctx->recv_ptr[k] * width;
    }
    if (ctx->cb_halo(ctx->cb_user, ctx->h_sendbuf.p, so.data(), ctx->h_recvbuf.p, ro.data(), (int32_t)ctx->nbr_ranks.size(),
                     ctx->nbr_ranks.data()) != 0)
        TDGL_FAIL(ctx, TDGL_ERR_HIP, "halo exchange callback failed");
    // the copy goes through the communication stream so that it does not queue behind the
    // ghost-free kernels; the compute stream then waits for it
    HIP_TRY(ctx, hipMemcpyAsync(v + ctx->n_own * (int64_t)width, ctx->h_recvbuf.p, n_recv * width * sizeof(double),
                                hipMemcpyHostToDevice, ctx->comm_stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_halo, ctx->comm_stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_halo, 0));
    // h_recvbuf is reused by the next exchange: make sure this copy has read it
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_halo));
    return TDGL_OK;
}

// In-place all-reduce of `count` device doubles; op: 0 = sum, 1 = max.
static int comm_allreduce(tdgl_ctx *ctx, double *dev, int64_t count, int op) {
    if (!distributed(ctx)) return TDGL_OK;
    ctx->stat_allreduces += 1;
    ctx->stat_allreduce_bytes += count * (int64_t)sizeof(double);
    if (ipc_on(ctx)) return ipc_allreduce(ctx, dev, count, op, /*as_f32=*/false);
    if (ctx->comm) {
        NCCL_TRY(ctx, ncclAllReduce(dev, dev, (size_t)count, ncclDouble, op == 0 ? ncclSum : ncclMax, ctx->comm, ctx->stream));
        return TDGL_OK;
    }
    std::vector<double> big;
    double *h = ctx->h_sendbuf.p;
    if (count > (int64_t)ctx->h_sendbuf.n) {
        big.resize(count);
        h = big.data();
    }
    HIP_TRY(ctx, hipMemcpyAsync(h, dev, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->cb_allreduce(ctx->cb_user, h, count, op) != 0) TDGL_FAIL(ctx, TDGL_ERR_HIP, "all-reduce callback failed");
    HIP_TRY(ctx, hipMemcpyAsync(dev, h, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TDGL_OK;
}

// Sum over ranks of a vector that feeds the fp32-stored V-cycle (the partial coarse right-hand sides
// R[:, owned] r): reduced in fp32 -- half the bytes on the links for the largest message of an
// iteration.  The perturbation (1e-7 relative) is the one the fp32 storage of the cycle's operators
// already makes; the CG around it is untouched.  dev is converted in place.
static int comm_allreduce_via_f32(tdgl_ctx *ctx, double *dev, int64_t count) {
    if (!distributed(ctx)) return TDGL_OK;
    if (ipc_on(ctx)) {  // carried and summed as floats by the two launches themselves
        ctx->stat_allreduces += 1;
        ctx->stat_allreduce_bytes += count * (int64_t)sizeof(float);
        return ipc_allreduce(ctx, dev, count, 0, /*as_f32=*/true);
    }
    if (ctx->world == 1) return TDGL_OK;  // (one rank: the sum is the vector)
    if ((int64_t)ctx->d_red32.n < count) HIP_TRY(ctx, ctx->d_red32.alloc(round_up(count, WAVE)));
    float *f = ctx->d_red32.p;
    hipLaunchKernelGGL(k_to_f32, dim3(grid_for(count)), dim3(BLOCK), 0, ctx->stream, count, (const double *)dev, f);
    ctx->stat_allreduces += 1;
    ctx->stat_allreduce_bytes += count * (int64_t)sizeof(float);
    if (ctx->comm) {
        NCCL_TRY(ctx, ncclAllReduce(f, f, (size_t)count, ncclFloat, ncclSum, ctx->comm, ctx->stream));
    } else {
        // callback transport (tests): the callback speaks doubles; the values stay fp32-representable
        std::vector<float> hf(count);
        std::vector<double> hd(count);
        HIP_TRY(ctx, hipMemcpyAsync(hf.data(), f, count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t i = 0; i < count; ++i) hd[i] = (double)hf[i];
        if (ctx->cb_allreduce(ctx->cb_user, hd.data(), count, 0) != 0) TDGL_FAIL(ctx, TDGL_ERR_HIP, "all-reduce callback failed");
        for (int64_t i = 0; i < count; ++i) hf[i] = (float)hd[i];
        HIP_TRY(ctx, hipMemcpyAsync(f, hf.data(), count * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    hipLaunchKernelGGL(k_from_f32, dim3(grid_for(count)), dim3(BLOCK), 0, ctx->stream, count, (const float *)f, dev);
    return TDGL_OK;
}

// ---- transport self-test (parity tests; `bench.py --selftest` before the first timed step of a multi-GPU run) ----
// One exchange / one sum through whatever transport the context uses, on caller-supplied values, so that the
// first contact of N real ranks yields a diagnosis (which rank, which neighbour, which entry) instead of a hang
// or a wrong trajectory.
extern "C" int tdgl_comm_test_halo(tdgl_ctx *ctx, double *vec_inout, int32_t width, int32_t deep) {
    CTX_GUARD(ctx);
    if (!vec_inout || (width != 1 && width != 2) || (deep && (!ctx->deep || width != 1)))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_comm_test_halo: bad arguments");
    TDGL_TRY(comm_ready(ctx));
    const int64_t len = (deep ? ctx->n_ext : ctx->n) * width;
    DevBuf<double> v;
    HIP_TRY(ctx, v.alloc(std::max<int64_t>(len, 2)));
    HIP_TRY(ctx, hipMemcpy(v.p, vec_inout, len * sizeof(double), hipMemcpyHostToDevice));
    if (deep) TDGL_TRY(comm_halo_deep(ctx, v.p));
    else TDGL_TRY(comm_halo(ctx, v.p, width));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(vec_inout, v.p, len * sizeof(double), hipMemcpyDeviceToHost));
    return ipc_check(ctx);
}

extern "C" int tdgl_comm_test_allreduce(tdgl_ctx *ctx, double *buf_inout, int64_t count, int32_t op, int32_t as_f32) {
    CTX_GUARD(ctx);
    if (!buf_inout || count < 1 || (op != 0 && op != 1) || (as_f32 && op != 0)) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_comm_test_allreduce: bad arguments");
    TDGL_TRY(comm_ready(ctx));
    DevBuf<double> v;
    HIP_TRY(ctx, v.alloc(count));
    HIP_TRY(ctx, hipMemcpy(v.p, buf_inout, count * sizeof(double), hipMemcpyHostToDevice));
    if (as_f32) TDGL_TRY(comm_allreduce_via_f32(ctx, v.p, count));
    else TDGL_TRY(comm_allreduce(ctx, v.p, count, op));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(buf_inout, v.p, count * sizeof(double), hipMemcpyDeviceToHost));
    return ipc_check(ctx);
}
