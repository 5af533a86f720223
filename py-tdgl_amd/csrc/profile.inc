// The in-run timers (tdgl_internal.h: Profile): the bracket around timed launches, the read-outs, and the cost of a bracket
// itself.  Included by tdgl_hip.hip.

// Begin a pair on the channel an admission rule returned (null: declined, nothing happens): two events from the pool -- created
// here only when it is empty, so that no creation falls into a timed region -- and the first record.  The launches follow.
static int profile_begin(tdgl_ctx *ctx, ProfileChannel *ch, ProfileScope &scope) {
    if (!ch) return TDGL_OK;
    for (Event *e : {&scope.a, &scope.b}) {
        if (ctx->prof.pool.empty()) {
            HIP_TRY(ctx, e->create());
        } else {
            *e = std::move(ctx->prof.pool.back());
            ctx->prof.pool.pop_back();
        }
    }
    HIP_TRY(ctx, hipEventRecord(scope.a, ctx->stream));
    scope.ch = ch;
    return TDGL_OK;
}

// ... the second record behind them; the pair waits in the channel for the next read-out
static int profile_end(tdgl_ctx *ctx, ProfileScope &scope) {
    if (!scope.ch) return TDGL_OK;
    HIP_TRY(ctx, hipEventRecord(scope.b, ctx->stream));
    scope.ch->pending.emplace_back(std::move(scope.a), std::move(scope.b));
    scope.ch = nullptr;
    return TDGL_OK;
}

extern "C" int tdgl_profile_enable(tdgl_ctx *ctx, int32_t on) {
    if (!ctx) return TDGL_ERR_ARG;
    if (on) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        while (ctx->prof.pool.size() < 1024) {  // 448 timed steps + the 64 sampled A p launches per read-out
            Event e;
            HIP_TRY(ctx, e.create());
            ctx->prof.pool.push_back(std::move(e));
        }
    }
    ctx->prof.reset(on != 0);
    return TDGL_OK;
}

// every pending pair into its channel's totals, its events back into the pool
static int profile_drain(tdgl_ctx *ctx) {
    for (ProfileChannel *ch : {&ctx->prof.k1, &ctx->prof.axp, &ctx->prof.direct}) {
        size_t done = 0;
        hipError_t e = hipSuccess;
        for (; done < ch->pending.size(); ++done) {
            auto &pr = ch->pending[done];
            float ms = 0.f;
            if ((e = hipEventSynchronize(pr.second)) != hipSuccess || (e = hipEventElapsedTime(&ms, pr.first, pr.second)) != hipSuccess) break;
            ch->ms += ms;
            ch->launches += 1;
            ctx->prof.pool.push_back(std::move(pr.first));
            ctx->prof.pool.push_back(std::move(pr.second));
        }
        ch->pending.erase(ch->pending.begin(), ch->pending.begin() + done);
        HIP_TRY(ctx, e);
    }
    return TDGL_OK;
}

static int profile_read(tdgl_ctx *ctx, const ProfileChannel &ch, int64_t *launches, double *total_ms) {
    CTX_GUARD(ctx);
    TDGL_TRY(profile_drain(ctx));
    if (launches) *launches = ch.launches;
    if (total_ms) *total_ms = ch.ms;
    return TDGL_OK;
}

extern "C" int tdgl_profile_read(tdgl_ctx *ctx, int64_t *launches, double *total_ms) {
    return ctx ? profile_read(ctx, ctx->prof.k1, launches, total_ms) : TDGL_ERR_ARG;
}

extern "C" int tdgl_profile_read_pcg(tdgl_ctx *ctx, int64_t *launches, double *total_ms) {
    return ctx ? profile_read(ctx, ctx->prof.axp, launches, total_ms) : TDGL_ERR_ARG;
}

extern "C" int tdgl_profile_read_direct(tdgl_ctx *ctx, int64_t *solves, double *total_ms) {
    return ctx ? profile_read(ctx, ctx->prof.direct, solves, total_ms) : TDGL_ERR_ARG;
}

// What an event pair reads with nothing between the two records: the marker packets' own
// processing.  bench.py reports it next to the in-run kernel durations so that they can be
// reconciled with rocprofv3's dispatch durations (which do not contain it).
extern "C" int tdgl_profile_event_overhead(tdgl_ctx *ctx, int32_t reps, double *avg_ms) {
    CTX_GUARD(ctx);
    if (reps < 1 || !avg_ms) TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_profile_event_overhead: reps >= 1 and avg_ms required");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double total = 0.0;
    for (int i = 0; i < reps; ++i) {
        Event e0, e1;
        HIP_TRY(ctx, e0.create());
        HIP_TRY(ctx, e1.create());
        HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
        HIP_TRY(ctx, hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
        total += ms;
    }
    *avg_ms = total / reps;
    return TDGL_OK;
}
