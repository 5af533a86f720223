// The per-step driver: TDGLSolver.update (tdgl/solver/solver.py:580-714) inside the loop of
// Runner._run_stage (tdgl/solver/runner.py:379-433).  Included by tdgl_hip.hip.
//
// Per step, on the context's stream:
//   1. k_psi_update      psi^n, mu^n, L psi^n (cached)  -> psi^{n+1}         (solver.py:383-439)
//   2. k_psi_laplacian   psi^{n+1} -> L psi^{n+1} (cached for step n+1) and the Poisson
//                        right-hand side b = -a (div J_s - B mu_b)           (solver.py:507-510)
//   3. AMG-PCG           A mu^{n+1} = b, warm-started from mu^n              (solver.py:516)
//   4. k_edge_currents   J_s, J_n on the edges                (operators.py:385-394, solver.py:519)
//   5. k_probes          mu / arg(psi) at the probe sites                   (solver.py:690-694)
// The host synchronises once before the PCG iterations (psi failure flag, max d|psi|^2,
// ||b||, ||r0||) and once per `check_every` PCG iterations.  The adaptive-dt controller
// (solver.py:698-707) runs on the host between steps, in the reference's arithmetic.
// psi and L psi are double-buffered so that a failed update can be repeated with a smaller
// dt (solver.py:475-485) from intact inputs.

extern "C" int tdgl_begin_stage(tdgl_ctx *ctx) {
    if (!ctx) return TDGL_ERR_ARG;
    ctx->loop.begin_stage();
    ctx->choice.reset();
    return TDGL_OK;
}

// Work counters of the time loop since the last reset: out6 = {steps accepted, psi updates that failed
// and were repeated with a smaller dt (solver.py:475-485), PCG iterations, host synchronisations,
// nanoseconds the host spent blocked in them, nanoseconds spent inside tdgl_run}.  Blocked / total
// close to 1: the GPU is the bottleneck; small: the host's launches are.
extern "C" int tdgl_get_step_stats(tdgl_ctx *ctx, int64_t *out6, int32_t reset) {
    if (!ctx || !out6) return TDGL_ERR_ARG;
    out6[0] = ctx->stat_steps;
    out6[1] = ctx->stat_psi_retries;
    out6[2] = ctx->stat_pcg_iters;
    out6[3] = ctx->stat_host_syncs;
    out6[4] = ctx->stat_wait_ns;
    out6[5] = ctx->stat_run_ns;
    if (reset)
        ctx->stat_steps = ctx->stat_psi_retries = ctx->stat_pcg_iters = ctx->stat_host_syncs = ctx->stat_wait_ns =
            ctx->stat_run_ns = 0;
    return TDGL_OK;
}

// ... and how often J_s / J_n were formed by the loop with one synchronisation per step or on request (a launch of
// k_edge_currents, or the psi update that carries them); the run-ahead loop's predicated launches are not counted
extern "C" int tdgl_get_edge_current_launches(tdgl_ctx *ctx, int64_t *count, int32_t reset) {
    if (!ctx || !count) return TDGL_ERR_ARG;
    *count = ctx->stat_edge_launches;
    if (reset) ctx->stat_edge_launches = 0;
    return TDGL_OK;
}

extern "C" int tdgl_get_loop_state(tdgl_ctx *ctx, int64_t *step, double *time, double *runner_dt,
                                   double *tentative_dt) {
    if (!ctx) return TDGL_ERR_ARG;
    ctx->loop.report(step, time, runner_dt, tentative_dt);
    return TDGL_OK;
}

extern "C" int tdgl_set_loop_state(tdgl_ctx *ctx, int64_t step, double time, double runner_dt) {
    if (!ctx) return TDGL_ERR_ARG;
    ctx->loop.restore(step, time, runner_dt);
    return TDGL_OK;
}

// Adaptive-dt controller state (solver.py:316-320, 698-707): tentative_dt and the persistent list
// d_psi_sq_vals, of which only the last `adaptive_window` entries are ever read.  Lets a caller
// checkpoint / restart a run, or replay steps from a recorded state (bench.py's parity leg).
extern "C" int tdgl_get_controller_state(tdgl_ctx *ctx, double *tentative_dt, double *history, int64_t capacity,
                                         int64_t *n_history) {
    if (!ctx || capacity < 0 || (capacity > 0 && !history)) return TDGL_ERR_ARG;
    if (tentative_dt) *tentative_dt = ctx->loop.tentative_dt;
    const int64_t have = (int64_t)ctx->loop.hist.size(), k = std::min(have, capacity);
    // the newest `k` entries, oldest first
    for (int64_t i = 0; i < k; ++i) history[i] = ctx->loop.hist[have - k + i];
    if (n_history) *n_history = have;
    return TDGL_OK;
}

extern "C" int tdgl_set_controller_state(tdgl_ctx *ctx, double tentative_dt, const double *history, int64_t n_history) {
    if (!ctx || n_history < 0 || (n_history > 0 && !history)) return TDGL_ERR_ARG;
    if (!(tentative_dt > 0.0) || !std::isfinite(tentative_dt))
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_set_controller_state: tentative_dt must be positive and finite (got %g)", tentative_dt);
    ctx->loop.restore_controller(tentative_dt, history, n_history);
    return TDGL_OK;
}

static int ensure_laplacian_cache(tdgl_ctx *ctx) {
    if (ctx->lap_valid) return TDGL_OK;
    launch_psi_laplacian(ctx, false, ctx->psi[ctx->loop.cur].p, ctx->lap[ctx->loop.cur].p);
    HIP_TRY(ctx, hipGetLastError());
    ctx->lap_valid = true;
    return TDGL_OK;
}

// the plan of the step about to be taken (tdgl_internal.h: currents_plan)
static tdgl_currents_plan step_plan(const tdgl_ctx *ctx) {
    return currents_plan({dense_on(ctx), distributed(ctx), !ctx->levels.empty(), ctx->popt.extrapolate, ctx->popt.edge_currents_every_step,
                          ctx->loop.field.moves, ctx->loop.field.has_dadt, ctx->sync_shadow_disabled, ctx->scr_enabled});
}

// what the step drivers read from the first status block of a solve: did the psi update fail, max d|psi|^2.  Returns
// pcg_solve's "go on" (false: abandon the solve, the update is repeated)
static bool psi_outcome(const StepStatus *st, bool *failed, double *dmax) {
    *failed = st->fail_flag != 0;
    unsigned long long bits = 0;
    for (int k = 0; k < 8; ++k) bits = std::max(bits, st->dmax_bits[k]);
    *dmax = __builtin_bit_cast(double, bits);
    return !*failed;
}

static int step_screening(tdgl_ctx *ctx, double *dt_out, double *dmax_out);
static int step_finish(tdgl_ctx *ctx, double dt, double dmax, double *dt_used, double *probe_mu,
                       double *probe_theta, int32_t *pcg_iters);

// Copy the probe read-outs of the steps since the last flush to the caller's arrays
// (rows [first_row, first_row + probe_ring_count) of out_mu / out_theta, n_probe columns each), and in the same
// synchronisation the census rows of those steps to the context's host vector (census.inc), followed by the records of
// those steps' vortex cores when they are on and there are any.
static int probe_ring_flush(tdgl_ctx *ctx, int64_t first_row, double *out_mu, double *out_theta) {
    const int np_ = (int)ctx->probes.size();
    const int cnt = np_ > 0 ? ctx->probe_ring_count : 0;
    ctx->probe_ring_count = 0;
    int census_rows = 0;
    TDGL_TRY(census_flush_queue(ctx, &census_rows));
    if (cnt == 0 && census_rows == 0) return TDGL_OK;
    if (cnt > 0)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_probe_out.p, ctx->d_probe_out.p, (size_t)cnt * 2 * np_ * sizeof(double),
                                    hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stat_host_syncs += 1;
    TDGL_TRY(census_flush_keep(ctx, census_rows));
    for (int k = 0; k < cnt; ++k) {
        const double *row = ctx->h_probe_out.p + (size_t)k * 2 * np_;
        if (out_mu) memcpy(out_mu + (first_row + k) * np_, row, np_ * sizeof(double));
        if (out_theta) memcpy(out_theta + (first_row + k) * np_, row + np_, np_ * sizeof(double));
    }
    return TDGL_OK;
}

// One call of TDGLSolver.update.
static int step_once(tdgl_ctx *ctx, double *dt_used, double *probe_mu, double *probe_theta,
                     int32_t *pcg_iters) {
    if (!ctx->have_links || !ctx->have_state || !ctx->have_eps)
        TDGL_FAIL(ctx, TDGL_ERR_NOT_READY, "tdgl_run: set link exponents, epsilon and state first");
    if (ctx->scr_enabled) {
        double dt_s = 0.0, dmax_s = 0.0;
        TDGL_TRY(step_screening(ctx, &dt_s, &dmax_s));
        return step_finish(ctx, dt_s, dmax_s, dt_used, probe_mu, probe_theta, pcg_iters);
    }
    TDGL_TRY(ensure_laplacian_cache(ctx));
    double dt = ctx->loop.begin_step();  // solver.py:666-668
    const int cur = ctx->loop.cur, nxt = 1 - cur;
    double dmax = 0.0;
    // (extrapolate == 3: the guess is the projection onto the previous solutions, formed inside
    // pcg_solve after the psi update is known to have succeeded -- mu^n stays in place until then)
    const bool extrapolate = ctx->popt.extrapolate && ctx->popt.extrapolate < 3 && !ctx->levels.empty();
    const double *mu_n = ctx->mu.p;  // mu^n as read by the psi update
    const tdgl_currents_plan plan = step_plan(ctx);  // where J_s, J_n of this step will be formed
    MuSolveArgs solve;
    for (bool first = true;; first = false) {
        if (mu_n == ctx->mu.p && ctx->currents.take_with_psi(plan)) {  // the previous step's, owed
            launch_psi_update_with_currents(ctx, ctx->psi[cur].p, mu_n, ctx->lap[cur].p, dt, ctx->psi[nxt].p);
        } else {
            launch_psi_update(ctx, ctx->psi[cur].p, mu_n, ctx->lap[cur].p, dt, ctx->psi[nxt].p, nullptr);
        }
        if (extrapolate && first) {
            // Initial guess of the mu solve: linear extrapolation in time.  Runs after the psi
            // update has read mu^n; afterwards mu_prev holds mu^n (a retry reads it from there)
            // and mu holds the guess the solve starts from.
            // Lagrange weights at t^{n+1} for the nodes t^n, t^{n-1}, t^{n-2}
            // Safeguard: when the controller opens the step up (dt grows 4x-1000x in one step)
            // the Lagrange weights explode and the "guess" is noise of huge norm, which costs
            // iterations and, worse, digits.  Extrapolate at most two previous steps ahead, and
            // use the quadratic only through comparable steps.
            const double h1 = ctx->prev_dt, h2 = ctx->prev_dt2;
            const double h = (h1 > 0.0) ? std::min(dt, 2.0 * h1) : dt;
            double l0 = 1.0, l1 = 0.0, l2 = 0.0;
            if (ctx->popt.extrapolate >= 2 && h1 > 0.0 && h2 > 0.0 && h1 <= 2.0 * h2 && h2 <= 2.0 * h1) {
                l0 = (h + h1) * (h + h1 + h2) / (h1 * (h1 + h2));
                l1 = -h * (h + h1 + h2) / (h1 * h2);
                l2 = h * (h + h1) / (h2 * (h1 + h2));
            } else if (h1 > 0.0) {
                l0 = 1.0 + h / h1;
                l1 = -h / h1;
            }
            hipLaunchKernelGGL(k_extrapolate, dim3(vec_grid(ctx->n_pad)), dim3(BLOCK), 0, ctx->stream,
                               ctx->n_pad, l0, l1, l2, ctx->mu.p, ctx->mu_prev.p, ctx->mu_prev2.p);
            mu_n = ctx->mu_prev.p;
        }
        // Speculative: L psi^{n+1}, the Poisson right-hand side and the PCG set-up are queued
        // before the host has seen the failure flag; a failed update simply repeats them.
        // (ghost copies of psi^{n+1} come from their owners before the stencil reads them)
        // (overlapped: the ghost-free rows of the stencil run on the compute stream while the
        // exchange travels on the communication stream; the remaining rows follow it)
        const bool ov = overlap_on(ctx);
        if (ov)
            TDGL_TRY(comm_halo_start(ctx, reinterpret_cast<double *>(ctx->psi[nxt].p), 2));
        else
            TDGL_TRY(comm_halo(ctx, reinterpret_cast<double *>(ctx->psi[nxt].p), 2));
        ProfileScope k1;
        TDGL_TRY(profile_begin(ctx, ctx->prof.admit_k1(), k1));
        if (ov) {
            launch_psi_laplacian(ctx, true, ctx->psi[nxt].p, ctx->lap[nxt].p, 1);
            TDGL_TRY(comm_halo_wait(ctx));
            launch_psi_laplacian(ctx, true, ctx->psi[nxt].p, ctx->lap[nxt].p, 2);
        } else {
            launch_psi_laplacian(ctx, true, ctx->psi[nxt].p, ctx->lap[nxt].p);
        }
        TDGL_TRY(profile_end(ctx, k1));
        bool failed = false, abandoned = false;
        solve = MuSolveArgs{ctx->popt.edge_currents_every_step != 0, plan};
        const int solve_status = pcg_solve(
            ctx, solve, [&](const StepStatus *st) { return psi_outcome(st, &failed, &dmax); }, &abandoned, /*allow_projection=*/true);
        if (solve.currents_queued && (failed || solve_status != TDGL_OK)) ctx->currents.speculation_failed();
        // A step that ends in an error must leave the accepted state behind: the extrapolation
        // moved mu^n to mu_prev and wrote a guess into mu.  Put mu^n back (the history is dropped:
        // mu^{n-2} was overwritten) so that tdgl_get_state returns the last accepted step and a
        // later tdgl_run does not extrapolate from a shifted history.
        auto roll_back_mu = [&]() {
            if (ctx->popt.extrapolate >= 3 && !abandoned) {
                // the newest basis vector IS mu^n (a failed solve does not join the basis); before the
                // first solve after tdgl_set_state there is none and pcg_solve kept a copy in mu_prev
                const double *src = ctx->guess.newest_x();
                if (!src && ctx->guess.mu_first_saved) src = ctx->mu_prev.p;
                if (src) {
                    (void)hipMemcpyAsync(ctx->mu.p, src, ctx->n_pad * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
                    // (basis vectors hold the owned rows only: the ghost copies come from their owners;
                    // every rank takes this path together, the convergence test uses all-reduced sums)
                    (void)comm_halo(ctx, ctx->mu.p, 1);
                    (void)hipStreamSynchronize(ctx->stream);
                }
            }
            if (mu_n != ctx->mu.p) {
                (void)hipMemcpyAsync(ctx->mu.p, ctx->mu_prev.p, ctx->n_pad * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
                (void)hipMemcpyAsync(ctx->mu_prev.p, ctx->mu_prev2.p, ctx->n_pad * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
                (void)hipStreamSynchronize(ctx->stream);
            }
            ctx->prev_dt = ctx->prev_dt2 = 0.0;
        };
        if (solve_status != TDGL_OK) {
            roll_back_mu();
            return solve_status;
        }
        if (!failed) break;
        if (!ctx->loop.retry()) {  // solver.py:475-485
            roll_back_mu();
            TDGL_FAIL(ctx, TDGL_ERR_PSI_RETRIES, "%s", ctx->loop.budget_message(-1, dt).c_str());
        }
        dt = ctx->loop.attempt_dt;
        ctx->stat_psi_retries += 1;
    }
    // accept the step
    ctx->prev_dt2 = ctx->prev_dt;
    ctx->prev_dt = dt;
    ctx->loop.cur = nxt;
    ctx->lap_valid = true;
    if (ctx->currents.accept(plan, solve.currents_queued)) {  // (else: queued by the direct solve already, owed, or on request)
        if (ctx->pend_v) {  // ghost values of mu still travelling: edges between owned sites first
            launch_edge_currents(ctx, ctx->psi[nxt].p, ctx->mu.p, ctx->js.p, ctx->jn.p, 1);
            TDGL_TRY(comm_halo_wait(ctx));
            launch_edge_currents(ctx, ctx->psi[nxt].p, ctx->mu.p, ctx->js.p, ctx->jn.p, 2);
        } else {
            launch_edge_currents(ctx, ctx->psi[nxt].p, ctx->mu.p, ctx->js.p, ctx->jn.p);
        }
    }
    if (ctx->pend_v) TDGL_TRY(comm_halo_wait(ctx));
    return step_finish(ctx, dt, dmax, dt_used, probe_mu, probe_theta, pcg_iters);
}

// probes (solver.py:690-694) and the adaptive time-step controller (solver.py:698-707)
static int step_finish(tdgl_ctx *ctx, double dt, double dmax, double *dt_used, double *probe_mu,
                       double *probe_theta, int32_t *pcg_iters) {
    const int nxt = ctx->loop.cur;
    const int np_ = (int)ctx->probes.size();
    if (np_ > 0 && (probe_mu || probe_theta)) {
        // running state "mu" / "theta" (solver.py:690-694, runner.py:186-221): written into a device
        // ring buffer, one slot per step, and flushed to the caller's arrays by tdgl_run once per
        // batch (probe_ring_flush) -- no host synchronisation per step
        hipLaunchKernelGGL(k_probes, dim3((np_ + 63) / 64), dim3(64), 0, ctx->stream, np_, ctx->d_probes.p,
                           ctx->psi[nxt].p, ctx->mu.p, ctx->d_probe_out.p + (size_t)ctx->probe_ring_count * 2 * np_);
        ctx->probe_ring_count += 1;
    }
    if (ctx->census.on()) census_launch(ctx, ctx->psi[nxt].p);
    HIP_TRY(ctx, hipGetLastError());
    *dt_used = dt;
    if (pcg_iters) *pcg_iters = ctx->last_pcg_iters;
    ctx->stat_steps += 1;
    ctx->choice.note_step(dmax, ctx->last_pcg_iters);
    ctx->loop.accept(dt, dmax);
    return TDGL_OK;
}

// TDGLSolver.update with include_screening (solver.py:654-688).  Reproduced as the reference
// runs it: every screening iteration (i) rebuilds the link variables from A_applied + A_induced,
// (ii) repeats the psi update FROM THE PREVIOUS ITERATION'S psi and mu with |psi|^2 of the step's
// starting psi in the formula, (iii) re-solves for mu and the currents, (iv) moves A_induced by a
// heavy-ball step towards the Biot-Savart-like integral of the site-averaged sheet current.  dt
// shrunk by a failed update stays shrunk for the remaining iterations.
static int step_screening(tdgl_ctx *ctx, double *dt_out, double *dmax_out) {
    if (distributed(ctx) && ctx->scr_Jglobal.n == 0)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "one-process-per-GPU mode: screening must be set with tdgl_set_screening_distributed");
    double dt = ctx->loop.begin_step(), dmax = 0.0, err = INFINITY;
    hipLaunchKernelGGL(k_abs_sq, dim3(grid_for(ctx->n)), dim3(BLOCK), 0, ctx->stream, ctx->n, ctx->psi[ctx->loop.cur].p,
                       ctx->abs_sq_old.p);
    HIP_TRY(ctx, hipMemsetAsync(ctx->scr_vel.p, 0, 2 * ctx->m_pad * sizeof(double), ctx->stream));
    int it = 0;
    for (;; ++it) {
        if (err < ctx->scr.tolerance) break;
        if (it > ctx->scr.max_iterations)
            TDGL_FAIL(ctx, TDGL_ERR_SCREENING,
                      "Screening calculation failed to converge at step %lld after %d iterations."
                      " Relative error in induced vector potential: %.2e (tolerance: %.2e).",
                      (long long)ctx->loop.stage_step, ctx->scr.max_iterations, err, ctx->scr.tolerance);
        const int cur = ctx->loop.cur, nxt = 1 - cur;
        screening_refresh_links(ctx);
        launch_psi_laplacian(ctx, false, ctx->psi[cur].p, ctx->lap[cur].p);
        ctx->loop.restart_retries();  // (every screening iteration has the whole budget; dt stays shrunk)
        for (;;) {
            launch_psi_update(ctx, ctx->psi[cur].p, ctx->mu.p, ctx->lap[cur].p, dt, ctx->psi[nxt].p, nullptr,
                              ctx->abs_sq_old.p);
            TDGL_TRY(comm_halo(ctx, reinterpret_cast<double *>(ctx->psi[nxt].p), 2));  // (no-op on one GPU)
            launch_psi_laplacian(ctx, true, ctx->psi[nxt].p, ctx->lap[nxt].p);
            bool failed = false, abandoned = false;
            // (mu is only written once the update is known to have succeeded)
            MuSolveArgs solve;  // (the currents follow below, in every iteration)
            TDGL_TRY(pcg_solve(
                ctx, solve, [&](const StepStatus *st) { return psi_outcome(st, &failed, &dmax); }, &abandoned, /*allow_projection=*/true));
            if (!failed) break;
            if (!ctx->loop.retry())
                TDGL_FAIL(ctx, TDGL_ERR_PSI_RETRIES, "%s", ctx->loop.budget_message(-1, dt).c_str());
            dt = ctx->loop.attempt_dt;
            ctx->stat_psi_retries += 1;
        }
        ctx->loop.cur = nxt;
        launch_edge_currents(ctx, ctx->psi[nxt].p, ctx->mu.p, ctx->js.p, ctx->jn.p);
        TDGL_TRY(screening_update_A(ctx, &err));
    }
    ctx->last_screening_iters = it;
    ctx->lap_valid = false;  // the links move with A_induced; the next step rebuilds L psi anyway
    ctx->currents.screening_done();
    ctx->prev_dt = ctx->prev_dt2 = 0.0;  // no extrapolated initial guess across screening steps
    *dt_out = dt;
    *dmax_out = dmax;
    return TDGL_OK;
}

// ---------------------------------------------------------------------------------------------------
// Run-ahead time loop (direct mu solves, static link variables, no screening, single GPU).
//
// In the classic loop the host waits for every step's outcome (failure flag, max d|psi|^2) before it can
// queue the next one: at launch-bound sizes that round trip is 10-20 us of a 50-70 us step.  Here the
// retry logic, the adaptive-dt controller and the loop's bookkeeping (solver.py:475-485, 698-707,
// runner.py:429-433) run on the device, in one thread of k_dense_sym_finish (kernels.inc: step_controller,
// same arithmetic and order as step_once / step_finish / tdgl_run), dt and "which buffer holds psi^n" are
// read from device memory by the kernels, and the host queues a whole batch of ATTEMPTS -- psi update
// (+ the owed edge currents), Laplacian / right-hand side, the direct solve, probes -- before it
// synchronises ONCE and reads the batch's records.  An attempt whose psi update fails leaves the state
// where it was and shrinks dt; the next queued attempt repeats the step, exactly as the classic retry
// loop would (one wasted attempt per retry in both).  Reaching end_time or spending the retry budget
// poisons the rest of the batch: every later kernel returns at once.
static bool run_ahead_ok(const tdgl_ctx *ctx) {
    const bool off = ctx->run_ahead_disabled;  // (TDGL_NO_RUN_AHEAD at tdgl_create)
    const tdgl_controller &ctl = ctx->loop.ctl;
    // (a moving vector potential: only the field the loop evaluates itself rides along -- k_ra_field_begin --, and it needs the
    // previous step's dt: from the second step of a stage on)
    if (ctx->loop.ramping() ? !(ctx->loop.runner_dt > 0.0) : ctx->loop.field.has_dadt) return false;
    // (the plans of the direct solve: no screening, currents every step)
    return !off && dense_on(ctx) && (ctx->direct->dense.tiles > 0) && currents_plan_runs_ahead(step_plan(ctx)) &&
           ctx->mu_tab.runs_ahead() && ctx->eps_tab.runs_ahead() && ctx->eps_spots.runs_ahead() && ctx->have_links &&
           ctx->have_state && ctx->have_eps && (!ctl.adaptive || (ctl.adaptive_window >= 1 && ctl.adaptive_window <= RA_HIST_MAX));
}

// Queues `batch` attempts, synchronises, delivers the accepted steps (out_dt[0 .. *accepted)).  *reached: the
// last accepted step reached end_time.  A spent retry budget is reported like the classic loop does.
static int run_ahead(tdgl_ctx *ctx, int batch, double end_time, double *out_dt, bool want_probes, int *accepted, bool *reached) {
    *accepted = 0;
    *reached = false;
    TDGL_TRY(ensure_laplacian_cache(ctx));
    StepCtl &h = *ctx->h_ctl.p;
    const bool ramping = ctx->loop.ramping();
    ctx->loop.fill(h, end_time, true);
    if (ramping) TDGL_TRY(ensure_link_flags(ctx));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ctl.p, &h, sizeof(StepCtl), hipMemcpyHostToDevice, ctx->stream));
    const int np_ = (int)ctx->probes.size();
    const bool probing = np_ > 0 && want_probes;
    const bool owed_on_entry = ctx->currents.owed();
    const bool mu_table = ctx->mu_tab.on(), eps_table = ctx->eps_tab.on(), eps_spots = ctx->eps_spots.on();
    if (mu_table) TDGL_TRY(ctx->mu_tab.handed_to_device(ctx));
    if (eps_table) ctx->eps_tab.handed_to_device();
    if (eps_spots) ctx->eps_spots.handed_to_device();
    for (int s = 0; s < batch; ++s) {
        if (mu_table) launch_ra_mu_table(ctx);
        if (eps_table) launch_ra_eps_table(ctx);
        if (eps_spots)
            launch_eps_spots(ctx, ctx->eps_spots, EpsSpotValues{}, ctx->eps_spots.xy.p, ctx->eps_spots.eps0.p, ctx->eps.p, ctx->d_ctl.p);
        if (ramping) {
            // A(t) moves: the owed currents of psi^n first (they belong to the links and dA/dt of the step that produced
            // it), then what TDGLSolver.update does before the psi update (solver.py:626-642) -- all of it skipped by
            // retries and dead attempts, decided on the device
            StepCtl *dc = ctx->d_ctl.p;
            const int32_t *go = &dc->ramp_do, *moved = ctx->link_changed.p;
            if (EdgeCurrents::batch_attempt_takes(s, owed_on_entry))
                hipLaunchKernelGGL(k_ra_edge_currents, dim3(grid_for(ctx->m)), dim3(BLOCK), 0, ctx->stream, ctx->m, (const int32_t *)ctx->e0.p,
                                   (const int32_t *)ctx->e1.p, (const double *)ctx->e_inv_len.p, (const double2 *)ctx->e_U.p,
                                   (const double2 *)ctx->psi[0].p, (const double2 *)ctx->psi[1].p, (const double *)ctx->mu.p, ctx->js.p, ctx->jn.p,
                                   (const double *)ctx->e_dAdt.p, (const StepCtl *)dc);
            launch_ra_field_begin(ctx);
            launch_field_links(ctx, FieldValues{}, dc);
            launch_any_flag(ctx, go);
            launch_ceff(ctx, ctx->e_dAdt.p, ctx->cvec.p, ctx->ceff.p, go);
            launch_links(ctx, nullptr, moved);
            launch_ra_laplacian_fresh(ctx);
        }
        // (the edge currents of psi^n ride along: always behind the first attempt, for the first if they are owed)
        launch_ra_psi(ctx, !ramping && EdgeCurrents::batch_attempt_takes(s, owed_on_entry));
        // (profile mode: K1, then the direct solve's launches, each bracketed once per batch -> tdgl_profile_read, _read_direct)
        ProfileScope k1, solve;
        TDGL_TRY(profile_begin(ctx, ctx->prof.admit_k1_batch(s), k1));
        launch_ra_laplacian(ctx);
        TDGL_TRY(profile_end(ctx, k1));
        TDGL_TRY(profile_begin(ctx, ctx->prof.admit_direct_batch(s), solve));
        (void)direct_solve_launch(ctx, ctx->bvec.p, ctx->mu.p, true, ctx->d_ctl.p, ctx->d_rec.p);
        TDGL_TRY(profile_end(ctx, solve));
        if (probing)
            hipLaunchKernelGGL(k_ra_probes, dim3((np_ + 63) / 64), dim3(64), 0, ctx->stream, np_, (const int32_t *)ctx->d_probes.p,
                               (const double2 *)ctx->psi[0].p, (const double2 *)ctx->psi[1].p, (const double *)ctx->mu.p,
                               ctx->d_probe_out.p, ctx->probe_ring_count, (const StepCtl *)ctx->d_ctl.p);
        if (ctx->census.on()) census_launch_ra(ctx);
    }
    ctx->psi_status_pending = false;
    const bool guard = !ctx->levels.empty();
    if (guard) {
        direct_guard_launch(ctx);
        direct_guard_fetch(ctx);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&h, ctx->d_ctl.p, sizeof(StepCtl), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_rec.p, ctx->d_rec.p, (size_t)batch * sizeof(StepRec), hipMemcpyDeviceToHost, ctx->stream));
    {
        const int64_t t0 = now_ns();
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        ctx->stat_wait_ns += now_ns() - t0;
        ctx->stat_host_syncs += 1;
        HIP_TRY(ctx, e);
    }
    if (eps_table || eps_spots) ctx->have_eps = true;
    const int done = h.n_done;
    // (mu and b are a pair when the last attempt that ran was accepted)
    if (guard) direct_guard_read(ctx, done > 0 && done <= batch && h.last_ok != 0);
    if (done == 0) TDGL_FAIL(ctx, TDGL_ERR_HIP, "run-ahead: no attempt of the batch ran");  // (cannot happen: the first one is always live)
    const LoopState::Batch b = ctx->loop.absorb(h, ctx->h_rec.p, batch, batch, ramping, out_dt);
    if (b.corrupt)
        TDGL_FAIL(ctx, TDGL_ERR_HIP, "run-ahead: corrupt attempt records (%d processed, %d accepted of %d; check %d)", done, h.n_acc, batch, b.corrupt);
    for (int s = 0; s < done; ++s)
        if (ctx->h_rec.p[s].ok) ctx->choice.note_step(ctx->h_rec.p[s].dmax, 0);
    const int acc = b.accepted;
    *accepted = acc;
    *reached = b.reached;
    ctx->stat_ra_batches += 1;
    ctx->stat_ra_dead += batch - done;
    ctx->stat_psi_retries += b.failed - (b.error ? 1 : 0);
    if (acc > 0) {
        ctx->prev_dt = ctx->prev_dt2 = 0.0;
        ctx->stat_steps += acc;
        ctx->last_pcg_iters = 0;
    }
    ctx->lap_valid = true;
    ctx->probe_ring_count += probing ? acc : 0;
    ctx->census.ring_count += ctx->census.on() ? acc : 0;
    ctx->currents.absorb_batch(done, b.last_accepted, acc, owed_on_entry);
    if (b.error) TDGL_FAIL(ctx, TDGL_ERR_PSI_RETRIES, "%s", ctx->loop.budget_message(-1, b.last_fail_dt).c_str());
    return TDGL_OK;
}

extern "C" int tdgl_run(tdgl_ctx *ctx, int64_t max_steps, double end_time, double *out_dt,
                        double *out_mu_probe, double *out_theta_probe, int32_t *out_pcg_iters,
                        int64_t *steps_done, int32_t *reached_end, int32_t *out_screening_iters) {
    CTX_GUARD(ctx);
    if (max_steps < 0 || (max_steps > 0 && !out_dt) || !steps_done || !reached_end)
        TDGL_FAIL(ctx, TDGL_ERR_ARG, "tdgl_run: bad arguments");
    *steps_done = 0;
    *reached_end = 0;
    ctx->probe_ring_count = 0;
    TDGL_TRY(census_begin_run(ctx));
    const int64_t t_enter = now_ns();
    int64_t flushed = 0;  // rows of the probe outputs already delivered
    int status = TDGL_OK;
    for (int64_t k = 0; k < max_steps && status == TDGL_OK;) {
        // a ramp that has reached its end: dA/dt is identically zero from here on (the array holds zeros; the
        // kernels drop the term), with or without the run-ahead loop
        const bool settled = ctx->loop.ramp_settled();
        if (settled && ctx->loop.field.has_dadt && !ctx->scr_enabled) ctx->loop.field.has_dadt = false;
        // direct or iterative (a pause hands over to AMG-PCG, whose projection window starts empty)
        if (ctx->choice.decide(!ctx->direct_fell_back && !distributed(ctx)) == SolverChoice::PAUSED) ctx->guess.reset();
        if (run_ahead_ok(ctx)) {
            const bool want_probes = out_mu_probe || out_theta_probe;
            int batch = (int)std::min<int64_t>(std::min<int64_t>(ctx->ra_batch, RA_BATCH_MAX), max_steps - k);
            if (!ctx->probes.empty() && want_probes) batch = std::min(batch, PROBE_RING_STEPS - ctx->probe_ring_count);
            if (ctx->census.on()) batch = std::min(batch, PROBE_RING_STEPS - ctx->census.ring_count);
            int acc = 0;
            bool reached = false;
            status = run_ahead(ctx, batch, end_time, out_dt + k, want_probes, &acc, &reached);
            for (int s = 0; s < acc; ++s) {
                if (out_pcg_iters) out_pcg_iters[k + s] = 0;
                if (out_screening_iters) out_screening_iters[k + s] = 0;
            }
            k += acc;
            *steps_done = k;
            if (status != TDGL_OK) break;
            ctx->ra_batch = std::min(2 * ctx->ra_batch, RA_BATCH_MAX);
            if (ctx->probe_ring_count >= PROBE_RING_STEPS || ctx->census.ring_count >= PROBE_RING_STEPS) {
                status = probe_ring_flush(ctx, flushed, out_mu_probe, out_theta_probe);
                flushed = k;
                if (status != TDGL_OK) break;
            }
            if (reached) {
                *reached_end = 1;
                break;
            }
            continue;
        }
        double dt = 0.0;
        if (ctx->loop.field.moves && !settled) {
            // update_applied_vector_potential (solver.py:347-362, 626-642) for the field the loop evaluates itself: every factor
            // (tdgl/sources/scaling.py LinearRamp, or a table) and every loop's values at this time; dA/dt uses the previous
            // step's dt (Runner.dt)
            double s[FIELD_TERMS_MAX], lp[FIELD_LOOPS_MAX * 4] = {};
            ctx->loop.field.values_at(ctx->loop.time, s, lp);
            status = update_field(ctx, s, lp, ctx->loop.runner_dt);
        }
        if (status == TDGL_OK) status = apply_time_tables(ctx);  // tabulated terminal currents / epsilon factor at this time
        if (status == TDGL_OK)
            status = step_once(ctx, &dt, out_mu_probe, out_theta_probe, out_pcg_iters ? out_pcg_iters + k : nullptr);
        if (status != TDGL_OK) ctx->loop.restart_retries();  // (a step given up in the middle of its retries leaves none pending)
        if (status != TDGL_OK) break;
        out_dt[k] = dt;
        if (out_screening_iters) out_screening_iters[k] = ctx->scr_enabled ? ctx->last_screening_iters : 0;
        *steps_done = k + 1;
        if (ctx->probe_ring_count >= PROBE_RING_STEPS || ctx->census.ring_count >= PROBE_RING_STEPS) {
            status = probe_ring_flush(ctx, flushed, out_mu_probe, out_theta_probe);
            flushed = k + 1;
            if (status != TDGL_OK) break;
        }
        if (ctx->loop.advance(dt, end_time)) {  // runner.py:429-433
            *reached_end = 1;
            break;
        }
        ++k;
    }
    if (ctx->currents.flush())  // J_s, J_n of the last accepted step, still owed
        launch_edge_currents(ctx, ctx->psi[ctx->loop.cur].p, ctx->mu.p, ctx->js.p, ctx->jn.p);
    // (also after an error: the steps completed before it keep their read-outs)
    const int flush_status = probe_ring_flush(ctx, flushed, out_mu_probe, out_theta_probe);
    if (status == TDGL_OK && flush_status == TDGL_OK) {
        const int64_t t0 = now_ns();
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        ctx->stat_wait_ns += now_ns() - t0;
        ctx->stat_run_ns += now_ns() - t_enter;
        HIP_TRY(ctx, e);
        return ipc_check(ctx);  // (peer-mapped transport: did every neighbour's data arrive?)
    }
    ctx->stat_run_ns += now_ns() - t_enter;
    // (peer-mapped transport: whatever went wrong after a neighbour's values failed to arrive -- a solve that does not
    // converge on garbage, for one -- is reported as what it is)
    if (ipc_check(ctx) != TDGL_OK) return TDGL_ERR_HIP;
    return status != TDGL_OK ? status : flush_status;
}
