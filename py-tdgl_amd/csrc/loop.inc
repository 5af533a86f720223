// LoopState (tdgl_internal.h): the time loop's rules on the host -- retry (solver.py:475-485), adaptive dt (solver.py:698-707),
// Runner.dt / time / step (runner.py:429-433) --, once for the classic, the run-ahead and the ensemble loop.  Plain host C++:
// nothing here touches the device, so the rules can be replayed without one (tdgl_host_loop_replay).  Beside it the currents'
// ledger (EdgeCurrents) and the loop's choice of solver (SolverChoice), replayed likewise.  Included by tdgl_hip.hip.

// numpy's pairwise summation (numpy/core/src/umath/loops_utils.h.src, pairwise_sum): a plain
// left-to-right sum below 8 elements, an 8-accumulator unrolled loop up to 128, and a recursive
// split (left half rounded down to a multiple of 8) above.
static double numpy_pairwise_sum(const double *a, int64_t n) {
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int k = 0; k < 8; ++k) r[k] = a[k];
        int64_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int k = 0; k < 8; ++k) r[k] += a[i + k];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return numpy_pairwise_sum(a, n2) + numpy_pairwise_sum(a + n2, n - n2);
}

// np.mean(d_psi_sq_vals[-window:]) of a Python list (solver.py:702-704).  window == 0 selects the
// WHOLE list in Python (`vals[-0:]`), reproduced.
static double numpy_mean_tail(const std::vector<double> &v, int window) {
    const int64_t cnt = window > 0 ? std::min<int64_t>(window, (int64_t)v.size()) : (int64_t)v.size();
    return numpy_pairwise_sum(v.data() + (v.size() - cnt), cnt) / (double)cnt;
}

// host-only helper behind the controller, exported so that the summation order can be pinned
// against numpy on any machine (tests/test_host_logic.py)
extern "C" double tdgl_host_mean_tail(const double *values, int64_t n, int32_t window) {
    if (!values || n <= 0) return 0.0;
    return numpy_mean_tail(std::vector<double>(values, values + n), window);
}

namespace tdgl {

// the reference's error of a spent retry budget at this step (solver.py:480-484); replica >= 0: its index in front
std::string LoopState::budget_message(int replica, double dt) const {
    char buf[256];
    const int at = replica >= 0 ? snprintf(buf, sizeof(buf), "replica %d: ", replica) : 0;
    snprintf(buf + at, sizeof(buf) - at, "Solver failed to converge in %d retries at step %lld with dt = %.2e. Try using a smaller dt_init.",
             ctl.max_solve_retries, (long long)stage_step, dt);
    return buf;
}

// tdgl_set_controller / tdgl_ensemble_set_controller: solver.py:316-320, runner.py:262; a step's pending retries
// belonged to the previous controller
void LoopState::reset(const tdgl_controller &c) {
    ctl = c;
    tentative_dt = attempt_dt = c.dt_init;           // solver.py:319
    dt_cap = c.adaptive ? c.dt_max : c.dt_init;      // solver.py:320
    hist.clear();                                    // solver.py:318
    runner_dt = c.dt_init;                           // runner.py:262
    time = 0.0;
    stage_step = 0;
    retries = 0;
}

// tdgl_get_loop_state / tdgl_ensemble_get_loop_state: every output is optional
void LoopState::report(int64_t *step, double *time_, double *runner_dt_, double *tentative) const {
    if (step) *step = stage_step;
    if (time_) *time_ = time;
    if (runner_dt_) *runner_dt_ = runner_dt;
    if (tentative) *tentative = tentative_dt;
}

// solver.py:475-485 after a failed psi update: false -- the budget is spent (attempt_dt stays the dt that failed) --, or
// attempt_dt shrinks for the next attempt
bool LoopState::retry() {
    if (!ctl.adaptive || retries > ctl.max_solve_retries) {
        retries = 0;
        return false;
    }
    attempt_dt *= ctl.adaptive_time_step_multiplier;
    retries += 1;
    return true;
}

// the adaptive time-step controller after an accepted step (solver.py:698-707)
void LoopState::accept(double dt, double dmax) {
    retries = 0;
    if (ctl.adaptive) {
        hist.push_back(dmax);
        if (stage_step > ctl.adaptive_window) {
            const double mean = numpy_mean_tail(hist, ctl.adaptive_window);
            const double new_dt = ctl.dt_init / std::max(1e-10, mean);
            tentative_dt = std::min(std::max(0.5 * (new_dt + dt), 0.0), dt_cap);
        }
        trim();
    }
    attempt_dt = tentative_dt;
}

// runner.py:429-433: true -- the step reached end_time (tested before time advances; Runner.dt is not touched)
bool LoopState::advance(double dt, double end_time) {
    if (time >= end_time) return true;
    runner_dt = dt;
    time += runner_dt;
    stage_step += 1;
    return false;
}

// ---- FieldDrive (tdgl_internal.h): the moving applied field on the host ---------------------------------------------------
void FieldDrive::clear() {
    form = STATIC, moves = false, n_terms = 0, n_loops = 0, a0 = false, n_moves = 0;
    for (int k = 0; k < FIELD_TERMS_MAX; ++k) term[k] = FieldTerm{}, term_t[k].clear(), term_v[k].clear();
    set_loops(0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

void FieldDrive::set_product(double s) {
    clear();
    form = PRODUCT, n_terms = 1;
    scale[0] = scale_prev[0] = s;
}

void FieldDrive::set_product_source(int32_t kind, const double *ramp, const double *times, const double *values, int64_t n) {
    term[0] = FieldTerm{};
    term[0].kind = kind, term[0].n = (int32_t)n;
    for (int j = 0; j < 4 && ramp; ++j) term[0].ramp[j] = ramp[j];
    term_t[0].assign(times, times + n), term_v[0].assign(values, values + n);
    moves = kind != TERM_HOST;
}

void FieldDrive::set_terms(int n, bool with_a0, const int32_t *kind, const double *ramp, const int32_t *tab_off, const double *times,
                           const double *values) {
    clear();
    form = SUM, moves = true, n_terms = n, a0 = with_a0;
    int32_t off = 0;
    for (int k = 0; k < n; ++k) {
        term[k].kind = kind[k];
        if (kind[k] == TERM_TABLE) {
            term_t[k].assign(times + tab_off[k], times + tab_off[k + 1]);
            term_v[k].assign(values + tab_off[k], values + tab_off[k + 1]);
            term[k].off = off, term[k].n = (int32_t)term_t[k].size();
            off += term[k].n;
        } else {
            for (int j = 0; j < 4; ++j) term[k].ramp[j] = ramp[4 * k + j];
        }
        scale[k] = scale_prev[k] = value(k, 0.0);
    }
}

void FieldDrive::set_loops(int n, double z_film, const double *radii, const int32_t *tab_off, const double *times, const double *cx,
                           const double *cy, const double *cz, const double *current) {
    n_loops = n, zfilm = z_film, n_moves = 0;
    const double *src[4] = {cx, cy, cz, current};
    for (int l = 0; l < FIELD_LOOPS_MAX; ++l) {
        loop_t[l].clear();
        for (int j = 0; j < 4; ++j) loop_v[l][j].clear(), loop_par[l][j] = loop_par_prev[l][j] = 0.0;
        radius[l] = 0.0;
        if (l >= n) continue;
        radius[l] = radii[l];
        loop_t[l].assign(times + tab_off[l], times + tab_off[l + 1]);
        for (int j = 0; j < 4; ++j) loop_v[l][j].assign(src[j] + tab_off[l], src[j] + tab_off[l + 1]);
        loop_values(l, 0.0, loop_par[l]);
        for (int j = 0; j < 4; ++j) loop_par_prev[l][j] = loop_par[l][j];
    }
    if (n > 0) moves = true;
}

double FieldDrive::value(int k, double t) const {
    if (term[k].kind == TERM_TABLE) return table_value(term_t[k].data(), term_v[k].data(), (int)term_t[k].size(), t);
    if (term[k].kind == TERM_RAMP) return linear_ramp_value(t, term[k].ramp[0], term[k].ramp[1], term[k].ramp[2], term[k].ramp[3]);
    return scale[k];  // (the caller's)
}

void FieldDrive::loop_values(int l, double t, double *out4) const {
    for (int j = 0; j < 4; ++j) out4[j] = table_value(loop_t[l].data(), loop_v[l][j].data(), (int)loop_t[l].size(), t);
}

void FieldDrive::values_at(double t, double *s, double *lp) const {
    for (int k = 0; k < FIELD_TERMS_MAX; ++k) s[k] = k < n_terms ? value(k, t) : 0.0;
    for (int l = 0; l < FIELD_LOOPS_MAX; ++l)
        if (l < n_loops) loop_values(l, t, lp + 4 * l);
}

bool FieldDrive::step(const double *s, const double *lp) {
    bool same = has_dadt;
    for (int k = 0; k < n_terms; ++k) same = same && s[k] == scale[k] && s[k] == scale_prev[k];
    for (int l = 0; l < n_loops; ++l)
        for (int j = 0; j < 4; ++j) same = same && lp[4 * l + j] == loop_par[l][j] && lp[4 * l + j] == loop_par_prev[l][j];
    if (same) return false;
    for (int k = 0; k < n_terms; ++k) scale_prev[k] = scale[k], scale[k] = s[k];
    for (int l = 0; l < n_loops; ++l)
        for (int j = 0; j < 4; ++j) loop_par_prev[l][j] = loop_par[l][j], loop_par[l][j] = lp[4 * l + j];
    n_moves += 1;
    return true;
}

bool FieldDrive::settled(double time) const {
    if (!moves) return false;
    for (int k = 0; k < n_terms; ++k) {
        const bool tab = term[k].kind == TERM_TABLE;
        const double t_end = tab ? term_t[k].back() : term[k].ramp[1], f_end = tab ? term_v[k].back() : term[k].ramp[3];
        if (!(time >= t_end && scale[k] == f_end && scale_prev[k] == f_end)) return false;
    }
    for (int l = 0; l < n_loops; ++l) {
        if (!(time >= loop_t[l].back())) return false;
        for (int j = 0; j < 4; ++j)
            if (!(loop_par[l][j] == loop_v[l][j].back() && loop_par_prev[l][j] == loop_v[l][j].back())) return false;
    }
    return true;
}

void FieldDrive::fill(StepCtl &h) const {
    h.has_dadt = has_dadt ? 1 : 0;
    h.n_terms = n_terms, h.n_loops = n_loops;
    for (int k = 0; k < n_terms; ++k) h.term_scale[k] = scale[k], h.term_scale_prev[k] = scale_prev[k];
    for (int l = 0; l < n_loops; ++l)
        for (int j = 0; j < 4; ++j) h.loop_par[l][j] = loop_par[l][j], h.loop_par_prev[l][j] = loop_par_prev[l][j];
}

void FieldDrive::absorb(const StepCtl &h) {
    has_dadt = h.has_dadt != 0;
    for (int k = 0; k < n_terms; ++k) scale[k] = h.term_scale[k], scale_prev[k] = h.term_scale_prev[k];
    for (int l = 0; l < n_loops; ++l)
        for (int j = 0; j < 4; ++j) loop_par[l][j] = h.loop_par[l][j], loop_par_prev[l][j] = h.loop_par_prev[l][j];
    n_moves += h.n_term_moves;
}

void FieldDrive::describe(FieldTerm *desc, std::vector<double> &times, std::vector<double> &values) const {
    for (int k = 0; k < FIELD_TERMS_MAX; ++k) {
        desc[k] = k < n_terms ? term[k] : FieldTerm{};
        if (k >= n_terms || term[k].kind != TERM_TABLE) continue;
        desc[k].off = (int32_t)times.size();
        times.insert(times.end(), term_t[k].begin(), term_t[k].end());
        values.insert(values.end(), term_v[k].begin(), term_v[k].end());
    }
}

// the device's controller at the start of a batch; live = false: poisoned from the first attempt on
void LoopState::fill(StepCtl &h, double end_time, bool live) const {
    memset(&h, 0, sizeof(h));
    h.tentative_dt = tentative_dt;
    h.attempt_dt = retries > 0 ? attempt_dt : tentative_dt;  // (the previous batch ended in the middle of a step's retries)
    h.time = time;
    h.end_time = end_time;
    h.dt_init = ctl.dt_init;
    h.dt_cap = dt_cap;
    h.multiplier = ctl.adaptive_time_step_multiplier;
    h.stage_step = stage_step;
    h.adaptive = ctl.adaptive;
    h.window = ctl.adaptive_window;
    h.max_retries = ctl.max_solve_retries;
    h.cur = cur;
    h.retries = retries;
    h.poisoned = live ? 0 : 1;
    h.runner_dt = runner_dt;
    field.fill(h);
    if (ctl.adaptive) {
        const int64_t have = (int64_t)hist.size(), cnt = std::min<int64_t>(have, ctl.adaptive_window);
        h.hist_count = (int)cnt;
        for (int64_t i = 0; i < cnt; ++i) h.hist[i] = hist[have - cnt + i];
    }
}

// The host's mirror after a batch of `batch` attempts of which at most `limit` may have been accepted: the accepted
// steps' dt to out_dt, their max d|psi|^2 to the history, the controller's state.  ramped: the batch evaluated the ramp.
LoopState::Batch LoopState::absorb(const StepCtl &h, const StepRec *rec, int batch, int limit, bool ramped, double *out_dt) {
    Batch b;
    const int done = h.n_done;
    if (done < 0 || done > batch || h.n_acc < 0 || h.n_acc > done || h.n_acc > limit) {
        b.corrupt = 1;
        return b;
    }
    for (int s = 0; s < done; ++s) {
        if (!rec[s].ok) {
            b.failed += 1;
            b.last_fail_dt = rec[s].dt;
            continue;
        }
        out_dt[b.accepted++] = rec[s].dt;
        b.last_accepted = s;
        if (ctl.adaptive) hist.push_back(rec[s].dmax);
    }
    if (b.accepted != h.n_acc) {
        b.corrupt = 2;
        return b;
    }
    b.reached = h.reached_end != 0;
    b.error = h.error != 0;
    if (ramped) field.absorb(h);
    cur = h.cur;
    retries = b.error ? 0 : h.retries;
    attempt_dt = h.attempt_dt;
    tentative_dt = h.tentative_dt;
    time = h.time;
    stage_step = h.stage_step;
    // Runner.dt (runner.py:431) is not touched by the step that reached end_time (the loop breaks before)
    const int last = b.reached ? b.accepted - 2 : b.accepted - 1;
    if (last >= 0) runner_dt = out_dt[last];
    trim();
    return b;
}

// Where the currents of the step about to be taken are formed -- the one place that decides it.
tdgl_currents_plan currents_plan(const tdgl_currents_facts &f) {
    if (f.screening) return TDGL_CURRENTS_NOW;  // (step_screening forms them in every iteration of its own loop)
    if (!f.edge_currents_every_step) return TDGL_CURRENTS_ON_REQUEST;
    const bool links_move = f.ramp_on || f.has_dadt;  // (field ramps and dA/dt: the links change at step begin)
    // Direct solve (launch-bound sizes) with static link variables: the edge currents of an accepted step
    // are not launched on their own but ride in the NEXT step's psi-update launch (same inputs: the
    // accepted psi and mu), or are formed when tdgl_run returns -- one launch less per step.  With moving links they
    // are queued right behind the solve, before the step's synchronisation; after a failed psi update they hold
    // scratch values until the repeated step rewrites them.
    if (f.dense_on) return links_move ? TDGL_CURRENTS_SPECULATIVE : TDGL_CURRENTS_WITH_NEXT_PSI;
    // Iterative solve on one GPU: the edge currents of an accepted step are not launched in front of the next step's
    // psi update but behind the first status copy of its solve (pcg_solve), where the GPU would otherwise wait for the
    // host, or when tdgl_run returns -- every reader of J outside tdgl_run therefore finds them formed.  The old order
    // stays with: an extrapolated guess (k_extrapolate writes mu before that look), moving links, screening, one
    // process per GPU, the dense and run-ahead paths (they have no such look), currents not formed every step, and
    // TDGL_NO_SYNC_SHADOW.
    if (!f.sync_shadow_disabled && !f.distributed && f.hierarchy && f.extrapolate >= 3 && !links_move)
        return TDGL_CURRENTS_BEHIND_NEXT_LOOK;
    return TDGL_CURRENTS_NOW;
}

// new link variables (finish_links): what was formed is void; what is owed stays owed
void EdgeCurrents::new_links() {
    if (state == FORMED) state = STALE;
}

// the psi update of an attempt: true -- it carries the owed currents (every plan but the one that has a better place)
bool EdgeCurrents::take_with_psi(tdgl_currents_plan plan) {
    if (state != OWED || plan == TDGL_CURRENTS_BEHIND_NEXT_LOOK) return false;
    state = FORMED;
    return true;
}

// the first status copy of an attempt's iterative solve: true -- the owed currents follow it.  (A psi retry comes back
// for the same step with nothing owed any more.)
bool EdgeCurrents::take_behind_look(tdgl_currents_plan plan) {
    if (state != OWED || plan != TDGL_CURRENTS_BEHIND_NEXT_LOOK) return false;
    state = FORMED;
    return true;
}

// the solve queued the currents behind itself and the step failed or the solve returned an error: js / jn hold scratch
void EdgeCurrents::speculation_failed() {
    if (state == FORMED) state = STALE;
}

// a step is accepted; queued: its solve has queued them already.  true -- the caller launches them now
bool EdgeCurrents::accept(tdgl_currents_plan plan, bool queued) {
    const bool later = plan == TDGL_CURRENTS_WITH_NEXT_PSI || plan == TDGL_CURRENTS_BEHIND_NEXT_LOOK;
    const bool now = !queued && !later && plan != TDGL_CURRENTS_ON_REQUEST;
    state = queued || now ? FORMED : later ? OWED : STALE;
    return now;
}

// somebody reads them: true -- the caller launches them first
bool EdgeCurrents::request() {
    if (state == FORMED) return false;
    state = FORMED;
    return true;
}

// A run-ahead batch of which `done` attempts ran and `accepted` were accepted, the last of them as attempt `last_accepted`:
// every live attempt behind the first (the first too, if they were owed on entry: batch_attempt_takes) forms the currents
// of psi^n as it stood when the attempt began.
void EdgeCurrents::absorb_batch(int done, int last_accepted, int accepted, bool owed_on_entry) {
    if (accepted > 0)
        state = done > last_accepted + 1 ? FORMED : OWED;  // (FORMED: a later live attempt, a failed one, saw the last accepted state)
    else if (done > 0 && batch_attempt_takes(done - 1, owed_on_entry))
        state = FORMED;
}

// ---- SolverChoice (tdgl_internal.h): direct <-> iterative mu solve, decided by the state ------------------------------------
void SolverChoice::reset() {
    is_paused = false;
    switch_steps = 0;
    recent_n = 0;
    hold = 256;
    pcg_ema = 0.0;
    for (double &w : win_max) w = 0.0;
}

void SolverChoice::note_step(double dmax, int pcg_iters) {
    if (!on) return;
    recent_dmax[recent_n % WINDOW] = dmax;
    recent_n += 1;
    if (recent_n % WINDOW == 0) {  // a window is complete: its maximum joins the last three
        double worst = 0.0;
        for (int i = 0; i < WINDOW; ++i) worst = std::max(worst, recent_dmax[i]);
        win_max[0] = win_max[1];
        win_max[1] = win_max[2];
        win_max[2] = win_max[3];
        win_max[3] = worst;
    }
    switch_steps += 1;
    if (is_paused) pcg_ema = 0.95 * pcg_ema + 0.05 * (double)pcg_iters;
}

SolverChoice::Change SolverChoice::decide(bool allowed) {
    if (!on || !allowed) return NONE;
    if (!is_paused) {
        if (switch_steps < hold || recent_n < WINDOW) return NONE;
        double worst = 0.0;
        for (int i = 0; i < WINDOW; ++i) worst = std::max(worst, recent_dmax[i]);
        const double *wm = win_max;
        const bool relaxing = recent_n >= 4 * WINDOW && wm[3] < RELAX_DMAX && wm[3] < 0.9 * wm[2] && wm[2] < 0.9 * wm[1] && wm[1] < 0.9 * wm[0];
        if (!(worst < PAUSE_DMAX) && !relaxing) return NONE;
        is_paused = true;  // stationary or on its way there: the iterative solve takes over
        pcg_ema = 0.0;
    } else {
        if (switch_steps < WINDOW || pcg_ema < RESUME_ITERS) return NONE;
        is_paused = false;  // the state moves again
        // (a pause that was worth it -- a plateau of an I-V staircase -- leaves the next one its short wait; one that ended
        // right away doubles it)
        hold = switch_steps >= 1024 ? 256 : std::min<int64_t>(2 * hold, 16384);
    }
    n_switches += 1;
    switch_steps = 0;
    return is_paused ? PAUSED : RESUMED;
}

}  // namespace tdgl

// Host-only: accepted steps through the time loop's solver choice, see include/tdgl_hip.h
extern "C" int tdgl_host_solver_choice_replay(int64_t n, const double *dmax, const int32_t *iters, int64_t n_resets,
                                              const int64_t *reset_at, int32_t *paused, tdgl_solver_choice_replay *res) {
    if (n < 0 || (n > 0 && (!dmax || !iters || !paused)) || !res || n_resets < 0 || (n_resets > 0 && !reset_at)) return TDGL_ERR_ARG;
    for (int64_t k = 0; k < n_resets; ++k)
        if (reset_at[k] < 0 || reset_at[k] >= n || (k > 0 && reset_at[k] <= reset_at[k - 1])) return TDGL_ERR_ARG;
    tdgl::SolverChoice choice;
    choice.enable(true);
    for (int64_t i = 0, k = 0; i < n; ++i) {  // tdgl_run's classic branch: the decision in front of the step, the note behind it
        if (k < n_resets && reset_at[k] == i) choice.reset(), ++k;
        (void)choice.decide(true);
        paused[i] = choice.paused() ? 1 : 0;
        choice.note_step(dmax[i], iters[i]);
    }
    *res = tdgl_solver_choice_replay{choice.switches(), choice.pause_hold(), choice.paused() ? 1 : 0, 0};
    return TDGL_OK;
}

// Host-only: a scripted sequence of attempts through the loop's rules, see include/tdgl_hip.h
extern "C" int tdgl_host_loop_replay(const tdgl_controller *c, double end_time, int64_t n_attempts, const double *dmax,
                                     const int32_t *fail, int32_t batch, int32_t mode, const tdgl_controller *c_next,
                                     int64_t next_at, double *out_dt, double *out_attempt_dt, tdgl_loop_replay *res) {
    using namespace tdgl;
    if (!c || n_attempts < 0 || (n_attempts > 0 && (!dmax || !fail || !out_dt)) || !res || (mode != 0 && mode != 1)) return TDGL_ERR_ARG;
    if (mode == 1 && (batch < 1 || batch > RA_BATCH_MAX)) return TDGL_ERR_ARG;
    for (const tdgl_controller *k : {c, c_next})  // (the device's history holds RA_HIST_MAX values)
        if (k && mode == 1 && k->adaptive && (k->adaptive_window < 1 || k->adaptive_window > RA_HIST_MAX)) return TDGL_ERR_ARG;
    LoopState L;
    L.reset(*c);
    *res = tdgl_loop_replay{};
    int64_t i = 0, acc = 0;
    bool stop = false;
    while (i < n_attempts && !stop) {
        if (c_next && i == next_at) L.reset(*c_next);
        if (mode == 0) {  // the classic loop: step_once / step_finish / tdgl_run, one attempt per turn
            const double dt = L.retries > 0 ? L.attempt_dt : L.begin_step();
            if (out_attempt_dt) out_attempt_dt[i] = dt;
            const bool failed = fail[i] != 0;
            const double d = dmax[i];
            ++i;
            if (failed) {
                if (L.retry()) continue;
                res->error = 1;
                res->error_dt = dt;
                break;
            }
            L.accept(dt, d);
            out_dt[acc++] = dt;
            if (L.advance(dt, end_time)) {
                res->reached = 1;
                break;
            }
            continue;
        }
        // the run-ahead loop: a batch of attempts behind one fill, the device's controller per attempt, one absorb
        int64_t room = n_attempts - i;
        if (c_next && i < next_at) room = std::min(room, next_at - i);
        const int nb = (int)std::min<int64_t>(batch, room);
        StepCtl h;
        StepRec rec[RA_BATCH_MAX];
        L.fill(h, end_time, true);
        for (int s = 0; s < nb; ++s) {
            h.live = h.poisoned ? 0 : 1;  // (k_ra_psi_update: not poisoned when the attempt begins)
            if (h.live && out_attempt_dt) out_attempt_dt[i + h.n_done] = h.attempt_dt;
            step_controller(&h, rec, dmax[i + h.n_done], fail[i + h.n_done]);
        }
        const LoopState::Batch b = L.absorb(h, rec, nb, nb, false, out_dt + acc);
        if (b.corrupt) return TDGL_ERR_HIP;
        i += h.n_done;
        acc += b.accepted;
        if (b.error) res->error = 1, res->error_dt = b.last_fail_dt;
        if (b.reached) res->reached = 1;
        stop = b.error || b.reached;
    }
    res->n_accepted = acc;
    res->n_attempts = i;
    res->stage_step = L.stage_step;
    res->time = L.time;
    res->tentative_dt = L.tentative_dt;
    res->runner_dt = L.runner_dt;
    res->attempt_dt = L.attempt_dt;
    res->retries = L.retries;
    return TDGL_OK;
}

// Host-only: ... and through the currents' plan and ledger, see include/tdgl_hip.h.  The order of an attempt's launches
// is step_once's and run_ahead's; every decision is the ledger's.
extern "C" int tdgl_host_currents_replay(int32_t plan_in, const tdgl_currents_facts *facts, const tdgl_controller *c,
                                         double end_time, int64_t n_attempts, const double *dmax, const int32_t *fail,
                                         int32_t batch, int32_t mode, int64_t n_actions, const int64_t *action_at,
                                         const int32_t *action_kind, int64_t *formed_at, tdgl_currents_replay *res) {
    using namespace tdgl;
    if (!c || n_attempts < 0 || (n_attempts > 0 && (!dmax || !fail || !formed_at)) || !res || (mode != 0 && mode != 1) ||
        n_actions < 0 || (n_actions > 0 && (!action_at || !action_kind)))
        return TDGL_ERR_ARG;
    if (!facts && (plan_in < TDGL_CURRENTS_NOW || plan_in > TDGL_CURRENTS_ON_REQUEST)) return TDGL_ERR_ARG;
    if (mode == 1 && (batch < 1 || batch > RA_BATCH_MAX || (c->adaptive && (c->adaptive_window < 1 || c->adaptive_window > RA_HIST_MAX))))
        return TDGL_ERR_ARG;
    const tdgl_currents_plan plan = facts ? currents_plan(*facts) : (tdgl_currents_plan)plan_in;
    const bool ahead = mode == 1 && currents_plan_runs_ahead(plan);  // (run_ahead_ok)
    LoopState L;
    L.reset(*c);
    EdgeCurrents J;
    *res = tdgl_currents_replay{};
    for (int64_t k = 0; k < n_attempts; ++k) formed_at[k] = -1;
    int64_t i = 0, acc = 0, last = -1, a = 0;  // last: the accepted step whose psi and mu are the state (-1: a state that was set)
    std::vector<double> out_dt((size_t)n_attempts + 1);
    auto formed = [&](int64_t event) {
        if (last < 0) return;
        if (formed_at[last] < 0) formed_at[last] = event;
        res->n_formations += 1;
    };
    auto act = [&](int kind) {  // tdgl_run returns (its flush), then tdgl_get_state's ensure_currents or tdgl_set_state
        if (J.flush()) formed(4 * i);
        if (kind == 1 && J.request()) formed(4 * i);
        if (kind == 2) J.new_state(), L.new_state(L.cur), last = -1;
    };
    bool stop = false;
    while (i < n_attempts && !stop) {
        for (; a < n_actions && action_at[a] <= i; ++a) act(action_kind[a]);
        if (!ahead) {  // step_once: one attempt per turn
            const double dt = L.retries > 0 ? L.attempt_dt : L.begin_step();
            if (J.take_with_psi(plan)) formed(4 * i + 1);
            if (J.take_behind_look(plan)) formed(4 * i + 2);
            MuSolveArgs solve{false, plan};
            solve.speculate(true);  // (direct_mu_solve inside a step; no other solve looks at that plan)
            const bool failed = fail[i] != 0;
            const double d = dmax[i];
            ++i;
            if (failed) {
                if (solve.currents_queued) J.speculation_failed();
                if (L.retry()) continue;
                res->error = 1;
                break;
            }
            last = acc++;
            if (J.accept(plan, solve.currents_queued) || solve.currents_queued) formed(4 * (i - 1) + 3);
            L.accept(dt, d);
            if (L.advance(dt, end_time)) {
                res->reached = 1;
                break;
            }
            continue;
        }
        // run_ahead: a batch of attempts, each with the currents of the state it starts from
        const int64_t room = a < n_actions ? std::min(n_attempts, action_at[a]) - i : n_attempts - i;
        const int nb = (int)std::min<int64_t>(batch, room);
        const bool owed_on_entry = J.owed();
        StepCtl h;
        StepRec rec[RA_BATCH_MAX];
        L.fill(h, end_time, true);
        for (int s = 0; s < nb; ++s) {
            h.live = h.poisoned ? 0 : 1;
            const int64_t at = i + h.n_done;
            if (h.live && EdgeCurrents::batch_attempt_takes(s, owed_on_entry) && last >= 0 && formed_at[last] < 0) formed(4 * at + 1);
            const int before = h.n_acc;
            step_controller(&h, rec, dmax[at], fail[at]);
            if (h.n_acc > before) last = acc + before;
        }
        const LoopState::Batch b = L.absorb(h, rec, nb, nb, false, out_dt.data());
        if (b.corrupt) return TDGL_ERR_HIP;
        J.absorb_batch(h.n_done, b.last_accepted, b.accepted, owed_on_entry);
        i += h.n_done;
        acc += b.accepted;
        if (b.error) res->error = 1;
        if (b.reached) res->reached = 1;
        stop = b.error || b.reached;
    }
    for (; a < n_actions && action_at[a] <= i; ++a) act(action_kind[a]);
    act(0);
    res->n_accepted = acc;
    res->n_attempts = i;
    res->plan = plan;
    res->state = J.state;
    return TDGL_OK;
}
