// Internal declarations of libtdgl_hip (gfx950 only).  See include/tdgl_hip.h for the ABI
// and DESIGN.md for the data layout.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_cooperative_groups.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "tdgl_hip.h"
#include "core_records.h"  // tdgl_cores::Record, assemble (plain C++)

namespace tdgl {

typedef _Float16 half_t;        // IEEE binary16 storage (level-0 V-cycle operators)
constexpr int WAVE = 64;        // CDNA wavefront
constexpr int BLOCK = 256;      // 4 waves per workgroup
constexpr int XCDS = 8;         // MI355X accelerator complex dies (one L2 each)
constexpr int REDUCE_BLOCK = 1024;
constexpr int PROBE_RING_STEPS = 1024;  // steps of probe read-outs kept on the device between flushes
constexpr int SUB_LEVELS_MAX = 3;       // levels of the nested dissection (DirectFactors::lv)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// ---------------------------------------------------------------- device buffers
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&other) noexcept { take(other); }
    DevBuf &operator=(DevBuf &&other) noexcept {
        if (this != &other) take(other);
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void take(DevBuf &other) {  // (this buffer's memory is freed, the other's becomes this one's)
        release();
        p = other.p;
        n = other.n;
        other.p = nullptr;
        other.n = 0;
    }
    hipError_t alloc(size_t count, bool zero = true) {
        release();
        n = count;
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            n = 0;
            return e;
        }
        if (zero) e = hipMemset(p, 0, count * sizeof(T));
        return e;
    }
    hipError_t upload(const std::vector<T> &h) {
        hipError_t e = alloc(h.size(), false);
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};

// ---------------------------------------------------------------- pinned host memory, events, streams
// The same shape for page-locked host memory (what an asynchronous copy lands in or leaves from)
template <class T>
struct PinnedBuf {
    T *p = nullptr;
    size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&other) noexcept : p(other.p), n(other.n) { other.p = nullptr, other.n = 0; }
    PinnedBuf &operator=(PinnedBuf &&other) noexcept {
        if (this != &other) release(), p = other.p, n = other.n, other.p = nullptr, other.n = 0;
        return *this;
    }
    ~PinnedBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count, bool zero = true) {
        release();
        n = count;
        if (count == 0) return hipSuccess;
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            n = 0;
            return e;
        }
        if (zero) memset(p, 0, count * sizeof(T));
        return e;
    }
};

// An owned runtime handle: empty until created, destroyed with its owner, read wherever the runtime wants the handle
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    Handle(Handle &&other) noexcept : h(other.h) { other.h = nullptr; }
    Handle &operator=(Handle &&other) noexcept {
        if (this != &other) release(), h = other.h, other.h = nullptr;
        return *this;
    }
    ~Handle() { release(); }
    void release() {
        if (h) (void)Destroy(h);
        h = nullptr;
    }
    operator H() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(bool timing = true) {  // (timing = false: an ordering marker only, cheaper to record)
        release();
        const hipError_t e = timing ? hipEventCreate(&h) : hipEventCreateWithFlags(&h, hipEventDisableTiming);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags = hipStreamDefault) {
        release();
        const hipError_t e = hipStreamCreateWithFlags(&h, flags);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
};
// A stream of its own with an event pair around the work of one call: what the field, vortex and sample plans are built
// on.  A plan that derives from it frees its device buffers before the stream goes (bases are destroyed last).
struct TimedStream {
    Stream stream;
    Event ev0, ev1;
    hipError_t create() {
        hipError_t e = stream.create();
        if (e == hipSuccess) e = ev0.create();
        if (e == hipSuccess) e = ev1.create();
        return e;
    }
};

// SELL-C-sigma with C = 64 (one slice per wavefront, sigma = 1: row order is kept, the
// site permutation already groups rows of equal degree).  Entry k of row r of slice s is
// stored at (slice_off[s] + k) * 64 + (r % 64): a wavefront's loads are 64 consecutive
// elements.  Padding entries point at the row itself with value 0.
struct SellPattern {
    int64_t n_rows = 0, n_pad = 0;
    int32_t n_slices = 0;
    int64_t n_slots = 0;  // slice_off[n_slices] * 64
    DevBuf<int32_t> slice_off;
    DevBuf<int32_t> cols;
    // Square operators in RCM order: column - row fits 16 bits (the bandwidth is ~2 sqrt(n)), which
    // halves the index stream of the kernels that run at the HBM ceiling.  Built only on request
    // and only when every delta fits; kernels fall back to `cols` otherwise.
    DevBuf<int16_t> cols16;
    bool use16 = false;
    // Rectangular operators (the level-0 prolongation): column - slice_base[slice] as 16 unsigned
    // bits, when the columns of every 64-row slice span < 65536 (coarse numbering follows the fine one).
    DevBuf<uint16_t> offs16;
    DevBuf<int32_t> slice_base;
    bool use_off16 = false;
};

struct SellF64 {
    SellPattern pat;
    DevBuf<double> vals;
};

struct Csr {
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    DevBuf<int32_t> indptr, indices;
    DevBuf<double> data;
    DevBuf<float> data32;  // fp32 copy of the values (mixed-precision preconditioner), on demand
};

// how the stored-precision cycle reads a level-0 operator (A, P, the fused restriction): values and indices
enum class StoredForm { F32_I32, F32_I16, F16_I16 };

// Level 0 (rows ~ 10^6, 7 entries each) streams through SELL-64, one lane per row.  Coarse
// levels and the restriction have few, longer rows: one lane per row would be a single long
// dependent gather chain per wave, so they use CSR with several lanes per row instead.
struct AmgLevel {
    int64_t n = 0, n_pad = 0, n_coarse = 0;
    int64_t n_cols = 0;              // entries of this level's right-hand side / iterate vectors (>= n: ghost entries)
    bool explicit_only = false;      // a distributed level 1: no A / P / R, only M, Wup, Vneg
    double rho = 2.0;
    SellF64 A;                       // level 0
    Csr Ac;                          // levels >= 1
    DevBuf<double> dinv;
    SellF64 P;                       // prolongation n x n_coarse (level 0)
    Csr Pc, R;                       // prolongation (levels >= 1); restriction n_coarse x n
    DevBuf<double> xa, xb, d, b, r;  // level vectors (level 0 borrows b from PCG)
    // fp32 copies of the level-0 V-cycle operators / iterates (mixed-precision preconditioner)
    DevBuf<float> A32, P32, dinv32, x32a, x32b;
    DevBuf<half_t> A16, P16;         // the same operators in binary16 (popt.precond_fp32 == 2)
    // optional pre-multiplied operators of a coarse level (tdgl_poisson_set_fused_level)
    bool fused = false;
    Csr RA;                          // R A   [n_coarse x n]
    Csr AP;                          // A P   [n x n_coarse]
    DevBuf<double> APp;              // P on the pattern of A P
    DevBuf<float> APp32;
    // collapsed coarse chain (tdgl_poisson_set_collapsed_level): M = R (I - A S) [n_coarse x n]
    Csr M;
    // ... and the way up as explicit operators (tdgl_poisson_set_collapsed_up): e = Wup b - Vneg e_next,
    // Wup = T_x S + T_b [n x n], Vneg = -T_x P [n x n_coarse]
    Csr Wup, Vneg;
    // compact forms for k_mid_up (when they fit): W columns = up_wbase[row] + up_woff, V columns 16-bit
    DevBuf<int32_t> up_wbase;
    DevBuf<uint16_t> up_woff, up_vidx;
    DevBuf<half_t> up_w16, up_v16;   // binary16 values (popt.precond_fp32 >= 2)
};

// scalars of the PCG recurrence, resident on the device
// (S_CONV_IT: first frozen iteration or -1; S_IT: iterations launched so far in this solve; S_TOL2:
// rtol^2 ||b||^2 -- kept on the device so that the iteration kernels take no per-iteration
// arguments and a pair of iterations can be replayed as a hipGraph)
// (S_CG_*: r.z and alpha of the previous iteration for the single-reduction CG, ping-pong by parity)
// (S_RR0: ||r_0||^2 of the current solve, recorded by the first update: the quality of the initial guess)
// (S_ALPHA: alpha of the last CG update, read by the next direction update's flexible beta)
enum Scal { S_RR = 0, S_BB, S_CONV_IT, S_IT, S_TOL2, S_CG_RZ0, S_CG_RZ1, S_CG_ALPHA0, S_CG_ALPHA1, S_RR0, S_ALPHA, S_COUNT = 12 };

// what a step reports back to the host at its synchronisation point
// arguments of the CG update x += alpha p, r -= alpha q (kernels.inc: xr_update_body)
struct XrArgs {
    const double *p, *q, *part_rz, *part_pq, *part_rr_in;
    double *scal, *x, *r, *part_rr_out;
    int64_t n;
    int npart;  // entries of every partial array in use (tdgl_ctx::npart)
    double *part_sx = nullptr;  // (optional) partials of sum x after the update: the zero-mean gauge needs no pass of its own
};

// up to 64 consecutive interior rows of ONE part of a substructure level, the work of one wavefront of the way up
// (kernels.inc: k_sub_up): where column `first row` of the part's -E_p^T block starts in the value pool, the part's
// size (= the block's row length), where the part's separator index list starts and how many entries it has,
// the chunk's first row and its rows
struct SubUpChunk {
    int64_t et;
    int32_t np, s0, cnt, row0, n_rows;
};

// the way down (kernels.inc: k_sub_down): a chunk of consecutive interior rows of ONE part -- where its first row of
// G_p starts in the pool, where b_p starts, the part's size, the chunk's first row and its rows -- and a row of the
// rest (separator rows, (G_p 1)^T rows) with up to four segments inline (nseg < 0: more, see the segment lists)
struct SubDownChunk {
    int64_t g;
    int32_t x0, ncols, row0, n_rows;
    int32_t ld, pad;  // (lane-per-row form: distance between consecutive rows of the part's G block in the pool; == ncols unless repacked)
};
// one part of a level while its fp64 pool is repacked into the padded fp32 pool (k_sub_repack)
struct SubRepack {
    int64_t old_g, new_g, old_et, new_et;
    int32_t np, sp, ld, pad;
};
struct SubDownRow {
    int32_t nseg, pad;
    int64_t val[4];
    int32_t x[4], len[4];
};

constexpr int GUESS_MAX = 16;  // maximal window of the projection guess (kernels.inc: GK)

// Run-ahead time loop of the direct solves (run.inc: run_ahead): the adaptive-dt controller and the loop's
// bookkeeping live on the device, so that the host can queue a batch of steps without waiting for each
// step's outcome.  `poisoned` stops everything behind a failed psi update (the host repeats that step the
// classic way with a smaller dt) or behind the step that reached end_time.
constexpr int RA_HIST_MAX = 128;   // adaptive_window up to here (numpy's pairwise sum has no recursion below 129 terms)
constexpr int RA_BATCH_MAX = 64;
// A moving applied field A(t) = A_0 + f_1(t) A_1 + ... + f_K(t) A_K + sum_l I_l(t) Aloop(r - c_l(t); a_l) (FieldDrive below): at
// most this many products, and where the factor of one of them comes from -- the caller (tdgl_update_link_scale), a LinearRamp
// (ramp: tmin, tmax, initial, final) or a table (nodes off .. off + n of the owner's pools of times and values)
constexpr int FIELD_TERMS_MAX = 4;
enum : int32_t { TERM_HOST = 0, TERM_RAMP = 1, TERM_TABLE = 2 };
struct FieldTerm {
    int32_t kind, off, n, pad;
    double ramp[4];
};
// ... and at most this many moving current loops (tdgl_set_link_loops); a loop's four tables (centre x, y, z and current) share
// the nodes off .. off + n of the owner's pools
constexpr int FIELD_LOOPS_MAX = 2;
struct FieldLoop {
    int32_t off, n;
    double radius;
};
struct StepCtl {
    double tentative_dt;   // dt the next STEP starts from (solver.py:316-320, 698-707)
    double attempt_dt;     // dt of the next attempt: tentative_dt, times the multiplier per failed attempt of the step
    double time;           // Runner.time (runner.py:433)
    double end_time;
    double dt_init, dt_cap, multiplier;
    long long stage_step;  // Runner step index of the current stage
    int adaptive, window, max_retries;
    int cur;               // which psi / L psi buffer holds psi^n
    int retries;           // failed attempts of the current step so far
    int poisoned;          // no further attempt may run (end reached, or the retry budget is spent)
    int live;              // the attempt being processed started un-poisoned (set by its psi-update kernel)
    int last_ok;           // ... and was accepted
    int reached_end, error;
    int n_done;            // attempts processed since the batch began
    int n_acc;             // ... of which accepted
    int hist_count;
    int pad;
    double hist[RA_HIST_MAX];  // the last min(window, count) values of max d|psi|^2, oldest first
    // the moving applied field evaluated inside the loop (k_ra_field_begin; FieldDrive::fill / absorb)
    double runner_dt;          // Runner.dt: dt of the previous accepted step (the dA/dt of this one divides by it)
    int has_dadt;              // a dynamic update has run (the step rule's "nothing moves" needs one)
    int ramp_do;               // this attempt is the first of a step and the vector potential moves
    int n_terms, n_loops;      // products and loops of the field
    int n_term_moves, pad2;    // attempts of this batch that moved the field (ran the body of the links kernel)
    // the factors of the current / previous A, term by term; centre x, y, z and current of the current / previous A, loop by loop
    double term_scale[FIELD_TERMS_MAX], term_scale_prev[FIELD_TERMS_MAX];
    double loop_par[FIELD_LOOPS_MAX][4], loop_par_prev[FIELD_LOOPS_MAX][4];
};
struct StepRec {
    double dt, dmax;
    int ok, pad;
};

// The census of the live state (census.inc): per accepted step one int32 row (n_plus, n_minus, w_0 .. w_{L-1}) --
// charged triangles by sign and the winding around every loop.  Triangles and loop sites are in the context's internal
// site numbering.  A device ring of PROBE_RING_STEPS rows rides along in the time loops like the probe ring and is
// flushed with it; the rows of the last tdgl_run collect on the host.  Off (no triangles and no loops): nothing allocated.
struct CensusPlan {  // what the kernels take by value
    int32_t n_tri, nblk_tri, n_loops, ncol;
    const int32_t *elements;  // [3][n_tri]: vertex k of triangle t at k * n_tri + t
    const int8_t *orient;     // [n_tri]
    const int64_t *loop_ptr;  // [n_loops + 1]
    const int32_t *loop_sites;
};
constexpr int CENSUS_MAX_BLOCKS = 1024;  // triangle workgroups of one launch (they stride): bounds the atomics per step at 2 x this
// Records of the cores themselves (tdgl_set_core_records; census.inc, core_records.h): one per charged triangle of every
// recorded step, appended to a pool through a cursor by the census launch.  They belong to the census they were set on.
struct CoresPlan {  // what the recording kernels take by value
    const int32_t *tri_id;            // [n_tri]: the caller's number of the census' triangle k
    const double2 *xy;                // [n]: the sites in the internal numbering
    tdgl_cores::Record *pool;         // [capacity]
    unsigned long long *cursor;       // slots reserved since the last flush
    unsigned long long capacity;
};
struct CoreRecords {
    int64_t capacity = 0, every = 1;  // records per flush window; 0: off
    int64_t window_first = 0;         // running index (accepted steps since the records were switched on) of the ring's row 0
    DevBuf<int32_t> tri_id;
    DevBuf<double2> xy;
    DevBuf<tdgl_cores::Record> pool;
    DevBuf<unsigned long long> cursor;
    PinnedBuf<tdgl_cores::Record> h_pool;
    // of the last tdgl_run, per recorded step: its row among the run's steps, where its records end, whether it is complete
    std::vector<int64_t> step, offset{0};
    std::vector<uint8_t> complete;
    std::vector<tdgl_cores::Record> records;
    bool on() const { return capacity > 0; }
    bool records_index(int64_t index) const { return index % every == 0; }
    CoresPlan plan() const { return {tri_id.p, xy.p, pool.p, cursor.p, (unsigned long long)capacity}; }
};
struct Census {
    int32_t n_tri = 0, n_loops = 0;
    int32_t max_blocks = CENSUS_MAX_BLOCKS;  // (TDGL_CENSUS_MAX_BLOCKS when the census was set: tests of the stride loop)
    CoreRecords cores;
    std::vector<int32_t> tri_order;  // [n_tri]: the caller's number of triangle k of `elements` (what a core record names)
    int64_t serial = 0;  // which tdgl_set_census call made this one (an ensemble that took it over checks it is still the same)
    DevBuf<int32_t> elements, loop_sites, ring;  // ring: [PROBE_RING_STEPS][ncol], counter columns zero between uses
    DevBuf<int8_t> orient;
    DevBuf<int64_t> loop_ptr;
    PinnedBuf<int32_t> h_ring;
    int ring_count = 0;         // rows written since the last flush
    std::vector<int32_t> rows;  // [n][ncol] of the last tdgl_run
    bool on() const { return n_tri > 0 || n_loops > 0; }
    int ncol() const { return 2 + n_loops; }
    CensusPlan plan() const {
        return {n_tri, tri_blocks(), n_loops, ncol(), elements.p, orient.p, loop_ptr.p, loop_sites.p};
    }
    int32_t tri_blocks() const { return std::min((n_tri + BLOCK - 1) / BLOCK, max_blocks); }
    // workgroups of one launch: the triangles', then one wavefront per loop
    unsigned grid() const { return (unsigned)(tri_blocks() + (n_loops + BLOCK / WAVE - 1) / (BLOCK / WAVE)); }
};

// The device arrays of a FieldDrive, one set per context and per replica of an ensemble: the K bases (slot k at 2 m_pad k,
// edge-permuted), the optional A_0, the descriptors with their table pool (all times, then all values), and for loops the
// edge centres, the loops' descriptors and their pool (all times, then all cx, cy, cz, currents)
struct FieldArrays {
    DevBuf<double> bases, a0, tab, centres, loop_tab;
    DevBuf<FieldTerm> terms;
    DevBuf<FieldLoop> loops;
    void take(FieldArrays &o) {
        bases.take(o.bases), a0.take(o.a0), tab.take(o.tab), centres.take(o.centres), loop_tab.take(o.loop_tab);
        terms.take(o.terms), loops.take(o.loops);
    }
};

// One description of a moving applied field, whatever entry point gave it:
//   A(t) = A_0 + f_1(t) A_1 + ... + f_K(t) A_K + sum_l I_l(t) Aloop(r - c_l(t); a_l)
// with K <= FIELD_TERMS_MAX products, an optional static part A_0 and L <= FIELD_LOOPS_MAX moving current loops.  A factor
// is a LinearRamp, a piecewise-linear table, or supplied by the caller step by step (TERM_HOST: tdgl_update_link_scale).
// A single product f(t) A_base (tdgl_set_link_exponents_base, _ramp, _table) is the sum with K = 1 and no A_0; a static A
// under loops is A_0 with K = 0.  The device's arrays (FieldArrays) belong to the drive's owner.  Its functions (loop.inc)
// are the one step rule, the one "has it settled" and the one way in and out of the device's controller.
struct FieldDrive {
    enum Form : int32_t { STATIC, PRODUCT, SUM };  // which entry point described it (the refusals and getters ask)
    Form form = STATIC;
    bool moves = false;     // the time loop evaluates the field before every step
    bool has_dadt = false;  // a dynamic update has run: e_dAdt holds the dA/dt of the links in force
    int n_terms = 0, n_loops = 0;
    bool a0 = false;
    int64_t n_moves = 0;    // steps that moved the field since it was set (tdgl_get_link_term_moves)
    FieldTerm term[FIELD_TERMS_MAX] = {};
    std::vector<double> term_t[FIELD_TERMS_MAX], term_v[FIELD_TERMS_MAX];       // a table term's nodes (the host's copy)
    double scale[FIELD_TERMS_MAX] = {1, 0, 0, 0}, scale_prev[FIELD_TERMS_MAX] = {1, 0, 0, 0};  // factors of the current / previous A
    double zfilm = 0.0, radius[FIELD_LOOPS_MAX] = {0, 0};
    std::vector<double> loop_t[FIELD_LOOPS_MAX], loop_v[FIELD_LOOPS_MAX][4];    // a loop's nodes: centre x, y, z and current
    double loop_par[FIELD_LOOPS_MAX][4] = {}, loop_par_prev[FIELD_LOOPS_MAX][4] = {};  // those four of the current / previous A

    bool product() const { return form == PRODUCT; }
    bool sum() const { return form == SUM; }
    bool loops() const { return n_loops > 0; }
    // static links: no products, no loops, nothing the loop evaluates (the single product's last factor stays readable)
    void clear();
    // the single product f(t) A_base with the caller's factor (tdgl_set_link_exponents_base) ...
    void set_product(double s);
    // ... and where its factor comes from: a ramp, a table (n nodes), or the caller again (TERM_HOST).  The factor in force stays
    void set_product_source(int32_t kind, const double *ramp, const double *times, const double *values, int64_t n);
    // the sum (validated by the caller: check_link_terms); the factors start at their values at t = 0
    void set_terms(int n, bool with_a0, const int32_t *kind, const double *ramp, const int32_t *tab_off, const double *times,
                   const double *values);
    // moving loops on top of the field in force (validated by the caller: tdgl_set_link_loops); the values start at t = 0.
    // n = 0: the loops go
    void set_loops(int n, double z_film, const double *radii, const int32_t *tab_off, const double *times, const double *cx,
                   const double *cy, const double *cz, const double *current);
    double value(int k, double t) const;                    // f_k(t): linear_ramp_value / table_value
    void loop_values(int l, double t, double *out4) const;  // centre x, y, z and current of loop l at t (table_value)
    // the factors and loop values the loop's own evaluation gives at t: s[FIELD_TERMS_MAX], lp[4 FIELD_LOOPS_MAX]
    void values_at(double t, double *s, double *lp) const;
    // The step rule (solver.py:626-642 with the reference's early return): false -- nothing moves, every factor and every loop's
    // four values equal their last two evaluations and a dynamic update has run; true -- the values are taken over (the
    // caller moves the links)
    bool step(const double *s, const double *lp);
    // A LinearRamp (tdgl/sources/scaling.py:4-14) is constant from t_max on, a table from its last node on.  Once the time has
    // passed every term's and every loop's end and every value has been seen twice at its end value -- the first evaluation
    // still sees dA/dt != 0, the second writes dA/dt = 0 (solver.py:626-642) -- the vector potential is static for the rest of
    // the stage: no dA/dt term, no per-step update, and the run-ahead loop can take over.
    bool settled(double time) const;
    void fill(StepCtl &h) const;
    void absorb(const StepCtl &h);
    // the descriptors and the table pool (all times, then all values) as the device reads them; off: where this drive's nodes
    // start in a pool shared with others
    void describe(FieldTerm *desc, std::vector<double> &times, std::vector<double> &values) const;
};

// Tabulated terminal currents (tdgl_set_mu_boundary_table, tdgl_ensemble_set_mu_boundary_table): piecewise-linear densities
// per group of boundary-edge positions, evaluated before every step without a Python round trip -- by the host in the loop with
// one synchronisation per step (step), by k_ra_mu_table / k_ens_mu_table at the device's own time otherwise.  The host walks the
// groups as given (CSR), the device the array groups() makes of them; a replica of an ensemble keeps the nodes only (the
// ensemble's pools are its device copy).  Its functions (drive.inc) are the only writers of its members.
struct MuTable {
    std::vector<double> t, dens;     // nodes; densities [n_groups x n_nodes]
    std::vector<int32_t> ptr, pos;   // groups of boundary-edge positions (CSR-like)
    std::vector<double> last, host;  // the densities the host applied last (NaN: void); the host's mirror of mu_boundary
    bool dev_synced = false;         // b_mu on the device holds `host` at the positions no table covers
    DevBuf<double> d_t, d_dens;      // the device's copy, for the run-ahead loop
    DevBuf<int32_t> d_group;         // [nb]: group of a boundary position, -1 = not tabulated
    bool on_device = false;

    bool on() const { return !t.empty(); }
    bool runs_ahead() const { return !on() || on_device; }  // nothing keeps the run-ahead loop from taking the steps
    void clear();
    // from validated arguments (check_mu_table); nb: the mesh's boundary positions.  The densities and the mirror start at 0
    void set(int32_t n_nodes, const double *times, int32_t n_groups, const int32_t *group_ptr, const int32_t *group_pos,
             const double *density, int64_t nb);
    std::vector<int32_t> groups(int64_t nb) const;  // [nb]: as d_group
    int to_device(tdgl_ctx *ctx);
    bool step(double time);  // the mirror at `time`; true: a density differs from the one applied last (the caller applies the mirror)
    void applied(const double *mu_boundary, int64_t nb);  // the caller's array went to the device (tdgl_set_mu_boundary)
    int handed_to_device(tdgl_ctx *ctx);                  // a run-ahead batch is about to apply densities the host does not see
};

// The separable epsilon(r, t) = factor(t) epsilon0(r) (tdgl_set_epsilon_table, tdgl_ensemble_set_epsilon_table), likewise
struct EpsTable {
    std::vector<double> t, f;
    double last = NAN;      // the factor the host applied last (NaN: void)
    DevBuf<double> eps0;    // the static part, internal site order (a replica's lies in the ensemble's pool)
    DevBuf<double> d_t, d_f;
    bool on_device = false;

    bool on() const { return !t.empty(); }
    bool runs_ahead() const { return !on() || on_device; }
    void clear();
    void set(int32_t n_nodes, const double *times, const double *factor);  // validated: check_eps_table
    int to_device(tdgl_ctx *ctx);
    bool step(double time);  // true: the factor at `time`, now in `last`, differs from the one applied last
    void handed_to_device();
};

// Gaussian hot spots epsilon(r, t) = epsilon0(r) - sum_k a_k(t) exp(-|r - c_k(t)|^2 / (2 sigma_k(t)^2)) (tdgl_set_epsilon_spots,
// tdgl_ensemble_set_epsilon_spots): per spot the centre x, y, the amplitude and the width, each piecewise linear over the spot's
// own nodes.  What the kernels take by value: the four values of every spot, and where the nodes lie in the owner's pool
// (times, then cx, cy, a, sigma, T apart, from base; spot k: nodes off[k] .. off[k + 1])
constexpr int EPS_SPOTS_MAX = 4;
struct EpsSpotValues {
    double v[EPS_SPOTS_MAX][4];  // cx, cy, a, sigma
    int32_t n, pad;
};
struct EpsSpotTabs {
    int32_t off[EPS_SPOTS_MAX + 1];
    int32_t n, T;
    int64_t base;
};
// ... and their one owner, next to EpsTable and likewise: the loop with one synchronisation per step evaluates the tables on
// the host (step) and hands k_eps_spots the values, the run-ahead loop hands it the controller.  A replica of an ensemble
// keeps the nodes only (the ensemble's pools are its device copy).  Its functions (drive.inc) are the only writers of its members.
struct EpsSpots {
    int n_spots = 0;
    std::vector<double> pool;        // the host's nodes: every spot's times, then cx, cy, a, sigma (as the device's pool)
    EpsSpotTabs tabs{};
    double last[EPS_SPOTS_MAX][4];   // the values the host applied last (NaN: void)
    DevBuf<double2> xy;              // site coordinates [n_pad] ...
    DevBuf<double> eps0;             // ... and the static part, internal site order
    DevBuf<double> d_pool;
    DevBuf<EpsSpotValues> d_applied; // what the kernel applied last (read when the host's record is void)
    bool on_device = false;

    EpsSpots() { forget(); }
    bool on() const { return n_spots > 0; }
    bool runs_ahead() const { return !on() || on_device; }
    void clear();
    // from validated arguments (check_eps_spots)
    void set(int32_t n, const int32_t *tab_off, const double *times, const double *cx, const double *cy, const double *amp,
             const double *sigma);
    // the device's copies: the caller's site coordinates [n, 2] and static part [n] through upload_sites' permutation, the
    // nodes, and whether the run-ahead loop (the single GPU's) may evaluate them
    int to_device(tdgl_ctx *ctx, const double *sites, const double *eps0_ref);
    EpsSpotValues values_at(double time) const;
    EpsSpotValues values() const;             // `last` as the kernel takes it
    bool step(double time);                   // true: a value at `time`, now in `last`, differs from the one applied last
    void applied(const EpsSpotValues &sv);    // the caller's values went to the device (tdgl_update_epsilon_spots)
    void handed_to_device() { forget(); }     // a run-ahead batch is about to apply values the host does not see
    void forget();
};

// The time loop's bookkeeping on the host, one per trajectory (tdgl_ctx, every replica of an ensemble): the controller
// (solver.py:316-320, 475-485, 698-707), Runner.dt / time / step (runner.py:260-263, 429-433), the retry state a run-ahead
// batch leaves behind and the moving applied field (FieldDrive).  The classic loop drives it event by event (begin_step,
// retry, accept, advance); the run-ahead and ensemble loops hand it to the device (fill) and take it back (absorb), where
// step_controller applies the same rules.  Its functions (loop.inc) are the only writers of the controller, loop and retry
// members; the field drive is written by the link setters, which own the arrays it describes (finish_links).
struct LoopState {
    tdgl_controller ctl{1e-6, 1e-1, 1, 10, 10, 0.25};
    double tentative_dt = 1e-6, dt_cap = 1e-1, runner_dt = 1e-6, time = 0.0;
    int64_t stage_step = 0;
    std::vector<double> hist;  // d_psi_sq_vals (solver.py:318, 701): only the last `adaptive_window` entries are ever read
    int cur = 0;               // which psi / L psi buffer holds psi^n
    int retries = 0;           // failed attempts of the step in progress (outlives a run-ahead batch) ...
    double attempt_dt = 0.0;   // ... and the dt its next attempt takes
    FieldDrive field;          // the applied field the loop moves, if any
    // what absorb tells its caller about a batch.  corrupt: 1 impossible counts, 2 the records disagree with the controller
    // (the state is void); last_accepted: index of the last accepted record
    struct Batch {
        int corrupt = 0, accepted = 0, failed = 0, last_accepted = -1;
        bool reached = false, error = false;
        double last_fail_dt = 0.0;
    };

    void reset(const tdgl_controller &c);
    void begin_stage() { time = 0.0, stage_step = 0; }  // runner.py:294-295, 315-316
    // restart from a checkpoint (tdgl_set_loop_state, tdgl_set_controller_state)
    void restore(int64_t step, double t, double rdt) { stage_step = step, time = t, runner_dt = rdt; }
    void restore_controller(double tentative, const double *h, int64_t n) { tentative_dt = tentative, retries = 0, hist.assign(h, h + n); }
    void new_state(int buffer) { cur = buffer, retries = 0; }  // a new psi in psi[buffer] (tdgl_set_state): no step is in progress
    std::string budget_message(int replica, double dt) const;
    void report(int64_t *step, double *time_, double *runner_dt_, double *tentative) const;
    // the classic loop's step: its first attempt takes tentative_dt (solver.py:666-668); a step begun by the run-ahead loop and
    // continued here starts its retries over
    double begin_step() { return retries = 0, attempt_dt = tentative_dt; }
    void restart_retries() { retries = 0; }
    bool retry();
    void accept(double dt, double dmax);
    bool advance(double dt, double end_time);
    bool ramp_settled() const { return field.settled(time); }
    bool ramping() const { return field.moves && !ramp_settled(); }
    void fill(tdgl::StepCtl &h, double end_time, bool live) const;
    Batch absorb(const tdgl::StepCtl &h, const tdgl::StepRec *rec, int batch, int limit, bool ramped, double *out_dt);
    void trim() {  // bound the history: only the last `window` entries are ever read
        const int w = ctl.adaptive_window;
        if (ctl.adaptive && w > 0 && (int64_t)hist.size() > 4 * (int64_t)w + 64) hist.erase(hist.begin(), hist.end() - w);
    }
};

// Where the step driver forms J_s, J_n of the step it accepts (tdgl_currents_plan), chosen per step by currents_plan
// (loop.inc) and by nobody else; the run-ahead loop takes the steps of the two plans of the direct solve.
tdgl_currents_plan currents_plan(const tdgl_currents_facts &f);
inline bool currents_plan_runs_ahead(tdgl_currents_plan p) { return p == TDGL_CURRENTS_SPECULATIVE || p == TDGL_CURRENTS_WITH_NEXT_PSI; }

// What js / jn hold, one per context.  FORMED: the currents of psi^n, mu^n with the links in force.  OWED: not formed, but
// the step that owes them left its inputs intact -- the next launch that may take them (or tdgl_run's return) forms them.
// STALE: neither.  Its functions (loop.inc) are the only writers; each says whether its caller has a launch to make.
struct EdgeCurrents {
    enum State : int32_t { STALE, FORMED, OWED };
    State state = STALE;
    bool formed() const { return state == FORMED; }
    bool owed() const { return state == OWED; }
    void new_state() { state = STALE; }  // tdgl_set_state, a replica loaded into the context
    void new_links();
    bool take_with_psi(tdgl_currents_plan plan);
    bool take_behind_look(tdgl_currents_plan plan);
    void speculation_failed();
    bool accept(tdgl_currents_plan plan, bool queued);
    bool request();
    bool flush() { return owed() && request(); }  // tdgl_run returns: what is owed is formed
    static bool batch_attempt_takes(int s, bool owed_on_entry) { return s > 0 || owed_on_entry; }
    void absorb_batch(int done, int last_accepted, int accepted, bool owed_on_entry);
    void screening_done() { state = FORMED; }  // (every screening iteration forms them: step_screening)
};

// Solver choice in the time loop (tdgl_direct_switching; meshes where BOTH a direct solve and the hierarchy are
// resident and large enough for the choice to matter).  A direct solve costs the same whatever the state; AMG-PCG
// started from the projection guess costs next to nothing once the state is stationary (a transport current
// through a strip: 0 iterations) and more than the direct solve while vortices move.  So: direct by default; while
// |psi|^2 has changed by less than PAUSE_DMAX per step for WINDOW steps the direct solve is paused (dense_on() is
// false: classic loop, AMG-PCG); when the iterations' running mean exceeds RESUME_ITERS it comes back, and the next
// pause has to wait twice as long.
// The choice is a function of the run's recent history.  Whatever makes that history meaningless -- a new state, a new
// stage, new boundary values or a new epsilon handed in by the caller -- returns it to its starting point (reset): the
// direct solve, no windows, the short wait.  So a restart from a checkpoint (tdgl_set_state + tdgl_set_loop_state +
// tdgl_set_controller_state) takes the same path whatever came before it.
// Plain host arithmetic, replayed without a device by tdgl_host_solver_choice_replay.  Its functions (loop.inc) are
// the only writers.
struct SolverChoice {
    static constexpr double PAUSE_DMAX = 1e-4;   // max d|psi|^2 per step below which AMG-PCG from the projection guess needs ~1 iteration
    static constexpr int WINDOW = 64;            // ... for this many accepted steps in a row
    static constexpr double RESUME_ITERS = 2.5;  // running mean of the PCG iterations above which the direct solve is the cheaper one again
    // A state that RELAXES smoothly towards a stationary one is extrapolated by the guess window long before it gets there
    // (a strip 300 steps after its current was switched on: 1e-3 per step, 1.5 iterations): three windows in a row, each
    // at least 10 % below the one before and the last below this, pause the direct solve as well
    static constexpr double RELAX_DMAX = 2e-3;
    enum Change : int32_t { NONE, PAUSED, RESUMED };

    void enable(bool yes) { on = yes, reset(); }  // tdgl_direct_switching; off wherever the factors become the CG's preconditioner
    void reset();
    void note_step(double dmax, int pcg_iters);   // a step was accepted
    // in front of a step; allowed: the direct solve is still there to choose (no fall-back, one GPU).  PAUSED: the iterative
    // solve takes over, and its window starts empty -- the caller resets the projection guess
    Change decide(bool allowed);
    bool paused() const { return is_paused; }
    int64_t switches() const { return n_switches; }
    int64_t pause_hold() const { return hold; }

private:
    bool on = false, is_paused = false;
    int64_t switch_steps = 0;         // accepted steps since the last switch
    int64_t hold = 256;               // steps the direct solve runs at least before it may be paused again
    int64_t n_switches = 0;           // (survives reset)
    double recent_dmax[WINDOW] = {0}; // ring of the last accepted steps' max d|psi|^2
    int64_t recent_n = 0;
    double win_max[4] = {0, 0, 0, 0}; // maxima of the last four complete windows, oldest first
    double pcg_ema = 0.0;             // running mean of the iterations while paused
};

// The in-run timers (tdgl_profile_enable / _read / _read_pcg / _read_direct): event pairs around launches inside
// tdgl_run, read out afterwards.  A channel is what one read-out reports; `budget` and `seen` are the state of its
// admission rule (Profile::admit_*).
struct ProfileChannel {
    int64_t launches = 0;
    double ms = 0.0;
    int64_t budget = 0, seen = 0;
    std::vector<std::pair<Event, Event>> pending;  // recorded, not read yet
    void reset(int64_t new_budget) { launches = 0, ms = 0.0, budget = new_budget, seen = 0; }
};
struct Profile {
    bool on = false;
    std::vector<Event> pool;  // created by tdgl_profile_enable, recycled by profile_drain: no hipEventCreate inside a timed region
    ProfileChannel k1;        // K1: L psi' and the right-hand side
    ProfileChannel axp;       // the kernel that dominates the iterative solve (the CG's fused A p), sampled
    // the launch sequence of a direct mu solve, or of one application of the factors as the CG's preconditioner (its own
    // counters, so that a window in which the loop changed the solver does not divide one kind of bytes by the other
    // kind of samples)
    ProfileChannel direct;

    // The admission rules, one per place that brackets launches: the channel the pair goes to, or null (no pair).
    // K1 in the classic loop: every attempt
    ProfileChannel *admit_k1() { return on ? &k1 : nullptr; }
    // K1 in the run-ahead loop: once per batch (event markers between back-to-back launches cost more than the launches
    // they bracket at these sizes)
    ProfileChannel *admit_k1_batch(int attempt) { return on && attempt == 0 ? &k1 : nullptr; }
    // A p: every 8th launch, at most `budget` samples (pairs on every launch would slow a short timed window down measurably)
    ProfileChannel *admit_axp() {
        if (!on || axp.budget <= 0 || (axp.seen++ % 8) != 0) return nullptr;
        axp.budget -= 1;
        return &axp;
    }
    // the factors as the CG's preconditioner: every application of the first 64
    ProfileChannel *admit_factor_apply() { return on && direct.launches + (int64_t)direct.pending.size() < 64 ? &direct : nullptr; }
    // the run-ahead loop's direct solve: once per batch.  Historical: it spends the A p channel's budget (both were one
    // channel once), so a run whose iterative solves used the budget up times no direct solve any more, and the other way
    // round.  The read-outs bench.py reports depend on it; kept as it is.
    ProfileChannel *admit_direct_batch(int attempt) {
        if (!on || attempt != 0 || axp.budget <= 0) return nullptr;
        axp.budget -= 1;
        return &direct;
    }
    void reset(bool enable) { on = enable, k1.reset(0), axp.reset(enable ? 64 : 0), direct.reset(0); }
};
// one admitted pair between its two records (profile.inc: profile_begin / profile_end); ch == null: declined
struct ProfileScope {
    ProfileChannel *ch = nullptr;
    Event a, b;
};

// What the step driver tells a mu solve and hears back from it (pcg_solve, direct_mu_solve); a solve outside the time
// loop passes the default.
struct MuSolveArgs {
    bool mu_halo_pending = false;  // in: leave the exchange of mu's ghosts started, the caller overlaps it and waits
    tdgl_currents_plan plan = TDGL_CURRENTS_ON_REQUEST;  // in: this step's
    bool currents_queued = false;  // out: the solve queued the step's currents behind itself (TDGL_CURRENTS_SPECULATIVE)
    // a direct solve inside a step (in_step) queues them at once where the plan says so
    bool speculate(bool in_step) { return currents_queued = in_step && plan == TDGL_CURRENTS_SPECULATIVE; }
};

struct StepStatus {
    int32_t fail_flag;          // psi update: discriminant < 0 or non-finite somewhere
    int32_t pad;
    unsigned long long dmax_bits[8];  // max | |psi'|^2 - |psi|^2 | as ordered uint64 bits, 8 slots
    double scal[S_COUNT];
    // projection guess, double-double sums (hi at 2 a, lo at 2 a + 1): a = 0: b . b, 1: sum b, 2 + j: y_j . b,
    // 2 + GUESS_MAX + j: y_newest . y_j
    double gdot[2 * (2 * GUESS_MAX + 2)];
};

// Projection guess of the mu solve (popt.extrapolate == 3): window of previous solutions x_j and their images
// y_j = A x_j (= b_j - r_j with the final residual of the CG recurrence), oldest first; G[i][j] = y_i . y_j in
// window order, kept on the host as double-double numbers (hi, lo).  Written by the functions below only (guess.inc).
struct GuessBasis {
    DevBuf<double> x[GUESS_MAX], y[GUESS_MAX];  // by slot; slot[j]: where the window's j-th vector lives
    int slot[GUESS_MAX] = {0};
    int count = 0;
    bool row_pending = false;      // the newest vector's Gram row arrives with the next solve's first status block
    bool mu_first_saved = false;   // mu_prev holds mu^n of a solve that started without a basis (set by pcg_solve)
    double G[GUESS_MAX][GUESS_MAX][2] = {{{0}}};
    double rhs[GUESS_MAX][2] = {{0}};  // y_j . b of the right-hand side being solved
    double bb[2] = {0, 0};             // its (b - mean) . (b - mean)
    DevBuf<double> part_dot;       // 2 (2 GUESS_MAX + 2) x NB partials, see StepStatus::gdot
    DevBuf<double> d_dot;          // their sums
    DevBuf<double> part_dot_rank;  // one process per GPU: every rank's totals (kernels.inc: k_guess_rank_totals)

    void reset() { count = 0, row_pending = false; }  // (a new operator or state: the basis belongs to the previous one)
    int ensure(tdgl_ctx *ctx);
    void take_gram_row(const StepStatus *st);
    void load_rhs(const StepStatus *st, int64_t n_global);
    int solve(double cut, double *c) const;
    double residual_estimate(const double *c) const;
    int next_slot(int window) const;  // where push will put the next solution: a free slot, or the oldest vector's
    int push(int window);
    const double *newest_x() const { return count > 0 ? x[slot[count - 1]].p : nullptr; }

private:
    void drop_oldest(int drop);
};

// One level of the nested-dissection factors (dense.inc: sub_upload_level; include/tdgl_hip.h: tdgl_substructure).  The
// first level works on the site vector (or a rank's interior), every further one on the previous level's separator.
struct SubLevel {
    int32_t parts = 0;
    int64_t nI = 0, nS = 0;                // interior rows / separator rows; nI + nS = the length of the level's vector
    DevBuf<int32_t> part_ptr, seg_ptr, seg_x, seg_len, sep_ptr, sep_idx, row_part;
    DevBuf<int64_t> seg_val, g_off;
    DevBuf<double> vals, u;
    DevBuf<float> vals32;                  // the pool in fp32 (the preconditioner's storage; `vals` released)
    DevBuf<SubUpChunk> up_chunks;
    DevBuf<SubDownChunk> down_chunks;
    DevBuf<SubDownRow> down_rows;
    DevBuf<double> w;                      // [nI + nS + parts] result of the way down
    DevBuf<double> xs;                     // [nS] separator solution
    Csr coupling;                          // (optional) A_SI [nS x nI]: r_S = r_S - coupling y_I behind the way down
    int sym_lds = 0;                       // rows of b_p k_sub_down_sym stages (0: whole blocks)
    int up_R = 1;                          // chunks of 64 rows a workgroup of the way up takes (a whole part where > 1)
    bool ident = false;                    // the separator rows are their identity segment alone (out = b)
    bool need_coupling = false;            // described without its -E^T rows: the coupling block must follow
};

// a symmetric matrix as its tiles on or below the diagonal (kernels.inc: k_dense_sym_tiles)
struct DenseTiles {
    DevBuf<double> G;
    DevBuf<float> G32;                     // (fp32 storage: G released)
    DevBuf<double> part;                   // per-tile contributions of k_dense_sym_tiles [tiles][tiles * DT]
    int tiles = 0;                         // tiles per side
    int64_t n = 0;                         // order of the matrix
};

// the preconditioner's top separator in block low-rank form (dense.inc: dense_to_blr; kernels.inc: k_blr_project /
// k_blr_finish).  ndense == 0: not in use (the dense fp32 tiles of DirectFactors::dense are)
struct BlrTop {
    DevBuf<float> Gd;                      // [ndense][DT * DT] the tiles kept dense (the diagonal, the blocks that do not pay)
    DevBuf<int32_t> dense_ij;              // [ndense] I << 16 | J
    DevBuf<float> F;                       // the low-rank columns of every row block
    DevBuf<int64_t> colbase;               // [tiles + 1]
    DevBuf<int32_t> twin;                  // [cols]
    DevBuf<int32_t> items;                 // [nitems][4] BlrItem
    DevBuf<double> coef;                   // [cols]
    DevBuf<int32_t> dslot_ptr, dslot;      // the dense slots of each row block
    int ndense = 0, nitems = 0;
    int64_t cols = 0;                      // columns (padded), summed over the row blocks
    int64_t pairs = 0;                     // tile pairs stored as factors
    int64_t bytes = 0;                     // what one application streams (each column twice: projection and way back)
    int64_t dense_bytes = 0;               // the same with every tile dense (k_dense_sym_tiles)
    int64_t rank_max = 0;
    double tol = 0.0, norm = 0.0;          // truncation tau, ||G||_2 estimate
};

// Everything a direct mu solve owns (dense.inc, schur.inc): the dense inverse of the whole matrix, or the levels of a
// nested dissection with the dense pseudo-inverse of the last level's separator; as the CG's preconditioner also the
// dissection map and its work vectors; in one-process-per-GPU mode the rank-level interface.  tdgl_ctx::direct holds it,
// and releasing it is a reset of that pointer.  Every set-up entry point checks its input before it touches the object
// and builds into a new object or a new level, which it moves in only once complete.
struct DirectFactors {
    enum Stage {
        SCHUR_BEGUN,       // tdgl_poisson_schur_begin: the interface is in place, the interior's levels are not
        INNER_PENDING,     // the first level came without a Schur complement: inner levels until one carries it
        COUPLING_PENDING,  // every level is there, some coupling block is not
        READY,             // a complete direct solve (one GPU), or the interior's factors (between schur_begin and _finish)
        PRECOND,           // the factors precondition the CG (tdgl_poisson_set_substructure_precond / _schur_finish)
    };
    Stage stage = READY;
    DenseTiles dense;                      // pinv of the whole matrix (levels == 0), or of the last level's separator
    int64_t ld = 0;                        // > 0: `dense` is the inverse of the whole matrix (tdgl_poisson_set_dense_inverse)
    // nested dissection
    SubLevel lv[SUB_LEVELS_MAX];
    int levels = 0;                        // levels described so far
    int nfin = 0;                          // workgroups of the separator's k_dense_sym_finish
    DevBuf<double> upart;                  // their partials of u . x_S
    DevBuf<double> mean;                   // [1] several levels: the mean of the solution, left for the first level's way up
    BlrTop blr;                            // (preconditioner, fp32) the top separator in block low-rank form
    bool fp32 = false;                     // the pools and the dense tiles are stored in fp32
    // the preconditioner's application in the dissection order: map[i] = the context's index of dissection position i
    DevBuf<int32_t> map;
    // gathered residual / solution in dissection order (the rank-level dissection, and one GPU with TDGL_PD_TWO_PASS: the
    // folded application needs neither) / z in the context's order
    DevBuf<double> bp, xp, z;
    // rank-level dissection (schur.inc): the levels are those of this rank's interior block A_II (n_local sites,
    // positive definite: plain inverse of the top separator, no gauge), Gamma = the interface between the ranks
    int64_t n_local = 0;                   // > 0: rank-level dissection
    int64_t ng = 0, ngo = 0;
    DevBuf<int32_t> owner_local;           // [ng] local index of the Gamma site if this rank owns it, else -1
    DevBuf<int32_t> go_local, go_gid;      // [ngo] owned Gamma sites: local index, position in Gamma
    Csr GI, IG;                            // A_GI [ng x n_I], A_IG [n_I x ng] (columns / rows in the local dissection order)
    DenseTiles S;                          // pinv of the interface complement, the same on every rank
    DevBuf<double> t, rg, xg, y, v, c;     // [ng] x 3, [n_I] x 3

    bool in_schur_setup() const { return n_local > 0 && stage != PRECOND; }
    // the stage a complete set of levels has reached
    Stage settled() const {
        for (int k = 0; k < levels; ++k)
            if (lv[k].need_coupling) return COUPLING_PENDING;
        return READY;
    }
};

struct ScrTree;  // the screening treecode's set-up (screening_tree.inc)

}  // namespace tdgl

struct IpcState;  // peer-mapped transport (ipc.inc)

// Members are destroyed in the reverse order of their declaration: the stream comes first here so that it goes last,
// behind every device buffer, pinned block, event and the communication stream (tdgl_destroy synchronises it, tears down
// RCCL and the peer-mapped transport, and deletes the context).  Every owning member is empty until create_impl fills it,
// so a half-built context is destroyed the same way.
struct tdgl_ctx {
    int device = 0;
    tdgl::Stream stream;
    std::string err;

    int64_t n = 0, m = 0, nb = 0, n_pad = 0, m_pad = 0;
    int64_t n_own = 0;     // rows this rank computes (sites [n_own, n) are ghost copies)
    int64_t n_global = 0;  // sites over all ranks
    double u = 5.79, gamma = 10.0;

    // ---- one-process-per-GPU mode (comm.inc) -----------------------------------------
    int rank = 0, world = 1;
    ncclComm_t comm = nullptr;
    tdgl_halo_fn cb_halo = nullptr;
    tdgl_allreduce_fn cb_allreduce = nullptr;
    void *cb_user = nullptr;
    std::vector<int32_t> nbr_ranks, send_ptr, recv_ptr;
    tdgl::DevBuf<int32_t> d_send_idx;
    tdgl::DevBuf<double> d_sendbuf, d_gstat;
    tdgl::DevBuf<float> d_red32;          // fp32 staging of the coarse right-hand side all-reduce
    tdgl::PinnedBuf<double> h_sendbuf, h_recvbuf;  // (callback transport; both of h_sendbuf.n doubles)
    bool fix_psi = true;
    // halo exchange overlapped with the ghost-free rows (comm.inc): second stream + events
    tdgl::Stream comm_stream;
    tdgl::Event ev_pack, ev_halo;
    int int_tiles = 0;        // leading 256-row tiles whose rows have no ghost neighbour
    int64_t m_int = 0;        // leading edges (internal order) between two owned sites
    int overlap = 1;          // tdgl_set_comm_overlap: 0 off, 1 auto (by size), 2 always
    int64_t stat_halos = 0, stat_halo_bytes = 0, stat_allreduces = 0, stat_allreduce_bytes = 0;
    double *pend_v = nullptr; // exchange started by comm_halo_start, completed by comm_halo_wait
    int pend_width = 0;
    IpcState *ipc = nullptr;  // peer-mapped transport (tdgl_comm_init_ipc)
    // two distributed AMG levels (tdgl_set_deep_halo_plan): the exchange of r on the whole ghost zone
    bool deep = false;
    int64_t n_ext = 0;        // owned + every ghost layer (length of the PCG's level-0 vectors)
    int64_t l1_interior = 0;  // leading level-1 rows whose restriction reads owned fine entries only
    std::vector<int32_t> deep_nbrs, deep_send_ptr, deep_recv_ptr;
    tdgl::DevBuf<int32_t> d_deep_send_idx, d_deep_recv_idx;
    tdgl::DevBuf<double> d_deep_sendbuf, d_deep_recvbuf;
    tdgl::PinnedBuf<double> h_deep_send, h_deep_recv;  // (callback transport)
    int64_t stat_deep_halos = 0;

    // permutations (host)
    std::vector<int32_t> perm, iperm;            // internal -> reference site, and inverse
    std::vector<int32_t> edge_perm, edge_iperm;  // internal -> reference edge, and inverse

    // ---- psi operators -------------------------------------------------------------
    tdgl::SellPattern lap_pat;            // off-diagonal pattern of the site graph
    tdgl::DevBuf<double2> lap_vals;       // (w_e / a_i) * U_ij, per slot
    tdgl::DevBuf<double> lap_slot_w;      // w_e / a_i per slot (static)
    tdgl::DevBuf<int32_t> lap_slot_edge;  // (internal edge << 1) | conj flag, -1 = padding
    tdgl::DevBuf<double> lap_diag;        // -sum_j w_ij / a_i
    tdgl::DevBuf<uint8_t> fixed_mask;     // 1 = identity row (terminal site with fix_psi)
    tdgl::DevBuf<double> area;            // a_i (0 on padding rows)
    // per edge (internal order, reference orientation)
    tdgl::DevBuf<int32_t> e0, e1;
    tdgl::DevBuf<double> e_inv_len, e_dirx, e_diry;
    tdgl::DevBuf<double2> e_U;
    tdgl::DevBuf<double> e_A, e_Aprev;    // link exponents now / at the previous step [2 * m_pad]
    tdgl::DevBuf<double> e_dAdt;          // dA/dt along the edges (time-dependent A: loop.field.has_dadt), else unused
    tdgl::DevBuf<int32_t> link_block_changed, link_changed;  // allclose(new_A, old_A) test (k_dadt)
    tdgl::FieldArrays field;              // the device arrays of loop.field (tdgl_set_link_exponents_base, _terms, _loops)
    // piecewise-linear time tables evaluated by tdgl_run itself before every step (drive.inc)
    tdgl::MuTable mu_tab;
    tdgl::EpsTable eps_tab;
    tdgl::EpsSpots eps_spots;
    // boundary term: c = mu_boundary_laplacian @ mu_boundary
    tdgl::DevBuf<int32_t> b_s0, b_s1;
    tdgl::DevBuf<int32_t> d_b_sites;      // the sites that boundary edges touch, each once (ensure_boundary_sites)
    int32_t n_b_sites = 0;
    tdgl::DevBuf<double> b_c0, b_c1, b_mu;
    tdgl::DevBuf<double> cvec;            // boundary part
    tdgl::DevBuf<double> ceff;            // cvec + divergence(dA/dt): what the rhs kernel reads

    // ---- state ---------------------------------------------------------------------
    tdgl::DevBuf<double2> psi[2];         // psi[loop.cur] is psi^n
    tdgl::DevBuf<double2> lap[2];         // lap[loop.cur] = L_psi psi^n (cached between steps)
    bool lap_valid = false;
    tdgl::DevBuf<double> mu, eps, bvec;
    tdgl::DevBuf<double> js, jn;          // per edge, internal order
    tdgl::EdgeCurrents currents;          // what js / jn hold (loop.inc)
    bool have_links = false, have_state = false, have_eps = false;

    // ---- Poisson ---------------------------------------------------------------------
    std::vector<tdgl::AmgLevel *> levels;
    tdgl::Csr fusedR;                     // R0 (I - c A0 D0^-1): restriction of the pre-smoothed residual
    double fusedR_c = 0.0;                // the smoothing coefficient it was built for
    tdgl::DevBuf<float> fusedR32;         // its values in fp32
    tdgl::DevBuf<tdgl::half_t> fusedR16;  // ... in binary16
    bool level0_f16 = false;              // the level-0 V-cycle kernels read the binary16 copies
    tdgl::StoredForm form_A = tdgl::StoredForm::F32_I32, form_P = form_A, form_R = form_A;  // ... each operator's form (ensure_f32)
    double level0_absmax = 0.0;           // largest |entry| of A0, P0 and the fused restriction (binary16 range check)
    tdgl::DevBuf<uint16_t> fusedR_off16;  // its columns as 16-bit offsets from fusedR_base[row], when they fit
    tdgl::DevBuf<int32_t> fusedR_base;
    bool f32_ready = false;               // fp32 copies are current
    bool coarse32_ready = false;          // ... of the intermediate-level operators
    int64_t pcg_epoch = 0;                // bumped whenever an operator of the solve is replaced
    int64_t f32_fallbacks = 0;            // solves that had to be finished with the fp64 operators
    tdgl::DevBuf<double> coarse_pinv;
    int64_t n_coarsest = 0;
    // direct mu solve (tdgl_poisson_set_dense_inverse / _build_dense_inverse / _set_substructure* / _schur_*): null = AMG-PCG
    std::unique_ptr<tdgl::DirectFactors> direct;
    int32_t pd_choice = 0;                // 0: by predicted cost, 1: always the factors, 2: never (AMG V-cycle)
    double pd_rate = 4.5;                 // decades per iteration observed with the factors as preconditioner (running mean)
    double pd_t_apply_us = 0.0, pd_t_vcycle_us = 0.0;  // measured at set-up: one application of either preconditioner
    int64_t pd_solves = 0, pd_iters = 0, pd_amg_solves = 0, pd_amg_iters = 0;  // solves / iterations by preconditioner since the last reset
    bool pd_last = false;                 // the last solve used the factors
    int64_t pd_handovers = 0;             // solves that began with the factors and were finished by the V-cycle
    tdgl::SolverChoice choice;            // direct or iterative, step by step (tdgl_direct_switching; loop.inc)
    // run-ahead time loop (direct solves, static links): device-resident controller + per-step records
    tdgl::DevBuf<tdgl::StepCtl> d_ctl;
    tdgl::DevBuf<tdgl::StepRec> d_rec;
    tdgl::PinnedBuf<tdgl::StepCtl> h_ctl;  // [1]
    tdgl::PinnedBuf<tdgl::StepRec> h_rec;  // [RA_BATCH_MAX]
    int ra_batch = 4;                     // attempts queued per synchronisation: doubles up to RA_BATCH_MAX
    bool run_ahead_disabled = false;      // TDGL_NO_RUN_AHEAD, read once when the context is created (tests, A/B runs)
    int64_t stat_ra_batches = 0, stat_ra_dead = 0;
    // Work queued behind a status copy while the host waits for it (poisson.inc: sync_status).  TDGL_NO_SYNC_SHADOW,
    // read once when the context is created, restores the order without it (tests, A/B runs).
    bool sync_shadow_disabled = false;
    // The factor preconditioner as gather, sequence, scatter (factors.inc: precond_direct_apply).  TDGL_PD_TWO_PASS, read
    // once when the context is created, restores that order (tests, A/B runs); the counters say which one ran.
    bool pd_two_pass = false;
    int64_t pd_applies_folded = 0, pd_applies_two_pass = 0;
    tdgl::Event ev_status;                // recorded right behind the status copy: the host waits for it, not for the stream
    int64_t stat_edge_launches = 0;       // formations of J_s / J_n since the last reset (tdgl_get_edge_current_launches)
    // collapsed coarse chain (tdgl_poisson_set_collapsed_tail): everything from level `tail_level`
    // down as explicit operators, built for the smoother settings (tail_nu, tail_smoother, tail_cheb_lo)
    int tail_level = -1;                  // -1: off
    int tail_mode = 0;                    // 0: e = B b (dense [n_t, n_t]);  1: y = G b, e = W b + V y
    int64_t tail_g_rows = 0;              // rows of G
    int64_t tail_v_cols = 0;              // columns of the dense V (leading entries of G b)
    int64_t tail_ldg = 0, tail_ldv = 0;   // leading dimensions of G / V (padded to 4 entries)
    tdgl::DevBuf<double> tailG, tailV;    // dense row-major (mode 0: tailG holds B)
    tdgl::DevBuf<float> tailG32, tailV32;
    tdgl::Csr tailW;
    tdgl::DevBuf<uint16_t> tailW_idx16;   // its column indices in 16 bits (the tail level has < 65536 rows)
    int tail_nu = 0, tail_smoother = 0;
    double tail_cheb_lo = 0.0;
    tdgl::DevBuf<double> pcg_r, pcg_p, pcg_q;
    tdgl::DevBuf<double> pcg_p2;          // second direction buffer (fused direction update, k_sell_axp)
    // Per-workgroup partials of the dot products: arrays of stride NB of which the first `npart` entries
    // are written and summed -- the number of 256-row tiles rounded up to a multiple of 8, at most NB
    // (NB itself in one-process-per-GPU mode, where the arrays are summed over ranks of different sizes)
    int npart = 1024;
    tdgl::DevBuf<double> part_pair[2];    // 2 x NB partials each: [r.z | ||r||^2], ping-pong
    tdgl::DevBuf<double> part_pq, part_tmp;  // NB per-workgroup partials each
    tdgl::DevBuf<double> scal;            // tdgl::Scal (numbers the host reads)
    tdgl::DevBuf<double> mu_prev, mu_prev2;  // mu^{n-1}, mu^{n-2} for the extrapolated initial guess
    double prev_dt = 0.0, prev_dt2 = 0.0;    // dt of the steps that produced mu / mu_prev (0: no history)
    tdgl_poisson_options popt{1e-10, 500, 2, 0, 1, 1, 0.1, 3, 1, 2, 0, 0};
    tdgl::GuessBasis guess;               // projection guess (popt.extrapolate == 3)
    // in-loop guard of the direct mu solves (factors.inc: direct_guard_*): ||b - A mu|| / ||b|| of an accepted step,
    // measured with the resident level-0 matrix once per run-ahead batch / every DIRECT_GUARD_EVERY classic steps
    double direct_relres_max = 0.0;
    int64_t direct_checks = 0;
    int32_t direct_fell_back = 0;         // a check exceeded direct_guard_limit: the factors were released, AMG-PCG took over
    int32_t direct_guard_countdown = 0;
    double direct_guard_limit = 1e-9;
    int32_t last_guess_vectors = 0;       // basis size the last guess was formed from
    double last_guess_relres = 0.0;
    int32_t last_pcg_iters = 0;
    double last_relres = 0.0;
    // how many iterations the first batch of a solve queues before the host looks (pcg_solve): predicted from the
    // guess's residual, which the host knows from the Gram data, and the running contraction per iteration
    double pcg_rate = 0.6;                // decades of ||r|| per iteration (running mean of the observed ones)
    int32_t pcg_predict_from_guess = 1;   // 0: the previous solve's count (TDGL_PCG_PREDICT=last)
    int64_t stat_pcg_launched = 0;        // iterations queued, frozen ones included
    int64_t stat_pcg_needed = 0;          // iterations up to convergence
    int64_t stat_pcg_extra_syncs = 0;     // host looks after the first batch of a solve

    // ---- step status / probes --------------------------------------------------------
    tdgl::DevBuf<double> psi_dmax_part;    // per-workgroup max d|psi|^2 of the last k_psi_update
    tdgl::DevBuf<int32_t> psi_fail_part;   // per-workgroup failure flags
    int psi_blocks = 0;                    // its grid
    bool psi_status_pending = false;       // not yet reduced into d_status
    tdgl::DevBuf<tdgl::StepStatus> d_status;
    tdgl::PinnedBuf<tdgl::StepStatus> h_status;  // [1]: d_status is copied here at every host synchronisation
    tdgl::StepStatus *status_dev = nullptr;  // what the kernels write (= d_status.p)
    std::vector<int32_t> probes;           // internal site ids
    tdgl::DevBuf<int32_t> d_probes;
    tdgl::DevBuf<double> d_probe_out;      // ring buffer [PROBE_RING_STEPS][2 * n_probe]: mu | theta per step
    tdgl::PinnedBuf<double> h_probe_out;   // the same shape
    int probe_ring_count = 0;              // steps written since the last flush (run.inc: probe_ring_flush)
    tdgl::Census census;                   // vortex counts and loop windings per accepted step (census.inc), flushed with the probes

    tdgl::LoopState loop;                  // controller, Runner.dt / time / step, retry and ramp state (loop.inc)
    // counters since the last reset (tdgl_get_step_stats): steps accepted, failed psi updates that were
    // repeated with a smaller dt, PCG iterations, host synchronisations inside tdgl_run
    int64_t stat_steps = 0, stat_psi_retries = 0, stat_pcg_iters = 0, stat_host_syncs = 0;
    int64_t stat_wait_ns = 0, stat_run_ns = 0;  // host time blocked in those synchronisations / inside tdgl_run

    // ---- screening (screening.inc) -------------------------------------------------------
    bool scr_enabled = false;
    tdgl_screening_options scr{1000, 1e-3, 0.1, 0.5};
    tdgl::DevBuf<double> scr_site_xyw;   // per site: x, y, scaled area  [3 * n_pad]
    tdgl::DevBuf<double> scr_edge_xy;    // per edge (internal order): x, y  [2 * m_pad]
    tdgl::DevBuf<double> scr_inv_2deg;   // 1 / (2 * number of incident edges)  [n_pad]
    tdgl::DevBuf<double> scr_Jsite;      // site-averaged K = J_s + J_n  [2 * n_pad]
    tdgl::DevBuf<double> scr_Aind, scr_vel;  // [2 * m_pad], internal edge order
    tdgl::DevBuf<double> scr_Anew;           // [scr_chunks][2 * m_pad] partial sums over site chunks
    int scr_chunks = 1, scr_tiles_per_chunk = 1;
    tdgl::DevBuf<double> abs_sq_old;     // |psi^n|^2 of the step's starting psi [n_pad]
    tdgl::DevBuf<unsigned long long> scr_err_bits;
    // one-process-per-GPU mode: the 1/r sum runs over ALL sites; every rank scatters the site
    // currents of its owned sites into a global array that is summed over ranks
    int64_t scr_n_sites = 0;             // sites the kernel sums over (n, or n_global)
    tdgl::DevBuf<int64_t> scr_owned_gid; // global id of each owned site
    tdgl::DevBuf<double> scr_Jglobal;    // [2 * n_global_pad]
    int32_t last_screening_iters = 0;
    // the barycentric Lagrange treecode (screening_tree.inc, tdgl_set_screening_tree); null: the all-pairs kernel
    std::shared_ptr<tdgl::ScrTree> scr_tree;

    // ---- measurement -------------------------------------------------------------------
    tdgl::Event ev0, ev1;                  // tdgl_time_kernel's pair
    tdgl::Profile prof;                    // the in-run timers (profile.inc)
};
