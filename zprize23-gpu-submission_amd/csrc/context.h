// context.h — the per-GPU context behind the C-ABI (replaces the reference's
// per-op SyncedMemory allocation, lib/caffe/syncedmem.cpp): one stream, the
// NTT tables, MSM work buffers, a scratch pool and the HBM-resident keys.
#pragma once
#include "pnp_internal.h"
#include "prover_key.h"
#include <array>
#include <atomic>
#include <chrono>
#include <memory>
#include <thread>

struct pnp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // low-priority side stream for challenge-independent work overlapped with
    // the MSMs (prover.cpp), created on first use, and its events
    hipStream_t stream_lo = nullptr;
    hipEvent_t ev_fork = nullptr, ev_w8 = nullptr, ev_z8 = nullptr;
    hipStream_t side_stream();
    pnp::NttTables ntt;
    pnp::MsmWork msm;
    pnp::DevBuf scratch_a, scratch_b;
    // pinned staging of the host -> HBM uploads (context.cpp h2d_batch): per copy
    // thread two chunks, a stream and an event per chunk; made on first use
    static constexpr int kStgThreads = 6;
    void *stg_buf[2 * kStgThreads] = {};
    hipStream_t stg_st[kStgThreads] = {};
    hipEvent_t stg_ev[2 * kStgThreads] = {};

    // ---- resident prover key and its wire map (prover_key.h) ----
    pnp::ResidentKey key;
    // ---- resident commit key ----
    bool ck_loaded = false;
    uint64_t ck_points = 0;
    pnp::DevBuf ck_owned;
    const uint64_t *ck_dev = nullptr;
    // device-pointer loads: the content hash of the SRS the derived tables
    // (folded tables, Lagrange basis, groups) were built from — a reload of
    // the same bytes keeps them
    uint64_t ck_hash[2] = {0, 0};
    bool ck_hash_valid = false;
    // folded MSM table of the first ck_table_n SRS points (msm_build_table),
    // built on the first commitment of that size
    pnp::DevBuf ck_table;
    uint64_t ck_table_n = 0, ck_table_p0 = 0, ck_table_p1 = 0;
    // the first lag_n SRS points in the Lagrange basis of the order-lag_n
    // subgroup (srs_lagrange, affine) and their folded table: witness
    // polynomials are committed from their evaluations (lagrange.hip); built
    // on the first commitment of that size; lag_ok = false: degenerate key
    pnp::DevBuf lag_points, lag_table;
    uint64_t lag_n = 0, lag_table_n = 0, lag_table_p0 = 0, lag_table_p1 = 0;
    bool lag_ok = false;
    // wire commitments over copy-constraint groups (wires.hip): the rows of
    // one wire that hold one variable (a cycle of sigma restricted to the
    // wire) share the base sum_i L_i, so a wire commits with one scalar per
    // group; built from sigma and the Lagrange points on the first proof that
    // needs them, kept while both are unchanged
    // Index 4 is z (round 3): its groups are the runs of rows sigma fixes
    // (the padding rows: z is constant there).
    struct WireBases {
        bool built = false, ok = false, wires_ok = false, z_ok = false;
        bool sliced = false;            // the table holds this rank's point range of each segment
        int c = 0;                      // its window bits (msm_fold_c of one segment's n)
        uint64_t n = 0, total = 0, m = 0, len = 0;  // domain, bases, largest group count, MSM length
        uint64_t g[5] = {}, off[5] = {};
        // what the build found per segment, for the counters (wires.hip
        // credit_group_counts): groups before an ungrouped wire takes its n
        // slots, and groups queued for a workgroup of their own
        uint64_t found[5] = {}, heavy[5] = {};
        bool ident[5] = {};             // ungrouped wire: its scalars are its evaluations
        pnp::DevBuf grp[5], rep[5];     // row -> group slot, slot -> representative row
        pnp::DevBuf scal[5];            // per-proof group scalars at their slots (n each)
        pnp::DevBuf table;              // folded table over the `total` bases
        pnp::DevBuf sigma;              // the sigma evaluations the groups came from
        pnp::DevBuf flag;
        uint64_t pk_gen = 0;            // prover-key load the sigma check last covered
    } wb;
    // the key-load HBM budget (pnp_load_prover_key) left no room for these
    // optional tables: the prover commits without them (same proof bytes)
    // (atomic: the background builder's failure paths set them while a proof
    // on the owning thread may read them; such a proof finds the build busy and
    // commits without the tables whatever it reads)
    std::atomic<bool> hbm_lag_off{false}, hbm_groups_off{false};
    bool hbm_checked = false;  // the budget of the loaded keys has been checked (first proof)
    // Deferred tables: the context's first proof commits without the
    // optional tables it would have to build first (Lagrange basis, copy
    // groups: ~3.4 s at 2^22), so a caller that proves once per process pays
    // its upload and proof only; same proof bytes either way.  On one GPU the
    // tables are then built in the background (bg_*: a thread on a
    // lowest-priority stream, one kernel in flight at a time) while the caller
    // goes on, and the first proof after the build finished uses them; with
    // several ranks the next proof builds them (the builds exchange status
    // with the peers).  PNP_DEFER_TABLES=1 / 0 forces it on / off; default:
    // on at world 1.  Once per context, so a caller reloading its keys every
    // call (PNP_V1_RELOAD) still gets the tables from then on
    int defer_tables = -1;   // -1: the default for the world size (resolved by the first proof)
    bool defer_now = false;  // this proof defers (set per proof)
    bool tables_wanted = false;  // this deferring proof found a table missing
    uint64_t proofs_started = 0;
    std::thread bg;
    std::atomic<int> bg_state{0};  // 0 idle, 1 building, 2 finished (not yet joined)
    std::atomic<bool> bg_cancel{false};
    hipStream_t bg_stream = nullptr;

    // ---- per-proof working set (sized on first use, reused) ----
    std::map<std::string, pnp::DevBuf> work;
    uint64_t *buf(const std::string &name, size_t elems_fr);

    pnp::KernelTimer ktimer;

    // ---- stage timing of the last proof ----
    std::vector<std::pair<std::string, double>> stages;
};

namespace pnp {
// bytes a proof at domain n still has to allocate on this rank (context.cpp)
struct HbmPlan {
    uint64_t mandatory = 0;  // per-proof buffers, NTT tables, commit-key table, MSM work
    uint64_t lag = 0;        // the Lagrange-basis key and its folded table (optional)
    uint64_t groups = 0;     // the copy-constraint groups and their table (optional)
    uint64_t transient = 0;  // the largest build scratch on top of them (max of the three below)
    uint64_t t_mand = 0, t_lag = 0, t_groups = 0;  // build scratch of the commit-key table, Lagrange, groups
};
HbmPlan hbm_plan(pnp_ctx *ctx, uint64_t n);
// multi-GPU: AND of every rank's `mine` (one tagged all-gather); world 1: mine
bool all_ranks_ok(pnp_ctx *ctx, bool mine);
bool lagrange_enabled();
// the HBM budget of the loaded keys, checked by the first proof (sets
// hbm_lag_off / hbm_groups_off, or throws PNP_E_NOMEM)
void hbm_budget(pnp_ctx *ctx);
bool wire_groups_enabled();
Fr root_of_unity(uint32_t lg);
Fr fr_from_u64(uint64_t x);
// drop everything derived from the resident SRS (folded tables, Lagrange basis)
void ck_derived_reset(pnp_ctx *ctx);
// commitments over the resident SRS (folded MSM)
const uint64_t *commit_table(pnp_ctx *ctx, uint64_t n);
// host -> HBM copies of caller buffers (pageable memory) through pinned
// staging chunks, several copy threads at once; returns when they have landed
struct H2D {
    void *dst;
    const void *src;
    size_t bytes;
};
void h2d_batch(pnp_ctx *ctx, const std::vector<H2D> &copies);
// device bytes held by every DevBuf of the process, now and at most (pnp_hbm_usage)
extern std::atomic<uint64_t> g_dev_live, g_dev_peak;
// (PNP_HIDDEN, pnp_internal.h: shared between the library's units only)
// free the staging pool (pnp_ctx_destroy)
PNP_HIDDEN void h2d_release(pnp_ctx *ctx);
// this thread's last error message (set_error writes it, pnp_last_error returns it)
PNP_HIDDEN const char *last_error();
// the end of every commitment: B XYZZ sums (24 words each) to affine on the
// host, x and y into out[b]
PNP_HIDDEN void store_affine(const uint64_t *xyzz, int B, CommitmentC *const *out);
// the folded table of the Lagrange-basis SRS of size n (this rank's point
// range), nullptr when it is unavailable (PNP_LAGRANGE=0, n not a power of
// two or above the key, degenerate key)
const uint64_t *lagrange_table(pnp_ctx *ctx, uint64_t n);
// B commitments of polynomials given by their n evaluations on the order-n
// subgroup (Montgomery Fr, natural order): sum_i e_i L_i; requires
// lagrange_table(ctx, n) != nullptr
void commit_evals_batch(pnp_ctx *ctx, const uint64_t *const *d_evals, int B, uint64_t n, CommitmentC *const *out);
void commit_affine(pnp_ctx *ctx, const uint64_t *d_scalars, uint64_t n, CommitmentC *out);
// the four wire commitments from their n padded evaluations over the
// copy-constraint-grouped bases (wires.hip); false (nothing written) when the
// groups are unavailable or the witness differs inside a group, and the caller
// commits with commit_evals_batch
bool commit_wires_grouped(pnp_ctx *ctx, const uint64_t *const *d_evals, uint64_t n, CommitmentC *const *out);
// z (round 3) from its n evaluations over its groups, the runs of rows sigma
// fixes (wires.hip); false when unavailable (the caller commits row by row)
bool commit_z_grouped(pnp_ctx *ctx, const uint64_t *d_z, uint64_t n, CommitmentC *out);
// drop the wire groups (a new commit key or Lagrange basis)
void wire_bases_reset(pnp_ctx *ctx);
// build the copy-constraint groups now if they are enabled and missing
// (wires.hip; the background table build)
void wire_bases_build(pnp_ctx *ctx, uint64_t n);
// ---- the background table build (context.cpp; see pnp_ctx::bg) ----
// start it after a deferring proof (world 1)
void tables_start_background(pnp_ctx *ctx, uint64_t n);
// PNP_DEFER_BG (default on): world-1 deferral builds in the background
bool tables_bg_enabled();
// true while it runs (joins it once it has finished); a proof then goes
// without the tables.  Always false on the builder's own thread
bool tables_busy(pnp_ctx *ctx);
// wait for it (pnp_sync, key loads, operator calls that need the tables)
void tables_wait(pnp_ctx *ctx);
// stop it at its next kernel and wait (context destruction, process exit)
void tables_cancel(pnp_ctx *ctx);
// the stream the table builds run on: the background stream on the builder's
// thread, else the context stream
hipStream_t tables_stream(pnp_ctx *ctx);
// B commitments over the resident SRS in one batched MSM
// local: on a multi-GPU run the scalars hold only this rank's point range
void commit_affine_batch(pnp_ctx *ctx, const uint64_t *const *d_scalars, int B, uint64_t n,
                         CommitmentC *const *out, bool local = false);
// v2 options of pnp_prove_ex: public inputs (positions, canonical values) and
// the transcript label; nullptr = the v1 contract (one PI from the circuit,
// label "Merkle tree")
struct ProveOpts {
    uint64_t n_pi;
    const uint64_t *pi_pos, *pi_canon;
    const char *label;
};
// the witness as a variable assignment over the resident wire map
// (pnp_prove_assignment): n_vars Montgomery Fr by variable id, in host memory
// or HBM as device_ptrs says
struct Assignment {
    const uint64_t *values;
    uint64_t n_vars;
};
// What a proof and a satisfiability check (check_witness.cpp) decide alike
// before any work (prover.cpp).  prove_domain: the keys are loaded (the commit
// key only with need_ck), an assignment has its wire map and variable count,
// and the domain n = 2^lg of the inputs is the resident key's; ng = the gate
// rows.  public_input_map: the public inputs of `opt` in BTreeMap order,
// zero values dropped, Montgomery; positions distinct and < n.  Both throw Error.
struct ProveDomain {
    uint64_t n = 1, ng = 0;
    uint32_t lg = 0;
};
ProveDomain prove_domain(pnp_ctx *ctx, const CircuitC *cs, const Assignment *asg, bool need_ck);
void public_input_map(const ProveOpts &opt, uint64_t n, std::vector<uint64_t> &pos, std::vector<Fr> &val);
// The witness comes from the columns of `cs`, or, with `asg` (then cs is
// nullptr and opt is given), from the assignment: the domain is the resident
// key's, the gates and q_lookup rows the resident wire map's.  Throws Error.
void prove_impl(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, ProofC *out, const ProveOpts *opt = nullptr,
                const Assignment *asg = nullptr);

// ---- what the proof, the check and the solver share (context.cpp) ----
// the argument tests of their entry points (each keeps its own message)
static inline bool pis_given(uint64_t n_pi, const uint64_t *pos, const uint64_t *canon) {
    return !n_pi || (pos && canon);
}
static inline bool hbm_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }  // Fr move 16 bytes at a time
// the stage clock of a call (pnp_last_stage_times): a stage ends when the context's stream has drained
struct PNP_HIDDEN StageTimer {
    pnp_ctx *ctx;
    std::chrono::steady_clock::time_point t0;
    explicit StageTimer(pnp_ctx *c) : ctx(c) {}
    void start() {
        ctx->stages.clear();
        t0 = std::chrono::steady_clock::now();
    }
    void mark(const char *name) {
        PNP_HIP(hipStreamSynchronize(ctx->stream));
        const auto t1 = std::chrono::steady_clock::now();
        ctx->stages.emplace_back(name, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};
// The row values of the key's polynomials on the domain 2^lg: a forward
// transform of the resident coefficients into a buffer of its own, when it is
// asked for; nullptr for an optional selector the key does not have
struct PNP_HIDDEN KeyRowValues {
    pnp_ctx *ctx;
    uint32_t lg;
    DevBuf rows[kKeyRows];
    const uint64_t *values(KeyPoly r);
};
// The public inputs of public_input_map in HBM: ascending rows, then their
// Montgomery values 16-byte aligned; one copy and a sync, nothing when there are none
struct PNP_HIDDEN DevicePis {
    DevBuf buf;
    const uint64_t *pos = nullptr, *val = nullptr;
    uint32_t n = 0;
    void upload(const std::vector<uint64_t> &pi_pos, const std::vector<Fr> &pi_val, hipStream_t s);
};
// the check and the solver run on one GPU: "<what>: the context is sharded ... (a multi-rank <noun> ...)"
PNP_HIDDEN void refuse_sharded(pnp_ctx *ctx, const char *what, const char *noun);
// the caller's four columns into dst (n rows each, zero from row ng on) on the
// context's stream: device copies now, host columns added to `up` for one
// h2d_batch with whatever else the caller stages (prover.cpp)
PNP_HIDDEN void stage_wire_columns(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, uint64_t *const dst[4],
                                   uint64_t ng, uint64_t n, std::vector<H2D> &up);

// ---- the satisfiability check (check_witness.cpp); pis: n_pi, pi_pos, pi_canon ----
PNP_HIDDEN void check_assignment(pnp_ctx *ctx, const Assignment &asg, int device_ptrs, const ProveOpts &pis,
                                 pnp_check_report *report);
PNP_HIDDEN void check_witness(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, const ProveOpts &pis,
                              pnp_check_report *report);
// ---- the witness solver (solve_witness.cpp); `what` opens the messages of a plan build ----
PNP_HIDDEN void load_solve_plan(pnp_ctx *ctx, const char *what, const uint32_t *input_ids, uint64_t n_inputs,
                                const uint64_t *output_rows, uint64_t n_outputs, uint32_t gates, uint32_t ecc,
                                uint32_t lookup, int device_ptrs, pnp_solve_info *info);
PNP_HIDDEN void solve_gate_entries(pnp_ctx *ctx, uint64_t out[2]);
PNP_HIDDEN void solve_ecc_entries(pnp_ctx *ctx, uint64_t out[2]);
PNP_HIDDEN void solve_lookup_entries(pnp_ctx *ctx, uint64_t out[2]);
PNP_HIDDEN void solve_assignment(pnp_ctx *ctx, const uint64_t *inputs, uint64_t n_inputs, int device_ptrs,
                                 const ProveOpts &pis);
PNP_HIDDEN void assignment_ptr(pnp_ctx *ctx, uint64_t **d_values, uint64_t *n_vars);
PNP_HIDDEN void assignment_values(pnp_ctx *ctx, const uint32_t *ids, uint64_t k, uint64_t *out);
PNP_HIDDEN void solved_public_inputs(pnp_ctx *ctx, uint64_t *pos, uint64_t *canon, uint64_t cap, uint64_t *n);
// The resident solution as pnp_prove_solved / pnp_check_solved pass it on: the
// caller's public inputs (none on an output row) and then the derived ones; returns the code
struct PNP_HIDDEN SolvedAssignment {
    std::vector<uint64_t> pos, canon;
    uint64_t *values = nullptr;
    uint64_t n_vars = 0;
};
PNP_HIDDEN int solved_assignment(pnp_ctx *ctx, const char *what, uint64_t n_pi, const uint64_t *pi_pos,
                                 const uint64_t *pi_canon, SolvedAssignment &out);
}  // namespace pnp

// the body of a v2 entry point: codes, never exceptions (bad_alloc,
// system_error, anything else), across the C ABI
#define PNP_TRY(...)                                   \
    try {                                              \
        __VA_ARGS__;                                   \
        return PNP_OK;                                 \
    } catch (const ::pnp::Error &e) {                  \
        return e.code;                                 \
    } catch (const std::exception &e) {                \
        ::pnp::set_error("exception: %s", e.what());   \
        return PNP_E_DEVICE;                           \
    } catch (...) {                                    \
        ::pnp::set_error("unknown exception");         \
        return PNP_E_DEVICE;                           \
    }
