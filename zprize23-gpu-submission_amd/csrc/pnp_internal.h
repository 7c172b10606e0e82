// pnp_internal.h — host-side declarations shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <map>
#include <string>
#include <tuple>
#include <vector>
#include "field.cuh"
#include "../../include/pnp_plonk.h"

namespace pnp {

void set_error(const char *fmt, ...);
// shared between the library's units only: kept out of its exports
#define PNP_HIDDEN __attribute__((visibility("hidden")))

#define PNP_HIP(expr)                                                              \
    do {                                                                           \
        hipError_t e_ = (expr);                                                    \
        if (e_ != hipSuccess) {                                                    \
            ::pnp::set_error("%s:%d %s: %s", __FILE__, __LINE__, #expr,            \
                             hipGetErrorString(e_));                               \
            throw ::pnp::Error(PNP_E_DEVICE);                                      \
        }                                                                          \
    } while (0)

struct Error {
    int code;
    explicit Error(int c) : code(c) {}
};

// device buffer with RAII
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    explicit DevBuf(size_t b) { alloc(b); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void alloc(size_t b);
    void reserve(size_t b) { if (bytes < b) alloc(b); }  // grow-only: the contents are lost when it grows
    void release();
    uint64_t *u64() const { return static_cast<uint64_t *>(p); }
    uint32_t *u32() const { return static_cast<uint32_t *>(p); }
};

// ---- NTT (ntt.hip) ----
struct NttTables {
    // tw[e] = w_N^e, e < N/2, for forward and inverse roots, per lg
    std::map<uint32_t, DevBuf> fwd, inv;
    // the same twiddles as dense rows per shift (ntt.hip ntt_twiddle_rows): row
    // sh = w_N^(i 2^sh), i < N / 2^(sh+1), at offset N - N / 2^sh
    std::map<uint32_t, DevBuf> fwd_rows, inv_rows;
    DevBuf coset_hi, coset_lo;        // g^(4096 k), g^k
    DevBuf coset_inv_hi, coset_inv_lo;  // g^-(4096 k), g^-k
    bool coset_ready = false;
    // coset LDE twist per lg_n: (g w_8n^rev3(b))^j for block b, j < n
    std::map<uint32_t, DevBuf> lde_twist;
    // block layout twists per lg_n: (g w_8n^m)^j and w_8n^(-m j), block m
    std::map<uint32_t, DevBuf> blk_twist, blk_twist_inv;
    // the forward block twists times 32 (lde_blocks form29)
    std::map<uint32_t, DevBuf> blk_twist32;
};
const uint64_t *ntt_twiddles(NttTables &t, uint32_t lg, bool inverse, hipStream_t s);
void ntt_prepare_coset(NttTables &t, hipStream_t s);
// natural-order NTT of 2^lg elements in place, or from `src` into d (the first
// pass reads src: no separate copy)
void ntt_run(NttTables &t, uint64_t *d, uint32_t lg, bool inverse, bool coset, hipStream_t s,
             const uint64_t *src = nullptr);
// out8[i] = i < n ? in[i] * g^i : 0, then forward NTT of size 8n (Ntt_coset::forward)
void coset_lde8(NttTables &t, const uint64_t *in, uint64_t *out8, uint32_t lg_n, hipStream_t s);

// block layout of the 8n coset (point i = 8 j + m -> block m, index j):
// LDE of n coefficients into blocks m0 .. m0+nb-1 (any nb, m0 + nb <= 8)
// build every NTT table of domain 2^lg_n on stream s (before forking work
// that reads them onto another stream)
void ntt_warm(NttTables &t, uint32_t lg_n, hipStream_t s);
// form29: the values times 32, i.e. in the 2^261 form of fr29.cuh (k_quotient29)
void lde_blocks(NttTables &t, const uint64_t *in, uint64_t *out, uint32_t lg_n, int m0, int nb,
                hipStream_t s, bool form29 = false);
// per block: unscaled inverse size-n DFT then twist by w_8n^(-m u)
void intt_blocks(NttTables &t, uint64_t *d, uint32_t lg_n, int m0, int nb, hipStream_t s);
// 8-point inverse DFT across blocks + g^-i / (8n): coefficient chunks u in [q0, q0+len)
void t_combine(NttTables &t, const uint64_t *Y, uint64_t len, uint64_t q0, uint64_t *out,
               uint32_t lg_n, unsigned *nz, hipStream_t s);
// coefficient chunks t_1 .. t_nb (out[k n + u]) from blocks 0 .. nb-1 after
// intt_blocks, for deg t < nb n (nb = 6 .. 8; 8 is t_combine).  Both OR into
// the device word *nz bit k when chunk k has a non-zero coefficient.
void t_combine_blocks(NttTables &t, const uint64_t *Y, int nb, uint64_t *out, uint32_t lg_n, unsigned *nz,
                      hipStream_t s);
void to_blocks(const uint64_t *in, uint64_t *out, uint32_t lg_n, int m0, int nb, hipStream_t s);

// ---- live per-kernel timing with HIP events on the launching stream ----
struct KernelTimer {
    bool enabled = false;
    struct Stat {
        double ms = 0, bytes = 0;
        int launches = 0;
    };
    struct Pending {
        std::string name;
        hipEvent_t e0, e1;
        double bytes;
    };
    std::map<std::string, Stat> stats;
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    hipEvent_t get();
    void begin(const char *name, hipStream_t s, hipEvent_t &e0);
    // `bytes`: algorithmic bytes credited to this launch
    void end(const char *name, hipStream_t s, hipEvent_t e0, double bytes = 0);
    void collect();  // call after the stream is synchronized
    // add `units` to a counter read back with pnp_kernel_bytes (no timing)
    void credit(const char *name, double units) {
        if (enabled) stats[name].bytes += units;
    }
};

// Background table builds (context.cpp tables_start_background): on the builder's
// thread every build kernel is followed by bg_step, which waits for it (one
// build kernel in flight at a time, so a proof's streams never queue behind
// more than one of them on a shared hardware queue) and stops the build when
// it is cancelled.  A no-op on every other thread.
extern thread_local bool t_bg_build;
void bg_step(hipStream_t s);

// ---- MSM (msm.hip) ----
// buffers of one group of an MSM batch: counts (coarse-bin counts -> offsets,
// scan_tmp), ent/fkey (pass-A entries and fine keys), offsets (bucket
// starts), sorted (entries by bucket), buckets (XYZZ buckets + reduction tree),
// seg (split-bucket pieces), redo (segments the radix-2^29 accumulation hands
// back to the exact path)
struct MsmGroup {
    DevBuf counts, offsets, scan_tmp, ent, fkey, sorted, buckets, seg, redo;
    DevBuf exc;  // folded: an F29 merge / tree addition met equal or opposite operands
    DevBuf heavy;  // folded: the merge's queue of buckets with many pieces
    uint64_t acc_nent = 0;  // entries the last accumulation was laid out for (msm_internal.h AccLayout)
    uint32_t exc_h = 0, nredo_h = 0;  // host copies of exc and the redo count, read back with the results
    // timed runs only (KernelTimer enabled): what the last k_accumulate29 launch
    // really did, counted on the device from the bucket starts — {sorted
    // entries, pieces started fresh}; mixed additions = entries - pieces
    DevBuf wctr;
    unsigned long long wctr_h[65] = {};  // entries, then 64 piece counters (msm.hip k_count_pieces)
    bool wctr_live = false;
};
struct MsmWork {
    DevBuf digits;  // u32 keys of every (MSM, window, point)
    MsmGroup grp;
    KernelTimer *timer = nullptr;
    // point-range sharding across ranks (pnp_set_msm_shard)
    // window bits of the folded layout (msm_cfg default when 0; PNP_FOLD_C)
    int fold_c = 0;
    int rank = 0, world = 1;
    pnp_allgather_fn allgather = nullptr;
    void *user = nullptr;
    uint64_t *xbuf = nullptr;
    uint64_t xbuf_bytes = 0;
    // all-to-all for the distributed quotient (pnp_set_exchange_a2a)
    pnp_alltoall_fn alltoall = nullptr;
    void *a2a_user = nullptr;
    uint64_t *a2a = nullptr;
    uint64_t a2a_bytes = 0;
    // variable all-to-all of the bucket-range sharded MSMs (pnp_set_exchange_v):
    // rank s owns buckets [s NB/W, (s+1) NB/W) of every MSM, the entries travel
    // to their bucket's owner; unset: point-range sharding
    pnp_alltoallv_fn alltoallv = nullptr;
    void *v_user = nullptr;
    uint64_t *v_send = nullptr, *v_recv = nullptr;
    uint64_t v_bytes = 0;
    // the exchange callbacks enqueue their collectives on the library's
    // stream (pnp_set_exchange_ordered: RCCL on pnp_ctx_stream): the data they
    // move is ordered behind the work that made it, no host synchronisation
    // before a callback; otherwise (host-memory exchanges) the stream is
    // synchronised first
    bool ordered = false;
    // the folded table covers ALL n points (bucket ranges gather any point)
    bool full_table() const { return world > 1 && alltoallv != nullptr; }
    // Fixed-slot bucket exchange (msm.hip msm_bucket_batch): every rank sends
    // every peer one slot of `cap` records with the bin counts in the slot's
    // header, so the records move in one equal-size all-to-all with no host
    // round trip to size it.  cap is per batch of a proof (its ordinal since
    // the proof began, B, the table's n), set from the all-gathered counts of
    // that batch's first variable-size run (the same on every rank); a batch
    // whose counts outgrow it is redone on the variable path, which raises it.
    // PNP_MSM_SLOTS=0: always the variable path.
    std::map<std::tuple<uint32_t, int, uint64_t>, uint64_t> slot_cap;
    uint32_t batch_seq = 0;  // bucket-range batches since the proof began
    DevBuf slot_dev;         // run table, bin starts, flags, per-destination counts
    unsigned long long slot_runs = 0, slot_overflows = 0;  // slotted batches / redone ones
};
// before an exchange callback: the data on the stream is complete
inline void ex_fence(const MsmWork &wk, hipStream_t s) {
    if (!wk.ordered) PNP_HIP(hipStreamSynchronize(s));
}
// all-gather of k words per rank (rank-major result, world x k), every slot
// tagged (PNP_EX_TAG_*, include/pnp_plonk.h) and the tags checked
std::vector<uint64_t> rank_allgather(MsmWork &wk, hipStream_t s, const uint64_t *mine, int k, uint64_t tag);
// sum_i s_i P_i; scalars Montgomery Fr; result written to host as XYZZ Fq (4x6 u64)
// `table` (optional): msm_build_table(d_points, n) — the folded layout
void msm_run(MsmWork &w, const uint64_t *d_points, const uint64_t *d_scalars_mont, uint64_t n,
             uint64_t *h_xyzz, hipStream_t s, const uint64_t *table = nullptr);
// A folded table built over n_table points holding several point sets: MSM b
// of a batch sums over points off[b] .. off[b] + n - 1 of it (wires.hip: the
// four wires' grouped bases in one table)
struct MsmSegs {
    uint64_t n_table = 0;
    uint64_t off[16] = {};
    // multi-GPU point ranges: the table holds only this rank's slice [p0, p1)
    // of every set (msm_point_range of the MSM length), off[] are the slices'
    // starts in it — 1/world of the full table
    bool sliced = false;
    // window bits of the table (0: msm_cfg(n_table)); a table over several
    // point sets takes the width for ONE set's size (msm_fold_c(n)): its
    // buckets serve one set per MSM
    int c = 0;
};
// the folded layout's window bits for an MSM over n_points points
int msm_fold_c(uint64_t n_points, int fold_c);
// scalars_local: multi-GPU, d_scalars[b] hold only this rank's point range
// segs: `table` is segmented as above (d_points unused)
void msm_run_batch(MsmWork &w, const uint64_t *d_points, const uint64_t *const *d_scalars, int B,
                   uint64_t n, uint64_t *h_xyzz, hipStream_t s, const uint64_t *table = nullptr,
                   bool scalars_local = false, const MsmSegs *segs = nullptr);
// HBM of the MSM machinery, upper bounds (the key-load budget): a folded table
// over n_points (windows of a table for n_cfg points), its build scratch, the
// work buffers of a B-MSM batch over n_pts points, and what wk holds now
uint64_t msm_table_bytes(uint64_t n_points, uint64_t n_cfg, int fold_c);
uint64_t msm_table_build_bytes(uint64_t n_points);
uint64_t msm_work_bytes(uint64_t n_pts, uint64_t n_cfg, int fold_c, int B, uint64_t v_bytes, int world);
uint64_t msm_work_held(const MsmWork &wk);
// multi-GPU MSMs: the points [p0, p1) rank `rank` of `world` takes
void msm_point_range(uint64_t n, int rank, int world, uint64_t &p0, uint64_t &p1);
// T[k*n + i] = 2^(c*k) P_i, k < W (msm_cfg(n)), affine, in the signed
// radix-2^30 form of field30s.cuh (x, y: 13 i32 each, padded to 128 B per point)
void msm_build_table(DevBuf &tab, const uint64_t *d_points, uint64_t n, int c, hipStream_t s);
// n device XYZZ points (24 u64) -> affine (12 u64; infinity -> (0, 0)), synchronous
void xyzz_to_affine_dev(const uint64_t *xyzz, uint64_t n, uint64_t *aff, hipStream_t s);
// the first n (a power of two) commit-key points d_aff (affine, 12 u64 each) in
// the Lagrange basis of the order-n subgroup (lagrange.hip): d_out[i] =
// n_inv sum_j omega_inv^(i j) d_aff[j]; false when the key is degenerate
// (an output at infinity or an exceptional addition); synchronous
bool srs_lagrange(const uint64_t *d_aff, uint64_t n, const Fr &omega_inv, const Fr &n_inv, uint64_t *d_out,
                  hipStream_t s);
// host: XYZZ -> affine Montgomery (inf -> (0, one))
void xyzz_to_affine_host(const uint64_t *xyzz, uint64_t *aff12);
// B points (24 u64 each) -> B affine (12 u64 each), one inversion
void xyzz_to_affine_batch_host(const uint64_t *xyzz, int B, uint64_t *aff12);

// ---- poly / elementwise (poly.hip) ----
void k_from_mont(uint64_t *d, uint64_t n, hipStream_t s);
void k_to_mont(uint64_t *d, uint64_t n, hipStream_t s);
void k_prefix_product(uint64_t *d, uint64_t n, DevBuf &scratch, hipStream_t s);
void k_batch_inverse(uint64_t *d, uint64_t n, DevBuf &scratch, hipStream_t s);
void k_poly_eval(const uint64_t *d, uint64_t n, const Fr &x, DevBuf &scratch, Fr *out,
                 hipStream_t s);
// several polys (same n) at the same point in one launch
void k_poly_eval_multi(const uint64_t *const *polys, int npolys, uint64_t n, const Fr &x,
                       DevBuf &scratch, Fr *out, hipStream_t s);
// several such sets (each its own point), one host round trip for all
struct EvalSet {
    const uint64_t *const *polys;
    int np;
    Fr x;
    Fr *out;
};
void k_poly_eval_sets(const EvalSet *sets, int nsets, uint64_t n, DevBuf &scratch, hipStream_t s);
void k_poly_div_linear(uint64_t *d, uint64_t n, const Fr &z, DevBuf &scratch, hipStream_t s);
// several divisions d_k / (X - z_k) sharing every launch
void k_poly_div_linear_batch(uint64_t *const *d, const Fr *z, int K, uint64_t n, DevBuf &scratch,
                             hipStream_t s);
// d[i] += c z^(len-1-i)
void k_add_powers(uint64_t *d, uint64_t len, const Fr &c, const Fr &z, hipStream_t s);
void k_random_fr(uint64_t *d, uint64_t n, uint64_t seed, hipStream_t s);
// d[i] = c0 * r^i
void k_geometric(uint64_t *d, uint64_t n, const Fr &c0, const Fr &r, hipStream_t s);
void k_srs(uint64_t *d, uint64_t n, const Fr &tau, hipStream_t s);
void k_coset_consts(uint64_t *vh, uint64_t *x, uint32_t lg_n, hipStream_t s);
// ---- key-load kernels (keyblocks.hip) ----
// the coset constants of blocks m0 .. m0 + nb - 1 in block-bitrev layout from
// their closed forms (coset_blocks.cuh): lin, lin32 = 32 lin (the 2^261 form),
// vh_inv, and l1_den = D (lin - 1), whose inverse is l1v; nullptr = not wanted
void k_coset_blocks(uint32_t lg_n, int m0, int nb, uint64_t *lin, uint64_t *lin32, uint64_t *vh_inv,
                    uint64_t *l1_den, hipStream_t s);
// d_out[k] = the point with natural index d_idx[k] (< 8n) of a block-layout
// array holding blocks m0 .. m0 + nb - 1 (zero when its block is not held)
void k_gather_blocks(const uint64_t *blk, uint32_t lg_n, int m0, int nb, const uint64_t *d_idx, uint32_t cnt,
                     uint64_t *d_out, hipStream_t s);
// ---- circuit preprocessing (preprocess.hip) ----
// slots (4 row + wire) one workgroup of the permutation's radix sort ranks
constexpr uint32_t PNP_SIGMA_TILE = 4096;
struct WireSigmaStats {
    int passes = 0;    // 8-bit digit passes the sort ran
    double bytes = 0;  // what the kernels must move (keys, slot ids, next)
};
uint64_t wire_sigma_scratch_bytes(uint64_t n_gates);
// the copy permutation of a wire map: d_next[j D + i] = j' D + i' (4 D u32)
// and the sigma columns K_j' w^i' (D Montgomery Fr each; nullptr = not
// wanted); returns the first slot 4 row + wire whose id is >= n_vars, ~0 when
// there is none.  Synchronous; scratch grows to wire_sigma_scratch_bytes
uint64_t wire_sigma(NttTables &ntt, const uint32_t *const d_var[4], uint64_t n_gates, uint64_t n_vars, uint32_t lg,
                    uint32_t *d_next, uint64_t *const d_sigma[4], DevBuf &scratch, hipStream_t s,
                    WireSigmaStats *stats = nullptr);
// the permutation's stable radix sort for any m u32 keys below 2^bits (bits >=
// 1): order[p] = the position the p-th smallest key came from, equal keys in
// position order.  The result lies in `scratch` (grown to fit); asynchronous
const uint32_t *sort_positions_u32(const uint32_t *d_keys, uint64_t m, int bits, DevBuf &scratch, hipStream_t s);
// dst[i] = src[i], i < n; then src[0] (first) or zero up to D; dst == src pads in place
void k_pad_col(uint64_t *dst, const uint64_t *src, uint64_t n, uint64_t D, bool first, hipStream_t s);
// ---- the witness from a variable assignment (assignment.hip) ----
// d_w[j][i] = d_values[d_var[j][i]] for i < n_gates, zero for n_gates <= i <
// 2^lg: one launch over the 2^lg rows.  An id >= n_vars reads as zero.
void k_gather_witness(const uint32_t *const d_var[4], uint64_t n_gates, const uint64_t *d_values, uint64_t n_vars,
                      uint32_t lg, uint64_t *const d_w[4], hipStream_t s);
// the first slot 4 row + wire at which the columns a[j] and b[j] (2^lg Fr
// each) differ, ~0 when they are equal.  Synchronous; scratch: 8 bytes
uint64_t k_first_diff4(const uint64_t *const a[4], const uint64_t *const b[4], uint32_t lg, DevBuf &scratch,
                       hipStream_t s);
// ---- the satisfiability check of a witness, row by row (check.hip) ----
// what the kernels leave behind: the least violated (row << 8 | kind << 4 |
// index), ~0 when none, and the violated (row, constraint) pairs per kind
struct CheckRecord {
    unsigned long long first;
    unsigned long long by_kind[PNP_CHECK_KINDS];
};
// the rows the gate kernels read: D = 2^lg rows each, HBM, 16-byte aligned
struct CheckRows {
    const uint64_t *w[4];  // the padded witness columns (zero from row n_gates on)
    const uint64_t *q_m, *q_l, *q_r, *q_o, *q_4, *q_c, *q_hl, *q_hr, *q_h4, *q_arith;  // q_m: nullptr = zero
    const uint64_t *fam[4];   // range, logic, fixed-base, curve-add selector rows; nullptr = absent
    const uint64_t *pi_pos;   // n_pi ascending rows and their Montgomery values (nullptr with n_pi = 0)
    const uint64_t *pi_val;
    uint32_t n_pi, lg;
};
void k_check_reset(CheckRecord *rec, hipStream_t s);
// ARITH, constraint 0, on every row
void k_check_arith(const CheckRows &r, CheckRecord *rec, hipStream_t s);
// family f (0 range .. 3 curve-add, r.fam[f] != nullptr), its own kernel
void k_check_family(int f, const CheckRows &r, CheckRecord *rec, hipStream_t s);
// the set of the distinct rows of the table t[0..3] (D rows each): row indices
// in `slots` (2 D u32, open addressing); rows equal to row 0 stay out but row 0
void k_check_table_set(const uint64_t *const t[4], uint32_t lg, uint32_t *slots, hipStream_t s);
// LOOKUP: s_rows (the first s_n rows read, zero beyond; nullptr = zero), k_rows
// (D rows; nullptr = zero) as include/pnp_plonk.h states it
void k_check_lookup(const uint64_t *const w[4], const uint64_t *s_rows, uint64_t s_n, const uint64_t *k_rows,
                    const uint64_t *const t[4], const uint32_t *slots, uint32_t lg, CheckRecord *rec, hipStream_t s);
// COPY: every slot of the wire map against the lowest slot of its variable;
// first: n_vars u32 of scratch.  An id >= n_vars (the loaders refuse such
// maps) is skipped
void k_check_copy(const uint32_t *const d_var[4], uint64_t n_gates, uint64_t n_vars, const uint64_t *const w[4],
                  uint32_t lg, uint32_t *first, CheckRecord *rec, hipStream_t s);

// ---- the witness from the circuit's inputs (solve.hip) ----
// the selector rows the plan is built from: D rows each, HBM; q_m nullptr = zero
struct SolveSel {
    const uint64_t *q_m, *q_l, *q_r, *q_o, *q_4, *q_c, *q_hl, *q_hr, *q_h4, *q_arith;
    // the gate families of pnp_load_solve_plan_gates: nullptr = the family's
    // flag is not set, or the key has no such rows
    const uint64_t *range, *logic;
    // the ECC families of pnp_load_solve_plan_ecc, likewise
    const uint64_t *fixed_add, *var_add;
    // the q_lookup rows of pnp_load_solve_plan_lookup, likewise
    const uint64_t *lookup;
};
// A plan in HBM, level order: entry p defines variable tgt[p] from row row[p] as
//   q_l' a + q_r' b + q_o' c + q_4' d + q_hl' a^5 + q_hr' b^5 + q_h4' d^5 + q_m' a b + q_c' + pik PI_row,
// a .. d the values of var[0..3][p]; every q' is the row's selector times
// -1 / coef, zero for the target's own slot and for slots that are not
// relevant; pik = -1 / (coef q_arith).  Level l is entries lvl_off[l] ..
// lvl_off[l + 1].  n entries; the arrays start 16-byte aligned.
enum { kSolveQl, kSolveQr, kSolveQo, kSolveQ4, kSolveQhl, kSolveQhr, kSolveQh4, kSolveQc, kSolvePik, kSolveQm,
       kSolveCoefs };
// The output rows of a plan, after the levels, in listed order: entry k derives
//   PI_row = q_l' a + q_r' b + q_o' c + q_4' d + q_hl' a^5 + q_hr' b^5 + q_h4' d^5 + q_m' a b + q_c'
// of row row[k], every q' the row's selector times -q_arith (every slot as it
// stands: one that is not relevant only meets zero coefficients); there is no
// pik (coef[kSolvePik] is nullptr).  pi: n_out Fr, the canonical values the
// last solve derived.
struct SolveOutView {
    uint64_t *coef[kSolveCoefs];
    uint32_t *row, *var[4];
    uint64_t *pi;
};
struct SolveView {
    uint64_t *coef[kSolveCoefs];  // coef[kSolveQm] nullptr: the key has no q_m
    uint32_t *tgt, *row, *var[4], *lvl_off, *ids;
    SolveOutView out;
    static uint64_t padded(uint64_t n) { return (n + 3) & ~3ULL; }
    static uint64_t bytes(uint64_t n, uint64_t n_levels, uint64_t n_inputs, uint64_t n_out, bool qm) {
        return padded(n) * (32 * (kSolveCoefs - (qm ? 0 : 1)) + 4 * 6) + 4 * padded(n_levels + 1) + 4 * padded(n_inputs) +
               padded(n_out) * (32 * (kSolveCoefs - (qm ? 1 : 2)) + 4 * 5 + 32);
    }
    void lay(void *base, uint64_t n, uint64_t n_levels, uint64_t n_inputs, uint64_t n_out, bool qm);
};
// What the plan build leaves on the host: per level its width (the rounds of
// include/pnp_plonk.h's plan rules), and what stayed undetermined.
struct SolveBuild {
    std::vector<uint32_t> widths;  // arithmetic entries of each level
    std::vector<uint32_t> gate_widths;  // gate entries of each level (as many levels; all zero without gate rows)
    uint64_t n_range = 0, n_logic = 0;  // gate entries by the family of the row that defines them
    uint64_t n_two = 0;                 // gate entries that read two values (the others read one)
    // pnp_load_solve_plan_ecc: the fixed-add scalar definitions are gate entries
    // (counted in gate_widths and in n_fixed); the other ECC definitions are
    // entries of their own, ecc_widths a level, defining ecc_vars variables
    std::vector<uint32_t> ecc_widths, ecc_vars;
    uint64_t n_fixed = 0, n_var = 0;    // variables fixed-add rows, var-add rows define
    // pnp_load_solve_plan_lookup: the lookup entries of each level (one a variable), and all of them
    std::vector<uint32_t> lookup_widths;
    uint64_t n_lookup = 0;
    uint64_t n_undetermined = 0;
    uint32_t first_undetermined = 0xffffffffu;
};
// The gate entries of a plan (range and logic rows), in arrays of their own,
// level order, by variable id within a level: entry g defines variable tgt[g]
// from the canonical integers A, B of the variables a[g], b[g] (b = a where
// only one is read); word[g] = kind | shift << 8:
//   kSolveGateShift  A >> shift          (every range slot; logic a_i, b_i)
//   kSolveGateProd   (A & 3) (B & 3)     (logic c_i)
//   kSolveGateAnd    (A >> shift) & (B >> shift)
//   kSolveGateXor    (A >> shift) ^ (B >> shift), minus r when that reaches r
//   kSolveGateNaf    (A - s) / 2, s the lowest width-2 NAF digit of A (fixed-add d)
// Level l is entries lvl_off[l] .. lvl_off[l + 1].
enum { kSolveGateShift, kSolveGateProd, kSolveGateAnd, kSolveGateXor, kSolveGateNaf };
struct SolveGateView {
    uint32_t *tgt, *a, *b, *word, *lvl_off;
    static uint64_t bytes(uint64_t n, uint64_t n_levels) {
        return 16 * SolveView::padded(n) + 4 * SolveView::padded(n_levels + 1);
    }
    void lay(void *base, uint64_t n) {
        const uint64_t nn = SolveView::padded(n);
        tgt = static_cast<uint32_t *>(base), a = tgt + nn, b = tgt + 2 * nn, word = tgt + 3 * nn, lvl_off = tgt + 4 * nn;
    }
};
// The ECC entries of a plan (fixed-add xy and point, var-add), in arrays of
// their own, level order, by (row, kind) within a level.  Entry e, read 16
// bytes at a time: tgt[e] = three target variables (~0: not won, or none) and
// the kind; src[e] = four source variables; q[0..2][e] = q_l, q_r, q_c of the
// row (Montgomery; zero for a var-add entry).  With bit = d_next - 2 d:
//   kSolveEccXy     src = d, d_next of the row and the next:   t0 = bit q_c
//   kSolveEccPoint  src = a, b, d, d_next: x = q_l bit, y = bit^2 (q_r - 1) + 1,
//                   m = (bit q_c) a b D:   t0 = (x b + y a) / (1 + m),
//                   t1 = (y b - A x a) / (1 - m)
//   kSolveEccVar    src = a, b, c, d of the row: n = a d, t = D n (b c):
//                   t0 = (n + b c) / (1 + t), t1 = (b d - A a c) / (1 - t), t2 = n
// one inversion of (1 + m)(1 - m) an entry, a zero factor left out of it and
// its quotient zero.  Level l is entries lvl_off[l] .. lvl_off[l + 1].
enum { kSolveEccXy, kSolveEccPoint, kSolveEccVar, kSolveEccKinds };
struct SolveEccView {
    uint4 *tgt, *src;
    uint64_t *q[3];
    uint32_t *lvl_off;
    static uint64_t bytes(uint64_t n, uint64_t n_levels) {
        return (32 + 96) * SolveView::padded(n) + 4 * SolveView::padded(n_levels + 1);
    }
    void lay(void *base, uint64_t n) {
        const uint64_t nn = SolveView::padded(n);
        for (int c = 0; c < 3; c++) q[c] = static_cast<uint64_t *>(base) + 4 * nn * c;
        tgt = reinterpret_cast<uint4 *>(q[2] + 4 * nn), src = tgt + nn;
        lvl_off = reinterpret_cast<uint32_t *>(src + nn);
    }
};
// The lookup entries of a plan (q_lookup rows), in an array of their own, level
// order, by variable id within a level: entry k, one uint4, is the target and
// the sources a, b, d; the target becomes column 2 of the lowest table row whose
// columns 0, 1, 3 equal the sources' values word for word, zero when there is
// none.  Level l is entries lvl_off[l] .. lvl_off[l + 1].
// The index (solve_lookup_index; a buffer of its own): a CSR over B = bmask + 1
// hash buckets.  rows[off[h] .. off[h + 1]] are the table rows of bucket h in
// ascending order, row 0 and every row that differs from row 0 (the padding
// repeats row 0: the copies change no answer); t[0..3] the key's resident table
// columns, D Montgomery rows each.
struct SolveLookupView {
    uint4 *ent;
    uint32_t *lvl_off;
    const uint32_t *off, *rows;
    uint32_t bmask;
    const uint64_t *t[4];
    static uint64_t bytes(uint64_t n, uint64_t n_levels) {
        return 16 * SolveView::padded(n) + 4 * SolveView::padded(n_levels + 1);
    }
    void lay(void *base, uint64_t n) {
        ent = static_cast<uint4 *>(base);
        lvl_off = reinterpret_cast<uint32_t *>(ent + SolveView::padded(n));
    }
    // m indexed rows: off[0 .. B], then rows[0 .. m - 1]
    static uint64_t buckets(uint64_t m) {
        uint64_t b = 2;
        while (b < 2 * m) b <<= 1;
        return b;
    }
    static uint64_t index_bytes(uint64_t m) { return 4 * SolveView::padded(buckets(m) + 1) + 4 * SolveView::padded(m); }
};
// The (row, role) of a bid and of a definition: 32 row + role, the least wins.
// Roles: the arithmetic slots a..d, then range a..d, then logic a, b, c, d,
// d_next, then fixed-add d, c, a_next, b_next, then var-add a_next, b_next,
// d_next, then lookup c
enum { kSolveRoleRange = 4, kSolveRoleLogic = 8, kSolveRoleFixed = 13, kSolveRoleVar = 17, kSolveRoleLookup = 20,
       kSolveRoles = 21, kSolveRoleBits = 5 };
// level[u] = 0 for the n_inputs listed variables (UNSET before); returns the
// lowest id >= n_vars in err[0], the lowest id listed twice in err[1] (~0: none)
void solve_mark_inputs(const uint32_t *d_ids, uint64_t n_inputs, uint64_t n_vars, uint32_t *d_level, uint32_t err[2],
                       DevBuf &scratch, hipStream_t s);
// The output rows: bit `row` of d_bits (n_gates bits, whole u32 words) set for
// each of the n_out listed rows.  err[0]: the lowest listed row >= n_gates,
// err[1]: the lowest row listed twice, err[2]: the lowest row whose q_arith is
// zero (~0: none); the same on every run
void solve_mark_outputs(const uint64_t *d_rows, uint64_t n_out, uint64_t n_gates, const uint64_t *q_arith,
                        uint32_t *d_bits, uint64_t err[3], DevBuf &scratch, hipStream_t s);
// the rounds: d_level[u] = the round that defines u (1-based), d_def[u] = 32 row
// + role of the rule that defines it (row: the row whose rule fires); d_level /
// d_def: n_vars u32, d_level as solve_mark_inputs left it.  A row of d_out_bits
// (solve_mark_outputs; nullptr: no outputs) is never looked at.  sel.range /
// sel.logic / sel.fixed_add / sel.var_add / sel.lookup switch the gate rules on
// (n_gates < 2^27).  ecc_level (with an ECC family on: 3 n_gates u32, allocated here):
// the round in which rule kind k of row i defined something at [3 i + k], 0 for
// none.  Synchronous (one read-back a round)
void solve_rounds(const uint32_t *const d_var[4], uint64_t n_gates, uint64_t n_vars, const SolveSel &sel,
                  const uint32_t *d_out_bits, uint32_t *d_level, uint32_t *d_def, DevBuf &ecc_level, SolveBuild &out,
                  hipStream_t s);
// the plan's entries in (level, variable id) order from d_level / d_def; the
// inversions by k_batch_inverse; then the entries of the n_out output rows
// d_out_rows.  `v` laid over a buffer of SolveView::bytes; `g` (read only when
// the build has gate entries) over one of SolveGateView::bytes, `e` (ECC
// entries, from d_ecc_level) over one of SolveEccView::bytes, `k` (lookup
// entries: ent and lvl_off) over one of SolveLookupView::bytes
void solve_emit(const uint32_t *const d_var[4], uint64_t n_gates, uint64_t n_vars, const SolveSel &sel,
                const uint32_t *d_level, const uint32_t *d_def, const uint32_t *d_ecc_level, const SolveBuild &b,
                const uint64_t *d_out_rows, uint64_t n_out, const SolveView &v, const SolveGateView &g,
                const SolveEccView &e, const SolveLookupView &k, hipStream_t s);
// the table index of a plan with lookup entries over the table columns t[0..3]
// (D rows each): counts the indexed rows m (returned), allocates `index`
// (SolveLookupView::index_bytes(m)) and fills it, k.off / rows / bmask / t set.
// No atomics: the same bytes on every run.  Synchronous
uint64_t solve_lookup_index(const uint64_t *const t[4], uint64_t D, DevBuf &index, SolveLookupView &k, hipStream_t s);
// vals[ids[k]] = in[k]
void k_solve_scatter(const uint32_t *d_ids, const uint64_t *d_in, uint64_t n_inputs, uint64_t *d_vals, hipStream_t s);
// levels [l0, l1) of the plan: each level one launch when `wide`, else all of
// them in one launch of one workgroup (every level at most 256 entries).
// pi_pos / pi_val as CheckRows
void k_solve_levels(const SolveView &v, uint32_t l0, uint32_t l1, uint64_t p0, uint64_t p1, bool wide, uint64_t *d_vals,
                    const uint64_t *pi_pos, const uint64_t *pi_val, uint32_t n_pi, hipStream_t s);

// the gate entries g0 .. g1 - 1 of one level, a lane an entry; naf: the plan
// has kSolveGateNaf entries (without them the kernels are the ones there were)
void k_solve_gate_level(const SolveGateView &g, uint64_t g0, uint64_t g1, uint64_t *d_vals, hipStream_t s,
                        bool naf = false);
// levels [l0, l1) with gate entries among them, every level at most 256 entries
// in all: one launch of one workgroup of 512, the arithmetic entries of a level
// in its first four waves and the gate entries in the other four
void k_solve_mixed_levels(const SolveView &v, const SolveGateView &g, uint32_t l0, uint32_t l1, uint64_t *d_vals,
                          const uint64_t *pi_pos, const uint64_t *pi_val, uint32_t n_pi, hipStream_t s,
                          bool naf = false);

// the ECC entries e0 .. e1 - 1 of one level, a lane an entry
void k_solve_ecc_level(const SolveEccView &e, uint64_t e0, uint64_t e1, uint64_t *d_vals, hipStream_t s);
// levels [l0, l1) with ECC entries among them, every level at most 256 entries
// in all: one launch of one workgroup of 768, arithmetic entries in waves 0-3,
// gate entries (gates: the plan has any) in waves 4-7, ECC entries in waves 8-11
void k_solve_ecc_levels(const SolveView &v, const SolveGateView &g, bool gates, const SolveEccView &e, uint32_t l0,
                        uint32_t l1, uint64_t *d_vals, const uint64_t *pi_pos, const uint64_t *pi_val, uint32_t n_pi,
                        hipStream_t s);

// the lookup entries k0 .. k1 - 1 of one level, a lane an entry
void k_solve_lookup_level(const SolveLookupView &k, uint64_t k0, uint64_t k1, uint64_t *d_vals, hipStream_t s);
// levels [l0, l1) with lookup entries among them, every level at most 256
// entries in all: one launch of one workgroup, arithmetic entries in waves 0-3,
// then (gates: the plan has gate entries) gate entries in waves 4-7, then the
// lookup entries in four waves of their own.  ecc: the plan has
// ECC entries; the workgroup is then k_solve_ecc_levels' 768 and the lookup
// entries take the lanes of waves 4-7 after the level's gate entries
void k_solve_lookup_levels(const SolveView &v, const SolveGateView &g, bool gates, const SolveEccView &e,
                           bool ecc, const SolveLookupView &k, uint32_t l0, uint32_t l1, uint64_t *d_vals,
                           const uint64_t *pi_pos, const uint64_t *pi_val, uint32_t n_pi, hipStream_t s);

// the derived public inputs of the plan's n_out output rows from the solved
// values: v.out.pi[k], canonical
void k_solve_outputs(const SolveView &v, uint64_t n_out, const uint64_t *d_vals, hipStream_t s);

void k_synth_merkle(int height, const uint64_t *pc_mont_host, const uint64_t *leaves, const uint64_t *blind,
                    uint64_t *nodes, uint64_t *const w[4], uint64_t *const sel[9], uint64_t *const sigma[4],
                    uint64_t n, hipStream_t s);
void k_synth_circuit(uint64_t *const w[4], uint64_t *const sel[9], uint64_t *const sigma[4],
                     uint64_t n, uint64_t n_gates, uint64_t pi_pos, const Fr &pi_mont,
                     hipStream_t s);

}  // namespace pnp
