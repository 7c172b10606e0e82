// prover.cpp — gen_proof orchestration on one MI355X.
//
// Protocol order and transcript labels follow the reference's prove()
// (lib/PLONK/src/gen_proof.cuh:10-489); the semantics are the ZK-Garage
// prover's (prover.rs:171-660), which the GPU path reproduces on its own
// circuit class (the Merkle circuit: no custom gates, no lookup tables, one
// public input) and abandons outside it (combine_split
// skipped, empty q_m / custom-selector / q_lookup coefficients, the 8-byte
// t_next / h1_next shift — proofs its verifier rejects).  Here, for any
// circuit: h1 / h2 from combine_split (lookup.hip), z2 with the true next
// row, the range / logic / fixed-base / curve-add widgets in the quotient
// (k_widgets) and the linearisation, q_m and q_lookup terms, and any number
// of public inputs (pnp_prove_ex).  On the Merkle class every extra term is
// zero and is skipped without a launch.
//
// What differs is HOW it runs on MI355X:
//   * the prover key and SRS are HBM-resident (pnp_load_*), no per-proof H2D
//     copies (the reference re-copies ~23 GB per proof, gen_proof.cuh:64-78,
//     166-180, quotient.cu:201-367);
//   * one stream, buffers sized once and reused (no per-op allocation);
//   * fused passes (protocol.hip) instead of ~100 single-op launches;
//   * MSMs of polynomials that are identically zero (h1, h2, and f / table
//     when the lookup tables are empty) are not launched: their commitment is
//     the point at infinity, exactly what the MSM would return;
//   * the 14 commitments in the openings whose values never reach the proof
//     (gen_proof.cuh:421, 450: aw/saw commits only feed empty randomness) are
//     not computed; z_comm is the z commitment (saw_commits[0] == commit(z)).
#include <string.h>
#include "context.h"
#include "protocol.h"
#include "transcript.h"
#include "widgets.cuh"
#include <algorithm>
#include <stddef.h>

namespace pnp {

Fr fr_from_u64(uint64_t x) {
    Fr r = Fr::zero();
    r.v[0] = (uint32_t)x;
    r.v[1] = (uint32_t)(x >> 32);
    return to_mont(r);
}

Fr root_of_unity(uint32_t lg) {
    const uint64_t root32[4] = {13381757501831005802ULL, 6564924994866501612ULL,
                                789602057691799140ULL, 6625830629041353339ULL};
    return pow_u64(from_u64_limbs<FrP>(root32), 1ULL << (32 - lg));
}

namespace {

void append_comm(Transcript &t, const char *label, const CommitmentC &c) {
    t.append_point(label, c.x, c.y);
}

void set_infinity(CommitmentC *c) {
    memset(c, 0, sizeof *c);
    to_u64_limbs(Fq::one(), c->y);
}

// k words from every rank (rank-major), one tagged all-gather
std::vector<uint64_t> shard_allgather(pnp_ctx *ctx, const uint64_t *mine, int k, uint64_t tag) {
    return rank_allgather(ctx->msm, ctx->stream, mine, k, tag);
}

// In place p_k <- p_k / (X - z_k) (kzg10.cu:87-99) for the K polynomials of
// round 6, where this rank holds the coefficient range [a, a + len) of each.
// Quotient coefficient q_i = sum_(k > i) p_k z^(k-i-1) = (division of the
// local slice) + z^(a+len-1-i) C with C = sum_(k >= a+len) p_k z^(k-a-len):
// every rank shares the value E_r of its slice at z, C follows from the E of
// the ranks above — both polynomials' values in ONE all-gather.
void div_linear_range(pnp_ctx *ctx, uint64_t *const *d, const Fr *z, int K, uint64_t len, bool dist) {
    hipStream_t s = ctx->stream;
    if (!dist) {
        k_poly_div_linear_batch(d, z, K, len, ctx->scratch_a, s);  // one chain of launches for all K
        return;
    }
    const int world = ctx->msm.world, rank = ctx->msm.rank;
    std::vector<uint64_t> mine(4 * K);
    std::vector<Fr> e(K);
    std::vector<EvalSet> sets(K);
    for (int k = 0; k < K; k++) sets[k] = {d + k, 1, z[k], &e[k]};
    k_poly_eval_sets(sets.data(), K, len, ctx->scratch_a, s);
    for (int k = 0; k < K; k++) to_u64_limbs(e[k], &mine[4 * k]);
    std::vector<uint64_t> all = shard_allgather(ctx, mine.data(), 4 * K, PNP_EX_TAG_DIV_CARRY);
    const uint64_t n = len * world;  // equal ranges (world divides 8 and n)
    k_poly_div_linear_batch(d, z, K, len, ctx->scratch_a, s);
    for (int k = 0; k < K; k++) {
        Fr c = Fr::zero();
        const Fr zl = pow_u64(z[k], n / world);
        for (int r = world - 1; r > rank; r--) c = c * zl + from_u64_limbs<FrP>(&all[4 * (K * r + k)]);
        if (rank < world - 1) k_add_powers(d[k], len, c, z[k], s);
    }
}

// the proof ends here: the message for pnp_last_error, the code for the entry point
template <class... A>
[[noreturn]] void fail(int code, const char *fmt, A... a) {
    set_error(fmt, a...);
    throw Error(code);
}

}  // namespace

// the keys, the assignment and the domain: the circuit's, which must be the
// key's; an assignment is proved (checked) on the key's (its wire map was
// loaded against it)
ProveDomain prove_domain(pnp_ctx *ctx, const CircuitC *cs, const Assignment *asg, bool need_ck) {
    if (!ctx->key.loaded || (need_ck && !ctx->ck_loaded))
        fail(PNP_E_NOKEY, need_ck ? "prover key / commit key not loaded" : "prover key not loaded");
    if (asg) {
        if (!ctx->key.wm_loaded)
            fail(PNP_E_NOKEY, "no wire map resident (pnp_preprocess or pnp_load_wire_map first)");
        if (asg->n_vars != ctx->key.wm_vars)
            fail(PNP_E_ARG, "assignment of %llu variables, the resident wire map has %llu",
                 (unsigned long long)asg->n_vars, (unsigned long long)ctx->key.wm_vars);
    }
    ProveDomain d;
    const uint64_t bound = asg ? ctx->key.n : cs->n > cs->lookup_len ? cs->n : cs->lookup_len;
    while (d.n < bound) { d.n <<= 1; d.lg++; }
    if (d.n != ctx->key.n)
        fail(PNP_E_ARG, "circuit domain %llu != prover key domain %llu", (unsigned long long)d.n,
             (unsigned long long)ctx->key.n);
    if (need_ck && ctx->ck_points < d.n)
        fail(PNP_E_ARG, "commit key has %llu points, need %llu", (unsigned long long)ctx->ck_points,
             (unsigned long long)d.n);
    d.ng = asg ? ctx->key.wm_gates : cs->n;
    return d;
}

// a PublicInputs map (pi.rs:16-86): BTreeMap order, zero values dropped, Montgomery
void public_input_map(const ProveOpts &opt, uint64_t n, std::vector<uint64_t> &pos, std::vector<Fr> &val) {
    std::vector<std::pair<uint64_t, Fr>> v;
    for (uint64_t k = 0; k < opt.n_pi; k++) {
        if (opt.pi_pos[k] >= n)
            fail(PNP_E_ARG, "public input position %llu out of range", (unsigned long long)opt.pi_pos[k]);
        v.emplace_back(opt.pi_pos[k], to_mont(from_u64_limbs<FrP>(opt.pi_canon + 4 * k)));
    }
    std::sort(v.begin(), v.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    for (size_t k = 0; k < v.size(); k++) {
        if (k && v[k].first == v[k - 1].first)
            fail(PNP_E_ARG, "public input position %llu given twice", (unsigned long long)v[k].first);
        if (v[k].second.is_zero()) continue;
        pos.push_back(v[k].first);
        val.push_back(v[k].second);
    }
}

// the caller's columns, padded (context.h): Proof::load_witness and the check stage them alike
void stage_wire_columns(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, uint64_t *const dst[4], uint64_t ng,
                        uint64_t n, std::vector<H2D> &up) {
    const uint64_t *wsrc[4] = {cs->w_l, cs->w_r, cs->w_o, cs->w_4};
    for (int j = 0; j < 4; j++) {
        if (device_ptrs) PNP_HIP(hipMemcpyAsync(dst[j], wsrc[j], 32 * ng, hipMemcpyDeviceToDevice, ctx->stream));
        else up.push_back({dst[j], wsrc[j], 32 * ng});
        if (n > ng) PNP_HIP(hipMemsetAsync(dst[j] + 4 * ng, 0, 32 * (n - ng), ctx->stream));
    }
}

namespace {

// Round 5's evaluations (Montgomery).  kEvalTable below is their one list:
// where each goes in the proof and under which label into the transcript.
struct Evals {
    Fr a, b, c, d, sig1, sig2, sig3, perm;  // at z; perm: z at z w
    Fr f, q_lookup, z2_next, h1, h1_next, h2, table, table_next;
    Fr q_arith, q_c, q_l, q_r, q_hl, q_hr, q_h4, a_next, b_next, d_next;
};
struct EvalRow {
    const char *label;  // nullptr: in the proof only
    Fr Evals::*val;
    size_t dst;         // its offset in ProofEvaluationsC
};
#define PNP_EV(label, m, field) {label, &Evals::m, offsetof(ProofEvaluationsC, field)}
// in transcript order (gen_proof.cuh:373-403)
const EvalRow kEvalTable[] = {
    PNP_EV("a_eval", a, wire_evals.a_eval),
    PNP_EV("b_eval", b, wire_evals.b_eval),
    PNP_EV("c_eval", c, wire_evals.c_eval),
    PNP_EV("d_eval", d, wire_evals.d_eval),
    PNP_EV("left_sig_eval", sig1, perm_evals.left_sigma_eval),
    PNP_EV("right_sig_eval", sig2, perm_evals.right_sigma_eval),
    PNP_EV("out_sig_eval", sig3, perm_evals.out_sigma_eval),
    PNP_EV("perm_eval", perm, perm_evals.permutation_eval),
    PNP_EV("f_eval", f, lookup_evals.f_eval),
    PNP_EV("q_lookup_eval", q_lookup, lookup_evals.q_lookup_eval),
    PNP_EV("lookup_perm_eval", z2_next, lookup_evals.z2_next_eval),
    PNP_EV("h_1_eval", h1, lookup_evals.h1_eval),
    PNP_EV("h_1_next_eval", h1_next, lookup_evals.h1_next_eval),
    PNP_EV("h_2_eval", h2, lookup_evals.h2_eval),
    PNP_EV("q_arith_eval", q_arith, custom_evals.q_arith_eval),
    PNP_EV("q_c_eval", q_c, custom_evals.q_c_eval),
    PNP_EV("q_l_eval", q_l, custom_evals.q_l_eval),
    PNP_EV("q_r_eval", q_r, custom_evals.q_r_eval),
    PNP_EV("q_hl_eval", q_hl, custom_evals.q_hl_eval),
    PNP_EV("q_hr_eval", q_hr, custom_evals.q_hr_eval),
    PNP_EV("q_h4_eval", q_h4, custom_evals.q_h4_eval),
    PNP_EV("a_next_eval", a_next, custom_evals.a_next_eval),
    PNP_EV("b_next_eval", b_next, custom_evals.b_next_eval),
    PNP_EV("d_next_eval", d_next, custom_evals.d_next_eval),
    PNP_EV(nullptr, table, lookup_evals.table_eval),
    PNP_EV(nullptr, table_next, lookup_evals.table_next_eval),
};
#undef PNP_EV
static_assert(sizeof kEvalTable / sizeof kEvalTable[0] == sizeof(Evals) / sizeof(Fr) &&
                  sizeof(Evals) / sizeof(Fr) == sizeof(ProofEvaluationsC) / 32,
              "one row per evaluation of the proof");

// One proof in flight.  What a round leaves for later rounds is a member
// here, under the round that sets it; everything else is local to its round.
struct Proof {
    // ---- the call, the context and its streams (plan)
    pnp_ctx *const ctx;
    const CircuitC *const cs;  // nullptr with asg
    const int device_ptrs;
    ProofC *const out;
    const ProveOpts *const opt;
    const Assignment *const asg;
    hipStream_t s = nullptr, s_lo = nullptr;  // main; the low-priority side stream (s when !overlap)
    bool overlap = true, bg_mode = false;
    // ---- the domain
    uint64_t n = 1, ng = 0;
    uint32_t lg = 0;
    // ---- the sharding: this rank's coset blocks [mb0, mb0 + nb) and
    // coefficient range [q0, q0 + len); nbq0: the blocks round 4 first covers
    int world = 1, rank = 0, mb0 = 0, nb = 8, nbq0 = 8;
    bool dist = false;
    uint64_t NB = 0, q0 = 0, len = 0;
    // ---- the path flags: commitments from evaluations (round 1), the radix
    // 2^29 quotient, L1 (and one PI) on the coset in closed form (round 3)
    bool lag = false, q29 = false, closed = false, pi_closed = false;
    // ---- the public inputs: BTreeMap order, zero values dropped, Montgomery
    std::vector<uint64_t> pi_pos;
    std::vector<Fr> pi_val;
    Transcript tr;
    StageTimer tm;
    // ---- the witness (load_witness): padded columns; qlk: the q_lookup rows,
    // the first qlk_rows of them read (none: a zero column)
    uint64_t *wsc[4] = {}, *wpoly[4] = {};  // wire columns, wire coefficients (round 1)
    const uint64_t *qlk = nullptr;
    uint64_t qlk_rows = 0;
    double inputs_h2d = 0;
    // ---- round 1: the wire LDEs on this rank's blocks
    uint64_t *w8[4] = {};
    // ---- round 2: compressed table and query, their polynomials, h1 / h2
    Fr zeta;
    uint64_t *tc = nullptr, *fc = nullptr, *table_poly = nullptr, *f_poly = nullptr;
    uint64_t *h1 = nullptr, *h2 = nullptr, *h1_poly = nullptr, *h2_poly = nullptr;
    bool f_zero = false, table_zero = false, h_zero = false;  // h_zero: h1 = h2 = 0 and z2 = 1
    // ---- round 3
    Fr beta, gamma, delta, eps, bk[4], opd, eopd, n_inv;  // bk = beta k_j; opd = 1 + delta, eopd = eps opd
    uint64_t *z_poly = nullptr, *z8 = nullptr, *z2_poly = nullptr, *pi_poly = nullptr;
    // ---- round 4 (each attempt)
    Fr alpha, alpha2, range_c, logic_c, fixed_c, var_c, lsep, sep2, sep3;
    uint64_t *t_poly = nullptr;  // the chunks over [q0, q0 + len): t_poly[k len + u]
    // ---- round 5 (each attempt)
    Fr zc, zw;
    Evals ev;
    uint64_t *lin = nullptr;

    Proof(pnp_ctx *c, const CircuitC *cs_, int dp, ProofC *o, const ProveOpts *op, const Assignment *a)
        : ctx(c), cs(cs_), device_ptrs(dp), out(o), opt(op), asg(a), tr(op ? op->label : "Merkle tree"), tm(c) {}

    // The proof's algorithmic HBM bytes (the whole-proof GB/s
    // beside the wall-clock): every op credits its minimal reads and writes in
    // Fr elements (32 B); the MSMs credit their scalars and the accumulation
    // its device-counted entries in msm.hip (bench.py adds them up; DESIGN.md 5
    // states the tally)
    void alg(double elems) { ctx->ktimer.credit("proof_alg_bytes", 32.0 * elems); }
    // the side stream takes up after what the main stream has queued
    void fork() {
        if (!overlap) return;
        PNP_HIP(hipEventRecord(ctx->ev_fork, s));
        PNP_HIP(hipStreamWaitEvent(s_lo, ctx->ev_fork, 0));
    }
    // coset evaluations in block layout, the first nbq of this rank's blocks
    void lde(hipStream_t st, const uint64_t *coeffs, uint64_t *dst, int nbq, bool f29) {
        lde_blocks(ctx->ntt, coeffs, dst, lg, mb0, nbq, st, f29);
    }

    // a challenge, appended back under `as` (its own label unless given)
    Fr challenge(const char *label, const char *as = nullptr) {
        Fr c = tr.challenge_scalar(label);
        tr.append_scalar(as ? as : label, c);
        return c;
    }

    void check_and_size(), public_inputs(), plan(), load_witness();
    void round1_wires(), round2_lookup(), round3_permutation(), public_input_poly();
    QuotArgs quotient_args(int nbq);
    void quotient_launch(const QuotArgs &q, int nbq, uint64_t *t_blk);
    const unsigned *quotient_chunks(int nbq, uint64_t *t_blk);
    void commit_chunks(int nbq, const unsigned *t_nz);
    void round4_quotient(int nbq), extend_ldes(int nbq), evaluate_at_z(), round6_openings();
    bool round5_linearise(int nbq);
};

// the keys and the domain (prove_domain), the output and the stream
void Proof::check_and_size() {
    const ProveDomain dom = prove_domain(ctx, cs, asg, true);
    memset(out, 0, sizeof *out);
    s = ctx->stream;
    PNP_HIP(hipSetDevice(ctx->device));
    n = dom.n, lg = dom.lg, ng = dom.ng;
}

// public inputs: v1 = the circuit's one (pi, intended_pi_pos), appended as
// the reference GPU path does (transcript.cuh:39-44); v2 = a PublicInputs
// map (pi.rs:16-86): BTreeMap order, zero values dropped.  They open the
// transcript.
void Proof::public_inputs() {
    if (!opt) {
        if (cs->intended_pi_pos >= n || !cs->pi) fail(PNP_E_ARG, "public input position out of range");
        pi_pos.push_back(cs->intended_pi_pos);
        pi_val.push_back(to_mont(from_u64_limbs<FrP>(cs->pi)));
        tr.append_pi("pi", cs->pi, cs->intended_pi_pos);
        return;
    }
    public_input_map(*opt, n, pi_pos, pi_val);
    std::vector<uint64_t> canon(4 * pi_val.size());
    for (size_t k = 0; k < pi_val.size(); k++) to_u64_limbs(from_mont(pi_val[k]), &canon[4 * k]);
    tr.append_pis("pi", pi_pos.size(), pi_pos.data(), canon.data());
}

// table deferral, the HBM budget, the sharding and the paths this proof takes
void Proof::plan() {
    // Deferred tables (context.h): a proof that finds the optional tables
    // missing goes without them.  One GPU: on by default, the tables are only
    // built in the background, started when such a proof returns; several
    // ranks: off by default, the context's first proof only (every rank: the
    // same call sequence; hbm_budget checks the ranks agree)
    if (ctx->defer_tables < 0) ctx->defer_tables = ctx->msm.world <= 1 ? 1 : 0;
    bg_mode = ctx->msm.world <= 1 && tables_bg_enabled();
    ctx->defer_now = ctx->defer_tables == 1 && (bg_mode || ctx->proofs_started == 0);
    ctx->proofs_started++;
    ctx->tables_wanted = false;
    if (!ctx->hbm_checked) {  // the first proof after a key load: the HBM budget (every rank)
        hbm_budget(ctx);
        ctx->hbm_checked = true;
    }
    ctx->msm.batch_seq = 0;  // the fixed-slot exchange keys its capacities by batch ordinal
    tm.start();
    k_proof_marker(s);
    // the twiddle / twist tables are built lazily; build them here, on the main
    // stream, so the side-stream LDEs (after fork()) and the main-stream LDEs
    // both read finished tables
    ntt_warm(ctx->ntt, lg, s);
    // round-4 distribution (pnp_set_exchange_a2a, fixed at key load): this
    // rank's coset blocks [mb0, mb0 + nb) and coefficient range [q0, q0 + len)
    world = ctx->msm.world;
    rank = ctx->msm.rank;
    if (ctx->key.blk_world != world || ctx->key.blk_rank != rank)
        fail(PNP_E_ARG, "sharding changed after pnp_load_prover_key");
    mb0 = ctx->key.mb0;
    nb = ctx->key.nb;
    dist = nb < 8;
    NB = (uint64_t)nb * n;
    uint64_t q1 = n;
    if (dist) msm_point_range(n, rank, world, q0, q1);
    len = q1 - q0;
    // The round-4 coset LDEs of the wires and of z depend on no challenge:
    // they run on a low-priority side stream beside the round-1 / round-3
    // MSMs, whose sort, merge and tree phases leave most SIMDs idle, and the
    // quotient waits for them (PNP_NO_OVERLAP=1: in round 4, as before).
    static const bool overlap_on = getenv("PNP_NO_OVERLAP") == nullptr;
    overlap = overlap_on;
    s_lo = overlap ? ctx->side_stream() : s;
    // Round 4 on one GPU runs on the first 6 coset blocks, not all 8: the
    // quotient of a satisfying circuit has degree < 6n (the largest term,
    // q_arith q_hl a^5, has degree < 7n; the reference's t_7, t_8 are zero),
    // so its values on 6n points of the coset already determine it — 25% fewer
    // LDE transforms, quotient points and inverse transforms.  Round 5 checks
    // the quotient identity at the challenge z (lin(z) = -r_0, the verifier's
    // equation); a circuit the witness does not satisfy fails it and round 4
    // is redone on all 8 blocks, exactly the reference's computation.
    // (PNP_QUOT_BLOCKS = 6 .. 8; distributed round 4 keeps its 8 / world
    // blocks per rank.)
    static const int quot_blocks = [] {
        const char *e = getenv("PNP_QUOT_BLOCKS");
        int v = e ? atoi(e) : 6;
        return v < 6 ? 6 : v > 8 ? 8 : v;
    }();
    nbq0 = dist ? nb : quot_blocks;
    // The quotient of the common case (no custom gates, no lookup, the
    // standard coset: the Merkle circuit) runs in radix 2^29 (protocol.h
    // k_quotient29): its wire, z (and multi-PI) LDEs are taken in the 2^261
    // form (the scaled twist, free) and the key arrays it reads are the
    // 2^261-form copies made at key load; any other key keeps k_quotient_
    // (PNP_QUOT29=0: every key)
    q29 = ctx->key.q29;
    closed = ctx->key.std_coset;
    pi_closed = closed && pi_pos.size() == 1;
}

// ---------------- inputs: padded witness evaluations (pad_poly)
// from the caller's columns (copies and zero fills), or gathered from its
// variable assignment through the resident wire map (assignment.hip: one
// launch writes the columns and their padding)
void Proof::load_witness() {
    for (int j = 0; j < 4; j++) {
        wsc[j] = ctx->buf("wsc" + std::to_string(j), n);
        wpoly[j] = ctx->buf("wpoly" + std::to_string(j), n);
    }
    qlk_rows = ng;
    if (asg) {
        const uint64_t *vals = asg->values;
        if (!device_ptrs) {  // one staged upload (context.cpp h2d_batch)
            uint64_t *dv = ctx->buf("asg_values", asg->n_vars);
            h2d_batch(ctx, {{dv, vals, 32 * asg->n_vars}});
            inputs_h2d = 32.0 * asg->n_vars;
            vals = dv;
        }
        const uint32_t *dvar[4];
        ctx->key.wm_columns(dvar);
        hipEvent_t e0 = nullptr;
        ctx->ktimer.begin("gather_witness", s, e0);
        k_gather_witness(dvar, ng, vals, asg->n_vars, lg, wsc, s);
        ctx->ktimer.end("gather_witness", s, e0, 16.0 * ng + 4.0 * 32 * ng + 4.0 * 32 * n);
        if (ctx->key.wm_qlk.p) qlk = ctx->key.wm_qlk.u64();
        else qlk_rows = 0;
        alg(4.0 * (ng / 8.0 + ng + n));  // ids, gathered values, padded columns
    } else {
        std::vector<H2D> up;  // a host witness: staged uploads (context.cpp h2d_batch)
        stage_wire_columns(ctx, cs, device_ptrs, wsc, ng, n, up);
        uint64_t *q = ctx->buf("qlk", n);
        if (device_ptrs) PNP_HIP(hipMemcpyAsync(q, cs->q_lookup, 32 * ng, hipMemcpyDeviceToDevice, s));
        else up.push_back({q, cs->q_lookup, 32 * ng});
        if (!up.empty()) h2d_batch(ctx, up);
        qlk = q;
        alg(4.0 * (2 * ng + (n - ng)) + 2.0 * ng);
    }
    tm.mark("inputs");
}

// ---------------- round 1: witness polynomials (gen_proof.cuh:25-50)
// With the Lagrange-basis key the commitments are taken from the padded
// evaluations (the same points; zero rows drop out of the MSM,
// lagrange.hip), and the coefficients feed only the round-4 LDEs and
// round 5: the wires' iNTTs move to the side stream with the LDEs, off
// the commitments' path.  Without it the iNTTs stay on the main stream,
// and the side stream forks off for the LDEs once they are done.
void Proof::round1_wires() {
    lag = lagrange_table(ctx, n) != nullptr;
    for (int j = 0; j < 4; j++) w8[j] = ctx->buf("w8_" + std::to_string(j), NB);
    CommitmentC *wc[4] = {&out->a_comm, &out->b_comm, &out->c_comm, &out->d_comm};
    auto ldes = [&] {
        for (int j = 0; j < 4; j++) lde(s_lo, wpoly[j], w8[j], nbq0, q29);
        if (overlap) PNP_HIP(hipEventRecord(ctx->ev_w8, s_lo));
    };
    if (lag) fork();
    for (int j = 0; j < 4; j++) ntt_run(ctx->ntt, wpoly[j], lg, true, false, lag ? s_lo : s, wsc[j]);
    if (lag) ldes();
    alg(4.0 * 2 * n + 4.0 * (1 + nbq0) * n);  // 4 iNTTs, 4 LDEs onto nbq0 blocks
    tm.mark("r1_intt");
    if (lag) {
        // over the copy-constraint groups when the key has them and the
        // witness keeps them (wires.hip), else row by row
        const uint64_t *sc[4] = {wsc[0], wsc[1], wsc[2], wsc[3]};
        if (commit_wires_grouped(ctx, sc, n, wc)) alg(4.0 * n * 72 / 32);  // row, group, representative
        else commit_evals_batch(ctx, sc, 4, n, wc);
    } else {
        fork();
        ldes();
        const uint64_t *sc[4] = {wpoly[0], wpoly[1], wpoly[2], wpoly[3]};
        commit_affine_batch(ctx, sc, 4, n, wc);
    }
    append_comm(tr, "w_l", *wc[0]);
    append_comm(tr, "w_r", *wc[1]);
    append_comm(tr, "w_o", *wc[2]);
    append_comm(tr, "w_4", *wc[3]);
    tm.mark("r1_commit");
}

// ---------------- round 2: lookup (gen_proof.cuh:52-125)
void Proof::round2_lookup() {
    const ProverKeyC &pk = ctx->key.dev;
    zeta = challenge("zeta");
    tc = ctx->buf("tc", n), table_poly = ctx->buf("table_poly", n);
    k_compress4(tc, pk.table1, pk.table2, pk.table3, pk.table4, zeta, n, s);
    table_zero = !k_any_nonzero(tc, 4 * n, ctx->scratch_b, s);
    fc = ctx->buf("fc", n), f_poly = ctx->buf("f_poly", n);
    const uint64_t *wconst[4] = {wsc[0], wsc[1], wsc[2], wsc[3]};
    k_query_f(fc, qlk, qlk_rows, wconst, tc, zeta, n, s);
    f_zero = !k_any_nonzero(fc, 4 * n, ctx->scratch_b, s);
    alg(5.0 * n + n + ng + n + n);  // compress, its check, query (q_lookup in, f out), its check
    // (zero f / table: their polynomials are never read)
    if (!table_zero) ntt_run(ctx->ntt, table_poly, lg, true, false, s, tc);
    if (!f_zero) ntt_run(ctx->ntt, f_poly, lg, true, false, s, fc);
    // s = sorted concatenation of f and t, halves h1 / h2 (prover.rs:304-329).
    // f = t = 0 (the Merkle circuit): h1 = h2 = 0, commitments at infinity.
    // The f, h1, h2 MSMs are independent of the transcript in between, so
    // they run as one batch.
    h_zero = f_zero && table_zero;
    h1 = ctx->buf("h1", n), h2 = ctx->buf("h2", n);
    h1_poly = ctx->buf("h1_poly", n), h2_poly = ctx->buf("h2_poly", n);
    const uint64_t *sc[3];
    CommitmentC *oc[3];
    int nc = 0;
    if (f_zero) {
        set_infinity(&out->f_comm);
    } else {
        sc[nc] = f_poly;
        oc[nc++] = &out->f_comm;
    }
    if (h_zero) {
        PNP_HIP(hipMemsetAsync(h1, 0, 32 * n, s));
        PNP_HIP(hipMemsetAsync(h2, 0, 32 * n, s));
        alg(2.0 * n);
        set_infinity(&out->h_1_comm);
        set_infinity(&out->h_2_comm);
    } else {
        if (!combine_split(ctx, tc, fc, n, h1, h2, s))
            fail(PNP_E_ARG, "lookup: a query value is not in the lookup table (Error::ElementNotIndexed)");
        ntt_run(ctx->ntt, h1_poly, lg, true, false, s, h1);
        ntt_run(ctx->ntt, h2_poly, lg, true, false, s, h2);
        sc[nc] = h1_poly;
        oc[nc++] = &out->h_1_comm;
        sc[nc] = h2_poly;
        oc[nc++] = &out->h_2_comm;
    }
    if (nc) commit_affine_batch(ctx, sc, nc, n, oc);
    append_comm(tr, "f", out->f_comm);
    append_comm(tr, "h1", out->h_1_comm);
    append_comm(tr, "h2", out->h_2_comm);
    tm.mark("r2_lookup");
}

// ---------------- round 3: permutation (gen_proof.cuh:127-208)
// z (committed here), z2 (committed with the quotient chunks in round 4: it is
// not appended to the transcript, gen_proof.cuh:200-205), the public-input
// polynomial and its closed form on the coset
void Proof::round3_permutation() {
    beta = challenge("beta");
    gamma = challenge("gamma");
    delta = challenge("delta");
    eps = challenge("epsilon");
    if (beta == gamma || beta == delta || beta == eps || gamma == delta || gamma == eps || delta == eps)
        fail(PNP_E_ARG, "challenges must be different");  // gen_proof.cuh:152-157 asserts
    opd = delta + Fr::one();
    eopd = eps * opd;
    PermArgs pa;
    for (int j = 0; j < 4; j++) {
        pa.w[j] = wsc[j];
        pa.sigma[j] = ctx->key.sigma_n[j].u64();  // NTT.forward(sigma_polys[j]), cached at key load
    }
    const uint64_t kv[4] = {1, 7, 13, 17};  // K1..K3 (permutation/constants.cu:3-15)
    for (int j = 0; j < 4; j++) pa.bk[j] = bk[j] = beta * fr_from_u64(kv[j]);
    pa.beta = beta;
    pa.gamma = gamma;
    pa.omega = root_of_unity(lg);
    pa.tw = ntt_twiddles(ctx->ntt, lg, false, s);  // built by ntt_warm (plan)
    uint64_t *num = ctx->buf("num", n), *den = ctx->buf("den", n);
    z_poly = ctx->buf("z_poly", n);
    k_perm_numden(num, den, pa, n, s);
    k_batch_inverse(den, n, ctx->scratch_a, s);
    k_mul_inplace(num, den, n, s);
    k_prefix_product(num, n, ctx->scratch_a, s);
    alg(10.0 * n + 2.0 * n + 3.0 * n + 2.0 * n);  // numerators / denominators, inverse, product, scan
    alg(2.0 * n + (1.0 + nbq0) * n);              // z's iNTT and LDE
    z8 = ctx->buf("z8", NB);
    auto z_lde = [&] {
        lde(s_lo, z_poly, z8, nbq0, q29);
        if (overlap) PNP_HIP(hipEventRecord(ctx->ev_z8, s_lo));
    };
    // as in round 1: z from its evaluations, its iNTT joins its LDE on the
    // side stream; else from its coefficients, the side stream forks after
    if (lag) fork();
    ntt_run(ctx->ntt, z_poly, lg, true, false, lag ? s_lo : s, num);
    if (lag) z_lde();
    tm.mark("r3_z");
    if (lag) {
        const uint64_t *sc[1] = {num};
        CommitmentC *oc[1] = {&out->z_comm};
        // z is constant over runs of rows sigma fixes (the padding): one
        // scalar per run (wires.hip), else row by row
        if (commit_z_grouped(ctx, num, n, &out->z_comm)) alg(1.0 * n * 72 / 32);
        else commit_evals_batch(ctx, sc, 1, n, oc);
    } else {
        fork();
        z_lde();
        commit_affine(ctx, z_poly, n, &out->z_comm);
    }
    append_comm(tr, "z", out->z_comm);
    // lookup grand product (permutation/mod.rs:754-822)
    z2_poly = ctx->buf("z2_poly", n);
    // lookup-trivial case (f = t = h1 = h2 = 0): every ratio is
    // (1+d) e (e(1+d)) / (e(1+d))^2 = 1, so z2 = 1 and its coefficients are [1, 0, ...]
    if (h_zero) {
        uint64_t one[4];
        to_u64_limbs(Fr::one(), one);
        PNP_HIP(hipMemsetAsync(z2_poly, 0, 32 * n, s));
        PNP_HIP(hipMemcpyAsync(z2_poly, one, 32, hipMemcpyHostToDevice, s));
        PNP_HIP(hipStreamSynchronize(s));
    } else {
        // num is rewritten: the side stream's z iNTT must have read it
        if (lag && overlap) PNP_HIP(hipStreamWaitEvent(s, ctx->ev_z8, 0));
        k_lookup_nd(num, den, fc, tc, h1, h2, delta, eps, n, s);
        k_batch_inverse(den, n, ctx->scratch_a, s);
        k_mul_inplace(num, den, n, s);
        k_prefix_product(num, n, ctx->scratch_a, s);
        ntt_run(ctx->ntt, z2_poly, lg, true, false, s, num);
    }
    public_input_poly();
    tm.mark("r3_z2_pi");
}

// public input poly (pi.cu:11-15)
// = iNTT of the evaluations v * e_pos, in closed form: v n^-1 w^(-pos j);
// on the standard coset one PI needs no polynomial, only 1 / (x - w^pos)
void Proof::public_input_poly() {
    n_inv = inverse(fr_from_u64(n));
    if (pi_pos.size() == 1 && !closed) {
        pi_poly = ctx->buf("pi_poly", n);
        Fr w_inv_pos = pow_u64(inverse(root_of_unity(lg)), pi_pos[0]);
        k_geometric(pi_poly, n, pi_val[0] * n_inv, w_inv_pos, s);
    } else if (pi_pos.size() > 1) {  // iNTT of the sparse evaluations (pi.rs:76-86)
        pi_poly = ctx->buf("pi_poly", n);
        PNP_HIP(hipMemsetAsync(pi_poly, 0, 32 * n, s));
        std::vector<uint64_t> limbs(4 * pi_val.size());
        for (size_t k = 0; k < pi_val.size(); k++) to_u64_limbs(pi_val[k], &limbs[4 * k]);
        for (size_t k = 0; k < pi_val.size(); k++)
            PNP_HIP(hipMemcpyAsync(pi_poly + 4 * pi_pos[k], &limbs[4 * k], 32, hipMemcpyHostToDevice, s));
        PNP_HIP(hipStreamSynchronize(s));
        ntt_run(ctx->ntt, pi_poly, lg, true, false, s);
    }
    if (pi_closed && ctx->key.pinv_pos != pi_pos[0]) {
        // 1 / (x_i - w^pos) on this rank's blocks, kept across proofs with the
        // same PI position
        ctx->key.pinv_pos = ~0ULL;
        ctx->key.pinv.reserve(32 * NB);
        Fr wpos = pow_u64(root_of_unity(lg), pi_pos[0]);
        k_affine(ctx->key.pinv.u64(), ctx->key.blk[kLin].u64(), Fr::one(), neg(wpos), NB, s);
        k_batch_inverse(ctx->key.pinv.u64(), NB, ctx->scratch_a, s);
        ctx->key.pinv_pos = pi_pos[0];
    }
}

// ---------------- round 4: quotient (gen_proof.cuh:209-267, quotient.cu:142-376)
// The remaining LDEs onto nbq blocks (main stream; the wires' and z's were
// forked off in rounds 1 and 3) and the quotient's arguments.  nullptr = known
// zero, not read (protocol.h)
QuotArgs Proof::quotient_args(int nbq) {
    const ResidentKey &key = ctx->key;
    // the LDE of `poly` onto this rank's blocks, into the working buffer `name`
    auto lde_to = [&](const char *name, const uint64_t *poly, bool f29) {
        uint64_t *dst = ctx->buf(name, NB);
        lde(s, poly, dst, nbq, f29);
        return dst;
    };
    QuotArgs q{};
    for (int j = 0; j < 4; j++) q.w8[j] = w8[j];
    uint64_t *z28 = ctx->buf("z28", NB);
    q.z8 = z8;
    if (closed) q.l1v = key.blk[kL1v].u64();
    if (pi_closed) {
        q.pinv = key.pinv.u64();
        q.c_pi = pi_val[0] * pow_u64(root_of_unity(lg), pi_pos[0]) * n_inv;
    } else if (pi_poly) {
        q.pi8 = lde_to("pi8", pi_poly, q29);
    }
    if (!h_zero) {  // else z2 = 1: its quotient terms cancel (protocol.h)
        lde(s, z2_poly, z28, nbq, false);
        q.z28 = z28;
    }
    if (!f_zero) q.f8 = lde_to("f8", f_poly, false);
    if (!table_zero) q.t8 = lde_to("t8", table_poly, false);
    if (!h_zero) {  // else h1 = h2 = 0
        q.h18 = lde_to("h18", h1_poly, false);
        q.h28 = lde_to("h28", h2_poly, false);
    }
    // compute_first_lagrange_poly_scaled(n, alpha^2) and (n, 1) (quotient.cu:3-8):
    // one LDE of L1 (coefficients n^-1, no iNTT); alpha^2 is applied in the kernel
    if (!closed) {
        uint64_t *l1 = ctx->buf("l1", n);
        k_geometric(l1, n, n_inv, Fr::one(), s);
        q.l18 = lde_to("l18", l1, false);
    }
    // prover-key evaluations: block-layout copies made at key load, the 2^261
    // forms for k_quotient29 (nullptr = zero selector)
    auto kb = [&](int r) { return key.key_block(KeyPoly(r)); };
    q.q_m = kb(kQm), q.q_l = kb(kQl), q.q_r = kb(kQr), q.q_o = kb(kQo), q.q_4 = kb(kQ4), q.q_c = kb(kQc);
    q.q_hl = kb(kQhl), q.q_hr = kb(kQhr), q.q_h4 = kb(kQh4), q.q_arith = kb(kQarith), q.q_lookup = kb(kQlookup);
    for (int j = 0; j < 4; j++) q.sig[j] = kb(kSig0 + j);
    q.lin = kb(kLin);
    q.vh_inv = kb(kVhInv);  // v_h^-1, computed at key load
    q.n = n, q.lg_n = lg;
    q.alpha = alpha, q.alpha2 = alpha2, q.beta = beta, q.gamma = gamma, q.delta = delta, q.eps = eps;
    q.zeta = zeta, q.lsep = lsep, q.opd = opd, q.eopd = eopd, q.sep2 = sep2, q.sep3 = sep3;
    for (int j = 0; j < 4; j++) q.bk[j] = bk[j];
    return q;
}

// k_quotient29's arguments: QuotArgs' arrays (the key's are its 2^261 copies,
// key_block) and the constants as nine 29-bit limbs
Quot29Args quotient29_args(const QuotArgs &q) {
    Quot29Args q2;
    for (int j = 0; j < 4; j++) q2.w8[j] = q.w8[j];
    q2.z8 = q.z8;
    q2.pi8 = q.pi8;
    q2.q_m = q.q_m, q2.q_l = q.q_l, q2.q_r = q.q_r, q2.q_o = q.q_o, q2.q_4 = q.q_4, q2.q_c = q.q_c;
    q2.q_hl = q.q_hl, q2.q_hr = q.q_hr, q2.q_h4 = q.q_h4, q2.q_arith = q.q_arith;
    for (int j = 0; j < 4; j++) q2.sig[j] = q.sig[j];
    q2.lin = q.lin;
    q2.vh_inv = q.vh_inv;
    q2.l1v = q.l1v;
    q2.pinv = q.pinv;
    fr_to_r29_limbs(q.pinv ? q.c_pi : Fr::zero(), q2.c_pi);
    fr_to_r29_limbs(q.alpha, q2.alpha);
    fr_to_r29_limbs(q.alpha2, q2.alpha2);
    fr_to_r29_limbs(q.beta, q2.beta);
    fr_to_r29_limbs(q.gamma, q2.gamma);
    fr_to_r29_limbs(Fr::one(), q2.one);
    q2.n = q.n;
    q2.lg_n = q.lg_n;
    if (!q2.l1v || !q2.q_l || !q2.lin || !q2.sig[3]) fail(PNP_E_ARG, "quotient29: key copies missing");
    return q2;
}

// the quotient over nbq blocks into t_blk (and the custom gates' terms), with
// its timer and credits
void Proof::quotient_launch(const QuotArgs &q, int nbq, uint64_t *t_blk) {
    const uint64_t NBq = (uint64_t)nbq * n;
    hipEvent_t qe0 = nullptr;
    ctx->ktimer.begin("quotient", s, qe0);
    if (q29) {
        k_quotient29(quotient29_args(q), NBq, t_blk, s);
        // VALU work for bench.py's roofline: Fr products per point on the
        // path this launch takes (protocol.hip k_quotient29_: 5 paired
        // products = 10, three fifth powers = 9, 14 more; + 2 with q_m, + 1
        // with the closed-form PI)
        ctx->ktimer.credit("quotient_points", (double)NBq);
        ctx->ktimer.credit("quotient_fr_products", (double)NBq * (34 + (q.q_m ? 2 : 0) + (q.pinv ? 1 : 0)));
    } else {
        k_quotient(q, NBq, t_blk, s);
    }
    if (ctx->key.any_custom()) {
        WidgetArgs g;
        for (int j = 0; j < 4; j++) g.w8[j] = q.w8[j];
        g.q_l = q.q_l, g.q_r = q.q_r, g.q_c = q.q_c, g.vh_inv = q.vh_inv;
        // range, logic, fixed-base, curve-add
        for (int k = 0; k < 4; k++) g.sel[k] = ctx->key.key_block(KeyPoly(kRange + k));
        g.sep[0] = range_c, g.sep[1] = logic_c, g.sep[2] = fixed_c, g.sep[3] = var_c;
        g.n = n, g.lg_n = lg;
        k_widgets(g, NBq, t_blk, s);
    }
    // algorithmic bytes: every coset array the kernel reads (nullptr = known
    // zero, not read) plus t, 32 B per point each
    const uint64_t *arrs[] = {q.w8[0], q.w8[1], q.w8[2], q.w8[3], q.q_m, q.q_l, q.q_r, q.q_o,
                              q.q_4, q.q_c, q.q_hl, q.q_hr, q.q_h4, q.q_arith, q.pi8, q.lin,
                              q.z8, q.sig[0], q.sig[1], q.sig[2], q.sig[3], q.f8,
                              q.t8, q.h18, q.h28, q.q_lookup, q.z28, q.l18, q.vh_inv, q.l1v, q.pinv};
    int nread = 0;
    for (const uint64_t *a : arrs) nread += a != nullptr;
    ctx->ktimer.end("quotient", s, qe0, 32.0 * (double)NBq * (nread + 1));
    alg((double)NBq * (nread + 1));
}

// Intt_coset of the coset values: per block an unscaled size-n inverse
// transform and a twist, then per coefficient index an inverse DFT (8
// blocks, ntt.hip t_combine) or Vandermonde solve (6 / 7 blocks,
// t_combine_blocks) across the blocks -> the chunks t_1..t_8, here over
// this rank's coefficient range [q0, q0 + len): t_poly[k len + u]; with
// nbq < 8 blocks the chunks from t_(nbq+1) on are zero.  Returns the device
// word whose bit k the combine set when chunk k != 0
const unsigned *Proof::quotient_chunks(int nbq, uint64_t *t_blk) {
    const uint64_t NBq = (uint64_t)nbq * n;
    intt_blocks(ctx->ntt, t_blk, lg, mb0, nbq, s);
    alg(2.0 * NBq + 2.0 * NBq);  // the block iNTTs and the combine
    t_poly = ctx->buf("t_poly", 8 * len);
    unsigned *t_nz = reinterpret_cast<unsigned *>(ctx->buf("t_nz", 1));
    PNP_HIP(hipMemsetAsync(t_nz, 0, 4, s));
    if (!dist) {
        t_combine_blocks(ctx->ntt, t_blk, nbq, t_poly, lg, t_nz, s);
        return t_nz;
    }
    // all-to-all: rank r' receives, from every rank, that rank's blocks
    // restricted to r''s coefficient range; slots arrive block-major
    const uint64_t slot = (uint64_t)nb * len * 32;
    if (!ctx->msm.alltoall || ctx->msm.a2a_bytes < 2 * slot * world)
        fail(PNP_E_ARG, "round-4 all-to-all buffer missing or < %llu B", (unsigned long long)(2 * slot * world));
    uint64_t *a2a = ctx->msm.a2a;
    for (int r = 0; r < world; r++) {
        uint64_t r0, r1;
        msm_point_range(n, r, world, r0, r1);
        for (int b = 0; b < nb; b++)
            PNP_HIP(hipMemcpyAsync(a2a + 4 * ((uint64_t)(r * nb + b) * len), t_blk + 4 * ((uint64_t)b * n + r0),
                                   32 * len, hipMemcpyDeviceToDevice, s));
    }
    ex_fence(ctx->msm, s);
    int rc = ctx->msm.alltoall(ctx->msm.a2a_user, slot);
    if (rc != 0) fail(PNP_E_DEVICE, "round-4 all-to-all callback failed (%d)", rc);
    t_combine(ctx->ntt, a2a + 4 * (uint64_t)nb * len * world, len, q0, t_poly, lg, t_nz, s);
    return t_nz;
}

// t_1 .. t_8 and z2 in one batched MSM.  Chunks that are identically zero
// (t_7, t_8 for a satisfying circuit: deg t < 6n) commit to the point at
// infinity without an MSM
void Proof::commit_chunks(int nbq, const unsigned *t_nz) {
    CommitmentC *tcm[8] = {&out->t_1_comm, &out->t_2_comm, &out->t_3_comm, &out->t_4_comm,
                           &out->t_5_comm, &out->t_6_comm, &out->t_7_comm, &out->t_8_comm};
    const int npieces = dist ? 8 : nbq;
    const uint64_t *sc[9];
    CommitmentC *oc[9];
    int nc = 0;
    uint64_t nz[8];
    unsigned bits = 0;  // flagged by the combine kernel as it wrote the chunks
    PNP_HIP(hipMemcpyAsync(&bits, t_nz, 4, hipMemcpyDeviceToHost, s));
    PNP_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < 8; k++) nz[k] = k < npieces && ((bits >> k) & 1);
    if (dist) {  // a chunk is zero when it is zero on every rank (own slot included)
        std::vector<uint64_t> all = shard_allgather(ctx, nz, 8, PNP_EX_TAG_T_FLAGS);
        for (int k = 0; k < 8; k++) {
            nz[k] = 0;
            for (int r = 0; r < world; r++) nz[k] |= all[8 * r + k];
        }
    }
    for (int k = 0; k < 8; k++) {
        if (!nz[k]) {
            set_infinity(tcm[k]);
            continue;
        }
        sc[nc] = t_poly + 4 * (uint64_t)k * len;
        oc[nc++] = tcm[k];
    }
    if (h_zero) {
        // z2 = 1: commit([1, 0, ...]) = 1 * powers_of_g[0], already affine
        uint64_t g0[12];
        PNP_HIP(hipMemcpyAsync(g0, ctx->ck_dev, sizeof g0, hipMemcpyDeviceToHost, s));
        PNP_HIP(hipStreamSynchronize(s));
        memcpy(out->z_2_comm.x, g0, 48);
        memcpy(out->z_2_comm.y, g0 + 6, 48);
    } else if (dist) {
        commit_affine(ctx, z2_poly, n, &out->z_2_comm);
    } else {
        sc[nc] = z2_poly;
        oc[nc++] = &out->z_2_comm;
    }
    // distributed: the chunks hold this rank's coefficient range only,
    // exactly the point range of its MSM share
    commit_affine_batch(ctx, sc, nc, n, oc, dist);
    const char *tl[8] = {"t_1", "t_2", "t_3", "t_4", "t_5", "t_6", "t_7", "t_8"};
    for (int k = 0; k < 8; k++) append_comm(tr, tl[k], *tcm[k]);
}

// one attempt over nbq blocks (a satisfying circuit: the only one; see plan)
void Proof::round4_quotient(int nbq) {
    alpha = challenge("alpha");
    // (appended under the reference's spelling)
    range_c = challenge("range separation challenge", "range seperation challenge");
    logic_c = challenge("logic separation challenge", "logic seperation challenge");
    fixed_c = challenge("fixed base separation challenge");
    var_c = challenge("variable base separation challenge");
    lsep = challenge("lookup separation challenge");
    alpha2 = alpha * alpha;
    sep2 = lsep * lsep;
    sep3 = sep2 * lsep;

    const QuotArgs q = quotient_args(nbq);
    if (overlap) {  // the side-stream LDEs of the wires and z
        PNP_HIP(hipStreamWaitEvent(s, ctx->ev_w8, 0));
        PNP_HIP(hipStreamWaitEvent(s, ctx->ev_z8, 0));
    }
    tm.mark("r4_lde");
    uint64_t *t_blk = ctx->buf("t_blk", NB);
    quotient_launch(q, nbq, t_blk);
    tm.mark("r4_quotient");
    const unsigned *t_nz = quotient_chunks(nbq, t_blk);
    tm.mark("r4_intt8");
    commit_chunks(nbq, t_nz);
    tm.mark("r4_commit");
    ctx->ktimer.collect();  // the quotient's events (the commitments' read-back drained the stream)
}

// ---------------- round 5: linearisation (linearisation.cu:73-306)
// The evaluations at z and z w into ev.  (Distributed: every rank evaluates
// its coefficient range [q0, q0 + len) of these replicated polynomials,
// scales by x^q0, and one all-gather of the 18 partial values sums them.)
void Proof::evaluate_at_z() {
    const ProverKeyC &pk = ctx->key.dev;
    const uint64_t eo = 4 * q0;
    const uint64_t *pz[12] = {wpoly[0] + eo, wpoly[1] + eo, wpoly[2] + eo, wpoly[3] + eo,
                              pk.left_sigma_coeffs + eo, pk.right_sigma_coeffs + eo,
                              pk.out_sigma_coeffs + eo, pk.q_arith_coeffs + eo, pk.q_c_coeffs + eo,
                              pk.q_l_coeffs + eo, pk.q_r_coeffs + eo, pk.q_hl_coeffs + eo};
    const uint64_t *pz2[2] = {pk.q_hr_coeffs + eo, pk.q_h4_coeffs + eo};
    // evaluations at z * omega
    const uint64_t *pw[4] = {z_poly + eo, wpoly[0] + eo, wpoly[1] + eo, wpoly[3] + eo};
    Fr r[18], *const rz = r, *const rz2 = r + 12, *const rw = r + 14;
    const EvalSet sets[3] = {{pz, 12, zc, rz}, {pz2, 2, zc, rz2}, {pw, 4, zw, rw}};
    k_poly_eval_sets(sets, 3, len, ctx->scratch_a, s);  // one host round trip
    alg(18.0 * len);
    if (dist) {
        const Fr sz = pow_u64(zc, q0), sw = pow_u64(zw, q0);
        uint64_t mine[4 * 18];
        for (int k = 0; k < 18; k++) to_u64_limbs(r[k] * (k < 14 ? sz : sw), mine + 4 * k);
        std::vector<uint64_t> all = shard_allgather(ctx, mine, 4 * 18, PNP_EX_TAG_EVALS);
        for (int k = 0; k < 18; k++) {
            r[k] = Fr::zero();
            for (int j = 0; j < world; j++) r[k] += from_u64_limbs<FrP>(&all[4 * (18 * j + k)]);
        }
    }
    ev.a = rz[0], ev.b = rz[1], ev.c = rz[2], ev.d = rz[3];
    ev.sig1 = rz[4], ev.sig2 = rz[5], ev.sig3 = rz[6], ev.perm = rw[0];
    ev.q_arith = rz[7], ev.q_c = rz[8], ev.q_l = rz[9], ev.q_r = rz[10], ev.q_hl = rz[11];
    ev.q_hr = rz2[0], ev.q_h4 = rz2[1];
    ev.a_next = rw[1], ev.b_next = rw[2], ev.d_next = rw[3];
    // the lookup's: zero (z2: one) where the polynomial is
    ev.z2_next = Fr::one();
    if (!h_zero) k_poly_eval(z2_poly, n, zw, ctx->scratch_a, &ev.z2_next, s);
    ev.f = ev.table = ev.table_next = ev.q_lookup = ev.h1 = ev.h1_next = ev.h2 = Fr::zero();
    if (!ctx->key.qlookup_zero()) k_poly_eval(pk.q_lookup_coeffs, n, zc, ctx->scratch_a, &ev.q_lookup, s);
    if (!h_zero) {
        k_poly_eval(h1_poly, n, zc, ctx->scratch_a, &ev.h1, s);
        k_poly_eval(h1_poly, n, zw, ctx->scratch_a, &ev.h1_next, s);
        k_poly_eval(h2_poly, n, zc, ctx->scratch_a, &ev.h2, s);
    }
    if (!f_zero) k_poly_eval(f_poly, n, zc, ctx->scratch_a, &ev.f, s);
    if (!table_zero) {
        k_poly_eval(table_poly, n, zc, ctx->scratch_a, &ev.table, s);
        k_poly_eval(table_poly, n, zw, ctx->scratch_a, &ev.table_next, s);
    }
    uint64_t *dst = reinterpret_cast<uint64_t *>(&out->evaluations);
    for (const EvalRow &r : kEvalTable) to_u64_limbs(ev.*r.val, dst + r.dst / 8);
}

// The linearisation polynomial over this rank's range and, where round 4 ran
// on fewer than 8 blocks, the quotient identity at z.  False: the identity
// failed and nothing of this attempt may reach the transcript
bool Proof::round5_linearise(int nbq) {
    const ProverKeyC &pk = ctx->key.dev;
    const ResidentKey &key = ctx->key;
    zc = challenge("z");
    const Fr omega = root_of_unity(lg);
    zw = zc * omega;
    const Fr vh = pow_u64(zc, n) - Fr::one();
    const Fr zn = vh + Fr::one();
    const Fr l1e = vh * inverse(fr_from_u64(n) * (zc - Fr::one()));
    evaluate_at_z();
    tm.mark("r5_evals");
    LinArgs la;
    la.k = 0;
    // over this rank's coefficient range (replicated polynomials offset by q0)
    auto push_local = [&](const uint64_t *p, const Fr &sc) {
        la.p[la.k] = p;
        la.s[la.k] = sc;
        la.k++;
    };
    auto push = [&](const uint64_t *p, const Fr &sc) { push_local(p + 4 * q0, sc); };
    auto p5 = [](const Fr &x) { Fr x2 = x * x; return x2 * x2 * x; };
    // arithmetic (widget/arithmetic.rs:82-100)
    if (!key.qm_zero()) push(pk.q_m_coeffs, ev.a * ev.b * ev.q_arith);
    push(pk.q_l_coeffs, ev.a * ev.q_arith);
    push(pk.q_r_coeffs, ev.b * ev.q_arith);
    push(pk.q_o_coeffs, ev.c * ev.q_arith);
    push(pk.q_4_coeffs, ev.d * ev.q_arith);
    push(pk.q_hl_coeffs, p5(ev.a) * ev.q_arith);
    push(pk.q_hr_coeffs, p5(ev.b) * ev.q_arith);
    push(pk.q_h4_coeffs, p5(ev.d) * ev.q_arith);
    push(pk.q_c_coeffs, ev.q_arith);
    // custom gates (linearisation_poly.rs:396-430): selector * constraints(evals)
    const WidgetVals wv{ev.a, ev.b, ev.c, ev.d, ev.a_next, ev.b_next, ev.d_next, ev.q_l, ev.q_r, ev.q_c};
    if (key.custom(0)) push(pk.range_selector_coeffs, w_range(range_c, wv));
    if (key.custom(1)) push(pk.logic_selector_coeffs, w_logic(logic_c, wv));
    if (key.custom(2)) push(pk.fixed_group_add_selector_coeffs, w_fbsm(fixed_c, wv));
    if (key.custom(3)) push(pk.variable_group_add_selector_coeffs, w_cadd(var_c, wv));
    // compute_linearisation_permutation (proof_system/permutation.cu:231-265);
    // perm3: the product over the first three sigmas, shared with the identity below
    const Fr perm3 =
        (ev.a + beta * ev.sig1 + gamma) * (ev.b + beta * ev.sig2 + gamma) * (ev.c + beta * ev.sig3 + gamma);
    const Fr bz = beta * zc;
    const Fr pa = (ev.a + bz + gamma) * (ev.b + fr_from_u64(7) * bz + gamma) *
                  (ev.c + fr_from_u64(13) * bz + gamma) * (ev.d + fr_from_u64(17) * bz + gamma) * alpha;
    push(z_poly, pa + l1e * alpha2);
    push(pk.fourth_sigma_coeffs, neg(perm3 * (beta * ev.perm) * alpha));
    // lookup (widget/lookup.rs:137-182)
    if (!key.qlookup_zero()) {
        Fr ct = ((ev.d * zeta + ev.c) * zeta + ev.b) * zeta + ev.a;
        push(pk.q_lookup_coeffs, (ct - ev.f) * lsep);
    }
    const Fr b0 = eps + ev.f, b1 = eopd + ev.table + delta * ev.table_next;
    push(z2_poly, opd * b0 * b1 * sep2 + l1e * sep3);
    if (!h_zero) push(h1_poly, neg(ev.z2_next) * sep2 * (eopd + ev.h2 + delta * ev.h1_next));
    // - Z_H(z) * sum_k z^(kn) t_(k+1)  (linearisation.cu:250-292)
    Fr tk = neg(vh);
    for (int k = 0; k < (dist ? 8 : nbq); k++) {
        push_local(t_poly + 4 * (uint64_t)k * len, tk);  // t_poly is range-local
        tk = tk * zn;
    }
    lin = ctx->buf("lin", len);
    k_lincomb(la, len, lin, s);
    alg((la.k + 1.0) * len);
    if (!dist && nbq < 8) {
        // the verifier's equation (proof.rs:433-494, oracle/verifier.c): for the
        // true quotient lin(z) = -r_0; otherwise the witness does not satisfy
        // the circuit, t has degree >= nbq n and round 4 runs again on all 8
        // blocks (a false pass needs z to be a root of a nonzero polynomial of
        // degree < 8n: probability < 2^-228 over the transcript hash)
        Fr lin_z;
        k_poly_eval(lin, len, zc, ctx->scratch_a, &lin_z, s);
        Fr pie = Fr::zero();
        const Fr w_inv = inverse(omega);
        for (size_t k = 0; k < pi_pos.size(); k++)
            pie += pi_val[k] * inverse(pow_u64(w_inv, pi_pos[k]) * zc - Fr::one());
        pie = pie * vh * n_inv;
        const Fr b = perm3 * (ev.d + gamma) * ev.perm * alpha;
        const Fr d = sep2 * ev.z2_next * (eopd + delta * ev.h2) * (eopd + ev.h2 + delta * ev.h1_next);
        const Fr r0 = pie - b - l1e * alpha2 - d - sep3 * l1e;
        if (!(lin_z + r0).is_zero()) return false;
    }
    tm.mark("r5_lin");
    for (const EvalRow &r : kEvalTable)
        if (r.label) tr.append_scalar(r.label, ev.*r.val);
    return true;
}

// after a failed identity: the wire and z LDEs on the blocks nbq .. 7 the
// first attempt left out (the other LDEs are redone by quotient_args)
void Proof::extend_ldes(int nbq) {
    ctx->ktimer.credit("quotient_all_blocks", 1);
    const uint64_t off = 4 * (uint64_t)nbq * n;
    for (int j = 0; j < 4; j++) lde_blocks(ctx->ntt, wpoly[j], w8[j] + off, lg, nbq, 8 - nbq, s, q29);
    lde_blocks(ctx->ntt, z_poly, z8 + off, lg, nbq, 8 - nbq, s, q29);
}

// ---------------- round 6: openings (gen_proof.cuh:405-463, kzg10.cu:116-145)
// Both "aggregate_witness" challenges are squeezed back to back in the
// reference (nothing is appended in between), so both witness
// polynomials are built first and committed in one batched MSM.
void Proof::round6_openings() {
    const ProverKeyC &pk = ctx->key.dev;
    uint64_t *comb = ctx->buf("comb", len), *comb2 = ctx->buf("comb2", len);
    Fr aw = tr.challenge_scalar("aggregate_witness");
    Fr saw = tr.challenge_scalar("aggregate_witness");
    // dst = sum_k c^k polys[k] over this rank's range; a nullptr entry is a zero
    // polynomial (it keeps its power of c); returns the terms read
    auto aggregate = [&](std::initializer_list<const uint64_t *> polys, const Fr &c, uint64_t *dst) {
        LinArgs oa;
        oa.k = 0;
        Fr p = Fr::one();
        for (const uint64_t *poly : polys) {
            if (poly) {
                oa.p[oa.k] = poly;
                oa.s[oa.k] = p;
                oa.k++;
            }
            p = p * c;
        }
        k_lincomb(oa, len, dst, s);
        return oa.k;
    };
    auto at = [&](const uint64_t *poly, bool zero = false) { return zero ? nullptr : poly + 4 * q0; };
    int k = aggregate({lin /* range-local */, at(pk.left_sigma_coeffs), at(pk.right_sigma_coeffs),
                       at(pk.out_sigma_coeffs), at(f_poly, f_zero), at(h2_poly, h_zero), at(table_poly, table_zero),
                       at(wpoly[0]), at(wpoly[1]), at(wpoly[2]), at(wpoly[3])},
                      aw, comb);
    alg((k + 1.0) * len);
    k = aggregate({at(z_poly), at(wpoly[0]), at(wpoly[1]), at(wpoly[3]), at(h1_poly, h_zero), at(z2_poly),
                   at(table_poly, table_zero)},
                  saw, comb2);
    alg((k + 1.0) * len + 4.0 * len);  // + both divisions
    uint64_t *dd[2] = {comb, comb2};
    const Fr zz[2] = {zc, zw};
    div_linear_range(ctx, dd, zz, 2, len, dist);
    tm.mark("r6_witness");
    const uint64_t *sc[2] = {comb, comb2};
    CommitmentC *oc[2] = {&out->aw_opening, &out->saw_opening};
    commit_affine_batch(ctx, sc, 2, n, oc, dist);
    tm.mark("r6_commit");
}

}  // namespace

// The protocol.  Round 4 runs on nbq0 blocks and round 5 checks the quotient
// identity; only when it fails (a witness that does not satisfy the circuit)
// are both repeated, on all 8 blocks and from the transcript as round 3 left it.
void prove_impl(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, ProofC *out, const ProveOpts *opt,
                const Assignment *asg) {
    struct DeferScope {  // the table deferral (plan) is this proof's only, on every exit
        pnp_ctx *c;
        ~DeferScope() { c->defer_now = false; }
    } defer_scope{ctx};
    Proof p(ctx, cs, device_ptrs, out, opt, asg);
    p.check_and_size();
    p.public_inputs();
    p.plan();
    p.load_witness();
    p.round1_wires();
    p.round2_lookup();
    p.round3_permutation();
    const Transcript tr3 = p.tr;  // before the round-4 challenges
    int nbq = p.nbq0;             // blocks this round-4 attempt covers
    p.round4_quotient(nbq);
    if (!p.round5_linearise(nbq)) {
        p.extend_ldes(nbq);
        p.tr = tr3;
        nbq = 8;
        p.round4_quotient(nbq);
        p.round5_linearise(nbq);  // all 8 blocks: nothing to check
    }
    p.round6_openings();
    // the tables this proof went without: built in the background from now
    if (p.bg_mode && ctx->defer_now && ctx->tables_wanted) tables_start_background(ctx, p.n);
    // a count in the same list (an assignment proof only): what its witness moved over PCIe
    if (asg) ctx->stages.emplace_back("inputs_h2d_bytes", p.inputs_h2d);
}

}  // namespace pnp
