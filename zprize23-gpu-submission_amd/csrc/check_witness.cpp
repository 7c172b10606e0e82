// check_witness.cpp — the satisfiability check of a witness against the
// resident key, row by row: the host driver of pnp_check_assignment and
// pnp_check_witness (abi.cpp checks their arguments) over the kernels of
// check.hip.  Nothing here is kept: every device buffer of a check is released
// when the call returns, whatever way it returns.
//
// A call, in order:
//   begin          the report zeroed; a sharded context refused; the prologue a
//                  proof runs (prove_domain, public_input_map) without a commit
//                  key; the stage clock started; the four padded columns
//   the columns    check_assignment gathers them through the resident wire map
//                  (assignment.hip), check_witness stages the caller's and its
//                  q_lookup rows as the prover does        -> "check_inputs"
//   selector_rows  forward transforms of the resident coefficients, of the
//                  selectors this key has; the public inputs -> "check_rows_ntt"
//   gates          arithmetic + PI on every row, a custom family only when the
//                  key has it                              -> "check_rows"
//   lookup         when the caller or the key selects a row -> "check_lookup"
//   copy           the columns against the wire map (check_witness with a map
//                  resident)                               -> "check_copy"
//   report         the record to the host; PNP_E_UNSAT with the first violated
//                  row in the message
#include <string.h>
#include "context.h"

namespace pnp {
namespace {

const char *const kCheckKindName[PNP_CHECK_KINDS] = {"arith", "range", "logic", "fixed_add",
                                                    "var_add", "lookup", "copy"};

// what the kernels left (CheckRecord) as the caller reads it; unsatisfied: the message
pnp_check_report check_report(const CheckRecord &h, uint32_t copy_checked) {
    pnp_check_report rep;
    memset(&rep, 0, sizeof rep);
    rep.first_row = ~0ULL;
    rep.copy_checked = copy_checked;
    for (int k = 0; k < PNP_CHECK_KINDS; k++) {
        rep.by_kind[k] = h.by_kind[k];
        rep.violations += h.by_kind[k];
    }
    if (rep.violations) {
        rep.first_row = h.first >> 8;
        rep.first_kind = (uint32_t)(h.first >> 4) & 15;
        rep.first_index = (uint32_t)h.first & 15;
        set_error("row %llu: %s constraint %u (%llu violations)", (unsigned long long)rep.first_row,
                  kCheckKindName[rep.first_kind], rep.first_index, (unsigned long long)rep.violations);
    }
    return rep;
}

// One check in flight.
struct Check {
    pnp_ctx *const ctx;
    const ProveOpts opt;
    pnp_check_report *const report;
    ProveDomain dom;
    hipStream_t s = nullptr;
    std::vector<uint64_t> pi_pos;
    std::vector<Fr> pi_val;
    DevBuf col[4];  // the padded witness columns, D rows each
    StageTimer tm;

    Check(pnp_ctx *c, const ProveOpts &pis, pnp_check_report *r) : ctx(c), opt(pis), report(r), tm(c) {}

    void begin(const CircuitC *cs, const Assignment *asg) {
        if (report) {
            memset(report, 0, sizeof *report);
            report->first_row = ~0ULL;
        }
        refuse_sharded(ctx, "check", "check");
        dom = prove_domain(ctx, cs, asg, false);
        public_input_map(opt, dom.n, pi_pos, pi_val);
        tables_wait(ctx);  // (the NTT tables are shared with a background build)
        PNP_HIP(hipSetDevice(ctx->device));
        s = ctx->stream;
        tm.start();
        for (auto &c : col) c.alloc(32 * dom.n);
    }

    CheckRows selector_rows(KeyRowValues &kv, DevicePis &pis, const uint64_t *&k_rows);
    void gates(const CheckRows &r, CheckRecord *rec);
    void lookup(const CheckRows &r, const uint64_t *s_rows, uint64_t s_n, const uint64_t *k_rows, CheckRecord *rec);
    void copy(const CheckRows &r, CheckRecord *rec);
    void report_out(const CheckRecord *rec, uint32_t copy_checked);
    void check_columns(const uint64_t *s_rows, uint64_t s_n, bool copy_over_map, uint32_t copy_checked);
};

// k_rows: the key's q_lookup rows (the resident wire map keeps them)
CheckRows Check::selector_rows(KeyRowValues &kv, DevicePis &pis, const uint64_t *&k_rows) {
    CheckRows r{};
    for (int j = 0; j < 4; j++) r.w[j] = col[j].u64();
    r.q_m = kv.values(kQm), r.q_l = kv.values(kQl), r.q_r = kv.values(kQr), r.q_o = kv.values(kQo);
    r.q_4 = kv.values(kQ4), r.q_c = kv.values(kQc), r.q_hl = kv.values(kQhl), r.q_hr = kv.values(kQhr);
    r.q_h4 = kv.values(kQh4), r.q_arith = kv.values(kQarith);
    for (int f = 0; f < 4; f++) r.fam[f] = kv.values(KeyPoly(kRange + f));
    k_rows = ctx->key.wm_qlk.p ? ctx->key.wm_qlk.u64() : kv.values(kQlookup);
    pis.upload(pi_pos, pi_val, s);
    r.pi_pos = pis.pos, r.pi_val = pis.val;
    r.n_pi = pis.n;
    r.lg = dom.lg;
    return r;
}

void Check::gates(const CheckRows &r, CheckRecord *rec) {
    int arith_cols = 4;
    for (const uint64_t *p : {r.q_m, r.q_l, r.q_r, r.q_o, r.q_4, r.q_c, r.q_hl, r.q_hr, r.q_h4, r.q_arith})
        arith_cols += p != nullptr;
    int fam_cols = 0;
    hipEvent_t e0 = nullptr;
    ctx->ktimer.begin("check_rows", s, e0);
    k_check_arith(r, rec, s);
    for (int f = 0; f < 4; f++) {
        if (!r.fam[f]) continue;
        k_check_family(f, r, rec, s);
        fam_cols++;  // its selector column; the wires only where it is non-zero
    }
    ctx->ktimer.end("check_rows", s, e0, 32.0 * (double)dom.n * (arith_cols + fam_cols));
    tm.mark("check_rows");
}

// nothing to do when neither the caller nor the key selects a row
void Check::lookup(const CheckRows &r, const uint64_t *s_rows, uint64_t s_n, const uint64_t *k_rows,
                   CheckRecord *rec) {
    if (s_rows || k_rows) {
        const ProverKeyC &d = ctx->key.dev;
        const uint64_t *t[4] = {d.table1, d.table2, d.table3, d.table4};
        DevBuf slots(8 * dom.n);
        k_check_table_set(t, dom.lg, slots.u32(), s);
        k_check_lookup(r.w, s_rows, s_n, k_rows, t, slots.u32(), dom.lg, rec, s);
        PNP_HIP(hipStreamSynchronize(s));  // (slots is released here)
    }
    tm.mark("check_lookup");
}

void Check::copy(const CheckRows &r, CheckRecord *rec) {
    const ResidentKey &key = ctx->key;
    DevBuf first(4 * key.wm_vars);
    const uint32_t *dvar[4];
    key.wm_columns(dvar);
    k_check_copy(dvar, key.wm_gates, key.wm_vars, r.w, dom.lg, first.u32(), rec, s);
    PNP_HIP(hipStreamSynchronize(s));
}

void Check::report_out(const CheckRecord *rec, uint32_t copy_checked) {
    CheckRecord h;
    PNP_HIP(hipMemcpyAsync(&h, rec, sizeof h, hipMemcpyDeviceToHost, s));
    PNP_HIP(hipStreamSynchronize(s));
    ctx->ktimer.collect();
    const pnp_check_report rep = check_report(h, copy_checked);
    if (report) *report = rep;
    if (rep.violations) throw Error(PNP_E_UNSAT);
}

// The common part: the witness is in col[] (padded), s_rows are the caller's
// q_lookup rows (the first s_n; nullptr: a zero column).
void Check::check_columns(const uint64_t *s_rows, uint64_t s_n, bool copy_over_map, uint32_t copy_checked) {
    tm.mark("check_inputs");
    KeyRowValues kv{ctx, dom.lg};
    DevicePis pis;
    const uint64_t *k_rows = nullptr;
    const CheckRows r = selector_rows(kv, pis, k_rows);
    DevBuf recbuf(sizeof(CheckRecord));
    CheckRecord *rec = static_cast<CheckRecord *>(recbuf.p);
    k_check_reset(rec, s);
    tm.mark("check_rows_ntt");
    gates(r, rec);
    lookup(r, s_rows, s_n, k_rows, rec);
    if (copy_over_map) copy(r, rec);
    tm.mark("check_copy");
    report_out(rec, copy_checked);
}

}  // namespace

void check_assignment(pnp_ctx *ctx, const Assignment &asg, int device_ptrs, const ProveOpts &pis,
                      pnp_check_report *report) {
    Check c(ctx, pis, report);
    c.begin(nullptr, &asg);
    // the columns through the resident wire map (assignment.hip), as the prover gathers them
    DevBuf up;
    const uint64_t *vals = asg.values;
    if (!device_ptrs) {
        up.alloc(32 * asg.n_vars);
        h2d_batch(ctx, {{up.p, asg.values, 32 * asg.n_vars}});
        vals = up.u64();
    }
    const uint32_t *dvar[4];
    ctx->key.wm_columns(dvar);
    uint64_t *w[4] = {c.col[0].u64(), c.col[1].u64(), c.col[2].u64(), c.col[3].u64()};
    k_gather_witness(dvar, c.dom.ng, vals, asg.n_vars, c.dom.lg, w, c.s);
    PNP_HIP(hipStreamSynchronize(c.s));
    up.release();
    // s = k: the key's q_lookup rows, as pnp_prove_assignment; one value a
    // variable: the copy constraints hold by construction
    const uint64_t *k_rows = ctx->key.wm_qlk.p ? ctx->key.wm_qlk.u64() : nullptr;
    c.check_columns(k_rows, c.dom.n, false, 1);
}

void check_witness(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, const ProveOpts &pis,
                   pnp_check_report *report) {
    Check c(ctx, pis, report);
    c.begin(cs, nullptr);
    // the padded columns as Proof::load_witness stages them, and the caller's
    // q_lookup rows, which may be absent here (nullptr: no row selected)
    const uint64_t ng = c.dom.ng;
    uint64_t *w[4] = {c.col[0].u64(), c.col[1].u64(), c.col[2].u64(), c.col[3].u64()};
    DevBuf qlk;
    std::vector<H2D> up;
    stage_wire_columns(ctx, cs, device_ptrs, w, ng, c.dom.n, up);
    const uint64_t *s_rows = nullptr;
    if (cs->q_lookup && ng) {
        qlk.alloc(32 * ng);
        if (device_ptrs) PNP_HIP(hipMemcpyAsync(qlk.p, cs->q_lookup, 32 * ng, hipMemcpyDeviceToDevice, c.s));
        else up.push_back({qlk.p, cs->q_lookup, 32 * ng});
        s_rows = qlk.u64();
    }
    if (!up.empty()) h2d_batch(ctx, up);
    // with a wire map resident the columns are checked against it
    const bool map = ctx->key.wm_loaded;
    c.check_columns(s_rows, ng, map, map ? 1 : 0);
}

}  // namespace pnp
