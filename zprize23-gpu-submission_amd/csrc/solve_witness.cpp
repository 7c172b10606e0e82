// solve_witness.cpp — the witness solver's host side over the kernels of
// solve.hip: the plan build (pnp_load_solve_inputs, pnp_load_solve_plan,
// pnp_load_solve_plan_gates, pnp_load_solve_plan_ecc, pnp_load_solve_plan_lookup), the solve (pnp_solve_assignment) and what reads
// the solved assignment back (pnp_assignment_*, pnp_solved_public_inputs, the
// prologue of pnp_prove_solved / pnp_check_solved).  abi.cpp checks the
// arguments; the plan and the solution live in ResidentKey::SolvePlan
// (prover_key.h), which also turns the levels' widths into launches.
//
// A plan build, in order (PlanBuild holds its scratch):
//   preconditions  key and wire map resident, one GPU, the old plan dropped,
//                  fewer than 2^27 gates
//   mark_inputs    the ids to HBM, level 0 for them; a bad or repeated id refused
//   selector_rows  forward transforms of the resident coefficients; a gate
//                  family's only where its flag is set
//   mark_outputs   the output rows checked on the device, marked for the mask
//   rounds         the levels; pnp_solve_info; an undetermined variable refused
//   emit           the plan's entries into HBM, the ids and output rows kept;
//                  with lookup entries, the index of the key's table
//   the launch runs (SolvePlan::launch_runs) and the counts
// A solve, in order:
//   preconditions  a plan, its input count, one GPU, no public input on an
//                  output row, public_input_map
//   stage_inputs   the solution zeroed, the inputs scattered, the public
//                  inputs uploaded                         -> "solve_inputs"
//   run_levels     one launch a run, with the byte credit  -> "solve_levels"
//   derive_outputs the output rows' public inputs to the host -> "solve_outputs"
#include <algorithm>
#include <string.h>
#include "context.h"

namespace pnp {
namespace {

using SolvePlan = ResidentKey::SolvePlan;

const SolvePlan &solved_plan(pnp_ctx *ctx) {
    const SolvePlan &sp = ctx->key.solve;
    if (!sp.loaded || !sp.solution.p) {
        set_error("no solved assignment resident (a plan and pnp_solve_assignment first)");
        throw Error(PNP_E_NOKEY);
    }
    return sp;
}

// the caller's public inputs, none of them on an output row of the plan
void refuse_pi_on_outputs(const SolvePlan &sp, const char *what, uint64_t n_pi, const uint64_t *pi_pos) {
    for (uint64_t k = 0; k < n_pi; k++)
        if (sp.is_output(pi_pos[k])) {
            set_error("%s: row %llu is an output of the plan (its public input is derived, not given)", what,
                      (unsigned long long)pi_pos[k]);
            throw Error(PNP_E_ARG);
        }
}

// One plan build in flight: its arguments and its scratch, released with it.
struct PlanBuild {
    pnp_ctx *const ctx;
    const char *const what;
    const uint64_t n_inputs, n_outputs;
    const uint32_t gates, ecc, lookup;
    const int device_ptrs;
    pnp_solve_info *const info;
    hipStream_t s = nullptr;
    uint64_t ng = 0, n_vars = 0, n_arith = 0, n_gate = 0, n_ecc = 0, n_lookup = 0;  // gates, variables; entries by kind
    DevBuf ids, level, def, small, ecc_level;
    KeyRowValues kv{ctx, 0};
    DevBuf out_rows, out_bits;
    SolveBuild b;
    SolveSel sel{};
    const uint32_t *dvar[4];

    hipMemcpyKind from_caller() const { return device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice; }
    void preconditions();
    void mark_inputs(const uint32_t *input_ids);
    void selector_rows();
    void mark_outputs(const uint64_t *output_rows);
    pnp_solve_info rounds();
    void emit(pnp_solve_info &out);
};

void PlanBuild::preconditions() {
    if (info) {
        memset(info, 0, sizeof *info);
        info->first_undetermined = ~0ULL;
    }
    ResidentKey &key = ctx->key;
    if (!key.loaded || !key.wm_loaded) {
        set_error(key.loaded ? "no wire map resident (pnp_preprocess or pnp_load_wire_map first)"
                             : "prover key not loaded");
        throw Error(PNP_E_NOKEY);
    }
    refuse_sharded(ctx, what, "solve");
    tables_wait(ctx);  // (the NTT tables are shared with a background build)
    PNP_HIP(hipSetDevice(ctx->device));
    s = ctx->stream;
    key.solve.drop();
    ng = key.wm_gates, n_vars = key.wm_vars;
    kv.lg = log2_exact(key.n);
    key.wm_columns(dvar);
    if (ng >= (1ULL << 27)) {  // a bid is 32 row + role in 32 bits
        set_error("%s: %llu gates (a plan covers fewer than 2^27)", what, (unsigned long long)ng);
        throw Error(PNP_E_ARG);
    }
}

// the input ids, and every variable's level: 0 for an input
void PlanBuild::mark_inputs(const uint32_t *input_ids) {
    ids.alloc(4 * std::max<uint64_t>(n_inputs, 1)), level.alloc(4 * n_vars), def.alloc(4 * n_vars);
    if (n_inputs) PNP_HIP(hipMemcpyAsync(ids.p, input_ids, 4 * n_inputs, from_caller(), s));
    uint32_t err[2];
    solve_mark_inputs(ids.u32(), n_inputs, n_vars, level.u32(), err, small, s);
    if (err[0] != 0xffffffffu) {
        set_error("%s: input id %u is not a variable (n_vars = %llu)", what, err[0], (unsigned long long)n_vars);
        throw Error(PNP_E_ARG);
    }
    if (err[1] != 0xffffffffu) {
        set_error("%s: input id %u is listed twice", what, err[1]);
        throw Error(PNP_E_ARG);
    }
}

void PlanBuild::selector_rows() {
    sel.q_m = kv.values(kQm), sel.q_l = kv.values(kQl), sel.q_r = kv.values(kQr), sel.q_o = kv.values(kQo);
    sel.q_4 = kv.values(kQ4), sel.q_c = kv.values(kQc), sel.q_hl = kv.values(kQhl);
    sel.q_hr = kv.values(kQhr), sel.q_h4 = kv.values(kQh4), sel.q_arith = kv.values(kQarith);
    // (a family's rows: only where its flag is set and the key has the selector)
    if (gates & PNP_SOLVE_RANGE) sel.range = kv.values(kRange);
    if (gates & PNP_SOLVE_LOGIC) sel.logic = kv.values(kLogic);
    if (ecc & PNP_SOLVE_FIXED_ADD) sel.fixed_add = kv.values(kFixedAdd);
    if (ecc & PNP_SOLVE_VAR_ADD) sel.var_add = kv.values(kVarAdd);
    // (the wire map keeps the q_lookup rows, as the check reads them)
    if (lookup & PNP_SOLVE_LOOKUP)
        sel.lookup = ctx->key.wm_qlk.p ? ctx->key.wm_qlk.u64() : kv.values(kQlookup);
}

// the output rows: checked on the device, their rows marked for the mask
void PlanBuild::mark_outputs(const uint64_t *output_rows) {
    if (!n_outputs) return;
    out_rows.alloc(8 * n_outputs);
    out_bits.alloc(4 * ((ng + 31) / 32));
    PNP_HIP(hipMemcpyAsync(out_rows.p, output_rows, 8 * n_outputs, from_caller(), s));
    uint64_t oerr[3];
    solve_mark_outputs(out_rows.u64(), n_outputs, ng, sel.q_arith, out_bits.u32(), oerr, small, s);
    const char *const why[3] = {"is not a gate", "is listed twice", "has q_arith = 0"};
    for (int k = 0; k < 3; k++)
        if (oerr[k] != ~0ULL) {
            set_error("%s: output row %llu %s", what, (unsigned long long)oerr[k], why[k]);
            throw Error(PNP_E_ARG);
        }
}

// the rounds, what they found for the caller, and the undetermined refusal
pnp_solve_info PlanBuild::rounds() {
    solve_rounds(dvar, ng, n_vars, sel, out_bits.u32(), level.u32(), def.u32(), ecc_level, b, s);
    pnp_solve_info out;
    memset(&out, 0, sizeof out);
    uint64_t n_ecc_vars = 0;  // (an ECC entry defines up to three variables)
    out.n_inputs = n_inputs;
    out.n_levels = b.widths.size();
    for (size_t l = 0; l < b.widths.size(); l++) {
        n_arith += b.widths[l];
        n_gate += b.gate_widths[l];
        n_ecc += b.ecc_widths[l];
        n_ecc_vars += b.ecc_vars[l];
        n_lookup += b.lookup_widths[l];
        out.max_width = std::max<uint64_t>(out.max_width, (uint64_t)b.widths[l] + b.gate_widths[l] + b.ecc_vars[l] +
                                                              b.lookup_widths[l]);
    }
    out.n_solved = n_arith + n_gate + n_ecc_vars + n_lookup;
    out.n_undetermined = b.n_undetermined;
    out.first_undetermined = b.n_undetermined ? b.first_undetermined : ~0ULL;
    if (b.n_undetermined) {
        if (info) *info = out;
        const char *const fmt =
            lookup  ? "%s: variable %u is neither an input nor defined by an arithmetic row whose other wires are "
                      "known, nor by a range, logic, fixed-add, var-add or lookup row that is ready (%llu such variables)"
            : ecc   ? "%s: variable %u is neither an input nor defined by an arithmetic row whose other wires are "
                      "known, nor by a range, logic, fixed-add or var-add row that is ready (%llu such variables)"
            : gates ? "%s: variable %u is neither an input nor defined by an arithmetic row whose other "
                      "wires are known, nor by a range or logic row whose next row is (%llu such variables)"
                    : "%s: variable %u is neither an input nor defined by an arithmetic row whose other "
                      "wires are known (%llu such variables)";
        set_error(fmt, what, b.first_undetermined, (unsigned long long)b.n_undetermined);
        throw Error(PNP_E_ARG);
    }
    return out;
}

// the entries into the resident plan, its launches and counts
void PlanBuild::emit(pnp_solve_info &out) {
    SolvePlan &sp = ctx->key.solve;
    sp.buf.alloc(SolveView::bytes(n_arith, out.n_levels, n_inputs, n_outputs, sel.q_m != nullptr));
    sp.view.lay(sp.buf.p, n_arith, out.n_levels, n_inputs, n_outputs, sel.q_m != nullptr);
    if (n_gate) {
        sp.gate_buf.alloc(SolveGateView::bytes(n_gate, out.n_levels));
        sp.gate_view.lay(sp.gate_buf.p, n_gate);
    }
    if (n_ecc) {
        sp.ecc_buf.alloc(SolveEccView::bytes(n_ecc, out.n_levels));
        sp.ecc_view.lay(sp.ecc_buf.p, n_ecc);
    }
    if (n_lookup) {
        sp.lookup_buf.alloc(SolveLookupView::bytes(n_lookup, out.n_levels));
        sp.lookup_view.lay(sp.lookup_buf.p, n_lookup);
        const ProverKeyC &d = ctx->key.dev;
        const uint64_t *t[4] = {d.table1, d.table2, d.table3, d.table4};
        if (!t[0] || !t[1] || !t[2] || !t[3]) {
            sp.drop();
            set_error("%s: the key has q_lookup rows and no table columns resident", what);
            throw Error(PNP_E_ARG);
        }
        sp.n_indexed = solve_lookup_index(t, ctx->key.n, sp.lookup_index, sp.lookup_view, s);
    }
    solve_emit(dvar, ng, n_vars, sel, level.u32(), def.u32(), ecc_level.u32(), b, out_rows.u64(), n_outputs, sp.view,
               sp.gate_view, sp.ecc_view, sp.lookup_view, s);
    if (n_inputs) PNP_HIP(hipMemcpyAsync(sp.view.ids, ids.p, 4 * n_inputs, hipMemcpyDeviceToDevice, s));
    sp.out_rows.resize(n_outputs);
    if (n_outputs) PNP_HIP(hipMemcpyAsync(sp.out_rows.data(), out_rows.p, 8 * n_outputs, hipMemcpyDeviceToHost, s));
    PNP_HIP(hipStreamSynchronize(s));
    sp.runs = SolvePlan::launch_runs(b.widths, b.gate_widths, b.ecc_widths, b.lookup_widths);
    sp.n_range = b.n_range, sp.n_logic = b.n_logic, sp.n_two = b.n_two;
    sp.n_fixed = b.n_fixed, sp.n_var = b.n_var, sp.n_ecc = n_ecc;
    sp.n_gate = n_gate;
    sp.n_lookup = n_lookup;
    sp.n_inputs = n_inputs;
    sp.n_solved = out.n_solved;
    sp.n_levels = out.n_levels;
    sp.loaded = true;
    out.plan_bytes = sp.buf.bytes + sp.gate_buf.bytes + sp.ecc_buf.bytes + sp.lookup_buf.bytes + sp.lookup_index.bytes;
}

// One solve in flight over the resident plan.
struct Solve {
    pnp_ctx *const ctx;
    SolvePlan &sp;
    hipStream_t s;
    StageTimer tm;
    uint64_t *vals = nullptr;
    DevBuf up;  // host inputs staged
    DevicePis pis;

    void stage_inputs(const uint64_t *inputs, uint64_t n_inputs, int device_ptrs, const std::vector<uint64_t> &pos,
                      const std::vector<Fr> &val);
    void run_levels();
    void derive_outputs();
};

void Solve::stage_inputs(const uint64_t *inputs, uint64_t n_inputs, int device_ptrs, const std::vector<uint64_t> &pos,
                         const std::vector<Fr> &val) {
    const uint64_t n_vars = ctx->key.wm_vars;
    if (!sp.solution.p) sp.solution.alloc(32 * n_vars);
    vals = sp.solution.u64();
    // (a slot that is not relevant may name a variable a later level writes: it reads zero)
    PNP_HIP(hipMemsetAsync(vals, 0, 32 * n_vars, s));
    const uint64_t *in = inputs;
    if (n_inputs && !device_ptrs) {
        up.alloc(32 * n_inputs);
        h2d_batch(ctx, {{up.p, inputs, 32 * n_inputs}});
        in = up.u64();
    }
    k_solve_scatter(sp.view.ids, in, n_inputs, vals, s);
    pis.upload(pos, val, s);
    tm.mark("solve_inputs");
}

void Solve::run_levels() {
    hipEvent_t e0 = nullptr;
    ctx->ktimer.begin("solve_levels", s, e0);
    const bool naf = sp.n_fixed != 0;  // (fixed-add scalar entries among the gate entries)
    for (const auto &r : sp.runs) {
        if (r.k1 != r.k0) {  // lookup entries: a launch a segment, or the workgroup with waves for them
            if (r.wide) {
                if (r.p1 > r.p0) k_solve_levels(sp.view, r.l0, r.l1, r.p0, r.p1, true, vals, pis.pos, pis.val, pis.n, s);
                k_solve_gate_level(sp.gate_view, r.g0, r.g1, vals, s, naf);
                k_solve_ecc_level(sp.ecc_view, r.e0, r.e1, vals, s);
                k_solve_lookup_level(sp.lookup_view, r.k0, r.k1, vals, s);
            } else {
                k_solve_lookup_levels(sp.view, sp.gate_view, sp.n_gate != 0, sp.ecc_view, sp.n_ecc != 0,
                                      sp.lookup_view, r.l0, r.l1, vals, pis.pos, pis.val, pis.n, s);
            }
        } else if (r.e1 != r.e0) {  // ECC entries: a launch a segment, or the three-part workgroup
            if (r.wide) {
                if (r.p1 > r.p0) k_solve_levels(sp.view, r.l0, r.l1, r.p0, r.p1, true, vals, pis.pos, pis.val, pis.n, s);
                k_solve_gate_level(sp.gate_view, r.g0, r.g1, vals, s, naf);
                k_solve_ecc_level(sp.ecc_view, r.e0, r.e1, vals, s);
            } else {
                k_solve_ecc_levels(sp.view, sp.gate_view, sp.n_gate != 0, sp.ecc_view, r.l0, r.l1, vals, pis.pos,
                                   pis.val, pis.n, s);
            }
        } else if (r.g1 == r.g0) {  // no gate entries: the arithmetic kernels alone
            k_solve_levels(sp.view, r.l0, r.l1, r.p0, r.p1, r.wide, vals, pis.pos, pis.val, pis.n, s);
        } else if (r.wide) {  // one level, a launch a segment
            if (r.p1 > r.p0) k_solve_levels(sp.view, r.l0, r.l1, r.p0, r.p1, true, vals, pis.pos, pis.val, pis.n, s);
            k_solve_gate_level(sp.gate_view, r.g0, r.g1, vals, s, naf);
        } else {
            k_solve_mixed_levels(sp.view, sp.gate_view, r.l0, r.l1, vals, pis.pos, pis.val, pis.n, s, naf);
        }
    }
    // an entry reads its coefficients and ids, four values, and writes one;
    // a gate entry reads its 16 bytes and one or two values, and writes one
    const double per_entry = 32.0 * (kSolveCoefs - (sp.view.coef[kSolveQm] ? 1 : 2)) + 4 * 6 + 32 * 5;
    // an ECC entry reads its 128 bytes and up to four values; every variable it defines is a value written
    const uint64_t n_ecc_vars = sp.n_fixed + sp.n_var - (sp.n_gate - sp.n_range - sp.n_logic);
    // a lookup entry reads its 16 bytes, three values, two offsets, and a row id and four columns of one
    // table row (a bucket of one), and writes a value
    ctx->ktimer.end("solve_levels", s, e0,
                    per_entry * (double)(sp.n_solved - sp.n_gate - n_ecc_vars - sp.n_lookup) + 80.0 * (double)sp.n_gate +
                        32.0 * (double)sp.n_two + 256.0 * (double)sp.n_ecc + 32.0 * (double)n_ecc_vars +
                        (16 + 96 + 8 + 4 + 128 + 32) * (double)sp.n_lookup);
    tm.mark("solve_levels");
    ctx->ktimer.collect();
}

// one launch after the last level, and the outputs' canonical values to the host
void Solve::derive_outputs() {
    const uint64_t n_out = sp.out_rows.size();
    sp.out_canon.assign(4 * n_out, 0);
    if (!n_out) return;
    k_solve_outputs(sp.view, n_out, vals, s);
    PNP_HIP(hipMemcpyAsync(sp.out_canon.data(), sp.view.out.pi, 32 * n_out, hipMemcpyDeviceToHost, s));
    tm.mark("solve_outputs");
}

}  // namespace

void load_solve_plan(pnp_ctx *ctx, const char *what, const uint32_t *input_ids, uint64_t n_inputs,
                     const uint64_t *output_rows, uint64_t n_outputs, uint32_t gates, uint32_t ecc, uint32_t lookup,
                     int device_ptrs, pnp_solve_info *info) {
    PlanBuild pb{ctx, what, n_inputs, n_outputs, gates, ecc, lookup, device_ptrs, info};
    pb.preconditions();
    pb.mark_inputs(input_ids);
    pb.selector_rows();
    pb.mark_outputs(output_rows);
    pnp_solve_info out = pb.rounds();
    pb.emit(out);
    if (info) *info = out;
}

void solve_gate_entries(pnp_ctx *ctx, uint64_t out[2]) {
    const SolvePlan &sp = ctx->key.solve;
    if (!sp.loaded) {
        set_error("no solve plan resident (pnp_load_solve_plan_gates first)");
        throw Error(PNP_E_NOKEY);
    }
    out[0] = sp.n_range;
    out[1] = sp.n_logic;
}

void solve_ecc_entries(pnp_ctx *ctx, uint64_t out[2]) {
    const SolvePlan &sp = ctx->key.solve;
    if (!sp.loaded) {
        set_error("no solve plan resident (pnp_load_solve_plan_ecc first)");
        throw Error(PNP_E_NOKEY);
    }
    out[0] = sp.n_fixed;
    out[1] = sp.n_var;
}

void solve_lookup_entries(pnp_ctx *ctx, uint64_t out[2]) {
    const SolvePlan &sp = ctx->key.solve;
    if (!sp.loaded) {
        set_error("no solve plan resident (pnp_load_solve_plan_lookup first)");
        throw Error(PNP_E_NOKEY);
    }
    out[0] = sp.n_lookup;
    out[1] = sp.n_indexed;
}

void solve_assignment(pnp_ctx *ctx, const uint64_t *inputs, uint64_t n_inputs, int device_ptrs,
                      const ProveOpts &opt) {
    SolvePlan &sp = ctx->key.solve;
    if (!sp.loaded) {
        set_error("no solve plan resident (pnp_load_solve_inputs or pnp_load_solve_plan first)");
        throw Error(PNP_E_NOKEY);
    }
    if (n_inputs != sp.n_inputs) {
        set_error("solve assignment: %llu inputs, the plan was built for %llu", (unsigned long long)n_inputs,
                  (unsigned long long)sp.n_inputs);
        throw Error(PNP_E_ARG);
    }
    refuse_sharded(ctx, "solve assignment", "solve");
    refuse_pi_on_outputs(sp, "solve assignment", opt.n_pi, opt.pi_pos);
    std::vector<uint64_t> pos;
    std::vector<Fr> val;
    public_input_map(opt, ctx->key.n, pos, val);
    tables_wait(ctx);
    PNP_HIP(hipSetDevice(ctx->device));
    Solve sv{ctx, sp, ctx->stream, StageTimer(ctx)};
    sv.tm.start();
    sv.stage_inputs(inputs, n_inputs, device_ptrs, pos, val);
    sv.run_levels();
    sv.derive_outputs();
    ctx->stages.emplace_back("inputs_h2d_bytes", device_ptrs ? 0.0 : 32.0 * (double)n_inputs);
}

void assignment_ptr(pnp_ctx *ctx, uint64_t **d_values, uint64_t *n_vars) {
    const SolvePlan &sp = solved_plan(ctx);
    *d_values = sp.solution.u64();
    if (n_vars) *n_vars = ctx->key.wm_vars;
}

void assignment_values(pnp_ctx *ctx, const uint32_t *ids, uint64_t k, uint64_t *out) {
    const SolvePlan &sp = solved_plan(ctx);
    const uint64_t n_vars = ctx->key.wm_vars;
    if (k > n_vars && !ids) {
        set_error("assignment values: %llu values of %llu variables", (unsigned long long)k,
                  (unsigned long long)n_vars);
        throw Error(PNP_E_ARG);
    }
    for (uint64_t j = 0; ids && j < k; j++)
        if (ids[j] >= n_vars) {
            set_error("assignment values: id %u is not a variable (n_vars = %llu)", ids[j],
                      (unsigned long long)n_vars);
            throw Error(PNP_E_ARG);
        }
    PNP_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (!ids) {
        if (k) PNP_HIP(hipMemcpyAsync(out, sp.solution.p, 32 * k, hipMemcpyDeviceToHost, s));
    } else {
        for (uint64_t j = 0; j < k; j++)  // (a handful of values: the root)
            PNP_HIP(hipMemcpyAsync(out + 4 * j, sp.solution.u64() + 4 * (uint64_t)ids[j], 32, hipMemcpyDeviceToHost,
                                   s));
    }
    PNP_HIP(hipStreamSynchronize(s));
}

void solved_public_inputs(pnp_ctx *ctx, uint64_t *pos, uint64_t *canon, uint64_t cap, uint64_t *n) {
    const SolvePlan &sp = solved_plan(ctx);
    *n = sp.out_rows.size();
    const uint64_t k = std::min<uint64_t>(cap, *n);
    std::copy_n(sp.out_rows.begin(), k, pos);
    std::copy_n(sp.out_canon.begin(), 4 * k, canon);
}

int solved_assignment(pnp_ctx *ctx, const char *what, uint64_t n_pi, const uint64_t *pi_pos,
                      const uint64_t *pi_canon, SolvedAssignment &out) {
    PNP_TRY({
        const SolvePlan &sp = solved_plan(ctx);
        refuse_pi_on_outputs(sp, what, n_pi, pi_pos);
        out.pos.assign(pi_pos, pi_pos + n_pi);
        out.canon.assign(pi_canon, pi_canon + 4 * n_pi);
        out.pos.insert(out.pos.end(), sp.out_rows.begin(), sp.out_rows.end());
        out.canon.insert(out.canon.end(), sp.out_canon.begin(), sp.out_canon.end());
        out.values = sp.solution.u64();
        out.n_vars = ctx->key.wm_vars;
    });
}

}  // namespace pnp
