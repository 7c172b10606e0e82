// prover_key.h — the one description of the prover key's polynomials, and the
// key as it is resident in HBM (prover_key.cpp: the loads; prover.cpp: the
// quotient's arguments; v1.cpp: the v1 hashing).
#pragma once
#include "pnp_internal.h"
#include <stddef.h>

namespace pnp {

// One row per polynomial of the key, in the order the loads build the block
// arrays (the optional selectors first: they decide the key's class).
enum KeyPoly : int {
    kQm, kQlookup, kRange, kLogic, kFixedAdd, kVarAdd,             // optional: may be the zero polynomial
    kQl, kQr, kQo, kQ4, kQc, kQhl, kQhr, kQh4, kQarith,            // always present
    kSig0, kSig1, kSig2, kSig3,
    kTable1, kTable2, kTable3, kTable4,                            // n-row columns (MultiSet::pad), no blocks
    kLin, kVhInv, kL1v,                                            // coset arrays that exist only as blocks
    kKeyRows
};
enum KeyClass : int { kSel, kOptSel, kSigma, kTable, kCoset };
constexpr int kPkFields = 44;  // ProverKeyC, lib.rs:157-223

struct KeyRow {
    KeyPoly id;
    const char *name;   // of its block array (messages)
    int coeffs, evals;  // ProverKeyC field of the n coefficients (a table: its n rows) / the 8n evaluations; -1: none
    KeyClass cls;
    // a key of k_quotient29's class (protocol.h) keeps the blocks in the 2^261
    // form, and (lin: the PI term) a 2^256 copy beside them
    bool in29, keeps256;
    int desc;  // index in pnp_circuit_desc.sel[], -1: none
    int vk;    // index in pnp_verifier_key.polys[], -1: none
    bool optional() const { return cls == kOptSel; }
};

// The q_m, custom-gate and q_lookup selectors (kOptSel) are read only when
// their 8n evaluations are non-zero: for the zero polynomial the Rust prover
// key holds EMPTY coefficient Vecs (prover.rs:765-808 passes their dangling
// pointers), so those coefficients are never touched.
constexpr KeyRow kKeyTable[kKeyRows] = {
    {kQm, "q_m", 0, 1, kOptSel, true, false, 0, 0},
    {kQlookup, "q_lookup", 28, 29, kOptSel, false, false, 14, 18},
    {kRange, "range", 20, 21, kOptSel, false, false, 10, 10},
    {kLogic, "logic", 22, 23, kOptSel, false, false, 11, 11},
    {kFixedAdd, "fixed_add", 24, 25, kOptSel, false, false, 12, 12},
    {kVarAdd, "var_add", 26, 27, kOptSel, false, false, 13, 13},
    {kQl, "q_l", 2, 3, kSel, true, false, 1, 1},
    {kQr, "q_r", 4, 5, kSel, true, false, 2, 2},
    {kQo, "q_o", 6, 7, kSel, true, false, 3, 3},
    {kQ4, "q_4", 8, 9, kSel, true, false, 4, 4},
    {kQc, "q_c", 10, 11, kSel, true, false, 5, 5},
    {kQhl, "q_hl", 12, 13, kSel, true, false, 6, 6},
    {kQhr, "q_hr", 14, 15, kSel, true, false, 7, 7},
    {kQh4, "q_h4", 16, 17, kSel, true, false, 8, 8},
    {kQarith, "q_arith", 18, 19, kSel, true, false, 9, 9},
    {kSig0, "sig0", 34, 35, kSigma, true, false, -1, 14},
    {kSig1, "sig1", 36, 37, kSigma, true, false, -1, 15},
    {kSig2, "sig2", 38, 39, kSigma, true, false, -1, 16},
    {kSig3, "sig3", 40, 41, kSigma, true, false, -1, 17},
    {kTable1, "table1", 30, -1, kTable, false, false, -1, 19},
    {kTable2, "table2", 31, -1, kTable, false, false, -1, 20},
    {kTable3, "table3", 32, -1, kTable, false, false, -1, 21},
    {kTable4, "table4", 33, -1, kTable, false, false, -1, 22},
    {kLin, "lin", -1, 42, kCoset, true, true, -1, -1},    // linear_evaluations
    {kVhInv, "vh_inv", -1, 43, kCoset, false, false, -1, -1},  // from v_h_coset_8n, inverted at key load
    {kL1v, "l1v", -1, -1, kCoset, false, false, -1, -1},  // n^-1 / (x - 1) = L1 / Z_H, the standard coset only
};

// a wrong row fails the build, not a proof
#define PNP_KEY_ROW(r, co, ev)                                                                        \
    static_assert(kKeyTable[r].id == r, "kKeyTable is indexed by KeyPoly");                           \
    static_assert(offsetof(ProverKeyC, co) == 8 * kKeyTable[r].coeffs, "ProverKeyC." #co);           \
    static_assert(offsetof(ProverKeyC, ev) == 8 * kKeyTable[r].evals, "ProverKeyC." #ev)
#define PNP_KEY_ROW1(r, member, f)                                                                    \
    static_assert(kKeyTable[r].id == r, "kKeyTable is indexed by KeyPoly");                           \
    static_assert(offsetof(ProverKeyC, f) == 8 * kKeyTable[r].member, "ProverKeyC." #f)
PNP_KEY_ROW(kQm, q_m_coeffs, q_m_evals);
PNP_KEY_ROW(kQlookup, q_lookup_coeffs, q_lookup_evals);
PNP_KEY_ROW(kRange, range_selector_coeffs, range_selector_evals);
PNP_KEY_ROW(kLogic, logic_selector_coeffs, logic_selector_evals);
PNP_KEY_ROW(kFixedAdd, fixed_group_add_selector_coeffs, fixed_group_add_selector_evals);
PNP_KEY_ROW(kVarAdd, variable_group_add_selector_coeffs, variable_group_add_selector_evals);
PNP_KEY_ROW(kQl, q_l_coeffs, q_l_evals);
PNP_KEY_ROW(kQr, q_r_coeffs, q_r_evals);
PNP_KEY_ROW(kQo, q_o_coeffs, q_o_evals);
PNP_KEY_ROW(kQ4, q_4_coeffs, q_4_evals);
PNP_KEY_ROW(kQc, q_c_coeffs, q_c_evals);
PNP_KEY_ROW(kQhl, q_hl_coeffs, q_hl_evals);
PNP_KEY_ROW(kQhr, q_hr_coeffs, q_hr_evals);
PNP_KEY_ROW(kQh4, q_h4_coeffs, q_h4_evals);
PNP_KEY_ROW(kQarith, q_arith_coeffs, q_arith_evals);
PNP_KEY_ROW(kSig0, left_sigma_coeffs, left_sigma_evals);
PNP_KEY_ROW(kSig1, right_sigma_coeffs, right_sigma_evals);
PNP_KEY_ROW(kSig2, out_sigma_coeffs, out_sigma_evals);
PNP_KEY_ROW(kSig3, fourth_sigma_coeffs, fourth_sigma_evals);
PNP_KEY_ROW1(kTable1, coeffs, table1);
PNP_KEY_ROW1(kTable2, coeffs, table2);
PNP_KEY_ROW1(kTable3, coeffs, table3);
PNP_KEY_ROW1(kTable4, coeffs, table4);
PNP_KEY_ROW1(kLin, evals, linear_evaluations);
PNP_KEY_ROW1(kVhInv, evals, v_h_coset_8n);
static_assert(kKeyTable[kL1v].id == kL1v && kKeyTable[kL1v].coeffs < 0 && kKeyTable[kL1v].evals < 0, "l1v");
#undef PNP_KEY_ROW
#undef PNP_KEY_ROW1

// the row whose column `col` (coeffs, evals, desc, vk) holds v; nullptr: none
constexpr const KeyRow *key_row_where(int KeyRow::*col, int v) {
    for (const KeyRow &r : kKeyTable)
        if (r.*col == v) return &r;
    return nullptr;
}
// what ProverKeyC field f holds: a row's n coefficients (or table rows), or
// its 8n evaluations
struct KeyField {
    const KeyRow *row;
    bool evals;
    uint64_t elems(uint64_t D) const { return evals ? 8 * D : D; }
};
constexpr KeyField key_field(int f) {
    const KeyRow *c = key_row_where(&KeyRow::coeffs, f);
    return c ? KeyField{c, false} : KeyField{key_row_where(&KeyRow::evals, f), true};
}
constexpr bool key_fields_covered() {
    for (int f = 0; f < kPkFields; f++)
        if (!key_field(f).row) return false;
    return true;
}
static_assert(key_fields_covered(), "every ProverKeyC field belongs to a row");

// D = 2^lg (the callers have checked that D is a power of two)
inline uint32_t log2_exact(uint64_t D) {
    uint32_t lg = 0;
    while ((1ULL << lg) < D) lg++;
    return lg;
}

// ---- the resident prover key (ProverKeyC mirrored in HBM) ----
struct ResidentKey {
    bool loaded = false;
    uint64_t n = 0;             // domain size D
    DevBuf owned[kPkFields];    // copies (device_ptrs == 0), by ProverKeyC field
    ProverKeyC dev{};           // HBM pointers for every field
    uint64_t gen = 0;           // incremented by every key load (wires.hip re-checks sigma)
    // which optional selectors are not the zero polynomial (bit = KeyPoly):
    // the quotient and the linearisation skip the others
    uint32_t present = 0;
    bool has(KeyPoly r) const { return !kKeyTable[r].optional() || (present >> r & 1); }
    bool qm_zero() const { return !has(kQm); }
    bool qlookup_zero() const { return !has(kQlookup); }
    bool custom(int k) const { return has(KeyPoly(kRange + k)); }  // range, logic, fixed-base, curve-add
    bool any_custom() const { return custom(0) || custom(1) || custom(2) || custom(3); }
    // from the loaded fields: an optional selector is present when the load kept a pointer to it
    void set_present(const ProverKeyC &d) {
        const uint64_t *const *f = reinterpret_cast<const uint64_t *const *>(&d);
        present = 0;
        for (const KeyRow &r : kKeyTable)
            if (r.optional() && (f[r.coeffs] || f[r.evals])) present |= 1u << r.id;
    }
    DevBuf sigma_n[4];  // sigma evaluations on the n-domain
    DevBuf tmp[4];      // key-load scratch (8n Fr each), kept for the next host-pointer full load
    // The quotient's 8n-point arrays in block layout (ntt.hip: point 8j + m
    // -> block m, index j), blocks mb0 .. mb0 + nb - 1 only, by row: the
    // selectors, sigmas, lin (coset points) and the proof-independent coset
    // constants computed at key load: vh_inv = v_h^-1 and, when std_coset
    // (linear_evaluations = 7 w_8n^i, v_h = x^n - 1), l1v.  An absent block
    // is an empty DevBuf (u64() == nullptr: the quotient's "zero selector").
    // blk29: the same arrays in the 2^261 form for k_quotient29, made at key
    // load for keys of its class (q29): the rows with in29
    DevBuf blk[kKeyRows], blk29[kKeyRows];
    int mb0 = 0, nb = 8, blk_rank = 0, blk_world = 1;
    bool std_coset = false, q29 = false;
    // the array of row r this key's quotient kernel reads (nullptr: absent)
    const uint64_t *key_block(KeyPoly r) const { return (q29 && kKeyTable[r].in29 ? blk29[r] : blk[r]).u64(); }
    DevBuf pinv;  // 1 / (x - w^pos) (block layout), pos = pinv_pos
    uint64_t pinv_pos = ~0ULL;

    // ---- the resident wire map (pnp_preprocess, pnp_load_wire_map) ----
    // the composer's variable ids of this key's circuit: column j (wire j of
    // every gate) at u32 offset j * wm_gates; pnp_prove_assignment gathers the
    // witness through it (assignment.hip).  Replaced by the next preprocess,
    // dropped by any other key load
    bool wm_loaded = false;
    uint64_t wm_gates = 0, wm_vars = 0;
    DevBuf wm_var;
    // the row values of q_lookup on the domain (n Fr), from the resident
    // coefficients when the map became resident; empty: the zero polynomial
    DevBuf wm_qlk;
    void wm_columns(const uint32_t *d[4]) const {
        for (int j = 0; j < 4; j++) d[j] = wm_var.u32() + j * wm_gates;
    }
    void wire_map_drop() {
        wm_loaded = false;
        wm_gates = wm_vars = 0;
        wm_var.release();
        wm_qlk.release();
        solve.drop();  // a plan is a schedule of this map's rows
    }

    // ---- the witness solver's plan and solution (pnp_load_solve_plan,
    // pnp_solve_assignment; solve.hip) ----
    // Built over the resident wire map for one choice of input variables and
    // output rows; replaced by the next pnp_load_solve_plan, dropped with the map
    struct SolvePlan {
        bool loaded = false;
        uint64_t n_inputs = 0, n_solved = 0, n_levels = 0;
        DevBuf buf;      // the entries, the level offsets, the input ids, the output entries (SolveView)
        SolveView view{};
        // the entries range and logic rows define (pnp_load_solve_plan_gates), in
        // arrays of their own; empty when the plan has none
        DevBuf gate_buf;
        SolveGateView gate_view{};
        uint64_t n_range = 0, n_logic = 0, n_two = 0;  // by family; n_two: those reading two values
        // the entries fixed-add and var-add rows define (pnp_load_solve_plan_ecc)
        // but for the fixed-add scalar's, which are gate entries; empty when
        // the plan has none.  n_fixed, n_var: the variables each family defines
        DevBuf ecc_buf;
        SolveEccView ecc_view{};
        uint64_t n_fixed = 0, n_var = 0, n_ecc = 0, n_gate = 0;  // n_ecc, n_gate: ECC entries, gate entries
        // the entries lookup rows define (pnp_load_solve_plan_lookup) and the
        // index of the key's table they search (n_indexed of its rows); both
        // empty when the plan has no such entry.  The index reads the resident
        // table columns: every key load drops the wire map and with it the plan
        DevBuf lookup_buf, lookup_index;
        SolveLookupView lookup_view{};
        uint64_t n_lookup = 0, n_indexed = 0;
        // the output rows in listed order, and the public inputs the last solve
        // derived for them (canonical, 4 words each; empty before a solve)
        std::vector<uint64_t> out_rows, out_canon;
        bool is_output(uint64_t row) const {
            return std::find(out_rows.begin(), out_rows.end(), row) != out_rows.end();
        }
        // the launches of a solve: one wide level (more than a workgroup,
        // arithmetic entries p0 .. p1, gate entries g0 .. g1, ECC entries
        // e0 .. e1 and lookup entries k0 .. k1 together), or a run of
        // consecutive levels that each fit one
        struct Run {
            uint32_t l0, l1;
            uint64_t p0, p1, g0, g1;
            bool wide;
            uint64_t e0 = 0, e1 = 0, k0 = 0, k1 = 0;
        };
        std::vector<Run> runs;
        // from the levels' widths (arithmetic, gate, ECC and lookup entries; ecc_widths
        // or lookup_widths empty: none): a level wider than a workgroup, all segments counted,
        // alone; narrower ones in runs
        PNP_HIDDEN static std::vector<Run> launch_runs(const std::vector<uint32_t> &widths,
                                                       const std::vector<uint32_t> &gate_widths,
                                                       const std::vector<uint32_t> &ecc_widths = {},
                                                       const std::vector<uint32_t> &lookup_widths = {}) {
            std::vector<Run> runs;
            uint64_t p = 0, g = 0, e = 0, k = 0;
            for (uint32_t l = 0; l < widths.size(); l++) {
                const uint64_t wa = widths[l], wg = gate_widths[l], we = l < ecc_widths.size() ? ecc_widths[l] : 0;
                const uint64_t wk = l < lookup_widths.size() ? lookup_widths[l] : 0;
                const bool wide = wa + wg + we + wk > 256;
                if (!wide && !runs.empty() && !runs.back().wide) {
                    runs.back().l1 = l + 1;
                    runs.back().p1 = p + wa;
                    runs.back().g1 = g + wg;
                    runs.back().e1 = e + we;
                    runs.back().k1 = k + wk;
                } else {
                    runs.push_back({l, l + 1, p, p + wa, g, g + wg, wide, e, e + we, k, k + wk});
                }
                p += wa;
                g += wg;
                e += we;
                k += wk;
            }
            return runs;
        }
        DevBuf solution;  // n_vars Fr of the last solve; empty before it
        void drop() {
            loaded = false;
            n_inputs = n_solved = n_levels = 0;
            n_range = n_logic = n_two = 0;
            n_fixed = n_var = n_ecc = n_gate = 0;
            n_lookup = n_indexed = 0;
            lookup_buf.release();
            lookup_index.release();
            buf.release();
            gate_buf.release();
            ecc_buf.release();
            runs.clear();
            out_rows.clear();
            out_canon.clear();
            solution.release();
        }
    } solve;
};

}  // namespace pnp
