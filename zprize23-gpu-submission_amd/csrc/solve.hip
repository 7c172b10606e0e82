// solve.hip — the witness from the circuit's inputs, on gfx950.
//
// A composer fills the assignment gate by gate on the CPU: almost every
// variable is the one unknown of one arithmetic row whose other wires are
// already known (the reference's witness generation, the "gadget" of its
// README, 9-10 s at HEIGHT 15).  Here the library derives the schedule of
// those rows once per circuit and per choice of input variables (the plan,
// rules in include/pnp_plonk.h), and a solve walks it.
//
// The plan build, all on the device:
//   k_solve_mask_    a lane a row: one byte, which slots are relevant (low
//                    nibble) and which of those are solvable (high nibble)
//   k_solve_ready_   round t, a lane a row not yet finished: the relevant slots
//                    whose variable is unknown; none left: the row is finished
//                    (its byte is cleared); exactly one, solvable: the row
//                    bids for it, atomicMin of 32 row + slot on winner[u]
//   k_solve_commit_  the same rows again: the bidder that holds winner[u]
//                    defines u (level[u] = t, def[u] = 32 row + slot).  "Known"
//                    is level[u] < t here, so the levels written by other
//                    lanes of this launch change nothing any lane decides
//   the variables are then sorted by level (preprocess.hip's stable radix
//   sort: ties in variable order, so the plan is the same on every run) and
//   k_solve_denoms_ / k_solve_fold_ write the entries around one batch
//   inverse: -1 / coef folded into every coefficient, so a solve divides
//   nothing.
// A round sweeps the mask bytes of all rows and goes on only where a byte is
// non-zero: at HEIGHT 15, 3.2 MB a launch for rows that finished long ago.
//
// The solve: k_solve_wide_ one lane an entry of one level; k_solve_narrow_ one
// workgroup over a run of consecutive levels of at most 256 entries each, a
// __syncthreads() between levels (the values a level wrote are read by the
// same workgroup: workgroup scope).  A slot that is not relevant may name a
// variable that is not written yet: its coefficients are zero and the value
// (zero: the buffer is cleared first) only ever meets a multiplication by them.
//
// Output rows (pnp_load_solve_plan): rows whose public input is derived, not
// given.  k_solve_mark_outputs_ checks the list (atomicMin of the offending
// row, a bitmap for the duplicates) and k_solve_mask_ gives their rows a zero
// byte, so they never bid; k_solve_out_emit_ stores each row's selectors times
// -q_arith after the level entries, and k_solve_outputs_, launched after the
// last level, a lane a row, writes PI = -q_arith S in canonical form.
//
// Range and logic rows (pnp_load_solve_plan_gates): a second byte a row
// (k_solve_mask_) says which gate rules the row still has; a ready gate row
// bids for up to five variables, one of them in the next row, so a bid and a
// definition are 32 row + role (atomicMin: the least (row, role) wins) and the
// commit counts what each family defined.  Their entries (16 bytes: target, two
// sources, kind and shift; k_solve_gate_emit_) live in arrays of their own, and
// run in lanes of their own: k_solve_gate_wide_ a lane an entry of one level,
// k_solve_mixed_ one workgroup of 512 over a run of narrow levels, arithmetic
// entries in waves 0-3 and gate entries in waves 4-7, so that no wave runs both
// bodies.  Plans without gate entries launch what they always launched.
//
// Fixed-base and curve-addition rows (pnp_load_solve_plan_ecc): four more bits
// of the second byte (the fixed-add scalar, xy and point rules, the var-add
// rule) and seven more roles, so a bid is 32 row + role.  The rounds' kernels
// are instantiated on "the plan has ECC rules": without them the bodies are the
// ones above.  The scalar definition is one more kind of gate entry (integer
// work on one canonical value); the others are ECC entries (SolveEccView): the
// commit notes the round of every (row, kind) that defined something, those
// are sorted by round, and k_solve_ecc_emit_ writes an entry for each with
// the targets it won and the row's q_l, q_r, q_c.  A solve runs them in lanes of
// their own: k_solve_ecc_wide_ a lane an entry of one level, k_solve_ecc_mixed_
// one workgroup of 768 over a run of narrow levels, ECC entries in waves 8-11.
// An entry inverts once, (1 + m)(1 - m), by kEccInverseBinary's choice of
// inverse() (Fermat) or fr_inverse_bin (binary Euclid); inv(0) = 0 in both.
//
// Lookup rows (pnp_load_solve_plan_lookup): the last bit of the second byte and
// one more role, lookup c, bid for when the row's a, b and d are known; the
// rounds' kernels are instantiated on "the plan has the lookup rule" as well.
// A lookup entry is one uint4 (target, sources a, b, d) in an array of its own.
// The table index is built once with the plan (solve_lookup_index): the rows
// that are row 0 or differ from it, sorted by a hash of their columns 0, 1, 3
// (lookup_hash, the same function at build and at solve) with the stable radix
// sort, so a bucket holds its rows in table order and the first exact match of
// a scan is the reference's `position`; off[] by a lower bound a bucket.  No
// atomics anywhere in it.  k_solve_lookup_wide_ a lane an entry of one level;
// k_solve_lookup_mixed_ the one workgroup of the narrow levels (512 lanes, 768
// with gate entries) with four waves for the lookup entries; a plan that has
// ECC entries too runs k_solve_lookup_ecc_mixed_, k_solve_ecc_mixed_'s 768
// lanes with the lookup entries in the gate waves' spare lanes.
// No LDS, no scalar-memory tricks; plain C++ and vector memory operations.
#include "pnp_internal.h"
#include "widgets.cuh"

namespace pnp {

namespace {

inline uint32_t nblk(uint64_t threads, uint32_t bs = 256) { return (uint32_t)((threads + bs - 1) / bs); }

constexpr uint32_t kUnset = 0xFFFFFFFFu;

struct MapArgs {
    const uint32_t *var[4];
};

__device__ __forceinline__ Fr pow5(const Fr &x) {
    const Fr x2 = x * x;
    return x2 * x2 * x;
}

__device__ __forceinline__ bool nz(const uint64_t *col, uint64_t i) { return col && !load_fr(col, i).is_zero(); }

// slots a (q_l, q_hl, q_m), b (q_r, q_hr, q_m), c (q_o), d (q_4, q_h4): bit j =
// slot j is relevant, bit 4 + j = it is solvable (only its linear selector)
__device__ __forceinline__ uint32_t row_mask(const SolveSel &q, uint64_t i) {
    if (!nz(q.q_arith, i)) return 0;
    const bool m = nz(q.q_m, i);
    const bool lin[4] = {nz(q.q_l, i), nz(q.q_r, i), nz(q.q_o, i), nz(q.q_4, i)};
    const bool oth[4] = {nz(q.q_hl, i) || m, nz(q.q_hr, i) || m, false, nz(q.q_h4, i)};
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (lin[j] || oth[j]) r |= 1u << j;
        if (lin[j] && !oth[j]) r |= 16u << j;
    }
    return r;
}

// the gate rules of row i: kGateRange, kGateLogic (with kGateXor: q_c = -1, else
// q_c = 1; a logic row with another q_c has no rule), none on the last row
// kFixScalar, kFixXy, kFixPoint: the three rules of a fixed-add row; kVarAdd
// kLookup: the lookup rule (it reads no next row: the last row has it too)
enum : uint32_t { kGateRange = 1, kGateLogic = 2, kGateXor = 4, kFixScalar = 8, kFixXy = 16, kFixPoint = 32,
                  kVarAdd = 64, kLookup = 128, kEccRules = kFixScalar | kFixXy | kFixPoint | kVarAdd };
__device__ __forceinline__ uint32_t row_gates(const SolveSel &q, uint64_t i, uint64_t n_gates) {
    uint32_t r = nz(q.lookup, i) ? kLookup : 0;
    if (i + 1 >= n_gates) return r;
    if (nz(q.range, i)) r |= kGateRange;
    if (nz(q.fixed_add, i)) r |= kFixScalar | kFixXy | kFixPoint;
    if (nz(q.var_add, i)) r |= kVarAdd;
    if (nz(q.logic, i)) {
        const Fr c = load_fr(q.q_c, i);
        if (c == Fr::one()) r |= kGateLogic;
        else if (c == neg(Fr::one())) r |= kGateLogic | kGateXor;
    }
    return r;
}

// (an output row's bytes are zero from the start: no sweep ever looks at it)
__global__ __launch_bounds__(256) void k_solve_mask_(SolveSel q, uint64_t n_gates, const uint32_t *out_bits,
                                                     uint8_t *mask, uint8_t *gmask) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n_gates) return;
    const bool out = out_bits && ((out_bits[i >> 5] >> (i & 31)) & 1);
    mask[i] = out ? (uint8_t)0 : (uint8_t)row_mask(q, i);
    if (gmask) gmask[i] = out ? (uint8_t)0 : (uint8_t)row_gates(q, i, n_gates);
}

// a lane a listed output row: its bit, and the lowest row of each kind of mistake
__global__ __launch_bounds__(256) void k_solve_mark_outputs_(const uint64_t *rows, uint64_t n_out, uint64_t n_gates,
                                                             const uint64_t *q_arith, uint32_t *bits,
                                                             unsigned long long *err) {
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (k >= n_out) return;
    const uint64_t i = rows[k];
    if (i >= n_gates) {
        atomicMin(&err[0], (unsigned long long)i);
        return;
    }
    const uint32_t bit = 1u << (i & 31);
    if (atomicOr(&bits[i >> 5], bit) & bit) atomicMin(&err[1], (unsigned long long)i);
    if (!nz(q_arith, i)) atomicMin(&err[2], (unsigned long long)i);
}

__global__ __launch_bounds__(256) void k_solve_inputs_(const uint32_t *ids, uint64_t n_inputs, uint64_t n_vars,
                                                       uint32_t *level, uint32_t *err) {
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (k >= n_inputs) return;
    const uint32_t id = ids[k];
    if (id >= n_vars) atomicMin(&err[0], id);
    else if (atomicExch(&level[id], 0u) == 0u) atomicMin(&err[1], id);
}

// the relevant slots of row i whose variable has level >= bound; u, slot: the last of them
__device__ __forceinline__ int unknowns(const MapArgs &a, uint64_t i, uint32_t m, const uint32_t *level,
                                        uint32_t bound, uint64_t n_vars, uint32_t &u, int &slot) {
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!((m >> j) & 1)) continue;
        const uint32_t v = a.var[j][i];
        if (v < n_vars && __atomic_load_n(&level[v], __ATOMIC_RELAXED) >= bound) {
            cnt++;
            u = v;
            slot = j;
        }
    }
    return cnt;
}

// The bids of row i in a round, arithmetic and gate rules alike: put(u, role)
// for every variable u the row would define, "known" being level < bound.
// Returns the row's bytes as they are after the round: an arithmetic byte with
// nothing left to define is cleared, and so is the bit of a gate rule none of
// whose slots is unknown, or that is ready (whatever it bid for is defined in
// this round, by this row or by a lower one).
template <bool ECC, bool LK, class Put>
__device__ __forceinline__ void row_bids(const MapArgs &a, uint64_t i, uint32_t &m, uint32_t &gm, const uint32_t *level,
                                         uint32_t bound, uint64_t n_vars, Put &&put) {
    auto unknown = [&](uint32_t v) { return v < n_vars && __atomic_load_n(&level[v], __ATOMIC_RELAXED) >= bound; };
    auto known = [&](uint32_t v) { return v < n_vars && __atomic_load_n(&level[v], __ATOMIC_RELAXED) < bound; };
    if (m) {
        uint32_t u = 0;
        int slot = 0;
        const int cnt = unknowns(a, i, m, level, bound, n_vars, u, slot);
        if (cnt == 0) m = 0;  // nothing left to define: a plain constraint from here on
        else if (cnt == 1 && ((m >> (4 + slot)) & 1)) put(u, (uint32_t)slot);
    }
    if (gm & kGateRange) {
        const bool ready = known(a.var[3][i + 1]);
        bool left = false;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t v = a.var[j][i];
            if (!unknown(v)) continue;
            left = true;
            if (ready) put(v, (uint32_t)(kSolveRoleRange + j));
        }
        if (ready || !left) gm &= ~kGateRange;
    }
    if (gm & kGateLogic) {
        const bool ready = known(a.var[0][i + 1]) && known(a.var[1][i + 1]);
        bool left = false;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const uint32_t v = j < 4 ? a.var[j][i] : a.var[3][i + 1];
            if (!unknown(v)) continue;
            left = true;
            if (ready) put(v, (uint32_t)(kSolveRoleLogic + j));
        }
        if (ready || !left) gm &= ~(kGateLogic | kGateXor);
    }
    if constexpr (ECC) {
        if (gm & (kFixScalar | kFixXy | kFixPoint)) {
            const bool d0 = known(a.var[3][i]), d1 = known(a.var[3][i + 1]);
            if (gm & kFixScalar) {
                const uint32_t v = a.var[3][i];
                const bool left = unknown(v);
                if (d1 && left) put(v, (uint32_t)kSolveRoleFixed);
                if (d1 || !left) gm &= ~kFixScalar;
            }
            if (gm & kFixXy) {
                const uint32_t v = a.var[2][i];
                const bool ready = d0 && d1, left = unknown(v);
                if (ready && left) put(v, (uint32_t)(kSolveRoleFixed + 1));
                if (ready || !left) gm &= ~kFixXy;
            }
            if (gm & kFixPoint) {
                const bool ready = d0 && d1 && known(a.var[0][i]) && known(a.var[1][i]);
                bool left = false;
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const uint32_t v = a.var[j][i + 1];
                    if (!unknown(v)) continue;
                    left = true;
                    if (ready) put(v, (uint32_t)(kSolveRoleFixed + 2 + j));
                }
                if (ready || !left) gm &= ~kFixPoint;
            }
        }
        if (gm & kVarAdd) {
            const bool ready = known(a.var[0][i]) && known(a.var[1][i]) && known(a.var[2][i]) && known(a.var[3][i]);
            bool left = false;
#pragma unroll
            for (int j = 0; j < 3; j++) {  // a_next, b_next, d_next
                const uint32_t v = a.var[j < 2 ? j : 3][i + 1];
                if (!unknown(v)) continue;
                left = true;
                if (ready) put(v, (uint32_t)(kSolveRoleVar + j));
            }
            if (ready || !left) gm &= ~kVarAdd;
        }
    }
    if constexpr (LK) {
        if (gm & kLookup) {
            const uint32_t v = a.var[2][i];
            const bool ready = known(a.var[0][i]) && known(a.var[1][i]) && known(a.var[3][i]), left = unknown(v);
            if (ready && left) put(v, (uint32_t)kSolveRoleLookup);
            if (ready || !left) gm &= ~kLookup;
        }
    }
}

template <bool ECC, bool LK>
__global__ __launch_bounds__(256) void k_solve_ready_(MapArgs a, uint64_t n_gates, uint64_t n_vars, uint8_t *mask,
                                                      const uint8_t *gmask, const uint32_t *level, uint32_t *winner) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n_gates) return;
    uint32_t m = mask[i], gm = gmask ? gmask[i] : 0;
    if (!m && !gm) return;
    const uint32_t m0 = m;
    row_bids<ECC, LK>(a, i, m, gm, level, kUnset, n_vars, [&](uint32_t u, uint32_t role) {
        const uint32_t key = ((uint32_t)i << kSolveRoleBits) + role;
        if (__atomic_load_n(&winner[u], __ATOMIC_RELAXED) > key) atomicMin(&winner[u], key);
    });
    // (a ready gate rule keeps its bit until the commit, which looks at the same rows)
    if (m0 && !m) mask[i] = 0;
}

// count[0..3]: the round's definitions by arithmetic, range and logic rules,
// and those of them that read two values (logic c, d, d_next); with ECC rules
// count[4..7]: by the fixed-add scalar rule, by the other fixed-add rules, by
// var-add rules, and the (row, kind) pairs those two defined anything for (the
// ECC entries), whose round goes to ecc_level[3 row + kind]; with the lookup
// rule count[8]: by lookup rows
template <bool ECC, bool LK>
__global__ __launch_bounds__(256) void k_solve_commit_(MapArgs a, uint64_t n_gates, uint64_t n_vars, uint8_t *mask,
                                                       uint8_t *gmask, uint32_t *level, const uint32_t *winner,
                                                       uint32_t *def, uint32_t t, uint32_t *count,
                                                       uint32_t *ecc_level) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    constexpr int kCounts = LK ? 9 : ECC ? 8 : 4;
    uint32_t won[kCounts] = {};
    if (i < n_gates) {
        uint32_t m = mask[i], gm = gmask ? gmask[i] : 0;
        if (m || gm) {
            const uint32_t gm0 = gm;
            uint32_t kinds = 0;
            row_bids<ECC, LK>(a, i, m, gm, level, t, n_vars, [&](uint32_t u, uint32_t role) {
                const uint32_t key = ((uint32_t)i << kSolveRoleBits) + role;
                if (winner[u] != key) return;
                __atomic_store_n(&level[u], t, __ATOMIC_RELAXED);
                def[u] = key;
                if (LK && role == kSolveRoleLookup) {
                    won[kCounts - 1]++;
                } else if (!ECC || role < kSolveRoleFixed) {
                    won[role < kSolveRoleRange ? 0 : role < kSolveRoleLogic ? 1 : 2]++;
                    if (role >= kSolveRoleLogic + 2) won[3]++;
                } else if constexpr (ECC) {
                    won[role == kSolveRoleFixed ? 4 : role < kSolveRoleVar ? 5 : 6]++;
                    if (role > kSolveRoleFixed)
                        kinds |= 1u << (role == kSolveRoleFixed + 1 ? kSolveEccXy
                                        : role < kSolveRoleVar      ? kSolveEccPoint
                                                                    : kSolveEccVar);
                }
                if (role < kSolveRoleRange) mask[i] = 0;
            });
            if (gm != gm0) gmask[i] = (uint8_t)gm;
            if constexpr (ECC) {
#pragma unroll
                for (int k = 0; k < kSolveEccKinds; k++)
                    if ((kinds >> k) & 1) ecc_level[kSolveEccKinds * i + k] = t, won[7]++;
            }
        }
    }
    // (a lane wins at most ten times: four bits of every counter)
#pragma unroll
    for (int c = 0; c < kCounts; c++) {
        if (!gmask && c) break;
        if (LK && !ECC && c >= 4 && c < 8) continue;  // (no ECC rules: nothing counted there)
        uint32_t sum = 0;
#pragma unroll
        for (int bit = 0; bit < 4; bit++) sum += (uint32_t)__popcll(__ballot((won[c] >> bit) & 1)) << bit;
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&count[c], sum);
    }
}

// the variables no round reached: their count and the lowest of them
__global__ __launch_bounds__(256) void k_solve_unset_(const uint32_t *level, uint64_t n_vars, uint32_t *out) {
    const uint64_t u = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const bool un = u < n_vars && level[u] == kUnset;
    const unsigned long long b = __ballot(un);
    if (!b) return;
    if (un) atomicMin(&out[1], (uint32_t)u);
    if ((threadIdx.x & 63) == 0) atomicAdd(&out[0], (uint32_t)__popcll(b));
}

// sort key: the 0-based level of a variable an arithmetic row defines, n_levels
// + that level for one a gate entry defines (only where gate_keys: a plan with
// gate entries), the key above all of those for every other
__global__ __launch_bounds__(256) void k_solve_keys_(const uint32_t *level, const uint32_t *def, uint64_t n_vars,
                                                     uint32_t n_levels, bool gate_keys, uint32_t *key) {
    const uint64_t u = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (u >= n_vars) return;
    const uint32_t l = level[u], rest = gate_keys ? 2 * n_levels : n_levels;
    if (l < 1 || l > n_levels) key[u] = rest;
    else {
        const uint32_t role = def[u] & ((1u << kSolveRoleBits) - 1);
        if (role > kSolveRoleFixed) key[u] = rest;  // (an ECC entry's: not in either array)
        else key[u] = gate_keys && role >= kSolveRoleRange ? n_levels + l - 1 : l - 1;
    }
}

// sort key of a (row, kind): the 0-based round in which it defined something, n_levels for none
__global__ __launch_bounds__(256) void k_solve_ecc_keys_(const uint32_t *ecc_level, uint64_t n, uint32_t n_levels,
                                                         uint32_t *key) {
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t l = ecc_level[k];
    key[k] = l >= 1 && l <= n_levels ? l - 1 : n_levels;
}

// entry p: its target, row and wires, and the two denominators coef and coef q_arith
__global__ __launch_bounds__(256) void k_solve_denoms_(MapArgs a, SolveSel q, const uint32_t *order,
                                                       const uint32_t *def, uint64_t n, uint64_t n_vars, SolveView v,
                                                       uint64_t *den) {
    const uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t u = order[p] < n_vars ? order[p] : 0, d = def[u];
    const uint64_t i = d >> kSolveRoleBits;
    const int slot = (int)(d & 3);  // (an arithmetic role is its slot)
    v.tgt[p] = u;
    v.row[p] = (uint32_t)i;
#pragma unroll
    for (int j = 0; j < 4; j++) v.var[j][p] = a.var[j][i];
    const uint64_t *lin = slot == 0 ? q.q_l : slot == 1 ? q.q_r : slot == 2 ? q.q_o : q.q_4;
    const Fr coef = load_fr(lin, i);
    store_fr(den, p, coef);
    store_fr(den, n + p, coef * load_fr(q.q_arith, i));
}

// den holds the inverses now: the row's selectors times -1 / coef, zero for
// the target's slot and for slots that are not relevant
__global__ __launch_bounds__(256) void k_solve_fold_(SolveSel q, uint64_t n, SolveView v, const uint32_t *def,
                                                     const uint64_t *den) {
    const uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t i = v.row[p];
    const int slot = (int)(def[v.tgt[p]] & 3);
    const uint32_t m = row_mask(q, i);
    const Fr k = neg(load_fr(den, p));
    bool use[4];
#pragma unroll
    for (int j = 0; j < 4; j++) use[j] = ((m >> j) & 1) && j != slot;
    auto put = [&](int c, const uint64_t *col, bool on) {
        store_fr(v.coef[c], p, on && col ? load_fr(col, i) * k : Fr::zero());
    };
    put(kSolveQl, q.q_l, use[0]);
    put(kSolveQr, q.q_r, use[1]);
    put(kSolveQo, q.q_o, use[2]);
    put(kSolveQ4, q.q_4, use[3]);
    put(kSolveQhl, q.q_hl, use[0]);
    put(kSolveQhr, q.q_hr, use[1]);
    put(kSolveQh4, q.q_h4, use[3]);
    put(kSolveQc, q.q_c, true);
    // (a solvable target slot has q_m = 0 on its row: a b never holds the target)
    if (v.coef[kSolveQm]) put(kSolveQm, q.q_m, use[0] && use[1]);
    store_fr(v.coef[kSolvePik], p, neg(load_fr(den, n + p)));
}

// output entry k: its row and wires, and the row's selectors times -q_arith
__global__ __launch_bounds__(256) void k_solve_out_emit_(MapArgs a, SolveSel q, const uint64_t *rows, uint64_t n_out,
                                                         SolveOutView o) {
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (k >= n_out) return;
    const uint64_t i = rows[k];
    o.row[k] = (uint32_t)i;
#pragma unroll
    for (int j = 0; j < 4; j++) o.var[j][k] = a.var[j][i];
    const Fr f = neg(load_fr(q.q_arith, i));
    auto put = [&](int c, const uint64_t *col) { store_fr(o.coef[c], k, col ? load_fr(col, i) * f : Fr::zero()); };
    put(kSolveQl, q.q_l);
    put(kSolveQr, q.q_r);
    put(kSolveQo, q.q_o);
    put(kSolveQ4, q.q_4);
    put(kSolveQhl, q.q_hl);
    put(kSolveQhr, q.q_hr);
    put(kSolveQh4, q.q_h4);
    put(kSolveQc, q.q_c);
    if (o.coef[kSolveQm]) put(kSolveQm, q.q_m);
}

// gate entry g: the variable at order[g] and what its (row, role) says it is
__global__ __launch_bounds__(256) void k_solve_gate_emit_(MapArgs a, SolveSel q, const uint32_t *order,
                                                          const uint32_t *def, uint64_t n, uint64_t n_gates,
                                                          uint64_t n_vars, SolveGateView g) {
    const uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t u = order[p] < n_vars ? order[p] : 0, d = def[u], role = d & ((1u << kSolveRoleBits) - 1);
    const uint64_t i = d >> kSolveRoleBits, nx = i + 1 < n_gates ? i + 1 : i;  // (a gate rule's row has a next row)
    uint32_t sa, sb, kind = kSolveGateShift, shift = 2;
    if (role == kSolveRoleFixed) {  // fixed-add d: (d_next - s) / 2
        sa = sb = a.var[3][nx];
        kind = kSolveGateNaf, shift = 1;
    } else if (role < kSolveRoleLogic) {  // range a..d: d_next >> 2, 4, 6, 8
        sa = sb = a.var[3][nx];
        shift = 2 * (role - kSolveRoleRange + 1);
    } else {
        const uint32_t op = load_fr(q.q_c, i) == Fr::one() ? kSolveGateAnd : kSolveGateXor;
        sa = a.var[0][nx], sb = a.var[1][nx];
        switch (role - kSolveRoleLogic) {
        case 0: sb = sa; break;             // a_i = A >> 2
        case 1: sa = sb; break;             // b_i = B >> 2
        case 2: kind = kSolveGateProd, shift = 0; break;
        case 3: kind = op; break;           // d_i = (A >> 2) op (B >> 2)
        default: kind = op, shift = 0;      // d_(i+1) = A op B
        }
    }
    g.tgt[p] = u, g.a[p] = sa, g.b[p] = sb, g.word[p] = kind | shift << 8;
}

// ECC entry p: the (row, kind) at order[p], the targets it won and the row's q_l, q_r, q_c
__global__ __launch_bounds__(256) void k_solve_ecc_emit_(MapArgs a, SolveSel q, const uint32_t *order,
                                                         const uint32_t *level, const uint32_t *def,
                                                         const uint32_t *ecc_level, uint64_t n, uint64_t n_gates,
                                                         uint64_t n_vars, SolveEccView e) {
    const uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t rk = order[p] < kSolveEccKinds * n_gates ? order[p] : 0;
    const uint64_t i = rk / kSolveEccKinds, nx = i + 1 < n_gates ? i + 1 : i;
    const uint32_t kind = (uint32_t)(rk % kSolveEccKinds), t = ecc_level[rk];
    // the variable, where this row's `role` defined it in round t
    auto won = [&](uint32_t v, uint32_t role) {
        return v < n_vars && level[v] == t && def[v] == ((uint32_t)i << kSolveRoleBits) + role ? v : kUnset;
    };
    uint4 tg = make_uint4(kUnset, kUnset, kUnset, kind), sr;
    if (kind == kSolveEccXy) {
        tg.x = won(a.var[2][i], kSolveRoleFixed + 1);
        sr = make_uint4(a.var[3][i], a.var[3][nx], a.var[3][i], a.var[3][i]);
    } else if (kind == kSolveEccPoint) {
        tg.x = won(a.var[0][nx], kSolveRoleFixed + 2), tg.y = won(a.var[1][nx], kSolveRoleFixed + 3);
        sr = make_uint4(a.var[0][i], a.var[1][i], a.var[3][i], a.var[3][nx]);
    } else {
        tg.x = won(a.var[0][nx], kSolveRoleVar), tg.y = won(a.var[1][nx], kSolveRoleVar + 1);
        tg.z = won(a.var[3][nx], kSolveRoleVar + 2);
        sr = make_uint4(a.var[0][i], a.var[1][i], a.var[2][i], a.var[3][i]);
    }
    e.tgt[p] = tg, e.src[p] = sr;
    const bool fixed = kind != kSolveEccVar;
    store_fr(e.q[0], p, fixed ? load_fr(q.q_l, i) : Fr::zero());
    store_fr(e.q[1], p, fixed ? load_fr(q.q_r, i) : Fr::zero());
    store_fr(e.q[2], p, fixed ? load_fr(q.q_c, i) : Fr::zero());
}

// sort key of a variable for the lookup entries: the 0-based level of one a lookup row defines, n_levels for others
__global__ __launch_bounds__(256) void k_solve_lookup_keys_(const uint32_t *level, const uint32_t *def, uint64_t n_vars,
                                                            uint32_t n_levels, uint32_t *key) {
    const uint64_t u = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (u >= n_vars) return;
    const uint32_t l = level[u];
    const bool mine = l >= 1 && l <= n_levels && (def[u] & ((1u << kSolveRoleBits) - 1)) == kSolveRoleLookup;
    key[u] = mine ? l - 1 : n_levels;
}

// lookup entry p: the variable at order[p], and slots a, b, d of the row that defines it
__global__ __launch_bounds__(256) void k_solve_lookup_emit_(MapArgs a, const uint32_t *order, const uint32_t *def,
                                                            uint64_t n, uint64_t n_vars, uint4 *ent) {
    const uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t u = order[p] < n_vars ? order[p] : 0;
    const uint64_t i = def[u] >> kSolveRoleBits;
    ent[p] = make_uint4(u, a.var[0][i], a.var[1][i], a.var[3][i]);
}

// ---- the table index of the lookup entries
struct LookupCols {
    const uint64_t *t[4];
};

// the bucket of a key before masking: a mix of its 24 Montgomery words (only
// the spread over the buckets depends on it); the index build and every query
// go through this one function
__device__ __forceinline__ uint32_t lookup_hash(const Fr &a, const Fr &b, const Fr &d) {
    uint32_t h = 0x9E3779B9u;
    auto mix = [&](const Fr &x) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            h ^= x.v[k];
            h *= 0x85EBCA6Bu;
            h = (h << 13) | (h >> 19);
        }
    };
    mix(a), mix(b), mix(d);
    h ^= h >> 16;
    h *= 0xC2B2AE35u;
    h ^= h >> 15;
    return h;
}

// row r is indexed: row 0, and every row whose four columns are not row 0's
__device__ __forceinline__ bool lookup_indexed(const LookupCols &t, uint64_t r) {
    if (r == 0) return true;
    bool same = true;
#pragma unroll
    for (int j = 0; j < 4; j++) same &= load_fr(t.t[j], r) == load_fr(t.t[j], 0);
    return !same;
}

// a wave 64 rows: part[wave] = how many of them are indexed (no atomics)
__global__ __launch_bounds__(256) void k_solve_lookup_count_(LookupCols t, uint64_t D, uint32_t *part) {
    const uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const unsigned long long b = __ballot(r < D && lookup_indexed(t, r));
    if ((threadIdx.x & 63) == 0) part[r >> 6] = (uint32_t)__popcll(b);
}

// one workgroup: out[0] = the sum of part[0 .. n - 1]; a lane a stride, four
// wave sums through part_out[1..4], added by lane 0
__global__ __launch_bounds__(256) void k_solve_lookup_sum_(const uint32_t *part, uint64_t n, uint32_t *out) {
    uint32_t sum = 0;
    for (uint64_t k = threadIdx.x; k < n; k += 256) sum += part[k];
    uint32_t wave = 0;  // (below 2^26 in all: the bits of the lanes' sums, a ballot a bit)
    for (int bit = 0; bit < 27; bit++) wave += (uint32_t)__popcll(__ballot((sum >> bit) & 1)) << bit;
    if ((threadIdx.x & 63) == 0) out[1 + (threadIdx.x >> 6)] = wave;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = out[1] + out[2] + out[3] + out[4];
}

// sort key of table row r: its bucket, B (above every bucket) for a row that is not indexed
__global__ __launch_bounds__(256) void k_solve_lookup_buckets_(LookupCols t, uint64_t D, uint32_t B, uint32_t *key) {
    const uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (r >= D) return;
    key[r] = lookup_indexed(t, r)
                 ? lookup_hash(load_fr(t.t[0], r), load_fr(t.t[1], r), load_fr(t.t[3], r)) & (B - 1)
                 : B;
}

// lane x: off[x] = how many sorted rows lie in buckets below x (x <= B; off[B] =
// m), and rows[x] = the x-th sorted row (x < m)
__global__ __launch_bounds__(256) void k_solve_lookup_csr_(const uint32_t *key, const uint32_t *order, uint64_t D,
                                                           uint32_t B, uint64_t m, uint32_t *off, uint32_t *rows) {
    const uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (x <= B) {
        uint64_t lo = 0, hi = D;  // the first sorted position whose key is >= x
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (key[order[mid]] < x) lo = mid + 1;
            else hi = mid;
        }
        off[x] = (uint32_t)lo;
    }
    if (x < m) rows[x] = order[x];
}

__global__ __launch_bounds__(256) void k_solve_scatter_(const uint32_t *ids, const uint64_t *in, uint64_t n_inputs,
                                                        uint64_t *vals) {
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (k < n_inputs) store_fr(vals, ids[k], load_fr(in, k));
}

struct PiList {
    const uint64_t *pos, *val;  // ascending rows, Montgomery values
    uint32_t n;
};

// (vals is read and written by the lanes of one launch: no __restrict__)
__device__ __forceinline__ void solve_entry(const SolveView &v, uint64_t p, uint64_t *vals, const PiList &pi) {
    const Fr a = load_fr(vals, v.var[0][p]), b = load_fr(vals, v.var[1][p]);
    const Fr c = load_fr(vals, v.var[2][p]), d = load_fr(vals, v.var[3][p]);
    Fr g = fr_mul2(load_fr(v.coef[kSolveQl], p), a, load_fr(v.coef[kSolveQr], p), b);
    g += fr_mul2(load_fr(v.coef[kSolveQo], p), c, load_fr(v.coef[kSolveQ4], p), d);
    g += fr_mul2(load_fr(v.coef[kSolveQhl], p), pow5(a), load_fr(v.coef[kSolveQhr], p), pow5(b));
    g += load_fr(v.coef[kSolveQh4], p) * pow5(d) + load_fr(v.coef[kSolveQc], p);
    if (v.coef[kSolveQm]) g += load_fr(v.coef[kSolveQm], p) * a * b;
    if (pi.n) {
        const uint64_t row = v.row[p];
        uint32_t lo = 0, hi = pi.n;  // the first listed row >= row
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pi.pos[mid] < row) lo = mid + 1;
            else hi = mid;
        }
        if (lo < pi.n && pi.pos[lo] == row) g += load_fr(v.coef[kSolvePik], p) * load_fr(pi.val, lo);
    }
    store_fr(vals, v.tgt[p], g);
}

__global__ __launch_bounds__(256) void k_solve_wide_(SolveView v, uint64_t p0, uint64_t p1, uint64_t *vals, PiList pi) {
    const uint64_t p = p0 + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p < p1) solve_entry(v, p, vals, pi);
}

// one workgroup: levels l0 .. l1 - 1, each of at most blockDim.x entries
__global__ __launch_bounds__(256) void k_solve_narrow_(SolveView v, uint32_t l0, uint32_t l1, uint64_t *vals, PiList pi) {
    for (uint32_t l = l0; l < l1; l++) {
        const uint64_t p = (uint64_t)v.lvl_off[l] + threadIdx.x;
        if (p < v.lvl_off[l + 1]) solve_entry(v, p, vals, pi);
        __syncthreads();  // the level's values: written, and visible to this workgroup
    }
}

// x >> sh over the eight 32-bit limbs, sh < 32
__device__ __forceinline__ Fr shr_bits(const Fr &x, uint32_t sh) {
    Fr r;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t two = (uint64_t)(k < 7 ? x.v[k + 1] : 0u) << 32 | x.v[k];
        r.v[k] = (uint32_t)(two >> sh);
    }
    return r;
}

// one or two values to canonical form, the quads, and back (SolveGateView);
// NAF: the plan has fixed-add scalar entries (without them: the body as it was)
template <bool NAF>
__device__ __forceinline__ void solve_gate_entry(const SolveGateView &g, uint64_t p, uint64_t *vals) {
    const uint32_t w = g.word[p], kind = w & 255, sh = w >> 8;
    const Fr a = from_mont(load_fr(vals, g.a[p]));
    Fr r;
    if (kind == kSolveGateShift) {
        r = shr_bits(a, sh);
    } else if (NAF && kind == kSolveGateNaf) {
        // A even: A / 2; A = 1 mod 4: (A - 1) / 2; A = 3 mod 4: (A + 1) / 2 <= r / 2
        r = shr_bits(a, 1);
        uint32_t c = (a.v[0] & 3) == 3;
#pragma unroll
        for (int k = 0; k < 8; k++) r.v[k] = __builtin_addc(r.v[k], 0u, c, &c);
    } else {
        const Fr b = from_mont(load_fr(vals, g.b[p]));
        if (kind == kSolveGateProd) {
            r = Fr::zero();
            r.v[0] = (a.v[0] & 3) * (b.v[0] & 3);
        } else {
            const Fr x = shr_bits(a, sh), y = shr_bits(b, sh);
#pragma unroll
            for (int k = 0; k < 8; k++) r.v[k] = kind == kSolveGateAnd ? x.v[k] & y.v[k] : x.v[k] ^ y.v[k];
            // an XOR of two integers below r is below 2^255 < 2 r
            Fr t;
            if (!sub_n<8>(t.v, r.v, FrP::P)) r = t;
        }
    }
    store_fr(vals, g.tgt[p], to_mont(r));
}

template <bool NAF>
__global__ __launch_bounds__(256) void k_solve_gate_wide_(SolveGateView g, uint64_t p0, uint64_t p1, uint64_t *vals) {
    const uint64_t p = p0 + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p < p1) solve_gate_entry<NAF>(g, p, vals);
}

// one workgroup of 512: levels l0 .. l1 - 1, each of at most 256 entries in all;
// lanes 0..255 (waves 0-3) take the arithmetic entries, lanes 256..511 the gate entries
template <bool NAF>
__global__ __launch_bounds__(512) void k_solve_mixed_(SolveView v, SolveGateView g, uint32_t l0, uint32_t l1,
                                                      uint64_t *vals, PiList pi) {
    const bool gate = threadIdx.x >= 256;
    const uint32_t lane = threadIdx.x & 255;
    for (uint32_t l = l0; l < l1; l++) {
        if (gate) {
            const uint64_t p = (uint64_t)g.lvl_off[l] + lane;
            if (p < g.lvl_off[l + 1]) solve_gate_entry<NAF>(g, p, vals);
        } else {
            const uint64_t p = (uint64_t)v.lvl_off[l] + lane;
            if (p < v.lvl_off[l + 1]) solve_entry(v, p, vals, pi);
        }
        __syncthreads();  // the level's values: written, and visible to this workgroup
    }
}

// Fermat's uniform ~380 products, or the binary Euclid's data-dependent ~500
// short steps: profiles/solve_ecc_time.json has both inside the level chain
// (-DPNP_ECC_INVERSE_BINARY=0 builds the other, for tools/solve_time.py --ecc)
#ifndef PNP_ECC_INVERSE_BINARY
#define PNP_ECC_INVERSE_BINARY 1
#endif
constexpr bool kEccInverseBinary = PNP_ECC_INVERSE_BINARY;
__device__ __forceinline__ Fr ecc_inverse(const Fr &x) {
    if constexpr (kEccInverseBinary) return fr_inverse_bin(x);
    else return inverse(x);
}

// one ECC entry (SolveEccView): an xy product, or one or two quotients over one inversion
__device__ __forceinline__ void solve_ecc_entry(const SolveEccView &e, uint64_t p, uint64_t *vals) {
    const uint4 tg = e.tgt[p], sr = e.src[p];
    const uint32_t kind = tg.w;
    if (kind == kSolveEccXy) {
        const Fr bit = load_fr(vals, sr.y) - dbl(load_fr(vals, sr.x));
        if (tg.x != kUnset) store_fr(vals, tg.x, bit * load_fr(e.q[2], p));
        return;
    }
    const Fr one = Fr::one();
    const Fr a = load_fr(vals, sr.x), b = load_fr(vals, sr.y);
    Fr n1, n2, m, dn;
    if (kind == kSolveEccPoint) {
        const Fr bit = load_fr(vals, sr.w) - dbl(load_fr(vals, sr.z));
        const Fr x = load_fr(e.q[0], p) * bit, y = bit * bit * (load_fr(e.q[1], p) - one) + one;
        m = bit * load_fr(e.q[2], p) * a * b * jj_coeff_d();
        n1 = x * b + y * a;
        n2 = y * b - jj_coeff_a() * x * a;
    } else {
        const Fr c = load_fr(vals, sr.z), d = load_fr(vals, sr.w), bc = b * c;
        dn = a * d;
        m = jj_coeff_d() * dn * bc;
        n1 = dn + bc;
        n2 = b * d - jj_coeff_a() * a * c;
    }
    // a zero denominator: its quotient is zero, and it stays out of the shared inversion
    const Fr p1 = one + m, p2 = one - m;
    const bool z1 = p1.is_zero(), z2 = p2.is_zero();
    const Fr f1 = z1 ? one : p1, f2 = z2 ? one : p2;
    const Fr inv = ecc_inverse(f1 * f2);
    if (tg.x != kUnset) store_fr(vals, tg.x, z1 ? Fr::zero() : n1 * f2 * inv);
    if (tg.y != kUnset) store_fr(vals, tg.y, z2 ? Fr::zero() : n2 * f1 * inv);
    if (kind == kSolveEccVar && tg.z != kUnset) store_fr(vals, tg.z, dn);
}

__global__ __launch_bounds__(256) void k_solve_ecc_wide_(SolveEccView e, uint64_t p0, uint64_t p1, uint64_t *vals) {
    const uint64_t p = p0 + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p < p1) solve_ecc_entry(e, p, vals);
}

// one workgroup of 768: levels l0 .. l1 - 1, each of at most 256 entries in all;
// lanes 0..255 the arithmetic entries, 256..511 the gate entries (gates: the
// plan has any), 512..767 (waves 8-11) the ECC entries
__global__ __launch_bounds__(768) void k_solve_ecc_mixed_(SolveView v, SolveGateView g, bool gates, SolveEccView e,
                                                          uint32_t l0, uint32_t l1, uint64_t *vals, PiList pi) {
    const uint32_t part = threadIdx.x >> 8, lane = threadIdx.x & 255;
    for (uint32_t l = l0; l < l1; l++) {
        if (part == 2) {
            const uint64_t p = (uint64_t)e.lvl_off[l] + lane;
            if (p < e.lvl_off[l + 1]) solve_ecc_entry(e, p, vals);
        } else if (part == 1) {
            if (gates) {
                const uint64_t p = (uint64_t)g.lvl_off[l] + lane;
                if (p < g.lvl_off[l + 1]) solve_gate_entry<true>(g, p, vals);
            }
        } else {
            const uint64_t p = (uint64_t)v.lvl_off[l] + lane;
            if (p < v.lvl_off[l + 1]) solve_entry(v, p, vals, pi);
        }
        __syncthreads();  // the level's values: written, and visible to this workgroup
    }
}

// one lookup entry (SolveLookupView): the bucket of the three values, then its
// rows in table order until one holds them in columns 0, 1, 3.  Values and
// table are fully reduced Montgomery residues: the compare is on the words
__device__ __forceinline__ void solve_lookup_entry(const SolveLookupView &k, uint64_t p, uint64_t *vals) {
    const uint4 e = k.ent[p];
    const Fr a = load_fr(vals, e.y), b = load_fr(vals, e.z), d = load_fr(vals, e.w);
    const uint32_t h = lookup_hash(a, b, d) & k.bmask;
    const uint32_t q1 = k.off[h + 1];
    Fr c = Fr::zero();  // no such key: zero, and the check names the row
    for (uint32_t q = k.off[h]; q < q1; q++) {
        const uint32_t r = k.rows[q];
        if (load_fr(k.t[0], r) == a && load_fr(k.t[1], r) == b && load_fr(k.t[3], r) == d) {
            c = load_fr(k.t[2], r);
            break;
        }
    }
    store_fr(vals, e.x, c);
}

__global__ __launch_bounds__(256) void k_solve_lookup_wide_(SolveLookupView k, uint64_t p0, uint64_t p1,
                                                            uint64_t *vals) {
    const uint64_t p = p0 + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p < p1) solve_lookup_entry(k, p, vals);
}

// one workgroup of 512 or 768 (GATE: the plan has gate entries): levels l0 ..
// l1 - 1, each of at most 256 entries in all; lanes 0..255 the arithmetic
// entries, then 256 lanes of gate entries (the body with the NAF kind, whether
// or not the plan has such entries), then the lookup entries in the last four
// waves
template <bool GATE>
__global__ __launch_bounds__(GATE ? 768 : 512) void k_solve_lookup_mixed_(SolveView v, SolveGateView g,
                                                                          SolveLookupView k, uint32_t l0, uint32_t l1,
                                                                          uint64_t *vals, PiList pi) {
    const uint32_t part = threadIdx.x >> 8, lane = threadIdx.x & 255;
    for (uint32_t l = l0; l < l1; l++) {
        if (part == (GATE ? 2 : 1)) {
            const uint64_t p = (uint64_t)k.lvl_off[l] + lane;
            if (p < k.lvl_off[l + 1]) solve_lookup_entry(k, p, vals);
        } else if (GATE && part == 1) {
            const uint64_t p = (uint64_t)g.lvl_off[l] + lane;
            if (p < g.lvl_off[l + 1]) solve_gate_entry<true>(g, p, vals);
        } else {
            const uint64_t p = (uint64_t)v.lvl_off[l] + lane;
            if (p < v.lvl_off[l + 1]) solve_entry(v, p, vals, pi);
        }
        __syncthreads();  // the level's values: written, and visible to this workgroup
    }
}

// the plan has ECC entries too: k_solve_ecc_mixed_'s workgroup of 768, the
// lookup entries in the lanes of the gate waves after the level's gate entries
// (at most 256 of both together).  A fourth part of waves would make it 1024
// lanes, 128 registers a lane, where the ECC body has 151 in the 768-lane
// kernel
__global__ __launch_bounds__(768) void k_solve_lookup_ecc_mixed_(SolveView v, SolveGateView g, bool gates,
                                                                 SolveEccView e, SolveLookupView k, uint32_t l0,
                                                                 uint32_t l1, uint64_t *vals, PiList pi) {
    const uint32_t part = threadIdx.x >> 8, lane = threadIdx.x & 255;
    for (uint32_t l = l0; l < l1; l++) {
        if (part == 2) {
            const uint64_t p = (uint64_t)e.lvl_off[l] + lane;
            if (p < e.lvl_off[l + 1]) solve_ecc_entry(e, p, vals);
        } else if (part == 1) {
            const uint32_t wg = gates ? g.lvl_off[l + 1] - g.lvl_off[l] : 0;
            if (lane < wg) {
                solve_gate_entry<true>(g, (uint64_t)g.lvl_off[l] + lane, vals);
            } else {
                const uint64_t p = (uint64_t)k.lvl_off[l] + (lane - wg);
                if (p < k.lvl_off[l + 1]) solve_lookup_entry(k, p, vals);
            }
        } else {
            const uint64_t p = (uint64_t)v.lvl_off[l] + lane;
            if (p < v.lvl_off[l + 1]) solve_entry(v, p, vals, pi);
        }
        __syncthreads();  // the level's values: written, and visible to this workgroup
    }
}

// after the last level (stream order): a lane an output row, PI = -q_arith S in canonical form
__global__ __launch_bounds__(256) void k_solve_outputs_(SolveOutView o, uint64_t n_out, const uint64_t *vals) {
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (k >= n_out) return;
    const Fr a = load_fr(vals, o.var[0][k]), b = load_fr(vals, o.var[1][k]);
    const Fr c = load_fr(vals, o.var[2][k]), d = load_fr(vals, o.var[3][k]);
    Fr g = fr_mul2(load_fr(o.coef[kSolveQl], k), a, load_fr(o.coef[kSolveQr], k), b);
    g += fr_mul2(load_fr(o.coef[kSolveQo], k), c, load_fr(o.coef[kSolveQ4], k), d);
    g += fr_mul2(load_fr(o.coef[kSolveQhl], k), pow5(a), load_fr(o.coef[kSolveQhr], k), pow5(b));
    g += load_fr(o.coef[kSolveQh4], k) * pow5(d) + load_fr(o.coef[kSolveQc], k);
    if (o.coef[kSolveQm]) g += load_fr(o.coef[kSolveQm], k) * a * b;
    store_fr(o.pi, k, from_mont(g));
}

}  // namespace

void SolveView::lay(void *base, uint64_t n, uint64_t n_levels, uint64_t n_inputs, uint64_t n_out, bool qm) {
    const uint64_t nn = padded(n);
    uint64_t *w = static_cast<uint64_t *>(base);
    for (int c = 0; c < kSolveCoefs; c++) {
        coef[c] = c == kSolveQm && !qm ? nullptr : w;
        if (coef[c]) w += 4 * nn;
    }
    uint32_t *h = reinterpret_cast<uint32_t *>(w);
    tgt = h, row = h + nn;
    for (int j = 0; j < 4; j++) var[j] = h + (2 + j) * nn;
    lvl_off = h + 6 * nn;
    ids = lvl_off + padded(n_levels + 1);
    // the output entries: Fr arrays first, so that they start 16-byte aligned
    const uint64_t no = padded(n_out);
    w = reinterpret_cast<uint64_t *>(ids + padded(n_inputs));
    for (int c = 0; c < kSolveCoefs; c++) {
        out.coef[c] = c == kSolvePik || (c == kSolveQm && !qm) ? nullptr : w;
        if (out.coef[c]) w += 4 * no;
    }
    out.pi = w;
    h = reinterpret_cast<uint32_t *>(w + 4 * no);
    out.row = h;
    for (int j = 0; j < 4; j++) out.var[j] = h + (1 + j) * no;
}

void solve_mark_outputs(const uint64_t *d_rows, uint64_t n_out, uint64_t n_gates, const uint64_t *q_arith,
                        uint32_t *d_bits, uint64_t err[3], DevBuf &scratch, hipStream_t s) {
    scratch.reserve(24);
    PNP_HIP(hipMemsetAsync(scratch.p, 0xff, 24, s));
    PNP_HIP(hipMemsetAsync(d_bits, 0, 4 * ((n_gates + 31) / 32), s));
    hipLaunchKernelGGL(k_solve_mark_outputs_, dim3(nblk(n_out)), dim3(256), 0, s, d_rows, n_out, n_gates, q_arith,
                       d_bits, static_cast<unsigned long long *>(scratch.p));
    PNP_HIP(hipGetLastError());
    PNP_HIP(hipMemcpyAsync(err, scratch.p, 24, hipMemcpyDeviceToHost, s));
    PNP_HIP(hipStreamSynchronize(s));
}

void solve_mark_inputs(const uint32_t *d_ids, uint64_t n_inputs, uint64_t n_vars, uint32_t *d_level, uint32_t err[2],
                       DevBuf &scratch, hipStream_t s) {
    scratch.reserve(8);
    PNP_HIP(hipMemsetAsync(scratch.p, 0xff, 8, s));
    PNP_HIP(hipMemsetAsync(d_level, 0xff, 4 * n_vars, s));
    if (n_inputs) {
        hipLaunchKernelGGL(k_solve_inputs_, dim3(nblk(n_inputs)), dim3(256), 0, s, d_ids, n_inputs, n_vars, d_level,
                           scratch.u32());
        PNP_HIP(hipGetLastError());
    }
    PNP_HIP(hipMemcpyAsync(err, scratch.p, 8, hipMemcpyDeviceToHost, s));
    PNP_HIP(hipStreamSynchronize(s));
}

void solve_rounds(const uint32_t *const d_var[4], uint64_t n_gates, uint64_t n_vars, const SolveSel &sel,
                  const uint32_t *d_out_bits, uint32_t *d_level, uint32_t *d_def, DevBuf &ecc_level, SolveBuild &out,
                  hipStream_t s) {
    const MapArgs a{{d_var[0], d_var[1], d_var[2], d_var[3]}};
    const bool ecc = sel.fixed_add || sel.var_add, lk = sel.lookup != nullptr;
    const bool gates = sel.range || sel.logic || ecc || lk;
    const size_t ctr_bytes = lk ? 36 : ecc ? 32 : 16;
    DevBuf mask(n_gates), gmask, winner(4 * n_vars), ctr(48);
    if (gates) gmask.alloc(n_gates);
    if (ecc) {
        ecc_level.alloc(4 * kSolveEccKinds * n_gates);
        PNP_HIP(hipMemsetAsync(ecc_level.p, 0, 4 * kSolveEccKinds * n_gates, s));
    }
    uint8_t *d_mask = static_cast<uint8_t *>(mask.p), *d_gmask = static_cast<uint8_t *>(gmask.p);
    PNP_HIP(hipMemsetAsync(winner.p, 0xff, 4 * n_vars, s));
    hipLaunchKernelGGL(k_solve_mask_, dim3(nblk(n_gates)), dim3(256), 0, s, sel, n_gates, d_out_bits,
                       d_mask, d_gmask);
    PNP_HIP(hipGetLastError());
    out.widths.clear();
    out.gate_widths.clear();
    out.ecc_widths.clear();
    out.ecc_vars.clear();
    out.lookup_widths.clear();
    out.n_range = out.n_logic = out.n_two = out.n_fixed = out.n_var = out.n_lookup = 0;
    // (a round defines at least one variable, so there are at most n_vars of them)
    for (uint64_t t = 1; t <= n_vars; t++) {
        PNP_HIP(hipMemsetAsync(ctr.p, 0, ctr_bytes, s));
        auto round = [&](auto ready, auto commit) {
            hipLaunchKernelGGL(ready, dim3(nblk(n_gates)), dim3(256), 0, s, a, n_gates, n_vars, d_mask, d_gmask, d_level,
                               winner.u32());
            hipLaunchKernelGGL(commit, dim3(nblk(n_gates)), dim3(256), 0, s, a, n_gates, n_vars, d_mask, d_gmask,
                               d_level, winner.u32(), d_def, (uint32_t)t, ctr.u32(), ecc_level.u32());
        };
        if (ecc && lk) round(k_solve_ready_<true, true>, k_solve_commit_<true, true>);
        else if (lk) round(k_solve_ready_<false, true>, k_solve_commit_<false, true>);
        else if (ecc) round(k_solve_ready_<true, false>, k_solve_commit_<true, false>);
        else round(k_solve_ready_<false, false>, k_solve_commit_<false, false>);
        PNP_HIP(hipGetLastError());
        // arithmetic, range, logic; of those, two sources; fixed-add scalar, fixed-add others, var-add; ECC entries;
        // lookup
        uint32_t won[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        PNP_HIP(hipMemcpyAsync(won, ctr.p, ctr_bytes, hipMemcpyDeviceToHost, s));
        PNP_HIP(hipStreamSynchronize(s));
        if (!(won[0] + won[1] + won[2] + won[4] + won[5] + won[6] + won[8])) break;
        out.widths.push_back(won[0]);
        out.gate_widths.push_back(won[1] + won[2] + won[4]);
        out.ecc_widths.push_back(won[7]);
        out.ecc_vars.push_back(won[5] + won[6]);
        out.n_range += won[1];
        out.n_logic += won[2];
        out.n_two += won[3];
        out.n_fixed += won[4] + won[5];
        out.n_var += won[6];
        out.lookup_widths.push_back(won[8]);
        out.n_lookup += won[8];
    }
    uint32_t un[2] = {0, kUnset};
    PNP_HIP(hipMemcpyAsync(ctr.p, un, 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_solve_unset_, dim3(nblk(n_vars)), dim3(256), 0, s, d_level, n_vars, ctr.u32());
    PNP_HIP(hipGetLastError());
    PNP_HIP(hipMemcpyAsync(un, ctr.p, 8, hipMemcpyDeviceToHost, s));
    PNP_HIP(hipStreamSynchronize(s));
    out.n_undetermined = un[0];
    out.first_undetermined = un[1];
}

void solve_emit(const uint32_t *const d_var[4], uint64_t n_gates, uint64_t n_vars, const SolveSel &sel,
                const uint32_t *d_level, const uint32_t *d_def, const uint32_t *d_ecc_level, const SolveBuild &b,
                const uint64_t *d_out_rows, uint64_t n_out, const SolveView &v, const SolveGateView &g,
                const SolveEccView &e, const SolveLookupView &k, hipStream_t s) {
    const uint32_t n_levels = (uint32_t)b.widths.size();
    std::vector<uint32_t> off(n_levels + 1, 0), goff(n_levels + 1, 0), eoff(n_levels + 1, 0), koff(n_levels + 1, 0);
    for (uint32_t l = 0; l < n_levels; l++) {
        off[l + 1] = off[l] + b.widths[l];
        goff[l + 1] = goff[l] + b.gate_widths[l];
        eoff[l + 1] = eoff[l] + b.ecc_widths[l];
        koff[l + 1] = koff[l] + b.lookup_widths[l];
    }
    const uint64_t n = off[n_levels], n_gate = goff[n_levels], n_ecc = eoff[n_levels], n_lookup = koff[n_levels];
    PNP_HIP(hipMemcpyAsync(v.lvl_off, off.data(), 4 * off.size(), hipMemcpyHostToDevice, s));
    if (n_gate) PNP_HIP(hipMemcpyAsync(g.lvl_off, goff.data(), 4 * goff.size(), hipMemcpyHostToDevice, s));
    if (n_ecc) PNP_HIP(hipMemcpyAsync(e.lvl_off, eoff.data(), 4 * eoff.size(), hipMemcpyHostToDevice, s));
    if (n_lookup) PNP_HIP(hipMemcpyAsync(k.lvl_off, koff.data(), 4 * koff.size(), hipMemcpyHostToDevice, s));
    const MapArgs a{{d_var[0], d_var[1], d_var[2], d_var[3]}};
    if (n_out) {  // products, not quotients: no inverse
        hipLaunchKernelGGL(k_solve_out_emit_, dim3(nblk(n_out)), dim3(256), 0, s, a, sel, d_out_rows, n_out, v.out);
        PNP_HIP(hipGetLastError());
    }
    if (n + n_gate) {  // the arithmetic entries by level, then (a plan that has them) the gate entries by level
        DevBuf keys(4 * n_vars), sort_scratch, den, inv_scratch;
        const uint32_t top = n_gate ? 2 * n_levels : n_levels;
        hipLaunchKernelGGL(k_solve_keys_, dim3(nblk(n_vars)), dim3(256), 0, s, d_level, d_def, n_vars, n_levels,
                           n_gate != 0, keys.u32());
        PNP_HIP(hipGetLastError());
        int bits = 1;
        while (bits < 32 && (top >> bits)) bits++;
        const uint32_t *order = sort_positions_u32(keys.u32(), n_vars, bits, sort_scratch, s);
        if (n) {
            den.alloc(64 * n);
            hipLaunchKernelGGL(k_solve_denoms_, dim3(nblk(n)), dim3(256), 0, s, a, sel, order, d_def, n, n_vars, v,
                               den.u64());
            PNP_HIP(hipGetLastError());
            k_batch_inverse(den.u64(), 2 * n, inv_scratch, s);
            hipLaunchKernelGGL(k_solve_fold_, dim3(nblk(n)), dim3(256), 0, s, sel, n, v, d_def, den.u64());
            PNP_HIP(hipGetLastError());
        }
        if (n_gate) {
            hipLaunchKernelGGL(k_solve_gate_emit_, dim3(nblk(n_gate)), dim3(256), 0, s, a, sel, order + n, d_def,
                               n_gate, n_gates, n_vars, g);
            PNP_HIP(hipGetLastError());
        }
    }
    if (n_ecc) {  // the (row, kind) pairs by round, ties in (row, kind) order
        const uint64_t m = kSolveEccKinds * n_gates;
        DevBuf keys(4 * m), sort_scratch;
        hipLaunchKernelGGL(k_solve_ecc_keys_, dim3(nblk(m)), dim3(256), 0, s, d_ecc_level, m, n_levels, keys.u32());
        PNP_HIP(hipGetLastError());
        int bits = 1;
        while (bits < 32 && (n_levels >> bits)) bits++;
        const uint32_t *order = sort_positions_u32(keys.u32(), m, bits, sort_scratch, s);
        hipLaunchKernelGGL(k_solve_ecc_emit_, dim3(nblk(n_ecc)), dim3(256), 0, s, a, sel, order, d_level, d_def,
                           d_ecc_level, n_ecc, n_gates, n_vars, e);
        PNP_HIP(hipGetLastError());
        PNP_HIP(hipStreamSynchronize(s));
    }
    if (n_lookup) {  // the variables lookup rows define by level, ties in variable order
        DevBuf keys(4 * n_vars), sort_scratch;
        hipLaunchKernelGGL(k_solve_lookup_keys_, dim3(nblk(n_vars)), dim3(256), 0, s, d_level, d_def, n_vars, n_levels,
                           keys.u32());
        PNP_HIP(hipGetLastError());
        int bits = 1;
        while (bits < 32 && (n_levels >> bits)) bits++;
        const uint32_t *order = sort_positions_u32(keys.u32(), n_vars, bits, sort_scratch, s);
        hipLaunchKernelGGL(k_solve_lookup_emit_, dim3(nblk(n_lookup)), dim3(256), 0, s, a, order, d_def, n_lookup,
                           n_vars, k.ent);
        PNP_HIP(hipGetLastError());
        PNP_HIP(hipStreamSynchronize(s));
    }
    PNP_HIP(hipStreamSynchronize(s));  // (off and the scratch go out of scope)
}

uint64_t solve_lookup_index(const uint64_t *const t[4], uint64_t D, DevBuf &index, SolveLookupView &k, hipStream_t s) {
    const LookupCols tc{{t[0], t[1], t[2], t[3]}};
    const uint64_t n_part = 4 * (uint64_t)nblk(D);
    DevBuf part(4 * n_part), total(32), keys(4 * D), sort_scratch;
    hipLaunchKernelGGL(k_solve_lookup_count_, dim3(nblk(D)), dim3(256), 0, s, tc, D, part.u32());
    hipLaunchKernelGGL(k_solve_lookup_sum_, dim3(1), dim3(256), 0, s, part.u32(), n_part, total.u32());
    PNP_HIP(hipGetLastError());
    uint32_t m32 = 0;
    PNP_HIP(hipMemcpyAsync(&m32, total.p, 4, hipMemcpyDeviceToHost, s));
    PNP_HIP(hipStreamSynchronize(s));
    const uint64_t m = m32, B = SolveLookupView::buckets(m);
    index.alloc(SolveLookupView::index_bytes(m));
    uint32_t *off = index.u32(), *rows = off + SolveView::padded(B + 1);
    hipLaunchKernelGGL(k_solve_lookup_buckets_, dim3(nblk(D)), dim3(256), 0, s, tc, D, (uint32_t)B, keys.u32());
    PNP_HIP(hipGetLastError());
    int bits = 1;
    while (bits < 32 && (B >> bits)) bits++;  // (keys 0 .. B)
    const uint32_t *order = sort_positions_u32(keys.u32(), D, bits, sort_scratch, s);
    hipLaunchKernelGGL(k_solve_lookup_csr_, dim3(nblk(std::max(B + 1, m))), dim3(256), 0, s, keys.u32(), order, D,
                       (uint32_t)B, m, off, rows);
    PNP_HIP(hipGetLastError());
    PNP_HIP(hipStreamSynchronize(s));  // (the scratch goes out of scope)
    k.off = off, k.rows = rows, k.bmask = (uint32_t)(B - 1);
    for (int j = 0; j < 4; j++) k.t[j] = t[j];
    return m;
}

void k_solve_scatter(const uint32_t *d_ids, const uint64_t *d_in, uint64_t n_inputs, uint64_t *d_vals, hipStream_t s) {
    if (!n_inputs) return;
    hipLaunchKernelGGL(k_solve_scatter_, dim3(nblk(n_inputs)), dim3(256), 0, s, d_ids, d_in, n_inputs, d_vals);
    PNP_HIP(hipGetLastError());
}

void k_solve_outputs(const SolveView &v, uint64_t n_out, const uint64_t *d_vals, hipStream_t s) {
    if (!n_out) return;
    hipLaunchKernelGGL(k_solve_outputs_, dim3(nblk(n_out)), dim3(256), 0, s, v.out, n_out, d_vals);
    PNP_HIP(hipGetLastError());
}

void k_solve_levels(const SolveView &v, uint32_t l0, uint32_t l1, uint64_t p0, uint64_t p1, bool wide, uint64_t *d_vals,
                    const uint64_t *pi_pos, const uint64_t *pi_val, uint32_t n_pi, hipStream_t s) {
    const PiList pi{pi_pos, pi_val, n_pi};
    if (wide) hipLaunchKernelGGL(k_solve_wide_, dim3(nblk(p1 - p0)), dim3(256), 0, s, v, p0, p1, d_vals, pi);
    else hipLaunchKernelGGL(k_solve_narrow_, dim3(1), dim3(256), 0, s, v, l0, l1, d_vals, pi);
    PNP_HIP(hipGetLastError());
}

void k_solve_gate_level(const SolveGateView &g, uint64_t g0, uint64_t g1, uint64_t *d_vals, hipStream_t s, bool naf) {
    if (g1 <= g0) return;
    if (naf) hipLaunchKernelGGL(k_solve_gate_wide_<true>, dim3(nblk(g1 - g0)), dim3(256), 0, s, g, g0, g1, d_vals);
    else hipLaunchKernelGGL(k_solve_gate_wide_<false>, dim3(nblk(g1 - g0)), dim3(256), 0, s, g, g0, g1, d_vals);
    PNP_HIP(hipGetLastError());
}

void k_solve_ecc_level(const SolveEccView &e, uint64_t e0, uint64_t e1, uint64_t *d_vals, hipStream_t s) {
    if (e1 <= e0) return;
    hipLaunchKernelGGL(k_solve_ecc_wide_, dim3(nblk(e1 - e0)), dim3(256), 0, s, e, e0, e1, d_vals);
    PNP_HIP(hipGetLastError());
}

void k_solve_ecc_levels(const SolveView &v, const SolveGateView &g, bool gates, const SolveEccView &e, uint32_t l0,
                        uint32_t l1, uint64_t *d_vals, const uint64_t *pi_pos, const uint64_t *pi_val, uint32_t n_pi,
                        hipStream_t s) {
    const PiList pi{pi_pos, pi_val, n_pi};
    hipLaunchKernelGGL(k_solve_ecc_mixed_, dim3(1), dim3(768), 0, s, v, g, gates, e, l0, l1, d_vals, pi);
    PNP_HIP(hipGetLastError());
}

void k_solve_lookup_level(const SolveLookupView &k, uint64_t k0, uint64_t k1, uint64_t *d_vals, hipStream_t s) {
    if (k1 <= k0) return;
    hipLaunchKernelGGL(k_solve_lookup_wide_, dim3(nblk(k1 - k0)), dim3(256), 0, s, k, k0, k1, d_vals);
    PNP_HIP(hipGetLastError());
}

void k_solve_lookup_levels(const SolveView &v, const SolveGateView &g, bool gates, const SolveEccView &e,
                           bool ecc, const SolveLookupView &k, uint32_t l0, uint32_t l1, uint64_t *d_vals,
                           const uint64_t *pi_pos, const uint64_t *pi_val, uint32_t n_pi, hipStream_t s) {
    const PiList pi{pi_pos, pi_val, n_pi};
    if (ecc)
        hipLaunchKernelGGL(k_solve_lookup_ecc_mixed_, dim3(1), dim3(768), 0, s, v, g, gates, e, k, l0, l1, d_vals, pi);
    else if (gates)
        hipLaunchKernelGGL(k_solve_lookup_mixed_<true>, dim3(1), dim3(768), 0, s, v, g, k, l0, l1, d_vals, pi);
    else
        hipLaunchKernelGGL(k_solve_lookup_mixed_<false>, dim3(1), dim3(512), 0, s, v, g, k, l0, l1, d_vals, pi);
    PNP_HIP(hipGetLastError());
}

void k_solve_mixed_levels(const SolveView &v, const SolveGateView &g, uint32_t l0, uint32_t l1, uint64_t *d_vals,
                          const uint64_t *pi_pos, const uint64_t *pi_val, uint32_t n_pi, hipStream_t s, bool naf) {
    const PiList pi{pi_pos, pi_val, n_pi};
    if (naf) hipLaunchKernelGGL(k_solve_mixed_<true>, dim3(1), dim3(512), 0, s, v, g, l0, l1, d_vals, pi);
    else hipLaunchKernelGGL(k_solve_mixed_<false>, dim3(1), dim3(512), 0, s, v, g, l0, l1, d_vals, pi);
    PNP_HIP(hipGetLastError());
}

}  // namespace pnp
