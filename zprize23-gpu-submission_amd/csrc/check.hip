// check.hip — does a witness satisfy the circuit?  Row by row, on gfx950.
//
// The quotient evaluates selector(x) * sum_k kappa^k constraint_k on the coset
// (k_widgets_, protocol.hip): an unsatisfied witness makes it a non-polynomial
// and nothing says where.  Here the same constraint expressions (widgets.cuh
// c_range / c_logic / c_fbsm / c_cadd, whose values w_* sum up) run on the
// D rows of the domain itself, one at a time, over the selector ROW values
// (forward transforms of the resident coefficients, check_witness.cpp):
// the composer's check_circuit_satisfied on the GPU.
//
//   k_check_arith_      a lane a row: the arithmetic gate + the row's public
//                       input (a sorted list in HBM, bisected)
//   k_check_family_<F>  a lane a row, one kernel per custom-gate family,
//                       launched only for a family the key has (so each keeps
//                       its own register budget, and a key without custom
//                       gates pays for arithmetic only); the row's selector is
//                       read first, the wires only where it is non-zero
//   k_check_table_set_  the distinct rows of the lookup table as an
//                       open-addressing set of row indices (2 D u32 slots)
//   k_check_lookup_     a lane a row: the membership of its query
//   k_copy_first_ / k_copy_check_   the lowest slot of every variable, then
//                       every slot's value against that slot's
//
// A violation is recorded by record(): one 64-bit atomicMin on (row, kind,
// index) and one atomicAdd per wave of the __ballot popcounts.  Both commute,
// so the report never depends on the order the atomics land in; a satisfied
// witness performs none.  No LDS; plain C++ and vector memory operations.
#include "pnp_internal.h"
#include "widgets.cuh"

namespace pnp {

namespace {

inline uint32_t nblk(uint64_t threads, uint32_t bs = 256) { return (uint32_t)((threads + bs - 1) / bs); }

constexpr uint32_t kEmpty = 0xFFFFFFFFu;

// Every lane of the wave calls this (no lane has returned): `bad` bit k = this
// lane's row violates constraint k of `kind`, k < nk.
__device__ __forceinline__ void record(CheckRecord *rec, uint64_t row, uint32_t kind, uint32_t bad, int nk) {
    if (!__ballot(bad != 0)) return;
    uint32_t cnt = 0;
    for (int k = 0; k < nk; k++) cnt += (uint32_t)__popcll(__ballot((bad >> k) & 1));
    if (bad)
        atomicMin(&rec->first, (unsigned long long)((row << 8) | ((uint64_t)kind << 4) | (uint32_t)(__ffs((int)bad) - 1)));
    if ((threadIdx.x & 63) == 0) atomicAdd(&rec->by_kind[kind], (unsigned long long)cnt);
}

__device__ __forceinline__ Fr pow5(const Fr &x) {
    const Fr x2 = x * x;
    return x2 * x2 * x;
}

// q_arith (q_m ab + q_l a + q_r b + q_o c + q_4 d + q_hl a^5 + q_hr b^5 + q_h4 d^5 + q_c) + PI
// (widget/arithmetic.rs:45-80; the quotient adds the PI polynomial beside it)
__global__ __launch_bounds__(256) void k_check_arith_(CheckRows r, CheckRecord *rec) {
    const uint64_t D = 1ULL << r.lg;
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    if (i < D) {
        const Fr a = load_fr(r.w[0], i), b = load_fr(r.w[1], i), c = load_fr(r.w[2], i), d = load_fr(r.w[3], i);
        Fr g = fr_mul2(load_fr(r.q_l, i), a, load_fr(r.q_r, i), b);
        g += fr_mul2(load_fr(r.q_o, i), c, load_fr(r.q_4, i), d);
        g += fr_mul2(load_fr(r.q_hl, i), pow5(a), load_fr(r.q_hr, i), pow5(b));
        g += load_fr(r.q_h4, i) * pow5(d) + load_fr(r.q_c, i);
        if (r.q_m) g += load_fr(r.q_m, i) * a * b;
        Fr v = load_fr(r.q_arith, i) * g;
        uint32_t lo = 0, hi = r.n_pi;  // the first listed row >= i
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (r.pi_pos[mid] < i) lo = mid + 1;
            else hi = mid;
        }
        if (lo < r.n_pi && r.pi_pos[lo] == i) v += load_fr(r.pi_val, lo);
        bad = v.is_zero() ? 0u : 1u;
    }
    record(rec, i, PNP_CHECK_ARITH, bad, 1);
}

template <int F>
struct Family;
template <>
struct Family<0> {
    static constexpr int kind = PNP_CHECK_RANGE, nk = kRangeConstraints;
    static constexpr bool next_ab = false, sel_c = false, sel_lr = false;
    template <class Emit>
    static __device__ __forceinline__ void each(const WidgetVals &w, Emit &&emit) { c_range(w, emit); }
};
template <>
struct Family<1> {
    static constexpr int kind = PNP_CHECK_LOGIC, nk = kLogicConstraints;
    static constexpr bool next_ab = true, sel_c = true, sel_lr = false;
    template <class Emit>
    static __device__ __forceinline__ void each(const WidgetVals &w, Emit &&emit) { c_logic(w, emit); }
};
template <>
struct Family<2> {
    static constexpr int kind = PNP_CHECK_FIXED_ADD, nk = kFbsmConstraints;
    static constexpr bool next_ab = true, sel_c = true, sel_lr = true;
    template <class Emit>
    static __device__ __forceinline__ void each(const WidgetVals &w, Emit &&emit) { c_fbsm(w, emit); }
};
template <>
struct Family<3> {
    static constexpr int kind = PNP_CHECK_VAR_ADD, nk = kCaddConstraints;
    static constexpr bool next_ab = true, sel_c = false, sel_lr = false;
    template <class Emit>
    static __device__ __forceinline__ void each(const WidgetVals &w, Emit &&emit) { c_cadd(w, emit); }
};

// selector row != 0 and constraint k != 0  <=>  selector * constraint_k != 0
// (Fr has no zero divisors).  "next" is row i + 1 mod D, the quotient's w x.
template <int F>
__global__ __launch_bounds__(256) void k_check_family_(CheckRows r, CheckRecord *rec) {
    using Fam = Family<F>;
    const uint64_t D = 1ULL << r.lg;
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    if (i < D && !load_fr(r.fam[F], i).is_zero()) {
        const uint64_t nx = (i + 1) & (D - 1);
        WidgetVals w;
        w.a = load_fr(r.w[0], i);
        w.b = load_fr(r.w[1], i);
        w.c = load_fr(r.w[2], i);
        w.d = load_fr(r.w[3], i);
        w.d_next = load_fr(r.w[3], nx);
        w.a_next = Fam::next_ab ? load_fr(r.w[0], nx) : Fr::zero();
        w.b_next = Fam::next_ab ? load_fr(r.w[1], nx) : Fr::zero();
        w.q_c = Fam::sel_c ? load_fr(r.q_c, i) : Fr::zero();
        w.q_l = Fam::sel_lr ? load_fr(r.q_l, i) : Fr::zero();
        w.q_r = Fam::sel_lr ? load_fr(r.q_r, i) : Fr::zero();
        Fam::each(w, [&](auto k, const Fr &v) {
            static_assert(decltype(k)::value < Fam::nk, "one bit a constraint");
            bad |= v.is_zero() ? 0u : 1u << decltype(k)::value;
        });
    }
    record(rec, i, Fam::kind, bad, Fam::nk);
}

// ---- lookup: exact membership of a 4 x 256-bit tuple in the table
struct Tuple {
    Fr v[4];
};
struct TableCols {
    const uint64_t *t[4];
};

__device__ __forceinline__ Tuple load_tuple(const uint64_t *const c[4], uint64_t i) {
    Tuple x;
#pragma unroll
    for (int j = 0; j < 4; j++) x.v[j] = load_fr(c[j], i);
    return x;
}
__device__ __forceinline__ bool same(const Tuple &x, const Tuple &y) {
    bool eq = true;
#pragma unroll
    for (int j = 0; j < 4; j++) eq &= x.v[j] == y.v[j];
    return eq;
}
// a mix of the 32 words (only the spread over the slots depends on it)
__device__ __forceinline__ uint32_t tuple_hash(const Tuple &x) {
    uint32_t h = 0x9E3779B9u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            h ^= x.v[j].v[k];
            h *= 0x85EBCA6Bu;
            h = (h << 13) | (h >> 19);
        }
    }
    h ^= h >> 16;
    h *= 0xC2B2AE35u;
    h ^= h >> 15;
    return h;
}

// One lane a table row.  MultiSet::pad repeats row 0 up to D - lookup_len
// times: those rows leave before they touch the set (else millions of lanes
// would meet on one word).  Any other row walks from its slot: an empty slot
// is taken with one CAS (the slot is read first, so an occupied one costs no
// atomic), an occupied one holding an equal row ends the walk (a duplicate),
// any other moves on.  At most D of the 2 D slots fill, so a walk ends.
__global__ __launch_bounds__(256) void k_check_table_set_(TableCols t, uint32_t lg, uint32_t *slots) {
    const uint64_t D = 1ULL << lg;
    const uint64_t row = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (row >= D) return;
    const Tuple me = load_tuple(t.t, row);
    if (row != 0 && same(me, load_tuple(t.t, 0))) return;
    const uint32_t mask = (uint32_t)(2 * D - 1);
    uint32_t h = tuple_hash(me) & mask;
    for (;;) {
        uint32_t cur = __atomic_load_n(&slots[h], __ATOMIC_RELAXED);
        if (cur == kEmpty) {
            cur = atomicCAS(&slots[h], kEmpty, (uint32_t)row);
            if (cur == kEmpty) return;
        }
        if (same(me, load_tuple(t.t, cur))) return;
        h = (h + 1) & mask;
    }
}

// the query rule of the prover (prover.rs:264-283) against the key's selector
__global__ __launch_bounds__(256) void k_check_lookup_(TableCols wc, const uint64_t *s_rows, uint64_t s_n,
                                                       const uint64_t *k_rows, TableCols t, const uint32_t *slots,
                                                       uint32_t lg, CheckRecord *rec) {
    const uint64_t D = 1ULL << lg;
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    if (i < D) {
        const bool s_on = s_rows && i < s_n && !load_fr(s_rows, i).is_zero();
        const bool k_on = k_rows && !load_fr(k_rows, i).is_zero();
        if (s_on) {  // index 0: the wires are queried and must be a table row
            const Tuple q = load_tuple(wc.t, i);
            const uint32_t mask = (uint32_t)(2 * D - 1);
            uint32_t h = tuple_hash(q) & mask;
            for (;;) {
                const uint32_t cur = slots[h];
                if (cur == kEmpty) {
                    bad = 1u;
                    break;
                }
                if (same(q, load_tuple(t.t, cur))) break;
                h = (h + 1) & mask;
            }
        } else if (k_on) {  // index 1: T[0] is queried where the key expects the wires
            if (!same(load_tuple(wc.t, i), load_tuple(t.t, 0))) bad = 2u;
        }
    }
    record(rec, i, PNP_CHECK_LOOKUP, bad, 2);
}

// ---- copy constraints over the wire map: slot = 4 row + wire
struct CopyArgs {
    const uint32_t *var[4];
    const uint64_t *w[4];
};

__global__ __launch_bounds__(256) void k_copy_first_(CopyArgs a, uint64_t n_gates, uint64_t n_vars, uint32_t *first) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n_gates) return;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t v = a.var[j][i], slot = (uint32_t)(4 * i + j);
        // (a variable in many slots, the constant zero: most lanes see a lower slot and leave it)
        if (v < n_vars && __atomic_load_n(&first[v], __ATOMIC_RELAXED) > slot) atomicMin(&first[v], slot);
    }
}

__global__ __launch_bounds__(256) void k_copy_check_(CopyArgs a, uint64_t n_gates, uint64_t n_vars, uint32_t lg,
                                                     const uint32_t *first, CheckRecord *rec) {
    const uint64_t D = 1ULL << lg;
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    if (i < D && i < n_gates) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t v = a.var[j][i];
            if (v >= n_vars) continue;
            const uint32_t f = first[v];
            if (f == (uint32_t)(4 * i + j)) continue;
            const Fr mine = load_fr(a.w[j], i);
            Fr head;
            switch (f & 3) {  // (a.w indexed by a constant: the argument struct stays in registers)
            case 0: head = load_fr(a.w[0], f >> 2); break;
            case 1: head = load_fr(a.w[1], f >> 2); break;
            case 2: head = load_fr(a.w[2], f >> 2); break;
            default: head = load_fr(a.w[3], f >> 2); break;
            }
            if (!(mine == head)) bad |= 1u << j;
        }
    }
    record(rec, i, PNP_CHECK_COPY, bad, 4);
}

}  // namespace

void k_check_reset(CheckRecord *rec, hipStream_t s) {
    PNP_HIP(hipMemsetAsync(rec, 0, sizeof *rec, s));
    PNP_HIP(hipMemsetAsync(&rec->first, 0xff, sizeof rec->first, s));
}

void k_check_arith(const CheckRows &r, CheckRecord *rec, hipStream_t s) {
    hipLaunchKernelGGL(k_check_arith_, dim3(nblk(1ULL << r.lg)), dim3(256), 0, s, r, rec);
    PNP_HIP(hipGetLastError());
}

void k_check_family(int f, const CheckRows &r, CheckRecord *rec, hipStream_t s) {
    const dim3 grid(nblk(1ULL << r.lg)), block(256);
    switch (f) {
    case 0: hipLaunchKernelGGL(k_check_family_<0>, grid, block, 0, s, r, rec); break;
    case 1: hipLaunchKernelGGL(k_check_family_<1>, grid, block, 0, s, r, rec); break;
    case 2: hipLaunchKernelGGL(k_check_family_<2>, grid, block, 0, s, r, rec); break;
    default: hipLaunchKernelGGL(k_check_family_<3>, grid, block, 0, s, r, rec); break;
    }
    PNP_HIP(hipGetLastError());
}

void k_check_table_set(const uint64_t *const t[4], uint32_t lg, uint32_t *slots, hipStream_t s) {
    const uint64_t D = 1ULL << lg;
    PNP_HIP(hipMemsetAsync(slots, 0xff, 8 * D, s));
    TableCols tc{{t[0], t[1], t[2], t[3]}};
    hipLaunchKernelGGL(k_check_table_set_, dim3(nblk(D)), dim3(256), 0, s, tc, lg, slots);
    PNP_HIP(hipGetLastError());
}

void k_check_lookup(const uint64_t *const w[4], const uint64_t *s_rows, uint64_t s_n, const uint64_t *k_rows,
                    const uint64_t *const t[4], const uint32_t *slots, uint32_t lg, CheckRecord *rec, hipStream_t s) {
    TableCols wc{{w[0], w[1], w[2], w[3]}}, tc{{t[0], t[1], t[2], t[3]}};
    hipLaunchKernelGGL(k_check_lookup_, dim3(nblk(1ULL << lg)), dim3(256), 0, s, wc, s_rows, s_n, k_rows, tc, slots,
                       lg, rec);
    PNP_HIP(hipGetLastError());
}

void k_check_copy(const uint32_t *const d_var[4], uint64_t n_gates, uint64_t n_vars, const uint64_t *const w[4],
                  uint32_t lg, uint32_t *first, CheckRecord *rec, hipStream_t s) {
    PNP_HIP(hipMemsetAsync(first, 0xff, 4 * n_vars, s));
    CopyArgs a{{d_var[0], d_var[1], d_var[2], d_var[3]}, {w[0], w[1], w[2], w[3]}};
    hipLaunchKernelGGL(k_copy_first_, dim3(nblk(n_gates)), dim3(256), 0, s, a, n_gates, n_vars, first);
    PNP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_copy_check_, dim3(nblk(1ULL << lg)), dim3(256), 0, s, a, n_gates, n_vars, lg, first, rec);
    PNP_HIP(hipGetLastError());
}

}  // namespace pnp
