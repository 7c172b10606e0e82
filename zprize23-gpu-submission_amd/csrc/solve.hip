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
//                    bids for it, atomicMin of the row on winner[u]
//   k_solve_commit_  the same rows again: the bidder that holds winner[u]
//                    defines u (level[u] = t, def[u] = 4 row + slot).  "Known"
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
// No LDS, no scalar-memory tricks; plain C++ and vector memory operations.
#include "pnp_internal.h"

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

// (an output row's byte is zero from the start: no sweep ever looks at it)
__global__ __launch_bounds__(256) void k_solve_mask_(SolveSel q, uint64_t n_gates, const uint32_t *out_bits,
                                                     uint8_t *mask) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n_gates) return;
    const bool out = out_bits && ((out_bits[i >> 5] >> (i & 31)) & 1);
    mask[i] = out ? (uint8_t)0 : (uint8_t)row_mask(q, i);
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

__global__ __launch_bounds__(256) void k_solve_ready_(MapArgs a, uint64_t n_gates, uint64_t n_vars, uint8_t *mask,
                                                      const uint32_t *level, uint32_t *winner) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n_gates) return;
    const uint32_t m = mask[i];
    if (!m) return;
    uint32_t u = 0;
    int slot = 0;
    const int cnt = unknowns(a, i, m, level, kUnset, n_vars, u, slot);
    if (cnt == 0) mask[i] = 0;  // nothing left to define: a plain constraint from here on
    else if (cnt == 1 && ((m >> (4 + slot)) & 1) && __atomic_load_n(&winner[u], __ATOMIC_RELAXED) > (uint32_t)i)
        atomicMin(&winner[u], (uint32_t)i);
}

__global__ __launch_bounds__(256) void k_solve_commit_(MapArgs a, uint64_t n_gates, uint64_t n_vars, uint8_t *mask,
                                                       uint32_t *level, const uint32_t *winner, uint32_t *def,
                                                       uint32_t t, uint32_t *count) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    bool won = false;
    if (i < n_gates) {
        const uint32_t m = mask[i];
        if (m) {
            uint32_t u = 0;
            int slot = 0;
            const int cnt = unknowns(a, i, m, level, t, n_vars, u, slot);
            if (cnt == 1 && ((m >> (4 + slot)) & 1) && winner[u] == (uint32_t)i) {
                won = true;
                __atomic_store_n(&level[u], t, __ATOMIC_RELAXED);
                def[u] = (uint32_t)(4 * i + slot);
                mask[i] = 0;
            }
        }
    }
    const unsigned long long b = __ballot(won);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (uint32_t)__popcll(b));
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

// sort key: the 0-based level of a solved variable, n_levels for every other
__global__ __launch_bounds__(256) void k_solve_keys_(const uint32_t *level, uint64_t n_vars, uint32_t n_levels,
                                                     uint32_t *key) {
    const uint64_t u = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (u >= n_vars) return;
    const uint32_t l = level[u];
    key[u] = l >= 1 && l <= n_levels ? l - 1 : n_levels;
}

// entry p: its target, row and wires, and the two denominators coef and coef q_arith
__global__ __launch_bounds__(256) void k_solve_denoms_(MapArgs a, SolveSel q, const uint32_t *order,
                                                       const uint32_t *def, uint64_t n, uint64_t n_vars, SolveView v,
                                                       uint64_t *den) {
    const uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t u = order[p] < n_vars ? order[p] : 0, d = def[u];
    const uint64_t i = d >> 2;
    const int slot = (int)(d & 3);
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
                  const uint32_t *d_out_bits, uint32_t *d_level, uint32_t *d_def, SolveBuild &out, hipStream_t s) {
    const MapArgs a{{d_var[0], d_var[1], d_var[2], d_var[3]}};
    DevBuf mask(n_gates), winner(4 * n_vars), ctr(8);
    uint8_t *d_mask = static_cast<uint8_t *>(mask.p);
    PNP_HIP(hipMemsetAsync(winner.p, 0xff, 4 * n_vars, s));
    hipLaunchKernelGGL(k_solve_mask_, dim3(nblk(n_gates)), dim3(256), 0, s, sel, n_gates, d_out_bits,
                       d_mask);
    PNP_HIP(hipGetLastError());
    out.widths.clear();
    // (a round defines at least one variable, so there are at most n_vars of them)
    for (uint64_t t = 1; t <= n_vars; t++) {
        PNP_HIP(hipMemsetAsync(ctr.p, 0, 4, s));
        hipLaunchKernelGGL(k_solve_ready_, dim3(nblk(n_gates)), dim3(256), 0, s, a, n_gates, n_vars, d_mask, d_level,
                           winner.u32());
        hipLaunchKernelGGL(k_solve_commit_, dim3(nblk(n_gates)), dim3(256), 0, s, a, n_gates, n_vars, d_mask, d_level,
                           winner.u32(), d_def, (uint32_t)t, ctr.u32());
        PNP_HIP(hipGetLastError());
        uint32_t won = 0;
        PNP_HIP(hipMemcpyAsync(&won, ctr.p, 4, hipMemcpyDeviceToHost, s));
        PNP_HIP(hipStreamSynchronize(s));
        if (!won) break;
        out.widths.push_back(won);
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

void solve_emit(const uint32_t *const d_var[4], uint64_t n_vars, const SolveSel &sel, const uint32_t *d_level,
                const uint32_t *d_def, const SolveBuild &b, const uint64_t *d_out_rows, uint64_t n_out,
                const SolveView &v, hipStream_t s) {
    const uint32_t n_levels = (uint32_t)b.widths.size();
    std::vector<uint32_t> off(n_levels + 1, 0);
    for (uint32_t l = 0; l < n_levels; l++) off[l + 1] = off[l] + b.widths[l];
    const uint64_t n = off[n_levels];
    PNP_HIP(hipMemcpyAsync(v.lvl_off, off.data(), 4 * off.size(), hipMemcpyHostToDevice, s));
    const MapArgs a{{d_var[0], d_var[1], d_var[2], d_var[3]}};
    if (n_out) {  // products, not quotients: no inverse
        hipLaunchKernelGGL(k_solve_out_emit_, dim3(nblk(n_out)), dim3(256), 0, s, a, sel, d_out_rows, n_out, v.out);
        PNP_HIP(hipGetLastError());
    }
    if (n) {
        DevBuf keys(4 * n_vars), sort_scratch, den(64 * n), inv_scratch;
        hipLaunchKernelGGL(k_solve_keys_, dim3(nblk(n_vars)), dim3(256), 0, s, d_level, n_vars, n_levels, keys.u32());
        PNP_HIP(hipGetLastError());
        int bits = 1;
        while (bits < 32 && (n_levels >> bits)) bits++;
        const uint32_t *order = sort_positions_u32(keys.u32(), n_vars, bits, sort_scratch, s);
        hipLaunchKernelGGL(k_solve_denoms_, dim3(nblk(n)), dim3(256), 0, s, a, sel, order, d_def, n, n_vars, v,
                           den.u64());
        PNP_HIP(hipGetLastError());
        k_batch_inverse(den.u64(), 2 * n, inv_scratch, s);
        hipLaunchKernelGGL(k_solve_fold_, dim3(nblk(n)), dim3(256), 0, s, sel, n, v, d_def, den.u64());
        PNP_HIP(hipGetLastError());
    }
    PNP_HIP(hipStreamSynchronize(s));  // (off and the scratch go out of scope)
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

}  // namespace pnp
