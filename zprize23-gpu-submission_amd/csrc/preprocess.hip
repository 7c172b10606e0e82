// preprocess.hip — circuit preprocessing on gfx950: the copy permutation from
// the composer's wire map, the sigma columns, column padding.
//
// Replaces the CPU side of StandardComposer::preprocess_shared
// (plonk-core/src/proof_system/preprocess.rs:318-520) that is not a transform
// or a commitment:
//   wire_sigma   Permutation::compute_sigma_permutations + compute_permutation_lagrange
//                (permutation/mod.rs:101-213): a HashMap<Variable, Vec<WireData>>
//                filled gate by gate in the order L, R, O, 4, each variable's
//                slots closed into a cycle
//   k_pad_col    the selector columns zero-padded to the domain, the table
//                columns padded with their first entry (MultiSet::pad,
//                lookup/multiset.rs:70-79)
//
// The permutation.  Slot s = 4 row + wire is the order the composer registers
// wires in, so the slots of one variable are its Vec in increasing s and
//   next(s) = the smallest later slot with the same variable, else the
//             variable's first slot.
// That is a stable sort of the slot ids by variable id followed by one linking
// pass: a least-significant-digit radix sort, 8 bits a pass, over
// ceil(log2 n_vars) bits only (a 2^22 Merkle circuit: 3 passes).  A pass is
//   k_sort_hist     per tile of 4096 slots the count of every digit
//   scan            exclusive prefix over (digit, tile), digit major
//   k_sort_scatter  every slot to prefix(digit, tile) + its rank in the tile
// Ranks are by position, not by atomics: a wave matches the lanes that hold
// its digit with 8 ballots, a lane's rank in the wave is the popcount of the
// matching lanes below it, and one lane per digit adds the group's size to the
// wave's own row of LDS counters.  The cost does not depend on the key
// distribution: the Merkle circuit's zero_var in a quarter of all slots (one
// digit in every lane of many waves) takes the 8 ballots of any other wave,
// where per-lane LDS atomics on one bin would serialise 64 deep.  The sort is
// stable by construction (tile, wave, 64-slot chunk, lane order = slot order),
// so the result is the definition's on every run.
#include <algorithm>
#include "pnp_internal.h"

namespace pnp {

namespace {

constexpr int SORT_THREADS = 256;                      // 4 waves
constexpr int SORT_WAVES = SORT_THREADS / 64;
constexpr int SORT_ITEMS = 16;                         // 64-slot chunks a wave ranks
constexpr uint32_t SORT_WAVE_SPAN = 64 * SORT_ITEMS;   // consecutive slots of one wave
constexpr uint32_t SORT_BINS = 256;
constexpr uint32_t SCAN_SPAN = 256 * 16;               // entries one scan block covers
static_assert(SORT_WAVE_SPAN * SORT_WAVES == PNP_SIGMA_TILE, "tile = waves x chunks x 64 slots");

inline uint32_t nblk(uint64_t threads, uint32_t bs = 256) { return (uint32_t)((threads + bs - 1) / bs); }

// flat keys in slot order (key[4 i + j] = var[j][i]) and the first slot whose
// id is not a variable (atomicMin; 0xffffffff = none)
__global__ __launch_bounds__(256) void k_wire_keys(const uint32_t *v0, const uint32_t *v1, const uint32_t *v2,
                                                    const uint32_t *v3, uint64_t n_gates, uint64_t n_vars,
                                                    uint32_t *key, uint32_t *bad) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n_gates) return;
    const uint4 k = make_uint4(v0[i], v1[i], v2[i], v3[i]);
    reinterpret_cast<uint4 *>(key)[i] = k;
    const uint32_t ks[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (ks[j] >= n_vars) {
            atomicMin(bad, (uint32_t)(4 * i + j));
            break;
        }
}

// One wave ranks its SORT_ITEMS chunks of 64 consecutive slots: rank[c] = how
// many earlier slots of the wave's span hold the lane's digit, cnt[d] = the
// span's count of digit d afterwards (cnt: the wave's own 256 LDS counters,
// zero on entry).  Lanes past `m` hold nothing.
__device__ __forceinline__ void wave_rank(const uint32_t *__restrict__ key, uint64_t base, uint64_t m, int shift,
                                          volatile uint32_t *cnt, uint32_t (&k)[SORT_ITEMS],
                                          uint32_t (&rank)[SORT_ITEMS]) {
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long below = (1ULL << lane) - 1;
#pragma unroll
    for (int c = 0; c < SORT_ITEMS; c++) {
        const uint64_t idx = base + 64u * c + lane;
        k[c] = idx < m ? key[idx] : 0;
    }
#pragma unroll
    for (int c = 0; c < SORT_ITEMS; c++) {
        const bool live = base + 64u * c + lane < m;
        const uint32_t d = (k[c] >> shift) & (SORT_BINS - 1);
        unsigned long long peers = __ballot(live);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const unsigned long long has = __ballot((d >> b) & 1);
            peers &= ((d >> b) & 1) ? has : ~has;
        }
        uint32_t r = 0;
        if (live) {
            r = cnt[d] + __popcll(peers & below);
        }
        // every lane has read its counter before the group's first lane moves it on
        __builtin_amdgcn_wave_barrier();
        if (live && (peers & below) == 0) cnt[d] = r + __popcll(peers);
        __builtin_amdgcn_wave_barrier();
        rank[c] = r;
    }
}

__global__ __launch_bounds__(SORT_THREADS) void k_sort_hist(const uint32_t *__restrict__ key, uint64_t m, int shift,
                                                             uint32_t ntiles, uint32_t *__restrict__ hist) {
    __shared__ uint32_t cnt[SORT_WAVES][SORT_BINS];
    const uint32_t t = threadIdx.x, w = t >> 6;
    for (int q = 0; q < SORT_WAVES; q++) cnt[q][t] = 0;
    __syncthreads();
    uint32_t k[SORT_ITEMS], rank[SORT_ITEMS];
    wave_rank(key, (uint64_t)blockIdx.x * PNP_SIGMA_TILE + w * SORT_WAVE_SPAN, m, shift, cnt[w], k, rank);
    __syncthreads();
    uint32_t s = 0;
    for (int q = 0; q < SORT_WAVES; q++) s += cnt[q][t];
    hist[(uint64_t)t * ntiles + blockIdx.x] = s;  // digit major
}

__global__ __launch_bounds__(SORT_THREADS) void k_sort_scatter(const uint32_t *__restrict__ key,
                                                                const uint32_t *__restrict__ val, uint64_t m,
                                                                int shift, uint32_t ntiles,
                                                                const uint32_t *__restrict__ offs,
                                                                uint32_t *__restrict__ key_out,
                                                                uint32_t *__restrict__ val_out) {
    __shared__ uint32_t cnt[SORT_WAVES][SORT_BINS];
    const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63;
    for (int q = 0; q < SORT_WAVES; q++) cnt[q][t] = 0;
    __syncthreads();
    uint32_t k[SORT_ITEMS], rank[SORT_ITEMS];
    const uint64_t base = (uint64_t)blockIdx.x * PNP_SIGMA_TILE + w * SORT_WAVE_SPAN;
    wave_rank(key, base, m, shift, cnt[w], k, rank);
    __syncthreads();
    // digit t: where each wave's slots of it start (the tile's start, then the waves in order)
    {
        uint32_t o = offs[(uint64_t)t * ntiles + blockIdx.x];
        for (int q = 0; q < SORT_WAVES; q++) {
            const uint32_t c = cnt[q][t];
            cnt[q][t] = o;
            o += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < SORT_ITEMS; c++) {
        const uint64_t idx = base + 64u * c + lane;
        if (idx < m) {
            const uint32_t dst = cnt[w][(k[c] >> shift) & (SORT_BINS - 1)] + rank[c];
            if (dst >= m) continue;  // (cannot happen: the counts sum to m; never write outside)
            key_out[dst] = k[c];
            val_out[dst] = val ? val[idx] : (uint32_t)idx;  // (first pass: the slot id is the position)
        }
    }
}

// exclusive prefix of 256 values, one a thread; `total` = their sum
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *wsum, uint32_t &total) {
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += o;
    }
    __syncthreads();  // (wsum may still be read from an earlier call)
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
    for (uint32_t q = 0; q < 4; q++) {
        if (q < w) pre += wsum[q];
        tot += wsum[q];
    }
    total = tot;
    return pre + inc - v;
}

// exclusive scan of n u32 in three launches: the sum of every SCAN_SPAN
// entries, the prefix of those sums (one block), the entries themselves
__global__ __launch_bounds__(256) void k_scan_sums(const uint32_t *__restrict__ a, uint64_t n, uint32_t *sums) {
    __shared__ uint32_t wsum[4];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_SPAN + threadIdx.x * 16u;
    uint32_t s = 0;
    for (int e = 0; e < 16; e++)
        if (base + e < n) s += a[base + e];
    uint32_t total;
    block_excl_scan(s, wsum, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void k_scan_top(uint32_t *sums, uint32_t nseg) {
    __shared__ uint32_t wsum[4];
    uint32_t carry = 0;
    for (uint32_t b = 0; b < nseg; b += 256) {
        const uint32_t i = b + threadIdx.x;
        const uint32_t v = i < nseg ? sums[i] : 0;
        uint32_t total;
        const uint32_t ex = block_excl_scan(v, wsum, total);
        if (i < nseg) sums[i] = carry + ex;
        carry += total;
    }
}
__global__ __launch_bounds__(256) void k_scan_apply(uint32_t *__restrict__ a, uint64_t n, const uint32_t *sums) {
    __shared__ uint32_t wsum[4];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_SPAN + threadIdx.x * 16u;
    uint32_t v[16], s = 0;
    for (int e = 0; e < 16; e++) {
        v[e] = base + e < n ? a[base + e] : 0;
        s += v[e];
    }
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + block_excl_scan(s, wsum, total);
    for (int e = 0; e < 16; e++) {
        if (base + e < n) a[base + e] = run;
        run += v[e];
    }
}

// slot 4 i + j -> position j D + i of the outputs
__device__ __forceinline__ uint32_t slot_pos(uint32_t s, uint32_t lg) { return ((s & 3u) << lg) + (s >> 2); }

// the sorted order closed into cycles: position p's slot maps to the next
// slot of its run, the run's last slot to its first (found by bisection: the
// keys are ascending).  val == nullptr: the identity order (no pass ran).
__global__ __launch_bounds__(256) void k_link(const uint32_t *__restrict__ key, const uint32_t *__restrict__ val,
                                               uint64_t m, uint32_t lg, uint32_t *__restrict__ next) {
    const uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p >= m) return;
    const uint32_t k = key[p];
    uint64_t q = p + 1;
    if (q == m || key[q] != k) {
        uint64_t lo = 0, hi = p;  // the first position holding k lies in [lo, hi]
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (key[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        q = lo;
    }
    const uint32_t s = val ? val[p] : (uint32_t)p, sn = val ? val[q] : (uint32_t)q;
    if (s < m && sn < m) next[slot_pos(s, lg)] = slot_pos(sn, lg);  // (slot ids are < m: a permutation of them)
}

// rows the composer never registered map to themselves
__global__ __launch_bounds__(256) void k_next_identity(uint32_t *next, uint64_t n_gates, uint32_t lg) {
    const uint64_t D = 1ULL << lg, pad = D - n_gates;
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= 4 * pad) return;
    const uint64_t pos = (t / pad) * D + n_gates + t % pad;
    next[pos] = (uint32_t)pos;
}

// sigma_j(w^i) = K_j' w^i' for next(j D + i) = j' D + i', K = (1, 7, 13, 17)
// (permutation/constants.rs); w^e from the NTT's forward twiddle table
// (e < D/2; w^(e + D/2) = -w^e), K x by doublings, as k_perm_numden_
struct SigmaOut {
    uint64_t *p[4];
};
__global__ __launch_bounds__(256) void k_sigma_cols(const uint32_t *__restrict__ next, const uint64_t *__restrict__ tw,
                                                     uint32_t lg, SigmaOut out) {
    const uint64_t D = 1ULL << lg;
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= 4 * D) return;
    uint64_t *dst = out.p[t >> lg];
    if (!dst) return;
    const uint32_t nx = next[t], j = nx >> lg;
    const uint64_t i = nx & (D - 1), half = D > 1 ? D >> 1 : 1;
    const Fr x = i < half ? load_fr(tw, i) : neg(load_fr(tw, i - half));
    const Fr x2 = x + x, x4 = x2 + x2, x8 = x4 + x4;
    const Fr r = j == 0 ? x : j == 1 ? x8 - x : j == 2 ? x8 + x4 + x : x8 + x8 + x;
    store_fr(dst, t & (D - 1), r);
}

// dst[i] = src[i] for i < n, then src[0] (first: MultiSet::pad) or zero up to D.
// In place (dst == src) only the tail is written.
__global__ __launch_bounds__(256) void k_pad_col_(uint64_t *dst, const uint64_t *src, uint64_t n, uint64_t D,
                                                   int first) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;  // one u64 limb a lane
    if (t >= 4 * D) return;
    const uint64_t i = t >> 2;
    if (i < n) {
        if (dst != src) dst[t] = src[t];
    } else {
        dst[t] = first && n ? src[t & 3] : 0;
    }
}

}  // namespace

void k_pad_col(uint64_t *dst, const uint64_t *src, uint64_t n, uint64_t D, bool first, hipStream_t s) {
    hipLaunchKernelGGL(k_pad_col_, dim3(nblk(4 * D)), dim3(256), 0, s, dst, src, n, D, first ? 1 : 0);
    PNP_HIP(hipGetLastError());
}

// the sort's buffers in one allocation of sort_bytes(m): two key and two value
// arrays of m u32 (a pass reads one pair and writes the other), the (digit,
// tile) histogram, the scan's segment sums, and 256 spare bytes behind them
struct SortLayout {
    uint64_t m, hist_n;
    uint32_t ntiles, nseg;
    uint32_t *key[2], *val[2], *hist, *sums;
    SortLayout(uint32_t *buf, uint64_t m_) : m(m_) {
        ntiles = (uint32_t)((m + PNP_SIGMA_TILE - 1) / PNP_SIGMA_TILE);
        hist_n = (uint64_t)SORT_BINS * ntiles;
        nseg = (uint32_t)((hist_n + SCAN_SPAN - 1) / SCAN_SPAN);
        key[0] = buf, key[1] = buf + m, val[0] = buf + 2 * m, val[1] = buf + 3 * m;
        hist = buf + 4 * m, sums = hist + hist_n;
    }
};
static uint64_t sort_bytes(uint64_t m) {
    const uint64_t ntiles = (m + PNP_SIGMA_TILE - 1) / PNP_SIGMA_TILE;
    const uint64_t hist = SORT_BINS * ntiles, nseg = (hist + SCAN_SPAN - 1) / SCAN_SPAN;
    return 4 * m * 4 + hist * 4 + nseg * 4 + 256;
}
// `passes` 8-bit passes over the keys in key[0] (values: the positions);
// returns the pair holding the result
static int sort_passes(const SortLayout &l, int passes, hipStream_t s) {
    int cur = 0;
    for (int pass = 0; pass < passes; pass++, cur ^= 1) {
        const int shift = 8 * pass;
        hipLaunchKernelGGL(k_sort_hist, dim3(l.ntiles), dim3(SORT_THREADS), 0, s, l.key[cur], l.m, shift, l.ntiles,
                           l.hist);
        hipLaunchKernelGGL(k_scan_sums, dim3(l.nseg), dim3(256), 0, s, l.hist, l.hist_n, l.sums);
        hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(256), 0, s, l.sums, l.nseg);
        hipLaunchKernelGGL(k_scan_apply, dim3(l.nseg), dim3(256), 0, s, l.hist, l.hist_n, l.sums);
        hipLaunchKernelGGL(k_sort_scatter, dim3(l.ntiles), dim3(SORT_THREADS), 0, s, l.key[cur],
                           pass ? l.val[cur] : nullptr, l.m, shift, l.ntiles, l.hist, l.key[cur ^ 1], l.val[cur ^ 1]);
        PNP_HIP(hipGetLastError());
    }
    return cur;
}

uint64_t wire_sigma_scratch_bytes(uint64_t n_gates) { return sort_bytes(4 * n_gates); }

// The same stable sort for any m u32 keys below 2^bits (solve.hip: variables
// by level): order[p] = the position the p-th smallest key came from, equal
// keys in position order.  The keys are copied, the result lies in `scratch`
// (grown to fit).  bits >= 1.  Asynchronous on s.
const uint32_t *sort_positions_u32(const uint32_t *d_keys, uint64_t m, int bits, DevBuf &scratch, hipStream_t s) {
    scratch.reserve(sort_bytes(m));
    const SortLayout lay(static_cast<uint32_t *>(scratch.p), m);
    PNP_HIP(hipMemcpyAsync(lay.key[0], d_keys, 4 * m, hipMemcpyDeviceToDevice, s));
    const int passes = (std::max(bits, 1) + 7) / 8;
    return lay.val[sort_passes(lay, passes, s)];
}

// next (4 D u32, must not be null) and the sigma columns (each may be null)
// from the wire map; returns the first slot (4 row + wire) whose id is >=
// n_vars, or ~0 when every id is a variable.  Synchronous; `scratch` is
// (re)allocated to wire_sigma_scratch_bytes and left to the caller.
uint64_t wire_sigma(NttTables &ntt, const uint32_t *const d_var[4], uint64_t n_gates, uint64_t n_vars, uint32_t lg,
                    uint32_t *d_next, uint64_t *const d_sigma[4], DevBuf &scratch, hipStream_t s,
                    WireSigmaStats *stats) {
    const uint64_t m = 4 * n_gates, D = 1ULL << lg;
    scratch.reserve(wire_sigma_scratch_bytes(n_gates));
    const SortLayout lay(static_cast<uint32_t *>(scratch.p), m);
    uint32_t *const *key = lay.key, *const *val = lay.val;
    uint32_t *bad = lay.sums + lay.nseg;
    PNP_HIP(hipMemsetAsync(bad, 0xff, 4, s));
    hipLaunchKernelGGL(k_wire_keys, dim3(nblk(n_gates)), dim3(256), 0, s, d_var[0], d_var[1], d_var[2], d_var[3],
                       n_gates, n_vars, key[0], bad);
    PNP_HIP(hipGetLastError());
    // the bits of the largest id
    int bits = 0;
    const uint64_t top = std::min<uint64_t>(n_vars, 1ULL << 32) - 1;
    while (bits < 32 && (top >> bits)) bits++;
    const int passes = (bits + 7) / 8;
    const int cur = sort_passes(lay, passes, s);
    hipLaunchKernelGGL(k_link, dim3(nblk(m)), dim3(256), 0, s, key[cur], passes ? val[cur] : nullptr, m, lg, d_next);
    if (n_gates < D)
        hipLaunchKernelGGL(k_next_identity, dim3(nblk(4 * (D - n_gates))), dim3(256), 0, s, d_next, n_gates, lg);
    PNP_HIP(hipGetLastError());
    if (d_sigma && (d_sigma[0] || d_sigma[1] || d_sigma[2] || d_sigma[3])) {
        SigmaOut o{{d_sigma[0], d_sigma[1], d_sigma[2], d_sigma[3]}};
        hipLaunchKernelGGL(k_sigma_cols, dim3(nblk(4 * D)), dim3(256), 0, s, d_next, ntt_twiddles(ntt, lg, false, s),
                           lg, o);
        PNP_HIP(hipGetLastError());
    }
    uint32_t h_bad = 0;
    PNP_HIP(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, s));
    PNP_HIP(hipStreamSynchronize(s));
    if (stats) {
        stats->passes = passes;
        // what the passes must move: a pass reads the keys twice (histogram,
        // scatter) and the slot ids once, and writes both
        stats->bytes = (double)passes * m * (4.0 * 2 + 4 + 8) + 16.0 * n_gates * 2 + (double)m * 12;
    }
    return h_bad == 0xffffffffu ? ~0ULL : h_bad;
}

}  // namespace pnp
