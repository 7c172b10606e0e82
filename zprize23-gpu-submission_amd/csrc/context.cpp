// context.cpp — what a pnp_ctx does (context.h): the error message, device
// buffers and the HBM counters; the tables derived from the resident SRS and
// the staged host -> HBM upload; the background table build; the HBM plan and
// budget of a key load; the commitments over the resident SRS, the kernel
// timer and the context's lazily made members.
#include <algorithm>
#include <dlfcn.h>
#include <atomic>
#include <mutex>
#include <set>
#include <thread>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include "context.h"
#include "protocol.h"

namespace pnp {

static thread_local char g_err[512] = "";
const char *last_error() { return g_err; }

// an integer switch of the environment, `dflt` when it is not set
static int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// device bytes held by every DevBuf of the process (pnp_hbm_usage)
std::atomic<uint64_t> g_dev_live{0}, g_dev_peak{0};

void DevBuf::alloc(size_t b) {
    release();
    if (b == 0) b = 16;
    // + 64 B past the end: the compiler widens the 8-byte tail load of an F29
    // (ec29.cuh load29: 14 limbs read as 3 x 16 + 8 B) to 16 bytes on the
    // assumption that the element is 16-B aligned; F29s at 56-B strides are only
    // 8-B aligned, so the last one of an array whose end falls on a page boundary
    // would read 8 bytes into the next page (found by tools/ubench_batch_affine
    // faulting on exactly that, DESIGN.md 4 "Fault record")
    hipError_t e = hipMalloc(&p, b + 64);
    if (e != hipSuccess) {
        p = nullptr;
        (void)hipGetLastError();  // clear the sticky out-of-memory status
        set_error("hipMalloc(%zu) failed: %s (%.2f GiB held by this library)", b, hipGetErrorString(e),
                  g_dev_live.load() / 1073741824.0);
        throw Error(PNP_E_NOMEM);
    }
    bytes = b;
    const uint64_t now = g_dev_live.fetch_add(b) + b;
    static const uint64_t trace = [] {  // PNP_HBM_TRACE=bytes: log allocations at least that large
        const char *e = getenv("PNP_HBM_TRACE");
        return e ? strtoull(e, nullptr, 0) : 0ULL;
    }();
    if (trace && b >= trace) {
        Dl_info di{};
        void *ra = __builtin_return_address(0);
        dladdr(ra, &di);
        fprintf(stderr, "pnp hbm: +%zu B (%.3f GiB live) from %s+%#lx\n", b, now / 1073741824.0,
                di.dli_sname ? di.dli_sname : "?", (unsigned long)((char *)ra - (char *)di.dli_saddr));
    }
    uint64_t pk = g_dev_peak.load();
    while (now > pk && !g_dev_peak.compare_exchange_weak(pk, now)) {
    }
}
void DevBuf::release() {
    if (p) {
        (void)hipFree(p);
        g_dev_live.fetch_sub(bytes);
    }
    p = nullptr;
    bytes = 0;
}

// folded table of this rank's point range (msm_point_range) of the first n
// SRS points, rebuilt when n or the sharding changes
const uint64_t *commit_table(pnp_ctx *ctx, uint64_t n) {
    uint64_t p0 = 0, p1 = n;
    if (!ctx->msm.full_table()) msm_point_range(n, ctx->msm.rank, ctx->msm.world, p0, p1);
    if (ctx->ck_table_n != n || ctx->ck_table_p0 != p0 || ctx->ck_table_p1 != p1) {
        ctx->ck_table_n = 0;
        msm_build_table(ctx->ck_table, ctx->ck_dev + 12 * p0, p1 - p0, ctx->msm.fold_c, ctx->stream);
        ctx->ck_table_n = n;
        ctx->ck_table_p0 = p0;
        ctx->ck_table_p1 = p1;
    }
    return ctx->ck_table.u64();
}

// Host -> HBM from the caller's pageable buffers: kStgThreads threads each
// memcpy 8-MiB chunks into two pinned staging buffers of their own and DMA them
// on a stream of their own, so the host copies and the DMAs of several chunks
// overlap (small chunks: pinning the staging memory is a fixed cost of a cold
// call, ~0.4 ms per MiB).  Copies below 4 MiB go through hipMemcpyAsync
// directly.  Measured against HIP's pageable copy (~29-32 GB/s for the 19.5 GB
// prover key of HEIGHT = 15 either way): level on one box, ahead on another
// when the SRS table builds beside the upload (the v1 call one
// proof per process).  PNP_H2D_STAGED=0: hipMemcpyAsync throughout; also the
// fallback when the staging memory cannot be pinned.
static bool h2d_staged_enabled() {
    static const bool on = env_int("PNP_H2D_STAGED", 1) != 0;
    return on;
}
void h2d_release(pnp_ctx *ctx) {
    for (int k = 0; k < 2 * pnp_ctx::kStgThreads; k++) {
        if (ctx->stg_buf[k]) (void)hipHostFree(ctx->stg_buf[k]);
        if (ctx->stg_ev[k]) (void)hipEventDestroy(ctx->stg_ev[k]);
        ctx->stg_buf[k] = nullptr;
        ctx->stg_ev[k] = nullptr;
    }
    for (int t = 0; t < pnp_ctx::kStgThreads; t++) {
        if (ctx->stg_st[t]) (void)hipStreamDestroy(ctx->stg_st[t]);
        ctx->stg_st[t] = nullptr;
    }
}
void h2d_batch(pnp_ctx *ctx, const std::vector<H2D> &copies) {
    constexpr size_t CH = 8u << 20;
    struct Chunk {
        char *dst;
        const char *src;
        size_t bytes;
    };
    std::vector<Chunk> chunks;
    for (const H2D &c : copies) {
        if (!c.bytes) continue;
        if (!h2d_staged_enabled() || c.bytes < (4u << 20)) {
            PNP_HIP(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyHostToDevice, ctx->stream));
            continue;
        }
        for (size_t o = 0; o < c.bytes; o += CH)
            chunks.push_back({static_cast<char *>(c.dst) + o, static_cast<const char *>(c.src) + o,
                              std::min(CH, c.bytes - o)});
    }
    PNP_HIP(hipStreamSynchronize(ctx->stream));
    if (chunks.empty()) return;
    constexpr int T = pnp_ctx::kStgThreads;
    if (!ctx->stg_st[T - 1]) {  // the pool, all of it or none (the last member is made last)
        bool ok = true;
        for (int k = 0; k < 2 * T && ok; k++)
            ok = hipHostMalloc(&ctx->stg_buf[k], CH, hipHostMallocDefault) == hipSuccess &&
                 hipEventCreateWithFlags(&ctx->stg_ev[k], hipEventDisableTiming) == hipSuccess;
        for (int t = 0; t < T && ok; t++)
            ok = hipStreamCreateWithFlags(&ctx->stg_st[t], hipStreamNonBlocking) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            h2d_release(ctx);
            for (const Chunk &c : chunks)
                PNP_HIP(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyHostToDevice, ctx->stream));
            PNP_HIP(hipStreamSynchronize(ctx->stream));
            return;
        }
    }
    std::atomic<size_t> next{0};
    std::atomic<int> failed{0};
    auto worker = [&](int t) {
        try {
            PNP_HIP(hipSetDevice(ctx->device));
            int use = 0;
            for (size_t j; (j = next.fetch_add(1)) < chunks.size() && !failed.load();) {
                const int k = 2 * t + use;
                use ^= 1;
                PNP_HIP(hipEventSynchronize(ctx->stg_ev[k]));  // this buffer's previous DMA has landed
                memcpy(ctx->stg_buf[k], chunks[j].src, chunks[j].bytes);
                PNP_HIP(hipMemcpyAsync(chunks[j].dst, ctx->stg_buf[k], chunks[j].bytes, hipMemcpyHostToDevice,
                                       ctx->stg_st[t]));
                PNP_HIP(hipEventRecord(ctx->stg_ev[k], ctx->stg_st[t]));
            }
            PNP_HIP(hipStreamSynchronize(ctx->stg_st[t]));
        } catch (...) {
            failed.store(1);
            (void)hipStreamSynchronize(ctx->stg_st[t]);  // no DMA of this thread outlives the call
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back(worker, t);
    worker(0);
    for (auto &x : th) x.join();
    if (failed.load()) {
        set_error("host -> HBM staged upload failed");
        throw Error(PNP_E_DEVICE);
    }
}

void ck_derived_reset(pnp_ctx *ctx) {
    ctx->ck_table_n = 0;
    ctx->ck_table.release();
    ctx->lag_n = 0;
    ctx->lag_ok = false;
    ctx->lag_points.release();
    ctx->lag_table_n = 0;
    ctx->lag_table.release();
    wire_bases_reset(ctx);
}

// every rank's verdict on a step that may fail on some rank only (an optional
// table that did not fit its HBM): true when it succeeded on all of them
bool all_ranks_ok(pnp_ctx *ctx, bool mine) {
    if (ctx->msm.world <= 1 || !ctx->msm.allgather) return mine;
    const uint64_t w = mine ? 1 : 0;
    for (uint64_t v : rank_allgather(ctx->msm, ctx->stream, &w, 1, PNP_EX_TAG_STATUS))
        if (!v) return false;
    return true;
}

// ---- background table build (context.h pnp_ctx::bg) ----
thread_local bool t_bg_build = false;
static thread_local std::atomic<bool> *t_bg_cancel = nullptr;

void bg_step(hipStream_t s) {
    if (!t_bg_build) return;
    PNP_HIP(hipStreamSynchronize(s));
    if (t_bg_cancel && t_bg_cancel->load()) {
        set_error("background table build cancelled");
        throw Error(PNP_E_DEVICE);
    }
}

hipStream_t tables_stream(pnp_ctx *ctx) { return t_bg_build ? ctx->bg_stream : ctx->stream; }

// contexts whose builder may still run at process exit (the v1 symbol's
// context is never destroyed): stopped and joined before the HIP runtime's
// own exit handlers run (registered after them, so called first)
static std::mutex g_bg_mu;
static std::set<pnp_ctx *> g_bg_live;
static void bg_atexit() {
    std::vector<pnp_ctx *> live;
    {
        std::lock_guard<std::mutex> lk(g_bg_mu);
        live.assign(g_bg_live.begin(), g_bg_live.end());
    }
    for (pnp_ctx *c : live) tables_cancel(c);
}

static void bg_build(pnp_ctx *ctx, uint64_t n) {
    t_bg_build = true;
    t_bg_cancel = &ctx->bg_cancel;
    bool groups_started = false;
    try {
        PNP_HIP(hipSetDevice(ctx->device));
        if (lagrange_table(ctx, n)) {
            groups_started = true;
            wire_bases_build(ctx, n);
        }
        PNP_HIP(hipStreamSynchronize(ctx->bg_stream));
    } catch (...) {
        // cancelled (a key load or the context's end) or failed: a half-built
        // group set is dropped (the next deferring proof starts a new build,
        // which resumes from the finished Lagrange parts); a failure leaves
        // the proofs without what is not complete
        (void)hipStreamSynchronize(ctx->bg_stream);
        if (groups_started) wire_bases_reset(ctx);
        if (!ctx->bg_cancel.load()) {
            ctx->hbm_lag_off = !(ctx->lag_ok && ctx->lag_table_n == n);
            ctx->hbm_groups_off = true;
        }
    }
    ctx->bg_state.store(2, std::memory_order_release);
}

bool tables_bg_enabled() {
    static const bool on = env_int("PNP_DEFER_BG", 1) != 0;
    return on;
}

void tables_start_background(pnp_ctx *ctx, uint64_t n) {
    if (ctx->msm.world > 1 || ctx->bg.joinable() || !tables_bg_enabled()) return;
    if (!ctx->bg_stream) {
        int lo = 0, hi = 0;
        PNP_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        PNP_HIP(hipStreamCreateWithPriority(&ctx->bg_stream, hipStreamNonBlocking, lo));
    }
    // the builder reads what this proof's stream wrote (the key uploads)
    PNP_HIP(hipStreamSynchronize(ctx->stream));
    {
        static std::once_flag once;
        std::call_once(once, [] { atexit(bg_atexit); });
        std::lock_guard<std::mutex> lk(g_bg_mu);
        g_bg_live.insert(ctx);
    }
    ctx->bg_cancel.store(false);
    ctx->bg_state.store(1, std::memory_order_release);
    ctx->bg = std::thread(bg_build, ctx, n);
}

static void bg_join(pnp_ctx *ctx) {
    if (ctx->bg.joinable()) ctx->bg.join();
    ctx->bg_state.store(0);
    std::lock_guard<std::mutex> lk(g_bg_mu);
    g_bg_live.erase(ctx);
}

bool tables_busy(pnp_ctx *ctx) {
    if (t_bg_build) return false;
    const int st = ctx->bg_state.load(std::memory_order_acquire);
    if (st == 2) bg_join(ctx);
    return st == 1;
}

void tables_wait(pnp_ctx *ctx) {
    if (!t_bg_build && ctx->bg.joinable()) bg_join(ctx);
}

void tables_cancel(pnp_ctx *ctx) {
    if (t_bg_build || !ctx->bg.joinable()) return;
    ctx->bg_cancel.store(true);
    bg_join(ctx);
    ctx->bg_cancel.store(false);
}

bool lagrange_enabled() {
    static const bool enabled = env_int("PNP_LAGRANGE", 1) != 0;
    return enabled;
}

const uint64_t *lagrange_table(pnp_ctx *ctx, uint64_t n) {
    if (!lagrange_enabled() || ctx->hbm_lag_off || n < 2 || (n & (n - 1)) || n > ctx->ck_points) return nullptr;
    if (tables_busy(ctx)) return nullptr;  // being built in the background: commit without it
    uint64_t p0 = 0, p1 = n;
    if (!ctx->msm.full_table()) msm_point_range(n, ctx->msm.rank, ctx->msm.world, p0, p1);
    // a deferring proof uses the table only if it is there
    if (ctx->defer_now && !t_bg_build &&
        !(ctx->lag_n == n && ctx->lag_ok && ctx->lag_table_n == n && ctx->lag_table_p0 == p0 &&
          ctx->lag_table_p1 == p1)) {
        if (!(ctx->lag_n == n && !ctx->lag_ok)) ctx->tables_wanted = true;  // (not a degenerate key)
        return nullptr;
    }
    // (re)built on the same call on every rank (same key and call sequence):
    // a rank whose HBM could not hold it makes every rank go without
    bool built = false, fits = true;
    try {
        if (ctx->lag_n != n) {
            built = true;
            ctx->lag_table_n = 0;
            ctx->lag_table.release();
            ctx->lag_n = 0;
            ctx->lag_points.alloc(n * 96);
            ctx->lag_ok = srs_lagrange(ctx->ck_dev, n, inverse(root_of_unity(log2_exact(n))), inverse(fr_from_u64(n)),
                                       ctx->lag_points.u64(), tables_stream(ctx));
            ctx->lag_n = n;
            if (!ctx->lag_ok) ctx->lag_points.release();
        }
        if (ctx->lag_ok && (ctx->lag_table_n != n || ctx->lag_table_p0 != p0 || ctx->lag_table_p1 != p1)) {
            built = true;
            ctx->lag_table_n = 0;
            msm_build_table(ctx->lag_table, ctx->lag_points.u64() + 12 * p0, p1 - p0, ctx->msm.fold_c,
                            tables_stream(ctx));
            ctx->lag_table_n = n;
            ctx->lag_table_p0 = p0;
            ctx->lag_table_p1 = p1;
        }
    } catch (const Error &e) {
        if (e.code != PNP_E_NOMEM) throw;
        fits = false;
    }
    if (built && !all_ranks_ok(ctx, fits)) fits = false;
    if (!fits) {  // commit from coefficients (prover.cpp), on every rank
        ctx->lag_points.release();
        ctx->lag_table.release();
        ctx->lag_table_n = 0;
        ctx->lag_n = n;
        ctx->lag_ok = false;
        ctx->hbm_lag_off = true;
        return nullptr;
    }
    if (!ctx->lag_ok) return nullptr;
    return ctx->lag_table.u64();
}

// ---- HBM budget (key load) ----
// Upper bounds of what a proof at domain n allocates on this rank, by part:
// the mandatory working set (per-proof buffers, NTT tables, the commit key's
// folded table and its build, the MSM work of the largest batch) and the two
// optional derived tables (the Lagrange basis with its table; the
// copy-constraint groups with theirs), each minus what is already held.
// Checked against the measured peak by tests/test_gpu_hbm.py.
template <class K>
static uint64_t map_bytes(const std::map<K, DevBuf> &m) {
    uint64_t b = 0;
    for (const auto &kv : m) b += kv.second.bytes;
    return b;
}
HbmPlan hbm_plan(pnp_ctx *ctx, uint64_t n) {
    HbmPlan p;
    const MsmWork &wk = ctx->msm;
    const int world = wk.world;
    const bool full = wk.full_table();
    const uint64_t per = (n + world - 1) / world;  // this rank's point range (at most)
    const uint64_t n_tab = full ? n : per;
    const bool dist = ctx->key.nb < 8;
    const uint64_t len = dist ? per : n, NB = (uint64_t)ctx->key.nb * n, N8 = 8 * n;
    const bool lookups = !ctx->key.qlookup_zero();
    // per-proof buffers (prover.cpp ctx->buf): 21 of n always (wires, their
    // coefficients, the lookup / grand-product vectors), the PI and L1
    // polynomials when not in closed form; 11 of the coefficient range (t
    // chunks, linearisation, opening combinations); of the rank's blocks: the
    // wire / z / z2 LDEs and t (7), the PI term's 1 / (x - w^pos), the lookup
    // LDEs, the L1 / PI LDEs when not in closed form; the batch-inverse /
    // scan scratch (about one vector of the longest length)
    const bool closed = ctx->key.std_coset;
    const uint64_t work = 32 * (21 * n + (closed ? 0 : 2 * n) + 11 * len +
                                NB * (8 + (lookups ? 4 : 0) + (closed ? 0 : 2)) + std::max(n, NB) * 9 / 8);
    const uint64_t work_held = map_bytes(ctx->work) + ctx->scratch_a.bytes + ctx->scratch_b.bytes + ctx->key.pinv.bytes;
    // NTT tables: twiddles of n (both directions), the block twists (forward,
    // inverse, x32) of the 8n coset
    // (+ the dense twiddle rows of both directions, 2 x (n - 1) entries)
    const uint64_t ntt = 32 * n + 64 * n + 3 * 32 * N8;
    // (the 8n LDE twist of pnp_coset_lde8 is not a proof's: not counted as held)
    const uint64_t ntt_held = map_bytes(ctx->ntt.fwd) + map_bytes(ctx->ntt.inv) + map_bytes(ctx->ntt.fwd_rows) +
                              map_bytes(ctx->ntt.inv_rows) + map_bytes(ctx->ntt.blk_twist) +
                              map_bytes(ctx->ntt.blk_twist_inv) + map_bytes(ctx->ntt.blk_twist32);
    const uint64_t ck_tab = msm_table_bytes(n_tab, n, wk.fold_c);
    const uint64_t msm = msm_work_bytes(per, n, wk.fold_c, 9, wk.v_bytes, world);
    const uint64_t held = work_held + ntt_held + ctx->ck_table.bytes + msm_work_held(wk);
    const uint64_t total = work + ntt + ck_tab + msm;
    p.mandatory = total > held ? total - held : 0;
    p.t_mand = ctx->ck_table.bytes ? 0 : msm_table_build_bytes(n_tab);
    // the Lagrange basis (n affine points) + its folded table; its build:
    // the radix-2^29 layer array, the window tables, the XYZZ output
    const uint64_t lag = n * 96 + msm_table_bytes(n_tab, n, wk.fold_c);
    const uint64_t lag_held = ctx->lag_points.bytes + ctx->lag_table.bytes;
    const bool lag_built = ctx->lag_n == n && (!ctx->lag_ok || ctx->lag_table_n == n);
    p.lag = lag_built ? 0 : lag > lag_held ? lag - lag_held : 0;
    if (p.lag) p.t_lag = n * (224 + 16 + 192 + 48) + std::min<uint64_t>(n / 2, 1ULL << 18) * 15 * 224;
    // the copy-constraint groups: 5 segments of n slots (this rank's slice in
    // point-range mode), their folded table, the group maps and scalars, the
    // sigma copy; the build: sort keys and labels, XYZZ bases, affine points
    const uint64_t seg = full ? n : (world > 1 ? per : n);
    const uint64_t grp = msm_table_bytes(5 * seg, n, wk.fold_c) + 5 * n * (4 + 4 + 32) + 4 * n * 32;
    uint64_t grp_held = ctx->wb.table.bytes + ctx->wb.sigma.bytes + ctx->wb.flag.bytes;
    for (int j = 0; j < 5; j++) grp_held += ctx->wb.grp[j].bytes + ctx->wb.rep[j].bytes + ctx->wb.scal[j].bytes;
    const bool grp_built = ctx->wb.built && ctx->wb.n == n;
    p.groups = grp_built ? 0 : grp > grp_held ? grp - grp_held : 0;
    if (p.groups)
        p.t_groups = 4 * n * (32 + 8 + 8 + 4 + 4 + 4 + 4 + 4 + 4) + 5 * n * 192 + 5 * seg * (192 + 96) +
                     msm_table_build_bytes(5 * seg);
    p.transient = std::max({p.t_mand, p.t_lag, p.t_groups});
    return p;
}

// The HBM budget, checked by the first proof after a key load (by then the
// caller has released what it no longer needs, e.g. its own 8n key arrays
// once the context holds their block copies): the rank's share of its GPU's
// free HBM (ranks on one device split it) against hbm_plan.  The optional
// tables that do not fit are switched off on every rank (the proof bytes do
// not change); when even the mandatory part does not fit, every rank's proof
// fails with PNP_E_NOMEM before any work, with a message naming the rank and
// the bytes, instead of one rank running out of memory mid-proof and its
// peers failing in an exchange.  PNP_HBM_LIMIT (bytes) caps the budget (tests).
static uint64_t device_key(int dev) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof bus, dev) != hipSuccess) snprintf(bus, sizeof bus, "dev%d", dev);
    uint64_t h = 1469598103934665603ULL;  // FNV-1a
    for (const char *c = bus; *c; c++) h = (h ^ (uint8_t)*c) * 1099511628211ULL;
    return h;
}
void hbm_budget(pnp_ctx *ctx) {
    MsmWork &wk = ctx->msm;
    const int W = wk.world > 1 && wk.allgather ? wk.world : 1;
    uint64_t share = 1;
    if (W > 1) {  // (also the barrier after which every rank's key load has allocated)
        const uint64_t id = device_key(ctx->device);
        share = 0;
        for (uint64_t v : rank_allgather(wk, ctx->stream, &id, 1, PNP_EX_TAG_DEVICE)) share += v == id;
    }
    size_t fr = 0, tot = 0;
    PNP_HIP(hipMemGetInfo(&fr, &tot));
    uint64_t budget = fr / std::max<uint64_t>(share, 1);
    if (const char *e = getenv("PNP_HBM_LIMIT")) {
        const uint64_t lim = strtoull(e, nullptr, 0), live = g_dev_live.load();
        budget = std::min<uint64_t>(budget, lim > live ? lim - live : 0);
    }
    const HbmPlan p = hbm_plan(ctx, ctx->key.n);
    // each optional table with the largest build scratch among what is built
    const uint64_t base = p.mandatory + p.t_mand;
    const uint64_t with_lag = p.mandatory + p.lag + std::max(p.t_mand, p.t_lag);
    const uint64_t with_groups = with_lag - std::max(p.t_mand, p.t_lag) + p.groups +
                                 std::max({p.t_mand, p.t_lag, p.t_groups});
    // PNP_HBM_BUDGET=0: the mandatory part is an upper bound (up to ~3x the
    // measured peak, test_gpu_hbm.py), so a caller that knows better lets the
    // real allocations decide; the optional tables are still sized here
    static const bool hard = env_int("PNP_HBM_BUDGET", 1) != 0;
    constexpr int K = 6;
    uint64_t mine[K];
    mine[0] = !hard || base <= budget;
    mine[1] = lagrange_enabled() && with_lag <= budget;
    mine[2] = mine[1] && wire_groups_enabled() && with_groups <= budget;
    mine[3] = base;
    mine[4] = budget;
    // PNP_DEFER_TABLES is read per process: the ranks defer together or not
    // at all (a deferring rank would skip the table builds' status exchange)
    mine[5] = ctx->defer_tables;
    std::vector<uint64_t> all(mine, mine + K);
    if (W > 1) all = rank_allgather(wk, ctx->stream, mine, K, PNP_EX_TAG_STATUS);
    bool ok = true, lag = true, groups = true, defer = true;
    int bad = -1;
    for (int r = 0; r < W; r++) {
        if (!all[K * r] && bad < 0) bad = r;
        ok &= all[K * r] != 0;
        lag &= all[K * r + 1] != 0;
        groups &= all[K * r + 2] != 0;
        defer &= all[K * r + 5] != 0;
    }
    ctx->hbm_lag_off = !lag;
    ctx->hbm_groups_off = !groups;
    if (!defer) {
        ctx->defer_tables = false;
        ctx->defer_now = false;
    }
    if (!ok) {
        set_error("HBM budget: rank %d of %d needs %.2f GiB more for a proof at n = %llu, %.2f GiB free to it "
                  "(%llu rank(s) on this rank's GPU; PNP_HBM_BUDGET=0 lets the allocations decide)", bad, W,
                  all[K * bad + 3] / 1073741824.0, (unsigned long long)ctx->key.n, all[K * bad + 4] / 1073741824.0,
                  (unsigned long long)share);
        throw Error(PNP_E_NOMEM);
    }
}

void store_affine(const uint64_t *xyzz, int B, CommitmentC *const *out) {
    std::vector<uint64_t> aff((size_t)B * 12);
    xyzz_to_affine_batch_host(xyzz, B, aff.data());
    for (int b = 0; b < B; b++) {
        memcpy(out[b]->x, &aff[12 * b], 48);
        memcpy(out[b]->y, &aff[12 * b + 6], 48);
    }
}

void commit_evals_batch(pnp_ctx *ctx, const uint64_t *const *d_evals, int B, uint64_t n, CommitmentC *const *out) {
    const uint64_t *table = lagrange_table(ctx, n);
    if (!table) {
        set_error("commit from evaluations: no Lagrange-basis key of size %llu", (unsigned long long)n);
        throw Error(PNP_E_ARG);
    }
    std::vector<uint64_t> xyzz((size_t)B * 24);
    msm_run_batch(ctx->msm, ctx->lag_points.u64(), d_evals, B, n, xyzz.data(), ctx->stream, table, false);
    store_affine(xyzz.data(), B, out);
}

void commit_affine(pnp_ctx *ctx, const uint64_t *d_scalars, uint64_t n, CommitmentC *out) {
    uint64_t xyzz[24];
    msm_run(ctx->msm, ctx->ck_dev, d_scalars, n, xyzz, ctx->stream, commit_table(ctx, n));
    store_affine(xyzz, 1, &out);
}

hipEvent_t KernelTimer::get() {
    if (!pool.empty()) {
        hipEvent_t e = pool.back();
        pool.pop_back();
        return e;
    }
    hipEvent_t e;
    PNP_HIP(hipEventCreate(&e));
    return e;
}
void KernelTimer::begin(const char *, hipStream_t s, hipEvent_t &e0) {
    if (!enabled) return;
    e0 = get();
    PNP_HIP(hipEventRecord(e0, s));
}
void KernelTimer::end(const char *name, hipStream_t s, hipEvent_t e0, double bytes) {
    if (!enabled || !e0) return;
    hipEvent_t e1 = get();
    PNP_HIP(hipEventRecord(e1, s));
    pending.push_back({name, e0, e1, bytes});
}
void KernelTimer::collect() {
    for (auto &p : pending) {
        float ms = 0;
        PNP_HIP(hipEventSynchronize(p.e1));  // (no-op once the stream has drained)
        PNP_HIP(hipEventElapsedTime(&ms, p.e0, p.e1));
        auto &st = stats[p.name];
        st.ms += ms;
        st.bytes += p.bytes;
        st.launches += 1;
        pool.push_back(p.e0);
        pool.push_back(p.e1);
    }
    pending.clear();
}

void commit_affine_batch(pnp_ctx *ctx, const uint64_t *const *d_scalars, int B, uint64_t n,
                         CommitmentC *const *out, bool local) {
    std::vector<uint64_t> xyzz((size_t)B * 24);
    msm_run_batch(ctx->msm, ctx->ck_dev, d_scalars, B, n, xyzz.data(), ctx->stream,
                  commit_table(ctx, n), local);
    store_affine(xyzz.data(), B, out);
}

// ---- shared by the check and the solver (check_witness.cpp, solve_witness.cpp)
const uint64_t *KeyRowValues::values(KeyPoly r) {
    if (!ctx->key.has(r)) return nullptr;
    const uint64_t *const *coeffs = reinterpret_cast<const uint64_t *const *>(&ctx->key.dev);
    rows[r].alloc(32ULL << lg);
    ntt_run(ctx->ntt, rows[r].u64(), lg, false, false, ctx->stream, coeffs[kKeyTable[r].coeffs]);
    return rows[r].u64();
}

void DevicePis::upload(const std::vector<uint64_t> &pi_pos, const std::vector<Fr> &pi_val, hipStream_t s) {
    n = (uint32_t)pi_pos.size();
    if (!n) return;
    // (the values start 16-byte aligned: an even count of words before them)
    const size_t val_off = (pi_pos.size() + 1) & ~size_t(1);
    std::vector<uint64_t> packed(val_off + 4 * pi_pos.size());
    for (size_t k = 0; k < pi_pos.size(); k++) {
        packed[k] = pi_pos[k];
        to_u64_limbs(pi_val[k], &packed[val_off + 4 * k]);
    }
    buf.alloc(8 * packed.size());
    PNP_HIP(hipMemcpyAsync(buf.p, packed.data(), 8 * packed.size(), hipMemcpyHostToDevice, s));
    PNP_HIP(hipStreamSynchronize(s));
    pos = buf.u64();
    val = buf.u64() + val_off;
}

void refuse_sharded(pnp_ctx *ctx, const char *what, const char *noun) {
    if (ctx->msm.world <= 1) return;
    set_error("%s: the context is sharded over %d ranks (a multi-rank %s is not supported)", what, ctx->msm.world,
              noun);
    throw Error(PNP_E_ARG);
}

}  // namespace pnp

hipStream_t pnp_ctx::side_stream() {
    if (!stream_lo) {
        int lo = 0, hi = 0;
        PNP_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));  // lo = least priority
        // PNP_SIDE_PRIORITY=hi: the side stream's transforms ahead of the main
        // stream's MSM (experiments)
        const char *pe = getenv("PNP_SIDE_PRIORITY");
        const bool side_hi = pe && !strcmp(pe, "hi");
        PNP_HIP(hipStreamCreateWithPriority(&stream_lo, hipStreamNonBlocking, side_hi ? hi : lo));
        for (hipEvent_t *e : {&ev_fork, &ev_w8, &ev_z8})
            PNP_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    return stream_lo;
}

uint64_t *pnp_ctx::buf(const std::string &name, size_t elems_fr) {
    auto &b = work[name];
    b.reserve(elems_fr * 32);
    return b.u64();
}
