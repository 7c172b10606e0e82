// abi.cpp — the extern "C" boundary (include/pnp_plonk.h): the v2 functions,
// which return PNP_* codes and never exit.  What a context does behind them is
// context.cpp, the proof prover.cpp, the prover-key loads prover_key.cpp; the
// v1 gen_proof, which wraps them in the reference's contract, is v1.cpp.  The
// satisfiability check (pnp_check_assignment, pnp_check_witness) is whole
// here, over the kernels of check.hip, and so is the witness solver
// (pnp_load_solve_plan, pnp_solve_assignment, pnp_prove_solved) over those of
// solve.hip.
#include <algorithm>
#include <chrono>
#include <memory>
#include <stdlib.h>
#include <string.h>
#include "context.h"
#include "ec.cuh"
#include "protocol.h"

using namespace pnp;

extern "C" {

const char *pnp_last_error(void) { return last_error(); }

int pnp_ctx_create(int device, pnp_ctx **out) {
    if (!out) return PNP_E_ARG;
    PNP_TRY({
        std::unique_ptr<pnp_ctx> c(new pnp_ctx());
        c->device = device;
        if (const char *e = getenv("PNP_FOLD_C")) c->msm.fold_c = atoi(e);  // experiments
        if (const char *e = getenv("PNP_DEFER_TABLES")) c->defer_tables = atoi(e) != 0 ? 1 : 0;
        PNP_HIP(hipSetDevice(device));
        PNP_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        *out = c.release();
    });
}

void pnp_ctx_destroy(pnp_ctx *ctx) {
    if (!ctx) return;
    tables_cancel(ctx);
    if (ctx->bg_stream) (void)hipStreamDestroy(ctx->bg_stream);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream_lo) {
        (void)hipStreamSynchronize(ctx->stream_lo);
        (void)hipStreamDestroy(ctx->stream_lo);
        for (hipEvent_t e : {ctx->ev_fork, ctx->ev_w8, ctx->ev_z8}) (void)hipEventDestroy(e);
    }
    (void)hipStreamDestroy(ctx->stream);
    h2d_release(ctx);
    for (hipEvent_t e : ctx->ktimer.pool) (void)hipEventDestroy(e);
    for (auto &p : ctx->ktimer.pending) {
        (void)hipEventDestroy(p.e0);
        (void)hipEventDestroy(p.e1);
    }
    delete ctx;
}

int pnp_kernel_timing(pnp_ctx *ctx, int enable) {
    if (!ctx) return PNP_E_ARG;
    ctx->ktimer.enabled = enable != 0;
    ctx->msm.timer = enable ? &ctx->ktimer : nullptr;
    if (enable) ctx->ktimer.stats.clear();
    return PNP_OK;
}

int pnp_kernel_stats(pnp_ctx *ctx, const char *name, double *total_ms, int *launches) {
    if (!ctx || !name) return PNP_E_ARG;
    PNP_TRY({
        ctx->ktimer.collect();  // operator calls leave their events pending
        auto it = ctx->ktimer.stats.find(name);
        if (total_ms) *total_ms = it == ctx->ktimer.stats.end() ? 0.0 : it->second.ms;
        if (launches) *launches = it == ctx->ktimer.stats.end() ? 0 : it->second.launches;
    });
}

int pnp_kernel_bytes(pnp_ctx *ctx, const char *name, double *bytes) {
    if (!ctx || !name || !bytes) return PNP_E_ARG;
    auto it = ctx->ktimer.stats.find(name);
    *bytes = it == ctx->ktimer.stats.end() ? 0.0 : it->second.bytes;
    return PNP_OK;
}

int pnp_set_msm_shard(pnp_ctx *ctx, int rank, int world, pnp_allgather_fn allgather, void *user,
                      uint64_t *d_xbuf, uint64_t xbuf_bytes) {
    if (!ctx || world < 1 || rank < 0 || rank >= world) return PNP_E_ARG;
    if (world > 1 && (!allgather || !d_xbuf)) return PNP_E_ARG;
    // a background table build reads msm.world / rank / allgather (all_ranks_ok)
    // and writes the tables whose point ranges these settings decide: stop it
    // first (the next deferring proof starts a new one)
    tables_cancel(ctx);
    ctx->msm.rank = world > 1 ? rank : 0;
    ctx->msm.world = world;
    ctx->msm.allgather = world > 1 ? allgather : nullptr;
    ctx->msm.user = user;
    ctx->msm.xbuf = world > 1 ? d_xbuf : nullptr;
    ctx->msm.xbuf_bytes = world > 1 ? xbuf_bytes : 0;
    return PNP_OK;
}

int pnp_set_exchange_a2a(pnp_ctx *ctx, pnp_alltoall_fn alltoall, void *user, uint64_t *d_a2a,
                         uint64_t a2a_bytes) {
    if (!ctx || (alltoall && !d_a2a)) return PNP_E_ARG;
    tables_cancel(ctx);  // (as pnp_set_msm_shard)
    ctx->msm.alltoall = alltoall;
    ctx->msm.a2a_user = user;
    ctx->msm.a2a = alltoall ? d_a2a : nullptr;
    ctx->msm.a2a_bytes = alltoall ? a2a_bytes : 0;
    return PNP_OK;
}

int pnp_set_exchange_v(pnp_ctx *ctx, pnp_alltoallv_fn alltoallv, void *user, uint64_t *d_send,
                       uint64_t *d_recv, uint64_t capacity_bytes) {
    if (!ctx || (alltoallv && (!d_send || !d_recv || capacity_bytes < 8))) return PNP_E_ARG;
    tables_cancel(ctx);  // the builder may be writing lag_table, released below
    ctx->msm.alltoallv = alltoallv;
    ctx->msm.v_user = user;
    ctx->msm.v_send = alltoallv ? d_send : nullptr;
    ctx->msm.v_recv = alltoallv ? d_recv : nullptr;
    ctx->msm.v_bytes = alltoallv ? capacity_bytes : 0;
    // the folded tables' point ranges change (the Lagrange points stay)
    ctx->ck_table_n = 0;
    ctx->ck_table.release();
    ctx->lag_table_n = 0;
    ctx->lag_table.release();
    return PNP_OK;
}

int pnp_set_exchange_ordered(pnp_ctx *ctx, int ordered) {
    if (!ctx) return PNP_E_ARG;
    ctx->msm.ordered = ordered != 0;
    return PNP_OK;
}

int pnp_ctx_stream(pnp_ctx *ctx, void **stream) {
    if (!ctx || !stream) return PNP_E_ARG;
    *stream = ctx->stream;
    return PNP_OK;
}

int pnp_sync(pnp_ctx *ctx) {
    if (!ctx) return PNP_E_ARG;
    // (and the background table build: pnp_sync waits for all of the context's work)
    PNP_TRY({
        tables_wait(ctx);
        PNP_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int pnp_ntt(pnp_ctx *ctx, uint64_t *d, uint32_t lg_n, int inverse, int coset) {
    if (!ctx || !d || lg_n > 28) return PNP_E_ARG;
    // timed (pnp_kernel_timing): "ntt", credited 2 x 32 B per element (one
    // read, one write: SURVEY 8(d)'s algorithmic bytes of a transform)
    PNP_TRY({
        hipEvent_t e0 = nullptr;
        ctx->ktimer.begin("ntt", ctx->stream, e0);
        ntt_run(ctx->ntt, d, lg_n, inverse != 0, coset != 0, ctx->stream);
        ctx->ktimer.end("ntt", ctx->stream, e0, 64.0 * (double)(1ULL << lg_n));
    });
}

int pnp_coset_lde8(pnp_ctx *ctx, const uint64_t *in, uint64_t *out8, uint32_t lg_n) {
    if (!ctx || !in || !out8 || lg_n > 25) return PNP_E_ARG;
    PNP_TRY(coset_lde8(ctx->ntt, in, out8, lg_n, ctx->stream));
}

// ---- operator forms of round 4's block-layout transforms (ntt.hip)
static bool blocks_ok(uint32_t lg_n, int m0, int nb) {
    if (m0 >= 0 && nb >= 1 && m0 + nb <= 8 && lg_n <= 25) return true;
    set_error("coset blocks [%d, %d) of [0, 8), lg_n = %u (at most 25)", m0, m0 + nb, lg_n);
    return false;
}

int pnp_lde_blocks(pnp_ctx *ctx, const uint64_t *d_coeffs, uint64_t *d_out, uint32_t lg_n, int m0, int nb,
                   int form29) {
    if (!ctx || !d_coeffs || !d_out || !blocks_ok(lg_n, m0, nb)) return PNP_E_ARG;
    PNP_TRY(lde_blocks(ctx->ntt, d_coeffs, d_out, lg_n, m0, nb, ctx->stream, form29 != 0));
}

int pnp_intt_blocks(pnp_ctx *ctx, uint64_t *d_inout, uint32_t lg_n, int m0, int nb) {
    if (!ctx || !d_inout || !blocks_ok(lg_n, m0, nb)) return PNP_E_ARG;
    PNP_TRY(intt_blocks(ctx->ntt, d_inout, lg_n, m0, nb, ctx->stream));
}

int pnp_to_blocks(pnp_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, uint32_t lg_n, int m0, int nb) {
    if (!ctx || !d_in || !d_out || !blocks_ok(lg_n, m0, nb)) return PNP_E_ARG;
    PNP_TRY(to_blocks(d_in, d_out, lg_n, m0, nb, ctx->stream));
}

// the chunk mask: the device word is zeroed first (as Proof::quotient_chunks
// does), the combine ORs into it, and it comes back in *nz_out
static unsigned *mask_begin(pnp_ctx *ctx) {
    unsigned *d_nz = reinterpret_cast<unsigned *>(ctx->buf("t_nz", 1));
    PNP_HIP(hipMemsetAsync(d_nz, 0, 4, ctx->stream));
    return d_nz;
}
static void mask_end(pnp_ctx *ctx, const unsigned *d_nz, unsigned *nz_out) {
    PNP_HIP(hipMemcpyAsync(nz_out, d_nz, 4, hipMemcpyDeviceToHost, ctx->stream));
    PNP_HIP(hipStreamSynchronize(ctx->stream));
}

int pnp_t_combine_blocks(pnp_ctx *ctx, const uint64_t *d_Y, int nb, uint64_t *d_out, uint32_t lg_n,
                         unsigned *nz_out) {
    if (!ctx || !d_Y || !d_out || !nz_out) return PNP_E_ARG;
    if (nb < 6 || nb > 8 || lg_n > 25) {
        set_error("t_combine_blocks: %d blocks (6 to 8), lg_n = %u (at most 25)", nb, lg_n);
        return PNP_E_ARG;
    }
    PNP_TRY({
        unsigned *d_nz = mask_begin(ctx);
        t_combine_blocks(ctx->ntt, d_Y, nb, d_out, lg_n, d_nz, ctx->stream);
        mask_end(ctx, d_nz, nz_out);
    });
}

int pnp_t_combine_range(pnp_ctx *ctx, const uint64_t *d_Y, uint64_t len, uint64_t q0, uint64_t *d_out,
                        uint32_t lg_n, unsigned *nz_out) {
    if (!ctx || !d_Y || !d_out || !nz_out) return PNP_E_ARG;
    if (lg_n > 25 || q0 > (1ULL << lg_n) || len > (1ULL << lg_n) - q0) {
        set_error("t_combine_range: [%llu, %llu + %llu) outside 2^%u (lg_n at most 25)", (unsigned long long)q0,
                  (unsigned long long)q0, (unsigned long long)len, lg_n);
        return PNP_E_ARG;
    }
    PNP_TRY({
        unsigned *d_nz = mask_begin(ctx);
        if (len) t_combine(ctx->ntt, d_Y, len, q0, d_out, lg_n, d_nz, ctx->stream);
        mask_end(ctx, d_nz, nz_out);
    });
}

int pnp_commit(pnp_ctx *ctx, const uint64_t *d_points, const uint64_t *d_scalars, uint64_t n,
               CommitmentC *out) {
    if (!ctx || !out || (n && (!d_points || !d_scalars))) return PNP_E_ARG;
    PNP_TRY({
        uint64_t xyzz[24];
        msm_run(ctx->msm, d_points, d_scalars, n, xyzz, ctx->stream);
        store_affine(xyzz, 1, &out);
    });
}

int pnp_commit_ck(pnp_ctx *ctx, const uint64_t *d_scalars, uint64_t n, CommitmentC *out) {
    if (!ctx || !out || (n && !d_scalars)) return PNP_E_ARG;
    if (!ctx->ck_loaded) {
        set_error("commit key not loaded");
        return PNP_E_NOKEY;
    }
    if (n > ctx->ck_points) {
        set_error("commit key has %llu points, need %llu", (unsigned long long)ctx->ck_points,
                  (unsigned long long)n);
        return PNP_E_ARG;
    }
    // timed (pnp_kernel_timing): "msm", the whole MSM (digits, sort,
    // accumulation, bucket reduction, result), credited n (96 + 32) B (every
    // point and scalar once); the folded table is built first
    PNP_TRY({
        commit_table(ctx, n);
        hipEvent_t e0 = nullptr;
        ctx->ktimer.begin("msm", ctx->stream, e0);
        commit_affine(ctx, d_scalars, n, out);
        ctx->ktimer.end("msm", ctx->stream, e0, 128.0 * (double)n);
    });
}

int pnp_commit_evals(pnp_ctx *ctx, const uint64_t *d_evals, uint64_t n, CommitmentC *out) {
    if (!ctx || !out || !d_evals) return PNP_E_ARG;
    tables_wait(ctx);  // (a background build of the Lagrange basis finishes first)
    if (!ctx->ck_loaded) {
        set_error("commit key not loaded");
        return PNP_E_NOKEY;
    }
    if (n < 2 || (n & (n - 1)) || n > ctx->ck_points) {
        set_error("commit from evaluations: n = %llu must be a power of two <= %llu", (unsigned long long)n,
                  (unsigned long long)ctx->ck_points);
        return PNP_E_ARG;
    }
    PNP_TRY({
        CommitmentC *o[1] = {out};
        const uint64_t *e[1] = {d_evals};
        commit_evals_batch(ctx, e, 1, n, o);
    });
}

int pnp_hbm_usage(pnp_ctx *ctx, uint64_t out[6]) {
    if (!out) return PNP_E_ARG;
    PNP_TRY({
        if (ctx) tables_wait(ctx);
        out[0] = g_dev_live.load();
        out[1] = g_dev_peak.exchange(out[0]);  // the peak since the previous call
        pnp::HbmPlan p;
        if (ctx && ctx->key.loaded) p = pnp::hbm_plan(ctx, ctx->key.n);
        out[2] = p.mandatory;
        out[3] = p.lag;
        out[4] = p.groups;
        out[5] = p.transient;
    });
}

int pnp_commit_segments(pnp_ctx *ctx, const uint64_t *d_points, uint64_t n_points, int B, const uint64_t *seg_off,
                        const uint64_t *const *d_scalars, uint64_t n, CommitmentC *out) {
    if (!ctx || !out || !seg_off || !d_scalars || B < 1 || B > 16 || (n_points && !d_points)) return PNP_E_ARG;
    for (int b = 0; b < B; b++) {
        if ((n && !d_scalars[b]) || seg_off[b] > n_points || n > n_points - seg_off[b]) {
            set_error("commit segments: MSM %d covers points [%llu, %llu) of %llu", b,
                      (unsigned long long)seg_off[b], (unsigned long long)(seg_off[b] + n),
                      (unsigned long long)n_points);
            return PNP_E_ARG;
        }
    }
    if (ctx->msm.world > 1) {
        set_error("commit segments: single-GPU operator");
        return PNP_E_ARG;
    }
    PNP_TRY({
        std::vector<uint64_t> xyzz((size_t)B * 24);
        if (n != 0) {  // n = 0: every sum is infinity (ZZ = 0)
            DevBuf tab;
            msm_build_table(tab, d_points, n_points, msm_fold_c(n, ctx->msm.fold_c), ctx->stream);
            MsmSegs segs;
            segs.n_table = n_points;
            for (int b = 0; b < B; b++) segs.off[b] = seg_off[b];
            segs.c = msm_fold_c(n, ctx->msm.fold_c);
            msm_run_batch(ctx->msm, nullptr, d_scalars, B, n, xyzz.data(), ctx->stream, tab.u64(), false, &segs);
        }
        CommitmentC *o[16];
        for (int b = 0; b < B; b++) o[b] = out + b;
        store_affine(xyzz.data(), B, o);
    });
}

int pnp_poly_eval(pnp_ctx *ctx, const uint64_t *d, uint64_t n, const uint64_t x[4], uint64_t out[4]) {
    if (!ctx || !d || !x || !out) return PNP_E_ARG;
    PNP_TRY({
        Fr r;
        k_poly_eval(d, n, from_u64_limbs<FrP>(x), ctx->scratch_a, &r, ctx->stream);
        to_u64_limbs(r, out);
    });
}

int pnp_poly_div_linear(pnp_ctx *ctx, uint64_t *d, uint64_t n, const uint64_t z[4]) {
    if (!ctx || !d || !z) return PNP_E_ARG;
    PNP_TRY(k_poly_div_linear(d, n, from_u64_limbs<FrP>(z), ctx->scratch_a, ctx->stream));
}

int pnp_prefix_product(pnp_ctx *ctx, uint64_t *d, uint64_t n) {
    if (!ctx || !d) return PNP_E_ARG;
    PNP_TRY(k_prefix_product(d, n, ctx->scratch_a, ctx->stream));
}

int pnp_batch_inverse(pnp_ctx *ctx, uint64_t *d, uint64_t n) {
    if (!ctx || !d) return PNP_E_ARG;
    PNP_TRY(k_batch_inverse(d, n, ctx->scratch_a, ctx->stream));
}

int pnp_synth_random_fr(pnp_ctx *ctx, uint64_t *d, uint64_t n, uint64_t seed) {
    if (!ctx || !d) return PNP_E_ARG;
    PNP_TRY(k_random_fr(d, n, seed, ctx->stream));
}

int pnp_synth_srs(pnp_ctx *ctx, uint64_t *d, uint64_t n, const uint64_t tau[4]) {
    if (!ctx || !d || !tau) return PNP_E_ARG;
    PNP_TRY(k_srs(d, n, from_u64_limbs<FrP>(tau), ctx->stream));
}

int pnp_synth_circuit(pnp_ctx *ctx, uint64_t *const w[4], uint64_t *const sel[9],
                      uint64_t *const sigma[4], uint64_t n, uint64_t n_gates, uint64_t pi_pos,
                      const uint64_t pi_canon[4]) {
    if (!ctx || !w || !sel || !sigma || !pi_canon || n_gates == 0 || n_gates > n || pi_pos >= n_gates)
        return PNP_E_ARG;
    PNP_TRY(k_synth_circuit(w, sel, sigma, n, n_gates, pi_pos, to_mont(from_u64_limbs<FrP>(pi_canon)),
                            ctx->stream));
}

int pnp_synth_merkle(pnp_ctx *ctx, uint32_t height, const uint64_t *consts, const uint64_t *d_leaves,
                     const uint64_t *d_blind, uint64_t *d_nodes, uint64_t *const w[4], uint64_t *const sel[9],
                     uint64_t *const sigma[4], uint64_t n, uint64_t root_canon[4]) {
    if (!ctx || !consts || !d_leaves || !d_blind || !d_nodes || !w || !sel || !sigma || !root_canon)
        return PNP_E_ARG;
    PNP_TRY({
        std::vector<uint64_t> pc(199 * 4);
        for (int k = 0; k < 199; k++) to_u64_limbs(to_mont(from_u64_limbs<FrP>(consts + 4 * k)), &pc[4 * k]);
        k_synth_merkle((int)height, pc.data(), d_leaves, d_blind, d_nodes, w, sel, sigma, n, ctx->stream);
        uint64_t r[4];
        PNP_HIP(hipMemcpy(r, d_nodes, 32, hipMemcpyDeviceToHost));
        to_u64_limbs(from_mont(from_u64_limbs<FrP>(r)), root_canon);
    });
}

int pnp_synth_coset_consts(pnp_ctx *ctx, uint64_t *d_vh, uint64_t *d_x, uint32_t lg_n) {
    if (!ctx || lg_n > 25) return PNP_E_ARG;
    PNP_TRY(k_coset_consts(d_vh, d_x, lg_n, ctx->stream));
}


int pnp_gather_witness(pnp_ctx *ctx, const uint32_t *const d_var[4], uint64_t n_gates, const uint64_t *d_values,
                       uint64_t n_vars, uint32_t lg_n, uint64_t *const d_w[4]) {
    if (!ctx || !d_var || !d_w || !d_values || n_gates == 0 || lg_n > 25 || n_gates > (1ULL << lg_n))
        return PNP_E_ARG;
    for (int j = 0; j < 4; j++)
        if (!d_var[j] || !d_w[j] || ((uintptr_t)d_w[j] & 15) || ((uintptr_t)d_var[j] & 3)) return PNP_E_ARG;
    if ((uintptr_t)d_values & 15) return PNP_E_ARG;  // (field elements are read and written 16 bytes at a time)
    PNP_TRY({
        PNP_HIP(hipSetDevice(ctx->device));
        pnp::k_gather_witness(d_var, n_gates, d_values, n_vars, lg_n, d_w, ctx->stream);
    });
}

}  // extern "C"

// ---------------------------------------------------------------- keys + prove
namespace {

// make `up` (n_points packed affine points in HBM) the resident SRS.  The
// folded MSM table built from the previous SRS stays valid when the bytes are
// the same (a per-call upload of an unchanged key, as the v1 symbol does).
void adopt_ck(pnp_ctx *ctx, pnp::DevBuf &up, uint64_t n_points) {
    const bool same = ctx->ck_owned.p && ctx->ck_dev == ctx->ck_owned.u64() && ctx->ck_points == n_points &&
                      !pnp::k_any_diff(up.u64(), ctx->ck_owned.u64(), 12 * n_points, ctx->scratch_b, ctx->stream);
    PNP_HIP(hipStreamSynchronize(ctx->stream));
    if (!same) {
        std::swap(ctx->ck_owned, up);
        ctx->ck_dev = ctx->ck_owned.u64();
        pnp::ck_derived_reset(ctx);  // rebuilt from the new key on the next commitment
    }
    ctx->ck_points = n_points;
    ctx->ck_loaded = true;
    ctx->hbm_checked = false;
}

}  // namespace

extern "C" {

int pnp_load_commit_key(pnp_ctx *ctx, const CommitKeyC *ck, uint64_t n_points, int device_ptrs) {
    if (!ctx || !ck || !ck->powers_of_g || n_points == 0) return PNP_E_ARG;
    PNP_TRY({
        tables_wait(ctx);  // a background build reads the SRS being replaced: let it finish
        PNP_HIP(hipSetDevice(ctx->device));
        ctx->ck_loaded = false;
        if (device_ptrs) {
            // the tables derived from the SRS survive a reload of the same
            // bytes (same address, size and content hash)
            uint64_t h[2];
            pnp::k_hash_words(ck->powers_of_g, 12 * n_points, ctx->scratch_b, ctx->stream, h);
            const bool same = ctx->ck_hash_valid && !ctx->ck_owned.p && ctx->ck_dev == ck->powers_of_g &&
                              ctx->ck_points == n_points && h[0] == ctx->ck_hash[0] && h[1] == ctx->ck_hash[1];
            ctx->ck_owned.release();
            ctx->ck_dev = ck->powers_of_g;
            ctx->ck_points = n_points;
            if (!same) pnp::ck_derived_reset(ctx);
            ctx->ck_hash[0] = h[0];
            ctx->ck_hash[1] = h[1];
            ctx->ck_hash_valid = true;
            ctx->ck_loaded = true;
            ctx->hbm_checked = false;
        } else {
            ctx->ck_hash_valid = false;
            // upload (as the reference does per call, load.cu:348-358)
            pnp::DevBuf up(n_points * 96);
            h2d_batch(ctx, {{up.p, ck->powers_of_g, n_points * 96}});
            adopt_ck(ctx, up, n_points);
        }
    });
}

int pnp_load_commit_key_strided(pnp_ctx *ctx, const void *points, uint64_t n_points,
                                const pnp_affine_layout *layout, int device_ptrs) {
    if (!ctx || !points || !layout || n_points == 0) return PNP_E_ARG;
    const pnp_affine_layout L = *layout;
    if (L.stride % 8 || L.x_off % 8 || L.y_off % 8 || L.x_off + 48 > L.stride || L.y_off + 48 > L.stride ||
        L.inf_off >= L.stride || (L.x_off < L.y_off + 48 && L.y_off < L.x_off + 48) ||
        (L.inf_off >= L.x_off && L.inf_off < L.x_off + 48) || (L.inf_off >= L.y_off && L.inf_off < L.y_off + 48)) {
        pnp::set_error("affine layout: stride %llu, x at %llu, y at %llu, infinity at %llu is not a G1Affine layout",
                       (unsigned long long)L.stride, (unsigned long long)L.x_off, (unsigned long long)L.y_off,
                       (unsigned long long)L.inf_off);
        return PNP_E_ARG;
    }
    PNP_TRY({
        tables_wait(ctx);
        PNP_HIP(hipSetDevice(ctx->device));
        ctx->ck_loaded = false;
        pnp::DevBuf raw;
        const uint8_t *src = static_cast<const uint8_t *>(points);
        if (!device_ptrs) {
            raw.alloc(n_points * L.stride);
            PNP_HIP(hipMemcpyAsync(raw.p, points, n_points * L.stride, hipMemcpyHostToDevice, ctx->stream));
            src = static_cast<const uint8_t *>(raw.p);
        }
        pnp::DevBuf up(n_points * 96);
        if (!pnp::k_pack_affine(src, n_points, L.stride, L.x_off, L.y_off, L.inf_off, up.u64(), ctx->scratch_b,
                                ctx->stream)) {
            pnp::set_error("commit key holds the point at infinity (an SRS [tau^i] G never does)");
            throw pnp::Error(PNP_E_ARG);
        }
        raw.release();
        adopt_ck(ctx, up, n_points);
    });
}

uint32_t pnp_proof_infinity_mask(const ProofC *p) {
    if (!p) return 0;
    const CommitmentC *c = reinterpret_cast<const CommitmentC *>(p);
    uint64_t one[6];
    to_u64_limbs(Fq::one(), one);
    uint32_t m = 0;
    for (int k = 0; k < PNP_PROOF_COMMITMENTS; k++) {
        bool x0 = true;
        for (int j = 0; j < 6; j++) x0 &= c[k].x[j] == 0;
        if (x0 && !memcmp(c[k].y, one, 48)) m |= 1u << k;
    }
    return m;
}

int pnp_prove(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, ProofC *out) {
    if (!ctx || !cs || !out) return PNP_E_ARG;
    PNP_TRY(prove_impl(ctx, cs, device_ptrs, out));
}

int pnp_prove_ex(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, uint64_t n_pi, const uint64_t *pi_pos,
                 const uint64_t *pi_canon, const char *label, ProofC *out) {
    if (!ctx || !cs || !out || (n_pi && (!pi_pos || !pi_canon))) return PNP_E_ARG;
    ProveOpts o{n_pi, pi_pos, pi_canon, label ? label : "Merkle tree"};
    PNP_TRY(prove_impl(ctx, cs, device_ptrs, out, &o));
}

int pnp_prove_assignment(pnp_ctx *ctx, const uint64_t *values, uint64_t n_vars, int device_ptrs, uint64_t n_pi,
                         const uint64_t *pi_pos, const uint64_t *pi_canon, const char *label, ProofC *out) {
    if (!ctx || !values || !out || (n_pi && (!pi_pos || !pi_canon))) return PNP_E_ARG;
    if (device_ptrs && ((uintptr_t)values & 15)) {
        set_error("prove assignment: HBM values must be 16-byte aligned");
        return PNP_E_ARG;
    }
    ProveOpts o{n_pi, pi_pos, pi_canon, label ? label : "Merkle tree"};
    Assignment a{values, n_vars};
    PNP_TRY(prove_impl(ctx, nullptr, device_ptrs, out, &o, &a));
}

}  // extern "C"

// ---------------------------------------------------------------- satisfiability check
namespace {

const char *const kCheckKindName[PNP_CHECK_KINDS] = {"arith", "range", "logic", "fixed_add",
                                                    "var_add", "lookup", "copy"};

// One check in flight (pnp_check_assignment, pnp_check_witness).  Every device
// buffer is a member or a local of check_columns: all of it is released when
// the call returns, whatever way it returns.
struct Check {
    pnp_ctx *const ctx;
    const pnp::ProveOpts opt;
    pnp_check_report *const report;
    pnp::ProveDomain dom;
    hipStream_t s = nullptr;
    std::vector<uint64_t> pi_pos;
    std::vector<Fr> pi_val;
    pnp::DevBuf col[4];  // the padded witness columns, D rows each
    std::chrono::steady_clock::time_point t0;

    Check(pnp_ctx *c, uint64_t n_pi, const uint64_t *pos, const uint64_t *canon, pnp_check_report *r)
        : ctx(c), opt{n_pi, pos, canon, nullptr}, report(r) {}

    void mark(const char *name) {
        PNP_HIP(hipStreamSynchronize(s));
        const auto t1 = std::chrono::steady_clock::now();
        ctx->stages.emplace_back(name, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }

    // the prologue pnp_prove_ex / pnp_prove_assignment run (prove_domain,
    // public_input_map), without a commit key; single GPU
    void begin(const CircuitC *cs, const pnp::Assignment *asg) {
        if (report) {
            memset(report, 0, sizeof *report);
            report->first_row = ~0ULL;
        }
        if (ctx->msm.world > 1) {
            set_error("check: the context is sharded over %d ranks (a multi-rank check is not supported)",
                      ctx->msm.world);
            throw pnp::Error(PNP_E_ARG);
        }
        dom = pnp::prove_domain(ctx, cs, asg, false);
        pnp::public_input_map(opt, dom.n, pi_pos, pi_val);
        tables_wait(ctx);  // (the NTT tables are shared with a background build)
        PNP_HIP(hipSetDevice(ctx->device));
        s = ctx->stream;
        ctx->stages.clear();
        t0 = std::chrono::steady_clock::now();
        for (auto &c : col) c.alloc(32 * dom.n);
    }

    void check_columns(const uint64_t *s_rows, uint64_t s_n, bool copy_over_map, uint32_t copy_checked);
};

// The common part: the witness is in col[] (padded), s_rows are the caller's
// q_lookup rows (the first s_n; nullptr: a zero column).
void Check::check_columns(const uint64_t *s_rows, uint64_t s_n, bool copy_over_map, uint32_t copy_checked) {
    using namespace pnp;
    const ResidentKey &key = ctx->key;
    const uint64_t D = dom.n;
    const uint32_t lg = dom.lg;
    mark("check_inputs");

    // the selector rows: forward transforms of the resident coefficients, of
    // the selectors this key has, into scratch
    DevBuf rows[kKeyRows];
    const uint64_t *const *coeffs = reinterpret_cast<const uint64_t *const *>(&key.dev);
    auto row_values = [&](KeyPoly r) -> const uint64_t * {
        if (!key.has(r)) return nullptr;
        rows[r].alloc(32 * D);
        ntt_run(ctx->ntt, rows[r].u64(), lg, false, false, s, coeffs[kKeyTable[r].coeffs]);
        return rows[r].u64();
    };
    CheckRows r{};
    for (int j = 0; j < 4; j++) r.w[j] = col[j].u64();
    r.q_m = row_values(kQm), r.q_l = row_values(kQl), r.q_r = row_values(kQr), r.q_o = row_values(kQo);
    r.q_4 = row_values(kQ4), r.q_c = row_values(kQc), r.q_hl = row_values(kQhl), r.q_hr = row_values(kQhr);
    r.q_h4 = row_values(kQh4), r.q_arith = row_values(kQarith);
    for (int f = 0; f < 4; f++) r.fam[f] = row_values(KeyPoly(kRange + f));
    // the key's q_lookup rows: the resident wire map keeps them
    const uint64_t *k_rows = key.wm_qlk.p ? key.wm_qlk.u64() : row_values(kQlookup);
    // the public inputs: ascending rows, Montgomery values
    DevBuf pis;
    r.n_pi = (uint32_t)pi_pos.size();
    r.lg = lg;
    if (r.n_pi) {
        // (the values start 16-byte aligned: an even count of words before them)
        const size_t val_off = (pi_pos.size() + 1) & ~size_t(1);
        std::vector<uint64_t> packed(val_off + 4 * pi_pos.size());
        for (size_t k = 0; k < pi_pos.size(); k++) {
            packed[k] = pi_pos[k];
            to_u64_limbs(pi_val[k], &packed[val_off + 4 * k]);
        }
        pis.alloc(8 * packed.size());
        PNP_HIP(hipMemcpyAsync(pis.p, packed.data(), 8 * packed.size(), hipMemcpyHostToDevice, s));
        PNP_HIP(hipStreamSynchronize(s));
        r.pi_pos = pis.u64();
        r.pi_val = pis.u64() + val_off;
    }
    DevBuf recbuf(sizeof(CheckRecord));
    CheckRecord *rec = static_cast<CheckRecord *>(recbuf.p);
    k_check_reset(rec, s);
    mark("check_rows_ntt");

    // the gates: arithmetic + PI on every row; a custom family only when the key has it
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
    ctx->ktimer.end("check_rows", s, e0, 32.0 * (double)D * (arith_cols + fam_cols));
    mark("check_rows");

    // the lookup: nothing to do when neither the caller nor the key selects a row
    if (s_rows || k_rows) {
        const uint64_t *t[4] = {key.dev.table1, key.dev.table2, key.dev.table3, key.dev.table4};
        DevBuf slots(8 * D);
        k_check_table_set(t, lg, slots.u32(), s);
        const uint64_t *w[4] = {r.w[0], r.w[1], r.w[2], r.w[3]};
        k_check_lookup(w, s_rows, s_n, k_rows, t, slots.u32(), lg, rec, s);
        PNP_HIP(hipStreamSynchronize(s));  // (slots is released here)
    }
    mark("check_lookup");

    if (copy_over_map) {
        DevBuf first(4 * key.wm_vars);
        const uint32_t *var = key.wm_var.u32();
        const uint64_t ng = key.wm_gates;
        const uint32_t *dvar[4] = {var, var + ng, var + 2 * ng, var + 3 * ng};
        const uint64_t *w[4] = {r.w[0], r.w[1], r.w[2], r.w[3]};
        k_check_copy(dvar, ng, key.wm_vars, w, lg, first.u32(), rec, s);
        PNP_HIP(hipStreamSynchronize(s));
    }
    mark("check_copy");

    CheckRecord h;
    PNP_HIP(hipMemcpyAsync(&h, rec, sizeof h, hipMemcpyDeviceToHost, s));
    PNP_HIP(hipStreamSynchronize(s));
    ctx->ktimer.collect();
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
    }
    if (report) *report = rep;
    if (rep.violations) {
        set_error("row %llu: %s constraint %u (%llu violations)", (unsigned long long)rep.first_row,
                  kCheckKindName[rep.first_kind], rep.first_index, (unsigned long long)rep.violations);
        throw Error(PNP_E_UNSAT);
    }
}

}  // namespace

extern "C" {

int pnp_check_assignment(pnp_ctx *ctx, const uint64_t *values, uint64_t n_vars, int device_ptrs, uint64_t n_pi,
                         const uint64_t *pi_pos, const uint64_t *pi_canon, pnp_check_report *report) {
    if (!ctx || !values || (n_pi && (!pi_pos || !pi_canon))) return PNP_E_ARG;
    if (device_ptrs && ((uintptr_t)values & 15)) {
        set_error("check assignment: HBM values must be 16-byte aligned");
        return PNP_E_ARG;
    }
    PNP_TRY({
        Check c(ctx, n_pi, pi_pos, pi_canon, report);
        const Assignment a{values, n_vars};
        c.begin(nullptr, &a);
        // the columns through the resident wire map (assignment.hip), as the prover gathers them
        pnp::DevBuf up;
        const uint64_t *vals = values;
        if (!device_ptrs) {
            up.alloc(32 * n_vars);
            h2d_batch(ctx, {{up.p, values, 32 * n_vars}});
            vals = up.u64();
        }
        const uint64_t ng = c.dom.ng;
        const uint32_t *var = ctx->key.wm_var.u32();
        const uint32_t *dvar[4] = {var, var + ng, var + 2 * ng, var + 3 * ng};
        uint64_t *w[4] = {c.col[0].u64(), c.col[1].u64(), c.col[2].u64(), c.col[3].u64()};
        pnp::k_gather_witness(dvar, ng, vals, n_vars, c.dom.lg, w, c.s);
        PNP_HIP(hipStreamSynchronize(c.s));
        up.release();
        // s = k: the key's q_lookup rows, as pnp_prove_assignment; one value a
        // variable: the copy constraints hold by construction
        const uint64_t *k_rows = ctx->key.wm_qlk.p ? ctx->key.wm_qlk.u64() : nullptr;
        c.check_columns(k_rows, c.dom.n, false, 1);
    });
}

int pnp_check_witness(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, uint64_t n_pi, const uint64_t *pi_pos,
                      const uint64_t *pi_canon, pnp_check_report *report) {
    if (!ctx || !cs || (n_pi && (!pi_pos || !pi_canon))) return PNP_E_ARG;
    if (cs->n && (!cs->w_l || !cs->w_r || !cs->w_o || !cs->w_4)) return PNP_E_ARG;
    PNP_TRY({
        Check c(ctx, n_pi, pi_pos, pi_canon, report);
        c.begin(cs, nullptr);
        // the padded columns and the caller's q_lookup rows, staged as pnp_prove_ex stages them
        const uint64_t ng = c.dom.ng, D = c.dom.n;
        const uint64_t *wsrc[4] = {cs->w_l, cs->w_r, cs->w_o, cs->w_4};
        pnp::DevBuf qlk;
        std::vector<H2D> up;
        for (int j = 0; j < 4; j++) {
            uint64_t *dst = c.col[j].u64();
            if (device_ptrs) PNP_HIP(hipMemcpyAsync(dst, wsrc[j], 32 * ng, hipMemcpyDeviceToDevice, c.s));
            else up.push_back({dst, wsrc[j], 32 * ng});
            if (D > ng) PNP_HIP(hipMemsetAsync(dst + 4 * ng, 0, 32 * (D - ng), c.s));
        }
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
    });
}

int pnp_last_stage_times(pnp_ctx *ctx, double *ms, const char **names, int cap) {
    if (!ctx) return 0;
    int k = 0;
    for (auto &st : ctx->stages) {
        if (k < cap) {
            if (ms) ms[k] = st.second;
            if (names) names[k] = st.first.c_str();
        }
        k++;
    }
    return k;
}

}  // extern "C"

// ---------------------------------------------------------------- the witness solver
namespace {

void solve_refuse_sharded(pnp_ctx *ctx, const char *what) {
    if (ctx->msm.world > 1) {
        set_error("%s: the context is sharded over %d ranks (a multi-rank solve is not supported)", what,
                  ctx->msm.world);
        throw pnp::Error(PNP_E_ARG);
    }
}

const pnp::ResidentKey::SolvePlan &solved_plan(pnp_ctx *ctx) {
    const pnp::ResidentKey::SolvePlan &sp = ctx->key.solve;
    if (!sp.loaded || !sp.solution.p) {
        set_error("no solved assignment resident (a plan and pnp_solve_assignment first)");
        throw pnp::Error(PNP_E_NOKEY);
    }
    return sp;
}

// the caller's public inputs, none of them on an output row of the plan
void refuse_pi_on_outputs(const pnp::ResidentKey::SolvePlan &sp, const char *what, uint64_t n_pi,
                          const uint64_t *pi_pos) {
    for (uint64_t k = 0; k < n_pi; k++)
        if (sp.is_output(pi_pos[k])) {
            set_error("%s: row %llu is an output of the plan (its public input is derived, not given)", what,
                      (unsigned long long)pi_pos[k]);
            throw pnp::Error(PNP_E_ARG);
        }
}

// pos / canon: the caller's public inputs and then the derived ones of the resident solution
void solved_pis(pnp_ctx *ctx, const char *what, uint64_t n_pi, const uint64_t *pi_pos, const uint64_t *pi_canon,
                std::vector<uint64_t> &pos, std::vector<uint64_t> &canon) {
    const pnp::ResidentKey::SolvePlan &sp = solved_plan(ctx);
    refuse_pi_on_outputs(sp, what, n_pi, pi_pos);
    pos.assign(pi_pos, pi_pos + n_pi);
    canon.assign(pi_canon, pi_canon + 4 * n_pi);
    pos.insert(pos.end(), sp.out_rows.begin(), sp.out_rows.end());
    canon.insert(canon.end(), sp.out_canon.begin(), sp.out_canon.end());
}

// pnp_load_solve_plan_gates, pnp_load_solve_plan (no gate families) and
// pnp_load_solve_inputs (no outputs either); `what` opens the messages
int load_solve_plan(pnp_ctx *ctx, const char *what, const uint32_t *input_ids, uint64_t n_inputs,
                    const uint64_t *output_rows, uint64_t n_outputs, uint32_t gates, int device_ptrs,
                    pnp_solve_info *info) {
    if (!ctx || (n_inputs && !input_ids) || n_inputs > 0xffffffffULL || (n_outputs && !output_rows) ||
        n_outputs > 0xffffffffULL)
        return PNP_E_ARG;
    if (gates & ~(uint32_t)(PNP_SOLVE_RANGE | PNP_SOLVE_LOGIC)) {
        set_error("%s: gates = 0x%x has a bit that is no gate family (PNP_SOLVE_RANGE | PNP_SOLVE_LOGIC)", what, gates);
        return PNP_E_ARG;
    }
    PNP_TRY({
        using namespace pnp;
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
        solve_refuse_sharded(ctx, what);
        tables_wait(ctx);  // (the NTT tables are shared with a background build)
        PNP_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        key.solve.drop();
        const uint64_t D = key.n, ng = key.wm_gates, n_vars = key.wm_vars;
        const uint32_t lg = log2_exact(D);
        if (ng >= (1ULL << 28)) {  // a bid is 16 row + role in 32 bits
            set_error("%s: %llu gates (a plan covers fewer than 2^28)", what, (unsigned long long)ng);
            throw Error(PNP_E_ARG);
        }

        // the input ids, and every variable's level: 0 for an input
        DevBuf ids(4 * std::max<uint64_t>(n_inputs, 1)), level(4 * n_vars), def(4 * n_vars), small;
        if (n_inputs)
            PNP_HIP(hipMemcpyAsync(ids.p, input_ids, 4 * n_inputs,
                                   device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        uint32_t err[2];
        solve_mark_inputs(ids.u32(), n_inputs, n_vars, level.u32(), err, small, s);
        if (err[0] != 0xffffffffu) {
            set_error("%s: input id %u is not a variable (n_vars = %llu)", what, err[0],
                      (unsigned long long)n_vars);
            throw Error(PNP_E_ARG);
        }
        if (err[1] != 0xffffffffu) {
            set_error("%s: input id %u is listed twice", what, err[1]);
            throw Error(PNP_E_ARG);
        }

        // the selector rows: forward transforms of the resident coefficients (as Check::check_columns)
        DevBuf rows[kKeyRows];
        const uint64_t *const *coeffs = reinterpret_cast<const uint64_t *const *>(&key.dev);
        auto row_values = [&](KeyPoly r) -> const uint64_t * {
            if (!key.has(r)) return nullptr;
            rows[r].alloc(32 * D);
            ntt_run(ctx->ntt, rows[r].u64(), lg, false, false, s, coeffs[kKeyTable[r].coeffs]);
            return rows[r].u64();
        };
        SolveSel sel{};
        sel.q_m = row_values(kQm), sel.q_l = row_values(kQl), sel.q_r = row_values(kQr), sel.q_o = row_values(kQo);
        sel.q_4 = row_values(kQ4), sel.q_c = row_values(kQc), sel.q_hl = row_values(kQhl);
        sel.q_hr = row_values(kQhr), sel.q_h4 = row_values(kQh4), sel.q_arith = row_values(kQarith);
        // (a family's rows: only where its flag is set and the key has the selector)
        if (gates & PNP_SOLVE_RANGE) sel.range = row_values(kRange);
        if (gates & PNP_SOLVE_LOGIC) sel.logic = row_values(kLogic);

        // the output rows: checked on the device, their rows marked for the mask
        DevBuf out_rows, out_bits;
        if (n_outputs) {
            out_rows.alloc(8 * n_outputs);
            out_bits.alloc(4 * ((ng + 31) / 32));
            PNP_HIP(hipMemcpyAsync(out_rows.p, output_rows, 8 * n_outputs,
                                   device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
            uint64_t oerr[3];
            solve_mark_outputs(out_rows.u64(), n_outputs, ng, sel.q_arith, out_bits.u32(), oerr, small, s);
            const char *const why[3] = {"is not a gate", "is listed twice", "has q_arith = 0"};
            for (int k = 0; k < 3; k++)
                if (oerr[k] != ~0ULL) {
                    set_error("%s: output row %llu %s", what, (unsigned long long)oerr[k], why[k]);
                    throw Error(PNP_E_ARG);
                }
        }

        const uint32_t *var = key.wm_var.u32();
        const uint32_t *dvar[4] = {var, var + ng, var + 2 * ng, var + 3 * ng};
        SolveBuild b;
        solve_rounds(dvar, ng, n_vars, sel, out_bits.u32(), level.u32(), def.u32(), b, s);
        pnp_solve_info out;
        memset(&out, 0, sizeof out);
        out.n_inputs = n_inputs;
        out.n_levels = b.widths.size();
        uint64_t n_arith = 0, n_gate = 0;
        for (size_t l = 0; l < b.widths.size(); l++) {
            n_arith += b.widths[l];
            n_gate += b.gate_widths[l];
            out.max_width = std::max<uint64_t>(out.max_width, (uint64_t)b.widths[l] + b.gate_widths[l]);
        }
        out.n_solved = n_arith + n_gate;
        out.n_undetermined = b.n_undetermined;
        out.first_undetermined = b.n_undetermined ? b.first_undetermined : ~0ULL;
        if (b.n_undetermined) {
            if (info) *info = out;
            set_error(gates ? "%s: variable %u is neither an input nor defined by an arithmetic row whose other "
                              "wires are known, nor by a range or logic row whose next row is (%llu such variables)"
                            : "%s: variable %u is neither an input nor defined by an arithmetic row whose other "
                              "wires are known (%llu such variables)",
                      what, b.first_undetermined, (unsigned long long)b.n_undetermined);
            throw Error(PNP_E_ARG);
        }

        ResidentKey::SolvePlan &sp = key.solve;
        sp.buf.alloc(SolveView::bytes(n_arith, out.n_levels, n_inputs, n_outputs, sel.q_m != nullptr));
        sp.view.lay(sp.buf.p, n_arith, out.n_levels, n_inputs, n_outputs, sel.q_m != nullptr);
        if (n_gate) {
            sp.gate_buf.alloc(SolveGateView::bytes(n_gate, out.n_levels));
            sp.gate_view.lay(sp.gate_buf.p, n_gate);
        }
        solve_emit(dvar, ng, n_vars, sel, level.u32(), def.u32(), b, out_rows.u64(), n_outputs, sp.view, sp.gate_view,
                   s);
        if (n_inputs) PNP_HIP(hipMemcpyAsync(sp.view.ids, ids.p, 4 * n_inputs, hipMemcpyDeviceToDevice, s));
        sp.out_rows.resize(n_outputs);
        if (n_outputs) PNP_HIP(hipMemcpyAsync(sp.out_rows.data(), out_rows.p, 8 * n_outputs, hipMemcpyDeviceToHost, s));
        PNP_HIP(hipStreamSynchronize(s));
        // the launches: a level wider than a workgroup (both segments counted) alone, narrower ones in runs
        uint64_t p = 0, g = 0;
        for (uint32_t l = 0; l < b.widths.size(); l++) {
            const uint64_t wa = b.widths[l], wg = b.gate_widths[l];
            const bool wide = wa + wg > 256;
            if (!wide && !sp.runs.empty() && !sp.runs.back().wide) {
                sp.runs.back().l1 = l + 1;
                sp.runs.back().p1 = p + wa;
                sp.runs.back().g1 = g + wg;
            } else {
                sp.runs.push_back({l, l + 1, p, p + wa, g, g + wg, wide});
            }
            p += wa;
            g += wg;
        }
        sp.n_range = b.n_range, sp.n_logic = b.n_logic, sp.n_two = b.n_two;
        sp.n_inputs = n_inputs;
        sp.n_solved = out.n_solved;
        sp.n_levels = out.n_levels;
        sp.loaded = true;
        out.plan_bytes = sp.buf.bytes + sp.gate_buf.bytes;
        if (info) *info = out;
    });
}

}  // namespace

extern "C" {

int pnp_load_solve_inputs(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs, int device_ptrs,
                          pnp_solve_info *info) {
    return load_solve_plan(ctx, "load solve inputs", input_ids, n_inputs, nullptr, 0, 0, device_ptrs, info);
}

int pnp_load_solve_plan(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs, const uint64_t *output_rows,
                        uint64_t n_outputs, int device_ptrs, pnp_solve_info *info) {
    return load_solve_plan(ctx, "load solve plan", input_ids, n_inputs, output_rows, n_outputs, 0, device_ptrs, info);
}

int pnp_load_solve_plan_gates(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs, const uint64_t *output_rows,
                              uint64_t n_outputs, uint32_t gates, int device_ptrs, pnp_solve_info *info) {
    return load_solve_plan(ctx, "load solve plan", input_ids, n_inputs, output_rows, n_outputs, gates, device_ptrs,
                           info);
}

int pnp_solve_gate_entries(pnp_ctx *ctx, uint64_t out[2]) {
    if (!ctx || !out) return PNP_E_ARG;
    PNP_TRY({
        const pnp::ResidentKey::SolvePlan &sp = ctx->key.solve;
        if (!sp.loaded) {
            set_error("no solve plan resident (pnp_load_solve_plan_gates first)");
            throw pnp::Error(PNP_E_NOKEY);
        }
        out[0] = sp.n_range;
        out[1] = sp.n_logic;
    });
}

int pnp_solve_assignment(pnp_ctx *ctx, const uint64_t *inputs, uint64_t n_inputs, int device_ptrs, uint64_t n_pi,
                         const uint64_t *pi_pos, const uint64_t *pi_canon) {
    if (!ctx || (n_inputs && !inputs) || (n_pi && (!pi_pos || !pi_canon))) return PNP_E_ARG;
    if (device_ptrs && ((uintptr_t)inputs & 15)) {
        set_error("solve assignment: HBM inputs must be 16-byte aligned");
        return PNP_E_ARG;
    }
    PNP_TRY({
        using namespace pnp;
        ResidentKey::SolvePlan &sp = ctx->key.solve;
        if (!sp.loaded) {
            set_error("no solve plan resident (pnp_load_solve_inputs or pnp_load_solve_plan first)");
            throw Error(PNP_E_NOKEY);
        }
        if (n_inputs != sp.n_inputs) {
            set_error("solve assignment: %llu inputs, the plan was built for %llu", (unsigned long long)n_inputs,
                      (unsigned long long)sp.n_inputs);
            throw Error(PNP_E_ARG);
        }
        solve_refuse_sharded(ctx, "solve assignment");
        refuse_pi_on_outputs(sp, "solve assignment", n_pi, pi_pos);
        const ProveOpts opt{n_pi, pi_pos, pi_canon, nullptr};
        std::vector<uint64_t> pos;
        std::vector<Fr> val;
        public_input_map(opt, ctx->key.n, pos, val);
        tables_wait(ctx);
        PNP_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        ctx->stages.clear();
        auto t0 = std::chrono::steady_clock::now();
        auto mark = [&](const char *name) {
            PNP_HIP(hipStreamSynchronize(s));
            const auto t1 = std::chrono::steady_clock::now();
            ctx->stages.emplace_back(name, std::chrono::duration<double, std::milli>(t1 - t0).count());
            t0 = t1;
        };

        const uint64_t n_vars = ctx->key.wm_vars;
        if (!sp.solution.p) sp.solution.alloc(32 * n_vars);
        uint64_t *vals = sp.solution.u64();
        // (a slot that is not relevant may name a variable a later level writes: it reads zero)
        PNP_HIP(hipMemsetAsync(vals, 0, 32 * n_vars, s));
        DevBuf up, pis;
        const uint64_t *in = inputs;
        if (n_inputs && !device_ptrs) {
            up.alloc(32 * n_inputs);
            h2d_batch(ctx, {{up.p, inputs, 32 * n_inputs}});
            in = up.u64();
        }
        k_solve_scatter(sp.view.ids, in, n_inputs, vals, s);
        const uint64_t *d_pos = nullptr, *d_val = nullptr;
        if (!pos.empty()) {  // ascending rows, then their Montgomery values 16-byte aligned (as the check)
            const size_t val_off = (pos.size() + 1) & ~size_t(1);
            std::vector<uint64_t> packed(val_off + 4 * pos.size());
            for (size_t k = 0; k < pos.size(); k++) {
                packed[k] = pos[k];
                to_u64_limbs(val[k], &packed[val_off + 4 * k]);
            }
            pis.alloc(8 * packed.size());
            PNP_HIP(hipMemcpyAsync(pis.p, packed.data(), 8 * packed.size(), hipMemcpyHostToDevice, s));
            PNP_HIP(hipStreamSynchronize(s));
            d_pos = pis.u64();
            d_val = pis.u64() + val_off;
        }
        mark("solve_inputs");

        hipEvent_t e0 = nullptr;
        ctx->ktimer.begin("solve_levels", s, e0);
        for (const auto &r : sp.runs) {
            if (r.g1 == r.g0) {  // no gate entries: the arithmetic kernels alone
                k_solve_levels(sp.view, r.l0, r.l1, r.p0, r.p1, r.wide, vals, d_pos, d_val, (uint32_t)pos.size(), s);
            } else if (r.wide) {  // one level, a launch a segment
                if (r.p1 > r.p0)
                    k_solve_levels(sp.view, r.l0, r.l1, r.p0, r.p1, true, vals, d_pos, d_val, (uint32_t)pos.size(), s);
                k_solve_gate_level(sp.gate_view, r.g0, r.g1, vals, s);
            } else {
                k_solve_mixed_levels(sp.view, sp.gate_view, r.l0, r.l1, vals, d_pos, d_val, (uint32_t)pos.size(), s);
            }
        }
        // an entry reads its coefficients and ids, four values, and writes one;
        // a gate entry reads its 16 bytes and one or two values, and writes one
        const double per_entry = 32.0 * (kSolveCoefs - (sp.view.coef[kSolveQm] ? 1 : 2)) + 4 * 6 + 32 * 5;
        const uint64_t n_gate = sp.n_range + sp.n_logic;
        ctx->ktimer.end("solve_levels", s, e0,
                        per_entry * (double)(sp.n_solved - n_gate) + 80.0 * (double)n_gate + 32.0 * (double)sp.n_two);
        mark("solve_levels");
        ctx->ktimer.collect();
        // the outputs: one launch after the last level, and their canonical values to the host
        const uint64_t n_out = sp.out_rows.size();
        sp.out_canon.assign(4 * n_out, 0);
        if (n_out) {
            k_solve_outputs(sp.view, n_out, vals, s);
            PNP_HIP(hipMemcpyAsync(sp.out_canon.data(), sp.view.out.pi, 32 * n_out, hipMemcpyDeviceToHost, s));
            mark("solve_outputs");
        }
        ctx->stages.emplace_back("inputs_h2d_bytes", device_ptrs ? 0.0 : 32.0 * (double)n_inputs);
    });
}

int pnp_assignment_ptr(pnp_ctx *ctx, uint64_t **d_values, uint64_t *n_vars) {
    if (!ctx || !d_values) return PNP_E_ARG;
    PNP_TRY({
        const pnp::ResidentKey::SolvePlan &sp = solved_plan(ctx);
        *d_values = sp.solution.u64();
        if (n_vars) *n_vars = ctx->key.wm_vars;
    });
}

int pnp_assignment_values(pnp_ctx *ctx, const uint32_t *ids, uint64_t k, uint64_t *out) {
    if (!ctx || (k && !out)) return PNP_E_ARG;
    PNP_TRY({
        const pnp::ResidentKey::SolvePlan &sp = solved_plan(ctx);
        const uint64_t n_vars = ctx->key.wm_vars;
        if (k > n_vars && !ids) {
            set_error("assignment values: %llu values of %llu variables", (unsigned long long)k,
                      (unsigned long long)n_vars);
            throw pnp::Error(PNP_E_ARG);
        }
        for (uint64_t j = 0; ids && j < k; j++)
            if (ids[j] >= n_vars) {
                set_error("assignment values: id %u is not a variable (n_vars = %llu)", ids[j],
                          (unsigned long long)n_vars);
                throw pnp::Error(PNP_E_ARG);
            }
        PNP_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        if (!ids) {
            if (k) PNP_HIP(hipMemcpyAsync(out, sp.solution.p, 32 * k, hipMemcpyDeviceToHost, s));
        } else {
            for (uint64_t j = 0; j < k; j++)  // (a handful of values: the root)
                PNP_HIP(hipMemcpyAsync(out + 4 * j, sp.solution.u64() + 4 * (uint64_t)ids[j], 32,
                                       hipMemcpyDeviceToHost, s));
        }
        PNP_HIP(hipStreamSynchronize(s));
    });
}

int pnp_solved_public_inputs(pnp_ctx *ctx, uint64_t *pos, uint64_t *canon, uint64_t cap, uint64_t *n) {
    if (!ctx || !n || (cap && (!pos || !canon))) return PNP_E_ARG;
    PNP_TRY({
        const pnp::ResidentKey::SolvePlan &sp = solved_plan(ctx);
        *n = sp.out_rows.size();
        const uint64_t k = std::min<uint64_t>(cap, *n);
        std::copy_n(sp.out_rows.begin(), k, pos);
        std::copy_n(sp.out_canon.begin(), 4 * k, canon);
    });
}

int pnp_prove_solved(pnp_ctx *ctx, uint64_t n_pi, const uint64_t *pi_pos, const uint64_t *pi_canon, const char *label,
                     ProofC *out) {
    if (!ctx || !out || (n_pi && (!pi_pos || !pi_canon))) return PNP_E_ARG;
    std::vector<uint64_t> pos, canon;
    uint64_t *values = nullptr;
    uint64_t n_vars = 0;
    const int rc = [&]() -> int {
        PNP_TRY({
            solved_pis(ctx, "prove solved", n_pi, pi_pos, pi_canon, pos, canon);
            values = ctx->key.solve.solution.u64();
            n_vars = ctx->key.wm_vars;
        });
    }();
    if (rc != PNP_OK) return rc;
    return pnp_prove_assignment(ctx, values, n_vars, 1, pos.size(), pos.data(), canon.data(), label, out);
}

int pnp_check_solved(pnp_ctx *ctx, uint64_t n_pi, const uint64_t *pi_pos, const uint64_t *pi_canon,
                     pnp_check_report *report) {
    if (!ctx || (n_pi && (!pi_pos || !pi_canon))) return PNP_E_ARG;
    std::vector<uint64_t> pos, canon;
    uint64_t *values = nullptr;
    uint64_t n_vars = 0;
    const int rc = [&]() -> int {
        PNP_TRY({
            solved_pis(ctx, "check solved", n_pi, pi_pos, pi_canon, pos, canon);
            values = ctx->key.solve.solution.u64();
            n_vars = ctx->key.wm_vars;
        });
    }();
    if (rc != PNP_OK) return rc;
    return pnp_check_assignment(ctx, values, n_vars, 1, pos.size(), pos.data(), canon.data(), report);
}

}  // extern "C"
