// abi.cpp — the extern "C" boundary (include/pnp_plonk.h): the v2 functions,
// which return PNP_* codes and never exit.  What a context does behind them is
// context.cpp, the proof prover.cpp, the prover-key loads prover_key.cpp; the
// v1 gen_proof, which wraps them in the reference's contract, is v1.cpp; the
// satisfiability check (pnp_check_*) is check_witness.cpp and the witness
// solver (pnp_load_solve_*, pnp_solve_assignment, pnp_assignment_*, the
// pnp_*_solved prologue) solve_witness.cpp.  What stays here of a call is its
// null and argument checks and PNP_TRY around the unit's function.
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
    if (!ctx || !cs || !out || !pis_given(n_pi, pi_pos, pi_canon)) return PNP_E_ARG;
    ProveOpts o{n_pi, pi_pos, pi_canon, label ? label : "Merkle tree"};
    PNP_TRY(prove_impl(ctx, cs, device_ptrs, out, &o));
}

int pnp_prove_assignment(pnp_ctx *ctx, const uint64_t *values, uint64_t n_vars, int device_ptrs, uint64_t n_pi,
                         const uint64_t *pi_pos, const uint64_t *pi_canon, const char *label, ProofC *out) {
    if (!ctx || !values || !out || !pis_given(n_pi, pi_pos, pi_canon)) return PNP_E_ARG;
    if (device_ptrs && !hbm_aligned(values)) {
        set_error("prove assignment: HBM values must be 16-byte aligned");
        return PNP_E_ARG;
    }
    ProveOpts o{n_pi, pi_pos, pi_canon, label ? label : "Merkle tree"};
    Assignment a{values, n_vars};
    PNP_TRY(prove_impl(ctx, nullptr, device_ptrs, out, &o, &a));
}

}  // extern "C"

// ---------------------------------------------------------------- the witness: check and solve
extern "C" {

int pnp_check_assignment(pnp_ctx *ctx, const uint64_t *values, uint64_t n_vars, int device_ptrs, uint64_t n_pi,
                         const uint64_t *pi_pos, const uint64_t *pi_canon, pnp_check_report *report) {
    if (!ctx || !values || !pis_given(n_pi, pi_pos, pi_canon)) return PNP_E_ARG;
    if (device_ptrs && !hbm_aligned(values)) {
        set_error("check assignment: HBM values must be 16-byte aligned");
        return PNP_E_ARG;
    }
    PNP_TRY(check_assignment(ctx, Assignment{values, n_vars}, device_ptrs, ProveOpts{n_pi, pi_pos, pi_canon, nullptr},
                             report));
}

int pnp_check_witness(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, uint64_t n_pi, const uint64_t *pi_pos,
                      const uint64_t *pi_canon, pnp_check_report *report) {
    if (!ctx || !cs || !pis_given(n_pi, pi_pos, pi_canon)) return PNP_E_ARG;
    if (cs->n && (!cs->w_l || !cs->w_r || !cs->w_o || !cs->w_4)) return PNP_E_ARG;
    PNP_TRY(check_witness(ctx, cs, device_ptrs, ProveOpts{n_pi, pi_pos, pi_canon, nullptr}, report));
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

// pnp_load_solve_plan_lookup, pnp_load_solve_plan_ecc (no lookup rule), pnp_load_solve_plan_gates (no ECC families),
// pnp_load_solve_plan (no gate families) and pnp_load_solve_inputs (no outputs
// either); `what` opens the messages
static int load_plan(pnp_ctx *ctx, const char *what, const uint32_t *input_ids, uint64_t n_inputs,
                     const uint64_t *output_rows, uint64_t n_outputs, uint32_t gates, uint32_t ecc, uint32_t lookup,
                     int device_ptrs, pnp_solve_info *info) {
    if (!ctx || (n_inputs && !input_ids) || n_inputs > 0xffffffffULL || (n_outputs && !output_rows) ||
        n_outputs > 0xffffffffULL)
        return PNP_E_ARG;
    if (gates & ~(uint32_t)(PNP_SOLVE_RANGE | PNP_SOLVE_LOGIC)) {
        set_error("%s: gates = 0x%x has a bit that is no gate family (PNP_SOLVE_RANGE | PNP_SOLVE_LOGIC)", what, gates);
        return PNP_E_ARG;
    }
    if (ecc & ~(uint32_t)(PNP_SOLVE_FIXED_ADD | PNP_SOLVE_VAR_ADD)) {
        set_error("%s: ecc = 0x%x has a bit that is no ECC family (PNP_SOLVE_FIXED_ADD | PNP_SOLVE_VAR_ADD)", what, ecc);
        return PNP_E_ARG;
    }
    if (lookup & ~(uint32_t)PNP_SOLVE_LOOKUP) {
        set_error("%s: lookup = 0x%x has a bit that is not the lookup rule (PNP_SOLVE_LOOKUP)", what, lookup);
        return PNP_E_ARG;
    }
    PNP_TRY(load_solve_plan(ctx, what, input_ids, n_inputs, output_rows, n_outputs, gates, ecc, lookup, device_ptrs,
                            info));
}

int pnp_load_solve_inputs(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs, int device_ptrs,
                          pnp_solve_info *info) {
    return load_plan(ctx, "load solve inputs", input_ids, n_inputs, nullptr, 0, 0, 0, 0, device_ptrs, info);
}

int pnp_load_solve_plan(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs, const uint64_t *output_rows,
                        uint64_t n_outputs, int device_ptrs, pnp_solve_info *info) {
    return load_plan(ctx, "load solve plan", input_ids, n_inputs, output_rows, n_outputs, 0, 0, 0, device_ptrs, info);
}

int pnp_load_solve_plan_gates(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs, const uint64_t *output_rows,
                              uint64_t n_outputs, uint32_t gates, int device_ptrs, pnp_solve_info *info) {
    return load_plan(ctx, "load solve plan", input_ids, n_inputs, output_rows, n_outputs, gates, 0, 0, device_ptrs,
                     info);
}

int pnp_load_solve_plan_ecc(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs, const uint64_t *output_rows,
                            uint64_t n_outputs, uint32_t gates, uint32_t ecc, int device_ptrs, pnp_solve_info *info) {
    return load_plan(ctx, "load solve plan", input_ids, n_inputs, output_rows, n_outputs, gates, ecc, 0, device_ptrs,
                     info);
}

int pnp_load_solve_plan_lookup(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs,
                               const uint64_t *output_rows, uint64_t n_outputs, uint32_t gates, uint32_t ecc,
                               uint32_t lookup, int device_ptrs, pnp_solve_info *info) {
    return load_plan(ctx, "load solve plan", input_ids, n_inputs, output_rows, n_outputs, gates, ecc, lookup,
                     device_ptrs, info);
}

int pnp_solve_lookup_entries(pnp_ctx *ctx, uint64_t out[2]) {
    if (!ctx || !out) return PNP_E_ARG;
    PNP_TRY(solve_lookup_entries(ctx, out));
}

int pnp_solve_ecc_entries(pnp_ctx *ctx, uint64_t out[2]) {
    if (!ctx || !out) return PNP_E_ARG;
    PNP_TRY(solve_ecc_entries(ctx, out));
}

int pnp_solve_gate_entries(pnp_ctx *ctx, uint64_t out[2]) {
    if (!ctx || !out) return PNP_E_ARG;
    PNP_TRY(solve_gate_entries(ctx, out));
}

int pnp_solve_assignment(pnp_ctx *ctx, const uint64_t *inputs, uint64_t n_inputs, int device_ptrs, uint64_t n_pi,
                         const uint64_t *pi_pos, const uint64_t *pi_canon) {
    if (!ctx || (n_inputs && !inputs) || !pis_given(n_pi, pi_pos, pi_canon)) return PNP_E_ARG;
    if (device_ptrs && !hbm_aligned(inputs)) {
        set_error("solve assignment: HBM inputs must be 16-byte aligned");
        return PNP_E_ARG;
    }
    PNP_TRY(solve_assignment(ctx, inputs, n_inputs, device_ptrs, ProveOpts{n_pi, pi_pos, pi_canon, nullptr}));
}

int pnp_assignment_ptr(pnp_ctx *ctx, uint64_t **d_values, uint64_t *n_vars) {
    if (!ctx || !d_values) return PNP_E_ARG;
    PNP_TRY(assignment_ptr(ctx, d_values, n_vars));
}

int pnp_assignment_values(pnp_ctx *ctx, const uint32_t *ids, uint64_t k, uint64_t *out) {
    if (!ctx || (k && !out)) return PNP_E_ARG;
    PNP_TRY(assignment_values(ctx, ids, k, out));
}

int pnp_solved_public_inputs(pnp_ctx *ctx, uint64_t *pos, uint64_t *canon, uint64_t cap, uint64_t *n) {
    if (!ctx || !n || (cap && (!pos || !canon))) return PNP_E_ARG;
    PNP_TRY(solved_public_inputs(ctx, pos, canon, cap, n));
}

int pnp_prove_solved(pnp_ctx *ctx, uint64_t n_pi, const uint64_t *pi_pos, const uint64_t *pi_canon, const char *label,
                     ProofC *out) {
    if (!ctx || !out || !pis_given(n_pi, pi_pos, pi_canon)) return PNP_E_ARG;
    SolvedAssignment a;
    const int rc = solved_assignment(ctx, "prove solved", n_pi, pi_pos, pi_canon, a);
    if (rc != PNP_OK) return rc;
    return pnp_prove_assignment(ctx, a.values, a.n_vars, 1, a.pos.size(), a.pos.data(), a.canon.data(), label, out);
}

int pnp_check_solved(pnp_ctx *ctx, uint64_t n_pi, const uint64_t *pi_pos, const uint64_t *pi_canon,
                     pnp_check_report *report) {
    if (!ctx || !pis_given(n_pi, pi_pos, pi_canon)) return PNP_E_ARG;
    SolvedAssignment a;
    const int rc = solved_assignment(ctx, "check solved", n_pi, pi_pos, pi_canon, a);
    if (rc != PNP_OK) return rc;
    return pnp_check_assignment(ctx, a.values, a.n_vars, 1, a.pos.size(), a.pos.data(), a.canon.data(), report);
}

}  // extern "C"
