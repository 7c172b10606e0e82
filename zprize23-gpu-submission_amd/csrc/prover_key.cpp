// prover_key.cpp — the ways a prover key becomes resident (include/pnp_plonk.h):
// pnp_load_prover_key (the caller's 8n arrays re-laid into blocks),
// pnp_load_prover_key_coeffs (the blocks derived from the coefficients),
// pnp_preprocess (the coefficients from a circuit description first), and the
// wire map on top (pnp_load_wire_map).  What each polynomial of the key is, is
// read from kKeyTable (prover_key.h).
#include <algorithm>
#include <chrono>
#include <string.h>
#include "context.h"
#include "ec.cuh"
#include "protocol.h"

using namespace pnp;

namespace {

bool host_all_zero(const uint64_t *p, uint64_t words) {
    uint64_t acc = 0;
    for (uint64_t i = 0; i < words; i++) acc |= p[i];
    return acc == 0;
}

// ---- steps shared by the loads ----

// Every load starts here: a background build reads the key being replaced, so
// it finishes first; that key is no longer loaded, its wire map goes with it,
// and the derived groups (wires.hip) re-check sigma.  The device copies
// (key.owned) are kept across loads and reused when a field's size is unchanged
// (the v1 symbol reloads every call: no hipMalloc / hipFree of ~20 GiB per call)
void pk_begin_load(pnp_ctx *ctx) {
    tables_wait(ctx);
    PNP_HIP(hipSetDevice(ctx->device));
    ctx->key.loaded = false;
    ctx->key.wire_map_drop();
    ctx->key.gen++;
}

// ProverKeyC field f in HBM: the caller's device array adopted in place, or
// the context's own buffer of `elems` Fr with the upload of the first n_src of
// them from host memory queued (src == nullptr: nothing queued)
uint64_t *pk_field(pnp_ctx *ctx, int f, const uint64_t *src, uint64_t elems, bool adopt, std::vector<H2D> &up,
                   uint64_t n_src) {
    DevBuf &o = ctx->key.owned[f];
    if (adopt) {
        o.release();
        return const_cast<uint64_t *>(src);
    }
    if (o.bytes != elems * 32) o.alloc(elems * 32);
    if (src) up.push_back({o.p, src, n_src * 32});
    return o.u64();
}

// The caller's key in HBM: every field `want` names must be there (device
// arrays adopted, host arrays uploaded together), the context's copy of any
// other field is released
template <class Want>
void pk_fields(pnp_ctx *ctx, const ProverKeyC *pk, ProverKeyC &dev, uint64_t D, int device_ptrs, Want want) {
    uint64_t *const *src = reinterpret_cast<uint64_t *const *>(pk);
    uint64_t **dst = reinterpret_cast<uint64_t **>(&dev);
    std::vector<H2D> up;
    for (int f = 0; f < kPkFields; f++) {
        const KeyField fld = key_field(f);
        dst[f] = nullptr;
        if (!want(f, fld)) {
            ctx->key.owned[f].release();
            continue;
        }
        if (!src[f]) {
            set_error("prover key field %d is null", f);
            throw Error(PNP_E_ARG);
        }
        dst[f] = pk_field(ctx, f, src[f], fld.elems(D), device_ptrs != 0, up, fld.elems(D));
    }
    h2d_batch(ctx, up);
}

// The quotient's 8n arrays are kept in block layout (point 8j + m -> block m,
// index j), only the blocks this rank owns: all 8 on one GPU; 8/world when the
// round-4 pipeline is distributed (pnp_set_exchange_a2a)
void pk_block_range(pnp_ctx *ctx) {
    const int world = ctx->msm.world;
    const bool split = world > 1 && 8 % world == 0 && ctx->msm.alltoall;
    ctx->key.nb = split ? 8 / world : 8;
    ctx->key.mb0 = split ? ctx->msm.rank * ctx->key.nb : 0;
}
// k_quotient29's keys (protocol.h): no custom gate, no lookup selector or
// table, the standard coset (key.present and key.std_coset are set)
bool pk_q29_class(pnp_ctx *ctx, const ProverKeyC &dev, uint64_t D) {
    static const bool q29_on = [] {
        const char *e = getenv("PNP_QUOT29");
        return !e || atoi(e) != 0;
    }();
    const ResidentKey &key = ctx->key;
    bool q29 = q29_on && key.std_coset && key.qlookup_zero() && !key.any_custom();
    const uint64_t *const *f = reinterpret_cast<const uint64_t *const *>(&dev);
    for (int t = kTable1; t <= kTable4 && q29; t++) {
        const uint64_t *tab = f[kKeyTable[t].coeffs];
        q29 = !tab || !k_any_nonzero(tab, 4 * D, ctx->scratch_b, ctx->stream);
    }
    return q29;
}
// the sigma n-domain evaluations (gen_proof.cuh:159-165 recomputes
// NTT.forward(sigma_coeffs) every proof)
void pk_sigma_domain(pnp_ctx *ctx, const ProverKeyC &dev, uint64_t D, uint32_t lg) {
    const uint64_t *const *f = reinterpret_cast<const uint64_t *const *>(&dev);
    for (int j = 0; j < 4; j++) {
        DevBuf &sn = ctx->key.sigma_n[j];
        sn.reserve(32 * D);
        PNP_HIP(hipMemcpyAsync(sn.p, f[kKeyTable[kSig0 + j].coeffs], 32 * D, hipMemcpyDeviceToDevice, ctx->stream));
        ntt_run(ctx->ntt, sn.u64(), lg, false, false, ctx->stream);
    }
}
// One walk over the table builds every block array of the key being loaded:
// make(row, d256, d29) fills the row's blocks in the 2^256 form, the 2^261
// form or both (nullptr: not kept in that form).  A slot this key does not
// fill, left by an earlier key, is released afterwards.
template <class Make>
void pk_build_blocks(pnp_ctx *ctx, uint64_t D, bool q29, Make make) {
    ResidentKey &key = ctx->key;
    const size_t bytes = 32 * (size_t)key.nb * D;
    bool filled[kKeyRows] = {}, filled29[kKeyRows] = {};
    auto slot = [&](DevBuf &b) {
        if (b.bytes != bytes) b.alloc(bytes);
        return b.u64();
    };
    for (const KeyRow &r : kKeyTable) {
        if (r.cls == kTable || !key.has(r.id) || (r.id == kL1v && !key.std_coset)) continue;
        filled29[r.id] = q29 && r.in29;
        filled[r.id] = !filled29[r.id] || r.keeps256;
        uint64_t *d256 = filled[r.id] ? slot(key.blk[r.id]) : nullptr;
        uint64_t *d29 = filled29[r.id] ? slot(key.blk29[r.id]) : nullptr;
        make(r, d256, d29);
    }
    for (int r = 0; r < kKeyRows; r++) {
        if (!filled[r]) key.blk[r].release();
        if (!filled29[r]) key.blk29[r].release();
    }
    key.q29 = q29;
}
// the key is resident: what every load leaves behind
void pk_load_done(pnp_ctx *ctx, const ProverKeyC &dev, uint64_t D) {
    ResidentKey &key = ctx->key;
    key.blk_rank = ctx->msm.rank;
    key.blk_world = ctx->msm.world;
    key.pinv.release();
    key.pinv_pos = ~0ULL;
    PNP_HIP(hipStreamSynchronize(ctx->stream));
    key.dev = dev;
    key.n = D;
    key.loaded = true;
    ctx->hbm_checked = false;  // the budget is checked by the next proof (pnp::hbm_budget)
}

// The resident key from its coefficient arrays in HBM (`dev`: the *_coeffs and
// table fields set, NULL = absent), shared by pnp_load_prover_key_coeffs and
// pnp_preprocess: drops all-zero optional selectors, derives every block
// array by the per-proof LDE and the coset constants from closed forms.
void pk_derive_from_coeffs(pnp_ctx *ctx, ProverKeyC &dev, uint64_t D) {
    ResidentKey &key = ctx->key;
    uint64_t **dst = reinterpret_cast<uint64_t **>(&dev);
    // an all-zero optional selector is the zero polynomial too
    for (int f = 0; f < kPkFields; f++) {
        if (!key_field(f).row->optional()) continue;
        if (dst[f] && !k_any_nonzero(dst[f], 4 * D, ctx->scratch_b, ctx->stream)) {
            dst[f] = nullptr;
            key.owned[f].release();
        }
    }
    key.set_present(dev);
    const uint32_t lg = log2_exact(D);
    pk_sigma_domain(ctx, dev, D, lg);
    key.std_coset = true;  // a derived key has the standard coset by construction
    pk_block_range(ctx);
    const bool q29 = pk_q29_class(ctx, dev, D);
    // every block array from its n coefficients, on the context's stream
    // (the tables first: lde_blocks would build them lazily one by one)
    ntt_warm(ctx->ntt, lg, ctx->stream);
    pk_build_blocks(ctx, D, q29, [&](const KeyRow &r, uint64_t *d256, uint64_t *d29) {
        if (r.cls != kCoset) {
            lde_blocks(ctx->ntt, dst[r.coeffs], d29 ? d29 : d256, lg, key.mb0, key.nb, ctx->stream, d29 != nullptr);
        } else if (r.id == kL1v) {
            // the coset constants (the table's last rows: their slots are
            // sized) from their closed forms, straight into the blocks: lin
            // (2^256 form always: the PI term), its 2^261 form for a q29 key,
            // v_h^-1, and D (lin - 1), inverted in place into l1v
            k_coset_blocks(lg, key.mb0, key.nb, key.blk[kLin].u64(), q29 ? key.blk29[kLin].u64() : nullptr,
                           key.blk[kVhInv].u64(), d256, ctx->stream);
            k_batch_inverse(d256, (uint64_t)key.nb * D, ctx->scratch_a, ctx->stream);
        }
    });
    // the natural-order scratch of an earlier full load is not needed again
    PNP_HIP(hipStreamSynchronize(ctx->stream));
    for (auto &b : key.tmp) b.release();
    pk_load_done(ctx, dev, D);
}

bool bad_variable(uint64_t slot, uint64_t n_vars) {
    if (slot == ~0ULL) return false;
    set_error("variable id >= n_vars (%llu) in wire %d of row %llu", (unsigned long long)n_vars, (int)(slot & 3),
              (unsigned long long)(slot >> 2));
    return true;
}

// the caller's four id columns (host or HBM) as one array the library owns:
// column j at u32 offset j * ng
void wire_map_copy(pnp_ctx *ctx, const uint32_t *const var[4], uint64_t ng, int device_ptrs, DevBuf &out) {
    out.alloc(16 * ng);
    std::vector<H2D> up;
    for (int j = 0; j < 4; j++) {
        uint32_t *d = static_cast<uint32_t *>(out.p) + j * ng;
        if (device_ptrs) PNP_HIP(hipMemcpyAsync(d, var[j], 4 * ng, hipMemcpyDeviceToDevice, ctx->stream));
        else up.push_back({d, var[j], 4 * ng});
    }
    if (!up.empty()) h2d_batch(ctx, up);
}

// `var` (wire_map_copy) becomes the resident wire map of the resident key, and
// the q_lookup row values are derived from the key's coefficients (a forward
// transform; nothing is kept for the zero polynomial)
void wire_map_adopt(pnp_ctx *ctx, DevBuf &var, uint64_t ng, uint64_t n_vars) {
    ResidentKey &key = ctx->key;
    key.wire_map_drop();
    const uint64_t D = key.n;
    if (key.dev.q_lookup_coeffs) {
        key.wm_qlk.alloc(32 * D);
        PNP_HIP(hipMemcpyAsync(key.wm_qlk.p, key.dev.q_lookup_coeffs, 32 * D, hipMemcpyDeviceToDevice, ctx->stream));
        ntt_run(ctx->ntt, key.wm_qlk.u64(), log2_exact(D), false, false, ctx->stream);  // (as pk_sigma_domain)
        PNP_HIP(hipStreamSynchronize(ctx->stream));
    }
    key.wm_var = std::move(var);
    key.wm_gates = ng;
    key.wm_vars = n_vars;
    key.wm_loaded = true;
}

}  // namespace

extern "C" {

int pnp_load_prover_key(pnp_ctx *ctx, const ProverKeyC *pk, uint64_t D, int device_ptrs) {
    if (!ctx || !pk || D == 0 || (D & (D - 1)) || D > (1ULL << 25)) return PNP_E_ARG;
    PNP_TRY({
        pk_begin_load(ctx);
        ResidentKey &key = ctx->key;
        ProverKeyC dev{};
        uint64_t *const *src = reinterpret_cast<uint64_t *const *>(pk);
        uint64_t **dst = reinterpret_cast<uint64_t **>(&dev);
        // non-zero selectors first: they decide which coefficient Vecs exist
        bool sel_nz[kKeyRows] = {};
        for (int f = 0; f < kPkFields; f++) {
            const KeyField fld = key_field(f);
            if (!fld.evals || !fld.row->optional()) continue;
            if (!src[f]) {
                set_error("prover key field %d is null", f);
                throw Error(PNP_E_ARG);
            }
            const uint64_t words = 4 * 8 * D;
            sel_nz[fld.row->id] = device_ptrs ? k_any_nonzero(src[f], words, ctx->scratch_b, ctx->stream)
                                              : !host_all_zero(src[f], words);
        }
        pk_fields(ctx, pk, dev, D, device_ptrs,
                  [&](int, KeyField fld) { return !fld.row->optional() || sel_nz[fld.row->id]; });
        // key-derived constants, computed once per key instead of per proof:
        // which optional selectors are present (the quotient kernel skips
        // known-zero selectors) and the sigma n-domain evaluations
        key.set_present(dev);
        const uint32_t lg = log2_exact(D);
        pk_sigma_domain(ctx, dev, D, lg);
        // coset constants: v_h^-1 (the reference divides by v_h every proof,
        // quotient.cu:369-370); when the key's coset arrays are the standard
        // ones (x_i = 7 w_8n^i, v_h = x^n - 1, as every key built by the
        // reference's preprocessing), the L1 and PI coset evaluations have the
        // closed forms of protocol.h and need no LDE per proof
        const uint64_t N8 = 8 * D;
        auto tmp = [&](int k) -> DevBuf & {  // per-load scratch, kept for the next load
            if (key.tmp[k].bytes != 32 * N8) key.tmp[k].alloc(32 * N8);
            return key.tmp[k];
        };
        DevBuf &vh_inv = tmp(0), &l1v = tmp(1);
        PNP_HIP(hipMemcpyAsync(vh_inv.p, dev.v_h_coset_8n, 32 * N8, hipMemcpyDeviceToDevice, ctx->stream));
        k_batch_inverse(vh_inv.u64(), N8, ctx->scratch_a, ctx->stream);
        {
            DevBuf &vh = tmp(2), &x = tmp(3);
            k_coset_consts(vh.u64(), x.u64(), lg, ctx->stream);
            key.std_coset = !k_any_diff(vh.u64(), dev.v_h_coset_8n, 4 * N8, ctx->scratch_b, ctx->stream) &&
                            !k_any_diff(x.u64(), dev.linear_evaluations, 4 * N8, ctx->scratch_b, ctx->stream);
            if (key.std_coset) {
                k_affine(l1v.u64(), x.u64(), Fr::one(), neg(Fr::one()), N8, ctx->stream);
                k_batch_inverse(l1v.u64(), N8, ctx->scratch_a, ctx->stream);
                Fr nf = Fr::zero();
                nf.v[0] = (uint32_t)D;
                nf.v[1] = (uint32_t)(D >> 32);
                k_affine(l1v.u64(), l1v.u64(), inverse(to_mont(nf)), Fr::zero(), N8, ctx->stream);
            }
            PNP_HIP(hipStreamSynchronize(ctx->stream));
        }
        // the blocks this rank owns
        pk_block_range(ctx);
        // k_quotient29's keys (pk_q29_class): their selector / sigma / lin
        // blocks are kept in the 2^261 form (key.blk29) and, but lin (the PI
        // term), not in the 2^256 form at all
        const bool q29 = pk_q29_class(ctx, dev, D);
        const uint64_t blk_elems = (uint64_t)key.nb * D;
        pk_build_blocks(ctx, D, q29, [&](const KeyRow &r, uint64_t *d256, uint64_t *d29) {
            const uint64_t *from = r.id == kVhInv ? vh_inv.u64() : r.id == kL1v ? l1v.u64() : dst[r.evals];
            if (d29) {
                to_blocks(from, d29, lg, key.mb0, key.nb, ctx->stream);
                k_to_form29(d29, d29, blk_elems, ctx->stream);  // elementwise, in place
            }
            if (d256) to_blocks(from, d256, lg, key.mb0, key.nb, ctx->stream);
        });
        // the coset-constant scratch (4 x 8n Fr) is kept only for callers that
        // load keys from host memory again and again (the v1 symbol); a
        // device-resident key is loaded once (and ranks sharing a GPU need the
        // HBM)
        if (device_ptrs) {
            PNP_HIP(hipStreamSynchronize(ctx->stream));
            for (auto &b : key.tmp) b.release();
        }
        pk_load_done(ctx, dev, D);
    });
}

// The same resident key from the coefficient arrays alone: every 8n array of
// a key built by the reference's preprocessing is coset_fft of a coefficient
// array the struct also carries (preprocess.rs:174-255) or a function of n
// (linear_evaluations, v_h_coset_8n: preprocess.rs:257-264), so the blocks
// pnp_load_prover_key copies out of the caller's arrays are derived here, by
// the per-proof LDE (lde_blocks) and from closed forms (k_coset_blocks), and
// nothing 8n-sized crosses PCIe or stays resident beside the blocks.
int pnp_load_prover_key_coeffs(pnp_ctx *ctx, const ProverKeyC *pk, uint64_t D, int device_ptrs) {
    if (!ctx || !pk || D == 0 || (D & (D - 1)) || D > (1ULL << 25)) return PNP_E_ARG;
    uint64_t *const *src = reinterpret_cast<uint64_t *const *>(pk);
    // the required fields are checked before anything is touched: a refused
    // call leaves the resident key as it was
    for (int f = 0; f < kPkFields; f++) {
        const KeyField fld = key_field(f);
        if (!fld.evals && !fld.row->optional() && !src[f]) {
            set_error("prover key field %d is null", f);
            return PNP_E_ARG;
        }
    }
    PNP_TRY({
        pk_begin_load(ctx);
        ProverKeyC dev{};
        // never read: the evaluations; an optional selector without
        // coefficients is the zero polynomial
        pk_fields(ctx, pk, dev, D, device_ptrs,
                  [&](int f, KeyField fld) { return !fld.evals && (!fld.row->optional() || src[f]); });
        pk_derive_from_coeffs(ctx, dev, D);
    });
}

int pnp_load_wire_map(pnp_ctx *ctx, const uint32_t *const var[4], uint64_t n_gates, uint64_t n_vars,
                      int device_ptrs) {
    if (!ctx || !var || !var[0] || !var[1] || !var[2] || !var[3] || n_gates == 0) return PNP_E_ARG;
    if (!ctx->key.loaded) {
        set_error("load wire map: prover key not loaded");
        return PNP_E_NOKEY;
    }
    if (ctx->msm.world > 1) {
        set_error("load wire map: the context is sharded over %d ranks (multi-rank wire maps are not supported)",
                  ctx->msm.world);
        return PNP_E_ARG;
    }
    const uint64_t D = ctx->key.n;
    if (n_gates > D) {
        set_error("load wire map: %llu gates, the resident key's domain has %llu rows", (unsigned long long)n_gates,
                  (unsigned long long)D);
        return PNP_E_ARG;
    }
    PNP_TRY({
        tables_wait(ctx);  // (the NTT tables are shared with a background build)
        PNP_HIP(hipSetDevice(ctx->device));
        ctx->key.wire_map_drop();  // a refused map leaves none resident
        const uint32_t lg = log2_exact(D);
        DevBuf ids;
        wire_map_copy(ctx, var, n_gates, device_ptrs, ids);
        {
            // the sigmas of this map must be the resident key's (the forward
            // transforms of its sigma coefficients, kept since the key load)
            DevBuf sig[4], next(16 * D), sort, first;
            const uint32_t *base = static_cast<const uint32_t *>(ids.p);
            const uint32_t *dvar[4] = {base, base + n_gates, base + 2 * n_gates, base + 3 * n_gates};
            uint64_t *dsig[4];
            const uint64_t *csig[4], *ksig[4];
            for (int j = 0; j < 4; j++) {
                sig[j].alloc(32 * D);
                csig[j] = dsig[j] = sig[j].u64();
                ksig[j] = ctx->key.sigma_n[j].u64();
            }
            const uint64_t bad = wire_sigma(ctx->ntt, dvar, n_gates, n_vars, lg, static_cast<uint32_t *>(next.p),
                                            dsig, sort, ctx->stream);
            if (bad_variable(bad, n_vars)) throw Error(PNP_E_ARG);
            const uint64_t diff = k_first_diff4(csig, ksig, lg, first, ctx->stream);
            if (diff != ~0ULL) {
                set_error("load wire map: the map's sigma differs from the resident key's in wire %d of row %llu",
                          (int)(diff & 3), (unsigned long long)(diff >> 2));
                throw Error(PNP_E_ARG);
            }
        }  // (the scratch is released here)
        wire_map_adopt(ctx, ids, n_gates, n_vars);
    });
}

// (the operator form of the loaders' permutation kernels: it shares their
// bad-id message, so it lives here; pnp_gather_witness stays in abi.cpp)
int pnp_wire_sigma(pnp_ctx *ctx, const uint32_t *const d_var[4], uint64_t n_gates, uint64_t n_vars, uint32_t lg_n,
                   uint32_t *d_next, uint64_t *const d_sigma[4]) {
    if (!ctx || !d_var || !d_var[0] || !d_var[1] || !d_var[2] || !d_var[3] || n_gates == 0 || lg_n > 25 ||
        n_gates > (1ULL << lg_n))
        return PNP_E_ARG;
    PNP_TRY({
        tables_wait(ctx);  // (the NTT tables are shared with a background build)
        PNP_HIP(hipSetDevice(ctx->device));
        DevBuf next, sort;
        if (!d_next) {
            next.alloc(16ULL << lg_n);
            d_next = static_cast<uint32_t *>(next.p);
        }
        const uint64_t bad = wire_sigma(ctx->ntt, d_var, n_gates, n_vars, lg_n, d_next, d_sigma, sort, ctx->stream);
        if (bad_variable(bad, n_vars)) throw Error(PNP_E_ARG);
    });
}

// Circuit::compile on the device: the padded columns and the sigmas of the
// wire map inverse-transformed into the arrays pnp_load_prover_key_coeffs
// would have been handed, then its derivation (pk_derive_from_coeffs), then
// the verifier key's commitments.
int pnp_preprocess(pnp_ctx *ctx, const pnp_circuit_desc *c, int device_ptrs, pnp_verifier_key *vk) {
    if (!ctx || !c) return PNP_E_ARG;
    const uint64_t ng = c->n_gates, tl = c->lookup_len;
    if (ng == 0 || ng > (1ULL << 25) || tl > (1ULL << 25)) {
        set_error("preprocess: %llu gates, %llu table rows (1 <= gates, domain <= 2^25)", (unsigned long long)ng,
                  (unsigned long long)tl);
        return PNP_E_ARG;
    }
    uint64_t D = 1;
    while (D < std::max(ng, tl)) D <<= 1;
    const uint32_t lg = log2_exact(D);
    // every refusal comes before the resident key is touched
    for (int j = 0; j < 4; j++) {
        if (!c->var[j]) {
            set_error("preprocess: var[%d] is null", j);
            return PNP_E_ARG;
        }
        if (tl && !c->table[j]) {
            set_error("preprocess: table[%d] is null with %llu table rows", j, (unsigned long long)tl);
            return PNP_E_ARG;
        }
    }
    if (ctx->msm.world > 1) {
        set_error("preprocess: the context is sharded over %d ranks (multi-rank preprocessing is not supported)",
                  ctx->msm.world);
        return PNP_E_ARG;
    }
    if (vk && (!ctx->ck_loaded || ctx->ck_points < D)) {
        set_error("preprocess: the verifier key needs a commit key of %llu points (%llu loaded)",
                  (unsigned long long)D, (unsigned long long)(ctx->ck_loaded ? ctx->ck_points : 0));
        return PNP_E_NOKEY;
    }
    PNP_TRY({
        tables_wait(ctx);  // (the NTT tables are shared with a background build)
        PNP_HIP(hipSetDevice(ctx->device));
        using clk = std::chrono::steady_clock;
        double t_up = 0, t_perm = 0, t_intt = 0, t_derive = 0, t_vk = 0, h2d_bytes = 0;
        auto t0 = clk::now();
        auto lap = [&](double &acc) {  // (every stage ends synchronised)
            PNP_HIP(hipStreamSynchronize(ctx->stream));
            const auto t1 = clk::now();
            acc += std::chrono::duration<double, std::milli>(t1 - t0).count();
            t0 = t1;
        };
        // the permutation first, into scratch: a bad id is an argument error
        // (the ids are copied whichever side they come from: the copy becomes
        // the resident wire map of the new key)
        DevBuf sig[4], vars;
        {
            DevBuf next(16 * D), sort;
            wire_map_copy(ctx, c->var, ng, device_ptrs, vars);
            if (!device_ptrs) h2d_bytes += 16.0 * ng;
            const uint32_t *vbase = static_cast<const uint32_t *>(vars.p);
            const uint32_t *dvar[4] = {vbase, vbase + ng, vbase + 2 * ng, vbase + 3 * ng};
            lap(t_up);
            uint64_t *dsig[4];
            for (int j = 0; j < 4; j++) {
                sig[j].alloc(32 * D);
                dsig[j] = sig[j].u64();
            }
            WireSigmaStats st;
            const uint64_t bad = wire_sigma(ctx->ntt, dvar, ng, c->n_vars, lg, static_cast<uint32_t *>(next.p), dsig,
                                            sort, ctx->stream, &st);
            if (bad_variable(bad, c->n_vars)) throw Error(PNP_E_ARG);
            ctx->stages.clear();
            ctx->stages.push_back({"pre_permutation_bytes", st.bytes});
        }  // (the sort scratch and next are released here)
        lap(t_perm);
        // ---- the resident key is replaced from here on, and its wire map with it
        pk_begin_load(ctx);
        ResidentKey &key = ctx->key;
        ProverKeyC dev{};
        uint64_t **dst = reinterpret_cast<uint64_t **>(&dev);
        for (int f = 0; f < kPkFields; f++)
            if (key_field(f).evals) key.owned[f].release();
        // the columns, padded to D in buffers the context owns: zeros, a
        // device column padded as it is copied, a host column uploaded first
        std::vector<H2D> up;
        auto column = [&](int f, const uint64_t *src, uint64_t len, bool first) {
            const bool host = src && len && !device_ptrs;
            dst[f] = pk_field(ctx, f, host ? src : nullptr, D, false, up, len);
            if (!src || !len) PNP_HIP(hipMemsetAsync(dst[f], 0, D * 32, ctx->stream));
            else if (device_ptrs) k_pad_col(dst[f], src, len, D, first, ctx->stream);
            else h2d_bytes += 32.0 * len;
        };
        constexpr int kDescSels = sizeof c->sel / sizeof c->sel[0];
        const KeyRow *sel_row[kDescSels];
        for (int k = 0; k < kDescSels; k++) {
            const KeyRow *r = sel_row[k] = key_row_where(&KeyRow::desc, k);
            // (an absent optional column leaves the field NULL; any other is a column of zeros)
            if (!c->sel[k] && r->optional()) key.owned[r->coeffs].release();
            else column(r->coeffs, c->sel[k], ng, false);
        }
        for (int t = kTable1; t <= kTable4; t++)
            column(kKeyTable[t].coeffs, tl ? c->table[t - kTable1] : nullptr, tl, true);
        if (!device_ptrs) {
            h2d_batch(ctx, up);
            for (int k = 0; k < kDescSels; k++)
                if (c->sel[k]) k_pad_col(dst[sel_row[k]->coeffs], dst[sel_row[k]->coeffs], ng, D, false, ctx->stream);
            for (int t = kTable1; t <= kTable4 && tl; t++)
                k_pad_col(dst[kKeyTable[t].coeffs], dst[kKeyTable[t].coeffs], tl, D, true, ctx->stream);
        }
        for (int j = 0; j < 4; j++) {
            const int f = kKeyTable[kSig0 + j].coeffs;
            key.owned[f] = std::move(sig[j]);
            dst[f] = key.owned[f].u64();
        }
        lap(t_up);
        // row values -> coefficients (the tables stay columns: ProverKeyC.table1..4)
        for (int f = 0; f < kPkFields; f++)
            if (dst[f] && key_field(f).row->cls != kTable) ntt_run(ctx->ntt, dst[f], lg, true, false, ctx->stream);
        lap(t_intt);
        pk_derive_from_coeffs(ctx, dev, D);
        wire_map_adopt(ctx, vars, ng, c->n_vars);
        lap(t_derive);
        if (vk) {
            vk->n = D;
            PNP_HIP(hipMemcpyAsync(vk->g, ctx->ck_dev, 96, hipMemcpyDeviceToHost, ctx->stream));
            const uint64_t *const *res = reinterpret_cast<const uint64_t *const *>(&key.dev);
            DevBuf tabc[4];
            std::vector<const uint64_t *> sc;
            std::vector<CommitmentC *> oc;
            uint64_t one[6];
            to_u64_limbs(Fq::one(), one);
            for (int k = 0; k < PNP_VK_POLYS; k++) {
                // (the tables are kept as padded columns: committed from a transformed copy)
                const KeyRow &r = *key_row_where(&KeyRow::vk, k);
                const uint64_t *p = res[r.coeffs];
                // (a mandatory selector or a table may be all zero too)
                if (p && !k_any_nonzero(p, 4 * D, ctx->scratch_b, ctx->stream)) p = nullptr;
                if (p && r.cls == kTable) {
                    DevBuf &t = tabc[r.id - kTable1];
                    t.alloc(32 * D);
                    PNP_HIP(hipMemcpyAsync(t.p, p, 32 * D, hipMemcpyDeviceToDevice, ctx->stream));
                    ntt_run(ctx->ntt, t.u64(), lg, true, false, ctx->stream);
                    p = t.u64();
                }
                if (!p) {  // the zero polynomial
                    memset(vk->polys[k].x, 0, 48);
                    memcpy(vk->polys[k].y, one, 48);
                    continue;
                }
                sc.push_back(p);
                oc.push_back(&vk->polys[k]);
            }
            for (size_t b = 0; b < sc.size(); b += 8)
                commit_affine_batch(ctx, sc.data() + b, (int)std::min<size_t>(8, sc.size() - b), D, oc.data() + b);
            lap(t_vk);
        }
        ctx->stages.push_back({"pre_upload", t_up});
        ctx->stages.push_back({"pre_permutation", t_perm});
        ctx->stages.push_back({"pre_intt", t_intt});
        ctx->stages.push_back({"pre_derive", t_derive});
        ctx->stages.push_back({"pre_vk", t_vk});
        ctx->stages.push_back({"pre_h2d_bytes", h2d_bytes});
    });
}

}  // extern "C"
