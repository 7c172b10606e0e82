// v1.cpp — gen_proof(CircuitC, ProverKeyC, CommitKeyC), the drop-in call
// (lib/hello.cu:4-6, plonk-core/src/lib.rs:237-239), over the v2 functions.
// The reference's contract: structs by value, ProofC by value, synchronous,
// device 0, print-and-exit on errors (caffe/common.hpp:23-30).
//
// The reference copies every key array to the device on every call
// (load.cu:311-358, gen_proof.cuh:64-78, 166-180, 280-314: ~22 GiB at
// HEIGHT=15), so a caller may rewrite its key buffers in place between calls.
// This call reads the caller's current keys too, without the upload where it
// can tell that the resident copy (one context per process, struct V1) is the
// same key.  What tells it is the call's key-identity policy (KeyId):
//   content hash (default): every word the key loads read, hashed on the host
//     (pk_content_hash / ck_content_hash);
//   sampled fingerprint (PNP_V1_REUSE=1, for callers that never mutate their
//     keys, like merkle-tree's main.rs and pnp_bench.rs): every field pointer,
//     the domain and 257 evenly spaced words of every array the prover reads;
//   none (PNP_V1_RELOAD=1, the reference's behaviour): nothing is compared,
//     both keys are uploaded.  With REUSE set as well RELOAD decides the
//     loading and the fingerprint is what is remembered.
// The switches are read from the environment on every call.  The expensive
// objects derived from the SRS (the folded MSM tables, the Lagrange basis of
// lagrange.hip) are kept when an uploaded SRS equals the resident one byte for
// byte (compared on the device, pnp_load_commit_key).
// PNP_V1_STRICT=1: reject prover keys outside the reference GPU path's
// envelope (non-zero custom-gate selectors, q_lookup or lookup tables), for
// which this backend returns the ZK-Garage prover's proof while the reference
// GPU path would return a different one.
// PNP_V1_DERIVE=1: see V1KeyLoad.
//
// Call for call, with D the domain (the power of two holding the gates and the
// lookup rows) and "known" meaning that V1 holds the identity of the resident
// copy:
//   the resident prover key was derived (DERIVE) and this call has no DERIVE:
//     the prover key counts as unknown;
//   SRS pointer null: print + exit, PNP_E_ARG;
//   content hash, both keys known and resident at D, no PNP_V1_NO_SPECULATE
//     (speculative_call): the hash runs on hash_threads(1) threads beside
//     pnp_prove on the resident keys.  Equal hashes: that proof is returned
//     (exit if it failed), the stage list is the proof's own.  Otherwise the
//     proof is zeroed and the tail follows with the hashes just computed; a
//     failed hasher makes both keys unknown, and they stay unknown;
//   content hash, both keys need loading (unknown, or not resident at D)
//     (cold_call): the hasher on hash_threads(1 + kStgThreads) threads beside,
//     in order: the SRS load; the table pre-build (world <= 1 and no table for
//     D); the prover-key load (through DERIVE when set); the pre-build's join;
//     the STRICT check; the proof.  Stages: v1_ctx_create, v1_load_prover_key,
//     v1_load_commit_key, v1_prove, [v1_zero_scan, v1_derive_key,
//     [v1_derive_fallback]], the proof's, v1_hash_wait, v1_call (bench.py's
//     process-cold line and tools/cold_call.py read them).  An error exits
//     only after the hasher has joined and the stages are published; the
//     hashes are remembered only if the hasher succeeded;
//   content hash otherwise (one key known, or NO_SPECULATE): both hashes
//     first, on all hash_threads() threads, then the tail;
//   fingerprint: {fingerprint, D} of both keys, then the tail;
//   none: nothing compared, then the tail;
//   the tail (load_changed_keys, then the proof): the prover key is loaded if
//     RELOAD is set, or it is unknown, or its identity differs, or it is not
//     resident at D; STRICT is checked after such a load only; the SRS
//     likewise.  If DERIVE was tried the stages are v1_load_prover_key,
//     v1_zero_scan, v1_derive_key, [v1_derive_fallback], the proof's.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <thread>
#include <stdlib.h>
#include <string.h>
#include "context.h"
#include "protocol.h"

using namespace pnp;

namespace {

using clk = std::chrono::steady_clock;
double ms_since(clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); }

// a thread joined where its scope ends, on every path out of it
struct ScopedThread {
    std::thread t;
    void join() {
        if (t.joinable()) t.join();
    }
    ~ScopedThread() { join(); }
};

// host threads of a key hash: up to 16 of the machine's, or OMP_NUM_THREADS
// (1..64), less the `busy` ones the caller keeps for work beside it; at least 1
unsigned hash_threads(unsigned busy = 0) {
    unsigned T = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (const char *e = getenv("OMP_NUM_THREADS")) T = std::max(1, std::min(atoi(e), 64));
    return T > busy ? T - busy : 1;
}

bool key_tables_zero(pnp_ctx *ctx) {
    const uint64_t *const *f = reinterpret_cast<const uint64_t *const *>(&ctx->key.dev);
    for (const KeyRow &r : kKeyTable)
        if (r.cls == kTable && f[r.coeffs] &&
            pnp::k_any_nonzero(f[r.coeffs], 4 * ctx->key.n, ctx->scratch_b, ctx->stream))
            return false;
    return true;
}
uint64_t mix64(uint64_t h, uint64_t v) {
    h ^= v + 0x9e3779b97f4a7c15ULL + (h << 6) + (h >> 2);
    return h * 0xff51afd7ed558ccdULL;
}
uint64_t sample_words(uint64_t h, const uint64_t *p, uint64_t words) {
    const uint64_t K = 256;
    for (uint64_t k = 0; k <= K; k++) h = mix64(h, p[(words - 1) * k / K]);
    return h;
}
uint64_t pk_fingerprint(const ProverKeyC &pk, uint64_t D) {
    uint64_t *const *f = reinterpret_cast<uint64_t *const *>(&pk);
    uint64_t h = mix64(0x1234567ULL, D);
    for (int i = 0; i < kPkFields; i++) {
        h = mix64(h, reinterpret_cast<uintptr_t>(f[i]));
        const KeyField fld = key_field(i);
        // selector coefficients may be empty Vecs: pointer only (their
        // evaluations, sampled, decide whether they are read)
        if ((fld.row->optional() && !fld.evals) || !f[i]) continue;
        h = sample_words(h, f[i], 4 * fld.elems(D));
    }
    return h;
}
// Full-content key hash (the v1 default): every word of every array the key
// load reads, hashed on the host by up to 16 threads (memory-bound: ~17 GiB at
// HEIGHT=15 in ~0.1-0.2 s, against ~0.55 s to upload it over PCIe), so an
// unchanged key is not uploaded again while any change — in any word — is.
// Per 8 MiB chunk a 4-lane multiply-fold hash (two 64-bit digests of the four
// lane states) and the OR of its words (a selector's all-zero test), chunks
// combined in order.
struct Seg {
    const uint64_t *p;
    uint64_t words;
};
struct SegHash {
    uint64_t h0 = 0, h1 = 0;
    bool nz = false;
};
inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t mum(uint64_t a, uint64_t b) {  // 64 x 64 -> 128, folded (wyhash's mixer)
    const unsigned __int128 t = (unsigned __int128)a * b;
    return (uint64_t)t ^ (uint64_t)(t >> 64);
}
void hash_chunk(const uint64_t *p, uint64_t w, uint64_t seed, uint64_t out[3]) {
    // 4 independent lanes, one 128-bit product per word: ~1 word per cycle,
    // faster than host memory
    const uint64_t K[4] = {0xa0761d6478bd642fULL, 0xe7037ed1a0b428dbULL, 0x8ebc6af09c88c6e3ULL,
                           0x589965cc75374cc3ULL};
    uint64_t a[4] = {seed ^ K[0], seed ^ K[1], seed ^ K[2], seed ^ K[3]};
    uint64_t o = 0, i = 0;
    for (; i + 4 <= w; i += 4) {
        for (int k = 0; k < 4; k++) {
            const uint64_t v = p[i + k];
            o |= v;
            a[k] = mum(v ^ a[k], K[k]) ^ v;
        }
    }
    for (; i < w; i++) {
        o |= p[i];
        a[0] = mum(p[i] ^ a[0], K[0]) ^ p[i];
    }
    out[0] = mix64(mix64(mix64(mix64(w, a[0]), a[1]), a[2]), a[3]);
    out[1] = mum(a[0] ^ K[2], a[1] ^ K[3]) ^ mum(a[2] ^ K[0], a[3] ^ K[1]) ^ w;
    out[2] = o;
}
std::vector<SegHash> hash_segments(const std::vector<Seg> &segs, unsigned cap = 0) {
    const uint64_t CH = 1 << 20;  // words per chunk (8 MiB)
    struct Job {
        int seg;
        uint64_t off, w;
    };
    std::vector<Job> jobs;
    for (int k = 0; k < (int)segs.size(); k++)
        for (uint64_t o = 0; o < segs[k].words; o += CH) jobs.push_back({k, o, std::min(CH, segs[k].words - o)});
    std::vector<uint64_t> res(jobs.size() * 3);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t j; (j = next.fetch_add(1)) < jobs.size();)
            hash_chunk(segs[jobs[j].seg].p + jobs[j].off, jobs[j].w, jobs[j].off, &res[3 * j]);
    };
    unsigned T = hash_threads();
    if (cap) T = std::min(T, cap);
    T = (unsigned)std::min<size_t>(T, std::max<size_t>(1, jobs.size()));
    std::vector<std::thread> th;
    try {
        for (unsigned t = 1; t < T; t++) th.emplace_back(work);
    } catch (...) {  // a thread that could not start: the started ones finish the jobs
    }
    work();
    for (auto &t : th) t.join();
    std::vector<SegHash> out(segs.size());
    for (size_t j = 0; j < jobs.size(); j++) {
        SegHash &h = out[jobs[j].seg];
        h.h0 = mix64(h.h0, res[3 * j]);
        h.h1 = mix64(h.h1, res[3 * j + 1]);
        h.nz |= res[3 * j + 2] != 0;
    }
    return out;
}
// the prover key as pnp_load_prover_key reads it at domain D: the fields it
// copies, the selector evaluations it tests, and a selector's coefficients
// only when its evaluations are non-zero (an all-zero selector's coefficient
// Vec is empty, lib.rs:157-223)
std::array<uint64_t, 2> pk_content_hash(const ProverKeyC &pk, uint64_t D, unsigned cap = 0) {
    uint64_t *const *f = reinterpret_cast<uint64_t *const *>(&pk);
    std::vector<Seg> segs;
    std::vector<int> field;
    for (int i = 0; i < kPkFields; i++) {
        const KeyField fld = key_field(i);
        if ((fld.row->optional() && !fld.evals) || !f[i]) continue;
        segs.push_back({f[i], 4 * fld.elems(D)});
        field.push_back(i);
    }
    std::vector<SegHash> h = hash_segments(segs, cap);
    std::vector<Seg> sel;
    for (size_t j = 0; j < segs.size(); j++) {
        const KeyRow &r = *key_field(field[j]).row;  // (an optional row is here with its evaluations)
        if (r.optional() && h[j].nz && f[r.coeffs]) sel.push_back({f[r.coeffs], 4 * D});
    }
    std::vector<SegHash> hs = hash_segments(sel, cap);
    std::array<uint64_t, 2> r = {mix64(0xABCDEFULL, D), mix64(0xFEDCBAULL, D)};
    for (size_t j = 0; j < h.size(); j++) {
        r[0] = mix64(mix64(r[0], field[j]), h[j].h0);
        r[1] = mix64(mix64(r[1], field[j]), h[j].h1);
    }
    for (const SegHash &x : hs) r[0] = mix64(r[0], x.h0), r[1] = mix64(r[1], x.h1);
    return r;
}
std::array<uint64_t, 2> ck_content_hash(const CommitKeyC &ck, uint64_t D, unsigned cap = 0) {
    std::vector<SegHash> h = hash_segments({{ck.powers_of_g, 12 * D}}, cap);
    return {mix64(0x13579BULL ^ D, h[0].h0), mix64(0x2468ACULL ^ D, h[0].h1)};
}

uint64_t ck_fingerprint(const CommitKeyC &ck, uint64_t D) {
    uint64_t h = mix64(mix64(0x7654321ULL, D), reinterpret_cast<uintptr_t>(ck.powers_of_g));
    return ck.powers_of_g ? sample_words(h, ck.powers_of_g, 12 * D) : h;
}

// PNP_V1_DERIVE=1 (opt-in, for callers whose prover key is what the
// reference's preprocessing produces: every *_evals array the coset FFT of its
// *_coeffs, linear_evaluations and v_h_coset_8n the standard coset's): wherever
// gen_proof decides the prover key must be (re)loaded it is loaded through
// pnp_load_prover_key_coeffs, so the 8n arrays (~17 GiB at HEIGHT=15) are not
// uploaded.  WHETHER the key changed is decided as without the switch (content
// hash, REUSE fingerprint, RELOAD).  A v1 caller cannot say which optional
// selectors exist (their coefficient Vecs are empty, dangling pointers), so
// that is read from the evaluations: a selector is the zero polynomial iff its
// first D evaluations are zero — exact for a consistent key, a non-zero
// polynomial of degree < D has fewer than D roots.  After the derivation the
// Fr elements holding the 257 sampled words (sample_words) of every 8n array
// the full load would have read are compared with the derived blocks; on a
// mismatch the full key is uploaded instead (same proof as the default, no
// error).  An inconsistency in unsampled elements is not seen: that is the
// caller's promise, like PNP_V1_REUSE's.
struct V1KeyLoad {
    bool derive = false;                              // the switch, this call
    bool tried = false, derived = false, fell_back = false;
    double ms_scan = 0, ms_derive = 0, ms_fallback = 0;
};
// the sampled elements of the caller's 8n arrays against the derived blocks
// (gathered on the device from the block layout; the blocks another rank owns
// are skipped); false: some element differs
bool v1_sampled_check(pnp_ctx *ctx, const ProverKeyC &pk, uint64_t D) {
    uint64_t *const *f = reinterpret_cast<uint64_t *const *>(&pk);
    const uint64_t K = 256, words = 4 * 8 * D;
    const uint32_t lg = log2_exact(D);
    std::vector<uint64_t> idx(K + 1);
    for (uint64_t k = 0; k <= K; k++) idx[k] = ((words - 1) * k / K) / 4;  // element of sampled word k
    const uint32_t cnt = (uint32_t)idx.size();
    struct Arr {
        int field;
        int form;  // 0: zero selector, 1: 2^256 form, 2: 2^261 form (x 32), 3: the inverse (v_h)
    };
    std::vector<Arr> arrs;
    std::vector<const uint64_t *> blks;
    for (int i = 0; i < kPkFields; i++) {  // every 8n array, in field order
        const KeyField fld = key_field(i);
        if (!fld.evals) continue;
        if (!f[i]) return false;  // the full load refuses it: let it say so
        const uint64_t *b = ctx->key.blk[fld.row->id].u64(), *b29 = ctx->key.blk29[fld.row->id].u64();
        arrs.push_back({i, fld.row->id == kVhInv ? 3 : b ? 1 : b29 ? 2 : 0});
        blks.push_back(b ? b : b29);
    }
    pnp::DevBuf d_idx(8 * cnt), d_out(32 * (size_t)cnt * arrs.size());
    std::vector<uint64_t> got(4 * (size_t)cnt * arrs.size());
    PNP_HIP(hipMemcpyAsync(d_idx.p, idx.data(), 8 * cnt, hipMemcpyHostToDevice, ctx->stream));
    for (size_t a = 0; a < arrs.size(); a++)
        if (blks[a])
            pnp::k_gather_blocks(blks[a], lg, ctx->key.mb0, ctx->key.nb, d_idx.u64(), cnt, d_out.u64() + 4 * cnt * a,
                                 ctx->stream);
    PNP_HIP(hipMemcpyAsync(got.data(), d_out.p, 8 * got.size(), hipMemcpyDeviceToHost, ctx->stream));
    PNP_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t zero[4] = {0, 0, 0, 0};
    uint64_t one[4];
    to_u64_limbs(Fr::one(), one);
    for (size_t a = 0; a < arrs.size(); a++) {
        const uint64_t *src = f[arrs[a].field];
        for (uint32_t k = 0; k < cnt; k++) {
            const int m = (int)(idx[k] & 7);
            const uint64_t *mine = src + 4 * idx[k], *dev = &got[4 * (cnt * a + k)];
            if (arrs[a].form == 0) {  // the zero polynomial: zero everywhere, whoever owns the block
                if (memcmp(mine, zero, 32)) return false;
                continue;
            }
            if (m < ctx->key.mb0 || m >= ctx->key.mb0 + ctx->key.nb) continue;
            uint64_t want[4];
            if (arrs[a].form == 1) {
                memcpy(want, mine, 32);
            } else if (arrs[a].form == 2) {
                Fr x = from_u64_limbs<FrP>(mine);
                for (int d = 0; d < 5; d++) x = x + x;
                to_u64_limbs(x, want);
            } else {  // v_h times the derived v_h^-1 is one
                to_u64_limbs(from_u64_limbs<FrP>(mine) * from_u64_limbs<FrP>(dev), want);
                dev = one;
            }
            if (memcmp(want, dev, 32)) return false;
        }
    }
    return true;
}
// the prover-key load of gen_proof: the full upload, or with PNP_V1_DERIVE
// the coefficient path with its zero scan, sampled check and fallback
int v1_load_prover_key(pnp_ctx *ctx, const ProverKeyC &pk, uint64_t D, V1KeyLoad &st, unsigned cap = 0) {
    if (!st.derive) return pnp_load_prover_key(ctx, &pk, D, 0);
    st.tried = true;
    uint64_t *const *f = reinterpret_cast<uint64_t *const *>(&pk);
    bool usable = true;
    for (const KeyRow &r : kKeyTable)
        if (r.optional()) usable &= f[r.evals] != nullptr;
    if (usable) {
        // which optional selectors exist: their first D evaluations, scanned on
        // the hash thread pool
        auto t = clk::now();
        std::vector<Seg> segs;
        std::vector<int> coeffs;
        for (const KeyRow &r : kKeyTable)
            if (r.optional()) {
                segs.push_back({f[r.evals], 4 * D});
                coeffs.push_back(r.coeffs);
            }
        const std::vector<SegHash> h = hash_segments(segs, cap);
        ProverKeyC compact = pk;
        uint64_t **c = reinterpret_cast<uint64_t **>(&compact);
        for (size_t k = 0; k < segs.size(); k++)
            if (!h[k].nz) c[coeffs[k]] = nullptr;
        st.ms_scan = ms_since(t);
        t = clk::now();
        bool ok = pnp_load_prover_key_coeffs(ctx, &compact, D, 0) == PNP_OK;
        try {
            ok = ok && v1_sampled_check(ctx, pk, D);
        } catch (const Error &) {
            ok = false;
        }
        st.ms_derive = ms_since(t);
        if (ok) {
            st.derived = true;
            return PNP_OK;
        }
    }
    const auto t = clk::now();
    st.fell_back = true;
    const int rc = pnp_load_prover_key(ctx, &pk, D, 0);
    st.ms_fallback = ms_since(t);
    return rc;
}

// The folded MSM table of a freshly uploaded SRS (what a context's first proof
// builds first: ~0.19 s at 2^22) built on a stream of its own, from a thread of
// its own (msm_build_table synchronises its stream and frees its level
// buffers), while the caller uploads the prover key over PCIe — the v1 cold
// call.  The first proof finds it (commit_table); if it could not be built
// (e.g. out of HBM) the proof builds it as before.  One GPU: the whole table.
std::thread table_prebuild(pnp_ctx *ctx, uint64_t n) {
    return std::thread([ctx, n] {
        hipStream_t s = nullptr;
        try {
            PNP_HIP(hipSetDevice(ctx->device));
            PNP_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            ctx->ck_table_n = 0;
            msm_build_table(ctx->ck_table, ctx->ck_dev, n, ctx->msm.fold_c, s);
            ctx->ck_table_p0 = 0;
            ctx->ck_table_p1 = n;
            ctx->ck_table_n = n;
        } catch (...) {
            ctx->ck_table_n = 0;
        }
        if (s) (void)hipStreamDestroy(s);
    });
}

// what says "the same key as the resident one"
enum class KeyId { Hash, Fingerprint, None };
using Id = std::array<uint64_t, 2>;
struct KeyIds {
    Id pk{}, ck{};
    bool valid = true;  // false: a hasher failed, the keys it leaves loaded stay unknown
};

// what outlives a call: one per process
struct V1 {
    pnp_ctx *ctx = nullptr;  // made by the first call, never destroyed (pnp_v1_context)
    // h_pk / h_ck identify the resident keys: set by the call that loads a key
    // (cold_call, load_changed_keys); cleared by a failed hasher, and for the
    // prover key by gen_proof when a derived key meets a call without DERIVE
    bool have_pk = false, have_ck = false;
    Id h_pk{}, h_ck{};        // hashes or {fingerprint, D}, as the loading call's policy had it
    bool pk_derived = false;  // set by every prover-key load: it went through DERIVE
} g_v1;

// what a call reads once at its top
struct Call {
    KeyId policy;
    bool reload, strict, speculate;  // RELOAD: load both keys whatever the policy finds; STRICT; no NO_SPECULATE
    uint64_t D = 0;
    clk::time_point t0;            // the call's clock
    double ms_ctx = 0, ms_pk = 0;  // the context's creation (first call), the tail's prover-key load
    V1KeyLoad kl;
};
bool env_on(const char *name) {  // read per call: a caller may switch modes
    const char *e = getenv(name);
    return e && atoi(e) != 0;
}
Call read_call() {
    Call c;
    c.reload = env_on("PNP_V1_RELOAD");
    c.policy = env_on("PNP_V1_REUSE") ? KeyId::Fingerprint : c.reload ? KeyId::None : KeyId::Hash;
    c.strict = env_on("PNP_V1_STRICT");
    c.speculate = !env_on("PNP_V1_NO_SPECULATE");
    c.kl.derive = env_on("PNP_V1_DERIVE");
    c.t0 = clk::now();
    return c;
}

[[noreturn]] void die(int rc) {
    fprintf(stderr, "gen_proof: error %d: %s\n", rc, pnp_last_error());
    exit(EXIT_FAILURE);
}

// PNP_V1_STRICT, after a prover-key load: false, with the message set, for a
// key the switch refuses (the caller exits with PNP_E_ENVELOPE)
bool enforce_envelope(pnp_ctx *ctx, bool strict) {
    if (!strict || (!ctx->key.present && key_tables_zero(ctx))) return true;
    set_error("PNP_V1_STRICT: prover key outside the reference GPU path's envelope (custom-gate "
              "selectors, q_m, q_lookup or lookup tables non-zero)");
    return false;
}

// the call's own stages around the proof's in pnp_last_stage_times(
// pnp_v1_context()): head, the DERIVE load's, the proof's, tail
using Stages = std::vector<std::pair<std::string, double>>;
void publish_stages(pnp_ctx *ctx, Stages st, const V1KeyLoad &kl, const Stages &tail = {}) {
    if (kl.tried) {
        st.push_back({"v1_zero_scan", kl.ms_scan});
        st.push_back({"v1_derive_key", kl.ms_derive});
        if (kl.fell_back) st.push_back({"v1_derive_fallback", kl.ms_fallback});
    }
    st.insert(st.end(), ctx->stages.begin(), ctx->stages.end());
    st.insert(st.end(), tail.begin(), tail.end());
    ctx->stages.swap(st);
}

// Both keys hashed on a thread of its own, on at most `cap` threads, beside
// the caller's GPU work.  wait() joins it and says whether pk and ck hold the
// hashes; a scope left any other way joins it too.
struct KeyHasher {
    Id pk{}, ck{};
    bool ok = true;
    ScopedThread th;  // (last: started after, joined before, what it writes)
    KeyHasher(const ProverKeyC &p, const CommitKeyC &c, uint64_t D, unsigned cap) {
        th.t = std::thread([this, &p, &c, D, cap] {
            try {
                pk = pk_content_hash(p, D, cap);
                ck = ck_content_hash(c, D, cap);
            } catch (...) {
                ok = false;
            }
        });
    }
    bool wait() {
        th.join();
        return ok;
    }
};

// Both keys known and resident at D: prove on them while the hash runs on the
// other cores (one fewer than it would take alone: this thread drives the
// proof).  True: the keys are unchanged and `out` is the proof.  False: that
// proof read an old key (or there is no hash); `ids` is what the hasher found.
bool speculative_call(V1 &v, const Call &c, const CircuitC &circuit, const ProverKeyC &pk, const CommitKeyC &ck,
                      KeyIds &ids, ProofC &out) {
    KeyHasher hasher(pk, ck, c.D, hash_threads(1));
    const int rc = pnp_prove(v.ctx, &circuit, 0, &out);
    ids.valid = hasher.wait();
    ids.pk = hasher.pk;
    ids.ck = hasher.ck;
    if (ids.valid && ids.pk == v.h_pk && ids.ck == v.h_ck) {
        if (rc != PNP_OK) die(rc);
        return true;
    }
    memset(&out, 0, sizeof out);
    if (!ids.valid) v.have_pk = v.have_ck = false;
    return false;
}

// Both keys are uploaded whatever their hashes (the reference driver's one
// proof per process, or a new domain): they are hashed for the next call on
// the cores that this thread and the upload's copy threads leave, beside the
// uploads and the proof.  The SRS goes first: its folded table builds on the
// GPU (table_prebuild) while the prover key crosses PCIe.
ProofC cold_call(V1 &v, Call &c, const CircuitC &circuit, const ProverKeyC &pk, const CommitKeyC &ck) {
    pnp_ctx *ctx = v.ctx;
    ProofC out;
    memset(&out, 0, sizeof out);
    const unsigned cap = hash_threads(1 + pnp_ctx::kStgThreads);
    KeyHasher hasher(pk, ck, c.D, cap);
    bool envelope = true;
    double ms_pk = 0, ms_ck = 0, ms_prove = 0;
    auto t = clk::now();
    int rc = pnp_load_commit_key(ctx, &ck, c.D, 0);
    if (rc == PNP_OK) {
        ms_ck = ms_since(t);
        ScopedThread tb;
        if (ctx->msm.world <= 1 && ctx->ck_table_n != c.D) tb.t = table_prebuild(ctx, c.D);
        t = clk::now();
        rc = v1_load_prover_key(ctx, pk, c.D, c.kl, cap);
        tb.join();
        if (rc == PNP_OK) {
            v.pk_derived = c.kl.derived;
            envelope = enforce_envelope(ctx, c.strict);
            ms_pk = ms_since(t);
            t = clk::now();
            if (envelope) rc = pnp_prove(ctx, &circuit, 0, &out);
            ms_prove = ms_since(t);
        }
    }
    const auto t_join = clk::now();
    const bool hashed = hasher.wait();
    publish_stages(ctx,
                   {{"v1_ctx_create", c.ms_ctx}, {"v1_load_prover_key", ms_pk}, {"v1_load_commit_key", ms_ck},
                    {"v1_prove", ms_prove}},
                   c.kl, {{"v1_hash_wait", ms_since(t_join)}, {"v1_call", ms_since(c.t0)}});
    v.have_pk = v.have_ck = false;
    if (rc != PNP_OK) die(rc);
    if (!envelope) die(PNP_E_ENVELOPE);
    if (hashed) {  // (otherwise the next call uploads again)
        v.have_pk = v.have_ck = true;
        v.h_pk = hasher.pk;
        v.h_ck = hasher.ck;
    }
    return out;
}

// the tail of every other call: each key is loaded if this call reloads, or
// the key is unknown, or its identity differs, or it is not resident at D
void load_changed_keys(V1 &v, Call &c, const KeyIds &ids, const ProverKeyC &pk, const CommitKeyC &ck) {
    pnp_ctx *ctx = v.ctx;
    int rc;
    if (c.reload || !v.have_pk || ids.pk != v.h_pk || !ctx->key.loaded || ctx->key.n != c.D) {
        v.have_pk = false;
        const auto t = clk::now();
        if ((rc = v1_load_prover_key(ctx, pk, c.D, c.kl)) != PNP_OK) die(rc);
        c.ms_pk = ms_since(t);
        v.pk_derived = c.kl.derived;
        if (!enforce_envelope(ctx, c.strict)) die(PNP_E_ENVELOPE);
        v.have_pk = ids.valid;
        v.h_pk = ids.pk;
    }
    if (c.reload || !v.have_ck || ids.ck != v.h_ck || !ctx->ck_loaded || ctx->ck_points != c.D) {
        v.have_ck = false;
        if ((rc = pnp_load_commit_key(ctx, &ck, c.D, 0)) != PNP_OK) die(rc);
        v.have_ck = ids.valid;
        v.h_ck = ids.ck;
    }
}

}  // namespace

extern "C" {

pnp_ctx *pnp_v1_context(void) { return g_v1.ctx; }

ProofC gen_proof(CircuitC circuit, ProverKeyC pk, CommitKeyC ck) {
    V1 &v = g_v1;
    Call c = read_call();
    // a resident key that was derived stands for the caller's arrays only
    // under PNP_V1_DERIVE's promise: a call without the switch uploads them
    if (v.pk_derived && !c.kl.derive) v.have_pk = false;
    int rc;
    if (!v.ctx) {
        if ((rc = pnp_ctx_create(0, &v.ctx)) != PNP_OK) die(rc);
        c.ms_ctx = ms_since(c.t0);
    }
    pnp_ctx *ctx = v.ctx;
    const uint64_t bound = circuit.n > circuit.lookup_len ? circuit.n : circuit.lookup_len;
    for (c.D = 1; c.D < bound;) c.D <<= 1;
    if (!ck.powers_of_g) die(PNP_E_ARG);

    ProofC out;
    memset(&out, 0, sizeof out);
    KeyIds ids;
    if (c.policy == KeyId::Fingerprint) {
        ids.pk = {pk_fingerprint(pk, c.D), c.D};
        ids.ck = {ck_fingerprint(ck, c.D), c.D};
    } else if (c.policy == KeyId::Hash) {
        const bool pk_here = v.have_pk && ctx->key.loaded && ctx->key.n == c.D;
        const bool ck_here = v.have_ck && ctx->ck_loaded && ctx->ck_points == c.D;
        if (pk_here && ck_here && c.speculate) {
            if (speculative_call(v, c, circuit, pk, ck, ids, out)) return out;
        } else if (!pk_here && !ck_here) {
            return cold_call(v, c, circuit, pk, ck);
        } else {
            ids.pk = pk_content_hash(pk, c.D);
            ids.ck = ck_content_hash(ck, c.D);
        }
    }
    load_changed_keys(v, c, ids, pk, ck);
    if ((rc = pnp_prove(ctx, &circuit, 0, &out)) != PNP_OK) die(rc);
    if (c.kl.tried) publish_stages(ctx, {{"v1_load_prover_key", c.ms_pk}}, c.kl);
    return out;
}

}  // extern "C"
