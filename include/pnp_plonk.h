/*
 * pnp_plonk.h — C-ABI boundary of the MI355X gen_proof backend.
 *
 * Drop-in replacement for the reference's CUDA library behind the Rust FFI:
 *   Rust declaration   : plonk-core/src/lib.rs:52-239   (repr(C) structs + extern "C" gen_proof)
 *   C implementation   : plonk-core/lib/hello.cu:4-6     (gen_proof -> prove)
 *   C struct mirror    : plonk-core/lib/PLONK/src/structure.cuh:7-329
 * (paths relative to /root/reference/Prize 1B/).
 *
 * Everything in section 1 is layout-identical to lib.rs, so the Rust host
 * links this library instead of libzprize without source changes
 * (see INTEGRATION.md).  Sections 2-4 are additive (v2) entry points: explicit
 * lengths, error codes, resident (HBM) keys and the operator API used by the
 * parity tests.  No torch or HIP types appear in any signature.
 *
 * Field encodings (identical to arkworks 0.3 / the reference):
 *   Fr  : 4 x u64 little-endian limbs, Montgomery form R = 2^256 mod r
 *   Fq  : 6 x u64 little-endian limbs, Montgomery form R = 2^384 mod q
 *   G1 affine point: {Fq x, Fq y} (12 u64), no infinity flag;
 *   the point at infinity is reported as x = 0, y = Fq::one (Montgomery),
 *   as the reference's to_affine (PLONK/src/point.cu:29-47).
 */
#ifndef PNP_PLONK_H
#define PNP_PLONK_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* 1. v1 ABI — byte-for-byte the reference FFI (lib.rs:52-239)         */
/* ------------------------------------------------------------------ */

/* lib.rs:53-59 */
typedef struct {
    uint64_t a_eval[4];
    uint64_t b_eval[4];
    uint64_t c_eval[4];
    uint64_t d_eval[4];
} WireEvaluationsC;

/* lib.rs:61-67 */
typedef struct {
    uint64_t left_sigma_eval[4];
    uint64_t right_sigma_eval[4];
    uint64_t out_sigma_eval[4];
    uint64_t permutation_eval[4];
} PermutationEvaluationsC;

/* lib.rs:69-81 */
typedef struct {
    uint64_t q_arith_eval[4];
    uint64_t q_c_eval[4];
    uint64_t q_l_eval[4];
    uint64_t q_r_eval[4];
    uint64_t q_hl_eval[4];
    uint64_t q_hr_eval[4];
    uint64_t q_h4_eval[4];
    uint64_t a_next_eval[4];
    uint64_t b_next_eval[4];
    uint64_t d_next_eval[4];
} CustomEvaluationsC;

/* lib.rs:101-111 */
typedef struct {
    uint64_t q_lookup_eval[4];
    uint64_t z2_next_eval[4];
    uint64_t h1_eval[4];
    uint64_t h1_next_eval[4];
    uint64_t h2_eval[4];
    uint64_t f_eval[4];
    uint64_t table_eval[4];
    uint64_t table_next_eval[4];
} LookupEvaluationsC;

/* lib.rs:112-118 */
typedef struct {
    WireEvaluationsC wire_evals;
    PermutationEvaluationsC perm_evals;
    LookupEvaluationsC lookup_evals;
    CustomEvaluationsC custom_evals;
} ProofEvaluationsC;

/* lib.rs:231-235 : affine G1, Montgomery Fq limbs */
typedef struct {
    uint64_t x[6];
    uint64_t y[6];
} CommitmentC;

/* lib.rs:120-142 */
typedef struct {
    CommitmentC a_comm;
    CommitmentC b_comm;
    CommitmentC c_comm;
    CommitmentC d_comm;
    CommitmentC z_comm;
    CommitmentC f_comm;
    CommitmentC h_1_comm;
    CommitmentC h_2_comm;
    CommitmentC z_2_comm;
    CommitmentC t_1_comm;
    CommitmentC t_2_comm;
    CommitmentC t_3_comm;
    CommitmentC t_4_comm;
    CommitmentC t_5_comm;
    CommitmentC t_6_comm;
    CommitmentC t_7_comm;
    CommitmentC t_8_comm;
    CommitmentC aw_opening;
    CommitmentC saw_opening;
    ProofEvaluationsC evaluations;
} ProofC;

/* lib.rs:144-155.  n = unpadded gate count; q_lookup/w_* hold n Montgomery Fr;
 * pi holds ONE Fr in canonical (non-Montgomery) form (prover.rs:717-725). */
typedef struct {
    uint64_t n;
    uint64_t lookup_len;
    uint64_t intended_pi_pos;
    uint64_t *q_lookup;
    uint64_t *pi;
    uint64_t *w_l;
    uint64_t *w_r;
    uint64_t *w_o;
    uint64_t *w_4;
} CircuitC;

/* lib.rs:157-223.  With D = next_pow2(max(n, lookup_len)):
 *   *_coeffs, table1..4 : D Montgomery Fr
 *   *_evals, linear_evaluations, v_h_coset_8n : 8*D Montgomery Fr
 * The coeff buffers of q_m, the four custom-gate selectors and q_lookup are
 * empty Rust Vecs for the Merkle circuit and are never read (gen_proof.cuh:277,
 * 319-329), exactly as in the reference. */
typedef struct {
    uint64_t *q_m_coeffs;
    uint64_t *q_m_evals;
    uint64_t *q_l_coeffs;
    uint64_t *q_l_evals;
    uint64_t *q_r_coeffs;
    uint64_t *q_r_evals;
    uint64_t *q_o_coeffs;
    uint64_t *q_o_evals;
    uint64_t *q_4_coeffs;
    uint64_t *q_4_evals;
    uint64_t *q_c_coeffs;
    uint64_t *q_c_evals;
    uint64_t *q_hl_coeffs;
    uint64_t *q_hl_evals;
    uint64_t *q_hr_coeffs;
    uint64_t *q_hr_evals;
    uint64_t *q_h4_coeffs;
    uint64_t *q_h4_evals;
    uint64_t *q_arith_coeffs;
    uint64_t *q_arith_evals;
    uint64_t *range_selector_coeffs;
    uint64_t *range_selector_evals;
    uint64_t *logic_selector_coeffs;
    uint64_t *logic_selector_evals;
    uint64_t *fixed_group_add_selector_coeffs;
    uint64_t *fixed_group_add_selector_evals;
    uint64_t *variable_group_add_selector_coeffs;
    uint64_t *variable_group_add_selector_evals;
    uint64_t *q_lookup_coeffs;
    uint64_t *q_lookup_evals;
    uint64_t *table1;
    uint64_t *table2;
    uint64_t *table3;
    uint64_t *table4;
    uint64_t *left_sigma_coeffs;
    uint64_t *left_sigma_evals;
    uint64_t *right_sigma_coeffs;
    uint64_t *right_sigma_evals;
    uint64_t *out_sigma_coeffs;
    uint64_t *out_sigma_evals;
    uint64_t *fourth_sigma_coeffs;
    uint64_t *fourth_sigma_evals;
    uint64_t *linear_evaluations;
    uint64_t *v_h_coset_8n;
} ProverKeyC;

/* lib.rs:225-229.  powers_of_g: >= D affine points (12 u64 each);
 * powers_of_gamma_g: 2 affine points (unused: hiding is disabled). */
typedef struct {
    const uint64_t *powers_of_g;
    const uint64_t *powers_of_gamma_g;
} CommitKeyC;

/* lib.rs:237-239 / hello.cu:4-6.  Structs by value, ProofC returned by value.
 * Synchronous, device 0.  On any device error it prints and exits, like the
 * reference's CUDA_CHECK (caffe/common.hpp:23-30).  Like the reference
 * (load.cu:311-358) it uploads the prover key and commit key on every call,
 * so a caller may rewrite its key buffers between calls; the folded MSM table
 * of the SRS is kept when the uploaded SRS is byte-identical to the last one.
 * Environment switches (read per call):
 *   PNP_V1_REUSE=1   reuse the keys resident from an earlier call while their
 *                    fingerprint (field pointers, domain, 257 sampled words
 *                    per array) is unchanged: no upload.  Only for callers
 *                    that never mutate key contents in place.
 *   PNP_V1_DERIVE=1  when the prover key has to be (re)loaded (decided as
 *                    without the switch), load it through
 *                    pnp_load_prover_key_coeffs: the 8n arrays are derived on
 *                    the GPU instead of uploaded.  Only for callers whose
 *                    *_evals are the coset FFTs of their *_coeffs and whose
 *                    linear_evaluations / v_h_coset_8n are the standard
 *                    coset's (any key built by the reference's preprocessing).
 *                    Which optional selectors exist is read from their first D
 *                    evaluations; the elements holding the 257 sampled words
 *                    of every 8n array are compared with the derived values
 *                    and a mismatch falls back to the full upload; an
 *                    inconsistency in unsampled elements is not seen.
 *   PNP_V1_STRICT=1  exit with PNP_E_ENVELOPE for keys outside the reference
 *                    GPU path's circuit class (non-zero q_m / custom-gate /
 *                    q_lookup selectors or lookup tables): there this backend
 *                    returns the ZK-Garage prover's proof (combine_split,
 *                    widgets, the true z2 shift), which differs byte for byte
 *                    from the reference GPU path's. */
ProofC gen_proof(CircuitC circuit, ProverKeyC pk, CommitKeyC ck);

/* ------------------------------------------------------------------ */
/* 2. v2 ABI — explicit errors, resident keys (additive)               */
/* ------------------------------------------------------------------ */

#define PNP_OK              0
#define PNP_E_ARG          -1   /* bad argument / size                      */
#define PNP_E_DEVICE       -2   /* HIP runtime error                        */
#define PNP_E_NOKEY        -3   /* prover / commit key not loaded           */
#define PNP_E_ENVELOPE     -4   /* key outside the reference GPU path's circuit class
                                       (v1 with PNP_V1_STRICT=1 only) */
#define PNP_E_NOMEM        -5   /* device allocation failed                 */

typedef struct pnp_ctx pnp_ctx;
/* The context the v1 symbol proves on (created by its first call; NULL
 * before).  Its first proof goes without the optional tables (Lagrange basis,
 * copy groups), which then build in the background (v2 pnp_prove likewise on
 * one GPU; PNP_DEFER_TABLES=0 builds them inside the first proof instead,
 * PNP_DEFER_BG=0 inside the second): pnp_sync(pnp_v1_context()) waits for
 * that build, e.g. before timing a steady state.  Extension, diagnostics. */
pnp_ctx *pnp_v1_context(void);

/* Human-readable message of the last error on this thread. */
const char *pnp_last_error(void);

/* One context per GPU; owns the stream, twiddle tables, scratch and keys. */
int pnp_ctx_create(int device, pnp_ctx **out);
void pnp_ctx_destroy(pnp_ctx *ctx);

/* Copy (or adopt) the prover key into HBM once; it stays resident for every
 * later pnp_prove.  domain_size = D (power of two).  If `device_ptrs` is
 * non-zero the pointers are HBM pointers that the context reads in place
 * (they must outlive the context) instead of copying. */
int pnp_load_prover_key(pnp_ctx *ctx, const ProverKeyC *pk, uint64_t domain_size,
                        int device_ptrs);
int pnp_load_commit_key(pnp_ctx *ctx, const CommitKeyC *ck, uint64_t n_points,
                        int device_ptrs);

/* The same resident key from its coefficient arrays alone.  A key built by the
 * reference's preprocessing defines every 8n array as the coset FFT of a
 * coefficient array of the same struct (preprocess.rs:174-255) or as a
 * function of the domain size (linear_evaluations, v_h_coset_8n:
 * preprocess.rs:257-264); this load derives them on the device, directly in
 * the layout the prover reads, instead of copying 8n-sized arrays: at D = 2^22
 * 2.1 GiB cross PCIe instead of 17.1 GiB, and with host pointers
 * nothing 8n-sized stays resident beside the prover's own blocks.
 * Afterwards the context is in the state pnp_load_prover_key leaves for the
 * full key whose evaluations are consistent with these coefficients; the
 * proofs are the same bytes.
 *   read, D Fr each, must not be NULL (PNP_E_ARG, the field index in
 *   pnp_last_error; the resident key is left as it was): the *_coeffs of q_l,
 *   q_r, q_o, q_4, q_c, q_hl, q_hr, q_h4, q_arith and of the four sigmas,
 *   and table1..4;
 *   optional, the *_coeffs of q_m, range_selector, logic_selector,
 *   fixed_group_add_selector, variable_group_add_selector, q_lookup: NULL is
 *   the zero polynomial, anything else is D coefficients (an all-zero array
 *   is treated exactly like NULL).  The v1 convention for a zero selector, an
 *   empty Vec's dangling non-NULL pointer, cannot be told from an array here:
 *   pass NULL;
 *   never read, may be NULL: every *_evals, linear_evaluations, v_h_coset_8n.
 * device_ptrs as for pnp_load_prover_key (the coefficient and table pointers
 * are adopted in place).  With several ranks (pnp_set_exchange_a2a) only the
 * rank's own coset blocks are derived. */
int pnp_load_prover_key_coeffs(pnp_ctx *ctx, const ProverKeyC *pk, uint64_t domain_size,
                               int device_ptrs);

/* Preprocessing on the GPU: the resident prover key, and the verifier key,
 * from what a composer holds — selector columns, the wire map, lookup tables —
 * instead of StandardComposer::preprocess_shared on the CPU (preprocess.rs:
 * 318-520: 15 selector iFFTs, the copy permutation over a
 * HashMap<Variable, Vec<WireData>> (permutation/mod.rs:101-213), 4 sigma and 4
 * table iFFTs, 23 commitments).
 *   D = next_pow2(max(n_gates, lookup_len)), 1 <= n_gates, D <= 2^25.
 *   var[j][i] : the variable in wire j (0 left, 1 right, 2 out, 3 fourth) of
 *     gate i (Variable is a usize in Rust: narrow to u32), each < n_vars.  The
 *     composer registers a gate's wires in the order L, R, O, 4 and gates in
 *     row order, so the slots of a variable are ordered by (row, wire) and each
 *     maps to the next, the last to the first (compute_sigma_permutations);
 *     rows >= n_gates map to themselves.
 *   sel[k][i] : the selector ROW VALUES (not coefficients), zero-padded to D
 *     here; NULL = a zero column.  An all-zero q_m, custom-gate or q_lookup
 *     column is the zero polynomial whether NULL or not.
 *   table[k]  : lookup_len entries each, padded to D with the first entry
 *     (MultiSet::pad); all zero when lookup_len == 0 (table[] ignored).
 * The columns are padded, inverse-transformed into arrays the context owns,
 * the sigmas built from the wire map on the device, and the 8n arrays derived
 * exactly as by pnp_load_prover_key_coeffs: afterwards the context is in the
 * state that call leaves for the reference's preprocessed key of this circuit
 * (proofs are the same bytes).  With `vk` non-NULL the 23 commitments are
 * computed against the resident commit key (pnp_load_commit_key first).
 * device_ptrs: var / sel / table are HBM pointers (read, not adopted).
 * Synchronous; the sort scratch is released before it returns.
 * Errors, all decided before the resident key is touched (it keeps proving):
 *   PNP_E_ARG    n_gates = 0, D > 2^25, a NULL var[j], a NULL table[j] with
 *                lookup_len > 0, a variable id >= n_vars (wire and row in
 *                pnp_last_error), or a context sharded over several ranks
 *                (pnp_set_msm_shard world > 1: multi-rank preprocessing is not
 *                supported; preprocess on one rank and load the coefficients)
 *   PNP_E_NOKEY  vk wanted without a commit key of >= D points */
#define PNP_VK_POLYS 23
/* layout-identical to the oracle's or_verifier_key: n, g = SRS_0, then q_m q_l q_r q_o q_4 q_c
 * q_hl q_hr q_h4 q_arith range logic fixed_group_add variable_group_add left/right/out/fourth
 * sigma q_lookup table_1..4; the zero polynomial is the header's infinity (x = 0, y = Fq one) */
typedef struct { uint64_t n; uint64_t g[12]; CommitmentC polys[PNP_VK_POLYS]; } pnp_verifier_key;

typedef struct {
    uint64_t n_gates, n_vars, lookup_len;
    const uint32_t *var[4];    /* n_gates each */
    const uint64_t *sel[15];   /* q_m q_l q_r q_o q_4 q_c q_hl q_hr q_h4 q_arith range logic
                                  fixed_group_add variable_group_add q_lookup: n_gates Montgomery Fr
                                  each (row evaluations, NOT coefficients); NULL = zero column */
    const uint64_t *table[4];  /* lookup_len Montgomery Fr each; ignored when lookup_len == 0 */
} pnp_circuit_desc;

/* Until the next proof, pnp_last_stage_times reports this call's stages
 * (pre_upload, pre_permutation, pre_intt, pre_derive, pre_vk; milliseconds) and
 * two counts in the same list: pre_permutation_bytes, what the permutation
 * kernels had to move, and pre_h2d_bytes, what crossed PCIe. */
int pnp_preprocess(pnp_ctx *ctx, const pnp_circuit_desc *c, int device_ptrs, pnp_verifier_key *vk /* may be NULL */);

/* The resident wire map.  pnp_preprocess keeps a device copy of the four id
 * columns it was given (4 n_gates u32) and of n_vars, owned by the context and
 * counted in pnp_hbm_usage out[0], with the row values of q_lookup on the
 * domain (D Montgomery Fr, a forward transform of the resident coefficients;
 * nothing for the zero polynomial): what pnp_prove_assignment needs to build
 * the witness columns itself.  The map is replaced by the next pnp_preprocess
 * and dropped by pnp_load_prover_key / pnp_load_prover_key_coeffs.
 *
 * pnp_load_wire_map gives a key loaded by one of those two its map.  var[j]:
 * n_gates variable ids of wire j (host, or HBM with device_ptrs; copied, not
 * adopted), each < n_vars, n_gates <= the key's domain size D.  The map must
 * be the key's: its sigma columns, built by the permutation kernels of
 * pnp_wire_sigma, must equal the forward transforms of the four resident
 * sigma coefficient arrays.  Synchronous; the scratch (the sort's, next, four
 * columns of D Fr) is released before it returns.
 * Errors (the key keeps proving; after a bad id or a sigma mismatch NO map is
 * resident, an earlier one included):
 *   PNP_E_ARG    a NULL column, n_gates = 0 or > D, a variable id >= n_vars
 *                (wire and row in pnp_last_error), a sigma that differs from
 *                the key's (the first wire and row, in (row, wire) order, in
 *                pnp_last_error), or a context sharded over several ranks
 *                (as pnp_preprocess)
 *   PNP_E_NOKEY  no prover key loaded */
int pnp_load_wire_map(pnp_ctx *ctx, const uint32_t *const var[4], uint64_t n_gates, uint64_t n_vars,
                      int device_ptrs);

/* The commit key straight from arkworks' memory, without the per-proof
 * conversion prove_pnp does today (prover.rs:700-711 rebuilds (x, y) tuples
 * of all 2^24+1 SRS points on every call): `points` = the address of
 * commit_key.powers_of_g (Vec<ark_bls12_381::G1Affine>, ark-ec 0.3
 * GroupAffine: x, y Fp384 = 6 u64 Montgomery limbs each (R = 2^384), an
 * `infinity` bool, padding).  The Rust struct's field order is not fixed by
 * the language, so the caller passes the layout it was compiled with:
 * stride = size_of::<G1Affine>() (104 on x86-64), x_off / y_off / inf_off =
 * offset_of!(G1Affine, x / y / infinity).  Only the first n_points points are
 * read (n_points >= the domain size).  A point flagged infinity is refused
 * (PNP_E_ARG: an SRS [tau^i] G never holds it).  device_ptrs: `points` is
 * an HBM address.  Otherwise as pnp_load_commit_key (an unchanged SRS keeps
 * its folded table). */
typedef struct {
    uint64_t stride, x_off, y_off, inf_off;
} pnp_affine_layout;
int pnp_load_commit_key_strided(pnp_ctx *ctx, const void *points, uint64_t n_points,
                                const pnp_affine_layout *layout, int device_ptrs);

/* Which of the 19 commitments of a ProofC (v1 or v2) are the point at
 * infinity: bit k = the k-th CommitmentC of ProofC in declaration order
 * (a_comm 0, b 1, c 2, d 3, z 4, f 5, h_1 6, h_2 7, z_2 8, t_1 .. t_8
 * 9 .. 16, aw_opening 17, saw_opening 18).  Infinity is encoded (x = 0, y = Fq one in Montgomery
 * form), which no curve point has (x = 0 gives y = +-2).  Replaces the
 * hard-coded flags of merkle-tree/src/main.rs:112-123 (f, h1, h2, t7, t8 =
 * true), wrong for any circuit with lookups or a quotient of degree >= 6n. */
#define PNP_PROOF_COMMITMENTS 19
uint32_t pnp_proof_infinity_mask(const ProofC *p);

/* Prove with the resident keys.  `device_ptrs`: the CircuitC witness pointers
 * (q_lookup, w_*) are HBM pointers; pi is always a host pointer. */
int pnp_prove(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, ProofC *out);

/* pnp_prove with the general public-input set and transcript label of the
 * ZK-Garage prover (Prover::prove_with_preprocessed, prover.rs:171-190: the
 * transcript holds the PublicInputs BTreeMap, pi.rs:16-86), which the v1 ABI
 * cannot carry (CircuitC has one pi / intended_pi_pos, prover.rs:717-725).
 * n_pi pairs (pi_pos[k], pi_canon[4k..4k+4)) — canonical (non-Montgomery)
 * values, host memory, any order; zero values are dropped like
 * PublicInputs::insert; positions must be distinct and < domain size.
 * cs->pi / cs->intended_pi_pos are ignored.  label = NULL is "Merkle tree".
 * With n_pi = 1, a non-zero value and the default label the proof equals
 * pnp_prove's. */
int pnp_prove_ex(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs, uint64_t n_pi,
                 const uint64_t *pi_pos, const uint64_t *pi_canon, const char *label, ProofC *out);

/* Prove from a variable assignment over the resident wire map (pnp_preprocess
 * or pnp_load_wire_map first): the host hands over one value per variable
 * instead of expanding them into four columns through the wire map it gave
 * the library a moment earlier (prover.rs:197-216: four passes of
 * variables[&w_x[i]] over a HashMap) — 32 n_vars bytes per proof, not
 * 5 * 32 * n_gates.  values: n_vars Montgomery Fr indexed by variable id, in
 * host memory (one staged upload) or, with device_ptrs, in HBM (16-byte
 * aligned; read in place).  n_gates and the domain are the ones the map and
 * the key were loaded with; q_lookup is the key's.  Public inputs and label
 * exactly as pnp_prove_ex.  The columns w_j[i] = values[var_j[i]], zero from
 * row n_gates on, are written by one gather launch into the prover's padded
 * witness buffers; from round 1 on the prover is pnp_prove_ex's, and the proof
 * is byte for byte the one pnp_prove_ex returns for those columns and the
 * key's q_lookup rows.  Whether the assignment satisfies the circuit is what
 * pnp_check_assignment (below) tells, row by row; this call does not look (an
 * unsatisfied one proves like unsatisfied columns do).  Single GPU.
 * Afterwards pnp_last_stage_times carries one extra entry, a count:
 * inputs_h2d_bytes = 32 n_vars for host values, 0 for HBM values; the gather
 * is timed as "gather_witness" (pnp_kernel_timing).
 *   PNP_E_NOKEY  no keys, or no wire map resident ("no wire map")
 *   PNP_E_ARG    n_vars differs from the map's; the errors of pnp_prove_ex */
int pnp_prove_assignment(pnp_ctx *ctx, const uint64_t *values, uint64_t n_vars, int device_ptrs,
                         uint64_t n_pi, const uint64_t *pi_pos, const uint64_t *pi_canon,
                         const char *label, ProofC *out);

/* Does a witness satisfy the resident key's circuit?  The row-by-row check of
 * the ZK-Garage composer's check_circuit_satisfied, on the GPU: every
 * constraint is evaluated alone on every row of the domain, not folded with a
 * separation challenge, so a failure names its row and its constraint.  (The
 * prover itself only notices that round 5's identity fails, redoes rounds 4-6
 * on all 8 coset blocks and returns PNP_OK with a proof no verifier accepts.)
 * pnp_check_assignment takes the arguments of pnp_prove_assignment, and
 * pnp_check_witness those of pnp_prove_ex, each without the label and the
 * proof; public inputs exactly as pnp_prove_ex.  Only the prover key is needed
 * (no commit key).  Wires at rows >= n_gates are zero, "next" is row
 * (i + 1) mod D, all D rows are checked.
 *   A custom-gate constraint k of a family is violated at row i when the
 * family's selector row is non-zero and constraint k alone is non-zero
 * (k in the order of the reference's widgets):
 *   ARITH      0: q_arith (q_m ab + q_l a + q_r b + q_o c + q_4 d + q_hl a^5 +
 *                 q_hr b^5 + q_h4 d^5 + q_c) + PI_i != 0
 *   RANGE      0..3: delta(c - 4d), delta(b - 4c), delta(a - 4b), delta(d_next - 4a)
 *   LOGIC      0..4: delta(a'), delta(b'), delta(d'), c - a'b', delta_xor_and,
 *                 with a' = a_next - 4a and so on
 *   FIXED_ADD  0..3: bit consistency, bit q_c - c, the x equation, the y equation
 *   VAR_ADD    0..2: x1 y2 - d_next, the x3 equation, the y3 equation
 *   LOOKUP     with k the key's q_lookup row value, s the caller's (cs->q_lookup,
 *              zero from cs->n on; the assignment form has s = k) and T the
 *              resident table of D rows —  0: s != 0 and (a, b, c, d) is no row
 *              of T, compared exactly on all 4 x 256 bits;  1: s = 0, k != 0 and
 *              (a, b, c, d) differs from T's row 0 (the prover queries T[0]
 *              where s = 0, the quotient asks for the wires where k != 0)
 *   COPY       pnp_check_witness with a wire map resident: slot (row i, wire j)
 *              holds another value than the lowest slot, in (row, wire) order,
 *              of its variable; the index is j.  Without a resident map copy
 *              constraints are NOT checked (copy_checked = 0); an assignment
 *              satisfies them by construction (copy_checked = 1, count 0).
 * Returns PNP_OK (every constraint holds: the report is zero, first_row = ~0)
 * or PNP_E_UNSAT (the report is filled and pnp_last_error names the first
 * violation, e.g. "row 24: fixed_add constraint 2"); the report is the same on
 * every run.  Synchronous, single GPU; every buffer it needs (the selector
 * rows are forward transforms of the resident coefficients) is released
 * before it returns, and no later proof is changed by it.  Afterwards, until
 * the next proof, pnp_last_stage_times reports check_inputs, check_rows_ntt,
 * check_rows, check_lookup, check_copy (ms); the row kernels are timed as
 * "check_rows" (pnp_kernel_timing).
 *   PNP_E_NOKEY  no prover key; pnp_check_assignment: no wire map resident
 *   PNP_E_ARG    as the proving calls (domain, n_vars, public inputs), or a
 *                context sharded over several ranks (as pnp_preprocess)
 *   PNP_E_NOMEM  the scratch does not fit */
#define PNP_E_UNSAT -6   /* the check ran; the witness violates the circuit (report filled) */

enum { PNP_CHECK_ARITH = 0, PNP_CHECK_RANGE, PNP_CHECK_LOGIC, PNP_CHECK_FIXED_ADD,
       PNP_CHECK_VAR_ADD, PNP_CHECK_LOOKUP, PNP_CHECK_COPY, PNP_CHECK_KINDS };

typedef struct {
    uint64_t violations;                 /* sum of by_kind */
    uint64_t by_kind[PNP_CHECK_KINDS];   /* violated (row, constraint) pairs; COPY: slots */
    uint64_t first_row;                  /* ~0 when none */
    uint32_t first_kind, first_index;    /* of the least (row, kind, index), lexicographic */
    uint32_t copy_checked;               /* 1: copy constraints checked, or hold by construction */
    uint32_t reserved;
} pnp_check_report;

int pnp_check_assignment(pnp_ctx *ctx, const uint64_t *values, uint64_t n_vars, int device_ptrs,
                         uint64_t n_pi, const uint64_t *pi_pos, const uint64_t *pi_canon,
                         pnp_check_report *report /* may be NULL */);
int pnp_check_witness(pnp_ctx *ctx, const CircuitC *cs, int device_ptrs,
                      uint64_t n_pi, const uint64_t *pi_pos, const uint64_t *pi_canon,
                      pnp_check_report *report /* may be NULL */);

/* The witness from the circuit's inputs: the library computes the assignment
 * itself, over the resident wire map and the key's selector rows, instead of
 * the composer filling it gate by gate on the CPU (the reference's witness
 * generation: 9-10 s at HEIGHT 15, run twice, circuit.rs:311).  A general
 * arithmetic-gate solver: almost every variable of a composer-built circuit is
 * the one unknown of one arithmetic row whose other wires are known.
 *
 * The plan (pnp_load_solve_inputs), once per circuit and per choice of input
 * variables.  Slots of a row and their selectors: a (q_l, q_hl, q_m),
 * b (q_r, q_hr, q_m), c (q_o), d (q_4, q_h4).  A slot of row i is RELEVANT when
 * q_arith[i] != 0 and any of its selectors is non-zero at row i, and SOLVABLE
 * when its linear selector (q_l, q_r, q_o, q_4) is non-zero and its other
 * selectors are zero.  K_0 = the input variables.  In round t a row is READY
 * when exactly one relevant slot holds a variable u outside K_(t-1) (u in two
 * relevant slots: not ready) and that slot is solvable; among the rows ready
 * for the same u the lowest defines it, the others stay plain constraints;
 * K_t = K_(t-1) + the round's targets; the first round without a ready row
 * ends it.  Rows of the custom gates and the lookup, and rows with
 * q_arith = 0, never define anything: variables only they touch must be
 * inputs.  The defining equation is
 *   u = -(S + PI_i / q_arith_i) / coef,
 * S the arithmetic sum of the row (q_m ab + q_l a + ... + q_c) with u's slot
 * and every slot that is not relevant taken as 0, PI_i the public input at
 * that row (0 without one), coef the linear selector of u's slot.  -1 / coef
 * is folded into the stored coefficients, so a solve inverts nothing and
 * cannot fail.  The plan is stored in level (round) order, within a level by
 * variable id, and is the same on every run; it is built on the device from
 * forward transforms of the resident selector coefficients into scratch that
 * is released before the call returns.
 *   input_ids: n_inputs distinct variable ids (host, or HBM with device_ptrs).
 *   info (may be NULL): n_inputs, n_solved, n_levels (rounds), max_width (the
 *   widest level), n_undetermined / first_undetermined (~0: none), plan_bytes.
 *   PNP_E_NOKEY  no prover key, or no wire map resident
 *   PNP_E_ARG    an id >= n_vars, an id listed twice, or a variable that is
 *                neither an input nor defined by any round (info is filled);
 *                pnp_last_error names the lowest such id.  A sharded context
 *                (as pnp_preprocess).  After PNP_E_ARG no plan is resident.
 * The plan is replaced by the next plan build (this call or
 * pnp_load_solve_plan, below: this call is that one without output rows) and dropped, with
 * the solution, by whatever drops or replaces the wire map.
 *
 * pnp_solve_assignment: inputs[k] = the Montgomery value of input_ids[k], host
 * memory (one staged upload) or HBM (16-byte aligned).  Public inputs as
 * pnp_prove_ex; they matter on defining rows only — a variable whose defining
 * row carries a public input takes its value from it (the Merkle circuit's
 * root variable is defined by the root row, PI = -root, from round 2 on:
 * INTEGRATION.md 4 has the flow).  Writes all n_vars values into a buffer the
 * context owns, rewritten by the next solve and dropped with the plan; a level
 * wider than a workgroup is one launch, a run of narrower levels one launch of
 * one workgroup.  Nothing says whether the inputs satisfy the rows that define
 * nothing: pnp_check_assignment does.  Stage times solve_inputs, solve_levels
 * (ms) and the count inputs_h2d_bytes (pnp_last_stage_times); the level
 * kernels are timed as "solve_levels" (pnp_kernel_timing).
 *   PNP_E_NOKEY  no plan resident          PNP_E_ARG  n_inputs differs from the plan's
 * pnp_assignment_ptr: the solution in HBM (n_vars Montgomery Fr), for
 * pnp_prove_assignment / pnp_check_assignment with device_ptrs = 1.
 * pnp_assignment_values: k values of it to host memory, out[4 j ..] = the value
 * of ids[j] (ids NULL: the first k variables); how a host without HIP reads
 * the Merkle root.  Both: PNP_E_NOKEY before a solve, PNP_E_ARG for an id or k
 * beyond n_vars.
 * pnp_hbm_usage out[0] counts the plan (plan_bytes) and the solution (32 n_vars).
 * All four are synchronous and single GPU. */
typedef struct {
    uint64_t n_inputs, n_solved, n_levels, max_width;
    uint64_t n_undetermined, first_undetermined;   /* first: ~0 when none */
    uint64_t plan_bytes;
} pnp_solve_info;
int pnp_load_solve_inputs(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs, int device_ptrs,
                          pnp_solve_info *info /* may be NULL */);
int pnp_solve_assignment(pnp_ctx *ctx, const uint64_t *inputs, uint64_t n_inputs, int device_ptrs,
                         uint64_t n_pi, const uint64_t *pi_pos, const uint64_t *pi_canon);
int pnp_assignment_ptr(pnp_ctx *ctx, uint64_t **d_values, uint64_t *n_vars);
int pnp_assignment_values(pnp_ctx *ctx, const uint32_t *ids, uint64_t k, uint64_t *out);

/* Public inputs that are outputs of the computation (a tree root, a hash, a
 * commitment opened to the verifier): the library derives them from the solve
 * instead of being told them.  An OUTPUT ROW is a row whose public input is
 * derived.  Two additions to the plan rules above, nothing else changes:
 *   - an output row is never READY: it defines nothing in any round (its mask
 *     byte is zero from the start of the plan build, no sweep looks at it);
 *   - after the last level, for every output row i,  PI_i = -q_arith_i S_i,
 *     S_i the full arithmetic sum of row i over the solved values, every slot
 *     as it stands (a slot that is not relevant only meets zero coefficients).
 * The Merkle circuit's root row, root 1 - 0 + PI = 0, as an output row: the
 * root variable is then defined by the root's assert_equal row from the last
 * hash's output (one more round), and PI = -root comes out of the solve.
 *
 * pnp_load_solve_plan is pnp_load_solve_inputs with output rows; that call is
 * this one with n_outputs = 0 (same info, same plan_bytes, same plan).
 * output_rows: n_outputs distinct row indices, as pi_pos, host memory or HBM
 * with device_ptrs (which speaks for both lists).  They are checked on the
 * device, the lowest offending row named, the same on every run:
 *   PNP_E_ARG  "output row R is not a gate" (R >= n_gates), "output row R is
 *              listed twice", "output row R has q_arith = 0" (its identity
 *              forces PI = 0: nothing can be derived there), in that order;
 *              no plan is resident afterwards.  A variable that only an output
 *              row could have defined is undetermined, reported as above.
 * The plan gains one entry per output row, in listed order after the levels
 * and counted in plan_bytes: the row, its four variable ids, the row's nine
 * selectors q_l q_r q_o q_4 q_hl q_hr q_h4 q_c q_m (q_m only when the key has
 * it) each already multiplied by -q_arith, and 32 bytes for the derived value.
 *
 * pnp_solve_assignment on a plan with outputs: a pi_pos that names an output
 * row is PNP_E_ARG ("row R is an output of the plan"); other public inputs act
 * on defining rows as before.  After the last level one more launch, a lane an
 * output row, writes PI_i in canonical form, and the call copies them to the
 * host.  The stage list gains solve_outputs (ms) after solve_levels, only when
 * the plan has outputs.
 * pnp_solved_public_inputs: the (row, canonical value) pairs of the last solve
 * in listed order; *n = their count, min(cap, *n) pairs are written (pos[k],
 * canon[4 k ..]).  A derived zero is reported as zero (the proving call drops
 * it like any zero public input).  PNP_E_NOKEY before a solve, PNP_E_ARG for
 * n NULL.
 * pnp_prove_solved / pnp_check_solved: pnp_prove_assignment /
 * pnp_check_assignment over the resident solution (pnp_assignment_ptr) with
 * the caller's public inputs followed by the derived ones: the same proof
 * bytes, the same report, the same errors.  A caller's pi_pos on an output row
 * is PNP_E_ARG; PNP_E_NOKEY before a solve. */
int pnp_load_solve_plan(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs,
                        const uint64_t *output_rows, uint64_t n_outputs, int device_ptrs,
                        pnp_solve_info *info /* may be NULL */);
int pnp_solved_public_inputs(pnp_ctx *ctx, uint64_t *pos, uint64_t *canon, uint64_t cap, uint64_t *n);
int pnp_prove_solved(pnp_ctx *ctx, uint64_t n_pi, const uint64_t *pi_pos, const uint64_t *pi_canon,
                     const char *label, ProofC *out);
int pnp_check_solved(pnp_ctx *ctx, uint64_t n_pi, const uint64_t *pi_pos, const uint64_t *pi_canon,
                     pnp_check_report *report /* may be NULL */);

/* Range and logic rows that define: the quads from the accumulators.  Both
 * families are deterministic base-4 decompositions, linked the way the
 * reference's composer links them: every wire of a range row follows from the
 * d wire of the next row, every wire of a logic row from the a and b wires of
 * the next row.  A range_gate(x, 64) or a xor_gate / and_gate over values the
 * circuit computes then needs no input beyond what defines x: range_gate ends
 * with assert_equal(last accumulator, x), an arithmetic row that defines the
 * last accumulator, and the chain unrolls upwards one row a round.  The
 * reference's logic_gate leaves its last accumulators unlinked to its operands
 * (INTEGRATION.md 4): list them as inputs or add the two assert_equal rows.
 *
 * pnp_load_solve_plan_gates is pnp_load_solve_plan with `gates`, the families
 * whose rows may define (PNP_SOLVE_RANGE | PNP_SOLVE_LOGIC); pnp_load_solve_plan
 * is this call with gates = 0: the same plan, info, plan_bytes, errors and
 * solution.  A bit outside the two flags is PNP_E_ARG; a flag for a family
 * whose selector the key does not have is accepted (there are no such rows).
 * The rules join the ones above, in the same rounds; in round t every rule
 * looks at K_(t-1):
 *   RANGE (flag set): row i with range_selector[i] != 0, i + 1 < n_gates, not
 *     an output row, is READY when the variable in slot d of row i + 1 is in
 *     K_(t-1), and then bids for each of its slots a, b, c, d whose variable is
 *     outside K_(t-1).  With V the canonical integer (0 <= V < r) of that
 *     d_next:  a = V >> 2, b = V >> 4, c = V >> 6, d = V >> 8.  A slot whose
 *     variable is known is not redefined: the composer's zero padding and
 *     whatever is listed as input stay plain constraints, for pnp_check_*.
 *   LOGIC (flag set): row i with logic_selector[i] != 0, q_c[i] = 1 (AND) or
 *     -1 (XOR), i + 1 < n_gates, not an output row (a logic row with another
 *     q_c is never ready), is READY when the variables in slots a and b of row
 *     i + 1 are both in K_(t-1).  With A, B their canonical integers and op
 *     the bitwise operation on the full integers it bids for whichever of
 *     these five are outside K_(t-1):  a_i = A >> 2, b_i = B >> 2,
 *     c_i = (A & 3) (B & 3), d_i = (A >> 2) op (B >> 2), and slot d of row
 *     i + 1, d_(i+1) = A op B.  An XOR result is below 2^255 < 2 r and is
 *     reduced with one conditional subtraction of r (the row's constraint then
 *     fails, as it must for operands that were never in range): the solve
 *     still inverts nothing and cannot fail.
 *   TIES: among all bids of a round for one variable the least (row, role)
 *     wins, the role order: the arithmetic slots a..d, range a..d, logic a, b,
 *     c, d, d_next; the row is the row whose rule fires (for d_next: row i, not
 *     i + 1).  This extends "the lowest row defines it" and keeps the plan the
 *     same on every run.  Arithmetic rows behave as above, output rows never
 *     bid, and a variable that nothing reaches is undetermined as above.
 * Fixed-base and curve-addition rows define through pnp_load_solve_plan_ecc,
 * lookup rows (a table search) through pnp_load_solve_plan_lookup, both below.
 * A gate entry is 16 bytes (target, two sources, kind and shift) in arrays of
 * their own beside the arithmetic entries, level order, by variable id within
 * a level, with their own level offsets, all counted in plan_bytes; with
 * gates = 0, or no such row defining anything, nothing is allocated for them.
 * pnp_solve_info counts every entry of every kind in n_solved and max_width;
 * pnp_solve_gate_entries: out[0], out[1] = the resident plan's entries defined
 * by range rows, by logic rows (PNP_E_NOKEY without a plan).  Everything that
 * takes a plan takes this one the same way: pnp_solve_assignment (a level is
 * an arithmetic segment and a gate segment, more than 256 entries in all: its
 * own launches, one a segment; solve_levels times and counts both),
 * pnp_assignment_ptr / _values, pnp_solved_public_inputs, pnp_prove_solved,
 * pnp_check_solved, pnp_hbm_usage, the drop and replace rules, and a sharded
 * context is refused. */
enum { PNP_SOLVE_RANGE = 1, PNP_SOLVE_LOGIC = 2 };
int pnp_load_solve_plan_gates(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs,
                              const uint64_t *output_rows, uint64_t n_outputs, uint32_t gates,
                              int device_ptrs, pnp_solve_info *info /* may be NULL */);
int pnp_solve_gate_entries(pnp_ctx *ctx, uint64_t out[2]);

/* Fixed-base and curve-addition rows that define: points from scalars.  The
 * reference's fixed_base_scalar_mul ends with assert_equal(last accumulated
 * bit, scalar) and point_addition_gate puts its result in the next row, so a
 * circuit that derives a key or opens a commitment needs no accumulator from
 * the host: the scalar chain unrolls upwards one row a round, then the point
 * chain downwards (about 2 + 254 + 255 levels for one 255-row multiplication,
 * shared by every multiplication of the circuit).
 *
 * pnp_load_solve_plan_ecc is pnp_load_solve_plan_gates with `ecc`, the ECC
 * families whose rows may define (PNP_SOLVE_FIXED_ADD | PNP_SOLVE_VAR_ADD);
 * pnp_load_solve_plan_gates is this call with ecc = 0: the same plan, info,
 * plan_bytes, errors, launches and solution.  An ecc bit outside the two flags
 * is PNP_E_ARG (the message names ecc); gates is validated as above; a flag
 * for a family whose selector the key does not have is accepted.
 * The rules join the ones above, in the same rounds; in round t every rule
 * looks at K_(t-1).  A row i of either family takes part only when
 * i + 1 < n_gates and i is not an output row.  "Canonical" is the integer
 * 0 <= V < r; A and D are Jubjub's a = -1 and d.
 *   FIXED_ADD (flag set, fixed_group_add_selector[i] != 0).  Slots: a, b the
 *     point accumulator, c is xy_alpha, d the scalar accumulator; q_l, q_r, q_c
 *     are x_beta, y_beta, xy_beta.  Three independent sub-rules:
 *     scalar: READY when the variable in slot d of row i + 1 is known; bids for
 *       slot d of row i.  With V the canonical d_next, d = (V - s) / 2 on
 *       integers, s = 0 for V even, 1 for V = 1 (mod 4), -1 for V = 3 (mod 4):
 *       the lowest digit of the width-2 NAF the reference's find_wnaf(2)
 *       produces, so unrolled upwards from assert_equal(last accumulated bit,
 *       scalar) it reproduces the reference's scalar_acc exactly.  V + 1 <= r:
 *       no reduction.
 *     xy: READY when slots d of rows i and i + 1 are known; bids for slot c of
 *       row i: c = bit q_c, with bit = d_next - 2 d in the field.
 *     point: READY when slots a, b, d of row i and slot d of row i + 1 are
 *       known; bids for slots a and b of row i + 1.  With x_alpha = q_l bit,
 *       y_alpha = bit^2 (q_r - 1) + 1 and m = (bit q_c) a b D:
 *         a_next = (x_alpha b + y_alpha a) / (1 + m),
 *         b_next = (y_alpha b - A x_alpha a) / (1 - m).
 *       Slot c is not read: its value is what the xy sub-rule would write, so
 *       the point chain does not wait a round for it.
 *   VAR_ADD (flag set, variable_group_add_selector[i] != 0): READY when slots
 *     a, b, c, d of row i are all known; bids for slots d, a, b of row i + 1.
 *     d_next = a d; with t = D d_next (b c):
 *       a_next = (d_next + b c) / (1 + t),  b_next = (b d - A a c) / (1 - t).
 *   Both: a division by zero yields 0 (the device inverse has inv(0) = 0), so
 *     the solve still cannot fail; the row's own constraint then fails in
 *     pnp_check_*, as it must.  A slot whose variable is already known is not
 *     redefined (the composer's constants, inputs, the zero variable): it
 *     stays a plain constraint for pnp_check_*.
 *   TIES: the least (row, role) still wins, the row the row whose rule fires;
 *     the role order goes on after logic's d_next: fixed-add d, c, a_next,
 *     b_next, then var-add a_next, b_next, d_next.  The order of every bid of
 *     the rules above is unchanged, so their plans are too.
 * A scalar whose width-2 NAF has more digits than the multiplication has rows
 * (the reference's composer asserts on it) is solved all the same; the first
 * fixed-add row's constraint 0 then fails in pnp_check_*.
 * The plan: a fixed-add scalar definition is one more kind of the 16-byte gate
 * entry, (A - s) / 2 (its variables count in pnp_solve_ecc_entries, not in
 * pnp_solve_gate_entries).  The xy, point and var-add definitions are ECC
 * entries in arrays of their own, level order, by (row, kind) within a level,
 * with their own level offsets: 128 bytes an entry, read 16 bytes at a time:
 * three targets (~0: not won) and the kind, four sources, and the row's q_l,
 * q_r, q_c (Montgomery; the selector rows are released after the build).  A
 * point or var-add entry inverts once, (1 + m)(1 - m), for both quotients.
 * All of it is counted in plan_bytes; with ecc = 0, or no such row defining
 * anything, nothing is allocated.  A level is an arithmetic, a gate and an ECC
 * segment: more than 256 entries in all, a launch a segment; narrower levels
 * with ECC entries share one workgroup in which the ECC entries have waves of
 * their own.
 * pnp_solve_info counts every defined variable of every kind in n_solved and
 * max_width.  pnp_solve_gate_entries keeps counting range and logic only;
 * pnp_solve_ecc_entries: out[0], out[1] = the variables fixed-add rows, var-add
 * rows define in the resident plan (PNP_E_NOKEY without a plan).  Everything
 * that takes a plan takes this one the same way, as listed above; the stage
 * list is unchanged and solve_levels times every kind of entry. */
enum { PNP_SOLVE_FIXED_ADD = 1, PNP_SOLVE_VAR_ADD = 2 };
int pnp_load_solve_plan_ecc(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs,
                            const uint64_t *output_rows, uint64_t n_outputs, uint32_t gates,
                            uint32_t ecc, int device_ptrs, pnp_solve_info *info /* may be NULL */);
int pnp_solve_ecc_entries(pnp_ctx *ctx, uint64_t out[2]);

/* Lookup rows that define: the output wire from a table search.  The
 * reference's caller computes c = LookupTable::lookup(a, b, d), the first table
 * row whose columns 0, 1 and 3 equal (a, b, d), and then calls
 * lookup_gate(a, b, c, Some(d)): c is a function of three wires that are
 * already known, so a circuit that XORs, adds or substitutes bytes through a
 * table needs no looked-up value from the host.
 *
 * pnp_load_solve_plan_lookup is pnp_load_solve_plan_ecc with `lookup`, zero or
 * PNP_SOLVE_LOOKUP; pnp_load_solve_plan_ecc is this call with lookup = 0: the
 * same plan, info, plan_bytes, errors, launches and solution.  Any other
 * lookup bit is PNP_E_ARG (the message names lookup), refused before anything
 * resident is dropped; gates and ecc are validated as above; the flag is
 * accepted for a key without q_lookup rows (there are then no such rows and
 * nothing is allocated).
 * The rule joins the ones above, in the same rounds; in round t every rule
 * looks at K_(t-1).
 *   LOOKUP (flag set, the key's q_lookup[i] != 0, i not an output row): READY
 *     when the variables in slots a, b and d of row i are known and the one in
 *     slot c is not; bids for slot c.  It reads no next row, so the last gate
 *     row takes part.  With T the key's resident table of D rows (its
 *     lookup_len rows, then copies of row 0: MultiSet::pad), c = T[p][2], p the
 *     lowest row with T[p][0] = a, T[p][1] = b, T[p][3] = d, compared exactly
 *     on 3 x 256 bits: the reference's LookupTable::lookup.  No such row:
 *     c = 0; the solve inverts nothing and cannot fail, and pnp_check_* reports
 *     `row i: lookup constraint 0`, as it must: with no row under that key,
 *     (a, b, 0, d) is no row of T either.  A slot c whose variable is already
 *     known is not redefined: it stays a plain constraint for pnp_check_*.
 *   TIES: the least (row, role) still wins; the role order goes on after
 *     var-add's d_next with one role, lookup c.  The order of every bid of
 *     the rules above is unchanged, so their plans are too.  A row with
 *     q_lookup and q_arith both set follows both rules independently; on the
 *     same row the arithmetic slot wins the tie.
 * The plan: a lookup entry is 16 bytes, read as one 16-byte word (the target,
 * the sources a, b, d), in an array of its own, level order, by variable id
 * within a level, with its own level offsets.  With at least one lookup entry
 * the plan build also indexes the table: row 0 and every row whose four
 * columns differ from row 0's (the padding copies carry row 0's key and value
 * and a higher index: leaving them out changes no answer), m rows, go into
 * B = next_pow2(2 m) hash buckets by a hash of the 24 Montgomery words of their
 * columns 0, 1, 3; the row ids are sorted by bucket with the stable radix sort,
 * so a bucket lists its rows in ascending table order and the first exact match
 * of a scan is the lowest row; offsets off[0..B].  The build uses no atomics:
 * the index, like the rest of the plan, is byte for byte the same on every run.
 * Rows that share a hash but not a key only cost time.  Entries, level offsets
 * and index (4 (B + 1) + 4 m bytes, padded to 16) are counted in plan_bytes and
 * dropped with the plan.  The index reads the key's resident table columns at
 * solve time: every key load drops the wire map, and with it the plan.
 * A level is an arithmetic, a gate, an ECC and a lookup segment: more than 256
 * entries in all, a launch a non-empty segment; narrower levels with lookup
 * entries share one workgroup in which the lookup entries have waves of their
 * own (in a plan that also has ECC entries: the lanes of the gate waves after
 * the level's gate entries).  A plan without lookup entries launches exactly
 * what it launched before.
 * pnp_solve_info counts every defined variable of every kind in n_solved and
 * max_width.  pnp_solve_lookup_entries: out[0] = the variables lookup rows
 * define in the resident plan, out[1] = the table rows in the index (0 without
 * lookup entries); PNP_E_NOKEY without a plan.  Everything that takes a plan
 * takes this one the same way, as listed above; the stage list is unchanged
 * and solve_levels times every kind of entry. */
enum { PNP_SOLVE_LOOKUP = 1 };
int pnp_load_solve_plan_lookup(pnp_ctx *ctx, const uint32_t *input_ids, uint64_t n_inputs,
                               const uint64_t *output_rows, uint64_t n_outputs, uint32_t gates,
                               uint32_t ecc, uint32_t lookup, int device_ptrs,
                               pnp_solve_info *info /* may be NULL */);
int pnp_solve_lookup_entries(pnp_ctx *ctx, uint64_t out[2]);

/* Per-stage wall-clock (ms) of the last pnp_prove, for the bench/profiles.
 * Writes up to `cap` doubles and their names; returns the stage count. */
int pnp_last_stage_times(pnp_ctx *ctx, double *ms, const char **names, int cap);

/* Live per-kernel timing with HIP events recorded on the context stream
 * around the named kernels ("msm_accumulate", "quotient"); totals since the
 * last enable.  Used by bench.py for the roofline numbers. */
int pnp_kernel_timing(pnp_ctx *ctx, int enable);
int pnp_kernel_stats(pnp_ctx *ctx, const char *name, double *total_ms, int *launches);
/* Algorithmic bytes the timed launches of `name` were credited with (sum over
 * launches; e.g. msm_accumulate: points*(96 B point + 32 B scalar) of the
 * windows it processed). */
int pnp_kernel_bytes(pnp_ctx *ctx, const char *name, double *bytes);

/* Multi-GPU (one process per GPU, every rank runs pnp_prove on the same
 * inputs and returns the same ProofC).
 *
 * pnp_set_msm_shard: MSMs are sharded by point range — rank r takes points
 * [r*ceil(n/world), ...) over every window (with the folded table of that
 * range) and writes its B partial sums (XYZZ, 192 B each) to
 * d_xbuf + r * bytes_per_rank; after synchronizing its stream the library
 * calls allgather(user, bytes_per_rank), which must leave every rank's slot at
 * its offset in d_xbuf on every rank (an in-place all-gather, e.g. RCCL) and
 * return 0 once the data is visible to the device.  The same exchange carries
 * a few scalars per rank (split polynomial divisions, chunk flags).
 * world = 1 disables.
 *
 * pnp_set_exchange_a2a (optional, before pnp_load_prover_key; world must
 * divide 8): distributes gen_proof's round 4 — rank r owns blocks
 * [r*8/world, (r+1)*8/world) of the 8n coset (residues i mod 8) for the LDEs
 * and the quotient, and coefficient range r of the quotient chunks, the
 * linearisation and the opening witnesses.  One all-to-all moves the inverse
 * block transforms: the library fills world slots of bytes_per_peer at
 * d_a2a (slot s for rank s) and calls alltoall(user, bytes_per_peer), which
 * must leave the slot rank s sent to this rank at
 * d_a2a + (world + s) * bytes_per_peer. */
typedef int (*pnp_allgather_fn)(void *user, uint64_t bytes_per_rank);
/* Every all-gather slot ends with one tag word naming the exchange (the last
 * 8 bytes of each rank's bytes_per_rank): an exchange harness can tell the
 * messages apart without inferring them from sizes, and the library refuses
 * (PNP_E_DEVICE, "out of step") a result in which a peer's tag differs. */
#define PNP_EX_TAG_COUNTS    0xB0C4E7C0ULL  /* bucket-range MSMs: entry bytes per destination */
#define PNP_EX_TAG_MSM_SUMS  0x5EC7A111ULL  /* point-range MSMs: B partial sums (XYZZ)       */
#define PNP_EX_TAG_T_FLAGS   0x7F1A6500ULL  /* round 4: non-zero quotient chunks (8 words)   */
#define PNP_EX_TAG_DIV_CARRY 0xD1FC0001ULL  /* split divisions by (X - z): slice values   */
#define PNP_EX_TAG_EVALS     0xE7A15000ULL  /* round 5: partial evaluations (18 x 4 words)  */
#define PNP_EX_TAG_STATUS    0x57A7A500ULL  /* key load / derived tables: per-rank status   */
#define PNP_EX_TAG_DEVICE    0xDE71CE00ULL  /* key load: which GPU each rank runs on        */
typedef int (*pnp_alltoall_fn)(void *user, uint64_t bytes_per_peer);
/* pnp_set_exchange_v (optional, before the first commitment; world must
 * divide the bucket count): the folded MSMs shard BUCKET ranges instead of
 * point ranges — rank s owns buckets [s NB/world, (s+1) NB/world) of every MSM
 * of a batch, so each rank sorts, accumulates and reduces 1/world of the
 * buckets (the point-range scheme reduces all of them on every rank).  Each
 * rank digitises its own point range and sends every entry (8 bytes) to its
 * bucket's owner: the library writes world segments to d_send (segment s,
 * send_bytes[s] bytes, for rank s, back to back in rank order) and calls
 * alltoallv(user, send_bytes, recv_bytes), which must leave the segment rank s
 * sent to this rank at offset recv_bytes[0] + ... + recv_bytes[s-1] of d_recv
 * (recv_bytes comes from a preceding all-gather of the counts).  A batch whose
 * segments would not fit `capacity_bytes` (pathological scalars that crowd one
 * bucket range) falls back to point ranges.  The commit key's folded table then
 * covers all n points on every rank (6.5 GiB at n = 2^22). */
typedef int (*pnp_alltoallv_fn)(void *user, const uint64_t *send_bytes, const uint64_t *recv_bytes);
/* The library's HIP stream (a hipStream_t): every kernel and copy of a proof
 * runs on it in order.  An exchange that enqueues its collectives on this
 * stream (RCCL: libpnp_rccl.so, include/pnp_rccl.h) declares itself with
 * pnp_set_exchange_ordered(ctx, 1): the library then calls the callbacks
 * without synchronising the stream first, and a callback returns once its
 * collective is enqueued (the library's next copies and kernels are ordered
 * behind it).  Default 0: the stream is synchronised before every callback,
 * which must return with the data visible to the device (host-memory
 * exchanges, other streams). */
int pnp_ctx_stream(pnp_ctx *ctx, void **stream);
int pnp_set_exchange_ordered(pnp_ctx *ctx, int ordered);
int pnp_set_msm_shard(pnp_ctx *ctx, int rank, int world, pnp_allgather_fn allgather,
                      void *user, uint64_t *d_xbuf, uint64_t xbuf_bytes);
int pnp_set_exchange_a2a(pnp_ctx *ctx, pnp_alltoall_fn alltoall, void *user, uint64_t *d_a2a,
                         uint64_t a2a_bytes);
int pnp_set_exchange_v(pnp_ctx *ctx, pnp_alltoallv_fn alltoallv, void *user, uint64_t *d_send,
                       uint64_t *d_recv, uint64_t capacity_bytes);

/* ------------------------------------------------------------------ */
/* 3. Operator API on HBM pointers (mirrors PLONK/utils/function.cuh) */
/*    All ops are asynchronous on the context stream; pnp_sync waits.  */
/* ------------------------------------------------------------------ */

int pnp_sync(pnp_ctx *ctx);

/* In-place natural-order radix-2 NTT of 2^lg_n Montgomery Fr
 * (function.cu:249-273 Ntt / Intt; arkworks fft / ifft semantics).
 * inverse=1 multiplies by n^-1.  coset=1 applies the g=7 coset
 * (forward: x_i *= g^i before, inverse: x_i *= g^-i after). */
int pnp_ntt(pnp_ctx *ctx, uint64_t *d_inout, uint32_t lg_n, int inverse, int coset);

/* Ntt_coset::forward (function.cu:261-267): zero-pad n -> 8n, coset NTT. */
int pnp_coset_lde8(pnp_ctx *ctx, const uint64_t *d_coeffs, uint64_t *d_out8, uint32_t lg_n);

/* commit (KZG/kzg10.cu:31-44): MSM of n affine points with n Montgomery
 * scalars (converted to canonical inside, arithmetic.cu:3-8), result as
 * affine Montgomery point (infinity -> x=0, y=Fq one). Synchronous. */
int pnp_commit(pnp_ctx *ctx, const uint64_t *d_points, const uint64_t *d_scalars,
               uint64_t n, CommitmentC *out);

/* KZG commit (kzg10.cu:31-55) against the RESIDENT commit key
 * (pnp_load_commit_key): sum_{i<n} s_i powers_of_g[i], as gen_proof's
 * commitments.  Uses the folded fixed-base layout (2^(c k) multiples of the
 * first n SRS points, built on the first call for this n and kept).  */
int pnp_commit_ck(pnp_ctx *ctx, const uint64_t *d_scalars, uint64_t n, CommitmentC *out);

/* Extension (no reference counterpart; what gen_proof's round 1 uses): the
 * KZG commitment of the polynomial given by its n evaluations on the order-n
 * subgroup <omega> (natural order, Montgomery) — the same point as
 * pnp_commit_ck over its coefficients iNTT(evals), computed as
 * sum_i evals_i [L_i(tau)] G against the resident commit key in the Lagrange
 * basis (derived from the first n SRS points on the first call for this n and
 * kept; zero evaluations cost nothing).  n a power of two <= the key's points.
 * PNP_E_ARG when the basis is unavailable (PNP_LAGRANGE=0, degenerate key).  */
int pnp_commit_evals(pnp_ctx *ctx, const uint64_t *d_evals, uint64_t n, CommitmentC *out);

/* HBM accounting (extension): out[0] = device bytes this library holds now
 * (every context of the process), out[1] = their peak since the previous
 * pnp_hbm_usage call (which restarts it), and for the loaded
 * prover key the upper bounds pnp_load_prover_key budgets a proof with, still
 * to be allocated on this rank: out[2] mandatory (per-proof buffers, NTT
 * tables, the commit key's folded table, MSM work), out[3] the Lagrange-basis
 * key + table, out[4] the copy-constraint groups + table, out[5] the largest
 * build scratch.  The first pnp_prove after a key load checks them against
 * the rank's share of its GPU's free HBM: it fails with PNP_E_NOMEM before any
 * work (every rank of a multi-GPU run, naming the short one) when out[2] +
 * out[5] does not fit, and switches the optional tables off (same proof bytes)
 * when they do not. */
int pnp_hbm_usage(pnp_ctx *ctx, uint64_t out[6]);

/* Extension (operator form of gen_proof's copy-group commitments, wires.hip):
 * B <= 16 MSMs over sub-ranges of ONE base set — out[b] = sum_{i<n}
 * s_b[i] P[seg_off[b] + i] over the n_points affine points d_points (12 u64
 * each, Montgomery) — through one folded table built over all n_points (the
 * segmented batch of the round-1 wire commitments; each MSM's entries carry its
 * segment offset).  seg_off[b] + n <= n_points.  Single GPU.  Synchronous.  */
int pnp_commit_segments(pnp_ctx *ctx, const uint64_t *d_points, uint64_t n_points, int B,
                        const uint64_t *seg_off, const uint64_t *const *d_scalars, uint64_t n,
                        CommitmentC *out);

/* Extension (operator form of pnp_preprocess' permutation kernels,
 * preprocess.hip): the copy permutation of a wire map on the domain
 * D = 2^lg_n >= n_gates (lg_n <= 25).  d_var[j]: n_gates variable ids of wire
 * j in HBM, each < n_vars.  d_next (4 D u32): d_next[j D + i] = j' D + i', the
 * slot after (wire j, row i) among the slots of its variable in (row, wire)
 * order, cyclically; rows >= n_gates map to themselves.  d_sigma[j] (D
 * Montgomery Fr each): sigma_j(w^i) = K_j' w^i', K = (1, 7, 13, 17).  Either
 * output may be NULL (d_sigma, or single columns of it).  Synchronous.
 * PNP_E_ARG with the wire and row in pnp_last_error when an id is >= n_vars
 * (the outputs are then unspecified). */
int pnp_wire_sigma(pnp_ctx *ctx, const uint32_t *const d_var[4], uint64_t n_gates, uint64_t n_vars,
                   uint32_t lg_n, uint32_t *d_next, uint64_t *const d_sigma[4]);

/* Extension (operator form of pnp_prove_assignment's gather, assignment.hip):
 * the witness columns of a variable assignment on the domain D = 2^lg_n >=
 * n_gates (lg_n <= 25), in one launch: d_w[j][i] = d_values[d_var[j][i]] for
 * i < n_gates and zero for n_gates <= i < D (every row of the four outputs is
 * written).  d_var[j]: n_gates u32 ids; d_values: n_vars Montgomery Fr;
 * d_w[j]: D Fr; all HBM pointers, the Fr arrays 16-byte aligned.  The ids are
 * trusted to be < n_vars (the loaders validate their maps); one that is not
 * reads as zero, never outside d_values.  Asynchronous on the context stream.
 * PNP_E_ARG for n_gates = 0, n_gates > 2^lg_n, lg_n > 25, a NULL or misaligned
 * pointer. */
int pnp_gather_witness(pnp_ctx *ctx, const uint32_t *const d_var[4], uint64_t n_gates,
                       const uint64_t *d_values, uint64_t n_vars, uint32_t lg_n, uint64_t *const d_w[4]);

/* Extension (operator form of gen_proof's round-4 block transforms, ntt.hip).
 * The 8n coset x_i = g w_8n^i, g = 7, is kept in "block-bitrev layout": point
 * i = 8 j + m lives in block m at index brev(j) (brev: lg_n-bit reversal), so
 * every block is a size-n transform of its own.  n = 2^lg_n; every array is
 * Montgomery Fr in HBM, 4 u64 each, and every length below is in elements.
 * m0 >= 0, nb >= 1, m0 + nb <= 8, lg_n <= 25, no NULL pointer: else PNP_E_ARG.
 * Asynchronous on the context stream unless a mask is returned.
 *
 * pnp_lde_blocks: d_coeffs (n) -> d_out (nb n), d_out[b n + brev(j)] =
 * f(g w_8n^(8 j + m0 + b)) for b < nb; form29 != 0: 32 f(..) mod r instead
 * (the 2^261 form the quotient kernel reads).  d_out must not alias d_coeffs.
 *
 * pnp_to_blocks: the same permutation of values already on the coset: d_in
 * (8 n, natural order) -> d_out (nb n), d_out[b n + brev(j)] = d_in[8 j + m0 + b].
 *
 * pnp_intt_blocks: d_inout (nb n) in place; block b, holding residue
 * m = m0 + b in block-bitrev layout, becomes
 * Y_m[u] = w_8n^(-m u) sum_j blk_m[j] w_n^(-j u), natural order, no 1 / n.
 *
 * pnp_t_combine_blocks: d_Y (nb n: Y_0 .. Y_(nb-1) of a polynomial of degree
 * < nb n, nb = 6, 7 or 8) -> d_out (nb n), the coefficients in chunks:
 * d_out[m1 n + u] = c_(u + n m1) = g^-(u + n m1) / (8 n) sum_m w_8^(-m m1) Y_m[u]
 * (the Y_m, m >= nb, solved from the chunks m1 >= nb being zero).  *nz_out:
 * bit m1 set iff chunk m1 < nb has a non-zero coefficient.  Synchronous.
 *
 * pnp_t_combine_range: the same on all 8 blocks for the coefficient indices
 * u in [q0, q0 + len) only (one rank's share): d_Y (8 len, d_Y[m len + (u - q0)]
 * = Y_m[u]) -> d_out (8 len), d_out[m1 len + (u - q0)] = c_(u + n m1); *nz_out
 * as above, over this range.  q0 + len <= n.  Synchronous. */
int pnp_lde_blocks(pnp_ctx *ctx, const uint64_t *d_coeffs, uint64_t *d_out, uint32_t lg_n, int m0, int nb,
                   int form29);
int pnp_to_blocks(pnp_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, uint32_t lg_n, int m0, int nb);
int pnp_intt_blocks(pnp_ctx *ctx, uint64_t *d_inout, uint32_t lg_n, int m0, int nb);
int pnp_t_combine_blocks(pnp_ctx *ctx, const uint64_t *d_Y, int nb, uint64_t *d_out, uint32_t lg_n,
                         unsigned *nz_out);
int pnp_t_combine_range(pnp_ctx *ctx, const uint64_t *d_Y, uint64_t len, uint64_t q0, uint64_t *d_out,
                        uint32_t lg_n, unsigned *nz_out);

/* evaluate (function.cu:162-173): sum_i c_i x^i; x and result Montgomery,
 * host-side scalars.  Synchronous. */
int pnp_poly_eval(pnp_ctx *ctx, const uint64_t *d_coeffs, uint64_t n,
                  const uint64_t x[4], uint64_t out[4]);

/* poly_div_poly with c = -z (kzg10.cu:87-99): in place, p <- p / (X - z),
 * remainder dropped, top coefficient set to zero. */
int pnp_poly_div_linear(pnp_ctx *ctx, uint64_t *d_poly, uint64_t n, const uint64_t z[4]);

/* accumulate_mul_poly (mont_arithmetic.cu:334-360): out[0]=1,
 * out[i] = prod_{j<i} in[j]; in place. */
int pnp_prefix_product(pnp_ctx *ctx, uint64_t *d_inout, uint64_t n);

/* Batch inverse in place (inv(0) = 0, like the reference inv_mod kernel). */
int pnp_batch_inverse(pnp_ctx *ctx, uint64_t *d_inout, uint64_t n);

/* ------------------------------------------------------------------ */
/* 4. Synthetic-input utilities (bench / test plumbing, not the path)  */
/* ------------------------------------------------------------------ */

/* d_out[i] = uniform-ish Montgomery Fr from a counter-based hash of (seed,i). */
int pnp_synth_random_fr(pnp_ctx *ctx, uint64_t *d_out, uint64_t n, uint64_t seed);
/* d_out[i] = tau^i * G1 generator, affine Montgomery (an SRS); tau Montgomery. */
int pnp_synth_srs(pnp_ctx *ctx, uint64_t *d_out, uint64_t n, const uint64_t tau[4]);
/* Satisfying random arithmetic circuit on the n-domain (tests/bench):
 * in:  w[0] = a, w[3] = d (n_gates each), sel[0..7] = q_l q_r q_o q_4 q_c q_hl
 *      q_hr q_h4 evaluations (n each, rows >= n_gates ignored);
 * out: w[1] = b (b_i = a_pi(i)), w[2] = c (solved from the gate), sel[8] =
 *      q_arith evaluations, sigma[0..3] evaluations (copy cycles b_i <-> a_pi(i)). */
int pnp_synth_circuit(pnp_ctx *ctx, uint64_t *const w[4], uint64_t *const sel[9],
                      uint64_t *const sigma[4], uint64_t n, uint64_t n_gates, uint64_t pi_pos,
                      const uint64_t pi_canon[4]);
/* The reference's own Poseidon Merkle-tree circuit of height `height`
 * (merkle-tree/src/constraints.rs:20-107 laid out like the reference composer;
 * 193 (2^(height-1) - 1) + 5 gates, mirrors tests/merkle_circuit.py):
 * in:  consts = 199 canonical Fr (4 limbs each): the 189 Poseidon round
 *      constants, the 3x3 MDS matrix row-major, the domain tag;
 *      d_leaves = 2^(height-1) Montgomery Fr, d_blind = 8 Montgomery Fr (the
 *      two blinding rows of StandardComposer::new);
 * out: d_nodes = the 2^(height-1) - 1 tree nodes (level order, root first),
 *      w[0..3] wire values of the gates, sel[0..8] = q_l q_r q_o q_4 q_c q_hl
 *      q_hr q_h4 q_arith and sigma[0..3] evaluations on the n-domain,
 *      root_canon = the root (PI = -root at row gates - 1). */
int pnp_synth_merkle(pnp_ctx *ctx, uint32_t height, const uint64_t *consts, const uint64_t *d_leaves,
                     const uint64_t *d_blind, uint64_t *d_nodes, uint64_t *const w[4], uint64_t *const sel[9],
                     uint64_t *const sigma[4], uint64_t n, uint64_t root_canon[4]);
/* d_out[i] = (g * w_8n^i)^n - 1 (v_h on the 8n coset) and the coset points. */
int pnp_synth_coset_consts(pnp_ctx *ctx, uint64_t *d_vh, uint64_t *d_x, uint32_t lg_n);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#ifdef __cplusplus
static_assert(sizeof(CommitmentC) == 96, "CommitmentC layout (lib.rs:231-235)");
static_assert(sizeof(ProofEvaluationsC) == 26 * 32, "ProofEvaluationsC layout");
static_assert(sizeof(ProofC) == 2656, "ProofC layout (lib.rs:120-142)");
static_assert(sizeof(CircuitC) == 72, "CircuitC layout (lib.rs:144-155)");
static_assert(sizeof(ProverKeyC) == 44 * 8, "ProverKeyC layout (lib.rs:157-223)");
static_assert(sizeof(CommitKeyC) == 16, "CommitKeyC layout (lib.rs:225-229)");
static_assert(sizeof(pnp_verifier_key) == 8 + 96 + PNP_VK_POLYS * 96, "pnp_verifier_key layout (or_verifier_key)");
static_assert(sizeof(pnp_circuit_desc) == 3 * 8 + (4 + 15 + 4) * 8, "pnp_circuit_desc layout");
static_assert(sizeof(pnp_check_report) == (2 + PNP_CHECK_KINDS) * 8 + 4 * 4, "pnp_check_report layout");
static_assert(sizeof(pnp_solve_info) == 7 * 8, "pnp_solve_info layout");
#else
_Static_assert(sizeof(ProofC) == 2656, "ProofC layout (lib.rs:120-142)");
_Static_assert(sizeof(ProverKeyC) == 44 * 8, "ProverKeyC layout (lib.rs:157-223)");
#endif

#endif /* PNP_PLONK_H */
