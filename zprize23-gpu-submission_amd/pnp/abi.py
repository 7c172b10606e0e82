"""ctypes mirror of include/pnp_plonk.h.

This is the Python-side equivalent of the Rust FFI declarations in
plonk-core/src/lib.rs:52-239 (the structs are repr(C) there and plain C
structs here, field for field).  The host program (tests, bench) uses it to
marshal CircuitC / ProverKeyC / CommitKeyC exactly like Prover::prove_pnp
(plonk-core/src/proof_system/prover.rs:693-907) does on the Rust side.
"""
import ctypes as C

U64P = C.POINTER(C.c_uint64)
FR4 = C.c_uint64 * 4


class WireEvaluationsC(C.Structure):
    _fields_ = [("a_eval", FR4), ("b_eval", FR4), ("c_eval", FR4), ("d_eval", FR4)]


class PermutationEvaluationsC(C.Structure):
    _fields_ = [("left_sigma_eval", FR4), ("right_sigma_eval", FR4),
                ("out_sigma_eval", FR4), ("permutation_eval", FR4)]


class CustomEvaluationsC(C.Structure):
    _fields_ = [(n, FR4) for n in (
        "q_arith_eval", "q_c_eval", "q_l_eval", "q_r_eval", "q_hl_eval",
        "q_hr_eval", "q_h4_eval", "a_next_eval", "b_next_eval", "d_next_eval")]


class LookupEvaluationsC(C.Structure):
    _fields_ = [(n, FR4) for n in (
        "q_lookup_eval", "z2_next_eval", "h1_eval", "h1_next_eval", "h2_eval",
        "f_eval", "table_eval", "table_next_eval")]


class ProofEvaluationsC(C.Structure):
    _fields_ = [("wire_evals", WireEvaluationsC), ("perm_evals", PermutationEvaluationsC),
                ("lookup_evals", LookupEvaluationsC), ("custom_evals", CustomEvaluationsC)]


class CommitmentC(C.Structure):
    _fields_ = [("x", C.c_uint64 * 6), ("y", C.c_uint64 * 6)]


PROOF_COMMITMENTS = ("a_comm", "b_comm", "c_comm", "d_comm", "z_comm", "f_comm",
                     "h_1_comm", "h_2_comm", "z_2_comm", "t_1_comm", "t_2_comm",
                     "t_3_comm", "t_4_comm", "t_5_comm", "t_6_comm", "t_7_comm",
                     "t_8_comm", "aw_opening", "saw_opening")


class ProofC(C.Structure):
    _fields_ = [(n, CommitmentC) for n in PROOF_COMMITMENTS] + [
        ("evaluations", ProofEvaluationsC)]


class CircuitC(C.Structure):
    _fields_ = [("n", C.c_uint64), ("lookup_len", C.c_uint64), ("intended_pi_pos", C.c_uint64),
                ("q_lookup", U64P), ("pi", U64P), ("w_l", U64P), ("w_r", U64P),
                ("w_o", U64P), ("w_4", U64P)]


PK_FIELDS = (
    "q_m_coeffs", "q_m_evals", "q_l_coeffs", "q_l_evals", "q_r_coeffs", "q_r_evals",
    "q_o_coeffs", "q_o_evals", "q_4_coeffs", "q_4_evals", "q_c_coeffs", "q_c_evals",
    "q_hl_coeffs", "q_hl_evals", "q_hr_coeffs", "q_hr_evals", "q_h4_coeffs", "q_h4_evals",
    "q_arith_coeffs", "q_arith_evals",
    "range_selector_coeffs", "range_selector_evals",
    "logic_selector_coeffs", "logic_selector_evals",
    "fixed_group_add_selector_coeffs", "fixed_group_add_selector_evals",
    "variable_group_add_selector_coeffs", "variable_group_add_selector_evals",
    "q_lookup_coeffs", "q_lookup_evals", "table1", "table2", "table3", "table4",
    "left_sigma_coeffs", "left_sigma_evals", "right_sigma_coeffs", "right_sigma_evals",
    "out_sigma_coeffs", "out_sigma_evals", "fourth_sigma_coeffs", "fourth_sigma_evals",
    "linear_evaluations", "v_h_coset_8n")


class ProverKeyC(C.Structure):
    _fields_ = [(n, U64P) for n in PK_FIELDS]


class CommitKeyC(C.Structure):
    _fields_ = [("powers_of_g", U64P), ("powers_of_gamma_g", U64P)]


class AffineLayout(C.Structure):
    """pnp_affine_layout: where x, y (6 u64 Montgomery limbs each) and the
    infinity byte sit in one arkworks G1Affine of `stride` bytes."""
    _fields_ = [("stride", C.c_uint64), ("x_off", C.c_uint64), ("y_off", C.c_uint64),
                ("inf_off", C.c_uint64)]


# ark-ec 0.3 GroupAffine<g1::Parameters> as rustc lays it out on x86-64
# (x: Fp384, y: Fp384, infinity: bool, 7 bytes of padding)
ARK_G1_AFFINE = AffineLayout(stride=104, x_off=0, y_off=48, inf_off=96)

U32P = C.POINTER(C.c_uint32)

# pnp_verifier_key.polys, in order (the oracle's or_verifier_key)
VK_POLYS = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_hl", "q_hr", "q_h4", "q_arith",
            "range_selector", "logic_selector", "fixed_group_add_selector",
            "variable_group_add_selector", "left_sigma", "right_sigma", "out_sigma",
            "fourth_sigma", "q_lookup", "table1", "table2", "table3", "table4")
# pnp_circuit_desc.sel, in order
DESC_SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_hl", "q_hr", "q_h4", "q_arith",
                  "range_selector", "logic_selector", "fixed_group_add_selector",
                  "variable_group_add_selector", "q_lookup")


class VerifierKey(C.Structure):
    """pnp_verifier_key: the domain size, SRS_0 and the 23 commitments of the
    preprocessed polynomials (VK_POLYS order); 1 + 12 + 23 * 12 u64."""
    _fields_ = [("n", C.c_uint64), ("g", C.c_uint64 * 12), ("polys", CommitmentC * len(VK_POLYS))]


class CircuitDesc(C.Structure):
    """pnp_circuit_desc: what a composer holds.  var: 4 x n_gates u32 variable
    ids (left, right, out, fourth); sel: DESC_SELECTORS row values (n_gates
    Montgomery Fr each, NULL = a zero column); table: 4 x lookup_len Fr."""
    _fields_ = [("n_gates", C.c_uint64), ("n_vars", C.c_uint64), ("lookup_len", C.c_uint64),
                ("var", U32P * 4), ("sel", U64P * len(DESC_SELECTORS)), ("table", U64P * 4)]


# Proving from a variable assignment over the resident wire map: the ctypes
# argument lists of the three entry points (pnp.load() installs them).
#   pnp_load_wire_map(ctx, var[4], n_gates, n_vars, device_ptrs)
#   pnp_gather_witness(ctx, d_var[4], n_gates, d_values, n_vars, lg_n, d_w[4])
#   pnp_prove_assignment(ctx, values, n_vars, device_ptrs, n_pi, pi_pos, pi_canon, label, out)
ASSIGNMENT_ARGTYPES = {
    "pnp_load_wire_map": [C.c_void_p, C.c_void_p * 4, C.c_uint64, C.c_uint64, C.c_int],
    "pnp_gather_witness": [C.c_void_p, C.c_void_p * 4, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                           C.c_void_p * 4],
    "pnp_prove_assignment": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,
                             C.c_char_p, C.POINTER(ProofC)],
}

# The satisfiability check (pnp_check_assignment, pnp_check_witness).
PNP_E_UNSAT = -6
CHECK_KINDS = ("arith", "range", "logic", "fixed_add", "var_add", "lookup", "copy")


class CheckReport(C.Structure):
    """pnp_check_report: violated (row, constraint) pairs by kind (CHECK_KINDS
    order; copy: slots), their sum, and the least (row, kind, index);
    first_row = 2^64 - 1 when nothing is violated."""
    _fields_ = [("violations", C.c_uint64), ("by_kind", C.c_uint64 * len(CHECK_KINDS)),
                ("first_row", C.c_uint64), ("first_kind", C.c_uint32), ("first_index", C.c_uint32),
                ("copy_checked", C.c_uint32), ("reserved", C.c_uint32)]


#   pnp_check_assignment(ctx, values, n_vars, device_ptrs, n_pi, pi_pos, pi_canon, report)
#   pnp_check_witness(ctx, cs, device_ptrs, n_pi, pi_pos, pi_canon, report)
CHECK_ARGTYPES = {
    "pnp_check_assignment": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,
                             C.POINTER(CheckReport)],
    "pnp_check_witness": [C.c_void_p, C.POINTER(CircuitC), C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,
                          C.POINTER(CheckReport)],
}

class SolveInfo(C.Structure):
    """pnp_solve_info: what a solve plan covers.  n_levels rounds, the widest
    max_width entries; first_undetermined = 2^64 - 1 when every variable is
    an input or solved; plan_bytes = the HBM the resident plan holds."""
    _fields_ = [(n, C.c_uint64) for n in ("n_inputs", "n_solved", "n_levels", "max_width", "n_undetermined",
                                          "first_undetermined", "plan_bytes")]


# The witness solver.
#   pnp_load_solve_inputs(ctx, input_ids, n_inputs, device_ptrs, info)
#   pnp_solve_assignment(ctx, inputs, n_inputs, device_ptrs, n_pi, pi_pos, pi_canon)
#   pnp_assignment_ptr(ctx, &d_values, &n_vars)
#   pnp_assignment_values(ctx, ids, k, out)
# With output rows (public inputs the solve derives):
#   pnp_load_solve_plan(ctx, input_ids, n_inputs, output_rows, n_outputs, device_ptrs, info)
#   pnp_solved_public_inputs(ctx, pos, canon, cap, &n)
#   pnp_prove_solved(ctx, n_pi, pi_pos, pi_canon, label, out)
#   pnp_check_solved(ctx, n_pi, pi_pos, pi_canon, report)
# With range and logic rows that define (gates: SOLVE_RANGE | SOLVE_LOGIC):
#   pnp_load_solve_plan_gates(ctx, input_ids, n_inputs, output_rows, n_outputs, gates, device_ptrs, info)
#   pnp_solve_gate_entries(ctx, out[2])
# With fixed-base and curve-addition rows that define (ecc: SOLVE_FIXED_ADD | SOLVE_VAR_ADD):
#   pnp_load_solve_plan_ecc(ctx, input_ids, n_inputs, output_rows, n_outputs, gates, ecc, device_ptrs, info)
#   pnp_solve_ecc_entries(ctx, out[2])
SOLVE_RANGE, SOLVE_LOGIC = 1, 2
# With lookup rows that define (lookup: SOLVE_LOOKUP):
#   pnp_load_solve_plan_lookup(ctx, input_ids, n_inputs, output_rows, n_outputs, gates, ecc, lookup, device_ptrs, info)
#   pnp_solve_lookup_entries(ctx, out[2])
SOLVE_FIXED_ADD, SOLVE_VAR_ADD = 1, 2
SOLVE_LOOKUP = 1
SOLVE_ARGTYPES = {
    "pnp_load_solve_plan_lookup": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_int, C.POINTER(SolveInfo)],
    "pnp_solve_lookup_entries": [C.c_void_p, C.POINTER(C.c_uint64 * 2)],
    "pnp_load_solve_plan_ecc": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                C.c_int, C.POINTER(SolveInfo)],
    "pnp_solve_ecc_entries": [C.c_void_p, C.POINTER(C.c_uint64 * 2)],
    "pnp_load_solve_plan_gates": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int,
                                  C.POINTER(SolveInfo)],
    "pnp_solve_gate_entries": [C.c_void_p, C.POINTER(C.c_uint64 * 2)],
    "pnp_load_solve_plan": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                            C.POINTER(SolveInfo)],
    "pnp_solved_public_inputs": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)],
    "pnp_prove_solved": [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(ProofC)],
    "pnp_check_solved": [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(CheckReport)],
    "pnp_load_solve_inputs": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(SolveInfo)],
    "pnp_solve_assignment": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p],
    "pnp_assignment_ptr": [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)],
    "pnp_assignment_values": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p],
}

# The block-layout transforms of round 4 in operator form (HBM addresses).
#   pnp_lde_blocks(ctx, d_coeffs, d_out, lg_n, m0, nb, form29)
#   pnp_to_blocks(ctx, d_in, d_out, lg_n, m0, nb)
#   pnp_intt_blocks(ctx, d_inout, lg_n, m0, nb)
#   pnp_t_combine_blocks(ctx, d_Y, nb, d_out, lg_n, nz_out)
#   pnp_t_combine_range(ctx, d_Y, len, q0, d_out, lg_n, nz_out)
BLOCK_ARGTYPES = {
    "pnp_lde_blocks": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int],
    "pnp_to_blocks": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int],
    "pnp_intt_blocks": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int],
    "pnp_t_combine_blocks": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint)],
    "pnp_t_combine_range": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                            C.POINTER(C.c_uint)],
}

assert C.sizeof(CheckReport) ==(2 + len(CHECK_KINDS)) * 8 + 16
assert C.sizeof(SolveInfo) == 7 * 8
assert C.sizeof(VerifierKey) == 8 + 96 + 23 * 96
assert C.sizeof(CircuitDesc) == 3 * 8 + (4 + 15 + 4) * 8
assert C.sizeof(ProofC) == 2656
assert C.sizeof(CircuitC) == 72
assert C.sizeof(ProverKeyC) == 44 * 8
assert C.sizeof(CommitKeyC) == 16


def proof_to_bytes(p: ProofC) -> bytes:
    return bytes(C.string_at(C.addressof(p), C.sizeof(p)))


def ptr(addr: int):
    """Raw integer address (host or HBM) -> uint64_t* for the structs."""
    return C.cast(C.c_void_p(addr), U64P)
