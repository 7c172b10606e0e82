"""Fixed-base and curve-addition rows that define, on the MI355X:
pnp_load_solve_plan_ecc (the plan build of csrc/solve.hip with the two ECC
families), the ECC entries of pnp_solve_assignment (k_solve_ecc_wide_,
k_solve_ecc_mixed_, the NAF kind of the gate entries) and everything
downstream of a plan, against the plain-integer model of
tests/solve_ecc_ref.py, the composer's own values and the oracle's proof
bytes.  Every comparison is exact.

A plan is compared through pnp_solve_info (defined variables, levels, the
widest level), pnp_solve_gate_entries and pnp_solve_ecc_entries."""
import ctypes
import functools

import numpy as np
import pytest

from circuits import Composer, R_MOD, jj_add, jj_point
from ecc_circuits import fixed_base_mul_of, point_add_of
from gate_circuits import M1
from pnp import abi
from solve_ecc_ref import FIXED_ADD, VAR_ADD, plan, plan_sweep, solve
from solve_gates_ref import LOGIC, RANGE
from solve_ref import merkle_inputs
from test_gpu_solve import NONE, PNP_E_ARG, context_for, info_tuple, mont, solve_gpu
from test_gpu_solve_gates import load_gates
from test_solve_ecc_ref import (fixed_rows, full_multiplication, last_row_circuits, mixed_circuit, scalar_mul,
                                tie_both_families_on_one_row, tie_point_and_arith, tie_var_roles, zero_denominator)

pytestmark = pytest.mark.gpu

ECC = FIXED_ADD | VAR_ADD
GATES = RANGE | LOGIC
PNP_E_NOKEY = -3
KIND_FIXED, KIND_VAR = abi.CHECK_KINDS.index("fixed_add"), abi.CHECK_KINDS.index("var_add")


def load_ecc(ctx, ids, ecc=ECC, gates=0, rows=()):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    return ctx.load_solve_plan_ecc(ids.ctypes.data if len(ids) else 0, len(ids),
                                   rows.ctypes.data if len(rows) else 0, len(rows), gates, ecc, False)


def model(cp, ids, ecc=ECC, gates=0, outputs=(), vals=None, sweep=True):
    """(plan, solution) of the model from the values cp holds (or `vals`) for ids."""
    n_vars = len(cp.vals)
    pl = (plan_sweep if sweep else plan)(cp.rows, n_vars, ids, outputs, gates, ecc)
    vals = cp.vals if vals is None else vals
    return pl, solve(cp.rows, pl, n_vars, {u: vals[u] for u in ids}, None, outputs)


def plan_matches(ctx, info, ids, pl):
    assert info_tuple(info) == (len(ids), pl.n_solved, len(pl.levels), pl.max_width, 0, NONE)
    assert ctx.solve_gate_entries() == (pl.n_range, pl.n_logic)
    assert ctx.solve_ecc_entries() == (pl.n_fixed, pl.n_var)


def computed_scalar_mul(seed, num_bits):
    """scalar = p + q = 170 through an arithmetic row, then one multiplication."""
    cp = Composer(seed)
    p, q = cp.var(100), cp.var(70)
    s = cp.var(170)
    cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, p, q, s, 0)
    first, res = fixed_base_mul_of(cp, s, jj_point(cp.rng), num_bits)
    return cp, [0, p, q], (p, q, s), first, res


# ------------------------------------------------------------------ 1. a computed scalar
def test_a_multiplication_of_a_computed_scalar_solves_checks_and_proves():
    cp, ids, (p, q, s), first, res = computed_scalar_mul(41, 8)
    inp = cp.build(min_lg=6)
    assert inp.n == 64
    exp = abi.proof_to_bytes(inp.oracle_proof())
    pl, vals = model(cp, ids)
    assert vals == cp.vals and pl.undetermined == [] and len(pl.levels) == 2 + 7 + 8
    ctx = context_for(cp, inp)
    try:
        rc, info = load_ecc(ctx, ids)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert ctx.solve_ecc_entries() == (7 + 8 + 16, 0)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
        assert list(dict(ctx.stage_times())) == ["solve_inputs", "solve_levels", "inputs_h2d_bytes"]
        ok, rep = ctx.check_solved([])
        assert ok and rep.violations == 0, ctx.last_error()
        assert abi.proof_to_bytes(ctx.prove_solved([])) == exp
        # other inputs over the same plan: 5 + 80 = 85, and 0
        for vp_, vq in ((5, 80), (0, 0)):
            other = list(cp.vals)
            other[p], other[q] = vp_, vq
            _, want = model(cp, ids, vals=other)
            assert want[s] == vp_ + vq
            assert np.array_equal(solve_gpu(ctx, other, ids, False), mont(want))
            assert ctx.check_solved([])[0], ctx.last_error()
        # the same plan with the flag of a family the key does not have
        rc, again = load_ecc(ctx, ids, ECC, GATES)
        assert rc == 0 and bytes(again) == bytes(info) and ctx.solve_ecc_entries() == (31, 0)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. a scalar with too many digits
def test_a_scalar_whose_naf_outgrows_the_rows_is_solved_and_the_check_names_the_row():
    cp, ids, (p, q, s), first, res = computed_scalar_mul(42, 8)
    other = list(cp.vals)
    other[p], other[q] = 100, 71  # 171: nine digits
    pl, want = model(cp, ids, vals=other)
    d1 = cp.rows[first + 1][1][3]
    assert want[s] == 171 and want[d1] == 2
    ctx = context_for(cp)
    try:
        rc, info = load_ecc(ctx, ids)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, other, ids, False), mont(want))  # (a failing solve raises)
        ok, rep = ctx.check_solved([])
        assert not ok and (rep.first_row, rep.first_kind, rep.first_index) == (first, KIND_FIXED, 0)
        assert f"row {first}: fixed_add constraint 0" in ctx.last_error()
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. the full width
def test_a_full_multiplication_by_2_254_minus_1():
    cp, ids, res = full_multiplication()
    inp = cp.build(min_lg=9)
    assert inp.n == 512
    exp = abi.proof_to_bytes(inp.oracle_proof())
    pl, vals = model(cp, ids, sweep=False)
    assert vals == cp.vals and len(pl.levels) == 2 + 254 + 255
    ctx = context_for(cp, inp)
    try:
        rc, info = load_ecc(ctx, ids)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
        ok, rep = ctx.check_solved([])
        assert ok and rep.violations == 0, ctx.last_error()
        assert abi.proof_to_bytes(ctx.prove_solved([])) == exp
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. point additions
def test_a_point_addition_of_two_curve_points():
    cp = Composer(43)
    p, q = jj_point(cp.rng), jj_point(cp.rng)
    pv, qv = (cp.var(p[0]), cp.var(p[1])), (cp.var(q[0]), cp.var(q[1]))
    r, res = point_add_of(cp, pv, qv)
    ids = [0, *pv, *qv]
    pl, vals = model(cp, ids)
    assert vals == cp.vals and (vals[res[0]], vals[res[1]]) == jj_add(p, q)
    ctx = context_for(cp)
    try:
        for ecc in (VAR_ADD, ECC):
            rc, info = load_ecc(ctx, ids, ecc)
            assert rc == 0, ctx.last_error()
            plan_matches(ctx, info, ids, pl)
            assert ctx.solve_ecc_entries() == (0, 3)
            assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
            assert ctx.check_solved([])[0], ctx.last_error()
    finally:
        ctx.close()


def test_a_zero_denominator_defines_zero_and_the_check_names_the_row():
    cp, ids, r, res = zero_denominator()
    pl, vals = model(cp, ids)
    assert vals == cp.vals and vals[res[0]] == 0 and vals[res[1]] != 0
    ctx = context_for(cp)
    try:
        rc, info = load_ecc(ctx, ids)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(vals))
        ok, rep = ctx.check_solved([])
        assert not ok and (rep.first_row, rep.first_kind, rep.first_index) == (r, KIND_VAR, 1)
        assert f"row {r}: var_add constraint 1" in ctx.last_error()
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. every family in one circuit
def test_every_family_into_an_output_row():
    cp, ids, out = mixed_circuit()
    inp = cp.build(min_lg=6)
    exp = abi.proof_to_bytes(inp.oracle_proof())
    pl, vals = model(cp, ids, ECC, GATES, [out])
    assert vals == cp.vals and pl.undetermined == [] and pl.n_var == 3 and pl.n_range == 3
    ctx = context_for(cp, inp)
    try:
        rc, info = load_ecc(ctx, ids, ECC, GATES, [out])
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
        assert ctx.solved_public_inputs() == [(out, cp.pis[out])]
        assert list(dict(ctx.stage_times())) == ["solve_inputs", "solve_levels", "solve_outputs", "inputs_h2d_bytes"]
        ok, rep = ctx.check_solved([])
        assert ok and rep.violations == 0, ctx.last_error()
        assert abi.proof_to_bytes(ctx.prove_solved([])) == exp
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6. width
@functools.lru_cache(maxsize=None)
def wide_multiplications():
    """300 two-row multiplications of input scalars 0..2 side by side: every
    level's segments (the scalar entries, the xy and point entries) hold 300
    entries or more."""
    cp = Composer(44)
    ids = [0]
    base = jj_point(cp.rng)
    for k in range(300):
        s = cp.var(k % 3)
        fixed_base_mul_of(cp, s, base, 2)
        ids.append(s)
    assert len(cp.rows) == 300 * 7
    pl, vals = model(cp, ids, sweep=False)
    return cp, ids, pl, vals


def test_wide_levels_of_ecc_entries():
    cp, ids, pl, vals = wide_multiplications()
    assert vals == cp.vals and pl.undetermined == []
    # the constants and last accumulators; d of the second row; the first point step (with c of both rows); the second
    assert pl.widths == [1200, 300, 1200, 600] and pl.ecc_widths == [0, 300, 1200, 600]
    ctx = context_for(cp)
    try:
        rc, info = load_ecc(ctx, ids, FIXED_ADD)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(vals))
        assert ctx.check_solved([])[0], ctx.last_error()
    finally:
        ctx.close()


def test_a_level_wide_only_by_the_three_segments_together():
    """100 arithmetic entries, 25 range rows (100 gate entries) and 100 var-add rows in one level."""
    cp = Composer(45)
    ids = [0]
    for k in range(100):
        x = cp.var(cp.rnd())
        cp.row({"q_arith": 1, "q_l": 5, "q_c": 7, "q_r": M1}, x, cp.var(5 * cp.vals[x] + 7), 0, 0)
        pv, qv = [tuple(cp.var(c) for c in jj_point(cp.rng)) for _ in range(2)]
        point_add_of(cp, pv, qv)
        ids += [x, *pv, *qv]
        if k < 25:
            v = cp.var(cp.rnd())
            cp.row({"range_selector": 1}, *(cp.var(cp.vals[v] >> s) for s in (2, 4, 6, 8)))
            cp.row({}, 0, 0, 0, v)
            ids.append(v)
    pl, vals = model(cp, ids, ECC, RANGE)
    assert vals == cp.vals and (pl.arith_widths, pl.gate_widths, pl.ecc_widths) == ([100], [100], [300])
    ctx = context_for(cp)
    try:
        rc, info = load_ecc(ctx, ids, ECC, RANGE)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(vals))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7. ties, known slots, the flag
def run_tie(cp, ids, vals=None):
    pl, want = model(cp, ids, vals=vals)
    ctx = context_for(cp)
    try:
        rc, info = load_ecc(ctx, ids)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        return pl, want, solve_gpu(ctx, cp.vals if vals is None else vals, ids, False)
    finally:
        ctx.close()


@pytest.mark.parametrize("arith_first", [True, False], ids=["arith_lower", "fixed_lower"])
def test_tie_between_an_arithmetic_and_a_fixed_add_row_goes_to_the_lower_row(arith_first):
    cp, ids, u, ra, rf, (pt, base) = tie_point_and_arith(arith_first)
    pl, vals, got = run_tie(cp, ids)
    assert vals[u] == ((cp.vals[ids[1]] + 1) % R_MOD if arith_first else jj_add(pt, base)[0])
    assert np.array_equal(got, mont(vals))


def test_tie_between_two_roles_of_one_var_add_row_goes_to_the_lower_role():
    cp, ids, u, r, total = tie_var_roles()
    pl, vals, got = run_tie(cp, ids)
    assert (vals[u], vals[u + 1]) == total and pl.n_var == 2
    assert np.array_equal(got, mont(vals))


def test_tie_on_one_row_goes_to_the_fixed_add_roles():
    cp, ids, (x3, y3, dn), r, (p, q, base) = tie_both_families_on_one_row()
    pl, vals, got = run_tie(cp, ids)
    assert (pl.n_fixed, pl.n_var) == (0, 3) and np.array_equal(got, mont(vals))
    given = list(cp.vals)
    given[dn] = (2 * q[1] + 1) % R_MOD
    pl, vals, got = run_tie(cp, ids + [dn], given)
    assert (pl.n_fixed, pl.n_var) == (2, 0) and (vals[x3], vals[y3]) == jj_add(p, base)
    assert np.array_equal(got, mont(vals))


def test_a_point_slot_listed_as_input_keeps_its_value_and_the_check_names_the_row():
    cp, ids, s, res = scalar_mul(99, 170, 8)
    row = fixed_rows(cp)[4]
    mid = cp.rows[row][1][0]
    given = list(cp.vals)
    given[mid] = 12345
    pl, vals, got = run_tie(cp, ids + [mid], given)
    assert vals[mid] == 12345 and pl.n_fixed == 7 + 8 + 15 and np.array_equal(got, mont(vals))
    ctx = context_for(cp)
    try:
        assert load_ecc(ctx, ids + [mid])[0] == 0
        solve_gpu(ctx, given, ids + [mid], False)
        ok, rep = ctx.check_solved([])
        assert not ok and (rep.first_row, rep.first_kind) == (row - 1, KIND_FIXED)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids + [mid], False), mont(cp.vals))  # the right value: clean
        assert ctx.check_solved([])[0]
    finally:
        ctx.close()


def test_ecc_variables_are_undetermined_without_the_flag_and_solved_with_it():
    cp, ids, s, res = scalar_mul(46, 170, 8)
    n_vars = len(cp.vals)
    pl, vals = model(cp, ids)
    none, _ = model(cp, ids, 0)
    assert none.n_solved == 4 and none.undetermined[0] == cp.rows[fixed_rows(cp)[0]][1][2]
    ctx = context_for(cp)
    try:
        for how in ("gates", 0, VAR_ADD):
            rc, info = load_gates(ctx, ids, GATES) if how == "gates" else load_ecc(ctx, ids, how, GATES)
            assert rc == PNP_E_ARG and info_tuple(info) == (2, 4, 1, 4, len(none.undetermined), none.undetermined[0])
            assert f"variable {none.undetermined[0]} " in ctx.last_error()
            assert ctx.lib.pnp_solve_ecc_entries(ctx.h, ctypes.byref((ctypes.c_uint64 * 2)())) == PNP_E_NOKEY
        rc, info = load_ecc(ctx, ids, FIXED_ADD)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
    finally:
        ctx.close()


def test_an_ecc_row_without_a_next_row_defines_nothing():
    for cp, ids, u in last_row_circuits():
        ctx = context_for(cp)
        try:
            rc, info = load_ecc(ctx, ids)
            assert rc == PNP_E_ARG and info_tuple(info) == (len(ids), 0, 0, 0, 1, u)
            rc, info = load_ecc(ctx, ids + [u])
            assert rc == 0 and info.n_solved == 0 and ctx.solve_ecc_entries() == (0, 0)
        finally:
            ctx.close()


# ------------------------------------------------------------------ 8. lifecycle
def test_lifecycle_accounting_flags_and_drop():
    import pnp
    from test_gpu_assignment import host_cols
    from test_preprocess_ref import wire_map
    cp, ids, out = mixed_circuit()
    n_vars = len(cp.vals)
    pl, vals = model(cp, ids, ECC, GATES, [out])
    pair = (ctypes.c_uint64 * 2)()
    ctx = context_for(cp)
    try:
        assert ctx.lib.pnp_solve_ecc_entries(ctx.h, ctypes.byref(pair)) == PNP_E_NOKEY  # before any plan
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.solve_ecc_entries()
        before = ctx.hbm_usage()["live"]
        # ecc = 0 is pnp_load_solve_plan_gates: the ECC variables as inputs
        ecc_vars = sorted(u for l in pl.levels for u, _, role in l if role >= 13)
        rc, plain = load_gates(ctx, ids + ecc_vars, GATES, [out])
        assert rc == 0, ctx.last_error()
        assert ctx.hbm_usage()["live"] == before + plain.plan_bytes and ctx.solve_ecc_entries() == (0, 0)
        rc, same = load_ecc(ctx, ids + ecc_vars, 0, GATES, [out])
        assert rc == 0 and bytes(same) == bytes(plain)
        rc, same = load_ecc(ctx, ids + ecc_vars, ECC, GATES, [out])  # (the flags on, nothing left for them to define)
        assert rc == 0 and bytes(same) == bytes(plain) and ctx.solve_ecc_entries() == (0, 0)
        assert ctx.hbm_usage()["live"] == before + plain.plan_bytes
        # bad ecc bits are refused before anything is dropped; bad gates bits as before
        for bad in (4, 8, ECC | 4, 1 << 31):
            rc, info = load_ecc(ctx, ids, bad, GATES, [out])
            assert rc == PNP_E_ARG and "ecc" in ctx.last_error()
        rc, info = load_ecc(ctx, ids, ECC, 4, [out])
        assert rc == PNP_E_ARG and "gates" in ctx.last_error()
        assert ctx.solve_gate_entries() == (pl.n_range, 0) and ctx.hbm_usage()["live"] == before + plain.plan_bytes
        # the ECC plan: 16 B a scalar entry, 128 B an ECC entry (at most one a variable), the level offsets
        rc, info = load_ecc(ctx, ids, ECC, GATES, [out])
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes
        n_scalar = 7
        n_ecc_vars = pl.n_fixed + pl.n_var - n_scalar
        assert info.plan_bytes > plain.plan_bytes - 4 * len(ecc_vars) + 16 * n_scalar + 128 * (n_ecc_vars // 3)
        assert info.plan_bytes <= plain.plan_bytes + 16 * (n_scalar + 3) + 128 * (n_ecc_vars + 3) \
            + 2 * 4 * (len(pl.levels) + 4) + 300 * len(pl.levels)
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):  # a plan, no solution yet
            ctx.assignment_ptr()
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(vals))
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes + 32 * n_vars
        addr, n = ctx.assignment_ptr()
        assert n == n_vars and ctx.check_assignment(addr, n, True, sorted(cp.pis.items()))[0]
        # a plan without ECC entries replaces it, and its arrays go
        rc, again = load_gates(ctx, ids + ecc_vars, GATES, [out])
        assert rc == 0 and bytes(again) == bytes(plain)
        assert ctx.hbm_usage()["live"] == before + plain.plan_bytes and ctx.solve_ecc_entries() == (0, 0)
        # whatever replaces the wire map drops the plan and the solution
        assert load_ecc(ctx, ids, ECC, GATES, [out])[0] == 0
        solve_gpu(ctx, cp.vals, ids, False)
        keep, addrs = host_cols(wire_map(cp))
        ctx.load_wire_map(addrs, len(cp.rows), n_vars, device_ptrs=False)
        assert ctx.hbm_usage()["live"] == before
        assert ctx.lib.pnp_solve_ecc_entries(ctx.h, ctypes.byref(pair)) == PNP_E_NOKEY
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.check_solved([])
    finally:
        ctx.close()


def test_a_sharded_context_is_refused():
    import torch
    from pnp.shard import SoloExchange, a2a_bytes_for, v_bytes_for
    from test_gpu_assignment import inst
    cp, inp, _, _, _ = inst("merkle4")
    ctx = context_for(cp)
    try:
        solo = SoloExchange(1, 2, device=torch.device("cuda", 0), a2a_bytes=a2a_bytes_for(inp.lg_n, 2),
                            v_bytes=v_bytes_for(inp.lg_n, 2))
        ctx.set_msm_shard(solo)
        rc, _ = load_ecc(ctx, merkle_inputs(cp), ECC, GATES, [len(cp.rows) - 1])
        assert rc == PNP_E_ARG and "ranks" in ctx.last_error()
    finally:
        ctx.close()
