"""Lookup rows that define, on the MI355X: pnp_load_solve_plan_lookup (the plan
build of csrc/solve.hip with the lookup rule and the table index), the lookup
entries of pnp_solve_assignment (k_solve_lookup_wide_, k_solve_lookup_mixed_,
k_solve_lookup_ecc_mixed_) and everything downstream of a plan, against the
plain-integer model of tests/solve_lookup_ref.py, the composer's own values and
the oracle's proof bytes.  Every comparison is exact.

A plan is compared through pnp_solve_info (defined variables, levels, the
widest level), pnp_solve_gate_entries, pnp_solve_ecc_entries and
pnp_solve_lookup_entries (the variables lookup rows define, the indexed table
rows).  The index itself is not exposed: which rows share a bucket is asserted
on the model's restatement of the hash (solve_lookup_ref.buckets_of), and the
device is held to the answers."""
import ctypes

import numpy as np
import pytest

from circuits import R_MOD
from lookup_circuits import domain_of
from pnp import abi
from solve_ecc_ref import FIXED_ADD, VAR_ADD
from solve_gates_ref import LOGIC, RANGE
from solve_lookup_ref import LOOKUP, buckets_of, indexed_rows, n_buckets, plan, plan_sweep, solve
from solve_ref import merkle_inputs
from test_gpu_solve import NONE, PNP_E_ARG, context_for, info_tuple, mont, solve_gpu
from test_gpu_solve_ecc import load_ecc
from test_solve_lookup_ref import (chain, computed_operands, duplicate_keys, every_row_query, four_segments,
                                   last_row_lookup, mixed_ops, no_such_key, tie_lookup_and_arith, tie_on_one_row,
                                   wide_lookups, zero_d)

pytestmark = pytest.mark.gpu

ECC = FIXED_ADD | VAR_ADD
GATES = RANGE | LOGIC
PNP_E_NOKEY = -3
KIND_LOOKUP = abi.CHECK_KINDS.index("lookup")


def load_lookup(ctx, ids, lk=LOOKUP, ecc=0, gates=0, rows=()):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    return ctx.load_solve_plan_lookup(ids.ctypes.data if len(ids) else 0, len(ids),
                                      rows.ctypes.data if len(rows) else 0, len(rows), gates, ecc, lk, False)


def model(cp, ids, lk=LOOKUP, ecc=0, gates=0, outputs=(), vals=None, sweep=True):
    """(plan, solution) of the model from the values cp holds (or `vals`) for ids."""
    n_vars = len(cp.vals)
    pl = (plan_sweep if sweep else plan)(cp.rows, n_vars, ids, outputs, gates, ecc, lk)
    vals = cp.vals if vals is None else vals
    return pl, solve(cp.rows, pl, n_vars, {u: vals[u] for u in ids}, None, outputs, cp.table, domain_of(cp))


def plan_matches(ctx, cp, info, ids, pl):
    assert info_tuple(info) == (len(ids), pl.n_solved, len(pl.levels), pl.max_width, 0, NONE)
    assert ctx.solve_gate_entries() == (pl.n_range, pl.n_logic)
    assert ctx.solve_ecc_entries() == (pl.n_fixed, pl.n_var)
    m = len(indexed_rows(cp.table, domain_of(cp))) if pl.n_lookup else 0
    assert ctx.solve_lookup_entries() == (pl.n_lookup, m)


def run(cp, ids, lk=LOOKUP, ecc=0, gates=0, vals=None, sweep=True, check=True):
    """Plan and solve on the GPU against the model; returns (plan, the model's solution)."""
    pl, want = model(cp, ids, lk, ecc, gates, vals=vals, sweep=sweep)
    ctx = context_for(cp)
    try:
        rc, info = load_lookup(ctx, ids, lk, ecc, gates)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, cp, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals if vals is None else vals, ids, False), mont(want))
        if check:
            ok, rep = ctx.check_solved([])
            assert ok and rep.violations == 0, ctx.last_error()
    finally:
        ctx.close()
    return pl, want


# ------------------------------------------------------------------ 1. computed operands
def test_a_lookup_of_computed_operands_solves_checks_and_proves():
    cp, ids, (p, q, u, x, y, z, w), r = computed_operands()
    inp = cp.build(min_lg=8)
    assert inp.n == 256 == domain_of(cp) and len(cp.table) == 256
    exp = abi.proof_to_bytes(inp.oracle_proof())
    pl, vals = model(cp, ids)
    assert vals == cp.vals and pl.undetermined == [] and pl.lookup_widths == [0, 1, 0]
    ctx = context_for(cp, inp)
    try:
        rc, info = load_lookup(ctx, ids)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, cp, info, ids, pl)
        assert ctx.solve_lookup_entries() == (1, 256)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
        assert list(dict(ctx.stage_times())) == ["solve_inputs", "solve_levels", "inputs_h2d_bytes"]
        ok, rep = ctx.check_solved([])
        assert ok and rep.violations == 0, ctx.last_error()
        assert abi.proof_to_bytes(ctx.prove_solved([])) == exp
        # other inputs over the same plan: 3 ^ 15, 0 ^ 1, 15 ^ 15
        for vp_, vq, vu in ((1, 2, 7), (0, 0, 0), (8, 7, 7)):
            other = list(cp.vals)
            other[p], other[q], other[u] = vp_, vq, vu
            _, want = model(cp, ids, vals=other)
            assert want[z] == (vp_ + vq) ^ (2 * vu + 1) and want[w] == want[z] + vp_
            assert np.array_equal(solve_gpu(ctx, other, ids, False), mont(want))
            assert ctx.check_solved([])[0], ctx.last_error()
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. every row of a table
def test_every_row_of_a_random_table_as_a_query():
    cp, ids, out = every_row_query()
    D = domain_of(cp)
    bk = buckets_of(cp.table, D)
    # 200 rows over 512 buckets of a fixed hash: some bucket holds several rows, each in table order
    assert D == 256 and n_buckets(200) == 512 and max(len(v) for v in bk.values()) >= 2
    pl, vals = run(cp, ids)
    assert pl.lookup_widths == [200] and [vals[c] for c in out] == [t[2] for t in cp.table]
    assert vals[out[0]] == cp.table[0][2]  # row 0's key: its own value, whatever the padded copies say


# ------------------------------------------------------------------ 3. duplicate keys
@pytest.mark.parametrize("row_0", [False, True], ids=["rows_2_5", "rows_0_3"])
def test_of_two_rows_with_one_key_the_lower_defines(row_0):
    cp, ids, out, (lo, hi) = duplicate_keys(row_0)
    pl, vals = run(cp, ids)
    assert vals[out[lo]] == vals[out[hi]] == cp.table[lo][2] != cp.table[hi][2]


# ------------------------------------------------------------------ 4. no such key
def test_a_key_the_table_does_not_hold_is_solved_to_zero_and_the_check_names_the_row():
    cp, ids, (p, q, b, a, z), r = no_such_key()
    other = list(cp.vals)
    other[p], other[q] = 2, 2
    pl, want = model(cp, ids, vals=other)
    assert want[a] == 4 and want[z] == 0
    ctx = context_for(cp)
    try:
        rc, info = load_lookup(ctx, ids)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, cp, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, other, ids, False), mont(want))  # (a failing solve raises)
        ok, rep = ctx.check_solved([])
        assert not ok and (rep.first_row, rep.first_kind, rep.first_index) == (r, KIND_LOOKUP, 0)
        assert f"row {r}: lookup constraint 0" in ctx.last_error()
        # the right inputs over the same plan
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
        ok, rep = ctx.check_solved([])
        assert ok and rep.violations == 0, ctx.last_error()
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. d
def test_d_left_to_the_zero_variable():
    cp, ids, out = zero_d()
    pl, vals = run(cp, ids)
    assert [vals[c] for _, _, c in out] == [0, 2, 3, 1] and all(cp.rows[i][1][3] == 0 for i in range(4))


def test_column_3_of_a_mixed_table_selects_the_operation():
    cp, ids, out = mixed_ops()
    pl, vals = run(cp, ids)
    assert {d: vals[c] for d, c in out.items()} == {0: 1, 1: 2, R_MOD - 1: 1, 2: 2}
    assert pl.lookup_widths == [1, 3]  # d = 0 at once, the others after their constants


# ------------------------------------------------------------------ 6. width
def test_a_wide_level_of_lookups():
    cp, ids = wide_lookups()
    assert domain_of(cp) == 512
    pl, vals = run(cp, ids, sweep=False)
    assert pl.lookup_widths == [300] and vals == cp.vals


def test_a_level_wide_only_by_the_four_segments_together():
    cp, ids = four_segments()
    pl, vals = run(cp, ids, LOOKUP, ECC, RANGE, sweep=False)
    assert (pl.arith_widths, pl.gate_widths, pl.ecc_widths, pl.lookup_widths) == ([100], [100], [300], [100])
    assert vals == cp.vals


@pytest.mark.parametrize("others,ecc,gates", [("", 0, 0), ("gates", 0, RANGE), ("ecc", ECC, RANGE)],
                         ids=["alone", "with_gate_entries", "with_gate_and_ecc_entries"])
def test_a_chain_of_40_dependent_lookups(others, ecc, gates):
    cp, ids, z = chain(others)
    pl, vals = run(cp, ids, LOOKUP, ecc, gates, sweep=False)
    assert pl.n_lookup == 40 and pl.lookup_widths[:40] == [1] * 40 and pl.max_width <= 256  # one workgroup
    assert vals == cp.vals
    if others:
        assert pl.n_range and any(k and g for k, g in zip(pl.lookup_widths, pl.gate_widths))
    if others == "ecc":
        assert pl.n_fixed and pl.n_var == 3 and any(k and e for k, e in zip(pl.lookup_widths, pl.ecc_widths))


# ------------------------------------------------------------------ 7. ties and known slots
@pytest.mark.parametrize("arith_first", [True, False], ids=["arith_lower", "lookup_lower"])
def test_tie_between_an_arithmetic_and_a_lookup_row_goes_to_the_lower_row(arith_first):
    cp, ids, (a, b, c), (ra, rl) = tie_lookup_and_arith(arith_first)
    other = list(cp.vals)
    other[b] = 1  # a + 2 = 3, a ^ b = 0: the rows disagree, the check is not asked
    pl, vals = run(cp, ids, vals=other, check=False)
    assert vals[c] == (3 if arith_first else 0) and pl.n_lookup == (0 if arith_first else 1)
    run(cp, ids)


def test_tie_on_one_row_goes_to_the_arithmetic_slot():
    cp, ids, (a, b, c), r = tie_on_one_row()
    other = list(cp.vals)
    other[b] = 1
    pl, vals = run(cp, ids, vals=other, check=False)
    assert vals[c] == 3 and pl.n_lookup == 0 and pl.n_solved == 1
    run(cp, ids)


def test_a_slot_c_listed_as_input_keeps_its_value_and_the_check_names_the_row():
    cp, ids, (p, q, u, x, y, z, w), r = computed_operands()
    given = list(cp.vals)
    given[z] = 9
    pl, want = model(cp, ids + [z], vals=given)
    assert want[z] == 9 and pl.n_lookup == 0
    ctx = context_for(cp)
    try:
        rc, info = load_lookup(ctx, ids + [z])
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, cp, info, ids + [z], pl)
        assert np.array_equal(solve_gpu(ctx, given, ids + [z], False), mont(want))
        ok, rep = ctx.check_solved([])
        assert not ok and (rep.first_row, rep.first_kind, rep.first_index) == (r, KIND_LOOKUP, 0)
        assert f"row {r}: lookup constraint 0" in ctx.last_error()
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids + [z], False), mont(cp.vals))  # the right value: clean
        assert ctx.check_solved([])[0]
    finally:
        ctx.close()


def test_the_last_gate_row_takes_part():
    cp, ids, out = last_row_lookup()
    assert len(cp.rows) == domain_of(cp) == 4
    pl, vals = run(cp, ids, check=False)
    assert pl.lookup_widths == [4] and [vals[c] for c in out] == [0, 1, 1, 0]


# ------------------------------------------------------------------ 8. the flag
def test_lookup_variables_are_undetermined_without_the_flag_and_solved_with_it():
    cp, ids, (p, q, u, x, y, z, w), r = computed_operands()
    pl, vals = model(cp, ids)
    none, _ = model(cp, ids, 0)
    assert none.undetermined == [z, w]
    pair = (ctypes.c_uint64 * 2)()
    ctx = context_for(cp)
    try:
        assert ctx.lib.pnp_solve_lookup_entries(ctx.h, ctypes.byref(pair)) == PNP_E_NOKEY  # before any plan
        for how in ("ecc", 0):
            rc, info = load_ecc(ctx, ids, ECC, GATES) if how == "ecc" else load_lookup(ctx, ids, 0, ECC, GATES)
            assert rc == PNP_E_ARG
            assert info_tuple(info) == (len(ids), none.n_solved, len(none.levels), none.max_width, 2, z)
            assert f"variable {z} " in ctx.last_error()
            assert ctx.lib.pnp_solve_lookup_entries(ctx.h, ctypes.byref(pair)) == PNP_E_NOKEY
        rc, info = load_lookup(ctx, ids)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, cp, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
    finally:
        ctx.close()


def test_bad_bits_are_refused_and_a_plan_without_lookup_entries_is_the_ecc_plan():
    cp, ids, (p, q, u, x, y, z, w), r = computed_operands()
    full = ids + [z]
    ctx = context_for(cp)
    try:
        before = ctx.hbm_usage()["live"]
        rc, plain = load_ecc(ctx, full, ECC, GATES)
        assert rc == 0, ctx.last_error()
        live = ctx.hbm_usage()["live"]
        assert live == before + plain.plan_bytes
        # bad lookup bits: refused before anything resident is dropped; ecc and gates as before
        for bad in (2, 1 << 31, LOOKUP | 2):
            rc, info = load_lookup(ctx, full, bad, ECC, GATES)
            assert rc == PNP_E_ARG and "lookup" in ctx.last_error()
        rc, info = load_lookup(ctx, full, LOOKUP, 4, GATES)
        assert rc == PNP_E_ARG and "ecc" in ctx.last_error()
        rc, info = load_lookup(ctx, full, LOOKUP, ECC, 4)
        assert rc == PNP_E_ARG and "gates" in ctx.last_error()
        assert ctx.hbm_usage()["live"] == live and ctx.solve_lookup_entries() == (0, 0)
        # the lookup variable listed as input: the flag changes nothing, and no index is built
        for lk in (0, LOOKUP):
            rc, same = load_lookup(ctx, full, lk, ECC, GATES)
            assert rc == 0 and bytes(same) == bytes(plain) and ctx.solve_lookup_entries() == (0, 0)
            assert ctx.hbm_usage()["live"] == live
    finally:
        ctx.close()


def test_a_key_without_q_lookup_accepts_the_flag():
    from test_solve_ecc_ref import scalar_mul
    cp, ids, s, res = scalar_mul(46, 170, 8)
    ctx = context_for(cp)
    try:
        rc, plain = load_ecc(ctx, ids, FIXED_ADD)
        assert rc == 0, ctx.last_error()
        rc, same = load_lookup(ctx, ids, LOOKUP, FIXED_ADD)
        assert rc == 0 and bytes(same) == bytes(plain) and ctx.solve_lookup_entries() == (0, 0)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 9. lifecycle
def test_lifecycle_accounting_and_drop():
    import pnp
    from test_gpu_assignment import host_cols
    from test_preprocess_ref import wire_map
    cp, ids, (p, q, u, x, y, z, w), r = computed_operands()
    n_vars = len(cp.vals)
    pl, vals = model(cp, ids)
    m, B, L = 256, 512, len(pl.levels)
    assert len(indexed_rows(cp.table, domain_of(cp))) == m and n_buckets(m) == B
    pair = (ctypes.c_uint64 * 2)()
    ctx = context_for(cp)
    try:
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.solve_lookup_entries()
        before = ctx.hbm_usage()["live"]
        rc, plain = load_lookup(ctx, ids + [z], LOOKUP)  # (nothing left for the rule to define)
        assert rc == 0 and ctx.hbm_usage()["live"] == before + plain.plan_bytes
        # the lookup plan: 16 B an entry, 4 B an indexed row, 4 (B + 1) B of offsets, the level offsets
        rc, info = load_lookup(ctx, ids)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, cp, info, ids, pl)
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes
        grown = 16 * 1 + 4 * m + 4 * (B + 1) + 4 * (L + 1)
        assert info.plan_bytes >= plain.plan_bytes - 4 - 16 + grown  # (one input id fewer)
        assert info.plan_bytes <= plain.plan_bytes + grown + 4 * 16 + 4 * (L - plain.n_levels + 4)
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):  # a plan, no solution yet
            ctx.assignment_ptr()
        first = solve_gpu(ctx, cp.vals, ids, False)
        assert np.array_equal(first, mont(vals))
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes + 32 * n_vars
        addr, n = ctx.assignment_ptr()
        assert n == n_vars and ctx.check_assignment(addr, n, True, sorted(cp.pis.items()))[0]
        # the same build and solve again: the same info and solution
        rc, again = load_lookup(ctx, ids)
        assert rc == 0 and bytes(again) == bytes(info) and ctx.hbm_usage()["live"] == before + info.plan_bytes
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), first)
        # a plan without lookup entries replaces it, and the entries and the index go
        rc, back = load_lookup(ctx, ids + [z], LOOKUP)
        assert rc == 0 and bytes(back) == bytes(plain)
        assert ctx.hbm_usage()["live"] == before + plain.plan_bytes and ctx.solve_lookup_entries() == (0, 0)
        # whatever replaces the wire map drops the plan, the index and the solution
        assert load_lookup(ctx, ids)[0] == 0
        solve_gpu(ctx, cp.vals, ids, False)
        keep, addrs = host_cols(wire_map(cp))
        ctx.load_wire_map(addrs, len(cp.rows), n_vars, device_ptrs=False)
        assert ctx.hbm_usage()["live"] == before
        assert ctx.lib.pnp_solve_lookup_entries(ctx.h, ctypes.byref(pair)) == PNP_E_NOKEY
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.check_solved([])
        # and a plan over the reloaded map solves as before
        assert load_lookup(ctx, ids)[0] == 0
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), first)
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
        rc, _ = load_lookup(ctx, merkle_inputs(cp), LOOKUP, ECC, GATES, [len(cp.rows) - 1])
        assert rc == PNP_E_ARG and "ranks" in ctx.last_error()
    finally:
        ctx.close()
