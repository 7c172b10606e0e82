"""Range and logic rows that define, on the MI355X: pnp_load_solve_plan_gates
(the plan build of csrc/solve.hip with the two gate families), the gate entries
of pnp_solve_assignment (k_solve_gate_wide_, k_solve_mixed_) and everything
downstream of a plan, against the plain-integer model of
tests/solve_gates_ref.py, the composer's own values and the oracle's proof
bytes.  Every comparison is exact.

The plan's per-level widths are not part of the interface: a plan is compared
through pnp_solve_info (entries, levels, the widest level) and
pnp_solve_gate_entries (entries by family)."""
import ctypes
import functools

import numpy as np
import pytest

from circuits import Composer, R_MOD
from gate_circuits import M1, logic_of, range_of
from pnp import abi
from solve_gates_ref import LOGIC, RANGE, plan, plan_sweep, solve
from solve_outputs_ref import derive
from solve_ref import merkle_inputs
from test_assignment_ref import assignment_values
from test_gpu_solve import NONE, PNP_E_ARG, context_for, info_tuple, mont, solve_gpu
from test_solve_gates_ref import (tie_arith_and_range, tie_d_next, tie_same_row_families, tie_two_slots)

pytestmark = pytest.mark.gpu

BOTH = RANGE | LOGIC
PNP_E_NOKEY = -3
KIND_RANGE, KIND_LOGIC = abi.CHECK_KINDS.index("range"), abi.CHECK_KINDS.index("logic")


def load_gates(ctx, ids, gates, rows=()):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    return ctx.load_solve_plan_gates(ids.ctypes.data if len(ids) else 0, len(ids),
                                     rows.ctypes.data if len(rows) else 0, len(rows), gates, False)


def model(cp, ids, gates, outputs=(), vals=None, sweep=True):
    """(plan, solution) of the model from the values cp holds (or `vals`) for ids."""
    n_vars = len(cp.vals)
    pl = (plan_sweep if sweep else plan)(cp.rows, n_vars, ids, outputs, gates)
    vals = cp.vals if vals is None else vals
    return pl, solve(cp.rows, pl, n_vars, {u: vals[u] for u in ids}, None, outputs)


def plan_matches(ctx, info, ids, pl):
    assert info_tuple(info) == (len(ids), pl.n_solved, len(pl.levels), pl.max_width, 0, NONE)
    assert ctx.solve_gate_entries() == (pl.n_range, pl.n_logic)


# ------------------------------------------------------------------ 1. range of a computed value
def test_range_of_a_computed_value_solves_checks_and_proves():
    cp = Composer(31)
    p, q = cp.var(int(cp.rng.integers(1 << 61, 1 << 62))), cp.var(int(cp.rng.integers(1 << 61, 1 << 62)))
    x = cp.var(cp.vals[p] + cp.vals[q])
    cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, p, q, x, 0)
    first, accs = range_of(cp, x, 64)
    ids = [0, p, q]
    inp = cp.build(min_lg=6)
    assert inp.n == 64
    exp = abi.proof_to_bytes(inp.oracle_proof())
    pl, vals = model(cp, ids, RANGE)
    assert vals == cp.vals and pl.undetermined == []
    # x, the last accumulator (assert_equal), then the eight range rows upwards
    assert pl.widths == [1, 1] + [4] * 7 + [3] and pl.gate_widths == [0, 0] + [4] * 7 + [3]
    ctx = context_for(cp, inp)
    try:
        rc, info = load_gates(ctx, ids, RANGE)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert ctx.solve_gate_entries() == (31, 0)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
        assert list(dict(ctx.stage_times())) == ["solve_inputs", "solve_levels", "inputs_h2d_bytes"]
        ok, rep = ctx.check_solved([])
        assert ok and rep.violations == 0, ctx.last_error()
        assert abi.proof_to_bytes(ctx.prove_solved([])) == exp
        # other inputs over the same plan
        other = list(cp.vals)
        other[p], other[q] = 12345, (1 << 63) + 99
        _, want = model(cp, ids, RANGE, vals=other)
        assert want[x] == 12345 + (1 << 63) + 99 and want[accs[-2]] == want[x] >> 2
        assert np.array_equal(solve_gpu(ctx, other, ids, False), mont(want))
        assert ctx.check_solved([])[0]
        # the same plan again, and BOTH flags where the key has no logic rows
        rc, again = load_gates(ctx, ids, BOTH)
        assert rc == 0 and bytes(again) == bytes(info) and ctx.solve_gate_entries() == (31, 0)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. limb crossings
def big(cp):
    while True:
        v = cp.rnd()
        if v >= 1 << 250:
            return v


def test_shifts_across_every_limb_boundary():
    """A 256-bit range chain and 254-bit XOR / AND chains over values in
    [2^250, r): every shift of 2..8 bits meets the 64, 128 and 192-bit
    boundaries somewhere along a chain."""
    cp = Composer(32)
    x, a, b = cp.var(big(cp)), cp.var(big(cp)), cp.var(big(cp))
    first, accs = range_of(cp, x, 256)
    assert len(cp.rows) - first == 32 + 2
    logic_of(cp, a, b, 254, True)
    logic_of(cp, a, b, 254, False)
    ids = [0, x, a, b]
    pl, vals = model(cp, ids, BOTH)
    assert pl.undetermined == [] and vals == cp.vals
    assert pl.n_range == 127 and pl.n_logic == 2 * (5 + 125 * 4 + 1)
    ctx = context_for(cp)
    try:
        rc, info = load_gates(ctx, ids, BOTH)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(vals))
        # the all-ones pattern below r, and the smallest values
        for vx, va, vb in ((R_MOD - 1, R_MOD - 2, (1 << 254) - 1), (0, 1, 3)):
            other = list(cp.vals)
            other[x], other[a], other[b] = vx, va, vb
            _, want = model(cp, ids, BOTH, vals=other)
            assert np.array_equal(solve_gpu(ctx, other, ids, False), mont(want))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. an XOR that reaches r
def test_xor_reaching_r_is_reduced_and_the_check_names_the_row():
    A, B = 1 << 254, (1 << 253) + (1 << 252) + (1 << 251)
    assert A < R_MOD and B < R_MOD and A ^ B >= R_MOD
    cp = Composer(33)
    a, b = cp.var(A), cp.var(B)
    d = cp.var((A ^ B) - R_MOD)
    cp.row({"q_arith": 1, "q_l": 1}, 0, 0, 0, 0)
    r = cp.row({"logic_selector": M1, "q_c": M1}, 0, 0, 0, 0)
    cp.row({}, a, b, 0, d)
    ids = [0, a, b]
    pl, vals = model(cp, ids, LOGIC)
    assert vals == cp.vals and [len(l) for l in pl.levels] == [1]
    ctx = context_for(cp)
    try:
        rc, info = load_gates(ctx, ids, LOGIC)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(vals))  # (a failing solve raises)
        ok, rep = ctx.check_solved([])
        assert not ok and rep.first_row == r and rep.first_kind == KIND_LOGIC and rep.by_kind[KIND_LOGIC] >= 1
        assert rep.violations == rep.by_kind[KIND_LOGIC]
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. logic into arithmetic into an output row
@pytest.mark.parametrize("xor", [False, True], ids=["and", "xor"])
def test_logic_feeds_arithmetic_and_an_output_row(xor):
    cp = Composer(34)
    a, b = cp.var(int(cp.rng.integers(0, 1 << 62))), cp.var(int(cp.rng.integers(0, 1 << 62)))
    _, res = logic_of(cp, a, b, 62, xor)
    w = cp.var(3 * cp.vals[res] + 1)
    cp.row({"q_arith": 1, "q_l": 3, "q_c": 1, "q_o": M1}, res, 0, w, 0)
    out = cp.row({"q_arith": 1, "q_l": 1}, w, 0, 0, 0)
    cp.pis[out] = -cp.vals[w] % R_MOD
    ids = [0, a, b]
    inp = cp.build(min_lg=6)
    exp = abi.proof_to_bytes(inp.oracle_proof())
    pl, vals = model(cp, ids, LOGIC, [out])
    assert vals == cp.vals and derive(cp.rows, vals, [out]) == cp.pis
    assert cp.vals[res] == (cp.vals[a] ^ cp.vals[b] if xor else cp.vals[a] & cp.vals[b])
    ctx = context_for(cp, inp)
    try:
        rc, info = load_gates(ctx, ids, LOGIC, [out])
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


# ------------------------------------------------------------------ 5. wide and narrow paths
@functools.lru_cache(maxsize=None)
def wide_and_narrow():
    """300 one-row range chains over 300 inputs and 300 rows y = 5 x + 7: the
    first level holds 300 arithmetic and 1200 gate entries (a launch each).  A
    33-row chain of a 256-bit value and a chain z -> z + 1 of 40 rows: levels of
    four gate entries and one arithmetic entry in one narrow run, then
    arithmetic entries alone."""
    cp = Composer(35)
    ids = [0]
    for _ in range(300):
        v = cp.var(int(cp.rng.integers(0, 1 << 62)))
        acc = [cp.var(cp.vals[v] >> s) for s in (2, 4, 6, 8)]
        cp.row({"range_selector": 1}, *acc)
        cp.row({}, 0, 0, 0, v)
        x = cp.var(cp.rnd())
        cp.row({"q_arith": 1, "q_l": 5, "q_c": 7, "q_r": M1}, x, cp.var(5 * cp.vals[x] + 7), 0, 0)
        ids += [v, x]
    big_x = cp.var(big(cp))
    first, _ = range_of(cp, big_x, 264)
    assert len(cp.rows) - first == 33 + 2
    z = cp.var(cp.rnd())
    ids += [big_x, z]
    for _ in range(40):
        nz = cp.var(cp.vals[z] + 1)
        cp.row({"q_arith": 1, "q_l": 1, "q_c": 1, "q_o": M1}, z, 0, nz, 0)
        z = nz
    assert len(cp.rows) < 1024
    pl, vals = model(cp, ids, RANGE, sweep=False)
    return cp, ids, pl, vals


def test_wide_levels_narrow_runs_and_levels_of_both_kinds():
    cp, ids, pl, vals = wide_and_narrow()
    assert vals == cp.vals and pl.undetermined == []
    assert (pl.arith_widths[0], pl.gate_widths[0]) == (302, 1200)  # (the last accumulator and z + 1 too)
    assert all(w <= 256 for w in pl.widths[1:])
    assert (pl.arith_widths[1], pl.gate_widths[1]) == (1, 4) and pl.gate_widths[34:] == [0] * 6 and len(pl.levels) == 40
    ctx = context_for(cp)
    try:
        rc, info = load_gates(ctx, ids, RANGE)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(vals))
        assert ctx.check_solved([])[0]
    finally:
        ctx.close()


def test_a_level_wide_only_by_both_segments_together():
    """150 arithmetic and 4 x 40 gate entries in one level: neither segment is wider than a workgroup, the level is."""
    cp = Composer(36)
    ids = [0]
    for k in range(150):
        x = cp.var(cp.rnd())
        cp.row({"q_arith": 1, "q_l": 5, "q_c": 7, "q_r": M1}, x, cp.var(5 * cp.vals[x] + 7), 0, 0)
        ids.append(x)
        if k < 40:
            v = cp.var(big(cp))
            cp.row({"range_selector": 1}, *(cp.var(cp.vals[v] >> s) for s in (2, 4, 6, 8)))
            cp.row({}, 0, 0, 0, v)
            ids.append(v)
    pl, vals = model(cp, ids, RANGE)
    assert vals == cp.vals and (pl.arith_widths, pl.gate_widths) == ([150], [160])
    ctx = context_for(cp)
    try:
        rc, info = load_gates(ctx, ids, RANGE)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(vals))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6. opt-in, and equivalence without gate rows
def test_a_range_variable_is_undetermined_without_the_flag_and_solved_with_it():
    from test_gpu_solve import stuck_circuit
    cp, inp, exp, bad = stuck_circuit()
    n_vars = len(cp.vals)
    u = bad["only_in_a_range_row"]
    ids = [v for v in range(n_vars) if v != u]
    ctx = context_for(cp, inp)
    try:
        for gates in (0, LOGIC):
            rc, info = load_gates(ctx, ids, gates)
            assert rc == PNP_E_ARG and info_tuple(info) == (n_vars - 1, 0, 0, 0, 1, u)
            assert f"variable {u} " in ctx.last_error()
            assert ctx.lib.pnp_solve_gate_entries(ctx.h, ctypes.byref((ctypes.c_uint64 * 2)())) == PNP_E_NOKEY
        rc, info = load_gates(ctx, ids, RANGE)
        assert rc == 0 and info_tuple(info) == (n_vars - 1, 1, 1, 1, 0, NONE), ctx.last_error()
        assert ctx.solve_gate_entries() == (1, 0)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), assignment_values(cp))
        from test_general import pis_of
        assert abi.proof_to_bytes(ctx.prove_solved(pis_of(inp))) == exp
    finally:
        ctx.close()


def test_an_arithmetic_circuit_gets_the_same_plan_whatever_the_flags():
    import merkle_circuit as mc
    from test_gpu_solve_outputs import load_plan
    cp = mc.merkle_circuit(4, seed=11)[0]
    ids = merkle_inputs(cp)
    root_row = len(cp.rows) - 1
    ctx = context_for(cp)
    try:
        before = ctx.hbm_usage()["live"]
        seen = []
        for how in ("plan", 0, BOTH):
            rc, info = load_plan(ctx, ids, [root_row]) if how == "plan" else load_gates(ctx, ids, how, [root_row])
            assert rc == 0, ctx.last_error()
            assert ctx.hbm_usage()["live"] == before + info.plan_bytes
            assert ctx.solve_gate_entries() == (0, 0)
            sol = solve_gpu(ctx, cp.vals, ids, False)
            seen.append((bytes(info), sol.tobytes(), ctx.solved_public_inputs()))
        assert seen[0] == seen[1] == seen[2]
        assert np.array_equal(np.frombuffer(seen[0][1], dtype=np.uint64).reshape(-1, 4), assignment_values(cp))
        assert seen[0][2] == sorted(cp.pis.items())
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7. ties
def run_tie(cp, ids, gates):
    pl, vals = model(cp, ids, gates)
    ctx = context_for(cp)
    try:
        rc, info = load_gates(ctx, ids, gates)
        assert rc == 0, ctx.last_error()
        plan_matches(ctx, info, ids, pl)
        return pl, vals, solve_gpu(ctx, cp.vals, ids, False)
    finally:
        ctx.close()


@pytest.mark.parametrize("arith_first", [True, False], ids=["arith_lower", "range_lower"])
def test_tie_between_an_arithmetic_and_a_range_row_goes_to_the_lower_row(arith_first):
    cp, ids, u, ra, rr = tie_arith_and_range(arith_first)
    pl, vals, got = run_tie(cp, ids, RANGE)
    assert (pl.n_solved - pl.n_range, pl.n_range) == ((1, 0) if arith_first else (0, 1))
    assert vals[u] == ((cp.vals[ids[1]] + 1) % R_MOD if arith_first else 0x1234567 >> 6)
    assert np.array_equal(got, mont(vals))


def test_tie_between_two_slots_of_one_range_row_goes_to_the_lower_role():
    cp, ids, u, r = tie_two_slots()
    pl, vals, got = run_tie(cp, ids, RANGE)
    assert vals[u] == 0xabcdef >> 2 and pl.n_range == 1
    assert np.array_equal(got, mont(vals))


def test_tie_on_one_row_goes_to_the_arithmetic_role():
    cp, ids, u, r = tie_same_row_families()
    pl, vals, got = run_tie(cp, ids, RANGE)
    assert vals[u] == (cp.vals[ids[1]] + 1) % R_MOD and pl.n_range == 0
    assert np.array_equal(got, mont(vals))


def test_tie_d_next_bids_as_the_logic_row_itself():
    cp, ids, u, r = tie_d_next()
    pl, vals, got = run_tie(cp, ids, LOGIC)
    assert vals[u] == 0b1101 & 0b0111 and pl.n_logic == 1
    assert np.array_equal(got, mont(vals))
    pl, vals, got = run_tie(cp, ids, RANGE)  # (no logic rule: the arithmetic row of the next row)
    assert vals[u] == 0b1101 + 0b0111 and np.array_equal(got, mont(vals))


# ------------------------------------------------------------------ 8. never ready, never redefined
def test_a_range_row_without_a_next_row_and_a_logic_row_with_another_q_c_define_nothing():
    cp = Composer(37)
    v = cp.var(77)
    lo, u = cp.var(0), cp.var(0)
    cp.row({}, 0, 0, 0, v)
    cp.row({"range_selector": 1}, u, lo, 0, 0)  # the last gate: no next row
    ctx = context_for(cp)
    try:
        rc, info = load_gates(ctx, [0, v], BOTH)
        assert rc == PNP_E_ARG and info_tuple(info) == (2, 0, 0, 0, 2, lo)
        assert f"variable {lo} " in ctx.last_error()
    finally:
        ctx.close()
    cp = Composer(38)
    a, b = cp.var(5), cp.var(6)
    lo, u = cp.var(0), cp.var(0)
    cp.row({"logic_selector": 1, "q_c": 2}, u, lo, 0, 0)
    cp.row({}, a, b, 0, 0)
    assert plan_sweep(cp.rows, len(cp.vals), [0, a, b], (), BOTH).undetermined == [lo, u]
    ctx = context_for(cp)
    try:
        rc, info = load_gates(ctx, [0, a, b], BOTH)
        assert rc == PNP_E_ARG and info_tuple(info) == (3, 0, 0, 0, 2, lo)
        assert f"variable {lo} " in ctx.last_error()
        rc, info = load_gates(ctx, [0, a, b, lo, u], BOTH)  # as inputs they are fine
        assert rc == 0 and info.n_solved == 0 and ctx.solve_gate_entries() == (0, 0)
    finally:
        ctx.close()


def test_a_known_variable_in_a_range_slot_keeps_its_value_and_the_check_names_the_row():
    cp = Composer(39)
    cp.row({"q_arith": 1, "q_l": 1}, 0, 0, 0, 0)
    cp.range_chain(2)
    last = cp.rows[-1][1][3]
    wrong = cp.rows[2][1][1]  # slot b of the second range row
    ids = [0, last, wrong]
    given = list(cp.vals)
    given[wrong] = (cp.vals[wrong] + 1) % R_MOD
    pl, vals = model(cp, ids, RANGE, vals=given)
    assert vals[wrong] == given[wrong] and [v for k, v in enumerate(vals) if k != wrong] == \
        [v for k, v in enumerate(cp.vals) if k != wrong]
    ctx = context_for(cp)
    try:
        rc, info = load_gates(ctx, ids, RANGE)
        assert rc == 0 and ctx.solve_gate_entries() == (7, 0), ctx.last_error()
        assert np.array_equal(solve_gpu(ctx, given, ids, False), mont(vals))
        ok, rep = ctx.check_solved([])
        assert not ok and rep.first_row == 2 and rep.first_kind == KIND_RANGE
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))  # the right value: clean
        assert ctx.check_solved([])[0]
    finally:
        ctx.close()


# ------------------------------------------------------------------ 9. lifecycle
def test_lifecycle_accounting_flags_and_drop():
    import pnp
    from test_gpu_assignment import host_cols
    from test_preprocess_ref import wire_map
    cp, ids, pl, vals = wide_and_narrow()
    n_vars = len(cp.vals)
    n_gate = pl.n_range + pl.n_logic
    pair = (ctypes.c_uint64 * 2)()
    ctx = context_for(cp)
    try:
        assert ctx.lib.pnp_solve_gate_entries(ctx.h, ctypes.byref(pair)) == PNP_E_NOKEY  # before any plan
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.solve_gate_entries()
        before = ctx.hbm_usage()["live"]
        # the arithmetic-only part: the gate variables as inputs
        gate_vars = sorted(u for l in pl.levels for u, _, role in l if role >= 4)
        rc, plain = load_gates(ctx, ids + gate_vars, 0)
        assert rc == 0 and plain.n_solved == pl.n_solved - n_gate, ctx.last_error()
        assert ctx.hbm_usage()["live"] == before + plain.plan_bytes
        for bad in (4, 8, BOTH | 4, 1 << 31):
            rc, info = load_gates(ctx, ids, bad)
            assert rc == PNP_E_ARG and "gates" in ctx.last_error()
        assert ctx.solve_gate_entries() == (0, 0)  # (refused before anything was dropped)
        rc, info = load_gates(ctx, ids, RANGE)
        assert rc == 0, ctx.last_error()
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes
        # 16 B an entry (padded to four entries) and the gate level offsets (4 B a level and one, padded to
        # four); the input list is shorter by the gate variables
        extra = info.plan_bytes - (plain.plan_bytes - 4 * ((len(ids) + n_gate + 3) // 4 * 4 - (len(ids) + 3) // 4 * 4))
        assert 16 * n_gate <= extra <= 16 * (n_gate + 3) + 4 * (len(pl.levels) + 1 + 3)
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):  # a plan, no solution yet
            ctx.assignment_ptr()
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(vals))
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes + 32 * n_vars
        addr, n = ctx.assignment_ptr()
        assert n == n_vars and ctx.check_assignment(addr, n, True, [])[0]
        assert ctx.assignment_values(ids=[ids[1]]) == [list(mont([cp.vals[ids[1]]])[0])]
        # a plan without gates replaces it, and its arrays go
        rc, again = load_gates(ctx, ids + gate_vars, 0)
        assert rc == 0 and bytes(again) == bytes(plain)
        assert ctx.hbm_usage()["live"] == before + plain.plan_bytes and ctx.solve_gate_entries() == (0, 0)
        # whatever replaces the wire map drops the plan and the solution
        assert load_gates(ctx, ids, RANGE)[0] == 0
        solve_gpu(ctx, cp.vals, ids, False)
        keep, addrs = host_cols(wire_map(cp))
        ctx.load_wire_map(addrs, len(cp.rows), n_vars, device_ptrs=False)
        assert ctx.hbm_usage()["live"] == before
        assert ctx.lib.pnp_solve_gate_entries(ctx.h, ctypes.byref(pair)) == PNP_E_NOKEY
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
        rc, _ = load_gates(ctx, merkle_inputs(cp), BOTH, [len(cp.rows) - 1])
        assert rc == PNP_E_ARG and "ranks" in ctx.last_error()
    finally:
        ctx.close()
