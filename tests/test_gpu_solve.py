"""The witness solver on the MI355X: pnp_load_solve_inputs (the plan, built on
the device) and pnp_solve_assignment (csrc/solve.hip, csrc/solve_witness.cpp) against the
plain-integer model of tests/solve_ref.py.  Every comparison is exact: field
elements, counts, proof bytes.

A level of more than 256 entries is one launch of 256-lane workgroups, a run of
narrower levels one launch of one workgroup: merkle4 (levels of at most 16) is
one such launch; merkle9 (49,220 rows, D = 2^16) starts 512, 385, 385, 384 wide
(multi-workgroup launches with ragged tails) and hands over to narrow runs and
back; 256 and 257 independent rows sit on either side of the threshold."""
import functools

import numpy as np
import pytest

from circuits import Composer, R_MOD
from pnp import abi
from pnp_testlib import fr_mont, ints_to_arr
from solve_ref import merkle_inputs, plan, plan_sweep, solve
from test_assignment_ref import assignment_values
from test_gpu_preprocess import Desc, dev_u32

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
PNP_E_ARG = -1


class Gates:
    """What Desc reads of a built instance, for circuits that are never proved."""

    def __init__(self, cp):
        self.n_gates = len(cp.rows)


def context_for(cp, inp=None):
    """A context with the circuit preprocessed (key and wire map resident);
    with the commit key too when there is an instance to prove."""
    import pnp
    ctx = pnp.Context(0)
    if inp is not None:
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
    desc = Desc(cp, inp or Gates(cp))
    ctx.preprocess(desc.d, device_ptrs=False)
    return ctx


def load_inputs(ctx, ids, device=False):
    arr = np.ascontiguousarray(ids, dtype=np.uint32)
    if device:
        t = dev_u32(arr)
        return ctx.load_solve_inputs(t.data_ptr(), len(arr), True)
    return ctx.load_solve_inputs(arr.ctypes.data if len(arr) else 0, len(arr), False)


def solve_gpu(ctx, cp_vals, ids, device, pis=()):
    """Solve from the values cp_vals holds for `ids`; returns the whole solution, (n_vars, 4) u64."""
    from gpu_util import to_dev
    inputs = ints_to_arr([fr_mont(cp_vals[u]) for u in ids])
    if device:
        t = to_dev(inputs)
        ctx.solve_assignment(t.data_ptr(), len(ids), True, pis)
    else:
        ctx.solve_assignment(inputs.ctypes.data, len(ids), False, pis)
    return solution(ctx, len(cp_vals))


def solution(ctx, n_vars):
    out = np.zeros((n_vars, 4), dtype=np.uint64)
    rc = ctx.lib.pnp_assignment_values(ctx.h, None, n_vars, out.ctypes.data)
    assert rc == 0, ctx.last_error()
    return out


def mont(vals):
    return ints_to_arr([fr_mont(v) for v in vals])


def info_tuple(info):
    return (info.n_inputs, info.n_solved, info.n_levels, info.max_width, info.n_undetermined, info.first_undetermined)


# ------------------------------------------------------------------ the Merkle circuit
@functools.lru_cache(maxsize=None)
def merkle(height, seed=11):
    """(composer, input ids, the model's plan), made once, never mutated."""
    import merkle_circuit as mc
    cp = mc.merkle_circuit(height, seed=seed)[0]
    ids = merkle_inputs(cp)
    return cp, ids, plan(cp.rows, len(cp.vals), ids)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("height", [4, 9])
def test_merkle_solution_equals_the_composers_values(height, device):
    cp, ids, pl = merkle(height)
    n_vars = len(cp.vals)
    if height == 4:
        assert len(pl.levels) == 194 and pl.max_width <= 16  # one launch of one workgroup
    else:
        assert (len(cp.rows), n_vars, len(ids)) == (49220, 49735, 519)
        assert len(pl.levels) == 519 and pl.widths[:4] == [512, 385, 385, 384] and min(pl.widths) == 2
    assert solve(cp.rows, pl, n_vars, {u: cp.vals[u] for u in ids}, cp.pis) == cp.vals
    pis = sorted(cp.pis.items())
    ctx = context_for(cp)
    try:
        rc, info = load_inputs(ctx, ids, device)
        assert rc == 0, ctx.last_error()
        assert info_tuple(info) == (len(ids), pl.n_solved, len(pl.levels), pl.max_width, 0, NONE)
        assert info.n_solved + info.n_inputs == n_vars and info.plan_bytes > 0
        got = solve_gpu(ctx, cp.vals, ids, device, pis)
        assert np.array_equal(got, assignment_values(cp))
        stages = dict(ctx.stage_times())
        assert list(stages) == ["solve_inputs", "solve_levels", "inputs_h2d_bytes"]
        assert stages["inputs_h2d_bytes"] == (0 if device else 32 * len(ids))
        # the solution in place satisfies the circuit
        addr, n = ctx.assignment_ptr()
        assert n == n_vars
        ok, rep = ctx.check_assignment(addr, n_vars, True, pis)
        assert ok and rep.violations == 0
        # another seed's inputs over the same plan give that seed's values
        cp2 = merkle(height, seed=23)[0]
        assert merkle(height, seed=23)[1] == ids and cp2.vals != cp.vals
        got2 = solve_gpu(ctx, cp2.vals, ids, device, sorted(cp2.pis.items()))
        assert np.array_equal(got2, assignment_values(cp2))
        # the same plan and info again
        rc, again = load_inputs(ctx, ids, device)
        assert rc == 0 and bytes(again) == bytes(info)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, device, pis), assignment_values(cp))
    finally:
        ctx.close()


def test_merkle_without_the_public_input_leaves_the_root_zero():
    """The root variable is defined by the root row (round 2) and the last
    hash's output by the root's assert_equal (round 3): PI = 0 gives both 0."""
    cp, ids, pl = merkle(4)
    exp = solve(cp.rows, pl, len(cp.vals), {u: cp.vals[u] for u in ids})
    ctx = context_for(cp)
    try:
        assert load_inputs(ctx, ids)[0] == 0
        got = solve_gpu(ctx, cp.vals, ids, False)
        assert np.array_equal(got, mont(exp))
        assert int((got != assignment_values(cp)).any(axis=1).sum()) == 2
    finally:
        ctx.close()


# ------------------------------------------------------------------ synthetic circuits
M1 = R_MOD - 1


def chain600():
    """x_(i+1) = 3 x_i^5 + i, the target in c: 600 levels one entry wide."""
    cp = Composer(3)
    x = cp.var(cp.rnd())
    ids = [0, x]
    for i in range(600):
        y = cp.var(3 * pow(cp.vals[x], 5, R_MOD) + i)
        cp.row({"q_arith": 1, "q_hl": 3, "q_c": i, "q_o": M1}, x, 0, y, 0)
        x = y
    return cp, ids


def one_level(width):
    """`width` independent rows y = 5 x + 7 (targets in b), then three rows on their results."""
    cp = Composer(width)
    ids, ys = [0], []
    for _ in range(width):
        x = cp.var(cp.rnd())
        y = cp.var(5 * cp.vals[x] + 7)
        cp.row({"q_arith": 1, "q_l": 5, "q_c": 7, "q_r": M1}, x, y, 0, 0)
        ids.append(x)
        ys.append(y)
    for k in (0, width // 2, width - 1):
        z = cp.var(cp.vals[ys[k]] * cp.vals[ys[0]])
        cp.row({"q_arith": 1, "q_m": 1, "q_o": M1}, ys[k], ys[0], z, 0)
    return cp, ids


def every_slot():
    """A target in each of a, b, c, d, q_arith = 7, every other selector in play."""
    cp = Composer(5)
    ids = [0]
    for slot in range(4):
        q = {"q_arith": 7, "q_l": cp.rnd(), "q_r": cp.rnd(), "q_o": cp.rnd(), "q_4": cp.rnd(), "q_c": cp.rnd(),
             "q_hl": cp.rnd(), "q_hr": cp.rnd(), "q_h4": cp.rnd(), "q_m": cp.rnd()}
        for k in (("q_hl", "q_m"), ("q_hr", "q_m"), (), ("q_h4",))[slot]:
            q[k] = 0
        ws = [cp.var(cp.rnd()) for _ in range(4)]
        ids += [w for j, w in enumerate(ws) if j != slot]
        a, b, c, d = (0 if j == slot else cp.vals[w] for j, w in enumerate(ws))
        s = (q["q_m"] * a * b + q["q_l"] * a + q["q_r"] * b + q["q_o"] * c + q["q_4"] * d + q["q_hl"] * pow(a, 5, R_MOD)
             + q["q_hr"] * pow(b, 5, R_MOD) + q["q_h4"] * pow(d, 5, R_MOD) + q["q_c"]) % R_MOD
        coef = q[("q_l", "q_r", "q_o", "q_4")[slot]]
        cp.vals[ws[slot]] = -s * pow(coef, -1, R_MOD) % R_MOD
        cp.row(q, *ws)
    return cp, ids


def pi_on_a_defining_row():
    """3 (2 x + 4 y) + PI = 0 defines y; a second row uses it."""
    cp = Composer(6)
    x = cp.var(cp.rnd())
    pi = cp.rnd()
    y = cp.var(-(2 * cp.vals[x] + pi * pow(3, -1, R_MOD)) * pow(4, -1, R_MOD))
    r = cp.row({"q_arith": 3, "q_l": 2, "q_4": 4}, x, 0, 0, y)
    cp.pis[r] = pi
    z = cp.var(cp.vals[y] + 1)
    cp.row({"q_arith": 1, "q_l": 1, "q_c": 1, "q_o": M1}, y, 0, z, 0)
    return cp, [0, x]


def two_rows_ready_for_one_variable():
    """Rows 1 and 2 are both ready for y in round 1 (row 0 is not: it needs z):
    the lower one defines it, the other stays a constraint that holds."""
    cp = Composer(7)
    x = cp.var(cp.rnd())
    y = cp.var(cp.vals[x] + 9)
    z = cp.var(2 * cp.vals[y])
    cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, y, y, z, 0)       # z = y + y
    cp.row({"q_arith": 1, "q_l": 2, "q_c": 18, "q_o": R_MOD - 2}, x, 0, y, 0)  # 2 y = 2 x + 18
    cp.row({"q_arith": 1, "q_l": 1, "q_c": 9, "q_o": M1}, x, 0, y, 0)       # y = x + 9
    return cp, [0, x]


def multiplication_with_c_unknown():
    cp = Composer(8)
    x, y = cp.var(cp.rnd()), cp.var(cp.rnd())
    z = cp.var(cp.vals[x] * cp.vals[y] + 11)
    cp.row({"q_arith": 1, "q_m": 1, "q_c": 11, "q_o": M1}, x, y, z, 0)
    return cp, [0, x, y]


SYNTHETIC = {"chain600": chain600, "level256": lambda: one_level(256), "level257": lambda: one_level(257),
             "every_slot": every_slot, "pi_defining": pi_on_a_defining_row,
             "lowest_wins": two_rows_ready_for_one_variable, "mul_c": multiplication_with_c_unknown}


@pytest.mark.parametrize("name", list(SYNTHETIC))
def test_synthetic_circuit_equals_the_model_and_passes_the_check(name):
    cp, ids = SYNTHETIC[name]()
    n_vars = len(cp.vals)
    pl = plan_sweep(cp.rows, n_vars, ids)
    assert pl.undetermined == []
    exp = solve(cp.rows, pl, n_vars, {u: cp.vals[u] for u in ids}, cp.pis)
    assert exp == cp.vals  # the builders' own arithmetic
    if name == "chain600":
        assert pl.widths == [1] * 600
    if name.startswith("level"):
        assert pl.widths == [int(name[5:]), 3]
    if name == "lowest_wins":
        assert pl.levels == [[(2, 1, 2)], [(3, 0, 2)]]
    if name == "every_slot":
        assert sorted(j for _, _, j in pl.levels[0]) == [0, 1, 2, 3]
    pis = sorted(cp.pis.items())
    ctx = context_for(cp)
    try:
        rc, info = load_inputs(ctx, ids)
        assert rc == 0, ctx.last_error()
        assert info_tuple(info) == (len(ids), pl.n_solved, len(pl.levels), pl.max_width, 0, NONE)
        got = solve_gpu(ctx, cp.vals, ids, False, pis)
        assert np.array_equal(got, mont(exp))
        addr, _ = ctx.assignment_ptr()
        ok, rep = ctx.check_assignment(addr, n_vars, True, pis)
        assert ok and rep.violations == 0, ctx.last_error()
        if name == "pi_defining":  # without the public input y is another value, and the check says so
            other = solve_gpu(ctx, cp.vals, ids, False)
            assert np.array_equal(other, mont(solve(cp.rows, pl, n_vars, {u: cp.vals[u] for u in ids})))
            assert not np.array_equal(other, got)
            assert not ctx.check_assignment(ctx.assignment_ptr()[0], n_vars, True, pis)[0]
    finally:
        ctx.close()


# ------------------------------------------------------------------ undetermined variables
@functools.lru_cache(maxsize=None)
def stuck_circuit():
    """(composer, instance, oracle proof, {case: variable}): four variables
    that no round can define, each for its own reason; every other variable is
    an input of the cases below."""
    cp = Composer(9)
    bad = {}
    k = cp.var(cp.rnd())
    u = cp.var(cp.rnd())
    cp.row({"q_arith": 1, "q_hl": 1, "q_o": M1}, u, 0, cp.var(pow(cp.vals[u], 5, R_MOD)), 0)
    bad["under_q_hl"] = u
    u = cp.var(cp.rnd())
    cp.row({"q_arith": 1, "q_m": 1, "q_l": 1, "q_o": M1}, u, k, cp.var(cp.vals[u] * (cp.vals[k] + 1)), 0)
    bad["in_a_with_q_m"] = u
    u = cp.var(cp.rnd())
    cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, u, u, cp.var(2 * cp.vals[u]), 0)
    bad["in_two_relevant_slots"] = u
    first = len(cp.vals)
    cp.range_chain(2)
    bad["only_in_a_range_row"] = first + 2  # wire b of the first range row
    assert cp.rows[3][0].get("range_selector") and cp.rows[3][1][1] == first + 2
    inp = cp.build()
    return cp, inp, abi.proof_to_bytes(inp.oracle_proof()), bad


@pytest.mark.parametrize("case", ["under_q_hl", "in_a_with_q_m", "in_two_relevant_slots", "only_in_a_range_row"])
def test_undetermined_variable_is_named_and_no_plan_stays(case):
    import pnp
    from test_general import pis_of
    cp, inp, exp, bad = stuck_circuit()
    n_vars = len(cp.vals)
    u = bad[case]
    ids = [v for v in range(n_vars) if v != u]
    pl = plan_sweep(cp.rows, n_vars, ids)
    assert pl.undetermined == [u] and pl.levels == []
    ctx = context_for(cp, inp)
    try:
        everything = list(range(n_vars))
        assert load_inputs(ctx, everything)[0] == 0  # a plan is resident, and solves
        assert np.array_equal(solve_gpu(ctx, cp.vals, everything, False), assignment_values(cp))
        rc, info = load_inputs(ctx, ids)
        assert rc == PNP_E_ARG
        assert info_tuple(info) == (n_vars - 1, 0, 0, 0, 1, u)
        assert f"variable {u} " in ctx.last_error()
        one = mont([0])
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY.*plan"):
            ctx.solve_assignment(one.ctypes.data, n_vars - 1, False)
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.assignment_ptr()
        assert abi.proof_to_bytes(ctx.prove_ex(inp.circuit, False, pis_of(inp))) == exp
    finally:
        ctx.close()


# ------------------------------------------------------------------ solve, read the root, prove
@pytest.mark.parametrize("kind", ["merkle4", "merkle6"])
def test_round_trip_solve_read_root_prove(kind):
    """preprocess, load inputs, solve, read the root, prove the resident
    solution with PI = -root: the oracle's proof bytes.  (The root row defines
    the root variable from the public input, so the solve is given it.)"""
    from test_general import pis_of
    from test_gpu_assignment import inst
    cp, inp, exp, var, values = inst(kind)
    ids = merkle_inputs(cp)
    n_vars = len(cp.vals)
    root_row = len(cp.rows) - 1
    root_var = cp.rows[root_row][1][0]
    assert pis_of(inp) == [(root_row, -cp.vals[root_var] % R_MOD)]
    ctx = context_for(cp, inp)
    try:
        assert load_inputs(ctx, ids)[0] == 0
        solve_gpu(ctx, cp.vals, ids, False, pis_of(inp))
        (limbs,) = ctx.assignment_values(ids=[root_var])
        root_mont = sum(int(w) << (64 * k) for k, w in enumerate(limbs))
        assert root_mont == fr_mont(cp.vals[root_var])
        root = root_mont * pow(1 << 256, -1, R_MOD) % R_MOD
        addr, n = ctx.assignment_ptr()
        got = ctx.prove_assignment(addr, n, True, [(root_row, -root % R_MOD)])
        assert abi.proof_to_bytes(got) == exp
        # proofs from the columns are what they were
        assert abi.proof_to_bytes(ctx.prove_ex(inp.circuit, False, pis_of(inp))) == exp
        # ... and the solution is still resident and whole
        assert np.array_equal(solution(ctx, n_vars), values)
    finally:
        ctx.close()


# ------------------------------------------------------------------ lifecycle
def test_lifecycle_errors_drop_and_accounting():
    import pnp
    from test_gpu_assignment import host_cols
    from test_preprocess_ref import wire_map
    cp, ids, pl = merkle(4)
    n_vars = len(cp.vals)
    pis = sorted(cp.pis.items())
    inputs = mont([cp.vals[u] for u in ids])
    ctx = context_for(cp)
    try:
        def no_plan():
            with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY.*plan"):
                ctx.solve_assignment(inputs.ctypes.data, len(ids), False, pis)
        no_plan()  # before any plan
        # the check transforms the selector rows as the plan build does: every table they need exists now
        values = assignment_values(cp)
        assert ctx.check_assignment(values.ctypes.data, n_vars, False, pis)[0]
        before = ctx.hbm_usage()["live"]
        # bad id lists: nothing resident afterwards
        for bad, what in ((ids[:-1] + [n_vars], f"input id {n_vars} is not a variable"),
                          (ids[:-1] + [ids[3]], f"input id {ids[3]} is listed twice")):
            rc, info = load_inputs(ctx, bad)
            assert rc == PNP_E_ARG and what in ctx.last_error(), ctx.last_error()
            no_plan()
            assert ctx.hbm_usage()["live"] == before
        rc, info = load_inputs(ctx, ids)
        assert rc == 0
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):  # a plan, no solution yet
            ctx.assignment_values(k=1)
        for n in (len(ids) - 1, len(ids) + 1):
            with pytest.raises(pnp.PnpError, match="PNP_E_ARG.*inputs"):
                ctx.solve_assignment(inputs.ctypes.data, n, False, pis)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False, pis), assignment_values(cp))
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes + 32 * n_vars
        assert ctx.assignment_values(k=2) == [list(r) for r in assignment_values(cp)[:2]]
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG"):
            ctx.assignment_values(ids=[n_vars])
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG"):
            ctx.assignment_values(k=n_vars + 1)
        # a second solve rewrites the same buffer
        solve_gpu(ctx, cp.vals, ids, False, pis)
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes + 32 * n_vars
        # whatever replaces the wire map drops the plan and the solution
        keep, addrs = host_cols(wire_map(cp))
        ctx.load_wire_map(addrs, len(cp.rows), n_vars, device_ptrs=False)
        no_plan()
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.assignment_ptr()
        assert ctx.hbm_usage()["live"] == before
        # ... and so does a key load
        assert load_inputs(ctx, ids)[0] == 0
        desc = Desc(cp, Gates(cp))
        ctx.preprocess(desc.d, device_ptrs=False)
        no_plan()
        assert load_inputs(ctx, ids)[0] == 0
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False, pis), assignment_values(cp))
    finally:
        ctx.close()


def test_no_key_no_map_and_a_sharded_context_are_refused():
    import pnp
    import torch
    from pnp.shard import SoloExchange, a2a_bytes_for, v_bytes_for
    from test_gpu_assignment import inst, load_coeff_key
    cp, inp, _, var, _ = inst("merkle4")
    ids = np.array(merkle_inputs(cp), dtype=np.uint32)
    ctx = pnp.Context(0)
    try:
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):  # no key
            ctx.load_solve_inputs(ids.ctypes.data, len(ids))
        load_coeff_key(ctx, inp)
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY.*wire map"):  # a key without its map
            ctx.load_solve_inputs(ids.ctypes.data, len(ids))
    finally:
        ctx.close()
    ctx = context_for(cp)
    try:
        solo = SoloExchange(1, 2, device=torch.device("cuda", 0), a2a_bytes=a2a_bytes_for(inp.lg_n, 2),
                            v_bytes=v_bytes_for(inp.lg_n, 2))
        ctx.set_msm_shard(solo)
        rc, _ = ctx.load_solve_inputs(ids.ctypes.data, len(ids))
        assert rc == PNP_E_ARG and "ranks" in ctx.last_error()
    finally:
        ctx.close()
