"""Output rows on the MI355X: pnp_load_solve_plan, the derived public inputs of
pnp_solve_assignment (csrc/solve.hip, k_solve_outputs_), pnp_solved_public_inputs,
pnp_prove_solved and pnp_check_solved against the plain-integer model of
tests/solve_outputs_ref.py and the oracle's proof bytes.  Every comparison is
exact: field elements, counts, proof bytes, messages.

The Merkle circuit's root row as the output: the solve is given the leaves and
no public input, and hands back PI = -root.  merkle4 is one narrow launch,
merkle9 (49,220 rows) wide and narrow runs; 256 and 257 output rows sit on
either side of the output kernel's workgroup boundary."""
import ctypes
import functools

import numpy as np
import pytest

from circuits import Composer, R_MOD
from pnp import abi
from solve_outputs_ref import derive, plan_outputs
from solve_ref import merkle_inputs, solve
from test_assignment_ref import assignment_values
from test_gpu_preprocess import dev_u32
from test_gpu_solve import M1, NONE, PNP_E_ARG, Gates, context_for, info_tuple, load_inputs, mont, solution, solve_gpu

pytestmark = pytest.mark.gpu

OUTPUT_OF_PLAN = "PNP_E_ARG.*row {} is an output of the plan"


def load_plan(ctx, ids, rows, device=False):
    from gpu_util import to_dev
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if device:
        t, r = dev_u32(ids), to_dev(rows if len(rows) else np.zeros(1, dtype=np.uint64))
        return ctx.load_solve_plan(t.data_ptr(), len(ids), r.data_ptr() if len(rows) else 0, len(rows), True)
    return ctx.load_solve_plan(ids.ctypes.data if len(ids) else 0, len(ids), rows.ctypes.data if len(rows) else 0,
                               len(rows), False)


# ------------------------------------------------------------------ the Merkle circuit
@functools.lru_cache(maxsize=None)
def merkle(height, seed=11):
    """(composer, input ids, root row, the model's plan with the root row as output), made once, never mutated."""
    import merkle_circuit as mc
    cp = mc.merkle_circuit(height, seed=seed)[0]
    ids = merkle_inputs(cp)
    root_row = len(cp.rows) - 1
    assert list(cp.pis) == [root_row]
    return cp, ids, root_row, plan_outputs(cp.rows, len(cp.vals), ids, [root_row])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("height", [4, 9])
def test_merkle_root_comes_out_of_the_solve(height, device):
    cp, ids, root_row, pl = merkle(height)
    n_vars = len(cp.vals)
    assert len(pl.levels) == {4: 195, 9: 520}[height] and pl.undetermined == []
    if height == 4:
        assert pl.max_width <= 16  # one launch of one workgroup
    else:
        assert len(cp.rows) == 49220 and pl.widths[:4] == [512, 384, 384, 384] and pl.widths[-3:] == [3, 3, 1]
    ctx = context_for(cp)
    try:
        rc, info = load_plan(ctx, ids, [root_row], device)
        assert rc == 0, ctx.last_error()
        assert info_tuple(info) == (len(ids), pl.n_solved, len(pl.levels), pl.max_width, 0, NONE)
        assert info.n_solved + info.n_inputs == n_vars and info.plan_bytes > 0
        got = solve_gpu(ctx, cp.vals, ids, device)  # no public input
        assert np.array_equal(got, assignment_values(cp))
        assert ctx.solved_public_inputs() == sorted(cp.pis.items())
        stages = dict(ctx.stage_times())
        assert list(stages) == ["solve_inputs", "solve_levels", "solve_outputs", "inputs_h2d_bytes"]
        ok, rep = ctx.check_solved([])
        assert ok and rep.violations == 0, ctx.last_error()
        # without the derived public input the root row is violated: the check looks
        addr, n = ctx.assignment_ptr()
        ok, rep = ctx.check_assignment(addr, n, True, [])
        assert not ok and rep.first_row == root_row
        # another seed's leaves over the same plan give that seed's root
        cp2 = merkle(height, seed=23)[0]
        assert cp2.pis != cp.pis
        assert np.array_equal(solve_gpu(ctx, cp2.vals, ids, device), assignment_values(cp2))
        assert ctx.solved_public_inputs() == sorted(cp2.pis.items())
        # the same plan and info on a second build
        rc, again = load_plan(ctx, ids, [root_row], device)
        assert rc == 0 and bytes(again) == bytes(info)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, device), assignment_values(cp))
        assert ctx.solved_public_inputs() == sorted(cp.pis.items())
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["merkle4", "merkle6"])
def test_prove_solved_is_the_oracles_proof(kind):
    """preprocess, plan with the root row as output, solve from the leaves,
    prove: the oracle's bytes, and again after a proof from columns."""
    from test_general import pis_of
    from test_gpu_assignment import inst
    cp, inp, exp, var, values = inst(kind)
    ids = merkle_inputs(cp)
    root_row = len(cp.rows) - 1
    assert pis_of(inp) == [(root_row, cp.pis[root_row])]
    ctx = context_for(cp, inp)
    try:
        assert load_plan(ctx, ids, [root_row])[0] == 0
        solve_gpu(ctx, cp.vals, ids, False)
        assert abi.proof_to_bytes(ctx.prove_solved([])) == exp
        assert abi.proof_to_bytes(ctx.prove_ex(inp.circuit, False, pis_of(inp))) == exp
        assert abi.proof_to_bytes(ctx.prove_solved([], label=b"Merkle tree")) == exp
        assert ctx.solved_public_inputs() == pis_of(inp)
        assert np.array_equal(solution(ctx, len(cp.vals)), values)
    finally:
        ctx.close()


# ------------------------------------------------------------------ synthetic circuits
def output_rows(width):
    """`width` rows w = x + 1 (one wide or narrow level), then `width`
    independent output rows 7 (3 x^5 + 2 y - x y + ... + c) + PI = 0 over
    (x, y, z, w) with every selector in play."""
    cp = Composer(100 + width)
    ids, quads = [0], []
    for _ in range(width):
        x, y, z = cp.var(cp.rnd()), cp.var(cp.rnd()), cp.var(cp.rnd())
        w = cp.var(cp.vals[x] + 1)
        cp.row({"q_arith": 1, "q_l": 1, "q_c": 1, "q_4": M1}, x, 0, 0, w)
        ids += [x, y, z]
        quads.append((x, y, z, w))
    outs = []
    for q in quads:
        outs.append(cp.row({"q_arith": 7, "q_hl": 3, "q_r": 2, "q_m": M1, "q_c": cp.rnd(), "q_l": cp.rnd(),
                            "q_o": cp.rnd(), "q_4": cp.rnd(), "q_hr": cp.rnd(), "q_h4": cp.rnd()}, *q))
    cp.pis = derive(cp.rows, cp.vals, outs)
    return cp, ids, outs


@pytest.mark.parametrize("width", [256, 257])
def test_output_rows_on_either_side_of_the_workgroup_boundary(width):
    cp, ids, outs = output_rows(width)
    n_vars = len(cp.vals)
    pl = plan_outputs(cp.rows, n_vars, ids, outs, sweep=True)
    assert pl.widths == [width] and pl.undetermined == []
    assert solve(cp.rows, pl, n_vars, {u: cp.vals[u] for u in ids}) == cp.vals
    assert len(set(cp.pis.values())) == width and 0 not in cp.pis.values()
    listed = outs[::-1]  # the listed order is kept, whatever it is
    ctx = context_for(cp)
    try:
        rc, info = load_plan(ctx, ids, listed)
        assert rc == 0, ctx.last_error()
        assert info_tuple(info) == (len(ids), width, 1, width, 0, NONE)
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), mont(cp.vals))
        assert ctx.solved_public_inputs() == [(r, cp.pis[r]) for r in listed]
        ok, rep = ctx.check_solved([])
        assert ok and rep.violations == 0, ctx.last_error()
    finally:
        ctx.close()


def test_a_derived_zero_is_reported_and_proves_like_no_public_input():
    cp = Composer(41)
    x = cp.var(cp.rnd())
    y = cp.var(3 * cp.vals[x])
    cp.row({"q_arith": 1, "q_l": 3, "q_o": M1}, x, 0, y, 0)
    out = cp.row({"q_arith": 5, "q_l": 3, "q_o": M1}, x, 0, y, 0)  # 5 (3 x - y) + PI = 0: PI = 0
    assert derive(cp.rows, cp.vals, [out]) == {out: 0} and not cp.pis
    inp = cp.build()
    exp = abi.proof_to_bytes(inp.oracle_proof())
    ids = [v for v in range(len(cp.vals)) if v != y]  # (build() may add variables: all of them inputs)
    ctx = context_for(cp, inp)
    try:
        rc, info = load_plan(ctx, ids, [out])
        assert rc == 0 and info.n_solved == 1, ctx.last_error()
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), assignment_values(cp))
        assert ctx.solved_public_inputs() == [(out, 0)]
        assert ctx.check_solved([])[0]
        assert abi.proof_to_bytes(ctx.prove_solved([])) == exp
    finally:
        ctx.close()


def test_a_given_and_a_derived_public_input_together():
    """test_gpu_solve's pi_on_a_defining_row, 3 (2 x + 4 y) + PI = 0 defining y
    from a given PI, and an output row over y in the same circuit."""
    cp = Composer(6)
    x = cp.var(cp.rnd())
    pi = cp.rnd()
    y = cp.var(-(2 * cp.vals[x] + pi * pow(3, -1, R_MOD)) * pow(4, -1, R_MOD))
    r = cp.row({"q_arith": 3, "q_l": 2, "q_4": 4}, x, 0, 0, y)
    z = cp.var(cp.vals[y] + 1)
    cp.row({"q_arith": 1, "q_l": 1, "q_c": 1, "q_o": M1}, y, 0, z, 0)
    out = cp.row({"q_arith": 2, "q_h4": 1, "q_m": 9, "q_c": 4}, y, z, 0, x)
    ids = [0, x]
    n_vars = len(cp.vals)
    derived = derive(cp.rows, cp.vals, [out])
    pl = plan_outputs(cp.rows, n_vars, ids, [out], sweep=True)
    assert solve(cp.rows, pl, n_vars, {u: cp.vals[u] for u in ids}, {r: pi}) == cp.vals and derived[out] != 0
    ctx = context_for(cp)
    try:
        rc, info = load_plan(ctx, ids, [out])
        assert rc == 0 and info_tuple(info) == (2, 2, 2, 1, 0, NONE), ctx.last_error()
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False, [(r, pi)]), mont(cp.vals))
        assert ctx.solved_public_inputs() == [(out, derived[out])]
        ok, rep = ctx.check_solved([(r, pi)])
        assert ok and rep.violations == 0, ctx.last_error()
        addr, n = ctx.assignment_ptr()
        assert ctx.check_assignment(addr, n, True, [(r, pi), (out, derived[out])])[0]
        ok, rep = ctx.check_solved([])  # the given one left out: its row says so
        assert not ok and rep.first_row == r
    finally:
        ctx.close()


def test_a_variable_only_an_output_row_could_define_is_undetermined():
    import pnp
    cp = Composer(43)
    x = cp.var(cp.rnd())
    y = cp.var(5 * cp.vals[x] + 7)
    r = cp.row({"q_arith": 1, "q_l": 5, "q_c": 7, "q_r": M1}, x, y, 0, 0)
    z = cp.var(cp.vals[y] + 1)
    cp.row({"q_arith": 1, "q_l": 1, "q_c": 1, "q_o": M1}, y, 0, z, 0)
    ids = [0, x]
    pl = plan_outputs(cp.rows, len(cp.vals), ids, [r], sweep=True)
    assert pl.undetermined == [y, z] and pl.levels == []
    two = mont([0, 1])
    ctx = context_for(cp)
    try:
        assert load_plan(ctx, ids, [])[0] == 0  # without the output the row defines y
        rc, info = load_plan(ctx, ids, [r])
        assert rc == PNP_E_ARG and info_tuple(info) == (2, 0, 0, 0, 2, y)
        assert f"variable {y} " in ctx.last_error()
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY.*plan"):
            ctx.solve_assignment(two.ctypes.data, 2, False)
    finally:
        ctx.close()


# ------------------------------------------------------------------ errors and lifecycle
def test_bad_output_rows_are_named_and_no_plan_stays():
    import pnp
    cp = Composer(44)
    x = cp.var(cp.rnd())
    y = cp.var(cp.vals[x] + 2)
    cp.row({"q_arith": 1, "q_l": 1, "q_c": 2, "q_o": M1}, x, 0, y, 0)
    good = [cp.row({"q_arith": 1, "q_l": 1 + k}, y, 0, 0, 0) for k in range(3)]
    dead = cp.row({"q_l": 1}, y, 0, 0, 0)  # q_arith = 0
    ng = len(cp.rows)
    ids = [0, x]
    two = mont([0, 1])
    ctx = context_for(cp)
    try:
        before = ctx.hbm_usage()["live"]
        for rows, what in ((good + [ng], f"output row {ng} is not a gate"),
                           ([1 << 40] + good, f"output row {1 << 40} is not a gate"),
                           ([good[2], good[1], good[2], good[1]], f"output row {good[1]} is listed twice"),
                           (good + [dead], f"output row {dead} has q_arith = 0"),
                           ([dead, good[0], good[0], ng + 5, ng], f"output row {ng} is not a gate"),
                           ([dead, good[0], good[0]], f"output row {good[0]} is listed twice")):
            for device in (False, True):
                assert load_plan(ctx, ids, good)[0] == 0
                rc, info = load_plan(ctx, ids, rows, device)
                assert rc == PNP_E_ARG and what in ctx.last_error(), ctx.last_error()
                with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY.*plan"):
                    ctx.solve_assignment(two.ctypes.data, 2, False)
                assert ctx.hbm_usage()["live"] == before
    finally:
        ctx.close()


def test_lifecycle_errors_drop_and_accounting():
    import pnp
    from test_gpu_assignment import host_cols
    from test_gpu_preprocess import Desc
    from test_preprocess_ref import wire_map
    cp, ids, root_row, pl = merkle(4)
    n_vars = len(cp.vals)
    root_pi = [(root_row, cp.pis[root_row])]
    inputs = mont([cp.vals[u] for u in ids])
    ctx = context_for(cp)
    try:
        def nothing_solved():
            with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
                ctx.solved_public_inputs()
            with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
                ctx.check_solved([])
            with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
                ctx.prove_solved([])
        nothing_solved()  # before any plan
        # (the check transforms the selector rows as the plan build does: every table they need exists now)
        values = assignment_values(cp)
        assert ctx.check_assignment(values.ctypes.data, n_vars, False, root_pi)[0]
        before = ctx.hbm_usage()["live"]
        # no outputs: pnp_load_solve_inputs, to the byte
        rc, plain = load_inputs(ctx, ids)
        assert rc == 0
        rc, none = load_plan(ctx, ids, [])
        assert rc == 0 and bytes(none) == bytes(plain)
        assert ctx.hbm_usage()["live"] == before + plain.plan_bytes
        sol = solve_gpu(ctx, cp.vals, ids, False, root_pi)
        assert np.array_equal(sol, assignment_values(cp))
        assert ctx.solved_public_inputs() == []
        assert list(dict(ctx.stage_times())) == ["solve_inputs", "solve_levels", "inputs_h2d_bytes"]
        assert load_inputs(ctx, ids)[0] == 0
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False, root_pi), sol)
        assert ctx.check_solved(root_pi)[0]  # the caller's list alone
        # with the output: its entry is counted in plan_bytes
        rc, info = load_plan(ctx, ids, [root_row])
        assert rc == 0 and info.plan_bytes > plain.plan_bytes
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes
        nothing_solved()  # a plan, no solution yet
        with pytest.raises(pnp.PnpError, match=OUTPUT_OF_PLAN.format(root_row)):
            ctx.solve_assignment(inputs.ctypes.data, len(ids), False, root_pi)
        nothing_solved()
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), assignment_values(cp))
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes + 32 * n_vars
        for call in (ctx.prove_solved, ctx.check_solved):
            with pytest.raises(pnp.PnpError, match=OUTPUT_OF_PLAN.format(root_row)):
                call([(3, 1)] + root_pi)
        with pytest.raises(pnp.PnpError, match=OUTPUT_OF_PLAN.format(root_row)):  # a zero one too
            ctx.check_solved([(root_row, 0)])
        assert ctx.solved_public_inputs() == root_pi  # the refusals changed nothing
        assert ctx.check_solved([])[0]
        n = ctypes.c_uint64(7)
        assert ctx.lib.pnp_solved_public_inputs(ctx.h, None, None, 0, None) == PNP_E_ARG
        assert ctx.lib.pnp_solved_public_inputs(ctx.h, None, None, 0, ctypes.byref(n)) == 0 and n.value == 1
        # a second solve rewrites the same buffers
        solve_gpu(ctx, cp.vals, ids, False)
        assert ctx.hbm_usage()["live"] == before + info.plan_bytes + 32 * n_vars
        # whatever replaces the wire map drops the plan, the solution and the outputs
        keep, addrs = host_cols(wire_map(cp))
        ctx.load_wire_map(addrs, len(cp.rows), n_vars, device_ptrs=False)
        nothing_solved()
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY.*plan"):
            ctx.solve_assignment(inputs.ctypes.data, len(ids), False)
        assert ctx.hbm_usage()["live"] == before
        # ... and so does a key load
        assert load_plan(ctx, ids, [root_row])[0] == 0
        solve_gpu(ctx, cp.vals, ids, False)
        desc = Desc(cp, Gates(cp))
        ctx.preprocess(desc.d, device_ptrs=False)
        nothing_solved()
        assert load_plan(ctx, ids, [root_row])[0] == 0
        assert np.array_equal(solve_gpu(ctx, cp.vals, ids, False), assignment_values(cp))
        assert ctx.solved_public_inputs() == root_pi
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
        rc, _ = load_plan(ctx, merkle_inputs(cp), [len(cp.rows) - 1])
        assert rc == PNP_E_ARG and "ranks" in ctx.last_error()
    finally:
        ctx.close()
