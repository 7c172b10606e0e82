"""Every refusal of the satisfiability check and the witness solver whose host
code lives in csrc/check_witness.cpp and csrc/solve_witness.cpp (and the
argument tests of their entry points in csrc/abi.cpp), by its code and the
whole pnp_last_error() text.  The other GPU tests match these messages by a
fragment ("ranks", "gates"); here each is written out, and where two refusals
apply to one call the one that wins is pinned too.

Shapes: merkle(4) of tests/test_gpu_solve.py (1356 rows, 1375 variables, 23
inputs, the root's public input on row 1355, D = 2048) and, for the `gates`
argument, one 2-bit range gate of tests/gate_circuits.py (3 rows)."""
import ctypes

import numpy as np
import pytest

from circuits import Composer
from gate_circuits import range_of
from solve_gates_ref import LOGIC, RANGE
from test_assignment_ref import assignment_values
from test_gpu_solve import context_for, load_inputs, merkle, mont
from test_gpu_solve_gates import load_gates
from test_gpu_solve_outputs import load_plan

pytestmark = pytest.mark.gpu

PNP_E_ARG, PNP_E_NOKEY = -1, -3
ROOT_ROW, N_VARS, N_INPUTS = 1355, 1375, 23
SHARDED = "{}: the context is sharded over 2 ranks (a multi-rank {} is not supported)"
NO_PLAN = "no solve plan resident (pnp_load_solve_inputs or pnp_load_solve_plan first)"
NO_SOLUTION = "no solved assignment resident (a plan and pnp_solve_assignment first)"
ON_OUTPUT = "{}: row 1355 is an output of the plan (its public input is derived, not given)"


def raises(ctx, call, text):
    """`call` raises pnp.PnpError with exactly "<call>: <code>: <text>", and pnp_last_error() is the text."""
    import pnp
    with pytest.raises(pnp.PnpError) as e:
        call()
    assert str(e.value) == text, str(e.value)
    assert ctx.last_error() == text.split(": ", 2)[2]


def shard(ctx, lg_n):
    import torch
    from pnp.shard import SoloExchange, a2a_bytes_for, v_bytes_for
    solo = SoloExchange(1, 2, device=torch.device("cuda", 0), a2a_bytes=a2a_bytes_for(lg_n, 2),
                        v_bytes=v_bytes_for(lg_n, 2))
    ctx.set_msm_shard(solo)
    return solo


def sizes(cp, ids):
    assert (len(cp.rows), len(cp.vals), len(ids), list(cp.pis)) == (ROOT_ROW + 1, N_VARS, N_INPUTS, [ROOT_ROW])


def test_a_sharded_context_every_entry_point_and_no_plan_first():
    from test_gpu_assignment import inst
    cp, ids, _ = merkle(4)
    sizes(cp, ids)
    inp = inst("merkle4")[1]
    pis = sorted(cp.pis.items())
    values = assignment_values(cp)
    inputs = mont([cp.vals[u] for u in ids])
    rows = np.array([ROOT_ROW], dtype=np.uint64)
    ctx = context_for(cp)
    try:
        keep = shard(ctx, 11)
        # sharded and no plan: the missing plan is what the caller hears
        raises(ctx, lambda: ctx.solve_assignment(inputs.ctypes.data, N_INPUTS, False, pis),
               "pnp_solve_assignment: PNP_E_NOKEY: " + NO_PLAN)
        raises(ctx, lambda: ctx.check_assignment(values.ctypes.data, N_VARS, False, pis),
               "pnp_check_assignment: PNP_E_ARG: " + SHARDED.format("check", "check"))
        raises(ctx, lambda: ctx.check_witness(inp.circuit, False, pis),
               "pnp_check_witness: PNP_E_ARG: " + SHARDED.format("check", "check"))
        rc, _ = load_inputs(ctx, ids)
        assert rc == PNP_E_ARG and ctx.last_error() == SHARDED.format("load solve inputs", "solve")
        rc, _ = load_plan(ctx, ids, rows)
        assert rc == PNP_E_ARG and ctx.last_error() == SHARDED.format("load solve plan", "solve")
        rc, _ = load_gates(ctx, ids, 3, rows)
        assert rc == PNP_E_ARG and ctx.last_error() == SHARDED.format("load solve plan", "solve")
        del keep
    finally:
        ctx.close()
    # a plan built on one GPU, the context sharded afterwards
    ctx = context_for(cp)
    try:
        assert load_inputs(ctx, ids)[0] == 0
        keep = shard(ctx, 11)
        raises(ctx, lambda: ctx.solve_assignment(inputs.ctypes.data, N_INPUTS, False, pis),
               "pnp_solve_assignment: PNP_E_ARG: " + SHARDED.format("solve assignment", "solve"))
        del keep
    finally:
        ctx.close()


def test_unaligned_hbm_pointers():
    from gpu_util import to_dev
    cp, ids, _ = merkle(4)
    dev = to_dev(np.zeros((N_VARS + 1, 4), dtype=np.uint64))
    odd = dev.data_ptr() + 8
    ctx = context_for(cp)
    try:
        raises(ctx, lambda: ctx.prove_assignment(odd, N_VARS, True, []),
               "pnp_prove_assignment: PNP_E_ARG: prove assignment: HBM values must be 16-byte aligned")
        raises(ctx, lambda: ctx.check_assignment(odd, N_VARS, True, []),
               "pnp_check_assignment: PNP_E_ARG: check assignment: HBM values must be 16-byte aligned")
        raises(ctx, lambda: ctx.solve_assignment(odd, N_INPUTS, True, []),
               "pnp_solve_assignment: PNP_E_ARG: solve assignment: HBM inputs must be 16-byte aligned")
    finally:
        ctx.close()


def test_no_plan_no_solution_counts_and_public_inputs_on_an_output_row():
    cp, ids, _ = merkle(4)
    sizes(cp, ids)
    inputs = mont([cp.vals[u] for u in ids])
    root = [(ROOT_ROW, cp.pis[ROOT_ROW])]
    ctx = context_for(cp)
    try:
        # nothing resident: the three wordings
        raises(ctx, lambda: ctx.solve_assignment(inputs.ctypes.data, N_INPUTS, False, []),
               "pnp_solve_assignment: PNP_E_NOKEY: " + NO_PLAN)
        raises(ctx, ctx.solve_gate_entries,
               "pnp_solve_gate_entries: PNP_E_NOKEY: no solve plan resident (pnp_load_solve_plan_gates first)")
        raises(ctx, ctx.assignment_ptr, "pnp_assignment_ptr: PNP_E_NOKEY: " + NO_SOLUTION)
        assert load_plan(ctx, ids, [ROOT_ROW])[0] == 0, ctx.last_error()
        # a plan, no solution yet
        raises(ctx, lambda: ctx.assignment_values(k=1), "pnp_assignment_values: PNP_E_NOKEY: " + NO_SOLUTION)
        raises(ctx, lambda: ctx.prove_solved(root), "pnp_prove_solved: PNP_E_NOKEY: " + NO_SOLUTION)
        raises(ctx, lambda: ctx.check_solved(root), "pnp_check_solved: PNP_E_NOKEY: " + NO_SOLUTION)
        raises(ctx, lambda: ctx.solve_assignment(inputs.ctypes.data, N_INPUTS - 1, False, []),
               "pnp_solve_assignment: PNP_E_ARG: solve assignment: 22 inputs, the plan was built for 23")
        # a bad count and a public input on the output row: the count is what the caller hears
        raises(ctx, lambda: ctx.solve_assignment(inputs.ctypes.data, N_INPUTS + 1, False, root),
               "pnp_solve_assignment: PNP_E_ARG: solve assignment: 24 inputs, the plan was built for 23")
        raises(ctx, lambda: ctx.solve_assignment(inputs.ctypes.data, N_INPUTS, False, root),
               "pnp_solve_assignment: PNP_E_ARG: " + ON_OUTPUT.format("solve assignment"))
        ctx.solve_assignment(inputs.ctypes.data, N_INPUTS, False, [])
        assert ctx.solved_public_inputs() == root
        raises(ctx, lambda: ctx.prove_solved(root), "pnp_prove_solved: PNP_E_ARG: " + ON_OUTPUT.format("prove solved"))
        raises(ctx, lambda: ctx.check_solved(root), "pnp_check_solved: PNP_E_ARG: " + ON_OUTPUT.format("check solved"))
        raises(ctx, lambda: ctx.assignment_values(ids=[0, N_VARS]),
               "pnp_assignment_values: PNP_E_ARG: assignment values: id 1375 is not a variable (n_vars = 1375)")
        raises(ctx, lambda: ctx.assignment_values(k=N_VARS + 1),
               "pnp_assignment_values: PNP_E_ARG: assignment values: 1376 values of 1375 variables")
        ok, rep = ctx.check_solved([])
        assert ok and rep.violations == 0, ctx.last_error()
    finally:
        ctx.close()


def test_the_unsatisfied_row_of_one_broken_value():
    cp, ids, _ = merkle(4)
    assert 28 in cp.rows[7][1]  # the variable changed below: row 7 is the first of the four rows that read it
    values = assignment_values(cp).copy()
    values[28, 0] ^= 1
    ctx = context_for(cp)
    try:
        ok, rep = ctx.check_assignment(values.ctypes.data, N_VARS, False, sorted(cp.pis.items()))
        assert not ok and (rep.violations, rep.first_row) == (4, 7)
        assert ctx.last_error() == "row 7: arith constraint 0 (4 violations)"
    finally:
        ctx.close()


def test_gates_with_a_bit_that_is_no_family():
    cp = Composer(31)
    x = cp.var(2)
    range_of(cp, x, 2)
    ids = list(range(len(cp.vals)))
    assert len(cp.rows) == 3 and ids == [0, 1, 2]
    ctx = context_for(cp)
    try:
        for bad, text in ((4, "0x4"), (1 << 31 | 1, "0x80000001")):
            rc, _ = load_gates(ctx, ids, bad)
            assert rc == PNP_E_ARG and ctx.last_error() == (
                f"load solve plan: gates = {text} has a bit that is no gate family (PNP_SOLVE_RANGE | PNP_SOLVE_LOGIC)")
        pair = (ctypes.c_uint64 * 2)()
        assert ctx.lib.pnp_solve_gate_entries(ctx.h, ctypes.byref(pair)) == PNP_E_NOKEY  # nothing was built
        assert load_gates(ctx, ids, RANGE | LOGIC)[0] == 0, ctx.last_error()
        assert ctx.solve_gate_entries() == (0, 0)  # (every variable an input)
    finally:
        ctx.close()
