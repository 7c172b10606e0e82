"""The witness solver's model (tests/solve_ref.py) pinned on the CPU: on the
reference's Merkle circuit, from the blinding values, the leaves and the
per-hash domain tags, the rules determine every other variable — zero_var, the
hash states, the tree nodes (through the assert_equal rows) — and reproduce
the composer's own values; 65 rounds a tree level, less the root's: the root
variable is defined in round 2 by the root row (root - PI-root = 0 with the
constant zero in c), so its assert_equal stays a constraint.  The counter form
of the plan equals the word-for-word sweep."""
import functools

import pytest

import merkle_circuit as mc
from circuits import Composer, R_MOD
from solve_ref import define, merkle_inputs, plan, plan_sweep, slot_masks, solve


@functools.lru_cache(maxsize=None)
def merkle(height, seed=11):
    return mc.merkle_circuit(height, seed=seed)[0]


@pytest.mark.parametrize("height,levels,n_vars,n_inputs", [(4, 194, 1375, 23), (6, 324, 6055, 71)])
def test_merkle_is_determined_by_blinding_leaves_and_tags(height, levels, n_vars, n_inputs):
    cp = merkle(height)
    ids = merkle_inputs(cp)
    assert (len(cp.vals), len(ids)) == (n_vars, n_inputs)
    pl = plan(cp.rows, n_vars, ids)
    assert pl.undetermined == [] and len(pl.levels) == levels
    assert pl.n_solved == n_vars - n_inputs
    assert pl.max_width <= (16 if height == 4 else 64)
    got = solve(cp.rows, pl, n_vars, {u: cp.vals[u] for u in ids}, cp.pis)
    assert got == cp.vals
    # The public input matters on a defining row: the root row defines the root
    # variable in round 2 (root = -PI), and the root's assert_equal row then
    # defines the last hash's output from it in round 3.  Without the public
    # input exactly those two variables differ (they come out 0): the rules do
    # not compute the root for a caller that does not know it.
    no_pi = solve(cp.rows, pl, n_vars, {u: cp.vals[u] for u in ids})
    root_row = len(cp.rows) - 1
    root_var, (eq_a, out_var) = cp.rows[root_row][1][0], cp.rows[root_row - 1][1][:2]
    assert eq_a == root_var
    assert [u for u in range(n_vars) if no_pi[u] != cp.vals[u]] == sorted([root_var, out_var])
    assert (root_var, root_row, 0) in pl.levels[1] and (out_var, root_row - 1, 1) in pl.levels[2]
    assert no_pi[root_var] == no_pi[out_var] == 0


def test_counter_plan_equals_the_sweep():
    cp = merkle(4)
    ids = merkle_inputs(cp)
    a, b = plan(cp.rows, len(cp.vals), ids), plan_sweep(cp.rows, len(cp.vals), ids)
    assert a.levels == b.levels and a.undetermined == b.undetermined == []
    # fewer inputs: what stays undetermined is the same too
    a, b = plan(cp.rows, len(cp.vals), ids[:-3]), plan_sweep(cp.rows, len(cp.vals), ids[:-3])
    assert a.levels == b.levels and a.undetermined == b.undetermined != []


def test_slot_masks():
    assert slot_masks({"q_l": 1}) == ((False,) * 4, (False,) * 4)  # q_arith = 0
    rel, solv = slot_masks({"q_arith": 1, "q_l": 3, "q_hr": 2, "q_o": R_MOD - 1, "q_h4": 1, "q_4": 1})
    assert rel == (True, True, True, True) and solv == (True, False, True, False)
    rel, solv = slot_masks({"q_arith": 1, "q_m": 1, "q_l": 1, "q_o": 1})
    assert rel == (True, True, True, False) and solv == (False, False, True, False)


def test_lowest_row_wins_and_q_arith_divides_the_public_input():
    cp = Composer(1)
    x = cp.var(5)
    y = cp.var(0)
    cp.row({"q_arith": 1, "q_l": 1, "q_o": R_MOD - 1, "q_c": 9}, x, 0, y, 0)   # y = x + 9
    cp.row({"q_arith": 1, "q_l": 2, "q_o": R_MOD - 1}, x, 0, y, 0)             # y = 2 x: ready too, loses
    z = cp.var(0)
    r = cp.row({"q_arith": 7, "q_r": 1, "q_4": 3}, 0, y, 0, z)                 # 7 (y + 3 z) + PI = 0
    pl = plan_sweep(cp.rows, 4, [0, x])
    assert pl.levels == [[(y, 0, 2)], [(z, r, 3)]]
    vals = solve(cp.rows, pl, 4, {0: 0, x: 5}, {r: 21})
    assert vals[y] == 14 and (7 * (vals[y] + 3 * vals[z]) + 21) % R_MOD == 0
    assert define(cp.rows[r][0], cp.rows[r][1], 3, vals, 21) == vals[z]
