"""The model of output rows (tests/solve_outputs_ref.py) on the Merkle circuit:
with the root row as an output the plan takes one more round, leaves nothing
undetermined, solves to the composer's values without any public input, and
derives the composer's public input."""
import functools

import pytest

import solve_ref
from solve_outputs_ref import derive, masked, plan_outputs
from solve_ref import merkle_inputs


@functools.lru_cache(maxsize=None)
def merkle(height):
    import merkle_circuit as mc
    cp = mc.merkle_circuit(height, seed=11)[0]
    return cp, merkle_inputs(cp), len(cp.rows) - 1


@pytest.mark.parametrize("height,rounds", [(3, 130), (4, 195), (6, 325)])
def test_root_row_as_output(height, rounds):
    cp, ids, root_row = merkle(height)
    n_vars = len(cp.vals)
    assert list(cp.pis) == [root_row]
    pl = plan_outputs(cp.rows, n_vars, ids, [root_row])
    assert len(pl.levels) == rounds == len(solve_ref.plan(cp.rows, n_vars, ids).levels) + 1
    assert pl.widths[-3:] == [3, 3, 1]
    assert pl.undetermined == []
    assert all(i != root_row for l in pl.levels for _, i, _ in l)
    if height <= 4:
        assert plan_outputs(cp.rows, n_vars, ids, [root_row], sweep=True).levels == pl.levels
    vals = solve_ref.solve(cp.rows, pl, n_vars, {u: cp.vals[u] for u in ids})  # no public input
    assert vals == cp.vals
    assert derive(cp.rows, vals, [root_row]) == cp.pis


def test_no_outputs_is_the_plan_of_solve_ref():
    cp, ids, _ = merkle(4)
    n_vars = len(cp.vals)
    assert masked(cp.rows, []) == cp.rows
    assert plan_outputs(cp.rows, n_vars, ids, []).levels == solve_ref.plan(cp.rows, n_vars, ids).levels
    assert plan_outputs(cp.rows, n_vars, ids, [], sweep=True).levels == solve_ref.plan_sweep(cp.rows, n_vars, ids).levels


def test_derive_is_minus_q_arith_times_the_full_sum():
    """Every slot as it stands: a slot that is not relevant meets zero coefficients."""
    from circuits import R_MOD
    rows = [({"q_arith": 7, "q_hl": 3, "q_r": 2, "q_m": R_MOD - 1, "q_c": 5}, (1, 2, 3, 4))]
    vals = [0, 2, 3, 1000, 10]
    s = 3 * 2 ** 5 + 2 * 3 - 2 * 3 + 5
    assert derive(rows, vals, [0]) == {0: -7 * s % R_MOD}
