"""Composer helpers for range and logic gates over values the circuit computes,
laid out as the reference's composer lays them (constraint_system/range.rs,
logic.rs, composer.rs assert_equal), for the tests of the witness solver's gate
rules (tests/solve_gates_ref.py, tests/test_gpu_solve_gates.py).  Built on
tests/circuits.py's Composer: `cp.vals` already holds the value of the variable
that is decomposed."""
from circuits import R_MOD

M1 = R_MOD - 1


def assert_equal(cp, a, b):
    """composer.rs assert_equal: the arithmetic row a - b = 0."""
    return cp.row({"q_arith": 1, "q_l": 1, "q_r": M1}, a, b, 0, 0)


def range_of(cp, var, num_bits):
    """constraint_system/range.rs range_gate over the variable `var` (whose
    value the composer knows): the accumulators of its base-4 digits, most
    significant first, four a row with d first, padded at the front with
    variable 0 so that the last accumulator stands alone in slot d of the row
    after the last range row; then assert_equal(last accumulator, var).
    Returns (first range row, the accumulator variables)."""
    assert num_bits % 2 == 0 and num_bits > 0
    v = cp.vals[var]
    n_quads = num_bits // 2
    accs = [cp.var(v >> (2 * (n_quads - 1 - k))) for k in range(n_quads)]
    # slots in order d, c, b, a of successive rows: 1 leading zero (the first d), then pad so that
    # the count after the padding is 1 mod 4 (the last accumulator opens a row)
    seq = [0] + accs
    pad = (1 - len(seq)) % 4
    seq = [0] * pad + seq
    first = len(cp.rows)
    while len(seq) > 1:
        d, c, b, a = seq[:4]
        cp.row({"range_selector": 1}, a, b, c, d)
        seq = seq[4:]
    cp.row({}, 0, 0, 0, seq[0])
    assert_equal(cp, seq[0], var)
    return first, accs


def logic_of(cp, a, b, num_bits, xor):
    """constraint_system/logic.rs logic_gate over the variables a, b: a zero
    row of accumulators first (variable 0 in a, b, d), then one row a quad,
    row k holding the accumulators of the k most significant quads of a, b and
    of the result in slots a, b, d and the product of the next quads in c; the
    row after the last logic row holds the full accumulators, which
    assert_equal links to the operands (the reference leaves them unlinked).
    Returns (first logic row, the result variable)."""
    assert num_bits % 2 == 0 and num_bits > 0
    va, vb = cp.vals[a], cp.vals[b]
    n = num_bits // 2
    res = (va ^ vb) if xor else (va & vb)
    acc = lambda x, k: x >> (2 * (n - k))  # the k most significant quads
    first = len(cp.rows)
    wa = wb = wd = 0
    for k in range(n):
        qa, qb = acc(va, k + 1) & 3, acc(vb, k + 1) & 3
        cp.row({"logic_selector": M1 if xor else 1, "q_c": M1 if xor else 1}, wa, wb, cp.var(qa * qb), wd)
        wa, wb, wd = cp.var(acc(va, k + 1)), cp.var(acc(vb, k + 1)), cp.var(acc(res, k + 1))
    cp.row({}, wa, wb, 0, wd)
    assert_equal(cp, wa, a)
    assert_equal(cp, wb, b)
    return first, wd
