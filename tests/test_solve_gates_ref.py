"""The plain-integer model of the gate rules (tests/solve_gates_ref.py) against
the composer's own values, the sweep against the counter form, and the tie
rules one by one.  No GPU: tests/test_gpu_solve_gates.py holds the library to
this model."""
import pytest

from circuits import Composer, R_MOD
from gate_circuits import M1, logic_of, range_of
from solve_gates_ref import LOGIC, RANGE, ROLE_LOGIC, ROLE_RANGE, plan, plan_sweep, solve
import solve_ref

BOTH = RANGE | LOGIC


def solved(cp, ids, gates, outputs=(), pis=None):
    n_vars = len(cp.vals)
    pl = plan_sweep(cp.rows, n_vars, ids, outputs, gates)
    return pl, solve(cp.rows, pl, n_vars, {u: cp.vals[u] for u in ids}, pis, outputs)


# ------------------------------------------------------------------ the model against the composer
@pytest.mark.parametrize("k", [1, 2, 5, 32])
def test_range_chain_from_its_last_accumulator(k):
    cp = Composer(60 + k)
    cp.range_chain(k)
    last = cp.rows[-1][1][3]
    pl, vals = solved(cp, [0, last], RANGE)
    assert pl.undetermined == [] and vals == cp.vals
    assert pl.widths == [4] * k and pl.n_range == 4 * k and pl.n_logic == 0
    # without the flag nothing moves
    assert plan_sweep(cp.rows, len(cp.vals), [0, last], (), LOGIC).levels == []


@pytest.mark.parametrize("xor", [False, True], ids=["and", "xor"])
@pytest.mark.parametrize("k", [1, 3, 32])
def test_logic_chain_from_its_last_operands(k, xor):
    cp = Composer(70 + k)
    cp.logic_chain(k, xor)
    a, b = cp.rows[-1][1][:2]
    pl, vals = solved(cp, [0, a, b], LOGIC)
    assert pl.undetermined == [] and vals == cp.vals
    # (the row above finds its d_next defined already: as d of the row that went before it)
    assert pl.widths == [5] + [4] * (k - 1) and pl.n_logic == 4 * k + 1 and pl.n_range == 0
    assert plan_sweep(cp.rows, len(cp.vals), [0, a, b], (), RANGE).levels == []


def computed_circuit(seed=3):
    """x = p + q ranged to 64 bits, y = x xor p and z = x and q over 64 bits, w = y + z an output row."""
    cp = Composer(seed)
    p, q = cp.var(int(cp.rng.integers(0, 2**62))), cp.var(int(cp.rng.integers(0, 2**62)))
    x = cp.var(cp.vals[p] + cp.vals[q])
    cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, p, q, x, 0)
    range_of(cp, x, 64)
    _, y = logic_of(cp, x, p, 64, True)
    _, z = logic_of(cp, x, q, 64, False)
    out = cp.row({"q_arith": 1, "q_l": 1, "q_r": 1}, y, z, 0, 0)
    cp.pis[out] = -(cp.vals[y] + cp.vals[z]) % R_MOD
    return cp, [0, p, q], out


def test_range_of_and_logic_of_a_computed_value():
    cp, ids, out = computed_circuit()
    pl, vals = solved(cp, ids, BOTH, [out])
    assert pl.undetermined == [] and vals == cp.vals
    # range: 8 rows of 4 slots, less the first d (variable 0); the last accumulator comes from assert_equal.
    # logic, 32 rows a gate: a, b, c, d and d_next from the last, a, b, c, d from 30, c from the first
    assert pl.n_range == 31 and pl.n_logic == 2 * (5 + 30 * 4 + 1)
    import solve_outputs_ref
    assert solve_outputs_ref.derive(cp.rows, vals, [out]) == cp.pis
    # the logic rows cannot start before the operands' accumulators are linked
    assert [u for u in plan_sweep(cp.rows, len(cp.vals), ids, [out], RANGE).undetermined] != []


def test_helpers_lay_the_composers_padding():
    for bits, rows in ((64, 9), (34, 6), (2, 2), (8, 2), (10, 3)):
        cp = Composer(1)
        x = cp.var((1 << bits) - 1 - 5 % (1 << bits))
        first, accs = range_of(cp, x, bits)
        assert len(cp.rows) - first == rows + 1 and len(accs) == bits // 2
        assert all(q.get("range_selector") for q, _ in cp.rows[first:first + rows - 1])
        assert cp.rows[first + rows - 1] == ({}, (0, 0, 0, accs[-1])) and cp.rows[first][1][3] == 0
        pl, vals = solved(cp, [0, x], RANGE)
        assert vals == cp.vals


# ------------------------------------------------------------------ sweep against counters
def plans_equal(a, b):
    return a.levels == b.levels and a.undetermined == b.undetermined


@pytest.mark.parametrize("gates", [0, RANGE, LOGIC, BOTH])
def test_sweep_equals_counters(gates):
    cp, ids, out = computed_circuit(5)
    n_vars = len(cp.vals)
    for outputs in ((), (out,)):
        assert plans_equal(plan_sweep(cp.rows, n_vars, ids, outputs, gates), plan(cp.rows, n_vars, ids, outputs, gates))
    cp = Composer(9)
    cp.range_chain(3)
    cp.logic_chain(4, True)
    cp.arith()
    ids = [0, cp.rows[3][1][3]]
    assert plans_equal(plan_sweep(cp.rows, len(cp.vals), ids, (), gates), plan(cp.rows, len(cp.vals), ids, (), gates))


def test_no_flag_is_the_arithmetic_model():
    import merkle_circuit as mc
    cp = mc.merkle_circuit(2, seed=11)[0]
    ids = solve_ref.merkle_inputs(cp)
    ref = solve_ref.plan_sweep(cp.rows, len(cp.vals), ids)
    for gates in (0, BOTH):
        got = plan_sweep(cp.rows, len(cp.vals), ids, (), gates)
        assert got.levels == ref.levels and got.n_range == got.n_logic == 0 and got.gate_widths == [0] * len(ref.levels)


# ------------------------------------------------------------------ ties
def tie_arith_and_range(arith_first):
    """u sits in slot c of a range row and is the one unknown of an arithmetic
    row u = s + 1; both are ready in round 1 and give different values."""
    cp = Composer(12)
    s = cp.var(cp.rnd())
    v = cp.var(0x1234567)
    u = cp.var(0)

    def arith():
        return cp.row({"q_arith": 1, "q_l": 1, "q_c": 1, "q_o": M1}, s, 0, u, 0)

    ra = arith() if arith_first else None
    rr = cp.row({"range_selector": 1}, 0, 0, u, 0)
    cp.row({}, 0, 0, 0, v)
    ra = arith() if ra is None else ra
    return cp, [0, s, v], u, ra, rr


@pytest.mark.parametrize("arith_first", [True, False], ids=["arith_lower", "range_lower"])
def test_tie_the_lower_row_wins_across_families(arith_first):
    cp, ids, u, ra, rr = tie_arith_and_range(arith_first)
    pl, vals = solved(cp, ids, RANGE)
    assert pl.levels == [[(u, ra, 2) if arith_first else (u, rr, ROLE_RANGE + 2)]]
    assert vals[u] == ((cp.vals[ids[1]] + 1) % R_MOD if arith_first else 0x1234567 >> 6)


def tie_two_slots():
    """u in slots a and c of one range row: a (V >> 2) wins over c (V >> 6)."""
    cp = Composer(13)
    v = cp.var(0xabcdef)
    u = cp.var(0)
    r = cp.row({"range_selector": 1}, u, 0, u, 0)
    cp.row({}, 0, 0, 0, v)
    return cp, [0, v], u, r


def test_tie_the_lower_role_wins_within_a_row():
    cp, ids, u, r = tie_two_slots()
    pl, vals = solved(cp, ids, RANGE)
    assert pl.levels == [[(u, r, ROLE_RANGE)]] and vals[u] == 0xabcdef >> 2


def tie_same_row_families():
    """One row with q_arith = 1 (c = a + 1) and range_selector = 1: the arithmetic slot is the lower role."""
    cp = Composer(14)
    s, v = cp.var(cp.rnd()), cp.var(0xfedcba)
    u = cp.var(0)
    r = cp.row({"q_arith": 1, "q_l": 1, "q_c": 1, "q_o": M1, "range_selector": 1}, s, 0, u, 0)
    cp.row({}, 0, 0, 0, v)
    return cp, [0, s, v], u, r


def test_tie_arithmetic_roles_come_before_range_roles():
    cp, ids, u, r = tie_same_row_families()
    pl, vals = solved(cp, ids, RANGE)
    assert pl.levels == [[(u, r, 2)]] and vals[u] == (cp.vals[ids[1]] + 1) % R_MOD


def tie_d_next():
    """Logic row i bids for slot d of row i + 1 as row i: it beats the
    arithmetic rule of row i + 1 itself (d = a + b), whose role is lower."""
    cp = Composer(15)
    a, b = cp.var(0b1101), cp.var(0b0111)
    u = cp.var(0)
    r = cp.row({"logic_selector": 1, "q_c": 1}, 0, 0, 0, 0)
    cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_4": M1}, a, b, 0, u)
    return cp, [0, a, b], u, r


def test_tie_d_next_counts_as_the_row_whose_rule_fires():
    cp, ids, u, r = tie_d_next()
    pl, vals = solved(cp, ids, LOGIC)
    assert pl.levels == [[(u, r, ROLE_LOGIC + 4)]] and vals[u] == 0b1101 & 0b0111
    # without the logic rule the arithmetic row defines it
    pl, vals = solved(cp, ids, RANGE)
    assert pl.levels == [[(u, r + 1, 3)]] and vals[u] == 0b1101 + 0b0111


def test_tie_range_roles_come_before_logic_roles():
    """A row that is a range row and an AND row: slot a from the range rule."""
    cp = Composer(16)
    a, b, v = cp.var(0b1101), cp.var(0b0111), cp.var(0x9999)
    u = cp.var(0)
    r = cp.row({"range_selector": 1, "logic_selector": 1, "q_c": 1}, u, 0, 0, 0)
    cp.row({}, a, b, 0, v)
    pl, vals = solved(cp, [0, a, b, v], RANGE | LOGIC)
    assert pl.levels == [[(u, r, ROLE_RANGE)]] and vals[u] == 0x9999 >> 2
    pl, vals = solved(cp, [0, a, b, v], LOGIC)
    assert pl.levels == [[(u, r, ROLE_LOGIC)]] and vals[u] == 0b1101 >> 2


# ------------------------------------------------------------------ never ready, not redefined, reduction
def test_last_row_and_other_q_c_are_never_ready():
    cp = Composer(17)
    v = cp.var(77)
    u = cp.var(0)
    cp.row({}, 0, 0, 0, v)
    cp.row({"range_selector": 1}, u, 0, 0, 0)  # the last row: no next row
    assert plan_sweep(cp.rows, len(cp.vals), [0, v], (), BOTH).undetermined == [u]
    cp = Composer(18)
    a, b = cp.var(5), cp.var(6)
    u = cp.var(0)
    cp.row({"logic_selector": 1, "q_c": 2}, u, 0, 0, 0)
    cp.row({}, a, b, 0, 0)
    assert plan_sweep(cp.rows, len(cp.vals), [0, a, b], (), BOTH).undetermined == [u]


def test_a_known_slot_is_not_redefined():
    cp = Composer(19)
    cp.range_chain(2)
    last = cp.rows[-1][1][3]
    wrong = cp.rows[0][1][1]
    pl, vals = solved(cp, [0, last, wrong], RANGE)
    assert wrong not in {u for l in pl.levels for u, _, _ in l} and pl.n_range == 7
    assert vals == cp.vals


def test_xor_reaching_r_loses_one_r():
    A, B = 1 << 254, (1 << 253) + (1 << 252) + (1 << 251)
    assert A < R_MOD and B < R_MOD and R_MOD <= A ^ B < 2 * R_MOD
    cp = Composer(20)
    a, b = cp.var(A), cp.var(B)
    d = cp.var(0)
    r = cp.row({"logic_selector": M1, "q_c": M1}, 0, 0, 0, 0)
    cp.row({}, a, b, 0, d)
    pl, vals = solved(cp, [0, a, b], LOGIC)
    assert pl.levels == [[(d, r, ROLE_LOGIC + 4)]] and vals[d] == (A ^ B) - R_MOD
