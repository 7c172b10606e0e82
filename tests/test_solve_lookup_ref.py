"""The plain-integer model of the lookup rule (tests/solve_lookup_ref.py) against
the composer's own values (tests/lookup_circuits.py lays the rows as the
reference's composer does), the sweep against the counter form, and the tie and
padding rules one by one.  No GPU: tests/test_gpu_solve_lookup.py holds the
library to this model, over the circuits built here."""
import functools

import pytest

from circuits import Composer, R_MOD, jj_point
from ecc_circuits import constrain_to_constant, fixed_base_mul_of, point_add_of
from gate_circuits import M1, range_of
from lookup_circuits import add_table, domain_of, lookup_of, mixed_table, random_table, xor_table
from solve_ecc_ref import FIXED_ADD, VAR_ADD
from solve_gates_ref import LOGIC, RANGE
from solve_lookup_ref import (LOOKUP, ROLE_LOOKUP, bucket, buckets_of, indexed_rows, lookup, n_buckets, padded_table,
                              plan, plan_sweep, solve)

ECC = FIXED_ADD | VAR_ADD
GATES = RANGE | LOGIC


def solved(cp, ids, lk=LOOKUP, ecc=0, gates=0, outputs=(), vals=None, sweep=True):
    """(plan, solution) of the model from the values cp holds (or `vals`) for ids."""
    n_vars = len(cp.vals)
    pl = (plan_sweep if sweep else plan)(cp.rows, n_vars, ids, outputs, gates, ecc, lk)
    vals = cp.vals if vals is None else vals
    return pl, solve(cp.rows, pl, n_vars, {u: vals[u] for u in ids}, None, outputs, cp.table, domain_of(cp))


def plans_equal(a, b):
    return a.levels == b.levels and a.undetermined == b.undetermined


def const_var(cp, v):
    """A variable an arithmetic row constrains to the constant v (so the solver defines it)."""
    u = cp.var(v)
    constrain_to_constant(cp, u, v)
    return u


def add_row(cp, a, b):
    """c = a + b through an arithmetic row; returns c."""
    c = cp.var(cp.vals[a] + cp.vals[b])
    cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, a, b, c, 0)
    return c


# ------------------------------------------------------------------ the circuits (shared with the GPU tests)
def computed_operands(seed=51):
    """x = p + q, y = 2 u + 1, z = x ^ y through a 4-bit XOR table (256 rows),
    w = z + p.  Returns (cp, ids, (p, q, u, x, y, z, w), the lookup row)."""
    cp = Composer(seed)
    cp.table = xor_table(4)
    m1 = const_var(cp, M1)
    p, q, u = cp.var(3), cp.var(9), cp.var(5)
    x = add_row(cp, p, q)
    y = cp.var(2 * cp.vals[u] + 1)
    cp.row({"q_arith": 1, "q_l": 2, "q_c": 1, "q_o": M1}, u, 0, y, 0)
    r, z = lookup_of(cp, x, y, m1)
    w = add_row(cp, z, p)
    return cp, [0, p, q, u], (p, q, u, x, y, z, w), r


@functools.lru_cache(maxsize=None)
def every_row_query(n_rows=200, seed=52):
    """A random table, every row's key an input and a query: one level of
    n_rows lookups.  Returns (cp, ids, [the looked-up variables])."""
    cp = Composer(seed)
    random_table(cp, n_rows)
    ids, out = [0], []
    for t in list(cp.table):
        a, b, d = cp.var(t[0]), cp.var(t[1]), cp.var(t[3])
        out.append(lookup_of(cp, a, b, d)[1])
        ids += [a, b, d]
    return cp, ids, out


def duplicate_keys(lower_is_row_0, seed=53):
    """Six random rows, two of which share (a, b, d) and differ in c; every
    row's key is queried.  Returns (cp, ids, [c variables], (lower, upper))."""
    cp = Composer(seed)
    random_table(cp, 6)
    lo, hi = (0, 3) if lower_is_row_0 else (2, 5)
    t = cp.table
    t[hi] = [t[lo][0], t[lo][1], (t[lo][2] + 1) % R_MOD, t[lo][3]]
    ids, out = [0], []
    for row in list(t):
        a, b, d = cp.var(row[0]), cp.var(row[1]), cp.var(row[3])
        out.append(lookup_of(cp, a, b, d)[1])
        ids += [a, b, d]
    return cp, ids, out, (lo, hi)


def no_such_key(seed=54):
    """a = p + q looked up against b in a 2-bit XOR table: p + q above 3 is no
    key.  Returns (cp, ids, (p, q, b, a, z), the lookup row)."""
    cp = Composer(seed)
    cp.table = xor_table(2)
    m1 = const_var(cp, M1)
    p, q, b = cp.var(1), cp.var(2), cp.var(1)
    a = add_row(cp, p, q)
    r, z = lookup_of(cp, a, b, m1)
    return cp, [0, p, q, b], (p, q, b, a, z), r


def zero_d(seed=55):
    """lookup_gate(a, b, c, None) against an addition table (column 3 = 0).
    Returns (cp, ids, [(a, b, c)])."""
    cp = Composer(seed)
    cp.table = add_table(2)
    ids, out = [0], []
    for va, vb in ((0, 0), (3, 3), (1, 2), (2, 3)):
        a, b = cp.var(va), cp.var(vb)
        out.append((a, b, lookup_of(cp, a, b, None)[1]))
        ids += [a, b]
    return cp, ids, out


def mixed_ops(seed=56):
    """3 op 2 for the four operations of a mixed table, column 3 choosing.
    Returns (cp, ids, {d value: c variable})."""
    cp = Composer(seed)
    cp.table = mixed_table(2)
    a, b = cp.var(3), cp.var(2)
    out = {}
    for dv in (0, 1, M1, 2):
        d = None if dv == 0 else const_var(cp, dv)
        out[dv] = lookup_of(cp, a, b, d)[1]
    return cp, [0, a, b], out


@functools.lru_cache(maxsize=None)
def wide_lookups(n=300, seed=57):
    """n independent 4-bit XORs of inputs: one level of n lookup entries."""
    cp = Composer(seed)
    cp.table = xor_table(4)
    m1 = cp.var(M1)
    ids = [0, m1]
    for k in range(n):
        a, b = cp.var(k % 16), cp.var((7 * k + 3) % 16)
        lookup_of(cp, a, b, m1)
        ids += [a, b]
    return cp, ids


@functools.lru_cache(maxsize=None)
def four_segments(seed=58):
    """100 arithmetic entries, 25 range rows (100 gate entries), 100 var-add
    rows and 100 lookups, all in one level."""
    cp = Composer(seed)
    cp.table = xor_table(2)
    m1 = cp.var(M1)
    ids = [0, m1]
    for k in range(100):
        x = cp.var(cp.rnd())
        cp.row({"q_arith": 1, "q_l": 5, "q_c": 7, "q_r": M1}, x, cp.var(5 * cp.vals[x] + 7), 0, 0)
        pv, qv = [tuple(cp.var(c) for c in jj_point(cp.rng)) for _ in range(2)]
        point_add_of(cp, pv, qv)
        a, b = cp.var(k % 4), cp.var((k // 4) % 4)
        lookup_of(cp, a, b, m1)
        ids += [x, *pv, *qv, a, b]
        if k < 25:
            v = cp.var(cp.rnd())
            cp.row({"range_selector": 1}, *(cp.var(cp.vals[v] >> s) for s in (2, 4, 6, 8)))
            cp.row({}, 0, 0, 0, v)
            ids.append(v)
    return cp, ids


@functools.lru_cache(maxsize=None)
def chain(others, n=40, seed=59):
    """z_(k+1) = z_k ^ b_k through a 4-bit XOR table, n times: each lookup's
    output is the next one's key.  others: "" (alone), "gates" (a range
    decomposition of p + q beside it) or "ecc" (that, and a multiplication of
    p + q and a point addition).  Returns (cp, ids, the last z)."""
    cp = Composer(seed)
    cp.table = xor_table(4)
    m1 = cp.var(M1)
    z = cp.var(5)
    ids = [0, m1, z]
    for k in range(n):
        b = cp.var((3 * k + 1) % 16)
        ids.append(b)
        z = lookup_of(cp, z, b, m1)[1]
    if others:
        p, q = cp.var(100), cp.var(70)
        s = add_row(cp, p, q)
        ids += [p, q]
        range_of(cp, s, 8)
        if others == "ecc":
            _, res = fixed_base_mul_of(cp, s, jj_point(cp.rng), 8)
            qv = tuple(cp.var(c) for c in jj_point(cp.rng))
            point_add_of(cp, res, qv)
            ids += list(qv)
    return cp, ids, z


def tie_lookup_and_arith(arith_first, seed=60):
    """c = a + 2 by an arithmetic row and c = a ^ b by a lookup row, ready in
    the same round.  Returns (cp, ids, (a, b, c), (arithmetic row, lookup row))."""
    cp = Composer(seed)
    cp.table = xor_table(2)
    m1 = cp.var(M1)
    a, b, c = cp.var(1), cp.var(2), cp.var(3)
    q = {"q_arith": 1, "q_l": 1, "q_c": 2, "q_o": M1}
    if arith_first:
        ra, rl = cp.row(q, a, 0, c, 0), cp.row({"q_lookup": 1}, a, b, c, m1)
    else:
        rl, ra = cp.row({"q_lookup": 1}, a, b, c, m1), cp.row(q, a, 0, c, 0)
    return cp, [0, m1, a, b], (a, b, c), (ra, rl)


def tie_on_one_row(seed=61):
    """One row with q_arith and q_lookup: c = a + 2 and c = a ^ b."""
    cp = Composer(seed)
    cp.table = xor_table(2)
    m1 = cp.var(M1)
    a, b, c = cp.var(1), cp.var(2), cp.var(3)
    r = cp.row({"q_arith": 1, "q_lookup": 1, "q_l": 1, "q_c": 2, "q_o": M1}, a, b, c, m1)
    return cp, [0, m1, a, b], (a, b, c), r


def last_row_lookup(seed=62):
    """A lookup on the last gate row of a full domain (4 rows, D = 4)."""
    cp = Composer(seed)
    cp.table = xor_table(1)
    m1 = cp.var(M1)
    ids, out = [0, m1], []
    for va, vb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        a, b = cp.var(va), cp.var(vb)
        out.append(lookup_of(cp, a, b, m1)[1])
        ids += [a, b]
    return cp, ids, out


CIRCUITS = {
    "computed_operands": lambda: (computed_operands()[:2], 0, 0),
    "every_row_query": lambda: (every_row_query()[:2], 0, 0),
    "duplicate_keys": lambda: (duplicate_keys(False)[:2], 0, 0),
    "duplicate_keys_row_0": lambda: (duplicate_keys(True)[:2], 0, 0),
    "no_such_key": lambda: (no_such_key()[:2], 0, 0),
    "zero_d": lambda: (zero_d()[:2], 0, 0),
    "mixed_ops": lambda: (mixed_ops()[:2], 0, 0),
    "wide_lookups": lambda: (wide_lookups(), 0, 0),
    "four_segments": lambda: (four_segments(), ECC, RANGE),
    "chain": lambda: (chain("")[:2], 0, 0),
    "chain_gates": lambda: (chain("gates")[:2], 0, RANGE),
    "chain_ecc": lambda: (chain("ecc")[:2], ECC, RANGE),
    "tie_arith_lower": lambda: (tie_lookup_and_arith(True)[:2], 0, 0),
    "tie_lookup_lower": lambda: (tie_lookup_and_arith(False)[:2], 0, 0),
    "tie_on_one_row": lambda: (tie_on_one_row()[:2], 0, 0),
    "last_row_lookup": lambda: (last_row_lookup()[:2], 0, 0),
}


# ------------------------------------------------------------------ the model against the composer
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_sweep_equals_counters_and_the_solution_is_the_composers(name):
    (cp, ids), ecc, gates = CIRCUITS[name]()
    pl, vals = solved(cp, ids, LOOKUP, ecc, gates)
    assert plans_equal(pl, plan(cp.rows, len(cp.vals), ids, (), gates, ecc, LOOKUP))
    assert pl.undetermined == [] and vals == cp.vals
    assert pl.n_solved == sum(pl.widths) == len(cp.vals) - len(ids)
    assert all(a + g + e + k == w for a, g, e, k, w in
               zip(pl.arith_widths, pl.gate_widths, pl.ecc_widths, pl.lookup_widths, pl.widths))


def test_computed_operands_levels_and_other_inputs():
    cp, ids, (p, q, u, x, y, z, w), r = computed_operands()
    pl, vals = solved(cp, ids)
    assert pl.lookup_widths == [0, 1, 0] and pl.n_lookup == 1 and pl.levels[1] == [(z, r, ROLE_LOOKUP)]
    assert (vals[x], vals[y], vals[z], vals[w]) == (12, 11, 7, 10)
    other = list(cp.vals)
    other[p], other[q], other[u] = 1, 2, 7
    assert solved(cp, ids, vals=other)[1][z] == 3 ^ 15
    # without the flag the variable and what follows it stay undetermined
    none, _ = solved(cp, ids, 0)
    assert none.undetermined == [z, w] and none.n_solved == 3


def test_every_row_of_a_table_and_its_buckets():
    cp, ids, out = every_row_query()
    pl, vals = solved(cp, ids)
    assert pl.lookup_widths == [200] and [vals[c] for c in out] == [t[2] for t in cp.table]
    D = domain_of(cp)
    assert D == 256 and indexed_rows(cp.table, D) == list(range(200)) and n_buckets(200) == 512
    bk = buckets_of(cp.table, D)
    assert sum(len(v) for v in bk.values()) == 200 and max(len(v) for v in bk.values()) >= 2
    assert all(v == sorted(v) for v in bk.values())


@pytest.mark.parametrize("row_0", [False, True], ids=["rows_2_5", "rows_0_3"])
def test_of_two_rows_with_one_key_the_lower_defines(row_0):
    cp, ids, out, (lo, hi) = duplicate_keys(row_0)
    pl, vals = solved(cp, ids)
    assert vals[out[lo]] == vals[out[hi]] == cp.table[lo][2] != cp.table[hi][2]
    assert indexed_rows(cp.table, domain_of(cp)) == list(range(6))  # (the upper row differs from row 0 in c)


def test_padding_copies_of_row_0_are_not_indexed_and_change_no_answer():
    table = [[1, 2, 3, 4], [5, 6, 7, 8], [1, 2, 3, 4], [1, 2, 9, 4]]
    t = padded_table(table, 8)
    assert t[4:] == [t[0]] * 4 and indexed_rows(table, 8) == [0, 1, 3]
    assert lookup(table, 8, 1, 2, 4) == 3 and lookup(table, 8, 5, 6, 8) == 7 and lookup(table, 8, 5, 6, 7) == 0
    # an empty table is D zero rows: the zero key is held, with value 0
    assert padded_table([], 4) == [(0, 0, 0, 0)] * 4 and indexed_rows([], 4) == [0]
    assert bucket(1, 2, 4, 8) == bucket(1 + R_MOD, 2, 4, 8) < 8


def test_a_key_the_table_does_not_hold_defines_zero():
    cp, ids, (p, q, b, a, z), r = no_such_key()
    other = list(cp.vals)
    other[p], other[q] = 2, 2
    pl, vals = solved(cp, ids, vals=other)
    assert vals[a] == 4 and vals[z] == 0 and solved(cp, ids)[1][z] == 3 ^ 1


def test_zero_d_and_the_operations_of_a_mixed_table():
    cp, ids, out = zero_d()
    _, vals = solved(cp, ids)
    assert [vals[c] for _, _, c in out] == [0, 2, 3, 1]
    cp, ids, out = mixed_ops()
    _, vals = solved(cp, ids)
    assert {d: vals[c] for d, c in out.items()} == {0: 1, 1: 2, M1: 1, 2: 2}


def test_widths():
    cp, ids = wide_lookups()
    pl, _ = solved(cp, ids, sweep=False)
    assert pl.lookup_widths == [300] and domain_of(cp) == 512
    cp, ids = four_segments()
    pl, _ = solved(cp, ids, LOOKUP, ECC, RANGE, sweep=False)
    assert (pl.arith_widths, pl.gate_widths, pl.ecc_widths, pl.lookup_widths) == ([100], [100], [300], [100])
    for others, ecc, gates in (("", 0, 0), ("gates", 0, RANGE), ("ecc", ECC, RANGE)):
        cp, ids, z = chain(others)
        pl, vals = solved(cp, ids, LOOKUP, ecc, gates, sweep=False)
        assert pl.lookup_widths[:40] == [1] * 40 and pl.n_lookup == 40 and pl.max_width <= 256
        assert vals[z] == cp.vals[z]
        if others == "ecc":
            assert pl.n_fixed and pl.n_var == 3 and pl.n_range and any(
                k and e for k, e in zip(pl.lookup_widths, pl.ecc_widths))


@pytest.mark.parametrize("arith_first", [True, False], ids=["arith_lower", "lookup_lower"])
def test_tie_between_an_arithmetic_and_a_lookup_row_goes_to_the_lower_row(arith_first):
    cp, ids, (a, b, c), (ra, rl) = tie_lookup_and_arith(arith_first)
    other = list(cp.vals)
    other[b] = 1  # a + 2 = 3, a ^ b = 0
    pl, vals = solved(cp, ids, vals=other)
    assert pl.levels == [[(c, ra, 2)]] if arith_first else pl.levels == [[(c, rl, ROLE_LOOKUP)]]
    assert vals[c] == (3 if arith_first else 0) and pl.n_lookup == (0 if arith_first else 1)


def test_tie_on_one_row_goes_to_the_arithmetic_slot():
    cp, ids, (a, b, c), r = tie_on_one_row()
    other = list(cp.vals)
    other[b] = 1
    pl, vals = solved(cp, ids, vals=other)
    assert pl.levels == [[(c, r, 2)]] and vals[c] == 3 and pl.n_lookup == 0


def test_a_known_slot_c_is_not_redefined():
    cp, ids, (p, q, u, x, y, z, w), r = computed_operands()
    given = list(cp.vals)
    given[z] = 9
    pl, vals = solved(cp, ids + [z], vals=given)
    assert vals[z] == 9 and pl.n_lookup == 0 and vals[w] == 12


def test_an_output_row_with_q_lookup_does_not_bid():
    cp, ids, (a, b, c), r = tie_on_one_row()
    pl = plan_sweep(cp.rows, len(cp.vals), ids, [r], 0, 0, LOOKUP)
    assert pl.levels == [] and pl.undetermined == [c]


def test_the_last_gate_row_takes_part():
    cp, ids, out = last_row_lookup()
    assert len(cp.rows) == domain_of(cp) == 4
    pl, vals = solved(cp, ids)
    assert pl.lookup_widths == [4] and [vals[c] for c in out] == [0, 1, 1, 0]
