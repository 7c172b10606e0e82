"""The plain-integer model of the ECC rules (tests/solve_ecc_ref.py) against
the composer's own values (tests/ecc_circuits.py lays the rows as the
reference's composer does), the sweep against the counter form, and the tie
rules one by one.  No GPU: tests/test_gpu_solve_ecc.py holds the library to
this model."""
import functools

import pytest

from circuits import Composer, JJ_D, R_MOD, jj_add, jj_point
from ecc_circuits import fixed_base_mul_of, naf, point_add_of
from gate_circuits import M1, range_of
from solve_ecc_ref import (FIXED_ADD, ROLE_FIXED, ROLE_VAR, VAR_ADD, naf_digit, plan, plan_sweep, solve)
from solve_gates_ref import LOGIC, RANGE
import solve_gates_ref

ECC = FIXED_ADD | VAR_ADD
GATES = RANGE | LOGIC


def solved(cp, ids, ecc=ECC, gates=0, outputs=(), vals=None, sweep=True):
    n_vars = len(cp.vals)
    pl = (plan_sweep if sweep else plan)(cp.rows, n_vars, ids, outputs, gates, ecc)
    vals = cp.vals if vals is None else vals
    return pl, solve(cp.rows, pl, n_vars, {u: vals[u] for u in ids}, None, outputs)


def plans_equal(a, b):
    return a.levels == b.levels and a.undetermined == b.undetermined


def scalar_mul(seed, scalar, num_bits):
    """One multiplication of an input scalar: (cp, ids, scalar variable, result)."""
    cp = Composer(seed)
    s = cp.var(scalar)
    _, res = fixed_base_mul_of(cp, s, jj_point(cp.rng), num_bits)
    return cp, [0, s], s, res


# ------------------------------------------------------------------ the model against the composer
@pytest.mark.parametrize("scalar", [0, 1, 3, 170, None])
def test_small_multiplications(scalar):
    seed = 80 + (scalar or 7)
    if scalar is None:
        scalar = int(Composer(seed).rng.integers(0, 171))
    cp, ids, s, res = scalar_mul(seed, scalar, 8)
    pl, vals = solved(cp, ids)
    assert pl.undetermined == [] and vals == cp.vals
    assert plans_equal(pl, plan(cp.rows, len(cp.vals), ids, (), 0, ECC))
    # the constants and the last accumulator, the scalar chain up to row 1, the point chain down
    assert len(pl.levels) == 1 + 7 + 8
    assert pl.n_fixed == 7 + 8 + 16 and pl.n_var == 0 and pl.n_range == pl.n_logic == 0
    # without the flag nothing but the arithmetic rows moves
    assert plan_sweep(cp.rows, len(cp.vals), ids, (), GATES, VAR_ADD).n_solved == 4


@functools.lru_cache(maxsize=None)
def full_multiplication(scalar=(1 << 254) - 1):
    """One 255-row multiplication of p + q = scalar: (cp, ids, result)."""
    cp = Composer(91)
    p = cp.var(scalar // 3)
    q = cp.var(scalar - scalar // 3)
    s = cp.var(scalar)
    cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, p, q, s, 0)
    _, res = fixed_base_mul_of(cp, s, jj_point(cp.rng))
    return cp, [0, p, q], res


@pytest.mark.parametrize("which", ["2^254 - 1", "random"])
def test_full_multiplications(which):
    if which == "random":
        scalar = int.from_bytes(Composer(92).rng.bytes(32), "little") % (1 << 254)
        cp, ids, res = full_multiplication(scalar)
    else:
        cp, ids, res = full_multiplication()
    pl, vals = solved(cp, ids, sweep=False)
    assert pl.undetermined == [] and vals == cp.vals
    # the constants and the scalar, its last accumulator, 254 rows up, 255 rows down
    assert len(pl.levels) == 2 + 254 + 255


def test_a_point_addition():
    cp = Composer(93)
    p, q = jj_point(cp.rng), jj_point(cp.rng)
    pv, qv = (cp.var(p[0]), cp.var(p[1])), (cp.var(q[0]), cp.var(q[1]))
    r, res = point_add_of(cp, pv, qv)
    assert (cp.vals[res[0]], cp.vals[res[1]]) == jj_add(p, q)
    ids = [0, *pv, *qv]
    pl, vals = solved(cp, ids)
    assert vals == cp.vals and pl.levels == [sorted([(res[0], r, ROLE_VAR), (res[1], r, ROLE_VAR + 1),
                                                     (cp.rows[r + 1][1][3], r, ROLE_VAR + 2)])]
    assert (pl.n_fixed, pl.n_var) == (0, 3)
    assert plan_sweep(cp.rows, len(cp.vals), ids, (), GATES, FIXED_ADD).levels == []


def mixed_circuit(num_bits=8):
    """scalar = p + q; R = scalar B; S = R + Q through a var-add row; w = 3 S.x
    + 1; an output row PI = -w; a range row over the scalar.  Returns (cp,
    ids, output row)."""
    cp = Composer(94)
    p, q = cp.var(100), cp.var(70)
    s = cp.var(170)
    cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, p, q, s, 0)
    _, res = fixed_base_mul_of(cp, s, jj_point(cp.rng), num_bits)
    pt = jj_point(cp.rng)
    qv = (cp.var(pt[0]), cp.var(pt[1]))
    _, total = point_add_of(cp, res, qv)
    w = cp.var(3 * cp.vals[total[0]] + 1)
    cp.row({"q_arith": 1, "q_l": 3, "q_c": 1, "q_o": M1}, total[0], 0, w, 0)
    out = cp.row({"q_arith": 1, "q_l": 1}, w, 0, 0, 0)
    cp.pis[out] = -cp.vals[w] % R_MOD
    range_of(cp, s, 8)
    return cp, [0, p, q, *qv], out


def test_a_mix_of_every_family():
    cp, ids, out = mixed_circuit()
    pl, vals = solved(cp, ids, ECC, GATES, [out])
    assert pl.undetermined == [] and vals == cp.vals
    assert plans_equal(pl, plan(cp.rows, len(cp.vals), ids, [out], GATES, ECC))
    assert pl.n_var == 3 and pl.n_fixed == 31 and pl.n_range == 3 and pl.n_logic == 0  # (the first d is variable 0)
    import solve_outputs_ref
    assert solve_outputs_ref.derive(cp.rows, vals, [out]) == cp.pis
    # ecc = 0 is the gate model
    a = plan_sweep(cp.rows, len(cp.vals), ids, [out], GATES, 0)
    b = solve_gates_ref.plan_sweep(cp.rows, len(cp.vals), ids, [out], GATES)
    assert plans_equal(a, b) and (a.n_fixed, a.n_var, a.n_range) == (0, 0, b.n_range)


# ------------------------------------------------------------------ the NAF digit
def test_the_digit_rule_is_the_naf():
    rng = Composer(95).rng
    for v in [0, 1, 2, 3, 170, 171, (1 << 254) - 1, R_MOD - 1] + [int.from_bytes(rng.bytes(32), "little") % R_MOD
                                                                 for _ in range(50)]:
        # the NAF directly: digit k is bit k of 3 v minus bit k of v, read one place up
        direct = [((3 * v >> (k + 1)) & 1) - ((v >> (k + 1)) & 1) for k in range((3 * v).bit_length())]
        while direct and direct[-1] == 0:
            direct.pop()
        assert naf(v) == direct
        assert all(x == 0 or y == 0 for x, y in zip(direct, direct[1:]))
        assert sum(d << k for k, d in enumerate(direct)) == v
        acc, k = v, 0
        while acc:
            assert naf_digit(acc) == direct[k] and acc + 1 <= R_MOD
            acc, k = (acc - naf_digit(acc)) // 2, k + 1


# ------------------------------------------------------------------ ties
def tie_point_and_arith(arith_first):
    """a_next of a fixed-add row is also the one unknown of u = s + 1; both are ready in round 1."""
    cp = Composer(96)
    s = cp.var(cp.rnd())
    pt = jj_point(cp.rng)
    ax, ay, u, by = cp.var(pt[0]), cp.var(pt[1]), cp.var(0), cp.var(0)
    d0, d1 = cp.var(5), cp.var(11)

    def arith():
        return cp.row({"q_arith": 1, "q_l": 1, "q_c": 1, "q_o": M1}, s, 0, u, 0)

    ra = arith() if arith_first else None
    xb, yb = jj_point(cp.rng)
    rf = cp.row({"fixed_group_add_selector": 1, "q_l": xb, "q_r": yb, "q_c": xb * yb % R_MOD}, ax, ay, 0, d0)
    cp.row({}, u, by, 0, d1)
    ra = arith() if ra is None else ra
    return cp, [0, s, ax, ay, d0, d1], u, ra, rf, (pt, (xb, yb))


@pytest.mark.parametrize("arith_first", [True, False], ids=["arith_lower", "fixed_lower"])
def test_tie_the_lower_row_wins_across_families(arith_first):
    cp, ids, u, ra, rf, (pt, base) = tie_point_and_arith(arith_first)
    pl, vals = solved(cp, ids)
    assert (u, ra, 2) in pl.levels[0] if arith_first else (u, rf, ROLE_FIXED + 2) in pl.levels[0]
    assert pl.undetermined == []
    # bit = 11 - 2 * 5 = 1: the accumulator plus the base
    assert vals[u] == ((cp.vals[ids[1]] + 1) % R_MOD if arith_first else jj_add(pt, base)[0])


def tie_var_roles():
    """The next row of a var-add row holds one variable in a and in d: a_next (the lower role) defines it."""
    cp = Composer(97)
    p, q = jj_point(cp.rng), jj_point(cp.rng)
    v = [cp.var(c) for c in (*p, *q)]
    u, y3 = cp.var(0), cp.var(0)
    r = cp.row({"variable_group_add_selector": 1}, *v)
    cp.row({}, u, y3, 0, u)
    return cp, [0, *v], u, r, jj_add(p, q)


def test_tie_two_roles_of_one_var_add_row():
    cp, ids, u, r, total = tie_var_roles()
    pl, vals = solved(cp, ids)
    assert pl.levels == [sorted([(u, r, ROLE_VAR), (u + 1, r, ROLE_VAR + 1)])] and pl.n_var == 2
    assert (vals[u], vals[u + 1]) == total


def tie_both_families_on_one_row():
    """A row with both selectors: fixed-add's a_next and b_next come before var-add's; d_next is var-add's
    (slot d of the next row is unknown, so of the fixed-add rules only ... none is ready but var-add)."""
    cp = Composer(98)
    p, q = jj_point(cp.rng), jj_point(cp.rng)
    v = [cp.var(c) for c in (*p, *q)]
    x3, y3, dn = cp.var(0), cp.var(0), cp.var(0)
    xb, yb = jj_point(cp.rng)
    r = cp.row({"variable_group_add_selector": 1, "fixed_group_add_selector": 1, "q_l": xb, "q_r": yb,
                "q_c": xb * yb % R_MOD}, *v)
    cp.row({}, x3, y3, 0, dn)
    return cp, [0, *v], (x3, y3, dn), r, (p, q, (xb, yb))


def test_tie_fixed_add_roles_come_before_var_add_roles():
    cp, ids, (x3, y3, dn), r, (p, q, base) = tie_both_families_on_one_row()
    # round 1: d_next is unknown, so only var-add is ready and defines all three
    pl, vals = solved(cp, ids)
    assert pl.levels == [sorted([(x3, r, ROLE_VAR), (y3, r, ROLE_VAR + 1), (dn, r, ROLE_VAR + 2)])]
    assert (vals[x3], vals[y3]) == jj_add(p, q) and vals[dn] == p[0] * q[1] % R_MOD
    # with d_next an input both are ready: the fixed-add point rule wins a_next and b_next
    given = list(cp.vals)
    given[dn] = (2 * q[1] + 1) % R_MOD  # bit = 1
    pl, vals = solved(cp, ids + [dn], vals=given)
    assert pl.levels == [sorted([(x3, r, ROLE_FIXED + 2), (y3, r, ROLE_FIXED + 3)])] and (pl.n_fixed, pl.n_var) == (2, 0)
    assert (vals[x3], vals[y3]) == jj_add(p, base)


def test_a_point_slot_listed_as_input_keeps_its_value():
    cp, ids, s, res = scalar_mul(99, 170, 8)
    mid = cp.rows[fixed_rows(cp)[4]][1][0]  # the x accumulator of the fifth fixed-add row
    given = list(cp.vals)
    given[mid] = 12345
    pl, vals = solved(cp, ids + [mid], vals=given)
    assert pl.undetermined == [] and vals[mid] == 12345 and pl.n_fixed == 7 + 8 + 15
    assert [v for k, v in enumerate(vals) if k < mid] == cp.vals[:mid]


def fixed_rows(cp):
    return [i for i, (q, _) in enumerate(cp.rows) if q.get("fixed_group_add_selector")]


# ------------------------------------------------------------------ never ready
def last_row_circuits():
    """A var-add and a fixed-add row that are the last gate: no next row."""
    out = []
    for sel in ({"variable_group_add_selector": 1}, {"fixed_group_add_selector": 1, "q_l": 3, "q_r": 4, "q_c": 12}):
        cp = Composer(100)
        v = [cp.var(k + 2) for k in range(3)]
        u = cp.var(0)
        cp.row({}, 0, 0, 0, v[0])
        cp.row(sel, v[0], v[1], u, v[2])
        out.append((cp, [0, *v], u))
    return out


def test_an_ecc_row_on_the_last_row_defines_nothing():
    for cp, ids, u in last_row_circuits():
        pl, _ = solved(cp, ids)
        assert pl.levels == [] and pl.undetermined == [u]


def zero_denominator():
    """Two points with 1 + t = 0: y2 = -1 / (D x1 y1 x2)."""
    cp = Composer(101)
    x1, y1 = jj_point(cp.rng)
    x2 = cp.rnd()
    y2 = -pow(JJ_D * x1 * y1 * x2 % R_MOD, -1, R_MOD) % R_MOD
    pv, qv = (cp.var(x1), cp.var(y1)), (cp.var(x2), cp.var(y2))
    r, res = point_add_of(cp, pv, qv)
    return cp, [0, *pv, *qv], r, res


def test_a_zero_denominator_gives_zero():
    cp, ids, r, res = zero_denominator()
    pl, vals = solved(cp, ids)
    assert vals == cp.vals and vals[res[0]] == 0 and vals[res[1]] != 0
