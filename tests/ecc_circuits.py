"""Composer helpers for the ECC gates over values the circuit computes, laid
out as the reference's composer lays them (constraint_system/ecc/scalar_mul/
fixed_base.rs fixed_base_scalar_mul, ecc/curve_addition/variable_base_gate.rs
point_addition_gate), for the tests of the witness solver's ECC rules
(tests/solve_ecc_ref.py, tests/test_gpu_solve_ecc.py).  Built on
tests/circuits.py's Composer and gate_circuits.assert_equal: `cp.vals` already
holds the scalar's value, or the coordinates of the points that are added."""
from circuits import JJ_A, JJ_D, R_MOD, jj_add
from gate_circuits import assert_equal

IDENTITY = (0, 1)


def naf(v):
    """The width-2 NAF of the integer v >= 0, lowest digit first (find_wnaf(2))."""
    out = []
    while v:
        s = 0 if v % 2 == 0 else 1 if v % 4 == 1 else -1
        out.append(s)
        v = (v - s) // 2
    return out


def constrain_to_constant(cp, var, c):
    """composer.rs constrain_to_constant: the arithmetic row var - c = 0."""
    return cp.row({"q_arith": 1, "q_l": 1, "q_c": -c % R_MOD}, var, 0, 0, 0)


def fixed_base_mul_of(cp, scalar_var, base, num_bits=255):
    """fixed_base_scalar_mul over the variable `scalar_var` and the curve point
    `base`: row i holds the point accumulator in a, b, xy_alpha in c, the scalar
    accumulator in d and the multiple 2^(num_bits - 1 - i) base in q_l, q_r
    (q_c their product); three constant rows for the first accumulators before
    the first fixed-add row; the closing row holds the result and the last
    scalar accumulator, which assert_equal links to the scalar.  num_bits is the
    reference's 255 but for small tests.  Returns (first fixed-add row, (x, y)
    the result's variables)."""
    digits = naf(cp.vals[scalar_var])
    assert len(digits) <= num_bits  # (the reference asserts the same)
    mult = [base]
    for _ in range(num_bits - 1):
        mult.append(jj_add(mult[-1], mult[-1]))
    mult.reverse()
    pad = num_bits - len(digits)
    scalar_acc, point_acc, xy = [0] * (pad + 1), [IDENTITY] * (pad + 1), [0] * pad
    for k, s in enumerate(reversed(digits)):
        x, y = mult[pad + k]
        add = IDENTITY if s == 0 else (s * x % R_MOD, y)
        scalar_acc.append(2 * scalar_acc[-1] + s)
        point_acc.append(jj_add(point_acc[-1], add))
        xy.append(add[0] * add[1] % R_MOD)
    first = None
    for i in range(num_bits):
        ax, ay, bit = cp.var(point_acc[i][0]), cp.var(point_acc[i][1]), cp.var(scalar_acc[i])
        if i == 0:
            constrain_to_constant(cp, ax, 0)
            constrain_to_constant(cp, ay, 1)
            constrain_to_constant(cp, bit, 0)
        xb, yb = mult[i]
        r = cp.row({"fixed_group_add_selector": 1, "q_l": xb, "q_r": yb, "q_c": xb * yb % R_MOD},
                   ax, ay, cp.var(xy[i]), bit)
        first = r if first is None else first
    ax, ay = cp.var(point_acc[num_bits][0]), cp.var(point_acc[num_bits][1])
    last = cp.var(scalar_acc[num_bits])
    cp.row({"q_arith": 1}, ax, ay, 0, last)
    assert_equal(cp, last, scalar_var)
    return first, (ax, ay)


def _div(n, d):
    return n * pow(d, -1, R_MOD) % R_MOD if d % R_MOD else 0


def point_add_of(cp, p, q):
    """point_addition_gate over the points p = (x1, y1), q = (x2, y2) (pairs of
    variables): the var-add row (x1, y1, x2, y2) and the row (x3, y3, 0, x1 y2)
    after it.  A zero denominator (points that are not on the curve) gives the
    coordinate 0.  Returns (the var-add row, (x3, y3) as variables)."""
    x1, y1, x2, y2 = (cp.vals[v] for v in (*p, *q))
    t = JJ_D * x1 * y2 * y1 * x2 % R_MOD
    x1y2 = cp.var(x1 * y2)
    x3 = cp.var(_div(x1 * y2 + y1 * x2, 1 + t))
    y3 = cp.var(_div(y1 * y2 - JJ_A * x1 * x2, 1 - t))
    r = cp.row({"variable_group_add_selector": 1}, p[0], p[1], q[0], q[1])
    cp.row({}, x3, y3, 0, x1y2)
    return r, (x3, y3)
