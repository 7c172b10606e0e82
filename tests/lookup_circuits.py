"""Composer helpers for lookup gates over values the circuit computes, laid out
as the reference's composer lays them (lookup/lookup_table.rs xor_table and the
insert_multi_* builders, constraint_system/composer.rs lookup_gate), for the
tests of the witness solver's lookup rule (tests/solve_lookup_ref.py,
tests/test_gpu_solve_lookup.py).  Built on tests/circuits.py's Composer:
`cp.table` holds the table rows, `cp.vals` the values of the key's variables."""
from circuits import R_MOD
from gate_circuits import M1
import solve_lookup_ref


def domain_of(cp):
    """The domain a circuit that is preprocessed as it stands gets: D rows."""
    D = 1
    while D < max(len(cp.rows), len(cp.table)):
        D <<= 1
    return D


def xor_table(n):
    """LookupTable::xor_table(0, n): (a, b, a ^ b, -1) for a, b below 2^n."""
    ub = 1 << n
    return [[a, b, (a ^ b) % ub, M1] for a in range(ub) for b in range(ub)]


def add_table(n):
    """LookupTable::add_table(0, n): (a, b, a + b mod 2^n, 0)."""
    ub = 1 << n
    return [[a, b, (a + b) % ub, 0] for a in range(ub) for b in range(ub)]


def mixed_table(n):
    """insert_multi_add, _mul, _xor and _and over 0 .. 2^n - 1, one after the
    other: column 3 tells the operation (0 add, 1 mul, -1 xor, 2 and)."""
    ub = 1 << n
    ops = ((lambda a, b: a + b, 0), (lambda a, b: a * b, 1), (lambda a, b: a ^ b, M1), (lambda a, b: a & b, 2))
    return [[a, b, op(a, b) % ub, d] for op, d in ops for a in range(ub) for b in range(ub)]


def random_table(cp, rows):
    """`rows` rows of four random field elements (Composer.lookup_table)."""
    cp.lookup_table(rows)
    return cp.table


def lookup_of(cp, a, b, d=None, D=None):
    """c = LookupTable::lookup(a, b, d) over cp.table, then lookup_gate(a, b, c,
    d) for the existing variables a, b, d (d None: the zero variable, as
    lookup_gate(.., None)).  A key the table does not hold gives the value 0.
    Returns (the row, the variable c)."""
    d = 0 if d is None else d
    D = D or max(len(cp.table), 1)
    c = cp.var(solve_lookup_ref.lookup(cp.table, D, cp.vals[a], cp.vals[b], cp.vals[d]))
    return cp.row({"q_lookup": 1}, a, b, c, d), c
