"""Circuits whose copy permutations the Merkle circuit does not have, for the
model of the copy-group builder (tests/groups_ref.py, tests/test_groups_ref.py)
and the directed GPU tests of it (tests/test_gpu_groups.py).

Built row by row (Composer.row / Composer.arith) and handed to
GeneralInputs(cp, n) directly: Composer.build() pads with zero-variable gate
rows, which would put one giant cross-wire cycle into every case.  The prover's
domain is next_pow2(gates), so every case has n/2 < gates <= n.  Most rows are
selector-free (every selector zero: any values satisfy them), so the witness
satisfies whatever the variables hold; variable 0 (the constant zero) is never
used, every slot is given a variable of its own or a shared one with a random
(non-zero, distinct) value."""
import functools

import numpy as np

from circuits import Composer, GeneralInputs, sigma_columns
from groups_ref import GroupModel


class Case:
    def __init__(self, cp, n, cycle_seed=None, **facts):
        assert n // 2 < len(cp.rows) <= n
        self.cp, self.n, self.cycle_seed = cp, n, cycle_seed
        self.facts = facts  # what the builder knows about its rows (for the tests)

    @functools.cached_property
    def model(self) -> GroupModel:
        return GroupModel(sigma_columns(self.cp, self.n, self.cycle_seed), self.n)

    @functools.cached_property
    def inputs(self) -> GeneralInputs:
        """(made once: never mutated by a test)"""
        return GeneralInputs(self.cp, self.n, self.cycle_seed)

    @functools.cached_property
    def oracle(self):
        return self.inputs.oracle_proof()


class Rows:
    """Rows of shared or fresh variables: slot (wire, row) -> variable id."""

    def __init__(self, seed, gates):
        self.cp = Composer(seed)
        self.gates = gates
        self.slot = {}

    def fresh(self):
        return self.cp.var(self.cp.rnd())

    def put(self, v, *slots):
        for s in slots:
            assert s not in self.slot and 0 <= s[0] < 4 and 0 <= s[1] < self.gates, s
            self.slot[s] = v

    def share(self, *slots):
        v = self.fresh()
        self.put(v, *slots)
        return v

    def free(self, wire):
        """The rows of a wire not yet given a shared variable."""
        return [i for i in range(self.gates) if (wire, i) not in self.slot]

    def done(self, arith_rows=()):
        """Selector-free rows, every open slot a fresh variable; arith_rows:
        default Composer.arith() rows instead (four fresh variables, sigma
        fixes the whole row)."""
        arith_rows = set(arith_rows)
        for i in range(self.gates):
            if i in arith_rows:
                assert not any((j, i) in self.slot for j in range(4))
                r, _ = self.cp.arith()
            else:
                r = self.cp.row({}, *(self.slot.get((j, i)) or self.fresh() for j in range(4)))
            assert r == i
        return self.cp


def _deal(rng, rows, sizes):
    """rows (shuffled by rng) dealt out in runs of the given sizes."""
    rows = [rows[k] for k in rng.permutation(len(rows))]
    out, t = [], 0
    for s in sizes:
        out.append(rows[t:t + s])
        t += s
    assert t <= len(rows)
    return out


# ---------------------------------------------------------------- (a)
A_SIZES = (31, 32, 33, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def case_a():
    """n = 2^11, n - 3 gates.  Wire a's groups have sizes 1..40 over and over
    with 31, 32, 33, 63, 64, 65 among them; group k's first row is row k (so
    the groups come in the order they are made and their starts are the prefix
    sums of the sizes: every residue mod 32), its other rows are scattered by a
    seeded shuffle.  The other wires are fresh variables."""
    n, gates = 1 << 11, (1 << 11) - 3
    pattern = list(range(1, 41)) + list(A_SIZES)
    sizes, left = [], gates
    while left:
        s = min(pattern[len(sizes) % len(pattern)], left)
        sizes.append(s)
        left -= s
    rw = Rows(101, gates)
    rng = np.random.default_rng(102)
    G = len(sizes)
    rest = _deal(rng, list(range(G, gates)), [s - 1 for s in sizes])
    for k, s in enumerate(sizes):
        rw.share(*[(0, i) for i in [k] + rest[k]])
    return Case(rw.done(), n, sizes=sizes)


# ---------------------------------------------------------------- (b), (g)
B_N = 1 << 15
# sorted positions of wire a: 31 single rows, then the three runs
B_RUNS = ((31, 8193), (8193, 16380), (16380, 25931))
B_GATES = 26000


@functools.lru_cache(maxsize=None)
def case_b():
    """n = 2^15.  Three non-zero variables in wire a of scattered rows; in
    wire a's sorted order (31 single rows first) their runs are
      [31, 8193): 257 pieces from the fewest positions that make them (8162:
                  one in the first piece, one in the last) — heavy;
      [8193, 16380): exactly 256 pieces, starting and ending mid-chunk — not heavy;
      [16380, 25931): 300 pieces, starting mid-chunk — heavy.
    (2^14 cannot hold them: 257, 256 and 300 pieces take at least 8162 + 8130
    + 9538 sorted positions of one wire.)  Wire c is ident with one real group
    (a variable in three of its rows); wires b and d are fresh variables."""
    rw = Rows(201, B_GATES)
    rng = np.random.default_rng(202)
    sizes = [b - a for a, b in B_RUNS]
    # rows 0..30 single; rows 31, 32, 33 the first rows of the three runs (their order)
    rest = _deal(rng, list(range(34, B_GATES)), [s - 1 for s in sizes])
    rows = []
    for k in range(3):
        rows.append(sorted([31 + k] + rest[k]))
        rw.share(*[(0, i) for i in rows[k]])
    c_rows = (700, 9000, 20011)
    rw.share(*[(2, i) for i in c_rows])
    return Case(rw.done(), B_N, run_rows=rows, c_rows=c_rows)


# ---------------------------------------------------------------- (c)
C_N = 1 << 14


def _moved(rw, rows):
    """Every row of `rows` gets a slot of a cycle across wires a and b (pairs
    of rows, one triple when their number is odd): sigma fixes none of them,
    and every wire keeps single-row groups."""
    rows = list(rows)
    assert len(rows) >= 2
    k = 0
    while k < len(rows):
        if len(rows) - k == 3:
            rw.share((0, rows[k]), (1, rows[k + 1]), (2, rows[k + 2]))
            break
        rw.share((0, rows[k]), (1, rows[k + 1]))
        k += 2


@functools.lru_cache(maxsize=None)
def case_c(kind):
    """n = 2^14.
    "boundary": n/2 + 1 gates, none fixed by sigma: z's run over the padding
        is [8193, 16384), exactly 256 pieces — not heavy;
    "heavy": the same gates, the last 32 default arith rows: the run is
        [8161, 16384), 257 pieces — heavy;
    "middle": 100 arith rows first (a run from row 0), moved rows, 8500 arith
        rows (a heavy run in the middle, [2000, 10501): 267 pieces, starting
        mid-chunk), moved rows, and the padding run."""
    if kind in ("boundary", "heavy"):
        gates = C_N // 2 + 1
        rw = Rows(301, gates)
        fixed = range(gates - 32, gates) if kind == "heavy" else range(0)
        _moved(rw, range(gates - len(fixed)))
        return Case(rw.done(fixed), C_N, cycle_seed=303)
    assert kind == "middle"
    gates = 12001
    rw = Rows(302, gates)
    fixed = list(range(100)) + list(range(2000, 10500))
    _moved(rw, range(100, 2000))
    _moved(rw, range(10500, gates))
    return Case(rw.done(fixed), C_N, cycle_seed=304)


# ---------------------------------------------------------------- (d)
@functools.lru_cache(maxsize=None)
def case_d(shuffled):
    """n = 2^10, n - 3 gates: one non-zero variable in every slot of every
    gate row — one cycle of length 4 (n - 3), which takes every
    pointer-jumping round; in slot order or shuffled."""
    n, gates = 1 << 10, (1 << 10) - 3
    rw = Rows(401, gates)
    rw.share(*[(j, i) for i in range(gates) for j in range(4)])
    return Case(rw.done(), n, cycle_seed=402 if shuffled else None)


# ---------------------------------------------------------------- (e), (i)
@functools.lru_cache(maxsize=None)
def case_e(shuffled=True):
    """n = 2^10, n - 3 gates.  250 variables, each in wire c of three scattered
    rows, in wire a of one other row and in wire d of a third — every fifth one
    in wires a AND d of the same row, every seventh in wire d of a second row.
    A cycle's label is its smallest position, a wire a row: wire c's (and d's)
    group order is set by the rows of wire a."""
    n, gates = 1 << 10, (1 << 10) - 3
    rw = Rows(501, gates)
    rng = np.random.default_rng(502)
    V = 250
    c_rows = _deal(rng, list(range(gates)), [3] * V)
    a_rows = _deal(rng, list(range(gates)), [1] * V)
    taken = {r[0] for r in a_rows}
    d_rows = _deal(rng, [i for i in range(gates) if i not in taken], [2] * V)
    twice = 0
    for k in range(V):
        ra = a_rows[k][0]
        slots = [(2, i) for i in c_rows[k]] + [(0, ra)]
        if k % 5 == 0:
            slots.append((3, ra))
            twice += 1
        else:
            slots.append((3, d_rows[k][0]))
        if k % 7 == 0:
            slots.append((3, d_rows[k][1]))
        rw.share(*slots)
    return Case(rw.done(), n, cycle_seed=503 if shuffled else None, c_rows=c_rows, a_rows=a_rows, twice=twice)


# ---------------------------------------------------------------- (f)
F_N = 1 << 10


def _pairs(rw, wire, count, rows=None):
    """`count` variables, each in two (free) rows of one wire: count fewer groups."""
    rows = rw.free(wire) if rows is None else rows
    for k in range(count):
        rw.share((wire, rows[2 * k]), (wire, rows[2 * k + 1]))


@functools.lru_cache(maxsize=None)
def case_f(kind):
    """n = 2^10 (9 n = 9216, 3 n = 3072).
    "mixed": groups a 767 (gain), b 921 (grouped, no gain of its own), c 922
        (ident inside a grouped batch, with real groups), d 1024;
    "z_alone": a 768 (4 g = 3 n: no gain), the others 1024, and z 921 runs
        (10 g = 9210 <= 9 n): the wires are not grouped, z is, alone;
    "wires_alone": n - 3 gates, every gate row in a group of three rows of
        wire a: the wires are grouped, z (1022 runs) is not."""
    n = F_N
    if kind == "mixed":
        rw = Rows(601, n - 3)
        _pairs(rw, 0, 257)
        _pairs(rw, 1, 103)
        _pairs(rw, 2, 102)
        return Case(rw.done(), n, cycle_seed=611)
    if kind == "z_alone":
        rw = Rows(602, 1000)
        _pairs(rw, 0, 256, rows=list(range(512)))         # rows 0..511 moved
        for k in range(204):                               # rows 512..919 moved, across wires
            rw.share((1, 512 + 2 * k), (2, 513 + 2 * k))
        return Case(rw.done(), n, cycle_seed=612)
    assert kind == "wires_alone"
    gates = n - 3
    rw = Rows(603, gates)
    rows = list(np.random.default_rng(613).permutation(gates))
    for k in range(0, gates - gates % 3 - 3, 3):
        rw.share(*[(0, int(i)) for i in rows[k:k + 3]])
    rw.share(*[(0, int(i)) for i in rows[gates - gates % 3 - 3:]])
    return Case(rw.done(), n, cycle_seed=614)


# ---------------------------------------------------------------- (h)
H_ROWS = (5, 77, 300, 301, 640, 1000)


@functools.lru_cache(maxsize=None)
def case_h(split):
    """n = 2^10, n - 3 gates: wire a in groups of three consecutive rows, and
    one variable in wire a of six rows (H_ROWS).  split: that copy constraint
    is removed between its first three rows and its last three, which hold
    another variable with another value — one group more."""
    n, gates = 1 << 10, (1 << 10) - 3
    rw = Rows(701, gates)
    if split:
        rw.share(*[(0, i) for i in H_ROWS[:3]])
        rw.share(*[(0, i) for i in H_ROWS[3:]])
    else:
        rw.share(*[(0, i) for i in H_ROWS])
    rows = rw.free(0)
    for k in range(0, len(rows) - 2, 3):
        rw.share(*[(0, i) for i in rows[k:k + 3]])
    return Case(rw.done(), n)
