"""Lookup rows that define (include/pnp_plonk.h, pnp_load_solve_plan_lookup) in
plain integers, over the model of tests/solve_ecc_ref.py: what the GPU plan
and solve (csrc/solve.hip) are tested against.

The rule joins the rounds of solve_ecc_ref; in round t every rule looks at
K_(t-1).
  LOOKUP   row i, q_lookup != 0, not an output row: READY when the variables in
           slots a, b and d are known and the one in slot c is not; bids for
           slot c.  It needs no next row, so the last row takes part.
           c = T[p][2], p the lowest row of the table T with T[p][0] = a,
           T[p][1] = b, T[p][3] = d; 0 when there is no such row.
T is the key's resident table: the circuit's table rows, then copies of row 0
up to D rows (MultiSet::pad; an empty table is one zero row).  The copies carry
row 0's key and value and a higher index, so only row 0 and the rows that
differ from it are searched (indexed_rows), in table order.
Among the bids of a round for one variable the least (row, role) wins: roles
0..19 as solve_ecc_ref, 20 lookup c.

bucket() restates the device's hash of a key (lookup_hash of csrc/solve.hip
over the 24 Montgomery words), so that a test can say which rows share a
bucket of the index; no answer depends on it.

plan_sweep is the rules word for word; plan is the same from counters.
"""
from circuits import R_MOD
from pnp_testlib import fr_mont
import solve_ecc_ref
import solve_outputs_ref

LOOKUP = 1
ROLE_LOOKUP, ROLES = 20, 21


class Plan(solve_ecc_ref.Plan):
    """solve_ecc_ref.Plan (ecc_widths, n_fixed, n_var: the ECC families only)
    with lookup_widths a level and n_lookup, the variables lookup rows define."""

    def __init__(self, levels, n_vars, inputs):
        super().__init__(levels, n_vars, inputs)
        self.lookup_widths = [sum(1 for _, _, r in l if r == ROLE_LOOKUP) for l in self.levels]
        self.ecc_widths = [e - k for e, k in zip(self.ecc_widths, self.lookup_widths)]
        self.n_var = sum(1 for l in self.levels for _, _, r in l if solve_ecc_ref.ROLE_VAR <= r < ROLE_LOOKUP)
        self.n_lookup = sum(self.lookup_widths)


def lookup_rules(rows, outputs, lookup):
    """Per row: the lookup rule."""
    outputs = set(outputs)
    return [bool(lookup & LOOKUP and q.get("q_lookup", 0) % R_MOD and i not in outputs)
            for i, (q, _) in enumerate(rows)]


def row_bids(rows, masks, rules, erules, lrules, i, known):
    """[(variable, role)] row i bids for when K_(t-1) = known."""
    bids = solve_ecc_ref.row_bids(rows, masks, rules, erules, i, known)
    a, b, c, d = rows[i][1]
    if lrules[i] and a in known and b in known and d in known and c not in known:
        bids.append((c, ROLE_LOOKUP))
    return bids


def _tables(rows, outputs, gates, ecc, lookup):
    return solve_ecc_ref._tables(rows, outputs, gates, ecc) + (lookup_rules(rows, outputs, lookup),)


def plan_sweep(rows, n_vars, inputs, outputs=(), gates=0, ecc=0, lookup=0):
    masks, rules, erules, lrules = _tables(rows, outputs, gates, ecc, lookup)
    known = set(inputs)
    levels = []
    while True:
        winner = {}
        for i in range(len(rows)):
            for u, role in row_bids(rows, masks, rules, erules, lrules, i, known):
                if u not in winner or (i, role) < winner[u]:
                    winner[u] = (i, role)
        if not winner:
            return Plan(levels, n_vars, inputs)
        levels.append([(u, i, role) for u, (i, role) in winner.items()])
        known |= set(winner)


def plan(rows, n_vars, inputs, outputs=(), gates=0, ecc=0, lookup=0):
    """plan_sweep from counters: a row is looked at in a round only when a
    variable of its own or of its next row became known in the round before
    (a lookup row waits for its own variables only)."""
    masks, rules, erules, lrules = _tables(rows, outputs, gates, ecc, lookup)
    known = set(inputs)
    watch = {}  # variable -> the rows whose bids may change when it becomes known
    for i, (_, ws) in enumerate(rows):
        for v in ws:
            watch.setdefault(v, set()).add(i)
            if i and (any(rules[i - 1]) or any(erules[i - 1])):
                watch[v].add(i - 1)
    fresh = set(range(len(rows)))
    pending = {}  # row -> its bids, as long as they stand
    levels = []
    while True:
        for i in fresh:
            pending[i] = row_bids(rows, masks, rules, erules, lrules, i, known)
        winner = {}
        for i in sorted(k for k, b in pending.items() if b):
            for u, role in pending[i]:
                if u not in winner or (i, role) < winner[u]:
                    winner[u] = (i, role)
        if not winner:
            return Plan(levels, n_vars, inputs)
        levels.append([(u, i, role) for u, (i, role) in winner.items()])
        known |= set(winner)
        fresh = set()
        for u in winner:
            fresh |= watch.get(u, set())


def padded_table(table, D):
    """The D rows the key holds: the table, then copies of its row 0."""
    rows = [tuple(v % R_MOD for v in r) for r in table] or [(0, 0, 0, 0)]
    assert len(rows) <= D
    return rows + [rows[0]] * (D - len(rows))


def indexed_rows(table, D):
    """The rows of the padded table a search looks at, ascending: row 0 and
    every row that differs from row 0."""
    t = padded_table(table, D)
    return [p for p, r in enumerate(t) if p == 0 or r != t[0]]


def lookup(table, D, a, b, d):
    """LookupTable::lookup over the padded table, 0 for a key it does not hold."""
    t = padded_table(table, D)
    key = (a % R_MOD, b % R_MOD, d % R_MOD)
    for p in indexed_rows(table, D):
        if (t[p][0], t[p][1], t[p][3]) == key:
            return t[p][2]
    return 0


def n_buckets(m):
    """B = next_pow2(2 m), at least 2."""
    b = 2
    while b < 2 * m:
        b <<= 1
    return b


def bucket(a, b, d, B):
    """The bucket of the key (a, b, d) among B: the device's mix of the 24
    32-bit Montgomery words, lowest word of a first."""
    M = 0xFFFFFFFF
    h = 0x9E3779B9
    for v in (a, b, d):
        w = fr_mont(v % R_MOD)
        for k in range(8):
            h ^= (w >> (32 * k)) & M
            h = h * 0x85EBCA6B & M
            h = (h << 13 | h >> 19) & M
    h ^= h >> 16
    h = h * 0xC2B2AE35 & M
    h ^= h >> 15
    return h & (B - 1)


def buckets_of(table, D):
    """{bucket: [indexed rows, ascending]} as the plan build lays the index out."""
    t = padded_table(table, D)
    rows = indexed_rows(table, D)
    B = n_buckets(len(rows))
    out = {}
    for p in rows:
        out.setdefault(bucket(t[p][0], t[p][1], t[p][3], B), []).append(p)
    return out


def define(rows, i, role, vals, pi, table, D):
    """The value a (row, role) definition gives its variable."""
    if role < ROLE_LOOKUP:
        return solve_ecc_ref.define(rows, i, role, vals, pi)
    a, b, _, d = rows[i][1]
    return lookup(table, D, vals[a], vals[b], vals[d])


def solve(rows, pl, n_vars, inputs, pis=None, outputs=(), table=(), D=1):
    """The whole assignment, as solve_ecc_ref.solve; `table` the circuit's
    table rows and D the domain they are padded to."""
    pis = pis or {}
    mrows = solve_outputs_ref.masked(rows, outputs)
    vals = [None] * n_vars
    for u, v in inputs.items():
        vals[u] = v % R_MOD
    for level in pl.levels:
        new = [(u, define(mrows, i, role, vals, pis.get(i, 0), table, D)) for u, i, role in level]
        for u, v in new:
            vals[u] = v
    return vals
