"""The witness solver's rules (include/pnp_plonk.h, pnp_load_solve_inputs) in
plain integers: the model the GPU plan and solve (csrc/solve.hip) are tested
against.

A circuit is a Composer's rows, [(selector dict, (a, b, c, d))], canonical
ints.  Slots and their selectors: a (q_l, q_hl, q_m), b (q_r, q_hr, q_m),
c (q_o), d (q_4, q_h4).  A slot is RELEVANT when q_arith != 0 and any of its
selectors is non-zero, SOLVABLE when its linear selector is non-zero and the
others are zero.  K_0 = the inputs; in round t a row is READY when exactly one
relevant slot holds a variable outside K_(t-1) (the same unknown in two
relevant slots counts twice: not ready) and that slot is solvable; the lowest
row ready for a variable defines it; the first round without a ready row ends
it.  u = -(S + PI / q_arith) / coef, S the row's arithmetic sum with u's slot
and the slots that are not relevant taken as 0.

plan_sweep is the rules word for word (every round looks at every row);
plan is the same result from counters (a row is looked at again only when one
of its variables became known), for circuits where the sweep takes too long.
"""
from circuits import R_MOD

LINEAR = ("q_l", "q_r", "q_o", "q_4")
OTHERS = (("q_hl", "q_m"), ("q_hr", "q_m"), (), ("q_h4",))


def slot_masks(q):
    """(relevant, solvable): four booleans each, slots a b c d."""
    g = lambda k: q.get(k, 0) % R_MOD
    if not g("q_arith"):
        return (False,) * 4, (False,) * 4
    lin = [g(k) != 0 for k in LINEAR]
    oth = [any(g(k) for k in ks) for ks in OTHERS]
    return tuple(l or o for l, o in zip(lin, oth)), tuple(l and not o for l, o in zip(lin, oth))


class Plan:
    """levels[t] = [(variable, row, slot)] in variable order; undetermined =
    the variables that are neither inputs nor targets, ascending."""

    def __init__(self, levels, n_vars, inputs):
        self.levels = [sorted(l) for l in levels]
        known = set(inputs) | {u for l in levels for u, _, _ in l}
        self.undetermined = [u for u in range(n_vars) if u not in known]
        self.n_solved = sum(len(l) for l in levels)
        self.widths = [len(l) for l in levels]
        self.max_width = max(self.widths, default=0)


def plan_sweep(rows, n_vars, inputs):
    masks = [slot_masks(q) for q, _ in rows]
    known = set(inputs)
    levels = []
    while True:
        winner = {}
        for i, (_, ws) in enumerate(rows):
            rel, solv = masks[i]
            unknown = [j for j in range(4) if rel[j] and ws[j] not in known]
            if len(unknown) == 1 and solv[unknown[0]]:
                u = ws[unknown[0]]
                if u not in winner:  # rows ascend: the first is the lowest
                    winner[u] = (i, unknown[0])
        if not winner:
            return Plan(levels, n_vars, inputs)
        levels.append([(u, i, j) for u, (i, j) in winner.items()])
        known |= set(winner)


def plan(rows, n_vars, inputs):
    masks = [slot_masks(q) for q, _ in rows]
    known = set(inputs)
    occ = {}  # variable -> [(row, slot)] over relevant slots
    cnt = [0] * len(rows)
    for i, (_, ws) in enumerate(rows):
        for j in range(4):
            if masks[i][0][j] and ws[j] not in known:
                occ.setdefault(ws[j], []).append((i, j))
                cnt[i] += 1
    fresh = [i for i in range(len(rows)) if cnt[i] == 1]  # rows that just came down to one unknown slot
    levels = []
    while True:
        winner = {}
        for i in sorted(fresh):
            ws = rows[i][1]
            j = next(j for j in range(4) if masks[i][0][j] and ws[j] not in known)
            if masks[i][1][j] and ws[j] not in winner:
                winner[ws[j]] = (i, j)
        # (a row whose one unknown slot is not solvable never becomes ready: it can be forgotten)
        if not winner:
            return Plan(levels, n_vars, inputs)
        levels.append([(u, i, j) for u, (i, j) in winner.items()])
        known |= set(winner)
        fresh = []
        for u in winner:
            for i, _ in occ.get(u, ()):
                cnt[i] -= 1
                if cnt[i] == 1:
                    fresh.append(i)
        fresh = [i for i in set(fresh) if cnt[i] == 1]


def define(q, ws, slot, vals, pi):
    """The defining equation of the variable in `slot` of one row."""
    g = lambda k: q.get(k, 0) % R_MOD
    rel, _ = slot_masks(q)
    a, b, c, d = (vals[ws[j]] if rel[j] and j != slot else 0 for j in range(4))
    s = (g("q_m") * a * b + g("q_l") * a + g("q_r") * b + g("q_o") * c + g("q_4") * d + g("q_hl") * pow(a, 5, R_MOD)
         + g("q_hr") * pow(b, 5, R_MOD) + g("q_h4") * pow(d, 5, R_MOD) + g("q_c")) % R_MOD
    s = (s + pi * pow(g("q_arith"), -1, R_MOD)) % R_MOD
    return -s * pow(g(LINEAR[slot]), -1, R_MOD) % R_MOD


def solve(rows, pl, n_vars, inputs, pis=None):
    """The whole assignment: inputs = {variable: value}, pis = {row: value};
    a variable the plan does not reach stays None."""
    pis = pis or {}
    vals = [None] * n_vars
    for u, v in inputs.items():
        vals[u] = v % R_MOD
    for level in pl.levels:
        new = [(u, define(rows[i][0], rows[i][1], j, vals, pis.get(i, 0))) for u, i, j in level]
        for u, v in new:
            vals[u] = v
    return vals


def merkle_inputs(cp):
    """The input variables of tests/merkle_circuit.py's circuit: the 8 blinding
    values, the leaves, and the domain-tag variable of every hash (wire a of
    the hash's first row)."""
    n_leaves = len(cp.leaves)
    leaves = list(range(9, 9 + n_leaves))
    assert [cp.vals[u] for u in leaves] == cp.leaves
    tags = [cp.rows[4 + 193 * h][1][0] for h in range(n_leaves - 1)]
    assert len({cp.vals[u] for u in tags}) == 1 and len(set(tags)) == len(tags)
    return list(range(1, 9)) + leaves + tags
