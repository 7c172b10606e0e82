"""Range and logic rows that define (include/pnp_plonk.h,
pnp_load_solve_plan_gates) in plain integers, over the models of
tests/solve_ref.py and tests/solve_outputs_ref.py: what the GPU plan and
solve (csrc/solve.hip) are tested against.

One set of rounds for every family; in round t every rule looks at K_(t-1).
  arithmetic  solve_ref's rule, on the rows as solve_outputs_ref masks them
  RANGE       row i, range_selector != 0, i + 1 < n_gates, not an output row:
              READY when slot d of row i + 1 is known; bids for its unknown
              slots a, b, c, d = V >> 2, 4, 6, 8, V the canonical d_next
  LOGIC       row i, logic_selector != 0, q_c = 1 (AND) or -1 (XOR), i + 1 <
              n_gates, not an output row: READY when slots a and b of row i + 1
              are known; bids for the unknown ones of a_i = A >> 2, b_i = B >> 2,
              c_i = (A & 3) (B & 3), d_i = (A >> 2) op (B >> 2) and slot d of
              row i + 1 = A op B; an XOR that reaches r loses one r
Among the bids of a round for one variable the least (row, role) wins: roles
0..3 the arithmetic slots, 4..7 range a..d, 8..12 logic a, b, c, d, d_next;
the row is the row whose rule fires.

plan_sweep is the rules word for word; plan is the same from counters (a row
is looked at again only when something it waits for became known).
"""
from circuits import R_MOD
import solve_outputs_ref
import solve_ref

RANGE, LOGIC = 1, 2
ROLE_RANGE, ROLE_LOGIC = 4, 8


class Plan(solve_ref.Plan):
    """solve_ref.Plan with levels of (variable, row, role), and the entries by
    kind: arith_widths / gate_widths a level, n_range / n_logic in all."""

    def __init__(self, levels, n_vars, inputs):
        super().__init__(levels, n_vars, inputs)
        self.arith_widths = [sum(1 for _, _, r in l if r < ROLE_RANGE) for l in self.levels]
        self.gate_widths = [w - a for w, a in zip(self.widths, self.arith_widths)]
        self.n_range = sum(1 for l in self.levels for _, _, r in l if ROLE_RANGE <= r < ROLE_LOGIC)
        self.n_logic = sum(1 for l in self.levels for _, _, r in l if r >= ROLE_LOGIC)


def gate_rules(rows, outputs, gates):
    """Per row (range rule, logic op): op = None, "and" or "xor"."""
    outputs = set(outputs)
    out = []
    for i, (q, _) in enumerate(rows):
        g = lambda k: q.get(k, 0) % R_MOD
        live = i + 1 < len(rows) and i not in outputs
        rng = bool(live and gates & RANGE and g("range_selector"))
        op = None
        if live and gates & LOGIC and g("logic_selector"):
            op = {1: "and", R_MOD - 1: "xor"}.get(g("q_c"))
        out.append((rng, op))
    return out


def row_bids(rows, masks, rules, i, known):
    """[(variable, role)] row i bids for when K_(t-1) = known."""
    ws = rows[i][1]
    bids = []
    rel, solv = masks[i]
    unknown = [j for j in range(4) if rel[j] and ws[j] not in known]
    if len(unknown) == 1 and solv[unknown[0]]:
        bids.append((ws[unknown[0]], unknown[0]))
    rng, op = rules[i]
    if rng and rows[i + 1][1][3] in known:
        bids += [(ws[j], ROLE_RANGE + j) for j in range(4) if ws[j] not in known]
    if op and rows[i + 1][1][0] in known and rows[i + 1][1][1] in known:
        targets = list(ws) + [rows[i + 1][1][3]]
        bids += [(targets[j], ROLE_LOGIC + j) for j in range(5) if targets[j] not in known]
    return bids


def plan_sweep(rows, n_vars, inputs, outputs=(), gates=0):
    mrows = solve_outputs_ref.masked(rows, outputs)
    masks = [solve_ref.slot_masks(q) for q, _ in mrows]
    rules = gate_rules(rows, outputs, gates)
    known = set(inputs)
    levels = []
    while True:
        winner = {}
        for i in range(len(rows)):
            for u, role in row_bids(rows, masks, rules, i, known):
                if u not in winner or (i, role) < winner[u]:
                    winner[u] = (i, role)
        if not winner:
            return Plan(levels, n_vars, inputs)
        levels.append([(u, i, role) for u, (i, role) in winner.items()])
        known |= set(winner)


def plan(rows, n_vars, inputs, outputs=(), gates=0):
    """plan_sweep from counters: a row is looked at in a round only when a
    variable of its own or of its next row became known in the round before."""
    mrows = solve_outputs_ref.masked(rows, outputs)
    masks = [solve_ref.slot_masks(q) for q, _ in mrows]
    rules = gate_rules(rows, outputs, gates)
    known = set(inputs)
    watch = {}  # variable -> the rows whose bids may change when it becomes known
    for i, (_, ws) in enumerate(rows):
        for v in ws:
            watch.setdefault(v, set()).add(i)
            if i and any(rules[i - 1]):
                watch[v].add(i - 1)
    fresh = set(range(len(rows)))
    pending = {}  # row -> its bids, as long as they stand
    levels = []
    while True:
        for i in fresh:
            pending[i] = row_bids(rows, masks, rules, i, known)
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


def define(rows, i, role, vals, pi):
    """The value a (row, role) definition gives its variable."""
    if role < ROLE_RANGE:
        return solve_ref.define(rows[i][0], rows[i][1], role, vals, pi)
    nxt = rows[i + 1][1]
    if role < ROLE_LOGIC:
        return vals[nxt[3]] >> (2 * (role - ROLE_RANGE + 1))
    a, b = vals[nxt[0]], vals[nxt[1]]
    xor = rows[i][0].get("q_c", 0) % R_MOD == R_MOD - 1
    op = (lambda x, y: x ^ y) if xor else (lambda x, y: x & y)
    j = role - ROLE_LOGIC
    v = (a >> 2, b >> 2, (a & 3) * (b & 3), op(a >> 2, b >> 2), op(a, b))[j]
    return v - R_MOD if v >= R_MOD else v


def solve(rows, pl, n_vars, inputs, pis=None, outputs=()):
    """The whole assignment, as solve_ref.solve; the arithmetic rows as the
    plan saw them (output rows masked)."""
    pis = pis or {}
    mrows = solve_outputs_ref.masked(rows, outputs)
    vals = [None] * n_vars
    for u, v in inputs.items():
        vals[u] = v % R_MOD
    for level in pl.levels:
        new = [(u, define(mrows, i, role, vals, pis.get(i, 0))) for u, i, role in level]
        for u, v in new:
            vals[u] = v
    return vals
