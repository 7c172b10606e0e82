"""Fixed-base and curve-addition rows that define (include/pnp_plonk.h,
pnp_load_solve_plan_ecc) in plain integers, over the model of
tests/solve_gates_ref.py: what the GPU plan and solve (csrc/solve.hip) are
tested against.

The rules join the rounds of solve_gates_ref; in round t every rule looks at
K_(t-1).  A row i of either family takes part only when i + 1 < n_gates and i
is not an output row.  A, D: Jubjub's a = -1 and d.
  FIXED_ADD   row i, fixed_group_add_selector != 0; slots a, b the point
              accumulator, c xy_alpha, d the scalar accumulator; q_l, q_r, q_c
              = x_beta, y_beta, xy_beta.  Three independent sub-rules:
    scalar    READY when slot d of row i + 1 is known; bids for slot d of row
              i: with V the canonical d_next, d = (V - s) / 2 on integers,
              s = 0 for V even, 1 for V = 1 (mod 4), -1 for V = 3 (mod 4)
    xy        READY when slots d of rows i and i + 1 are known; bids for slot
              c of row i: c = bit q_c, bit = d_next - 2 d in the field
    point     READY when slots a, b, d of row i and slot d of row i + 1 are
              known; bids for slots a and b of row i + 1: x = q_l bit,
              y = bit^2 (q_r - 1) + 1, m = (bit q_c) a b D,
              a_next = (x b + y a) / (1 + m), b_next = (y b - A x a) / (1 - m);
              slot c is not read
  VAR_ADD     row i, variable_group_add_selector != 0: READY when slots a, b,
              c, d of row i are known; bids for slots d, a, b of row i + 1:
              d_next = a d, t = D d_next (b c), a_next = (d_next + b c) / (1 + t),
              b_next = (b d - A a c) / (1 - t)
A division by zero yields 0; a slot whose variable is known is not redefined.
Among the bids of a round for one variable the least (row, role) wins: roles
0..12 as solve_gates_ref, 13..16 fixed-add d, c, a_next, b_next, 17..19
var-add a_next, b_next, d_next; the row is the row whose rule fires.

plan_sweep is the rules word for word; plan is the same from counters.
"""
from circuits import JJ_A, JJ_D, R_MOD
import solve_gates_ref
import solve_outputs_ref
import solve_ref

FIXED_ADD, VAR_ADD = 1, 2
ROLE_FIXED, ROLE_VAR, ROLES = 13, 17, 20


class Plan(solve_gates_ref.Plan):
    """solve_gates_ref.Plan (gate_widths, n_range, n_logic: range and logic
    only) with ecc_widths a level and n_fixed / n_var, the variables fixed-add
    and var-add rows define."""

    def __init__(self, levels, n_vars, inputs):
        super().__init__(levels, n_vars, inputs)
        self.ecc_widths = [sum(1 for _, _, r in l if r >= ROLE_FIXED) for l in self.levels]
        self.gate_widths = [g - e for g, e in zip(self.gate_widths, self.ecc_widths)]
        self.n_logic = sum(1 for l in self.levels for _, _, r in l if solve_gates_ref.ROLE_LOGIC <= r < ROLE_FIXED)
        self.n_fixed = sum(1 for l in self.levels for _, _, r in l if ROLE_FIXED <= r < ROLE_VAR)
        self.n_var = sum(1 for l in self.levels for _, _, r in l if r >= ROLE_VAR)


def ecc_rules(rows, outputs, ecc):
    """Per row (fixed-add rule, var-add rule)."""
    outputs = set(outputs)
    out = []
    for i, (q, _) in enumerate(rows):
        g = lambda k: q.get(k, 0) % R_MOD
        live = i + 1 < len(rows) and i not in outputs
        out.append((bool(live and ecc & FIXED_ADD and g("fixed_group_add_selector")),
                    bool(live and ecc & VAR_ADD and g("variable_group_add_selector"))))
    return out


def row_bids(rows, masks, rules, erules, i, known):
    """[(variable, role)] row i bids for when K_(t-1) = known."""
    bids = solve_gates_ref.row_bids(rows, masks, rules, i, known)
    fixed, var = erules[i]
    ws = rows[i][1]
    if fixed:
        nx = rows[i + 1][1]
        d0, d1 = ws[3] in known, nx[3] in known
        if d1 and ws[3] not in known:
            bids.append((ws[3], ROLE_FIXED))
        if d0 and d1 and ws[2] not in known:
            bids.append((ws[2], ROLE_FIXED + 1))
        if d0 and d1 and ws[0] in known and ws[1] in known:
            bids += [(nx[j], ROLE_FIXED + 2 + j) for j in range(2) if nx[j] not in known]
    if var and all(w in known for w in ws):
        nx = rows[i + 1][1]
        targets = (nx[0], nx[1], nx[3])
        bids += [(targets[j], ROLE_VAR + j) for j in range(3) if targets[j] not in known]
    return bids


def _tables(rows, outputs, gates, ecc):
    mrows = solve_outputs_ref.masked(rows, outputs)
    return ([solve_ref.slot_masks(q) for q, _ in mrows], solve_gates_ref.gate_rules(rows, outputs, gates),
            ecc_rules(rows, outputs, ecc))


def plan_sweep(rows, n_vars, inputs, outputs=(), gates=0, ecc=0):
    masks, rules, erules = _tables(rows, outputs, gates, ecc)
    known = set(inputs)
    levels = []
    while True:
        winner = {}
        for i in range(len(rows)):
            for u, role in row_bids(rows, masks, rules, erules, i, known):
                if u not in winner or (i, role) < winner[u]:
                    winner[u] = (i, role)
        if not winner:
            return Plan(levels, n_vars, inputs)
        levels.append([(u, i, role) for u, (i, role) in winner.items()])
        known |= set(winner)


def plan(rows, n_vars, inputs, outputs=(), gates=0, ecc=0):
    """plan_sweep from counters: a row is looked at in a round only when a
    variable of its own or of its next row became known in the round before."""
    masks, rules, erules = _tables(rows, outputs, gates, ecc)
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
            pending[i] = row_bids(rows, masks, rules, erules, i, known)
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


def naf_digit(v):
    """The lowest digit of the width-2 NAF of the integer v."""
    return 0 if v % 2 == 0 else 1 if v % 4 == 1 else -1


def div(n, d):
    """n / d in the field, 0 for d = 0."""
    return n * pow(d, -1, R_MOD) % R_MOD if d % R_MOD else 0


def define(rows, i, role, vals, pi):
    """The value a (row, role) definition gives its variable."""
    if role < ROLE_FIXED:
        return solve_gates_ref.define(rows, i, role, vals, pi)
    q, ws = rows[i]
    nx = rows[i + 1][1]
    g = lambda k: q.get(k, 0) % R_MOD
    if role == ROLE_FIXED:
        v = vals[nx[3]]
        return (v - naf_digit(v)) // 2
    a, b, c, d = (vals[w] for w in ws)
    if role < ROLE_VAR:
        bit = (vals[nx[3]] - 2 * d) % R_MOD
        if role == ROLE_FIXED + 1:
            return bit * g("q_c") % R_MOD
        x, y = g("q_l") * bit % R_MOD, (bit * bit * (g("q_r") - 1) + 1) % R_MOD
        m = bit * g("q_c") * a * b * JJ_D % R_MOD
        if role == ROLE_FIXED + 2:
            return div(x * b + y * a, 1 + m)
        return div(y * b - JJ_A * x * a, 1 - m)
    dn = a * d % R_MOD
    t = JJ_D * dn * b * c % R_MOD
    if role == ROLE_VAR:
        return div(dn + b * c, 1 + t)
    if role == ROLE_VAR + 1:
        return div(b * d - JJ_A * a * c, 1 - t)
    return dn


def solve(rows, pl, n_vars, inputs, pis=None, outputs=()):
    """The whole assignment, as solve_gates_ref.solve."""
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
