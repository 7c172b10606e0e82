"""Output rows of a solve plan (include/pnp_plonk.h, pnp_load_solve_plan) in
plain integers, over the model of tests/solve_ref.py.

An output row is a row whose public input is derived instead of given.  It is
never READY, which is what a row with q_arith = 0 is: the plan is solve_ref's
plan over rows whose output rows carry {"q_arith": 0}.  After the last level
PI_i = -q_arith_i S_i, S_i the row's full arithmetic sum over the solved
values, every slot as it stands.
"""
from circuits import R_MOD
import solve_ref


def masked(rows, outputs):
    """The rows with q_arith = 0 on the output rows (the originals are not touched)."""
    outputs = set(outputs)
    return [({**q, "q_arith": 0}, ws) if i in outputs else (q, ws) for i, (q, ws) in enumerate(rows)]


def plan_outputs(rows, n_vars, inputs, outputs, sweep=False):
    return (solve_ref.plan_sweep if sweep else solve_ref.plan)(masked(rows, outputs), n_vars, inputs)


def derive(rows, vals, outputs):
    """{row: -q_arith S mod r} for the output rows, in listed order."""
    out = {}
    for i in outputs:
        q, ws = rows[i]
        g = lambda k: q.get(k, 0) % R_MOD
        a, b, c, d = (vals[w] for w in ws)
        s = (g("q_m") * a * b + g("q_l") * a + g("q_r") * b + g("q_o") * c + g("q_4") * d + g("q_hl") * pow(a, 5, R_MOD)
             + g("q_hr") * pow(b, 5, R_MOD) + g("q_h4") * pow(d, 5, R_MOD) + g("q_c")) % R_MOD
        out[i] = -g("q_arith") * s % R_MOD
    return out
