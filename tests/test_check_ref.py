"""The reference the GPU satisfiability check (pnp_check_assignment /
pnp_check_witness, csrc/check.hip) is tested against, pinned on the CPU.

check_columns_ref is the check of include/pnp_plonk.h in plain Python
integers: every constraint of every gate family alone on every row of the
domain (wires zero from n_gates on, "next" = row i + 1 mod D), the lookup
query rule with an exact tuple comparison, and the copy constraints of a wire
map over columns.  It returns the sorted (row, kind, index) list; report_of
folds that into the fields of pnp_check_report.

Here the model is tied to the verifier: the circuits of the suite give no
violation and their oracle proofs are accepted; one wire value changed gives
the violations listed below and a proof the restated verifier rejects."""
import ctypes as C

import pytest

from circuits import JJ_A, JJ_D, R_MOD, SEL
from pnp import abi
from pnp_testlib import oracle, verify, vp
from test_general import make_circuit, pis_of

ARITH, RANGE, LOGIC, FIXED_ADD, VAR_ADD, LOOKUP, COPY = range(7)
KINDS = 7


def _delta(f):
    return f * (f - 1) * (f - 2) * (f - 3) % R_MOD


def _delta_xor_and(a, b, w, c, q_c):
    F = w * (w * (4 * w - 18 * (a + b) + 81) + 18 * (a * a + b * b) - 81 * (a + b) + 83)
    E = 3 * (a + b + c) - 2 * F
    B = q_c * (9 * c - 3 * (a + b))
    return (B + E) % R_MOD


def _range(a, b, c, d, an, bn, dn, q):
    return [_delta(c - 4 * d), _delta(b - 4 * c), _delta(a - 4 * b), _delta(dn - 4 * a)]


def _logic(a, b, c, d, an, bn, dn, q):
    a_, b_, d_ = (an - 4 * a) % R_MOD, (bn - 4 * b) % R_MOD, (dn - 4 * d) % R_MOD
    return [_delta(a_), _delta(b_), _delta(d_), (c - a_ * b_) % R_MOD, _delta_xor_and(a_, b_, c, d_, q["q_c"])]


def _fixed_add(a, b, c, d, an, bn, dn, q):
    bit = (dn - 2 * d) % R_MOD
    y_alpha = (bit * bit * (q["q_r"] - 1) + 1) % R_MOD
    x_alpha = q["q_l"] * bit % R_MOD
    m = c * a * b * JJ_D % R_MOD
    return [bit * (bit - 1) * (bit + 1) % R_MOD, (bit * q["q_c"] - c) % R_MOD,
            (an + an * m - (x_alpha * b + y_alpha * a)) % R_MOD,
            (bn - bn * m - (y_alpha * b - JJ_A * x_alpha * a)) % R_MOD]


def _var_add(a, b, c, d, an, bn, dn, q):
    dm = JJ_D * dn * b * c % R_MOD
    return [(a * d - dn) % R_MOD, (dn + b * c - (an + an * dm)) % R_MOD,
            (b * d - JJ_A * a * c - (bn - bn * dm)) % R_MOD]


FAMILIES = ((RANGE, "range_selector", _range), (LOGIC, "logic_selector", _logic),
            (FIXED_ADD, "fixed_group_add_selector", _fixed_add),
            (VAR_ADD, "variable_group_add_selector", _var_add))


def check_columns_ref(sel, w, D, pis, table=(), s=None, var=None):
    """sel: selector name -> n_gates row values (absent: zero); w: four lists
    of n_gates wire values; pis: [(row, value)]; table: the unpadded table
    rows; s: the caller's q_lookup rows (None: the key's, sel["q_lookup"]);
    var: (4, n_gates) variable ids, or None (no copy check).  Canonical ints."""
    ng = len(w[0])
    assert ng <= D and all(len(c) == ng for c in w)
    q = {name: [v % R_MOD for v in sel.get(name, [])] + [0] * (D - len(sel.get(name, []))) for name in SEL}
    col = [[v % R_MOD for v in c] + [0] * (D - ng) for c in w]
    pi = dict(pis)
    tab = [tuple(v % R_MOD for v in row) for row in table] or [(0, 0, 0, 0)]
    tab = tab + [tab[0]] * (D - len(tab))  # MultiSet::pad
    rows_of_t = set(tab)
    s = q["q_lookup"] if s is None else [v % R_MOD for v in s] + [0] * (D - len(s))
    out = []
    for i in range(D):
        a, b, c, d = (col[j][i] for j in range(4))
        nx = (i + 1) % D
        an, bn, dn = col[0][nx], col[1][nx], col[3][nx]
        qi = {name: q[name][i] for name in SEL}
        g = (qi["q_m"] * a * b + qi["q_l"] * a + qi["q_r"] * b + qi["q_o"] * c + qi["q_4"] * d
             + qi["q_hl"] * pow(a, 5, R_MOD) + qi["q_hr"] * pow(b, 5, R_MOD) + qi["q_h4"] * pow(d, 5, R_MOD)
             + qi["q_c"])
        if (qi["q_arith"] * g + pi.get(i, 0)) % R_MOD:
            out.append((i, ARITH, 0))
        for kind, name, fn in FAMILIES:
            if qi[name]:
                out += [(i, kind, k) for k, v in enumerate(fn(a, b, c, d, an, bn, dn, qi)) if v % R_MOD]
        if s[i]:
            if (a, b, c, d) not in rows_of_t:
                out.append((i, LOOKUP, 0))
        elif qi["q_lookup"] and (a, b, c, d) != tab[0]:
            out.append((i, LOOKUP, 1))
    if var is not None:
        first = {}
        for i in range(ng):
            for j in range(4):
                first.setdefault(int(var[j][i]), (i, j))
        for i in range(ng):
            for j in range(4):
                fi, fj = first[int(var[j][i])]
                if col[j][i] != col[fj][fi]:
                    out.append((i, COPY, j))
    return sorted(out)


def composer_columns(cp):
    """(sel, w, table, var) of a circuits.Composer, for check_columns_ref."""
    sel = {name: [r[0].get(name, 0) for r in cp.rows] for name in SEL}
    w = [[cp.vals[r[1][j]] for r in cp.rows] for j in range(4)]
    var = [[r[1][j] for r in cp.rows] for j in range(4)]
    return sel, w, cp.table, var


def check_ref(cp, D, pis):
    """The violations of a Composer's own witness (one value a variable: the
    copy constraints hold), sorted (row, kind, index)."""
    sel, w, table, _ = composer_columns(cp)
    return check_columns_ref(sel, w, D, pis, table)


def report_of(violations, copy_checked):
    """The fields of pnp_check_report for a violation list."""
    by_kind = [sum(1 for v in violations if v[1] == k) for k in range(KINDS)]
    first = min(violations) if violations else ((1 << 64) - 1, 0, 0)
    return {"violations": len(violations), "by_kind": by_kind, "first_row": first[0], "first_kind": first[1],
            "first_index": first[2], "copy_checked": copy_checked}


# ------------------------------------------------------------------ the mutations of "all"
MUTATIONS = ("range", "logic", "fbsm", "curve_add", "no_pis", "lookup_outside")
_ROW_SEL = {"range": "range_selector", "logic": "logic_selector", "fbsm": "fixed_group_add_selector",
            "curve_add": "variable_group_add_selector"}


def mutated_all(name):
    """make_circuit("all") with one defect: + 1 on the variable in wire a of
    the first gate of a family, the public inputs dropped, or a lookup of a
    tuple outside the table.  Returns (composer, public inputs to check with)."""
    cp = make_circuit("all")
    pis = sorted(cp.pis.items())
    if name in _ROW_SEL:
        row = next(i for i, r in enumerate(cp.rows) if r[0].get(_ROW_SEL[name]))
        va = cp.rows[row][1][0]
        cp.vals[va] = (cp.vals[va] + 1) % R_MOD
    elif name == "no_pis":
        pis = []
    elif name == "lookup_outside":
        row = next(i for i, r in enumerate(cp.rows) if r[0].get("q_lookup"))
        cp.vals[cp.rows[row][1][2]] = 12345  # no such table row
    else:
        assert name is None
    return cp, pis


# the model on make_circuit("all", seed 5): 43 rows, D = 64
EXPECTED = {
    "range": [(8, RANGE, 3)],
    "logic": [(14, LOGIC, 0), (14, LOGIC, 3), (14, LOGIC, 4)],
    "fbsm": [(24, FIXED_ADD, 2)],
    "curve_add": [(31, VAR_ADD, 0), (31, VAR_ADD, 2)],
    "no_pis": [(1, ARITH, 0), (4, ARITH, 0)],
    "lookup_outside": [(35, LOOKUP, 0)],
}


@pytest.mark.parametrize("kind", ["arith_qm_pis", "range", "logic", "fbsm", "curve_add", "lookup", "all"])
def test_satisfying_circuits_have_no_violation(kind):
    cp = make_circuit(kind)
    inp = cp.build()
    sel, w, table, var = composer_columns(cp)
    assert check_columns_ref(sel, w, inp.n, sorted(cp.pis.items()), table, var=var) == []


def test_satisfying_merkle_circuit_has_no_violation():
    import merkle_circuit as mc
    cp = mc.merkle_circuit(4, seed=11)[0]
    inp = cp.build()
    assert (inp.n_gates, inp.n) == (1356, 2048) and list(cp.pis) == [1355]
    assert check_ref(cp, inp.n, sorted(cp.pis.items())) == []


@pytest.mark.parametrize("name", MUTATIONS)
def test_model_names_the_broken_constraint(name):
    cp, pis = mutated_all(name)
    inp = cp.build()
    assert (inp.n_gates, inp.n) == (43, 64)
    got = check_ref(cp, inp.n, pis)
    assert got == EXPECTED[name]
    rep = report_of(got, 1)
    assert rep["violations"] == len(got) == sum(rep["by_kind"])
    assert (rep["first_row"], rep["first_kind"], rep["first_index"]) == got[0]


def _oracle_rc_and_proof(inp, pis):
    lib = oracle()
    out = abi.ProofC()
    import numpy as np
    from pnp_testlib import to_limbs
    pos = np.array([p for p, _ in pis] or [0], dtype=np.uint64)
    vals = np.array([to_limbs(v, 4) for _, v in pis] or [[0] * 4], dtype=np.uint64).reshape(-1, 4)
    lib.or_gen_proof_ex.argtypes = [C.c_void_p] * 3 + [C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p]
    lib.or_gen_proof_ex.restype = C.c_int
    rc = lib.or_gen_proof_ex(C.byref(inp.circuit), C.byref(inp.pk), C.byref(inp.ck), len(pis), vp(pos), vp(vals),
                             b"Merkle tree", C.byref(out))
    return rc, out


def test_unmutated_circuit_is_accepted_by_the_verifier():
    cp, pis = mutated_all(None)
    inp = cp.build()
    assert check_ref(cp, inp.n, pis) == [] and pis == pis_of(inp)
    rc, proof = _oracle_rc_and_proof(inp, pis)
    assert rc == 0
    assert verify(inp.vk(), proof, pis, inp.tau_mont[0])


@pytest.mark.parametrize("name", MUTATIONS)
def test_what_the_model_flags_the_verifier_rejects(name):
    cp, pis = mutated_all(name)
    inp = cp.build()
    assert check_ref(cp, inp.n, pis) != []
    rc, proof = _oracle_rc_and_proof(inp, pis)
    if name == "lookup_outside":
        assert rc == -1  # Error::ElementNotIndexed: the prover itself stops
        return
    assert rc == 0
    assert not verify(inp.vk(), proof, pis, inp.tau_mont[0])


def test_copy_model_flags_the_changed_slot():
    cp = make_circuit("all")
    inp = cp.build()
    sel, w, table, var = composer_columns(cp)
    # gate 7 reuses gate 6's variables: wire 1 of row 7 is wire 0 of row 6
    assert var[1][7] == var[0][6]
    w[1][7] = (w[1][7] + 1) % R_MOD
    got = check_columns_ref(sel, w, inp.n, sorted(cp.pis.items()), table, var=var)
    assert (7, COPY, 1) in got and [v for v in got if v[1] == COPY] == [(7, COPY, 1)]
    # without the map only the gate the value enters is flagged
    assert check_columns_ref(sel, w, inp.n, sorted(cp.pis.items()), table) == [v for v in got if v[1] != COPY]


def test_lookup_model_query_rule():
    t = [(1, 2, 3, 4), (5, 6, 7, 8), (5, 6, 7, 8), (9, 9, 9, 9)]
    w = [[5, 1, 9, 5, 1], [6, 2, 9, 6, 0], [7, 3, 9, 7, 0], [8, 4, 9, 8 + (1 << 224), 0]]
    key = {"q_lookup": [1, 1, 1, 1, 1]}
    # the key's rows: the duplicated, first and last table rows pass; a top-word difference and a stranger do not
    assert check_columns_ref(key, w, 8, [], t) == [(3, LOOKUP, 0), (4, LOOKUP, 0)]
    # the caller selects nothing: T[0] is queried where the key expects the wires
    assert check_columns_ref(key, w, 8, [], t, s=[0] * 5) == [(i, LOOKUP, 1) for i in (0, 2, 3, 4)]


def test_check_ctypes_signatures():
    sig = abi.CHECK_ARGTYPES
    assert sorted(sig) == ["pnp_check_assignment", "pnp_check_witness"]
    rep = C.POINTER(abi.CheckReport)
    assert sig["pnp_check_assignment"] == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p,
                                           C.c_void_p, rep]
    assert sig["pnp_check_witness"] == [C.c_void_p, C.POINTER(abi.CircuitC), C.c_int, C.c_uint64, C.c_void_p,
                                        C.c_void_p, rep]
    assert C.sizeof(abi.CheckReport) == 88 and abi.CheckReport.first_row.offset == 64
    assert abi.CheckReport.copy_checked.offset == 80 and len(abi.CHECK_KINDS) == KINDS
    assert abi.PNP_E_UNSAT == -6
    import pnp
    assert pnp.ERRORS[abi.PNP_E_UNSAT] == "PNP_E_UNSAT"
    lib = pnp.load()
    for name, argtypes in sig.items():
        assert name in pnp.SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is C.c_int
    for meth in ("check_assignment", "check_witness"):
        assert callable(getattr(pnp.Context, meth))
