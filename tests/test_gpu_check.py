"""The satisfiability check on the MI355X: pnp_check_assignment and
pnp_check_witness (csrc/check.hip, csrc/check_witness.cpp) against the plain-integer
model of tests/test_check_ref.py.  A satisfied witness gives PNP_OK and a zero
report; a violated one PNP_E_UNSAT and a report equal to the model's in every
field (counts by kind, the first (row, kind, index)), whatever order the
kernels' atomics land in.  No proof is needed but for the isolation test:
every case is pnp_preprocess + the check.

The row kernels run one lane a row, 256 rows a workgroup: D = 16 is a quarter
of one workgroup, merkle6 (D = 8192) is 32 of them."""
import ctypes as C
import functools

import numpy as np
import pytest

from circuits import R_MOD, SEL
from pnp import abi
from pnp_testlib import fr_mont, ints_to_arr, ptr_of
from test_assignment_ref import assignment_values
from test_check_ref import (ARITH, COPY, LOOKUP, RANGE, MUTATIONS, check_columns_ref, check_ref, composer_columns,
                            mutated_all, report_of)
from test_general import make_circuit
from test_gpu_preprocess import Desc
from test_preprocess_ref import wire_map

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
KIND_NAME = abi.CHECK_KINDS


def report_dict(rep: abi.CheckReport):
    return {"violations": rep.violations, "by_kind": list(rep.by_kind), "first_row": rep.first_row,
            "first_kind": rep.first_kind, "first_index": rep.first_index, "copy_checked": rep.copy_checked}


def expect(ctx, got, violations, copy_checked):
    """(ok, report) of a check equals the model's violation list."""
    ok, rep = got
    assert report_dict(rep) == report_of(violations, copy_checked)
    assert ok == (not violations) and rep.reserved == 0
    if violations:
        row, kind, index = violations[0]
        assert f"row {row}: {KIND_NAME[kind]} constraint {index}" in ctx.last_error()


@functools.lru_cache(maxsize=None)
def circuit(kind):
    """(composer, instance, public inputs) of a satisfying circuit, made once, never mutated."""
    import merkle_circuit as mc
    cp = mc.merkle_circuit(int(kind[len("merkle"):]), seed=11)[0] if kind.startswith("merkle") else make_circuit(kind)
    return cp, cp.build(), sorted(cp.pis.items())


def context_for(cp, inp, with_map=True):
    """A context with the circuit's key resident: through pnp_preprocess (the
    wire map stays), or through the coefficient load (no map)."""
    import pnp
    from test_gpu_assignment import coeff_pk
    ctx = pnp.Context(0)
    if with_map:
        desc = Desc(cp, inp)
        ctx.preprocess(desc.d, device_ptrs=False)
    else:
        ctx.load_prover_key_coeffs(coeff_pk(inp), inp.n, device_ptrs=False)
    return ctx


def check_both_forms(ctx, cp, inp, pis, device):
    """[(ok, report)] of the assignment form and the columns form of a
    Composer's own witness, from host memory or from HBM."""
    from gpu_util import to_dev
    values = assignment_values(cp)
    n_vars = len(cp.vals)
    if not device:
        return [ctx.check_assignment(values.ctypes.data, n_vars, False, pis),
                ctx.check_witness(inp.circuit, False, pis)]
    dv = to_dev(values)
    cols = {k: to_dev(inp.arrays[k]) for k in ("q_lookup", "w_l", "w_r", "w_o", "w_4")}
    cs = abi.CircuitC(n=inp.n_gates, lookup_len=inp.lookup_len, intended_pi_pos=0, pi=None,
                      **{k: abi.ptr(t.data_ptr()) for k, t in cols.items()})
    return [ctx.check_assignment(dv.data_ptr(), n_vars, True, pis), ctx.check_witness(cs, True, pis)]


# ------------------------------------------------------------------ satisfied
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", ["arith_qm_pis", "range", "logic", "fbsm", "curve_add", "lookup", "all",
                                  "merkle4", "merkle6"])
def test_satisfied_witness_is_ok(kind, device):
    cp, inp, pis = circuit(kind)
    if kind == "merkle6":
        assert (inp.n_gates, inp.n) == (5988, 8192)
    if kind == "all":
        assert (inp.n_gates, inp.n) == (43, 64)
    elif not kind.startswith("merkle"):
        assert inp.n == 16 or kind == "arith_qm_pis"
    ctx = context_for(cp, inp)
    try:
        for got in check_both_forms(ctx, cp, inp, pis, device):
            expect(ctx, got, [], 1)
            assert got[1].first_row == NONE
        names = [n for n, _ in ctx.stage_times()]
        assert names == ["check_inputs", "check_rows_ntt", "check_rows", "check_lookup", "check_copy"]
        # a NULL report is allowed
        assert ctx.lib.pnp_check_witness(ctx.h, C.byref(inp.circuit), 0, 0, None, None, None) in (0, abi.PNP_E_UNSAT)
    finally:
        ctx.close()


# ------------------------------------------------------------------ violated
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", MUTATIONS)
def test_mutations_of_all_families(name, device):
    """+ 1 on wire a of the first gate of a family, the public inputs dropped,
    a lookup outside the table: the report is the model's."""
    good, good_inp, _ = circuit("all")
    cp, pis = mutated_all(name)
    inp = cp.build()
    exp = check_ref(cp, inp.n, pis)
    assert exp
    ctx = context_for(good, good_inp)  # (the key is the unmutated circuit's: the same selectors and map)
    try:
        for got in check_both_forms(ctx, cp, inp, pis, device):
            expect(ctx, got, exp, 1)
        # ... and the same report again (no dependence on the order of the atomics)
        again = check_both_forms(ctx, cp, inp, pis, device)
        assert [bytes(r) for _, r in again] == [bytes(got[1])] * 2
    finally:
        ctx.close()


def test_violations_in_different_workgroups():
    """merkle6 (5,988 rows, D = 8192): one defect below row 4096 and one beyond."""
    import merkle_circuit as mc
    good, good_inp, pis = circuit("merkle6")
    cp = mc.merkle_circuit(6, seed=11)[0]
    for row in (700, 5000):
        v = cp.rows[row][1][0]
        cp.vals[v] = (cp.vals[v] + 1) % R_MOD
    inp = cp.build()
    exp = check_ref(cp, inp.n, pis)
    rows = sorted({r for r, _, _ in exp})
    assert rows[0] < 4096 < rows[-1] and rows[0] // 256 != rows[-1] // 256
    assert all(k == ARITH for _, k, _ in exp) and len(exp) >= 2
    ctx = context_for(good, good_inp)
    try:
        for got in check_both_forms(ctx, cp, inp, pis, False):
            expect(ctx, got, exp, 1)
    finally:
        ctx.close()


# ------------------------------------------------------------------ raw columns (next-row edges, lookup)
class Raw:
    """A circuit given as raw columns: sel[name] = {row: value}, w = {(row,
    wire): value} (canonical ints), every slot its own variable.  desc() is
    the pnp_circuit_desc, circuit() the witness columns (s: the caller's
    q_lookup rows, default the key's)."""

    def __init__(self, n_gates, sel, w, table=()):
        self.ng, self.table = n_gates, [tuple(r) for r in table]
        self.sel = {name: [rows.get(i, 0) % R_MOD for i in range(n_gates)] for name, rows in sel.items()}
        self.w = [[w.get((i, j), 0) % R_MOD for i in range(n_gates)] for j in range(4)]
        self.D = 1
        while self.D < max(n_gates, len(self.table)):
            self.D <<= 1
        self.keep = []

    def _arr(self, vals):
        self.keep.append(ints_to_arr([fr_mont(v) for v in vals]))
        return ptr_of(self.keep[-1])

    def desc(self):
        d = abi.CircuitDesc(n_gates=self.ng, n_vars=4 * self.ng, lookup_len=len(self.table))
        for j in range(4):
            self.keep.append(np.arange(j, 4 * self.ng, 4, dtype=np.uint32))
            d.var[j] = self.keep[-1].ctypes.data_as(abi.U32P)
        for k, name in enumerate(abi.DESC_SELECTORS):
            if any(self.sel.get(name, [])):
                d.sel[k] = self._arr(self.sel[name])
        for j in range(4):
            if self.table:
                d.table[j] = self._arr([row[j] for row in self.table])
        return d

    def circuit(self, w=None, s=None):
        w = self.w if w is None else w
        s = self.sel.get("q_lookup", [0] * self.ng) if s is None else s
        return abi.CircuitC(n=self.ng, lookup_len=len(self.table), intended_pi_pos=0, pi=None,
                            q_lookup=self._arr(s), w_l=self._arr(w[0]), w_r=self._arr(w[1]), w_o=self._arr(w[2]),
                            w_4=self._arr(w[3]))

    def model(self, w=None, s=None):
        return check_columns_ref(self.sel, self.w if w is None else w, self.D, [], self.table, s=s,
                                 var=[list(range(j, 4 * self.ng, 4)) for j in range(4)])


def range_row(d_next, quads):
    """(a, b, c, d) of a range gate whose next row holds d_next: d_next = 4a +
    q3, a = 4b + q2, b = 4c + q1, c = 4d + q0, solved backwards in the field."""
    inv4 = pow(4, -1, R_MOD)
    a = (d_next - quads[3]) * inv4 % R_MOD
    b = (a - quads[2]) * inv4 % R_MOD
    c = (b - quads[1]) * inv4 % R_MOD
    d = (c - quads[0]) * inv4 % R_MOD
    return a, b, c, d


def run_raw(raw, cases):
    """cases: [(w or None, s or None)]; each checked on the columns form against the model."""
    import pnp
    ctx = pnp.Context(0)
    try:
        ctx.preprocess(raw.desc(), device_ptrs=False)
        for w, s in cases:
            expect(ctx, ctx.check_witness(raw.circuit(w, s), False, []), raw.model(w, s), 1)
    finally:
        ctx.close()


def test_range_gate_on_the_last_gate_row_reads_a_padding_row():
    """n_gates = 11 < D = 16: next of row 10 is the zero row 11."""
    a, b, c, d = range_row(0, (1, 2, 3, 1))
    assert a and b and c and d
    raw = Raw(11, {"range_selector": {10: 1}}, {(10, 0): a, (10, 1): b, (10, 2): c, (10, 3): d})
    assert raw.D == 16 and raw.model() == []
    bad = [list(col) for col in raw.w]
    bad[0][10] = (a + 1) % R_MOD  # d_next - 4a = -4 - q3 and a - 4b = q2 + 1
    assert (10, RANGE, 3) in raw.model(bad)
    run_raw(raw, [(None, None), (bad, None)])


def test_range_gate_on_row_D_minus_1_wraps_to_row_0():
    """n_gates = D = 16: next of row 15 is row 0, once satisfied by its d, once not."""
    d0 = 0x1234567
    a, b, c, d = range_row(d0, (3, 0, 2, 1))
    raw = Raw(16, {"range_selector": {15: 1}},
              {(15, 0): a, (15, 1): b, (15, 2): c, (15, 3): d, (0, 3): d0})
    assert raw.D == 16 and raw.model() == []
    bad = [list(col) for col in raw.w]
    bad[3][0] = d0 + 4  # another quad's worth: d_next - 4a = q3 + 4
    assert raw.model(bad) == [(15, RANGE, 3)]
    run_raw(raw, [(None, None), (bad, None)])


def _lookup_cases(table, ng, rows):
    """Queries at `rows` of: the first, the last, a chosen table row, a tuple
    that differs from a table row only in the top word of d, and T[0] with the
    caller's selector off."""
    first, last, dup = table[0], table[-1], table[1]
    # (in the Montgomery words the library holds: d' R = d R +- 2^224)
    step = (1 << 224) if fr_mont(dup[3]) + (1 << 224) < R_MOD else -(1 << 224)
    top = dup[:3] + ((dup[3] + step * pow(1 << 256, -1, R_MOD)) % R_MOD,)
    assert fr_mont(top[3]) == fr_mont(dup[3]) + step and fr_mont(top[3]) % (1 << 224) == fr_mont(dup[3]) % (1 << 224)
    q = dict(zip(rows, (first, last, dup, top, first)))
    raw = Raw(ng, {"q_lookup": {r: 1 for r in rows}}, {(r, j): t[j] for r, t in q.items() for j in range(4)}, table)
    exact = [(rows[3], LOOKUP, 0)]
    assert raw.model() == exact
    # the caller's selector all zero: T[0] is queried, rows holding T[0] pass (index 1 elsewhere)
    s0 = [0] * ng
    assert raw.model(None, s0) == [(r, LOOKUP, 1) for r in sorted(rows[1:4])]
    # ... and off on one key lookup row only: that row once with the table's first row, once with another
    s1 = list(raw.sel["q_lookup"])
    s1[rows[4]] = 0
    s2 = list(raw.sel["q_lookup"])
    s2[rows[1]] = 0
    assert raw.model(None, s1) == exact and raw.model(None, s2) == sorted(exact + [(rows[1], LOOKUP, 1)])
    return raw, [(None, None), (None, s0), (None, s1), (None, s2)]


def _rand_table(seed, rows):
    rng = np.random.default_rng(seed)
    return [tuple(int.from_bytes(rng.bytes(32), "little") % R_MOD for _ in range(4)) for _ in range(rows)]


def test_lookup_three_row_table_padded_to_8192():
    """The resident table is 3 rows and 8,189 copies of row 0."""
    table = _rand_table(1, 3)
    raw, cases = _lookup_cases(table, 5000, (3, 300, 4097, 4500, 4999))
    assert raw.D == 8192
    run_raw(raw, cases)


def test_lookup_table_with_an_interior_duplicate_row():
    t = _rand_table(2, 4)
    table = [t[0], t[1], t[2], t[1], t[3]]
    raw, cases = _lookup_cases(table, 12, (0, 2, 5, 7, 11))
    assert raw.D == 16
    run_raw(raw, cases)


# ------------------------------------------------------------------ copy constraints (columns form)
def test_copy_constraints_with_and_without_a_resident_map():
    cp, inp, pis = circuit("all")
    sel, w, table, var = composer_columns(cp)
    assert var[1][7] == var[0][6]  # gate 7 reuses gate 6's variables
    w[1][7] = (w[1][7] + 1) % R_MOD
    with_map = check_columns_ref(sel, w, inp.n, pis, table, var=var)
    without = check_columns_ref(sel, w, inp.n, pis, table)
    assert [v for v in with_map if v[1] == COPY] == [(7, COPY, 1)] and without and COPY not in [v[1] for v in without]
    keep = [ints_to_arr([fr_mont(v) for v in col]) for col in w]
    cs = abi.CircuitC(n=inp.n_gates, lookup_len=inp.lookup_len, intended_pi_pos=0, pi=None,
                      q_lookup=ptr_of(inp.arrays["q_lookup"]), w_l=ptr_of(keep[0]), w_r=ptr_of(keep[1]),
                      w_o=ptr_of(keep[2]), w_4=ptr_of(keep[3]))
    ctx = context_for(cp, inp, with_map=True)
    try:
        expect(ctx, ctx.check_witness(cs, False, pis), with_map, 1)
    finally:
        ctx.close()
    ctx = context_for(cp, inp, with_map=False)
    try:
        expect(ctx, ctx.check_witness(cs, False, pis), without, 0)
        expect(ctx, ctx.check_witness(inp.circuit, False, pis), [], 0)
    finally:
        ctx.close()


# ------------------------------------------------------------------ isolation from proofs
def test_a_check_changes_no_later_proof():
    from test_general import pis_of
    cp, inp, pis = circuit("all")
    exp = abi.proof_to_bytes(inp.oracle_proof())
    bad, bad_pis = mutated_all("fbsm")
    bad_inp = bad.build()
    ctx = context_for(cp, inp)
    try:
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
        ctx.kernel_timing(True)
        assert abi.proof_to_bytes(ctx.prove_ex(inp.circuit, False, pis_of(inp))) == exp
        ctx.sync()  # (the optional tables of the first proof are built)
        assert abi.proof_to_bytes(ctx.prove_ex(inp.circuit, False, pis_of(inp))) == exp
        stages = [n for n, _ in ctx.stage_times()]
        fallbacks = ctx.kernel_bytes("quotient_all_blocks")
        ctx.sync()
        hbm = ctx.hbm_usage()
        ok, rep = ctx.check_witness(bad_inp.circuit, False, bad_pis)
        assert not ok and rep.violations
        assert ctx.kernel_stats("check_rows")[1] == 1
        after = ctx.hbm_usage()
        assert after["live"] == hbm["live"] and [after[k] for k in ("mandatory", "lagrange", "groups", "transient")] \
            == [hbm[k] for k in ("mandatory", "lagrange", "groups", "transient")]
        assert abi.proof_to_bytes(ctx.prove_ex(inp.circuit, False, pis_of(inp))) == exp
        assert [n for n, _ in ctx.stage_times()] == stages
        assert ctx.kernel_bytes("quotient_all_blocks") == fallbacks
    finally:
        ctx.close()


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_context_proving():
    import pnp
    from test_general import pis_of
    cp, inp, pis = circuit("all")
    values = assignment_values(cp)
    n_vars = len(cp.vals)
    ctx = pnp.Context(0)
    try:
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.check_witness(inp.circuit, False, pis)
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.check_assignment(values.ctypes.data, n_vars, False, pis)
    finally:
        ctx.close()
    ctx = context_for(cp, inp, with_map=False)
    try:
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY.*no wire map"):
            ctx.check_assignment(values.ctypes.data, n_vars, False, pis)
        desc = Desc(cp, inp)
        ctx.preprocess(desc.d, device_ptrs=False)
        longer = np.concatenate([values, values[:1]])
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG"):
            ctx.check_assignment(longer.ctypes.data, n_vars + 1, False, pis)
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG"):
            ctx.check_assignment(values.ctypes.data, n_vars - 1, False, pis)
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG.*given twice"):
            ctx.check_witness(inp.circuit, False, [pis[0], pis[0]])
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG.*out of range"):
            ctx.check_witness(inp.circuit, False, [(inp.n, 1)])
        assert ctx.check_assignment(values.ctypes.data, n_vars, False, pis)[0]
        assert abi.proof_to_bytes(ctx.prove_ex(inp.circuit, False, pis_of(inp))) == abi.proof_to_bytes(inp.oracle_proof())
    finally:
        ctx.close()


def test_check_refuses_a_sharded_context():
    import pnp
    import torch
    from pnp.shard import SoloExchange, a2a_bytes_for, v_bytes_for
    cp, inp, pis = circuit("all")
    ctx = context_for(cp, inp)
    try:
        solo = SoloExchange(1, 2, device=torch.device("cuda", 0), a2a_bytes=a2a_bytes_for(inp.lg_n, 2),
                            v_bytes=v_bytes_for(inp.lg_n, 2))
        ctx.set_msm_shard(solo)
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG.*ranks"):
            ctx.check_witness(inp.circuit, False, pis)
        values = assignment_values(cp)
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG.*ranks"):
            ctx.check_assignment(values.ctypes.data, len(cp.vals), False, pis)
    finally:
        ctx.close()
