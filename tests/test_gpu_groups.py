"""The copy-group commitments (csrc/wires.hip) on permutations other than the
Merkle circuit's, on the MI355X.

Proof bytes cannot see a broken builder: a labelling that splits a cycle still
sums the right Lagrange points, one that merges two is caught by the per-proof
check and the proof falls back to row-by-row commitments.  So every case holds
the builder to the CPU model of tests/groups_ref.py through the counters of a
timed proof — the four used / fallback counters and, per segment (a, b, c, d,
z), groups_found_* and groups_heavy_* — besides the bytes: the second proof of
a context (the first defers the tables, tests/gpu_util.py proof_after_tables)
equals the first and the oracle's byte for byte, _diff names no field, and the
restated verifier accepts it when the witness satisfies.
tests/test_groups_ref.py holds every circuit here to the edge its case is for.

Two things differ from a literal reading of the cases.  The heavy wire groups
(b) and the broken constraints on them (g) run at 2^15: runs of 257, 256 and
300 pieces take at least 8162 + 8130 + 9538 sorted positions of one wire, more
than 2^14.  And the two other roads to the commitments (i) take (e)'s circuit
with its cycles in slot order: pnp_preprocess builds sigma from the wire map
and pnp_load_wire_map compares the key's sigma with it, both in slot order.

The z fallback (z_group_fallback) has no case: it needs the ratio of a row
that sigma fixes to differ from 1, i.e. a zero denominator under the
Fiat-Shamir challenges beta and gamma, which cannot be constructed."""
import copy
import functools

import pytest

import group_circuits as gc
from groups_ref import COUNTERS, model_of, witness_columns
from pnp import abi
from test_general import check_accepts, pis_of
from test_gpu_prove import _diff

pytestmark = pytest.mark.gpu


def _pis(inp):
    from pnp_testlib import inputs_pis
    return pis_of(inp) if hasattr(inp, "pis") else inputs_pis(inp)


def _columns(inp):
    return lambda ctx: ctx.prove_ex(inp.circuit, False, _pis(inp))


def _same(got, exp):
    assert _diff(got, exp) == []
    assert abi.proof_to_bytes(got) == abi.proof_to_bytes(exp)


def check(case, inp=None, exp=None, accept=True, prove=None, load=None, after=None):
    """The second proof of a fresh context over inp (default: the case's own
    inputs) against the oracle and the model of the case's permutation."""
    from gpu_util import host_keys, second_proof_counters
    if inp is None:
        inp, exp = case.inputs, case.oracle
    elif exp is None:
        exp = inp.oracle_proof()
    got, c = second_proof_counters(load or host_keys(inp), prove or _columns(inp), COUNTERS, after)
    _same(got, exp)
    if accept:
        check_accepts(inp, got)
    assert c == case.model.counters(witness_columns(inp))
    assert c["wire_group_fallback"] == 0 or not accept
    return got, c


# ---------------------------------------------------------------- (a) .. (f)
def test_every_start_offset_and_piece_shape():
    _, c = check(gc.case_a())
    assert (c["wire_groups_used"], c["z_groups_used"]) == (1, 0)


def test_heavy_groups_in_a_wire():
    _, c = check(gc.case_b())
    assert c["groups_heavy_a"] == 2 and c["wire_groups_used"] == 1 and c["z_groups_used"] == 1


@pytest.mark.parametrize("kind,heavy", [("boundary", 0), ("heavy", 1), ("middle", 1)])
def test_heavy_z_run_and_its_boundary(kind, heavy):
    _, c = check(gc.case_c(kind))
    assert c["groups_heavy_z"] == heavy and (c["wire_groups_used"], c["z_groups_used"]) == (0, 1)


@pytest.mark.parametrize("shuffled", [True, False], ids=["shuffled", "slot_order"])
def test_one_cycle_through_everything(shuffled):
    _, c = check(gc.case_d(shuffled))
    assert [c["groups_found_" + s] for s in "abcd"] == [4] * 4 and c["wire_groups_used"] == 1


def test_cycles_across_wires():
    _, c = check(gc.case_e())
    assert (c["wire_groups_used"], c["z_groups_used"]) == (1, 1)


@pytest.mark.parametrize("kind,used", [("mixed", (1, 1)), ("z_alone", (0, 1)), ("wires_alone", (1, 0))])
def test_thresholds(kind, used):
    _, c = check(gc.case_f(kind))
    assert (c["wire_groups_used"], c["z_groups_used"]) == used
    assert (c["wire_group_fallback"], c["z_group_fallback"]) == (0, 0)


def test_thresholds_nothing_grouped():
    """pnp_testlib.Inputs: a <-> b 2-cycles only.  Nothing is grouped, and a
    later proof still equals the oracle."""
    from pnp_testlib import Inputs, inputs_vk, verify
    inp = Inputs(10, 21)
    exp = inp.oracle_proof()
    m = model_of(inp)

    def third(ctx, got):
        _same(ctx.prove_ex(inp.circuit, False, _pis(inp)), exp)
    from gpu_util import host_keys, second_proof_counters
    got, c = second_proof_counters(host_keys(inp), _columns(inp), COUNTERS, third)
    _same(got, exp)
    assert verify(inputs_vk(inp), got, _pis(inp), inp.tau_mont[0])
    assert c == m.counters()
    assert [c[k] for k in COUNTERS[:4]] == [0, 0, 0, 0]
    assert [c["groups_found_" + s] for s in "abcdz"] == [1024] * 4 + [inp.n_gates + 1]


# ---------------------------------------------------------------- (g)
def _changed(inp, column, row):
    """inp with one witness value changed (still < r: another field element);
    the shared instance stays as it is."""
    v = copy.copy(inp)
    v.arrays = dict(inp.arrays)
    v.arrays[column] = inp.arrays[column].copy()
    v.arrays[column][row, 0] ^= 1
    v._build_structs()
    return v


@pytest.mark.parametrize("which", ["heavy_last_row", "far_from_representative", "ident_wire"])
def test_broken_copy_constraint_outside_merkle(which):
    """(b)'s circuit with one row of a group changed.  In a grouped wire the
    per-proof check sends round 1 back to the row-by-row commitment; in an
    ident wire nothing reads the groups.  The bytes are the oracle's either
    way (it commits every row)."""
    case = gc.case_b()
    runs = case.facts["run_rows"]
    column, row = {"heavy_last_row": ("w_l", runs[0][-1]),
                   "far_from_representative": ("w_l", runs[1][len(runs[1]) // 2]),
                   "ident_wire": ("w_o", case.facts["c_rows"][1])}[which]
    _, c = check(case, _changed(case.inputs, column, row), accept=False)
    fell = which != "ident_wire"
    assert (c["wire_groups_used"], c["wire_group_fallback"]) == ((0, 1) if fell else (1, 0))
    assert (c["z_groups_used"], c["z_group_fallback"]) == (1, 0)


# ---------------------------------------------------------------- (h)
@functools.lru_cache(maxsize=None)
def _h_split_inputs():
    """Q's instance under P's SRS (each instance draws its own)."""
    from circuits import GeneralInputs
    P, Q = gc.case_h(False), gc.case_h(True)
    inp = GeneralInputs(Q.cp, Q.n)
    inp.arrays["srs"], inp.tau_mont = P.inputs.arrays["srs"], P.inputs.tau_mont
    inp._build_structs()
    return inp, inp.oracle_proof()


def test_keys_changing_under_live_groups():
    import pnp
    from gpu_util import proof_after_tables
    P, Q = gc.case_h(False), gc.case_h(True)
    p, exp_p = P.inputs, P.oracle
    q, exp_q = _h_split_inputs()
    assert Q.model.g[0] == P.model.g[0] + 1
    ctx = pnp.Context(0)
    try:
        ctx.load_prover_key(p.pk, p.n, device_ptrs=False)
        ctx.load_commit_key(p.ck, p.n, device_ptrs=False)
        for k, (case, inp, exp) in enumerate(((P, p, exp_p), (Q, q, exp_q), (P, p, exp_p))):
            if k:  # the other circuit's key over the groups of the one before
                ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
            got, c = proof_after_tables(ctx, _columns(inp), COUNTERS)
            _same(got, exp)
            # (stale groups would show as wire_group_fallback 1, or as the other key's counts)
            assert c == case.model.counters(witness_columns(inp))
            assert c["wire_groups_used"] == 1
            check_accepts(inp, got)
        # the same key loaded again: the groups are kept and the very next proof uses them
        ctx.load_prover_key(p.pk, p.n, device_ptrs=False)
        ctx.kernel_timing(True)
        _same(ctx.prove_ex(p.circuit, False, _pis(p)), exp_p)
        assert {k: ctx.kernel_bytes(k) for k in COUNTERS} == P.model.counters()
    finally:
        ctx.close()


# ---------------------------------------------------------------- (i)
@pytest.mark.parametrize("road", ["preprocess", "wire_map"])
def test_other_roads_to_the_same_commitments(road):
    """(e)'s circuit in slot order through pnp_preprocess (sigma built on the
    device from the wire map) and through pnp_load_prover_key_coeffs +
    pnp_load_wire_map, proved from the assignment: the model's counts, and
    the bytes of pnp_prove_ex and the oracle."""
    from test_assignment_ref import assignment_values
    from test_gpu_assignment import host_cols, load_coeff_key
    from test_gpu_preprocess import Desc
    from test_preprocess_ref import wire_map
    case = gc.case_e(False)
    cp, inp = case.cp, case.inputs
    var, values = wire_map(cp), assignment_values(cp)
    keep = []

    def load(ctx):
        if road == "preprocess":
            ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
            keep.append(Desc(cp, inp))
            ctx.preprocess(keep[-1].d, device_ptrs=False)
        else:
            load_coeff_key(ctx, inp)
            cols, addrs = host_cols(var)
            keep.append(cols)
            ctx.load_wire_map(addrs, var.shape[1], len(cp.vals), device_ptrs=False)

    def prove(ctx):
        return ctx.prove_assignment(values.ctypes.data, values.shape[0], False, _pis(inp))

    def columns_too(ctx, got):
        _same(ctx.prove_ex(inp.circuit, False, _pis(inp)), got)
    _, c = check(case, prove=prove, load=load, after=columns_too)
    assert (c["wire_groups_used"], c["z_groups_used"]) == (1, 1)
