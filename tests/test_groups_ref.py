"""The CPU model of the copy-group builder (tests/groups_ref.py) pinned on
permutations small enough to count by hand and on the Merkle circuit, and the
circuits of tests/test_gpu_groups.py held to the property each of its cases
needs — the exact group counts, the piece counts 256 and 257, the sides of the
thresholds — so a GPU case that no longer exercises its edge fails here."""
from collections import Counter

import pytest

import group_circuits as gc
from circuits import Composer, sigma_columns
from groups_ref import GroupModel, HEAVY, model_of, pieces, sigma_of, witness_columns


# ---------------------------------------------------------------- by hand
def _hand(cycle_seed=None):
    """n = 8, 5 gates.  x in a0, d0, a1, a3; y in b0, c1, d3; rows 2 and 4 and
    every other slot fresh."""
    cp = Composer(1)
    f = lambda: cp.var(cp.rnd())  # noqa: E731
    x, y = f(), f()
    cp.row({}, x, y, f(), x)
    cp.row({}, x, f(), y, f())
    cp.row({}, f(), f(), f(), f())
    cp.row({}, x, f(), f(), y)
    cp.row({}, f(), f(), f(), f())
    return cp, GroupModel(sigma_columns(cp, 8, cycle_seed), 8)


def test_hand_counted_permutation():
    _, m = _hand()
    n = 8
    # slot order: (a,0) -> (d,0) -> (a,1) -> (a,3) -> ; (b,0) -> (c,1) -> (d,3) ->
    assert [m.next[p] for p in (0, 24, 1, 3)] == [24, 1, 3, 0]
    assert [m.next[p] for p in (8, 17, 27)] == [17, 27, 8]
    moved = {0, 24, 1, 3, 8, 17, 27}
    assert all(m.next[p] == p for p in range(4 * n) if p not in moved)
    assert sorted(map(sorted, (c for c in m.cycles if len(c) > 1))) == [[0, 1, 3, 24], [8, 17, 27]]
    assert len(m.cycles) == 32 - 7 + 2
    assert m.groups[0] == [[0, 1, 3], [2], [4], [5], [6], [7]]
    assert m.groups[1] == [[i] for i in range(8)]
    # wire c: row 1 holds y, whose label 8 is a position of wire b: it comes first
    assert m.groups[2] == [[1], [0], [2], [3], [4], [5], [6], [7]]
    # wire d: row 0 (x, label 0), row 3 (y, label 8), then the single rows
    assert m.groups[3] == [[0], [3], [1], [2], [4], [5], [6], [7]]
    # z: rows 0, 1, 3 are moved: runs start at 0, 1, 2, 4
    assert m.groups[4] == [[0], [1], [2, 3], [4, 5, 6, 7]]
    assert m.g == [6, 8, 8, 8, 4]
    assert m.runs[0] == [(0, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8)]
    assert m.pieces[0] == [1] * 6 and m.heavy == [0] * 5
    # 10 g > 9 n: 60, 80 > 72; 4 g < 3 n: 24 < 24 is false; z: 40 > 72 is false
    assert m.ident == [False, True, True, True, False]
    assert not m.wires_ok and m.z_ok


def test_any_cyclic_order_is_the_same_groups():
    _, m = _hand()
    _, s = _hand(cycle_seed=2)
    assert s.next != m.next
    assert s.groups == m.groups and s.g == m.g and s.label == m.label


def test_identity_sigma():
    n = 4
    w = sigma_columns(Composer(1), n)  # no rows: the identity
    m = GroupModel(w, n)
    assert m.next == list(range(16))
    assert m.g == [4, 4, 4, 4, 1] and m.groups[4] == [[0, 1, 2, 3]]
    assert m.ident == [True] * 4 + [False] and not m.wires_ok and m.z_ok


def test_piece_arithmetic():
    assert pieces(0, 1) == 1 and pieces(0, 32) == 1 and pieces(0, 33) == 2
    assert pieces(31, 33) == 2 and pieces(31, 32) == 1 and pieces(32, 33) == 1
    assert pieces(0, 8192) == 256 and pieces(0, 8193) == 257
    # the fewest positions that make 257 pieces: one in the first, one in the last
    assert pieces(31, 8193) == 257 and 8193 - 31 == 255 * 32 + 2
    assert pieces(32, 8193) == 256 and pieces(31, 8192) == 256
    assert pieces(8193, 16384) == 256 and pieces(8161, 16384) == 257


def test_one_value_per_group():
    cp, m = _hand()
    cols = [[cp.vals[r[1][j]] for r in cp.rows] + [0] * 3 for j in range(4)]
    assert m.witness_keeps_groups(cols) and all(m.one_value(cols[j], j) for j in range(4))
    assert m.counters(cols)["wire_group_fallback"] == 0
    cols[0][3] += 1  # x's third row of wire a
    assert not m.one_value(cols[0], 0) and not m.witness_keeps_groups(cols)
    cols[0][3] -= 1
    cols[3][0] += 1  # wire d is ident (single rows anyway): not looked at
    assert m.witness_keeps_groups(cols)


# ---------------------------------------------------------------- the circuits the suite had
def test_merkle_circuit_groups():
    """merkle_circuit(4): a, b, d mostly in groups of 3 rows, c ident; both
    grouped paths are taken."""
    import merkle_circuit as mc
    cp, _ = mc.merkle_circuit(4, seed=11)
    inp = cp.build()
    m = model_of(inp)
    assert sigma_of(inp) == inp._sig
    assert m.ident == [False, False, True, False, False]
    for j in (0, 1, 3):
        sizes = Counter(len(r) for r in m.groups[j] if r[0] < inp.n_gates)
        assert sizes.most_common(1)[0][0] == 3 and 4 * m.g[j] < 3 * inp.n
    assert m.wires_ok and m.z_ok
    assert m.witness_keeps_groups(witness_columns(inp))
    c = m.counters()
    assert (c["wire_groups_used"], c["z_groups_used"]) == (1, 1)
    # the one z run over the padding rows
    assert m.groups[4][-1][-(inp.n - inp.n_gates):] == list(range(inp.n_gates, inp.n))


def test_synthetic_inputs_have_no_groups():
    """pnp_testlib.Inputs: a <-> b 2-cycles only — every wire all single rows,
    every gate row moved: nothing is grouped."""
    from pnp_testlib import Inputs
    inp = Inputs(6, 3)
    m = model_of(inp)
    assert sorted(Counter(len(c) for c in m.cycles).items()) == [(1, 4 * 64 - 2 * inp.n_gates), (2, inp.n_gates)]
    assert m.g == [64, 64, 64, 64, inp.n_gates + 1]
    assert m.ident == [True] * 5 and not m.wires_ok and not m.z_ok
    assert all(v == 0 for k, v in m.counters().items() if "found" not in k)


# ---------------------------------------------------------------- the cases of test_gpu_groups.py
def test_case_a_every_start_offset_and_piece_shape():
    case = gc.case_a()
    m = case.model
    sizes = case.facts["sizes"]
    assert (case.n, len(case.cp.rows)) == (2048, 2045)
    runs = m.runs[0][:len(sizes)]
    assert [b - a for a, b in runs] == sizes  # the groups come in the order they were made
    assert {a % 32 for a, _ in runs} == set(range(32))
    assert set(range(1, 41)) | {31, 32, 33, 63, 64, 65} <= set(sizes)
    assert {1, 2, 3} == set(m.pieces[0])
    # scattered rows: hardly a group of consecutive rows
    multi = [r for r in m.groups[0] if len(r) > 2]
    assert sum(1 for r in multi if r[-1] - r[0] == len(r) - 1) == 0
    assert m.g[0] == len(sizes) + 3 and m.ident == [False, True, True, True, True]
    assert m.wires_ok and not m.z_ok
    vals = [case.cp.vals[case.cp.rows[r[0]][1][0]] for r in m.groups[0][:len(sizes)]]
    assert 0 not in vals and len(set(vals)) == len(vals)


def test_case_b_heavy_groups_in_a_wire():
    case = gc.case_b()
    m = case.model
    assert case.n == 1 << 15
    big = [(r, p) for r, p in zip(m.runs[0], m.pieces[0]) if p > 1]
    assert big == [((31, 8193), 257), ((8193, 16380), 256), ((16380, 25931), 300)]
    assert all(a % 32 for (a, _), _ in big)  # each starts mid-chunk
    assert m.heavy_queued == [2, 0, 0, 0, 0] and HEAVY == 256
    assert 257 + 256 + 300 > (1 << 14) // 32 + 2  # (why not 2^14: more pieces than its wire has)
    # scattered: each run's rows span the gates
    for rows, (a, b) in zip(case.facts["run_rows"], gc.B_RUNS):
        assert len(rows) == b - a and rows[-1] - rows[0] > 20000
        assert len({case.cp.rows[i][1][0] for i in rows}) == 1
    assert m.ident == [False, True, True, True, False] and m.wires_ok and m.z_ok
    # wire c: ident, with one real group
    assert [r for r in m.groups[2] if len(r) > 1] == [list(case.facts["c_rows"])]
    # what (g) changes: the heavy run's last sorted row; a row 256-row blocks away from its representative
    g1, g2 = m.groups[0][31], m.groups[0][32]
    assert g1 == case.facts["run_rows"][0] and g2 == case.facts["run_rows"][1]
    assert g2[0] // 256 != g2[len(g2) // 2] // 256


@pytest.mark.parametrize("kind,last_run,np_,heavy", [("boundary", (8193, 16384), 256, 0),
                                                     ("heavy", (8161, 16384), 257, 1),
                                                     ("middle", (12001, 16384), 137, 1)])
def test_case_c_z_runs(kind, last_run, np_, heavy):
    case = gc.case_c(kind)
    m = case.model
    assert case.n == 1 << 14
    assert m.runs[4][-1] == last_run and m.pieces[4][-1] == np_
    assert m.heavy_queued == [0, 0, 0, 0, heavy]
    assert m.g[:4] == [case.n] * 4 and not m.wires_ok and m.z_ok
    if kind == "boundary":
        assert len(case.cp.rows) == case.n // 2 + 1 and m.g[4] == case.n // 2 + 2  # every gate row moved
    if kind == "middle":
        assert m.runs[4][0] == (0, 101)
        mid = [(r, p) for r, p in zip(m.runs[4], m.pieces[4]) if p > HEAVY]
        assert mid == [((2000, 10501), 267)] and 2000 % 32


@pytest.mark.parametrize("shuffled", [True, False])
def test_case_d_one_cycle(shuffled):
    case = gc.case_d(shuffled)
    m = case.model
    n = case.n
    assert n == 1024 and max(map(len, m.cycles)) == 4 * (n - 3)
    assert m.g == [4, 4, 4, 4, n - 2]
    assert all(m.groups[j][0] == list(range(n - 3)) for j in range(4))
    assert m.wires_ok and not m.z_ok
    # 2^11 < 4 (n - 3): the label reaches every position only in the last of the log2(4n) rounds
    assert 1 << 11 < 4 * (n - 3) <= 1 << 12
    other = gc.case_d(not shuffled).model
    assert other.next != m.next and other.groups == m.groups


def test_case_e_cycles_across_wires():
    case = gc.case_e()
    m = case.model
    assert case.n == 1024 and case.cycle_seed is not None
    assert m.ident == [True, True, False, True, False] and m.g[2] == 1024 - 500
    assert m.wires_ok and m.z_ok
    # wire c's groups follow wire a's rows, not their own
    heads = [r[0] for r in m.groups[2][:250]]
    assert all(len(r) == 3 for r in m.groups[2][:250])
    assert heads != sorted(heads)
    a_row = {tuple(sorted(c)): a[0] for c, a in zip(case.facts["c_rows"], case.facts["a_rows"])}
    order = [a_row[tuple(r)] for r in m.groups[2][:250]]
    assert order == sorted(order)
    assert case.facts["twice"] == 50
    # the same circuit in slot order (the roads that derive sigma from the wire map)
    plain = gc.case_e(False)
    assert plain.cycle_seed is None and plain.model.groups == m.groups and plain.model.next != m.next


def test_case_f_thresholds():
    n = gc.F_N
    m = gc.case_f("mixed").model
    assert m.g[:4] == [767, 921, 922, 1024]
    assert 4 * 767 < 3 * n <= 4 * 768 and 10 * 921 <= 9 * n < 10 * 922
    assert m.ident[:4] == [False, False, True, True] and m.wires_ok
    assert any(len(r) > 1 for r in m.groups[2])  # the ident wire has real groups
    m = gc.case_f("z_alone").model
    assert m.g == [768, 1024, 1024, 1024, 921] and min(m.g[:4]) >= 768
    assert n - m.g[4] >= 103 and not m.wires_ok and m.z_ok
    case = gc.case_f("wires_alone")
    m = case.model
    assert len(case.cp.rows) == n - 3 and m.g[4] == n - 2 and n - m.g[4] < 103
    assert m.wires_ok and not m.z_ok and m.g[0] == 340 + 3


def test_case_h_one_constraint_removed():
    P, Q = gc.case_h(False), gc.case_h(True)
    p, q = P.model, Q.model
    assert (P.n, len(P.cp.rows)) == (Q.n, len(Q.cp.rows)) == (1024, 1021)
    assert q.g[0] == p.g[0] + 1 and q.g[1:] == p.g[1:]
    assert list(gc.H_ROWS) in p.groups[0]
    assert list(gc.H_ROWS[:3]) in q.groups[0] and list(gc.H_ROWS[3:]) in q.groups[0]
    assert p.wires_ok and q.wires_ok
    # Q's witness under P's (stale) groups: the two halves differ
    cols = [[Q.cp.vals[r[1][j]] for r in Q.cp.rows] + [0] * 3 for j in range(4)]
    assert q.witness_keeps_groups(cols) and not p.witness_keeps_groups(cols)
