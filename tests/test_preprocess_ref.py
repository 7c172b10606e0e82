"""The reference the GPU preprocessing (pnp_preprocess / pnp_wire_sigma,
csrc/preprocess.hip) is tested against, pinned on the CPU.

next_ref is the copy permutation of a wire map as compute_sigma_permutations
(plonk-core/src/permutation/mod.rs:101-213) defines it: the slots of one
variable in the order the composer registers them (gates in row order, a
gate's wires L, R, O, 4: slot = 4 row + wire) closed into a cycle; rows the
composer never registered map to themselves.  Here: a stable argsort of the
slots by variable id, next inside every run of equal ids, wrapping to the
run's head.  It is checked against the dict-of-cycles construction of
tests/circuits.py (GeneralInputs, the sigmas every oracle proof of the suite
is made with), and the ctypes mirrors of the two new ABI structs against the
C layout."""
import ctypes as C

import numpy as np

from circuits import K_COSET
from pnp import abi
from pnp_testlib import R_MOD, fr_root, fr_mont, ints_to_arr


def wire_map(cp) -> np.ndarray:
    """(4, n_gates) u32 variable ids of a Composer's rows: left, right, out, fourth."""
    return np.array([[r[1][j] for r in cp.rows] for j in range(4)], dtype=np.uint32)


def next_ref(var: np.ndarray, D: int) -> np.ndarray:
    """next[j D + i] = j' D + i' (u32, 4 D entries) for var[j][i], i < n_gates."""
    var = np.asarray(var)
    n_gates = var.shape[1]
    flat = var.T.reshape(-1).astype(np.uint64)  # slot = 4 row + wire
    m = flat.size
    order = np.argsort(flat, kind="stable")
    keys = flat[order]
    brk = keys[1:] != keys[:-1]
    head = np.ones(m, dtype=bool)
    head[1:] = brk
    tail = np.ones(m, dtype=bool)
    tail[:-1] = brk
    idx = np.arange(m)
    run_head = np.maximum.accumulate(np.where(head, idx, 0))
    nxt_pos = np.where(tail, run_head, np.minimum(idx + 1, m - 1))
    nxt_slot = np.empty(m, dtype=np.int64)
    nxt_slot[order] = order[nxt_pos]

    def pos(s):
        return (s & 3) * D + (s >> 2)
    out = np.arange(4 * D, dtype=np.uint32)
    out[pos(idx)] = pos(nxt_slot).astype(np.uint32)
    assert n_gates <= D
    return out


def sigma_ints(nxt: np.ndarray, lg: int):
    """The four sigma columns (canonical ints) of a next array: K_j' w^i'."""
    D = 1 << lg
    w = fr_root(lg)
    wp = [1] * D
    for i in range(1, D):
        wp[i] = wp[i - 1] * w % R_MOD
    return [[K_COSET[int(t) >> lg] * wp[int(t) & (D - 1)] % R_MOD for t in nxt[j * D:(j + 1) * D]]
            for j in range(4)]


def sigma_arrays(nxt: np.ndarray, lg: int):
    return [ints_to_arr([fr_mont(v) for v in col]) for col in sigma_ints(nxt, lg)]


def test_next_ref_hand_example():
    # rows (L, R, O, 4): variable 7 sits in slots 0, 5, 6; 3 in slots 1, 4; 9 alone; 0 in 3, 7
    var = np.array([[7, 3], [3, 7], [9, 7], [0, 0]], dtype=np.uint32)
    D = 4
    nxt = next_ref(var, D)
    exp = np.arange(16, dtype=np.uint32)
    # (wire, row) -> (wire, row): 7: (0,0)->(1,1)->(2,1)->(0,0); 3: (1,0)->(0,1)->(1,0); 0: (3,0)->(3,1)->(3,0)
    exp[0 * D + 0] = 1 * D + 1
    exp[1 * D + 1] = 2 * D + 1
    exp[2 * D + 1] = 0 * D + 0
    exp[1 * D + 0] = 0 * D + 1
    exp[0 * D + 1] = 1 * D + 0
    exp[3 * D + 0] = 3 * D + 1
    exp[3 * D + 1] = 3 * D + 0
    assert nxt.tolist() == exp.tolist()


def test_next_ref_equals_composer_cycles_all_families():
    from test_general import make_circuit
    cp = make_circuit("all")
    inp = cp.build()
    var = wire_map(cp)
    assert var.shape == (4, inp.n_gates) and inp.n_gates < inp.n
    nxt = next_ref(var, inp.n)
    assert sigma_ints(nxt, inp.lg_n) == inp._sig
    # padding rows are fixed, gate rows of a shared variable are not
    assert all(int(nxt[j * inp.n + i]) == j * inp.n + i for j in range(4) for i in range(inp.n_gates, inp.n))
    assert sorted(nxt.tolist()) == list(range(4 * inp.n))


def test_next_ref_equals_composer_cycles_merkle():
    import merkle_circuit as mc
    cp, _ = mc.merkle_circuit(3, seed=3)
    inp = cp.build()
    assert inp.n_gates == mc.merkle_rows(3)
    nxt = next_ref(wire_map(cp), inp.n)
    assert sigma_ints(nxt, inp.lg_n) == inp._sig


def test_new_struct_layouts():
    assert C.sizeof(abi.VerifierKey) == 8 + 96 + 23 * 96
    assert abi.VerifierKey.g.offset == 8 and abi.VerifierKey.polys.offset == 104
    assert len(abi.VK_POLYS) == 23 and len(abi.DESC_SELECTORS) == 15
    assert C.sizeof(abi.CircuitDesc) == 24 + 4 * 8 + 15 * 8 + 4 * 8
    assert (abi.CircuitDesc.var.offset, abi.CircuitDesc.sel.offset, abi.CircuitDesc.table.offset) == (24, 56, 176)
    # the same order as the oracle's verifier key
    from pnp_testlib import VK_POLYS, VK_WORDS
    assert abi.VK_POLYS == VK_POLYS and C.sizeof(abi.VerifierKey) == 8 * VK_WORDS
