"""The reference the GPU gather (pnp_gather_witness / pnp_prove_assignment,
csrc/assignment.hip) is tested against, pinned on the CPU.

A composer holds one value per variable (Composer.vals, dense ids) and the
wire map var[j][i]; the witness columns the prover is handed are
vals[var[j]] (prover.rs:197-216), zero from row n_gates on.  assignment_ref
is that, as numpy indexing over Montgomery limbs; here it is checked against
the columns the GeneralInputs instances of the suite carry (every oracle proof
is made from them).  The q_lookup rows an assignment proof reads are the
forward transform of the key's q_lookup coefficients: checked to be the
q_lookup column of the instance, zero-padded.  And the ctypes argument lists
of the three new entry points."""
import ctypes as C

import numpy as np
import pytest

from pnp import abi
from pnp_testlib import fr_mont, ints_to_arr, oracle, vp
from test_preprocess_ref import wire_map

WIRES = ("w_l", "w_r", "w_o", "w_4")


def assignment_values(cp) -> np.ndarray:
    """(n_vars, 4) u64: the composer's values in Montgomery form, by variable id."""
    return ints_to_arr([fr_mont(v) for v in cp.vals])


def assignment_ref(values: np.ndarray, var: np.ndarray, D: int):
    """The four padded witness columns ((D, 4) u64 each) of values over var."""
    var = np.asarray(var)
    out = []
    for j in range(4):
        col = np.zeros((D, 4), dtype=np.uint64)
        col[:var.shape[1]] = values[var[j].astype(np.int64)]
        out.append(col)
    return out


def _circuits():
    from test_general import make_circuit
    import merkle_circuit as mc
    yield "all", make_circuit("all")
    yield "merkle4", mc.merkle_circuit(4, seed=4)[0]


@pytest.mark.parametrize("name,cp", list(_circuits()), ids=["all", "merkle4"])
def test_assignment_ref_equals_instance_columns(name, cp):
    inp = cp.build()
    var = wire_map(cp)
    ng = inp.n_gates
    assert var.shape == (4, ng) and int(var.max()) < len(cp.vals)
    cols = assignment_ref(assignment_values(cp), var, inp.n)
    for j, w in enumerate(WIRES):
        assert np.array_equal(cols[j][:ng], inp.arrays[w]), w
        assert not cols[j][ng:].any()
    # every variable of the merkle circuit sits in about three state slots
    if name == "merkle4":
        assert (ng, inp.n) == (1356, 2048) and len(cp.vals) < 2 * ng


@pytest.mark.parametrize("name,cp", list(_circuits()), ids=["all", "merkle4"])
def test_q_lookup_rows_are_the_transform_of_the_key_coefficients(name, cp):
    inp = cp.build()
    rows = np.zeros((inp.n, 4), dtype=np.uint64)
    rows[:inp.n_gates] = inp.arrays["q_lookup"]
    if "q_lookup" in inp.nonzero:
        c = inp.arrays["q_lookup_coeffs"].copy()
        assert c.shape == (inp.n, 4)
        oracle().or_ntt(vp(c), inp.lg_n, 0, 0)
        assert np.array_equal(c, rows)
        assert name == "all" and rows.any()
    else:  # the zero polynomial: no coefficients, a zero column
        assert not rows.any()
        assert name == "merkle4"


def test_assignment_ctypes_signatures():
    sig = abi.ASSIGNMENT_ARGTYPES
    assert sorted(sig) == ["pnp_gather_witness", "pnp_load_wire_map", "pnp_prove_assignment"]
    ids4 = C.c_void_p * 4
    assert sig["pnp_load_wire_map"] == [C.c_void_p, ids4, C.c_uint64, C.c_uint64, C.c_int]
    assert sig["pnp_gather_witness"] == [C.c_void_p, ids4, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, ids4]
    assert sig["pnp_prove_assignment"] == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p,
                                           C.c_void_p, C.c_char_p, C.POINTER(abi.ProofC)]
    import pnp
    lib = pnp.load()
    for name, argtypes in sig.items():
        assert name in pnp.SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is C.c_int
    for meth in ("load_wire_map", "gather_witness", "prove_assignment"):
        assert callable(getattr(pnp.Context, meth))
