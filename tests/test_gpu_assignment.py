"""Proving from a variable assignment over the resident wire map on the MI355X:
pnp_gather_witness (csrc/assignment.hip) against the numpy reference of
tests/test_assignment_ref.py, and pnp_prove_assignment end to end after
pnp_preprocess and after pnp_load_prover_key_coeffs + pnp_load_wire_map: the
proof is byte for byte the oracle's, and the one pnp_prove_ex returns for the
columns on the same context.  Every comparison is integers or bytes.

The gather runs one lane a row, 256 rows a workgroup, over the D rows of the
domain."""
import ctypes as C
import functools

import numpy as np
import pytest

from pnp import abi
from pnp_testlib import oracle, ptr_of, rand_fr_mont_arr, vp
from test_assignment_ref import assignment_ref, assignment_values
from test_general import make_circuit, pis_of
from test_gpu_preprocess import Desc, _case_b, dev_u32
from test_preprocess_ref import next_ref, wire_map

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A5A5A5A5A


# ------------------------------------------------------------------ pnp_gather_witness
def run_gather(var, values, lg):
    """The four (D, 4) u64 columns pnp_gather_witness writes over pre-filled buffers."""
    import pnp
    import torch
    from gpu_util import from_dev, to_dev
    D = 1 << lg
    ctx = pnp.Context(0)
    try:
        dv = [dev_u32(var[j]) for j in range(4)]
        dvals = to_dev(values)
        w = [torch.full((D, 4), PATTERN, dtype=torch.int64, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        ctx.gather_witness([t.data_ptr() for t in dv], var.shape[1], dvals.data_ptr(), values.shape[0], lg,
                           [t.data_ptr() for t in w])
        ctx.sync()
        return [from_dev(t) for t in w]
    finally:
        ctx.close()


def check_gather(var, n_vars, lg, seed):
    values = rand_fr_mont_arr(np.random.default_rng(seed), n_vars)
    got = run_gather(var, values, lg)
    exp = assignment_ref(values, var, 1 << lg)
    ng = var.shape[1]
    for j in range(4):
        assert not got[j][ng:].any(), j  # the padding rows are exactly zero
        assert np.array_equal(got[j], exp[j]), j


@pytest.mark.parametrize("n_gates", [1, 16])
def test_gather_one_row_and_no_padding_rows(n_gates):
    rng = np.random.default_rng(n_gates)
    var = rng.integers(0, 5, size=(4, n_gates)).astype(np.uint32)
    check_gather(var, 5, 4, seed=n_gates)


def test_gather_random_ids_and_one_variable_rows():
    var, _ = _case_b()  # 1000 rows over 300 variables, rows whose four wires are one variable
    assert var.shape == (4, 1000) and (var[:, 500] == 299).all()
    check_gather(var, 300, 10, seed=3)


def test_gather_many_workgroups_ragged_tail_ids_far_apart():
    rng = np.random.default_rng(17)
    ng, n_vars = (1 << 17) - 3, 3 << 16
    var = rng.integers(0, n_vars, size=(4, ng)).astype(np.uint32)
    assert ng % 256 and int(var.max()) > n_vars - 64
    check_gather(var, n_vars, 17, seed=5)


def test_gather_argument_errors():
    import pnp
    from gpu_util import empty_dev
    ctx = pnp.Context(0)
    try:
        dv = [dev_u32(np.zeros(16, dtype=np.uint32)) for _ in range(4)]
        vals, w = empty_dev(4), [empty_dev(16) for _ in range(4)]
        V, W = [t.data_ptr() for t in dv], [t.data_ptr() for t in w]
        for args in ((V, 0, vals.data_ptr(), 4, 4, W), (V, 17, vals.data_ptr(), 4, 4, W),
                     (V, 16, vals.data_ptr(), 4, 26, W), (V, 16, 0, 4, 4, W), (V, 16, vals.data_ptr(), 4, 4, W[:3] + [0]),
                     ([0] + V[1:], 16, vals.data_ptr(), 4, 4, W)):
            with pytest.raises(pnp.PnpError, match="PNP_E_ARG"):
                ctx.gather_witness(*args)
    finally:
        ctx.close()


# ------------------------------------------------------------------ pnp_prove_assignment
@functools.lru_cache(maxsize=None)
def inst(kind):
    """(composer, instance, oracle proof bytes, wire map, values), made once, never mutated."""
    import merkle_circuit as mc
    if kind == "all":
        cp = make_circuit("all")
    elif kind == "no_table":
        cp = make_circuit("arith_qm_pis")
    else:
        cp = mc.merkle_circuit(int(kind[len("merkle"):]), seed=11)[0]
    inp = cp.build()
    return cp, inp, abi.proof_to_bytes(inp.oracle_proof()), wire_map(cp), assignment_values(cp)


@functools.lru_cache(maxsize=None)
def other_witness(kind, seed=23):
    """Another seed of a merkle circuit: the same wire map and key, other
    values; its oracle proof under the FIRST instance's keys (each instance
    draws its own SRS)."""
    import merkle_circuit as mc
    cp, inp, _, var, _ = inst(kind)
    cp2 = mc.merkle_circuit(int(kind[len("merkle"):]), seed=seed)[0]
    inp2 = cp2.build()
    assert np.array_equal(wire_map(cp2), var) and len(cp2.vals) == len(cp.vals)
    assert all(a[0] == b[0] for a, b in zip(cp.rows, cp2.rows))  # the same selectors: the same key
    lib = oracle()
    out = abi.ProofC()
    pos, vals = inp2.pi_args()
    lib.or_gen_proof_ex.argtypes = [C.c_void_p] * 3 + [C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p]
    lib.or_gen_proof_ex.restype = C.c_int
    rc = lib.or_gen_proof_ex(C.byref(inp2.circuit), C.byref(inp.pk), C.byref(inp.ck), len(pos), vp(pos), vp(vals),
                             b"Merkle tree", C.byref(out))
    assert rc == 0
    exp2 = abi.proof_to_bytes(out)
    assert exp2 != inst(kind)[2]
    return inp2, exp2, assignment_values(cp2)


def prove_asg(ctx, values, device, pis):
    """(proof bytes, stage list) of pnp_prove_assignment from host or HBM values."""
    from gpu_util import to_dev
    if device:
        t = to_dev(values)
        got = ctx.prove_assignment(t.data_ptr(), values.shape[0], True, pis)
    else:
        got = ctx.prove_assignment(values.ctypes.data, values.shape[0], False, pis)
    return abi.proof_to_bytes(got), dict(ctx.stage_times())


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", ["all", "merkle4", "merkle6", "no_table"])
def test_preprocess_then_prove_assignment(kind, device):
    """all: every gate family, two public inputs, an 11-row table, q_lookup
    rows derived from the key; merkle4: 1,356 rows, D = 2048; merkle6: 5,988
    rows, D = 8192 (several workgroups); no_table: no lookup at all."""
    import pnp
    cp, inp, exp, var, values = inst(kind)
    if kind == "all":
        assert len(inp.pis) == 2 and inp.lookup_len == 11 and "q_lookup" in inp.nonzero
    if kind == "merkle6":
        assert (inp.n_gates, inp.n) == (5988, 8192)
    if kind == "no_table":
        assert inp.lookup_len == 0
    n_vars = len(cp.vals)
    ctx = pnp.Context(0)
    try:
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
        desc = Desc(cp, inp)
        ctx.preprocess(desc.d, device_ptrs=False)
        got, stages = prove_asg(ctx, values, device, pis_of(inp))
        assert got == exp
        assert stages["inputs_h2d_bytes"] == (0 if device else 32 * n_vars)
        # the columns on the same context: the same bytes, and its stage list as before
        cols = ctx.prove_ex(inp.circuit, False, pis_of(inp))
        assert abi.proof_to_bytes(cols) == exp
        assert "inputs_h2d_bytes" not in dict(ctx.stage_times())
        if kind == "merkle4":  # other values through the same resident map
            inp2, exp2, values2 = other_witness(kind)
            got2, _ = prove_asg(ctx, values2, device, pis_of(inp2))
            assert got2 == exp2
            assert abi.proof_to_bytes(ctx.prove_ex(inp2.circuit, False, pis_of(inp2))) == exp2
    finally:
        ctx.close()


def coeff_pk(inp):
    """The coefficient-only ProverKeyC of a GeneralInputs instance: the tables,
    the mandatory coefficient arrays, and the optional selectors it has."""
    from circuits import _ALWAYS
    pk = abi.ProverKeyC()
    for f in abi.PK_FIELDS:
        if f.endswith("_coeffs"):
            name = f[:-len("_coeffs")]
            if name in _ALWAYS or name in inp.nonzero:
                assert inp.arrays[f].shape == (inp.n, 4)
                setattr(pk, f, ptr_of(inp.arrays[f]))
        elif f.startswith("table"):
            setattr(pk, f, ptr_of(inp.arrays[f]))
    return pk


def host_cols(var):
    keep = [np.ascontiguousarray(var[j], dtype=np.uint32) for j in range(4)]
    return keep, [a.ctypes.data for a in keep]


def load_coeff_key(ctx, inp):
    ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
    ctx.load_prover_key_coeffs(coeff_pk(inp), inp.n, device_ptrs=False)


@pytest.mark.parametrize("device_map", [False, True], ids=["host_map", "device_map"])
def test_load_wire_map_then_prove_assignment(device_map):
    import pnp
    cp, inp, exp, var, values = inst("all")
    ctx = pnp.Context(0)
    try:
        load_coeff_key(ctx, inp)
        if device_map:
            keep = [dev_u32(var[j]) for j in range(4)]
            addrs = [t.data_ptr() for t in keep]
        else:
            keep, addrs = host_cols(var)
        ctx.load_wire_map(addrs, var.shape[1], len(cp.vals), device_ptrs=device_map)
        got, stages = prove_asg(ctx, values, False, pis_of(inp))
        assert got == exp
        assert stages["inputs_h2d_bytes"] == 32 * len(cp.vals)
    finally:
        ctx.close()


def first_sigma_diff(var_a, var_b, D):
    """(wire, row) of the first slot, in (row, wire) order, whose successor
    differs; None when the permutations are equal (the maps differ by a
    renaming of variables: two variables that occur nowhere else)."""
    a, b = next_ref(var_a, D), next_ref(var_b, D)
    pos = np.nonzero(a != b)[0]
    if not pos.size:
        return None
    slot = int((4 * (pos % D) + pos // D).min())
    return slot & 3, slot >> 2


def test_refusals_leave_the_context_proving():
    import pnp
    cp, inp, exp, var, values = inst("all")
    ng, n_vars, pis = var.shape[1], len(cp.vals), pis_of(inp)
    keep, good = host_cols(var)
    ctx = pnp.Context(0)
    try:
        # no key at all
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.load_wire_map(good, ng, n_vars, device_ptrs=False)
        load_coeff_key(ctx, inp)

        def still_proves():
            assert abi.proof_to_bytes(ctx.prove_ex(inp.circuit, False, pis)) == exp

        def no_map():
            with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY.*no wire map"):
                ctx.prove_assignment(values.ctypes.data, n_vars, False, pis)
        # before any map
        no_map()
        still_proves()
        # one id equal to n_vars
        bad = var.copy()
        bad[2, 5] = n_vars
        k2, addrs = host_cols(bad)
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG.*wire 2 of row 5"):
            ctx.load_wire_map(addrs, ng, n_vars, device_ptrs=False)
        no_map()
        still_proves()
        # two ids of different variables swapped in one row, over a good resident map
        ctx.load_wire_map(good, ng, n_vars, device_ptrs=False)
        for row in range(ng):
            bad = var.copy()
            bad[0, row], bad[1, row] = var[1, row], var[0, row]
            if var[0, row] != var[1, row] and first_sigma_diff(var, bad, inp.n):
                break
        wire, r = first_sigma_diff(var, bad, inp.n)
        assert r <= row
        k3, addrs = host_cols(bad)
        with pytest.raises(pnp.PnpError, match=f"PNP_E_ARG.*sigma.*wire {wire} of row {r}$"):
            ctx.load_wire_map(addrs, ng, n_vars, device_ptrs=False)
        no_map()  # no map is left resident, the earlier one included
        still_proves()
        # n_vars off by one
        ctx.load_wire_map(good, ng, n_vars, device_ptrs=False)
        longer = np.concatenate([values, values[:1]])
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG"):
            ctx.prove_assignment(longer.ctypes.data, n_vars + 1, False, pis)
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG"):
            ctx.prove_assignment(values.ctypes.data, n_vars - 1, False, pis)
        still_proves()
        assert prove_asg(ctx, values, False, pis)[0] == exp
        # a key load after a preprocess drops the map
        desc = Desc(cp, inp)  # (it owns the arrays its struct points to)
        ctx.preprocess(desc.d, device_ptrs=False)
        assert prove_asg(ctx, values, True, pis)[0] == exp
        ctx.load_prover_key_coeffs(coeff_pk(inp), inp.n, device_ptrs=False)
        no_map()
        still_proves()
    finally:
        ctx.close()


def test_load_wire_map_refuses_a_sharded_context():
    import pnp
    import torch
    from pnp.shard import SoloExchange, a2a_bytes_for, v_bytes_for
    cp, inp, _, var, _ = inst("all")
    ctx = pnp.Context(0)
    try:
        load_coeff_key(ctx, inp)
        solo = SoloExchange(1, 2, device=torch.device("cuda", 0), a2a_bytes=a2a_bytes_for(inp.lg_n, 2),
                            v_bytes=v_bytes_for(inp.lg_n, 2))
        ctx.set_msm_shard(solo)
        keep, addrs = host_cols(var)
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG.*ranks"):
            ctx.load_wire_map(addrs, var.shape[1], len(cp.vals), device_ptrs=False)
    finally:
        ctx.close()


def test_hbm_usage_counts_the_resident_map():
    import pnp
    cp, inp, _, var, _ = inst("merkle4")
    ng = var.shape[1]
    ctx = pnp.Context(0)
    try:
        base = ctx.hbm_usage()["live"]  # (nothing of this context yet)
        load_coeff_key(ctx, inp)
        before = ctx.hbm_usage()["live"]
        keep, addrs = host_cols(var)
        ctx.load_wire_map(addrs, ng, len(cp.vals), device_ptrs=False)
        after = ctx.hbm_usage()["live"]
        assert after - before >= 16 * ng
        assert after - before < 16 * ng + 4096  # (the scratch was released; q_lookup is zero here)
    finally:
        ctx.close()
    out = (C.c_uint64 * 6)()
    assert pnp.load().pnp_hbm_usage(None, out) == 0
    assert out[0] == base
