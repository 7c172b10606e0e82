"""Preprocessing on the MI355X: pnp_wire_sigma (the copy permutation from the
wire map, csrc/preprocess.hip) against the numpy reference of
tests/test_preprocess_ref.py, and pnp_preprocess end to end: a circuit given
as selector columns, wire map and tables is proved byte for byte like the
oracle proves the GeneralInputs key of the same circuit, and its verifier key
equals the oracle's.  Every comparison is integers or bytes.

The sort ranks TILE = 4096 slots (4 waves x 16 chunks of 64) a workgroup, one
workgroup a tile (the grid is the tile count: no grid pass holds less than
the input), 8 bits a pass over ceil(log2 n_vars) bits."""
import ctypes as C
import functools

import numpy as np
import pytest

from pnp import abi
from pnp_testlib import R_MOD, fr_mont, ints_to_arr, ptr_of, verify
from test_general import make_circuit, pis_of
from test_preprocess_ref import wire_map, next_ref, sigma_arrays

pytestmark = pytest.mark.gpu

TILE = 4096  # PNP_SIGMA_TILE (csrc/pnp_internal.h)


# ------------------------------------------------------------------ pnp_wire_sigma
def dev_u32(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def run_wire_sigma(var, n_vars, lg, sigma=True):
    """(next, [4 sigma arrays] or None) of pnp_wire_sigma for a (4, n_gates) id array."""
    import pnp
    import torch
    from gpu_util import empty_dev, from_dev
    D = 1 << lg
    ctx = pnp.Context(0)
    try:
        dv = [dev_u32(var[j]) for j in range(4)]
        nxt = torch.zeros(4 * D, dtype=torch.int32, device="cuda")
        sig = [empty_dev(D) for _ in range(4)] if sigma else None
        torch.cuda.synchronize()
        ctx.wire_sigma([t.data_ptr() for t in dv], var.shape[1], n_vars, lg, nxt.data_ptr(),
                       [t.data_ptr() for t in sig] if sigma else None)
        torch.cuda.synchronize()
        return nxt.cpu().numpy().view(np.uint32), [from_dev(t) for t in sig] if sigma else None
    finally:
        ctx.close()


@pytest.mark.parametrize("n_gates,n_vars", [(1, 5), (16, 5), (16, 1)])
def test_next_tiny_and_no_padding_rows(n_gates, n_vars):
    """One gate; n_gates = D = 16 (no padding rows); one variable only (no digit pass)."""
    rng = np.random.default_rng(n_gates)
    var = rng.integers(0, n_vars, size=(4, n_gates)).astype(np.uint32)
    got, _ = run_wire_sigma(var, n_vars, 4, sigma=False)
    assert np.array_equal(got, next_ref(var, 16))


@functools.lru_cache(maxsize=None)
def _case_b():
    rng = np.random.default_rng(10)
    var = rng.integers(0, 300, size=(4, 1000)).astype(np.uint32)
    for row, v in ((0, 7), (500, 299), (999, 0), (17, 7)):  # four wires, one variable
        var[:, row] = v
    return var, next_ref(var, 1024)


def test_next_random_ids_and_one_variable_rows():
    var, exp = _case_b()
    got, _ = run_wire_sigma(var, 300, 10, sigma=False)
    assert np.array_equal(got, exp)


def test_next_heavy_variable_sparse_ids_high_bit():
    """Half of all slots on one variable (the id with bit 31 set), the others
    sparse below n_vars = 2^31 + 5: four digit passes."""
    rng = np.random.default_rng(31)
    ng, n_vars = 3000, (1 << 31) + 5
    ids = rng.integers(0, n_vars, size=700, dtype=np.uint64).astype(np.uint32)
    ids[:3] = (0, (1 << 31) + 3, 0x00FF00FF)
    var = ids[rng.integers(0, ids.size, size=(4, ng))]
    heavy = rng.random((4, ng)) < 0.5
    var[heavy] = n_vars - 1
    assert var.max() == n_vars - 1
    got, _ = run_wire_sigma(var, n_vars, 12, sigma=False)
    assert np.array_equal(got, next_ref(var, 4096))


@functools.lru_cache(maxsize=None)
def _case_d():
    rng = np.random.default_rng(17)
    ng, n_vars = (1 << 17) - 3, 3 << 16
    var = rng.integers(0, n_vars, size=(4, ng)).astype(np.uint32)
    assert 4 * ng > 3 * TILE and (4 * ng) % TILE  # 127 full tiles and a ragged one
    return var, n_vars, next_ref(var, 1 << 17)


def test_next_many_tiles_ragged_tail_and_repeatable():
    var, n_vars, exp = _case_d()
    got, sig = run_wire_sigma(var, n_vars, 17)
    assert np.array_equal(got, exp)
    again, sig2 = run_wire_sigma(var, n_vars, 17)
    assert got.tobytes() == again.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(sig, sig2))


def test_sigma_columns_python_integers():
    var, exp = _case_b()
    got, sig = run_wire_sigma(var, 300, 10)
    assert np.array_equal(got, exp)
    for j, col in enumerate(sigma_arrays(exp, 10)):
        assert np.array_equal(sig[j], col), j


def test_single_sigma_column_without_next():
    import pnp
    from gpu_util import empty_dev, from_dev
    var, exp = _case_b()
    ctx = pnp.Context(0)
    try:
        dv = [dev_u32(var[j]) for j in range(4)]
        out = empty_dev(1024)
        ctx.wire_sigma([t.data_ptr() for t in dv], 1000, 300, 10, 0, [0, 0, out.data_ptr(), 0])
        assert np.array_equal(from_dev(out), sigma_arrays(exp, 10)[2])
    finally:
        ctx.close()


def test_sigma_columns_equal_synth_merkle():
    """merkle_circuit(4) (1,356 rows, D = 2048): the sigmas of its wire map are
    the columns pnp_synth_merkle writes for the same height."""
    import pnp
    import merkle_circuit as mc
    from gpu_util import to_dev, empty_dev, from_dev
    pc = mc.PoseidonConstants()
    cp, nodes = mc.merkle_circuit(4, seed=4, pc=pc)
    inp = cp.build()
    n, ng = inp.n, len(cp.rows)
    assert (n, ng) == (2048, 1356)
    ctx = pnp.Context(0)
    try:
        leaves = to_dev(ints_to_arr([fr_mont(v) for v in cp.leaves]))
        blind = to_dev(ints_to_arr([fr_mont(v) for v in cp.blind]))
        dnodes = empty_dev(len(nodes))
        w = [empty_dev(ng) for _ in range(4)]
        sel = [empty_dev(n) for _ in range(9)]
        ref = [empty_dev(n) for _ in range(4)]
        ctx.synth_merkle(4, mc.flat_constants(pc), leaves.data_ptr(), blind.data_ptr(), dnodes.data_ptr(),
                         [t.data_ptr() for t in w], [t.data_ptr() for t in sel], [t.data_ptr() for t in ref], n)
        ctx.sync()
        var = wire_map(cp)
        dv = [dev_u32(var[j]) for j in range(4)]
        sig = [empty_dev(n) for _ in range(4)]
        ctx.wire_sigma([t.data_ptr() for t in dv], ng, len(cp.vals), 11, 0, [t.data_ptr() for t in sig])
        for j in range(4):
            assert np.array_equal(from_dev(sig[j]), from_dev(ref[j])), j
    finally:
        ctx.close()


def test_wire_sigma_id_out_of_range():
    import pnp
    var, _ = _case_b()
    var = var.copy()
    var[1, 321] = 300
    with pytest.raises(pnp.PnpError, match="PNP_E_ARG.*wire 1 of row 321"):
        run_wire_sigma(var, 300, 10, sigma=False)


# ------------------------------------------------------------------ pnp_preprocess
class Desc:
    """abi.CircuitDesc of a built Composer circuit and the arrays behind it."""

    def __init__(self, cp, inp, device=False, zero_columns=()):
        self.keep = []
        rows = cp.rows
        assert len(rows) == inp.n_gates
        d = abi.CircuitDesc(n_gates=len(rows), n_vars=len(cp.vals), lookup_len=len(cp.table))
        var = wire_map(cp)
        for j in range(4):
            d.var[j] = self._u32(var[j], device)
        for k, name in enumerate(abi.DESC_SELECTORS):
            vals = [r[0].get(name, 0) % R_MOD for r in rows]
            if any(vals) or name in zero_columns:
                d.sel[k] = self._fr(ints_to_arr([fr_mont(v) for v in vals]), device)
        for j in range(4):
            if cp.table:
                d.table[j] = self._fr(ints_to_arr([fr_mont(row[j]) for row in cp.table]), device)
        self.d = d

    def _fr(self, arr, device):
        if device:
            from gpu_util import to_dev
            self.keep.append(to_dev(arr))
            return abi.ptr(self.keep[-1].data_ptr())
        self.keep.append(arr)
        return ptr_of(arr)

    def _u32(self, arr, device):
        if device:
            self.keep.append(dev_u32(arr))
            return C.cast(C.c_void_p(self.keep[-1].data_ptr()), abi.U32P)
        self.keep.append(np.ascontiguousarray(arr, dtype=np.uint32))
        return self.keep[-1].ctypes.data_as(abi.U32P)


def vk_words(vk: abi.VerifierKey) -> np.ndarray:
    return np.frombuffer(bytes(vk), dtype=np.uint64)


def preprocess_and_prove(cp, inp, device=False, want_vk=True, zero_columns=()):
    import pnp
    ctx = pnp.Context(0)
    try:
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
        desc = Desc(cp, inp, device, zero_columns)
        vk = ctx.preprocess(desc.d, device_ptrs=device, want_vk=want_vk)
        return ctx.prove_ex(inp.circuit, False, pis_of(inp)), vk
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _all_families():
    cp = make_circuit("all")
    inp = cp.build()
    assert len(inp.pis) == 2 and inp.lookup_len == 11
    return cp, inp, abi.proof_to_bytes(inp.oracle_proof()), inp.vk()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_preprocess_all_families_proof_and_verifier_key(device):
    """Every gate family, a lookup table, two public inputs.  (The oracle's
    verifier key of a GeneralInputs instance is its vk(): verifier_key over the
    coefficients it has, absent polynomials NULL, like pnp_testlib.inputs_vk
    for an Inputs instance.)"""
    cp, inp, exp, exp_vk = _all_families()
    got, vk = preprocess_and_prove(cp, inp, device)
    assert abi.proof_to_bytes(got) == exp
    words = vk_words(vk)
    assert words.shape == exp_vk.shape and np.array_equal(words, exp_vk)
    assert verify(words.copy(), got, pis_of(inp), inp.tau_mont[0])


def test_preprocess_merkle_and_zero_qm_column():
    """merkle_circuit(4): the proof is the oracle's; its all-zero q_m column
    passed as zeros gives the same key as NULL."""
    import merkle_circuit as mc
    cp, _ = mc.merkle_circuit(4, seed=11)
    inp = cp.build()
    exp = abi.proof_to_bytes(inp.oracle_proof())
    got, vk = preprocess_and_prove(cp, inp)
    assert abi.proof_to_bytes(got) == exp
    assert np.array_equal(vk_words(vk), inp.vk())
    got0, vk0 = preprocess_and_prove(cp, inp, zero_columns=("q_m",))
    assert abi.proof_to_bytes(got0) == exp
    assert bytes(vk0) == bytes(vk)


def test_preprocess_without_lookup_table():
    cp = make_circuit("arith_qm_pis")
    inp = cp.build()
    assert inp.lookup_len == 0
    got, vk = preprocess_and_prove(cp, inp)
    assert abi.proof_to_bytes(got) == abi.proof_to_bytes(inp.oracle_proof())
    assert np.array_equal(vk_words(vk), inp.vk())


def test_preprocess_table_longer_than_gates():
    from circuits import Composer
    cp = Composer(9)
    cp.lookup_table(40)
    for k in (0, 39, 39, 12):
        cp.lookup(k)
    cp.arith()
    inp = cp.build()
    assert inp.lookup_len == 40 > inp.n_gates and inp.n == 64
    got, vk = preprocess_and_prove(cp, inp)
    assert abi.proof_to_bytes(got) == abi.proof_to_bytes(inp.oracle_proof())
    assert np.array_equal(vk_words(vk), inp.vk())


def test_preprocess_errors_keep_the_resident_key():
    import pnp
    cp, inp, exp, _ = _all_families()
    big = make_circuit("all", seed=6)
    big_inp = big.build(min_lg=inp.lg_n + 1)
    assert big_inp.n > inp.n
    ctx = pnp.Context(0)
    try:
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
        good = Desc(cp, inp)
        ctx.preprocess(good.d, device_ptrs=False)

        def still_proves():
            assert abi.proof_to_bytes(ctx.prove_ex(inp.circuit, False, pis_of(inp))) == exp
        still_proves()
        # one id equal to n_vars
        bad = Desc(cp, inp)
        var2 = bad.keep[2].copy()
        var2[5] = bad.d.n_vars
        bad.d.var[2] = var2.ctypes.data_as(abi.U32P)
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG.*wire 2 of row 5"):
            ctx.preprocess(bad.d, device_ptrs=False)
        still_proves()
        # a NULL wire column
        bad = Desc(cp, inp)
        bad.d.var[2] = None
        with pytest.raises(pnp.PnpError, match=r"PNP_E_ARG.*var\[2\]"):
            ctx.preprocess(bad.d, device_ptrs=False)
        still_proves()
        # a NULL table column with table rows
        bad = Desc(cp, inp)
        bad.d.table[1] = None
        with pytest.raises(pnp.PnpError, match=r"PNP_E_ARG.*table\[1\]"):
            ctx.preprocess(bad.d, device_ptrs=False)
        still_proves()
        # a verifier key over a domain the commit key does not cover
        big_desc = Desc(big, big_inp)
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.preprocess(big_desc.d, device_ptrs=False, want_vk=True)
        still_proves()
    finally:
        ctx.close()
    # ... and with no commit key at all
    ctx = pnp.Context(0)
    try:
        with pytest.raises(pnp.PnpError, match="PNP_E_NOKEY"):
            ctx.preprocess(good.d, device_ptrs=False, want_vk=True)
    finally:
        ctx.close()


def test_preprocess_refuses_a_sharded_context():
    """One rank of two (pnp.shard.SoloExchange, as bench.py --solo):
    multi-rank preprocessing is not supported."""
    import pnp
    import torch
    from pnp.shard import SoloExchange, a2a_bytes_for, v_bytes_for
    cp, inp, _, _ = _all_families()
    ctx = pnp.Context(0)
    try:
        solo = SoloExchange(1, 2, device=torch.device("cuda", 0), a2a_bytes=a2a_bytes_for(inp.lg_n, 2),
                            v_bytes=v_bytes_for(inp.lg_n, 2))
        ctx.set_msm_shard(solo)
        desc = Desc(cp, inp)
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG.*ranks"):
            ctx.preprocess(desc.d, device_ptrs=False)
    finally:
        ctx.close()
