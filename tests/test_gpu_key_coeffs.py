"""pnp_load_prover_key_coeffs: the prover key loaded from its coefficient
arrays alone, the 8n evaluations derived on the GPU (lde_blocks per
polynomial, the coset constants from closed forms), and the v1 switch
PNP_V1_DERIVE that routes gen_proof's key loads through it.

pnp_testlib.Inputs builds its evaluations with or_coset_lde8 of its
coefficients, so the oracle's proof, which reads the full key, is the expected
proof of the compact key.  Every check compares bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

from pnp_testlib import Inputs, ptr_of
from pnp import abi

pytestmark = pytest.mark.gpu

OPTIONAL = ("q_m", "range_selector", "logic_selector", "fixed_group_add_selector",
            "variable_group_add_selector", "q_lookup")


def compact_pk(inp, extra=None, to_ptr=ptr_of):
    """inp.pk without what the coefficient load never reads: every *_evals,
    linear_evaluations and v_h_coset_8n NULL, the optional selectors'
    coefficients NULL unless the instance has them (or `extra` gives them)."""
    extra = extra or {}
    pk = abi.ProverKeyC()
    for f in abi.PK_FIELDS:
        if f.endswith("_evals") or f in ("linear_evaluations", "v_h_coset_8n"):
            continue  # NULL
        if f in extra:
            setattr(pk, f, to_ptr(extra[f]))
        elif f in inp.arrays:
            setattr(pk, f, to_ptr(inp.arrays[f]))
        else:
            assert f[:-len("_coeffs")] in OPTIONAL, f
    return pk


@functools.lru_cache(maxsize=None)
def inst(*args, **kw):
    """An instance and its oracle proof, made once and shared (never mutated)."""
    inp = Inputs(*args, **kw)
    return inp, abi.proof_to_bytes(inp.oracle_proof())


def prove_compact(inp, pk=None, device_ptrs=False):
    import pnp
    ctx = pnp.Context(0)
    try:
        ctx.load_prover_key_coeffs(pk if pk is not None else compact_pk(inp), inp.n, device_ptrs=device_ptrs)
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
        ctx.kernel_timing(True)
        got = abi.proof_to_bytes(ctx.prove(inp.circuit, device_ptrs=False))
        return got, ctx.kernel_bytes("quotient_all_blocks")
    finally:
        ctx.close()


@pytest.mark.parametrize("lg,seed,n_gates", [(5, 1, None), (8, 2, None), (11, 3, None), (14, 21, (1 << 14) - 1000)])
def test_coeff_key_proof_equals_oracle(lg, seed, n_gates):
    """Host pointers; lg 5 goes through k_ntt_small, 11 and 14 through the
    radix-4 tiles; satisfying circuits, the k_quotient29 class (x32 blocks)."""
    inp, exp = inst(lg, seed, n_gates=n_gates)
    got, all_blocks = prove_compact(inp)
    assert got == exp
    assert all_blocks == 0


def test_live_qm_qlookup_general_class():
    """Live q_m / q_lookup selectors and a lookup table: not the q29 class,
    every block (lin included) in the 2^256 form."""
    inp, exp = inst(8, 47, lookup_rows=17, qm_qlookup_evals=True)
    assert "q_m_coeffs" in inp.arrays and "q_lookup_coeffs" in inp.arrays
    got, _ = prove_compact(inp)
    assert got == exp


def test_unsatisfied_witness_all_blocks():
    inp, exp = inst(6, 4, satisfying=False)
    got, all_blocks = prove_compact(inp)
    assert got == exp
    assert all_blocks == 1


def test_all_zero_optional_selector_is_null():
    inp, exp = inst(8, 2)
    zeros = np.zeros((inp.n, 4), dtype=np.uint64)
    pk = compact_pk(inp, extra={"range_selector_coeffs": zeros, "q_lookup_coeffs": zeros})
    got, all_blocks = prove_compact(inp, pk)
    assert got == exp
    assert all_blocks == 0


def test_device_pointers():
    from gpu_util import to_dev
    inp, exp = inst(8, 2)
    keep = []

    def dev_ptr(arr):
        keep.append(to_dev(arr))
        return abi.ptr(keep[-1].data_ptr())

    pk = compact_pk(inp, to_ptr=dev_ptr)
    got, _ = prove_compact(inp, pk, device_ptrs=True)
    assert got == exp


def test_no_stale_state_between_full_and_coeff_loads():
    import pnp
    a, exp_a = inst(8, 2)
    b, exp_b = inst(6, 9)
    ctx = pnp.Context(0)
    try:
        for inp, exp, coeffs in ((a, exp_a, False), (b, exp_b, True), (a, exp_a, False)):
            if coeffs:
                ctx.load_prover_key_coeffs(compact_pk(inp), inp.n, device_ptrs=False)
            else:
                ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
            ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
            assert abi.proof_to_bytes(ctx.prove(inp.circuit, device_ptrs=False)) == exp
    finally:
        ctx.close()


def _live(lib):
    o = (C.c_uint64 * 6)()
    assert lib.pnp_hbm_usage(None, o) == 0
    return int(o[0])


@functools.lru_cache(maxsize=None)
def _merkle4():
    import merkle_circuit as mc
    cp, _ = mc.merkle_circuit(4, seed=11)
    inp = cp.build()
    return cp, inp, abi.proof_to_bytes(inp.oracle_proof())


def _general_compact(inp):
    """compact_pk of a circuits.GeneralInputs, whose arrays hold a one-element
    stand-in (the empty Rust Vec) for the coefficients of a zero polynomial."""
    pk = compact_pk(inp)
    for name in OPTIONAL:
        if name not in inp.nonzero:
            setattr(pk, name + "_coeffs", None)
    return pk


# What the context of test_no_stale_blocks_between_key_classes holds after its
# step 4 beyond a fresh context that did only step 4 (47,565,988 B against
# 21,086,228 B).  Read from the commit before the key loads moved into
# csrc/prover_key.cpp, not from this code: what the three earlier proofs left
# in the context and no key load releases.
STEP4_HELD_BEYOND_FRESH = 26_479_760


def test_no_stale_blocks_between_key_classes():
    """One context alternates a general-class key (the all-families circuit:
    lookups and the four custom selectors live, 2^256 blocks) and a
    Merkle-class key (merkle_circuit(4): k_quotient29, 2^261 blocks) through
    the three loads; a block that survived from the earlier key would give a
    wrong proof (a selector read that should be zero, the wrong quotient
    kernel).  Every proof is the oracle's, byte for byte.

    A leftover that changes no byte is HBM: after step 4 (the Merkle key by
    the full load) and before any proof with it, the context holds what a
    fresh context holds after the same load plus STEP4_HELD_BEYOND_FRESH, the
    figure the parent commit gives for this sequence."""
    import pnp
    from test_general import pis_of
    from test_gpu_preprocess import Desc, _all_families
    lib = pnp.load()
    lib.pnp_v1_context.restype = C.c_void_p
    v1 = lib.pnp_v1_context()
    if v1:  # (an earlier test's gen_proof may still be building its tables)
        assert lib.pnp_sync(C.c_void_p(v1)) == 0
    gcp, ginp, gexp, _ = _all_families()
    mcp, minp, mexp = _merkle4()
    assert ginp.n <= 1 << 11 and minp.n == 1 << 11
    assert {"q_lookup", "range_selector", "logic_selector", "fixed_group_add_selector",
            "variable_group_add_selector"} <= ginp.nonzero and not (set(OPTIONAL) & minp.nonzero)

    def load(ctx, how, cp, inp):
        if how == "full":
            ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
        elif how == "coeffs":
            ctx.load_prover_key_coeffs(_general_compact(inp), inp.n, device_ptrs=False)
        else:
            desc = Desc(cp, inp)  # (owns the arrays desc.d points to)
            ctx.preprocess(desc.d, device_ptrs=False)
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)

    steps = (("full", gcp, ginp, gexp), ("coeffs", mcp, minp, mexp), ("preprocess", gcp, ginp, gexp),
             ("full", mcp, minp, mexp), ("coeffs", gcp, ginp, gexp))
    base = _live(lib)
    ctx = pnp.Context(0)
    try:
        for k, (how, cp, inp, exp) in enumerate(steps):
            load(ctx, how, cp, inp)
            if k == 3:
                held = ctx.hbm_usage()["live"] - base
            assert abi.proof_to_bytes(ctx.prove_ex(inp.circuit, False, pis_of(inp))) == exp, (k, how)
    finally:
        ctx.close()
    base = _live(lib)
    ctx = pnp.Context(0)
    try:
        load(ctx, *steps[3][:3])
        fresh = ctx.hbm_usage()["live"] - base
    finally:
        ctx.close()
    print(f"held after step 4: {held} B, a fresh context after the same load: {fresh} B, beyond: {held - fresh} B")
    assert held - fresh == STEP4_HELD_BEYOND_FRESH


def test_hbm_no_natural_order_arrays_stay():
    """With host pointers the full load keeps the 15 natural-order 8n arrays
    it uploaded (9 selectors, 4 sigmas, linear_evaluations, v_h_coset_8n;
    prover_key.h ResidentKey owned) beside the blocks, and four 8n scratch arrays (tmp);
    the coefficient load keeps neither: the difference in held HBM is at least
    15 * 8 D * 32 bytes (a bound read off the code, not a measurement)."""
    import pnp
    lib = pnp.load()
    inp, exp = inst(10, 9, n_gates=1000, pi_pos=17)
    held = {}
    for mode in ("full", "coeffs"):
        base = _live(lib)
        ctx = pnp.Context(0)
        try:
            if mode == "full":
                ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
            else:
                ctx.load_prover_key_coeffs(compact_pk(inp), inp.n, device_ptrs=False)
            ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
            assert abi.proof_to_bytes(ctx.prove(inp.circuit, device_ptrs=False)) == exp
            ctx.sync()
            held[mode] = ctx.hbm_usage()["live"] - base
        finally:
            ctx.close()
    print(f"held after one proof at 2^10: full {held['full']} B, coefficients {held['coeffs']} B")
    assert held["full"] - held["coeffs"] >= 15 * 8 * inp.n * 32


@pytest.mark.parametrize("rank,world", [(1, 2), (3, 4)])
def test_rank_blocks_equal_full_load(rank, world):
    """One rank of a multi-GPU proof run alone (pnp.shard.SoloExchange, as
    bench.py --solo): only the rank's own coset blocks are derived.  A solo
    proof is no real proof; the one after the coefficient load equals the one
    after the full load on the same set-up."""
    import pnp
    import torch
    from pnp.shard import SoloExchange, a2a_bytes_for, v_bytes_for
    lg = 10
    inp, _ = inst(lg, 9, n_gates=1000, pi_pos=17)
    proofs = []
    for coeffs in (False, True):
        ctx = pnp.Context(0)
        try:
            solo = SoloExchange(rank, world, device=torch.device("cuda", 0), a2a_bytes=a2a_bytes_for(lg, world),
                                v_bytes=v_bytes_for(lg, world))
            ctx.set_msm_shard(solo)
            if coeffs:
                ctx.load_prover_key_coeffs(compact_pk(inp), inp.n, device_ptrs=False)
            else:
                ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
            ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
            proofs.append(abi.proof_to_bytes(ctx.prove(inp.circuit, device_ptrs=False)))
        finally:
            ctx.close()
    assert proofs[0] == proofs[1]


def test_null_required_field_keeps_previous_key():
    import pnp
    inp, exp = inst(8, 2)
    ctx = pnp.Context(0)
    try:
        ctx.load_prover_key_coeffs(compact_pk(inp), inp.n, device_ptrs=False)
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
        assert abi.proof_to_bytes(ctx.prove(inp.circuit, device_ptrs=False)) == exp
        for field in ("q_c_coeffs", "out_sigma_coeffs", "table3"):
            bad = compact_pk(inp)
            setattr(bad, field, None)
            with pytest.raises(pnp.PnpError, match=f"PNP_E_ARG.*field {abi.PK_FIELDS.index(field)} "):
                ctx.load_prover_key_coeffs(bad, inp.n, device_ptrs=False)
        assert abi.proof_to_bytes(ctx.prove(inp.circuit, device_ptrs=False)) == exp
    finally:
        ctx.close()


def _v1_stages(lib):
    lib.pnp_v1_context.restype = C.c_void_p
    h = C.c_void_p(lib.pnp_v1_context())
    cap = 96
    ms = (C.c_double * cap)()
    names = (C.c_char_p * cap)()
    k = lib.pnp_last_stage_times(h, ms, names, cap)
    assert 0 < k <= cap
    return [names[i].decode() for i in range(k)]


def test_v1_derive_switch(monkeypatch):
    """PNP_V1_DERIVE=1: gen_proof loads a changed key through the coefficient
    path; a sampled element that disagrees with the derivation sends that load
    back to the full upload (the mutated key's proof); a disagreement in an
    unsampled element is not seen (the documented promise: the consistent
    key's proof); without the switch the caller's arrays are read again."""
    import pnp
    for name in ("PNP_V1_REUSE", "PNP_V1_RELOAD", "PNP_V1_DERIVE", "PNP_V1_NO_SPECULATE"):
        monkeypatch.delenv(name, raising=False)
    lib = pnp.load()
    other, exp_other = inst(5, 1)
    # another key first: whatever an earlier test left resident, the next call loads
    assert abi.proof_to_bytes(lib.gen_proof(other.circuit, other.pk, other.ck)) == exp_other
    inp = Inputs(10, 44, n_gates=1000, pi_pos=17)  # (mutated below: not shared)
    exp = abi.proof_to_bytes(inp.oracle_proof())
    qc = inp.arrays["q_c_evals"]
    assert (qc.size - 1) // 256 > 15  # element 3 (words 12..15) lies between two sampled words
    monkeypatch.setenv("PNP_V1_DERIVE", "1")
    assert abi.proof_to_bytes(lib.gen_proof(inp.circuit, inp.pk, inp.ck)) == exp
    names = _v1_stages(lib)
    assert "v1_derive_key" in names and "v1_zero_scan" in names and "v1_load_prover_key" in names
    assert "v1_derive_fallback" not in names
    # element 0 holds sampled word 0
    saved0 = qc[0].copy()
    qc[0] = qc[5]
    exp0 = abi.proof_to_bytes(inp.oracle_proof())
    assert exp0 != exp
    assert abi.proof_to_bytes(lib.gen_proof(inp.circuit, inp.pk, inp.ck)) == exp0
    names = _v1_stages(lib)
    assert "v1_derive_key" in names and "v1_derive_fallback" in names
    # element 3 is not sampled
    qc[0] = saved0
    qc[3] = qc[5]
    exp3 = abi.proof_to_bytes(inp.oracle_proof())
    assert exp3 != exp
    assert abi.proof_to_bytes(lib.gen_proof(inp.circuit, inp.pk, inp.ck)) == exp
    names = _v1_stages(lib)
    assert "v1_derive_key" in names and "v1_derive_fallback" not in names
    monkeypatch.delenv("PNP_V1_DERIVE")
    assert abi.proof_to_bytes(lib.gen_proof(inp.circuit, inp.pk, inp.ck)) == exp3
