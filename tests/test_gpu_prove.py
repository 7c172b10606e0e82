"""End-to-end parity: gen_proof on the MI355X vs the CPU restatement, byte for
byte on the 2656-byte ProofC, through both the v1 symbol (host inputs, exactly
as the Rust FFI calls it) and the v2 resident-key API."""
import pytest

from pnp_testlib import Inputs, inputs_pis, inputs_vk, verify
from pnp import abi

pytestmark = pytest.mark.gpu


def _diff(a, b):
    bad = []
    for name in abi.PROOF_COMMITMENTS:
        ca, cb = getattr(a, name), getattr(b, name)
        if list(ca.x) != list(cb.x) or list(ca.y) != list(cb.y):
            bad.append(name)
    ea, eb = a.evaluations, b.evaluations
    for grp in ("wire_evals", "perm_evals", "lookup_evals", "custom_evals"):
        ga, gb = getattr(ea, grp), getattr(eb, grp)
        for f, _ in ga._fields_:
            if list(getattr(ga, f)) != list(getattr(gb, f)):
                bad.append(f"{grp}.{f}")
    return bad


@pytest.mark.parametrize("lg,seed", [(5, 1), (8, 2), (11, 3)])
def test_gen_proof_v1_parity(lg, seed):
    import pnp
    inp = Inputs(lg, seed)
    exp = inp.oracle_proof()
    lib = pnp.load()
    got = lib.gen_proof(inp.circuit, inp.pk, inp.ck)
    assert _diff(got, exp) == []
    assert abi.proof_to_bytes(got) == abi.proof_to_bytes(exp)
    # and the GPU proof is accepted by the restated reference verifier
    assert verify(inputs_vk(inp), got, inputs_pis(inp), inp.tau_mont[0])


@pytest.mark.parametrize("lookup_rows,extra", [(0, True), (17, False), (40, True)])
def test_gen_proof_general_lookup_and_selectors(lookup_rows, extra):
    """Random (unsatisfied) inputs outside the lookup-trivial fast path:
    non-zero q_lookup witness rows whose wire tuples form the lookup table
    (f != 0, t != 0: combine_split, h1 / h2 committed, z2 a real grand
    product) and live q_m / q_lookup selectors (coefficients + evaluations)."""
    import pnp
    inp = Inputs(8, 30 + lookup_rows, lookup_rows=lookup_rows, qm_qlookup_evals=extra)
    exp = inp.oracle_proof()
    ctx = pnp.Context(0)
    ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
    ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
    ctx.kernel_timing(True)
    got = ctx.prove(inp.circuit, device_ptrs=False)
    assert _diff(got, exp) == []
    if lookup_rows:
        assert any(v != 0 for v in exp.f_comm.x)
        assert any(v != 0 for v in exp.h_1_comm.x)
    # random q_m / q_lookup evaluations leave the circuit unsatisfied: the
    # 6-block round 4 fails the identity at z and is redone on all 8 blocks
    if extra:
        assert ctx.kernel_bytes("quotient_all_blocks") == 1
    ctx.close()


@pytest.mark.parametrize("lg,seed", [(6, 4), (10, 5)])
def test_gen_proof_unsatisfied_witness_all_blocks(lg, seed):
    """Independent random witness / selectors / sigmas: the reference's t
    pieces t_7 / t_8 are non-zero, so only the 8-block round 4 reproduces
    them; the proof is still byte-identical to the oracle's."""
    import pnp
    inp = Inputs(lg, seed, satisfying=False)
    exp = inp.oracle_proof()
    assert any(v != 0 for v in exp.t_8_comm.x)
    ctx = pnp.Context(0)
    ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
    ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
    ctx.kernel_timing(True)
    got = ctx.prove(inp.circuit, device_ptrs=False)
    assert abi.proof_to_bytes(got) == abi.proof_to_bytes(exp)
    assert ctx.kernel_bytes("quotient_all_blocks") == 1
    ctx.close()


def test_gen_proof_v2_resident(tmp_path):
    import pnp
    inp = Inputs(10, 9, n_gates=1000, pi_pos=17)
    exp = inp.oracle_proof()
    ctx = pnp.Context(0)
    ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
    ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
    ctx.kernel_timing(True)
    for _ in range(2):  # resident keys are reused across proofs
        got = ctx.prove(inp.circuit, device_ptrs=False)
        assert abi.proof_to_bytes(got) == abi.proof_to_bytes(exp)
    names = [n for n, _ in ctx.stage_times()]
    assert "r4_quotient" in names
    # satisfying circuit: round 4 on 6 coset blocks, identity check passed
    assert ctx.kernel_bytes("quotient_all_blocks") == 0
    ctx.close()


_R45 = ["r4_lde", "r4_quotient", "r4_intt8", "r4_commit", "r5_evals"]


@pytest.mark.parametrize("satisfying", [True, False])
def test_stage_order(satisfying):
    """The exact ordered stage names of a resident-key proof (bench.py and the
    tools under tools/ read them): rounds 4 and 5 up to the identity check
    stand once for a satisfying witness and twice (6 blocks, then all 8) for
    an unsatisfied one; round 6 always stands once."""
    import pnp
    inp = Inputs(8, 12, satisfying=satisfying)
    exp = inp.oracle_proof()
    ctx = pnp.Context(0)
    ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
    ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
    ctx.kernel_timing(True)
    got = ctx.prove(inp.circuit, device_ptrs=False)
    assert abi.proof_to_bytes(got) == abi.proof_to_bytes(exp)
    assert ctx.kernel_bytes("quotient_all_blocks") == (0 if satisfying else 1)
    names = [n for n, _ in ctx.stage_times()]
    assert names == (["inputs", "r1_intt", "r1_commit", "r2_lookup", "r3_z", "r3_z2_pi"]
                     + _R45 * (1 if satisfying else 2) + ["r5_lin", "r6_witness", "r6_commit"])
    ctx.close()


@pytest.mark.parametrize("switch,value,satisfying,redo", [
    ("PNP_NO_OVERLAP", "1", True, None),
    ("PNP_QUOT29", "0", True, 0),
    ("PNP_QUOT_BLOCKS", "7", True, 0),
    ("PNP_QUOT_BLOCKS", "7", False, 1),   # the redo goes from 7 to 8 blocks
    ("PNP_QUOT_BLOCKS", "8", False, 0),   # all 8 blocks at once: no check, no redo
])
def test_prover_switches_same_proof(switch, value, satisfying, redo):
    """The operator switches that decide branches inside the prover
     leave the proof byte for byte the oracle's; redo = the
    expected quotient_all_blocks count.  Each case runs in a fresh child
    process: the switches are read once per process."""
    import os
    import subprocess
    import sys
    here = os_path_tests()
    code = (
        "import sys; sys.path[:0] = [%r, %r]\n"
        "from pnp import abi\n"
        "from pnp_testlib import Inputs\n"
        "import pnp\n"
        "inp = Inputs(8, 61, satisfying=%r)\n"
        "exp = inp.oracle_proof()\n"
        "ctx = pnp.Context(0)\n"
        "ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)\n"
        "ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)\n"
        "ctx.kernel_timing(True)\n"
        "got = ctx.prove(inp.circuit, device_ptrs=False)\n"
        "redo = ctx.kernel_bytes('quotient_all_blocks')\n"
        "ctx.close()\n"
        "assert abi.proof_to_bytes(got) == abi.proof_to_bytes(exp)\n"
        "print('SAME redo=%%d' %% redo)\n"
    ) % (here, os.path.join(os.path.dirname(here), "zprize23-gpu-submission_amd"), satisfying)
    env = dict(os.environ, **{switch: value})
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SAME" in r.stdout
    if redo is not None:
        assert "redo=%d" % redo in r.stdout


def test_synth_circuit_matches_cpu_generator():
    """pnp_synth_circuit (bench generator) == tests' satisfying_witness."""
    import numpy as np
    import pnp
    from gpu_util import to_dev, from_dev, empty_dev
    from pnp_testlib import (satisfying_witness, rand_fr_mont_arr, arr_to_ints, fr_unmont,
                             fr_mont, ints_to_arr)
    lg, ng, pos = 6, 50, 7
    n = 1 << lg
    rng = np.random.default_rng(11)
    names = ("q_l", "q_r", "q_o", "q_4", "q_c", "q_hl", "q_hr", "q_h4")
    sel_m = {k: rand_fr_mont_arr(rng, n) for k in names}
    for k in names:
        sel_m[k][ng:] = 0
    a_m, d_m = rand_fr_mont_arr(rng, ng), rand_fr_mont_arr(rng, ng)
    pi = [12345, 0, 0, 0]
    ctx = pnp.Context(0)
    w = [to_dev(a_m), empty_dev(ng), empty_dev(ng), to_dev(d_m)]
    sel = [to_dev(sel_m[k]) for k in names] + [empty_dev(n)]
    sig = [empty_dev(n) for _ in range(4)]
    ctx.synth_circuit([t.data_ptr() for t in w], [t.data_ptr() for t in sel],
                      [t.data_ptr() for t in sig], n, ng, pos, pi)
    un = lambda arr: [fr_unmont(v) for v in arr_to_ints(arr)]
    sel_c = {k: un(sel_m[k]) for k in names}
    sel_c["q_arith"] = [1] * ng + [0] * (n - ng)
    b, c, sg = satisfying_witness(sel_c, un(a_m) + [0] * (n - ng), un(d_m) + [0] * (n - ng),
                                  ng, pos, fr_mont(12345), lg)
    assert un(from_dev(w[1])) == b[:ng]
    assert un(from_dev(w[2])) == c[:ng]
    assert un(from_dev(sel[8])) == sel_c["q_arith"]
    for j in range(4):
        assert un(from_dev(sig[j])) == sg[j]
    ctx.close()


def test_gen_proof_parity_2e14():
    """Larger parity point: satisfying circuit at n = 2^14 (8n = 2^17 coset)."""
    import pnp
    inp = Inputs(14, 21, n_gates=(1 << 14) - 1000, pi_pos=99)
    exp = inp.oracle_proof()
    got = pnp.load().gen_proof(inp.circuit, inp.pk, inp.ck)
    assert _diff(got, exp) == []


@pytest.mark.parametrize("circuit", ["arith", "merkle"])
def test_full_size_height15_properties(circuit):
    """BASELINE config 4 size (3,161,924 gates, n = 2^22): properties that hold
    for any correct prover on a satisfying circuit: deg t < 6n so t_7 = t_8 =
    infinity while t_1..t_6 are not; h1 = h2 = f = infinity; z2 commits to
    [1, 0, ...] = G; proving is deterministic.  circuit = "merkle" is the
    reference's own HEIGHT=15 Poseidon Merkle circuit (pnp_synth_merkle): the
    round-5 check lin(z) = -r_0 (the verifier's equation) passing on the
    6-block quotient shows the generated witness satisfies every gate and copy
    constraint."""
    import os
    import sys
    import pnp
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import Synthetic, HEIGHT15_GATES
    ctx = pnp.Context(0)
    syn = Synthetic(ctx, 22, HEIGHT15_GATES, seed=5, circuit=circuit)
    assert syn.gates == HEIGHT15_GATES
    ctx.load_prover_key(syn.pk, syn.n, device_ptrs=True)
    ctx.load_commit_key(syn.ck, syn.n, device_ptrs=True)
    ctx.kernel_timing(True)
    p1 = ctx.prove(syn.cs, device_ptrs=True)
    p2 = ctx.prove(syn.cs, device_ptrs=True)
    assert abi.proof_to_bytes(p1) == abi.proof_to_bytes(p2)
    assert ctx.kernel_bytes("quotient_all_blocks") == 0  # the 6-block round 4
    inf = lambda c: all(v == 0 for v in c.x)
    assert inf(p1.t_7_comm) and inf(p1.t_8_comm)
    assert not any(inf(getattr(p1, f"t_{k}_comm")) for k in range(1, 7))
    assert inf(p1.h_1_comm) and inf(p1.h_2_comm) and inf(p1.f_comm)
    assert not inf(p1.a_comm) and not inf(p1.z_comm) and not inf(p1.aw_opening)
    # z2 = constant 1 polynomial -> commitment = powers_of_g[0] = G (tau^0 G)
    import torch
    g0 = syn.keep["srs"][0].cpu().numpy().view("uint64")
    assert list(p1.z_2_comm.x) == [int(v) for v in g0[:6]]
    assert list(p1.z_2_comm.y) == [int(v) for v in g0[6:]]
    ctx.close()


def test_v1_reloads_mutated_key(monkeypatch):
    """The v1 symbol keeps the reference's per-call key read (load.cu:311-358):
    a caller that rewrites its key buffers in place between two calls (same
    pointers, a change in words the reuse fingerprint does not sample) gets a
    proof over the NEW key, byte-identical to the oracle's — the default hashes
    every word the load reads and uploads only a changed key; an unchanged SRS
    keeps its folded table (device-side comparison) and the proof stays exact.
    With PNP_V1_REUSE=1 (opt-in: the caller promises immutable keys) the
    resident copy is reused and the second proof is the stale one."""
    import pnp
    monkeypatch.delenv("PNP_V1_REUSE", raising=False)
    lib = pnp.load()
    inp = Inputs(10, 44, n_gates=1000, pi_pos=17)
    first = lib.gen_proof(inp.circuit, inp.pk, inp.ck)
    assert abi.proof_to_bytes(first) == abi.proof_to_bytes(inp.oracle_proof())
    # element 3 of q_c's 8n evaluations: words 12..15, between the sampled
    # words 0 and (32n - 1) / 256 of the fingerprint
    qc = inp.arrays["q_c_evals"]
    assert (qc.size - 1) // 256 > 15
    saved = qc[3].copy()
    qc[3] = qc[5]
    exp = inp.oracle_proof()
    assert abi.proof_to_bytes(exp) != abi.proof_to_bytes(first)
    second = lib.gen_proof(inp.circuit, inp.pk, inp.ck)
    assert abi.proof_to_bytes(second) == abi.proof_to_bytes(exp)
    # the default compares the full-content hash of every array the load reads:
    # an unchanged key is not uploaded again (same proof), a changed word of a
    # zero selector's evaluations or of the SRS is seen
    # (with both keys resident the call proves on them while the hash runs and
    # proves again after the upload when the hash differs: the second call above
    # and the SRS change below take that path; PNP_V1_NO_SPECULATE hashes first)
    again = lib.gen_proof(inp.circuit, inp.pk, inp.ck)
    assert abi.proof_to_bytes(again) == abi.proof_to_bytes(exp)
    monkeypatch.setenv("PNP_V1_NO_SPECULATE", "1")
    assert abi.proof_to_bytes(lib.gen_proof(inp.circuit, inp.pk, inp.ck)) == abi.proof_to_bytes(exp)
    monkeypatch.delenv("PNP_V1_NO_SPECULATE")
    pts = inp.arrays["srs"]
    keep_pt = pts[7].copy()
    pts[7] = pts[9]  # a different curve point at index 7: every commitment moves
    exp_ck = inp.oracle_proof()
    assert abi.proof_to_bytes(lib.gen_proof(inp.circuit, inp.pk, inp.ck)) == abi.proof_to_bytes(exp_ck)
    pts[7] = keep_pt
    assert abi.proof_to_bytes(lib.gen_proof(inp.circuit, inp.pk, inp.ck)) == abi.proof_to_bytes(exp)
    # the opt-in reuse: a third call on a reverted key returns the resident
    # (mutated-key) proof, then a reload once the switch is off again
    qc[3] = saved
    monkeypatch.setenv("PNP_V1_REUSE", "1")
    lib.gen_proof(inp.circuit, inp.pk, inp.ck)          # loads (fingerprint unknown)
    qc[3] = qc[5]
    stale = lib.gen_proof(inp.circuit, inp.pk, inp.ck)  # same fingerprint: reused
    assert abi.proof_to_bytes(stale) == abi.proof_to_bytes(first)
    monkeypatch.delenv("PNP_V1_REUSE")
    fresh = lib.gen_proof(inp.circuit, inp.pk, inp.ck)
    assert abi.proof_to_bytes(fresh) == abi.proof_to_bytes(exp)


def test_v1_srs_change_rebuilds_table():
    """v1 with a different SRS in the SAME buffer: the device-side comparison
    sees the change and the folded MSM table is rebuilt (proof == oracle)."""
    import numpy as np
    import pnp
    from pnp_testlib import oracle, vp
    lib = pnp.load()
    inp = Inputs(9, 45)
    assert abi.proof_to_bytes(lib.gen_proof(inp.circuit, inp.pk, inp.ck)) == \
        abi.proof_to_bytes(inp.oracle_proof())
    tau2 = np.array([[7, 0, 0, 0]], dtype=np.uint64)
    oracle().or_srs(vp(inp.arrays["srs"]), inp.n, vp(tau2))   # new SRS written in place
    got = lib.gen_proof(inp.circuit, inp.pk, inp.ck)
    assert abi.proof_to_bytes(got) == abi.proof_to_bytes(inp.oracle_proof())


def test_v1_strict_envelope(monkeypatch, tmp_path):
    """PNP_V1_STRICT=1 refuses (print + exit, the v1 error contract) a key with
    live q_m / q_lookup selectors, where the reference GPU path and this
    backend return different proofs; a Merkle-class key proves normally."""
    import subprocess
    import sys
    import textwrap
    code = textwrap.dedent("""
        import os, sys
        sys.path.insert(0, %r)
        import conftest  # noqa: F401  (sys.path)
        import pnp
        from pnp import abi
        from pnp_testlib import Inputs
        inp = Inputs(8, 47, qm_qlookup_evals=(sys.argv[1] == "live"))
        p = pnp.load().gen_proof(inp.circuit, inp.pk, inp.ck)
        print("ok", abi.proof_to_bytes(p) == abi.proof_to_bytes(inp.oracle_proof()))
    """ % os_path_tests())
    env = dict(__import__("os").environ, PNP_V1_STRICT="1")
    ok = subprocess.run([sys.executable, "-c", code, "merkle"], env=env, capture_output=True, text=True,
                        timeout=300)
    assert ok.returncode == 0 and "ok True" in ok.stdout, ok.stderr[-2000:]
    bad = subprocess.run([sys.executable, "-c", code, "live"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert bad.returncode != 0 and "PNP_V1_STRICT" in bad.stderr, bad.stderr[-2000:]


def os_path_tests():
    import os
    return os.path.dirname(os.path.abspath(__file__))


# The rows of the v1 call's contract (csrc/v1.cpp, its header comment) that the
# tests above do not reach.  The call's state is per process, so each case is
# a script run in a fresh child: n = 2^8 (one domain change to 2^9), the oracle
# proof as the expected bytes.
_V1_CHILD = """
import ctypes as C, os, sys
sys.path[:0] = [%r, %r]
import pnp
from pnp import abi
from pnp_testlib import Inputs
lib = pnp.load()
def same(p, inp):
    return abi.proof_to_bytes(p) == abi.proof_to_bytes(inp.oracle_proof())
def v1_stages():
    ms, names = (C.c_double * 96)(), (C.c_char_p * 96)()
    k = lib.pnp_last_stage_times(C.c_void_p(lib.pnp_v1_context()), ms, names, 96)
    assert 0 < k <= 96
    return [(names[i].decode(), ms[i]) for i in range(k)]
"""


def _v1_child(body, **env):
    import os
    import subprocess
    import sys
    import textwrap
    here = os_path_tests()
    code = _V1_CHILD % (here, os.path.join(os.path.dirname(here), "zprize23-gpu-submission_amd"))
    return subprocess.run([sys.executable, "-c", code + textwrap.dedent(body)], env=dict(os.environ, **env),
                          capture_output=True, text=True, timeout=240)


_V1_COLD_HEAD = ["v1_ctx_create", "v1_load_prover_key", "v1_load_commit_key", "v1_prove"]
_V1_COLD_TAIL = ["v1_hash_wait", "v1_call"]


def test_v1_cold_stage_list():
    """A fresh process's first gen_proof (both keys need loading) publishes its
    own stages around the proof's; the second call on the unchanged keys proves
    beside the hash and publishes the proof's stages alone."""
    r = _v1_child("""
        inp = Inputs(8, 71)
        assert same(lib.gen_proof(inp.circuit, inp.pk, inp.ck), inp)
        cold = [n for n, _ in v1_stages()]
        assert same(lib.gen_proof(inp.circuit, inp.pk, inp.ck), inp)
        warm = [n for n, _ in v1_stages()]
        ctx = pnp.Context(0)
        ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
        assert same(ctx.prove(inp.circuit, device_ptrs=False), inp)
        v2 = [n for n, _ in ctx.stage_times()]
        ctx.close()
        assert v2 and not any(n.startswith("v1_") for n in v2), v2
        assert cold == %r + v2 + %r, cold
        assert warm == v2, warm
        print("DONE")
    """ % (_V1_COLD_HEAD, _V1_COLD_TAIL))
    assert r.returncode == 0 and "DONE" in r.stdout, r.stderr[-2000:]


@pytest.mark.parametrize("no_speculate", [False, True])
def test_v1_strict_on_resident_context(no_speculate):
    """PNP_V1_STRICT=1 after the first call: the key buffers of a Merkle-class
    key that proved are rewritten to a key with live q_m / q_lookup selectors;
    the next call sees the change (by the hash beside the proof on the
    resident keys, or with PNP_V1_NO_SPECULATE by the hash first), loads the
    key and refuses it."""
    env = {"PNP_V1_STRICT": "1"}
    if no_speculate:
        env["PNP_V1_NO_SPECULATE"] = "1"
    r = _v1_child("""
        inp = Inputs(8, 47)
        live = Inputs(8, 47, qm_qlookup_evals=True)
        assert same(lib.gen_proof(inp.circuit, inp.pk, inp.ck), inp)
        print("FIRST", flush=True)
        for name, arr in inp.arrays.items():
            if live.arrays[name].shape == arr.shape:
                arr[...] = live.arrays[name]
        for f in ("q_m_coeffs", "q_m_evals", "q_lookup_coeffs", "q_lookup_evals"):
            if f not in inp.arrays:
                inp.arrays[f] = live.arrays[f]
        inp._build_structs()
        lib.gen_proof(inp.circuit, inp.pk, inp.ck)
        print("SECOND", flush=True)
    """, **env)
    assert "FIRST" in r.stdout, r.stderr[-2000:]
    assert r.returncode != 0 and "SECOND" not in r.stdout and "PNP_V1_STRICT" in r.stderr, r.stderr[-2000:]


@pytest.mark.parametrize("reuse", [False, True])
def test_v1_reload(reuse):
    """PNP_V1_RELOAD=1 uploads both keys on every call: a word rewritten
    between two calls, one the reuse fingerprint does not sample, is read, also
    with PNP_V1_REUSE=1 set beside it (RELOAD decides the loading)."""
    env = {"PNP_V1_RELOAD": "1"}
    if reuse:
        env["PNP_V1_REUSE"] = "1"
    r = _v1_child("""
        inp = Inputs(8, 72)
        first = lib.gen_proof(inp.circuit, inp.pk, inp.ck)
        assert same(first, inp)
        assert same(lib.gen_proof(inp.circuit, inp.pk, inp.ck), inp)
        qc = inp.arrays["q_c_evals"]
        assert (qc.size - 1) // 256 > 15   # element 3: between two sampled words
        qc[3] = qc[5]
        got = lib.gen_proof(inp.circuit, inp.pk, inp.ck)
        assert abi.proof_to_bytes(got) != abi.proof_to_bytes(first)
        assert same(got, inp)
        print("DONE")
    """, **env)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stderr[-2000:]


def test_v1_domain_change():
    """2^8, 2^9, then the 2^8 input again, default mode: the second and third
    calls find keys resident at another domain and take the cold call's path on
    the context that exists (v1_ctx_create reported as 0)."""
    r = _v1_child("""
        a, b = Inputs(8, 73), Inputs(9, 74)
        for k, inp in enumerate((a, b, a)):
            assert same(lib.gen_proof(inp.circuit, inp.pk, inp.ck), inp), k
            st = v1_stages()
            names = [n for n, _ in st]
            assert names[:4] == %r and names[-2:] == %r, (k, names)
            assert (st[0][1] > 0) == (k == 0), (k, st[0])
        print("DONE")
    """ % (_V1_COLD_HEAD, _V1_COLD_TAIL))
    assert r.returncode == 0 and "DONE" in r.stdout, r.stderr[-2000:]
