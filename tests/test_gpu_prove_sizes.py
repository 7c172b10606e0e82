"""Proofs at the domain sizes between the ones tests/test_gpu_prove.py and
tests/test_gpu_full.py pin, byte for byte against the CPU restatement.  The
size decides the NTT pass split (2^7: the first size where 8 blocks are whole
tiles and 6 are not; 2^11 (6, 5), 2^12 (6, 6), 2^13 (7, 6), 2^15 (8, 7)), the
MSM window, the depth of the scans' CHUNK = 32 recursions and the evaluation
grid."""
import os
import subprocess
import sys

import pytest

from pnp_testlib import Inputs, inputs_pis, inputs_vk, verify
from pnp import abi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)


@pytest.mark.parametrize("lg", [7, 11, 12, 13, 15])
def test_synthetic_gpu_equals_cpu_sizes(lg):
    """bench.Synthetic on the GPU and SyntheticCPU build the same instance;
    the resident-key proof is the oracle's, and the restated verifier accepts."""
    import pnp
    from bench import Synthetic
    from synth_cpu import SyntheticCPU
    n = 1 << lg
    gates, seed = (n - 20 if lg == 7 else n - 1000), 40 + lg
    cpu = SyntheticCPU(lg, gates, seed)
    exp = cpu.oracle_proof()
    ctx = pnp.Context(0)
    try:
        syn = Synthetic(ctx, lg, gates, seed=seed)
        ctx.load_prover_key(syn.pk, syn.n, device_ptrs=True)
        ctx.load_commit_key(syn.ck, syn.n, device_ptrs=True)
        got = ctx.prove(syn.cs, device_ptrs=True)
        assert abi.proof_to_bytes(got) == abi.proof_to_bytes(exp)
        assert verify(cpu.vk(), got, cpu.pis(), cpu.tau_mont[0])
    finally:
        ctx.close()


@pytest.mark.parametrize("lg", [7, 11, 12])
def test_general_key_sizes(lg):
    """The general key (k_quotient_, k_widgets_, live lookups: random q_m /
    q_lookup evaluations and 17 lookup rows) at the same pass splits."""
    import pnp
    inp = Inputs(lg, 50 + lg, lookup_rows=17, qm_qlookup_evals=True)
    exp = inp.oracle_proof()
    ctx = pnp.Context(0)
    try:
        ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
        got = ctx.prove(inp.circuit, device_ptrs=False)
        assert abi.proof_to_bytes(got) == abi.proof_to_bytes(exp)
        assert any(v != 0 for v in exp.f_comm.x) and any(v != 0 for v in exp.h_1_comm.x)
    finally:
        ctx.close()


@pytest.mark.parametrize("satisfying,redo", [(True, 0), (False, 1)])
def test_quot_blocks_7_whole_tiles(satisfying, redo):
    """PNP_QUOT_BLOCKS=7 at 2^10, where 7 blocks are whole tiles: round 4's
    transforms run k_ntt_pass4<10> over 7 blocks (at 2^8, where
    test_prover_switches_same_proof runs, 7 blocks take the small path).  A
    fresh child process: the switch is read once per process.  redo = the
    expected quotient_all_blocks count (unsatisfied: from 7 to 8 blocks)."""
    code = (
        "import sys; sys.path[:0] = [%r, %r]\n"
        "from pnp import abi\n"
        "from pnp_testlib import Inputs\n"
        "import pnp\n"
        "inp = Inputs(10, 71, satisfying=%r)\n"
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
    ) % (HERE, os.path.join(REPO, "zprize23-gpu-submission_amd"), satisfying)
    env = dict(os.environ, PNP_QUOT_BLOCKS="7")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SAME" in r.stdout
    assert "redo=%d" % redo in r.stdout


def test_first_proof_lagrange_lookups_two_pass(monkeypatch):
    """A fresh context's first proof with the Lagrange basis built up front
    (PNP_DEFER_TABLES=0) of a lookup circuit at 2^11: round 1's inverse
    transforms of the wires run on the side stream and rounds 2 and 3's on the
    main stream, all two-pass (6, 5) through the inverse twiddle rows.
    ntt_warm builds those rows on the main stream before the first fork; when
    the side stream's first transform built them lazily, the main stream read
    the buffer with no event after the build kernel.  A race cannot be made to
    fail on demand: the fix holds by construction (ntt_warm), and this test
    pins that the path (first proof, Lagrange on, lookups, two-pass inverse
    transforms) runs at all and gives the oracle's bytes."""
    import pnp
    inp = Inputs(11, 66, lookup_rows=17)
    exp = inp.oracle_proof()
    monkeypatch.setenv("PNP_DEFER_TABLES", "0")
    ctx = pnp.Context(0)  # the switch is read when the context is made
    try:
        ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
        got = ctx.prove(inp.circuit, device_ptrs=False)
        assert abi.proof_to_bytes(got) == abi.proof_to_bytes(exp)
        assert any(v != 0 for v in exp.f_comm.x)
        assert verify(inputs_vk(inp), got, inputs_pis(inp), inp.tau_mont[0])
    finally:
        ctx.close()
