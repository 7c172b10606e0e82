#!/usr/bin/env python3
"""One fixed sequence of witness calls in one process, for counting the HIP
calls a library makes for them (run it under the profiler's HIP trace with
stats, once per library; PNP_PLONK_LIB selects the library):

    timeout -k 10 600 rocprofv3 --hip-trace --stats -d OUT -- python tools/witness_calls.py

At merkle(9) of tests/merkle_circuit.py (49,220 rows, D = 2^16), a synthetic
SRS:
  1. pnp_preprocess;
  2. pnp_check_witness, columns in host memory and in HBM;
  3. pnp_check_assignment, host and HBM;
  4. the three plan loads: pnp_load_solve_inputs, pnp_load_solve_plan (the root
     row as output) and, on a context of its own with the range-chain
     circuit of tests/test_gpu_solve_gates.py, pnp_load_solve_plan_gates with
     a solve;
  5. two solves over the plan with the output row, inputs in host memory and
     in HBM;
  6. pnp_solved_public_inputs, pnp_check_solved, pnp_prove_solved;
  7. one unsatisfied check (a changed value).
Every result is asserted, and the proof's bytes are printed as a hash: they
must be equal between the libraries."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "zprize23-gpu-submission_amd"), os.path.join(REPO, "tests")]


def main():
    import torch
    import pnp
    from pnp import abi
    from gpu_util import to_dev
    from pnp_testlib import ptr_of
    from solve_gates_ref import RANGE
    from test_assignment_ref import assignment_values
    from test_gpu_solve import context_for, load_inputs, merkle, mont
    from test_gpu_solve_gates import load_gates, wide_and_narrow
    from test_gpu_solve_outputs import load_plan
    from test_preprocess_ref import wire_map

    if not torch.cuda.is_available():
        raise SystemExit("witness_calls: no GPU")
    cp, ids, _ = merkle(9)
    ng, n_vars, root_row = len(cp.rows), len(cp.vals), len(cp.rows) - 1
    D = 1 << 16
    assert ng == 49220 and list(cp.pis) == [root_row]
    pis = sorted(cp.pis.items())
    values = assignment_values(cp)
    var = wire_map(cp)
    cols = [np.ascontiguousarray(values[var[j]]) for j in range(4)]
    inputs = mont([cp.vals[u] for u in ids])

    ctx = context_for(cp)  # 1. preprocess
    srs = torch.zeros((D, 12), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.srs(srs.data_ptr(), D, [5, 0, 0, 0])
    ctx.sync()
    ck = abi.CommitKeyC(powers_of_g=abi.ptr(srs.data_ptr()), powers_of_gamma_g=abi.ptr(srs.data_ptr()))
    ctx.load_commit_key(ck, D, device_ptrs=True)

    def circuit(w):
        return abi.CircuitC(n=ng, lookup_len=0, intended_pi_pos=0, pi=None, q_lookup=None, w_l=w[0], w_r=w[1],
                            w_o=w[2], w_4=w[3])
    # 2. the columns form
    ok, rep = ctx.check_witness(circuit([ptr_of(c) for c in cols]), False, pis)
    assert ok and rep.copy_checked == 1, ctx.last_error()
    dcols = [to_dev(c) for c in cols]
    ok, rep = ctx.check_witness(circuit([abi.ptr(t.data_ptr()) for t in dcols]), True, pis)
    assert ok and rep.copy_checked == 1, ctx.last_error()
    # 3. the assignment form
    assert ctx.check_assignment(values.ctypes.data, n_vars, False, pis)[0], ctx.last_error()
    dvalues = to_dev(values)
    assert ctx.check_assignment(dvalues.data_ptr(), n_vars, True, pis)[0], ctx.last_error()
    # 4. the plans (the gates one below)
    assert load_inputs(ctx, ids)[0] == 0, ctx.last_error()
    assert load_plan(ctx, ids, [root_row])[0] == 0, ctx.last_error()
    # 5. two solves
    ctx.solve_assignment(inputs.ctypes.data, len(ids), False, [])
    dinputs = to_dev(inputs)
    ctx.solve_assignment(dinputs.data_ptr(), len(ids), True, [])
    # 6. what reads the solution
    assert ctx.solved_public_inputs() == pis
    ok, rep = ctx.check_solved([])
    assert ok and rep.violations == 0, ctx.last_error()
    proof = abi.proof_to_bytes(ctx.prove_solved([]))
    # 7. one unsatisfied check
    broken = values.copy()
    broken[28, 0] ^= 1
    ok, rep = ctx.check_assignment(broken.ctypes.data, n_vars, False, pis)
    assert not ok and rep.violations > 0
    unsat = ctx.last_error()
    ctx.close()

    # 4. the plan with gate rows, and a solve over it
    gcp, gids, gpl, gvals = wide_and_narrow()
    gctx = context_for(gcp)
    assert load_gates(gctx, gids, RANGE)[0] == 0, gctx.last_error()
    ginputs = mont([gcp.vals[u] for u in gids])
    gctx.solve_assignment(ginputs.ctypes.data, len(gids), False, [])
    entries = gctx.solve_gate_entries()
    assert entries == (gpl.n_range, gpl.n_logic)
    assert gctx.check_solved([])[0], gctx.last_error()
    gctx.close()
    print("witness_calls ok: proof sha256 %s; unsat: %s; gate entries %s" %
          (hashlib.sha256(proof).hexdigest()[:16], unsat, entries))


if __name__ == "__main__":
    main()
