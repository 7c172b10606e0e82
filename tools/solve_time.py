#!/usr/bin/env python3
"""Time the witness solver at the bench's size (one GPU process; run it once,
under a timeout of its own):

    timeout -k 10 900 python tools/solve_time.py [--height 15] [--out profiles/solve_time.json]

The circuit is the reference's Poseidon Merkle tree at HEIGHT (15: 3,161,924
rows on D = 2^22, 3,194,709 variables) as tests/merkle_circuit.py lays it out.
Building that composer in Python would take minutes, so the wire map, the
selector rows and the input list are tiled with numpy from the per-hash
template (193 rows, 193 fresh variables) taken from merkle_circuit(3); before
anything runs on the GPU the tiling is asserted to reproduce merkle_circuit(6)
exactly (wire map, every selector row, n_vars, the input ids).  The inputs are
the 8 blinding values, the leaves and the per-hash domain tags; the root (for
the public input, which defines the root variable) comes from the native
Poseidon tree on the CPU.

Measured: pnp_preprocess, the plan build (pnp_load_solve_inputs, three times),
the solve alone, and after the warm-up proofs two paths interleaved, --reps of
each: solve + prove from the resident solution, against prove from the same
assignment uploaded from host memory.  The solution must pass
pnp_check_assignment, hold the CPU's root, and every proof must be the same
bytes.

    timeout -k 10 900 python tools/solve_time.py --outputs [--out profiles/solve_outputs_time.json]

The root row as an output of the plan (pnp_load_solve_plan): the solve is given
the leaves and no public input, PI = -root comes out of it, pnp_prove_solved
proves, and nothing computes the root on the CPU before the proofs.  Beside it,
in the same process, the present path: the plan without outputs, the solve and
the proof given the public input (here the derived one).  After two warm-up
visits --reps visits of each path, interleaved; a visit is the plan build, a
solve, and a solve + prove, each timed.  Afterwards the native tree is
computed once and the derived root compared with it; every proof of both paths
must be the same bytes.

    timeout -k 10 900 python tools/solve_time.py --gates [--out profiles/solve_gates_time.json]

Range and logic rows that define (pnp_load_solve_plan_gates): a synthetic
circuit of N 64-bit range checks of computed sums x = p + q and N / 2 64-bit
XORs of pairs of those sums, laid out as the reference's composer lays
range_gate and logic_gate (tests/gate_circuits.py), N chosen so that the domain
is 2^20.  One unit (two sums, their range checks, one XOR: 57 rows) is built by
the composer and tiled with numpy; the tiling is asserted to reproduce a
three-unit composer circuit exactly.  The inputs are the p and q alone.
Measured: the plan build (three times), the solve (--reps), the solve_levels
kernels' own time, the entries by family and plan_bytes.  The solution must
pass pnp_check_solved and hold the sums and the XORs Python computes.

    timeout -k 10 900 python tools/solve_time.py --ecc [--inverse binary] [--out profiles/solve_ecc_time.json]

Fixed-base and curve-addition rows that define (pnp_load_solve_plan_ecc): K
units of a sum s = p + q, the reference's 255-row fixed_base_scalar_mul of s
and a point_addition_gate that adds the result to a running point
(tests/ecc_circuits.py), for K = 1 and K = 1024 on D = 2^19: the depth (about
2 + 254 + 255 levels a multiplication, then one a var-add row) is paid once
whatever K.  One unit is built by the composer and tiled with numpy, the
running point's variables patched to the unit before; the tiling is asserted to
reproduce a three-unit composer circuit.  The inputs are the first point and
the p and q alone.  Measured per K: the plan build (three times), the solve
(--reps), the solve_levels kernels' own time, levels and entries by family.
The solution must pass pnp_check_solved, and the first unit's sum must be
Python's.  --inverse names the inversion the loaded library was built with
(csrc/solve.hip kEccInverseBinary: "binary", or "fermat" for a library built
with -DPNP_ECC_INVERSE_BINARY=0 and given in PNP_PLONK_LIB); the result goes
under that name, beside what the file already holds.

    timeout -k 10 900 python tools/solve_time.py --lookup [--out profiles/solve_lookup_time.json]

Lookup rows that define (pnp_load_solve_plan_lookup), against the 8-bit XOR
table (LookupTable::xor_table(0, 8), 65,536 rows), two shapes:
  wide   N units of x = p + q, y = r + s, z = lookup(x, y, -1): N independent
         byte XORs over values the circuit computes, N chosen for D = 2^20;
         two levels, the second one N lookup entries
  deep   a chain of L = 4,096 lookups, z_(k+1) = lookup(z_k, b_k, -1): each
         output is the next key, one entry a level, D = 2^16 (the table)
Both are laid out with numpy; a three-unit (three-step) instance is asserted
to reproduce the composer's circuit of tests/lookup_circuits.py.  The inputs
are the p, q, r, s (z_0 and the b_k) alone.  Measured per shape: the plan build
(three times; it includes the table index), the solve (--reps), the
solve_levels kernels' own time, levels, entries, indexed rows and plan_bytes.
The solution must pass pnp_check_solved and probed XORs must be Python's.  The
result goes under "lookup", beside what the file already holds."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "zprize23-gpu-submission_amd"), os.path.join(REPO, "tests")]

HASH_ROWS = 193   # rows, and fresh variables, per hash
HEAD_ROWS = 4     # zero_var's gate and the three blinding rows
ZERO, LEFT, RIGHT, NODE = -1, -2, -3, -4
SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_hl", "q_hr", "q_h4", "q_arith")


def shape(height):
    leaves = 1 << (height - 1)
    hashes = leaves - 1
    return leaves, hashes, HASH_ROWS * hashes + HEAD_ROWS + 1, 9 + leaves + hashes + HASH_ROWS * hashes


def hash_order(height):
    """Node index of every hash in row order (constraints.rs:39-99: the bottom
    non-leaf level first, then upwards; within a level ascending)."""
    starts, idx = [], 0
    for _ in range(height - 1):
        starts.append(idx)
        idx = 2 * idx + 1
    return np.concatenate([np.arange(s, 2 * s + 1, dtype=np.int64) for s in reversed(starts)])


def template(height=3):
    """(codes (4, 193), head ids (4, 4), {selector: (head, hash, last) canonical ints}) from merkle_circuit(height):
    a wire of the first hash is a fresh variable of the hash (its offset), zero_var, the hash's left or right input,
    or the node it is asserted equal to."""
    import merkle_circuit as mc
    cp = mc.merkle_circuit(height, seed=1)[0]
    leaves, hashes, ng, n_vars = shape(height)
    assert (len(cp.rows), len(cp.vals)) == (ng, n_vars)
    base = 9 + leaves + hashes
    node = 9 + leaves + int(hash_order(height)[0])
    named = {0: ZERO, 9: LEFT, 10: RIGHT, node: NODE}
    codes = np.zeros((4, HASH_ROWS), dtype=np.int64)
    for k in range(HASH_ROWS):
        for j, v in enumerate(cp.rows[HEAD_ROWS + k][1]):
            codes[j, k] = v - base if base <= v < base + HASH_ROWS else named[v]
    head = np.array([cp.rows[i][1] for i in range(HEAD_ROWS)], dtype=np.int64).T
    assert cp.rows[-1][1] == (9 + leaves, 0, 0, 0)
    sel = {}
    for name in SELECTORS:
        col = [r[0].get(name, 0) for r in cp.rows]
        # every hash has the template's selectors
        assert all(col[HEAD_ROWS + HASH_ROWS * h:HEAD_ROWS + HASH_ROWS * (h + 1)] == col[HEAD_ROWS:HEAD_ROWS + HASH_ROWS]
                   for h in range(hashes))
        sel[name] = (col[:HEAD_ROWS], col[HEAD_ROWS:HEAD_ROWS + HASH_ROWS], col[-1:])
    return codes, head, sel


def tile(height, tpl):
    """(var (4, n_gates) u32, {selector: canonical ints by part}, input ids, n_vars, root variable) at `height`."""
    codes, head, sel = tpl
    leaves, hashes, ng, n_vars = shape(height)
    node_i = hash_order(height)
    base = 9 + leaves + hashes + HASH_ROWS * np.arange(hashes, dtype=np.int64)
    bottom = node_i >= leaves // 2 - 1
    left = np.where(bottom, 9 + 2 * node_i + 1 - (leaves - 1), 9 + leaves + 2 * node_i + 1)
    named = {ZERO: np.zeros(hashes, dtype=np.int64), LEFT: left, RIGHT: left + 1, NODE: 9 + leaves + node_i}
    var = np.zeros((4, ng), dtype=np.uint32)
    var[:, :HEAD_ROWS] = head
    for j in range(4):
        block = base[:, None] + codes[j][None, :]
        for code, ids in named.items():
            block = np.where(codes[j][None, :] == code, ids[:, None], block)
        var[j, HEAD_ROWS:ng - 1] = block.reshape(-1)
    var[:, ng - 1] = (9 + leaves, 0, 0, 0)
    ids = np.concatenate([np.arange(1, 9 + leaves), var[0, HEAD_ROWS:ng - 1:HASH_ROWS].astype(np.int64)])
    return var, sel, ids.astype(np.uint32), n_vars, 9 + leaves


def mont_rows(ints):
    from pnp_testlib import fr_mont, ints_to_arr
    return ints_to_arr([fr_mont(v) for v in ints])


def selector_column(parts, hashes):
    head, one, last = (mont_rows(p) for p in parts)
    return np.ascontiguousarray(np.concatenate([head, np.tile(one, (hashes, 1)), last]))


def assert_tiling_reproduces(height, tpl):
    import merkle_circuit as mc
    from solve_ref import merkle_inputs
    from test_preprocess_ref import wire_map
    cp = mc.merkle_circuit(height, seed=2)[0]
    var, sel, ids, n_vars, root_var = tile(height, tpl)
    assert n_vars == len(cp.vals) and np.array_equal(var, wire_map(cp))
    hashes = shape(height)[1]
    for name in SELECTORS:
        assert np.array_equal(selector_column(sel[name], hashes), mont_rows([r[0].get(name, 0) for r in cp.rows])), name
    assert list(ids) == merkle_inputs(cp) and cp.rows[-1][1][0] == root_var
    assert not any(r[0].get(k) for r in cp.rows for k in r[0] if k not in SELECTORS)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def setup(args, with_root):
    """The instance at args.height and a context with its key and wire map
    resident.  with_root: the root from the native Poseidon tree on the CPU
    (r.root, r.cpu_tree_s); without it nothing here knows the root."""
    from types import SimpleNamespace
    r = SimpleNamespace()
    t0 = time.perf_counter()
    tpl = template()
    assert_tiling_reproduces(6, tpl)
    from pnp_testlib import R_MOD, fr_mont, ints_to_arr
    from merkle_circuit import merkle_tree
    from poseidon import PoseidonConstants
    r.height = args.height
    r.leaves, r.hashes, r.ng, r.n_vars = shape(r.height)
    r.D = 1 << max(4, (r.ng - 1).bit_length())
    r.var, sel, r.ids, r.n_vars, r.root_var = tile(r.height, tpl)
    r.cols = {name: selector_column(parts, r.hashes) for name, parts in sel.items() if any(any(p) for p in parts)}
    rng = np.random.default_rng(args.seed)
    rnd = lambda: int.from_bytes(rng.bytes(32), "little") % R_MOD
    pc = PoseidonConstants()
    blind, r.leaf_vals = [rnd() for _ in range(8)], [rnd() for _ in range(r.leaves)]
    r.cpu_root = lambda: merkle_tree(pc, r.leaf_vals)[0]
    r.root = r.cpu_tree_s = None
    if with_root:
        t1 = time.perf_counter()
        r.root = r.cpu_root()
        r.cpu_tree_s = time.perf_counter() - t1
    r.inputs = ints_to_arr([fr_mont(v) for v in blind + r.leaf_vals + [pc.domain_tag] * r.hashes])
    assert len(r.inputs) == len(r.ids)
    r.build_s = time.perf_counter() - t0

    import torch
    import pnp
    from pnp import abi
    if not torch.cuda.is_available():
        raise SystemExit("solve_time: no GPU (a measurement needs one; nothing is written)")
    desc = abi.CircuitDesc(n_gates=r.ng, n_vars=r.n_vars, lookup_len=0)
    for j in range(4):
        desc.var[j] = r.var[j].ctypes.data_as(abi.U32P)
    for k, name in enumerate(abi.DESC_SELECTORS):
        if name in r.cols:
            desc.sel[k] = r.cols[name].ctypes.data_as(abi.U64P)
    r.ctx = ctx = pnp.Context(0)
    r.srs = torch.zeros((r.D, 12), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.srs(r.srs.data_ptr(), r.D, [5, 0, 0, 0])
    ctx.sync()
    ck = abi.CommitKeyC(powers_of_g=abi.ptr(r.srs.data_ptr()), powers_of_gamma_g=abi.ptr(r.srs.data_ptr()))
    ctx.load_commit_key(ck, r.D, device_ptrs=True)
    t0 = time.perf_counter()
    ctx.preprocess(desc, device_ptrs=False)
    r.preprocess_s = time.perf_counter() - t0
    return r


def spread(xs):
    return max(xs) - min(xs)


def main_outputs(args, reps):
    """The root row as an output of the plan: nothing computes the root on the
    CPU before the proofs; the present path (PI given, here the derived one)
    runs beside it, plan build, solve and solve + prove interleaved."""
    from pnp import abi
    from pnp_testlib import R_MOD
    r = setup(args, with_root=False)
    ctx, ids, inputs, n_vars = r.ctx, r.ids, r.inputs, r.n_vars
    root_row = np.array([r.ng - 1], dtype=np.uint64)

    def timed(f, *a):
        t0 = time.perf_counter()
        out = f(*a)
        return time.perf_counter() - t0, out

    def plan(outputs):
        if outputs:
            rc, info = ctx.load_solve_plan(ids.ctypes.data, len(ids), root_row.ctypes.data, 1, False)
        else:
            rc, info = ctx.load_solve_inputs(ids.ctypes.data, len(ids), False)
        if rc != 0 or info.n_solved + info.n_inputs != n_vars:
            raise SystemExit(f"solve_time: no plan: {ctx.last_error()}")
        return info

    def solve(pis):
        ctx.solve_assignment(inputs.ctypes.data, len(ids), False, pis)
        return dict(ctx.stage_times())

    def solve_and_prove(outputs, pis):
        ctx.solve_assignment(inputs.ctypes.data, len(ids), False, [] if outputs else pis)
        if outputs:
            return abi.proof_to_bytes(ctx.prove_solved([]))
        addr, n = ctx.assignment_ptr()
        return abi.proof_to_bytes(ctx.prove_assignment(addr, n, True, pis))

    def visit(outputs, pis, keep):
        """One path once: its plan, a solve, a solve + prove."""
        t_plan, info = timed(plan, outputs)
        t_solve, st = timed(solve, [] if outputs else pis)
        t_both, proof = timed(solve_and_prove, outputs, pis)
        if keep is not None:
            keep["plan_build"].append(t_plan)
            keep["solve"].append(t_solve)
            keep["solve_and_prove"].append(t_both)
            keep["stages"].append(st)
        return info, proof

    # the derived root is what the present path is given: nothing else knows it yet
    plan(True)
    solve([])
    derived = ctx.solved_public_inputs()
    ok, rep = ctx.check_solved([])
    if not ok or [p for p, _ in derived] != [r.ng - 1]:
        raise SystemExit(f"solve_time: the solution fails the check: {ctx.last_error()}")
    # warm-up: the first proof goes without the context's tables, which are then
    # built in the background (pnp_sync waits for them); one more visit of each path
    info_out, ref = visit(True, derived, None)
    ctx.sync()
    info_in, proof = visit(False, derived, None)
    proofs = [proof, visit(True, derived, None)[1]]
    ctx.sync()
    runs = {"outputs": {"plan_build": [], "solve": [], "solve_and_prove": [], "stages": []},
            "given": {"plan_build": [], "solve": [], "solve_and_prove": [], "stages": []}}
    infos = {"outputs": [bytes(info_out)], "given": [bytes(info_in)]}
    for _ in range(reps):
        for name, outputs in (("outputs", True), ("given", False)):
            info, proof = visit(outputs, derived, runs[name])
            infos[name].append(bytes(info))
            proofs.append(proof)
            if outputs and ctx.solved_public_inputs() != derived:
                raise SystemExit("solve_time: the derived public input differs between solves")
    hbm = ctx.hbm_usage()["live"]
    ctx.close()
    all_equal = all(p == ref for p in proofs)
    same_plans = all(len(set(v)) == 1 for v in infos.values())
    # only now the native tree, once, as a check
    t0 = time.perf_counter()
    root = r.cpu_root()
    cpu_tree_s = time.perf_counter() - t0
    root_ok = derived == [(r.ng - 1, -root % R_MOD)]

    out = {"height": r.height, "lg": r.D.bit_length() - 1, "n_gates": r.ng, "n_vars": n_vars,
           "n_inputs": int(info_out.n_inputs), "output_rows": [r.ng - 1],
           "n_levels": {"outputs": int(info_out.n_levels), "given": int(info_in.n_levels)},
           "plan_bytes": {"outputs": int(info_out.plan_bytes), "given": int(info_in.plan_bytes)},
           "reps_each": reps, "interleaved": True, "warm_up_visits": {"outputs": 2, "given": 1},
           "derived_root_equals_cpu_tree": bool(root_ok), "cpu_root_computed_before_proving": False,
           "solution_passes_check_solved": True, "plan_same_on_every_build": bool(same_plans),
           "all_proofs_equal": bool(all_equal), "proofs_compared": len(proofs) + 1,
           "hbm_live_bytes_at_end": int(hbm),
           "host_side_s": {"build_instance": round(r.build_s, 2), "cpu_poseidon_tree_afterwards": round(cpu_tree_s, 2),
                           "preprocess": round(r.preprocess_s, 3)}}
    for what in ("plan_build", "solve", "solve_and_prove"):
        o, g = runs["outputs"][what], runs["given"][what]
        out[what + "_s"] = {
            "outputs_runs": [round(x, 5) for x in o], "given_runs": [round(x, 5) for x in g],
            "outputs_median": round(median(o), 5), "given_median": round(median(g), 5),
            "outputs_range": round(spread(o), 5), "given_range": round(spread(g), 5),
            "median_difference": round(median(o) - median(g), 5),
            "difference_exceeds_own_range": bool(median(o) - median(g) > max(spread(o), spread(g)))}
    out["solve_stage_ms_median"] = {
        name: {k: round(median([st[k] for st in runs[name]["stages"]]), 4) for k in runs[name]["stages"][0]
               if k != "inputs_h2d_bytes"} for name in runs}
    if not (all_equal and same_plans and root_ok):
        raise SystemExit("solve_time: " + json.dumps({k: out[k] for k in (
            "all_proofs_equal", "plan_same_on_every_build", "derived_root_equals_cpu_tree")}))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


GATE_SELECTORS = SELECTORS + ("range_selector", "logic_selector")


def gates_unit(cp, rng):
    """Two sums x = p + q with range_of(x, 64) and the XOR of the two over 64
    bits; returns ([p, q, p, q], [x, x], the result variable)."""
    from gate_circuits import M1, logic_of, range_of
    ins, xs = [], []
    for _ in range(2):
        p, q = cp.var(int(rng.integers(0, 1 << 62))), cp.var(int(rng.integers(0, 1 << 62)))
        x = cp.var(cp.vals[p] + cp.vals[q])
        cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, p, q, x, 0)
        range_of(cp, x, 64)
        ins += [p, q]
        xs.append(x)
    return ins, xs, logic_of(cp, xs[0], xs[1], 64, True)[1]


def gates_circuit(units, tpl=None):
    """(var (4, n_gates) u32, {selector: (n_gates, 4) Montgomery rows}, n_vars, input ids, [x ids], [result ids]):
    from the composer itself (tpl None), or the one-unit template tiled."""
    from circuits import Composer
    from test_preprocess_ref import wire_map
    if tpl is None:
        cp = Composer(1)
        rng = np.random.default_rng(1)
        got = [gates_unit(cp, rng) for _ in range(units)]
        cols = {name: mont_rows([r[0].get(name, 0) for r in cp.rows]) for name in GATE_SELECTORS}
        assert not any(k not in GATE_SELECTORS for r in cp.rows for k in r[0])
        return (wire_map(cp), cols, len(cp.vals), [0] + [v for g in got for v in g[0]], [v for g in got for v in g[1]],
                [g[2] for g in got])
    var1, cols1, n_vars1, ids1, xs1, res1 = tpl
    per, rows = n_vars1 - 1, var1.shape[1]
    shift = per * np.repeat(np.arange(units, dtype=np.int64), rows)
    tiled = np.tile(var1.astype(np.int64), (1, units))
    var = np.where(tiled == 0, 0, tiled + shift[None, :]).astype(np.uint32)
    cols = {name: np.ascontiguousarray(np.tile(c, (units, 1))) for name, c in cols1.items()}
    off = per * np.arange(units, dtype=np.int64)
    spread_ids = lambda vs: (np.array(vs, dtype=np.int64)[None, :] + off[:, None]).reshape(-1)
    ids = np.concatenate([[0], spread_ids(ids1[1:])])
    return var, cols, 1 + per * units, ids, spread_ids(xs1), spread_ids(res1)


def main_gates(args, reps):
    from pnp import abi
    from pnp_testlib import R_MOD, fr_mont, ints_to_arr
    t0 = time.perf_counter()
    tpl = gates_circuit(1)
    rows_unit = tpl[0].shape[1]
    want, got = gates_circuit(3), gates_circuit(3, tpl)
    assert np.array_equal(want[0], got[0]) and want[2] == got[2] and list(want[3]) == list(got[3])
    assert all(np.array_equal(want[1][k], got[1][k]) for k in GATE_SELECTORS)
    assert list(want[4]) == list(got[4]) and list(want[5]) == list(got[5])
    lg = args.lg
    units = ((1 << lg) - 1) // rows_unit
    var, cols, n_vars, ids, xs, res = gates_circuit(units, tpl)
    ng = var.shape[1]
    assert (1 << (lg - 1)) < ng < (1 << lg)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    rng = np.random.default_rng(args.seed)
    vals = [0] + [int(v) for v in rng.integers(0, 1 << 62, size=len(ids) - 1)]
    inputs = ints_to_arr([fr_mont(v) for v in vals])
    sums = [vals[1 + 2 * k] + vals[2 + 2 * k] for k in range(2 * units)]
    xors = [sums[2 * k] ^ sums[2 * k + 1] for k in range(units)]
    build_s = time.perf_counter() - t0

    import torch
    import pnp
    if not torch.cuda.is_available():
        raise SystemExit("solve_time: no GPU (a measurement needs one; nothing is written)")
    desc = abi.CircuitDesc(n_gates=ng, n_vars=n_vars, lookup_len=0)
    var = np.ascontiguousarray(var)
    for j in range(4):
        desc.var[j] = var[j].ctypes.data_as(abi.U32P)
    for k, name in enumerate(abi.DESC_SELECTORS):
        if name in cols and cols[name].any():
            desc.sel[k] = cols[name].ctypes.data_as(abi.U64P)
    ctx = pnp.Context(0)
    t0 = time.perf_counter()
    ctx.preprocess(desc, device_ptrs=False)
    preprocess_s = time.perf_counter() - t0

    plan_s, infos = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        rc, info = ctx.load_solve_plan_gates(ids.ctypes.data, len(ids), 0, 0, abi.SOLVE_RANGE | abi.SOLVE_LOGIC, False)
        plan_s.append(time.perf_counter() - t0)
        if rc != 0:
            raise SystemExit(f"solve_time: no plan: {ctx.last_error()}")
        infos.append(bytes(info))
    if len(set(infos)) != 1 or info.n_solved + info.n_inputs != n_vars:
        raise SystemExit("solve_time: the plan differs between builds, or does not cover every variable")
    n_range, n_logic = ctx.solve_gate_entries()

    def solve():
        t0 = time.perf_counter()
        ctx.solve_assignment(inputs.ctypes.data, len(ids), False)
        return time.perf_counter() - t0, dict(ctx.stage_times())

    solve()
    ok, rep = ctx.check_solved([])
    if not ok:
        raise SystemExit(f"solve_time: the solution fails the check: {ctx.last_error()}")
    to_int = lambda limbs: sum(int(w) << (64 * k) for k, w in enumerate(limbs))
    probe = sorted(set(range(0, units, max(1, units // 64))) | {units - 1})
    got_x = [to_int(l) for l in ctx.assignment_values(ids=[int(xs[2 * k]) for k in probe])]
    got_r = [to_int(l) for l in ctx.assignment_values(ids=[int(res[k]) for k in probe])]
    if got_x != [fr_mont(sums[2 * k]) for k in probe] or got_r != [fr_mont(xors[k]) for k in probe]:
        raise SystemExit("solve_time: the solved sums or XORs are not Python's")
    runs = [solve() for _ in range(reps)]
    ctx.kernel_timing(True)
    solve()
    levels_ms, _ = ctx.kernel_stats("solve_levels")
    levels_bytes = ctx.kernel_bytes("solve_levels")
    ctx.kernel_timing(False)
    hbm = ctx.hbm_usage()["live"]
    ctx.close()
    out = {
        "circuit": "N sums x = p + q with range_gate(x, 64), N / 2 xor_gate(x, x', 64), composer layout",
        "lg": lg, "n_gates": ng, "n_vars": n_vars, "range_checks": 2 * units, "xors": units,
        "n_inputs": int(info.n_inputs), "n_solved": int(info.n_solved), "n_levels": int(info.n_levels),
        "max_width": int(info.max_width), "entries": {"arithmetic": int(info.n_solved) - n_range - n_logic,
                                                     "range": int(n_range), "logic": int(n_logic)},
        "plan_bytes": int(info.plan_bytes), "tiling_reproduces_the_composer": True,
        "solution_passes_check_solved": True, "sums_and_xors_probed": len(probe), "plan_same_on_every_build": True,
        "plan_build_s_runs": [round(x, 4) for x in plan_s], "plan_build_s": round(median(plan_s), 4),
        "solve_s_runs": [round(t, 5) for t, _ in runs], "solve_s": round(median([t for t, _ in runs]), 5),
        "solve_stage_ms_median": {k: round(median([st[k] for _, st in runs]), 4) for k in ("solve_inputs", "solve_levels")},
        "levels_kernels_ms": round(levels_ms, 4), "levels_kernels_bytes": int(levels_bytes),
        "levels_kernels_gb_s": round(levels_bytes / (levels_ms * 1e-3) / 1e9, 1) if levels_ms > 0 else None,
        "reps": reps, "hbm_live_bytes_at_end": int(hbm),
        "host_side_s": {"build_instance": round(build_s, 2), "preprocess": round(preprocess_s, 3)},
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


ECC_SELECTORS = SELECTORS + ("fixed_group_add_selector", "variable_group_add_selector")


def ecc_circuit(units, tpl=None):
    """(var (4, n_gates) u32, {selector: rows}, n_vars, input ids, the last sum's (x, y) ids, the first unit's
    sum ids): from the composer itself (tpl None), or the one-unit template tiled.  Variables 1, 2 are the
    first running point."""
    from circuits import Composer, jj_point
    from ecc_circuits import fixed_base_mul_of, point_add_of
    from gate_circuits import M1
    from test_preprocess_ref import wire_map
    if tpl is None:
        cp = Composer(1)
        rng = np.random.default_rng(1)
        base = jj_point(cp.rng)
        start = jj_point(cp.rng)
        run = (cp.var(start[0]), cp.var(start[1]))
        ids, sums = [0, *run], []
        for _ in range(units):
            p, q = cp.var(int(rng.integers(0, 1 << 62))), cp.var(int(rng.integers(0, 1 << 62)))
            sv = cp.var(cp.vals[p] + cp.vals[q])
            cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, p, q, sv, 0)
            _, res = fixed_base_mul_of(cp, sv, base)
            _, run = point_add_of(cp, run, res)
            ids += [p, q]
            sums.append(run)
        cols = {name: mont_rows([r[0].get(name, 0) for r in cp.rows]) for name in ECC_SELECTORS}
        assert not any(k not in ECC_SELECTORS for r in cp.rows for k in r[0])
        return wire_map(cp), cols, len(cp.vals), ids, sums[-1], sums[0], (base, start)
    var1, cols1, n_vars1, ids1, last1, _, pts = tpl
    per, rows = n_vars1 - 3, var1.shape[1]
    tiled = np.tile(var1.astype(np.int64), (1, units))
    unit = np.repeat(np.arange(units, dtype=np.int64), rows)[None, :]
    var = np.where(tiled >= 3, tiled + per * unit, tiled)
    for j, prev in ((1, last1[0]), (2, last1[1])):  # the running point: the unit before's sum
        var = np.where((tiled == j) & (unit > 0), prev + per * (unit - 1), var)
    cols = {name: np.ascontiguousarray(np.tile(c, (units, 1))) for name, c in cols1.items()}
    off = per * np.arange(units, dtype=np.int64)
    ids = np.concatenate([[0, 1, 2], (np.array(ids1[3:], dtype=np.int64)[None, :] + off[:, None]).reshape(-1)])
    last = tuple(int(v) + per * (units - 1) for v in last1)
    return var.astype(np.uint32), cols, 3 + per * units, ids, last, tuple(last1), pts


def main_ecc(args, reps):
    from circuits import jj_add
    from pnp import abi
    from pnp_testlib import fr_mont, ints_to_arr
    import torch
    import pnp
    t0 = time.perf_counter()
    tpl = ecc_circuit(1)
    want, got = ecc_circuit(3), ecc_circuit(3, tpl)
    assert np.array_equal(want[0], got[0]) and want[2] == got[2] and list(want[3]) == list(got[3])
    assert all(np.array_equal(want[1][k], got[1][k]) for k in ECC_SELECTORS) and tuple(want[4]) == tuple(got[4])
    base, start = tpl[6]
    build_s = time.perf_counter() - t0
    if not torch.cuda.is_available():
        raise SystemExit("solve_time: no GPU (a measurement needs one; nothing is written)")
    to_int = lambda limbs: sum(int(w) << (64 * k) for k, w in enumerate(limbs))
    result = {"circuit": "K units: s = p + q, fixed_base_scalar_mul(s, B) over 255 rows, point_addition_gate(running "
                         "point, s B); composer layout", "inverse": args.inverse, "by_k": {}}
    for units in (1, 1024):
        var, cols, n_vars, ids, last, first_sum, _ = ecc_circuit(units, tpl)
        ng = var.shape[1]
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        rng = np.random.default_rng(args.seed)
        vals = [0, start[0], start[1]] + [int.from_bytes(rng.bytes(32), "little") >> 4 for _ in range(len(ids) - 3)]
        inputs = ints_to_arr([fr_mont(v) for v in vals])
        desc = abi.CircuitDesc(n_gates=ng, n_vars=n_vars, lookup_len=0)
        var = np.ascontiguousarray(var)
        for j in range(4):
            desc.var[j] = var[j].ctypes.data_as(abi.U32P)
        for k, name in enumerate(abi.DESC_SELECTORS):
            if name in cols and cols[name].any():
                desc.sel[k] = cols[name].ctypes.data_as(abi.U64P)
        ctx = pnp.Context(0)
        ctx.preprocess(desc, device_ptrs=False)
        plan_s, infos = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            rc, info = ctx.load_solve_plan_ecc(ids.ctypes.data, len(ids), 0, 0, 0,
                                               abi.SOLVE_FIXED_ADD | abi.SOLVE_VAR_ADD, False)
            plan_s.append(time.perf_counter() - t0)
            if rc != 0:
                raise SystemExit(f"solve_time: no plan: {ctx.last_error()}")
            infos.append(bytes(info))
        if len(set(infos)) != 1 or info.n_solved + info.n_inputs != n_vars:
            raise SystemExit("solve_time: the plan differs between builds, or does not cover every variable")
        n_fixed, n_var = ctx.solve_ecc_entries()

        def solve():
            t0 = time.perf_counter()
            ctx.solve_assignment(inputs.ctypes.data, len(ids), False)
            return time.perf_counter() - t0, dict(ctx.stage_times())

        solve()
        ok, rep = ctx.check_solved([])
        if not ok:
            raise SystemExit(f"solve_time: the solution fails the check: {ctx.last_error()}")
        # the first unit's sum: start + (p + q) B by double and add
        k, acc, dbl = vals[3] + vals[4], (0, 1), base
        while k:
            if k & 1:
                acc = jj_add(acc, dbl)
            dbl, k = jj_add(dbl, dbl), k >> 1
        expect = jj_add(start, acc)
        got_pt = tuple(to_int(l) for l in ctx.assignment_values(ids=[int(v) for v in first_sum]))
        if got_pt != tuple(fr_mont(c) for c in expect):
            raise SystemExit("solve_time: the first unit's point is not Python's")
        runs = [solve() for _ in range(reps)]
        ctx.kernel_timing(True)
        solve()
        levels_ms, _ = ctx.kernel_stats("solve_levels")
        ctx.kernel_timing(False)
        ctx.close()
        result["by_k"][str(units)] = {
            "lg": max(4, int(ng).bit_length()), "n_gates": int(ng), "n_vars": int(n_vars),
            "n_inputs": int(info.n_inputs), "n_solved": int(info.n_solved), "n_levels": int(info.n_levels),
            "max_width": int(info.max_width),
            "defined": {"arithmetic": int(info.n_solved) - n_fixed - n_var, "fixed_add": int(n_fixed),
                        "var_add": int(n_var)},
            "plan_bytes": int(info.plan_bytes), "solution_passes_check_solved": True,
            "plan_build_ms_runs": [round(1e3 * x, 2) for x in plan_s], "plan_build_ms": round(1e3 * median(plan_s), 2),
            "solve_ms_runs": [round(1e3 * t, 3) for t, _ in runs], "solve_ms": round(1e3 * median([t for t, _ in runs]), 3),
            "levels_kernels_ms": round(levels_ms, 3), "reps": reps,
        }
    result["host_build_s"] = round(build_s, 2)
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    out[args.inverse] = result
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


LOOKUP_SELECTORS = ("q_l", "q_r", "q_o", "q_c", "q_arith", "q_lookup")


def palette_rows(codes, values):
    """(len(codes), 4) u64 Montgomery rows: values[codes[i]] for every i."""
    from pnp_testlib import fr_mont, ints_to_arr
    return np.ascontiguousarray(ints_to_arr([fr_mont(v) for v in values])[np.asarray(codes, dtype=np.int64)])


def lookup_circuit(shape_, units, composer=False):
    """(var (4, n_gates) u32, {selector: codes into (0, 1, -1)}, n_vars, input ids, the z ids): the wide
    shape (units of p, q, r, s, x = p + q, y = r + s, z) or the deep one (z_0, then b_k, z_(k+1) a step);
    variable 1 is the constant -1 of row 0.  composer: from tests/lookup_circuits.py, for the comparison."""
    if composer:
        from circuits import Composer
        from ecc_circuits import constrain_to_constant
        from gate_circuits import M1
        from lookup_circuits import lookup_of, xor_table
        from test_preprocess_ref import wire_map
        cp = Composer(1)
        cp.table = xor_table(8)
        m1 = cp.var(M1)
        constrain_to_constant(cp, m1, M1)
        ids, zs = [0], []
        z = None
        if shape_ == "deep":
            z = cp.var(0)
            ids.append(z)
        for _ in range(units):
            if shape_ == "wide":
                p, q, r, s = (cp.var(0) for _ in range(4))
                x, y = cp.var(0), cp.var(0)
                cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, p, q, x, 0)
                cp.row({"q_arith": 1, "q_l": 1, "q_r": 1, "q_o": M1}, r, s, y, 0)
                ids += [p, q, r, s]
                zs.append(lookup_of(cp, x, y, m1)[1])
            else:
                b = cp.var(0)
                ids.append(b)
                z = lookup_of(cp, z, b, m1)[1]
                zs.append(z)
        code = {0: 0, 1: 1, M1: 2}
        cols = {name: np.array([code[r[0].get(name, 0)] for r in cp.rows]) for name in LOOKUP_SELECTORS}
        return wire_map(cp), cols, len(cp.vals), ids, zs
    k = np.arange(units, dtype=np.int64)
    if shape_ == "wide":
        b = 2 + 7 * k  # p, q, r, s, x, y, z
        one = np.ones(units, dtype=np.int64)
        rows = np.stack([np.stack([b, b + 1, b + 4, 0 * k]), np.stack([b + 2, b + 3, b + 5, 0 * k]),
                         np.stack([b + 4, b + 5, b + 6, one])], axis=2).reshape(4, -1)  # (4, units, 3) -> unit-major
        arith = np.tile([1, 1, 0], units)
        ids = np.concatenate([[0], (b[:, None] + np.arange(4)[None, :]).reshape(-1)])
        n_vars, zs = 2 + 7 * units, b + 6
    else:
        z = 2 + 2 * k  # z_k; b_k = z_k + 1; z_(k+1) = z_k + 2
        rows = np.stack([z, z + 1, z + 2, np.ones(units, dtype=np.int64)])
        arith = np.zeros(units, dtype=np.int64)
        ids = np.concatenate([[0, 2], z + 1])
        n_vars, zs = 3 + 2 * units, z + 2
    var = np.concatenate([np.array([[1], [0], [0], [0]]), rows], axis=1).astype(np.uint32)
    arith = np.concatenate([[1], arith])
    cols = {"q_arith": arith, "q_l": arith.copy(), "q_r": np.concatenate([[0], arith[1:]]),
            "q_o": 2 * np.concatenate([[0], arith[1:]]), "q_c": np.concatenate([[1], 0 * arith[1:]]),
            "q_lookup": 1 - arith}
    return var, cols, n_vars, ids, zs


def main_lookup(args, reps):
    from pnp import abi
    from pnp_testlib import R_MOD
    import torch
    import pnp
    t0 = time.perf_counter()
    for shape_ in ("wide", "deep"):
        want, got = lookup_circuit(shape_, 3, composer=True), lookup_circuit(shape_, 3)
        assert np.array_equal(want[0], got[0]) and want[2] == got[2] and list(want[3]) == list(got[3])
        assert all(np.array_equal(want[1][k], got[1][k]) for k in LOOKUP_SELECTORS) and list(want[4]) == list(got[4])
    byte = np.arange(256, dtype=np.int64)
    a, b = np.repeat(byte, 256), np.tile(byte, 256)
    pal = list(range(256)) + [R_MOD - 1]
    table = [palette_rows(c, pal) for c in (a, b, a ^ b, np.full(65536, 256))]
    build_s = time.perf_counter() - t0
    if not torch.cuda.is_available():
        raise SystemExit("solve_time: no GPU (a measurement needs one; nothing is written)")
    to_int = lambda limbs: sum(int(w) << (64 * k) for k, w in enumerate(limbs))
    result = {"table": "xor_table(0, 8): 65,536 rows (a, b, a ^ b, -1)", "shapes": {}}
    for shape_, units in (("wide", ((1 << 20) - 2) // 3), ("deep", 4096)):
        var, codes, n_vars, ids, zs = lookup_circuit(shape_, units)
        ng = var.shape[1]
        cols = {name: palette_rows(c, (0, 1, R_MOD - 1)) for name, c in codes.items()}
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        rng = np.random.default_rng(args.seed)
        vals = np.concatenate([[0], rng.integers(0, 128 if shape_ == "wide" else 256, size=len(ids) - 1)])
        inputs = palette_rows(vals, pal)
        if shape_ == "wide":
            v4 = vals[1:].reshape(-1, 4)
            expect = (v4[:, 0] + v4[:, 1]) ^ (v4[:, 2] + v4[:, 3])
        else:
            expect = np.bitwise_xor.accumulate(vals[1:])[1:]
        desc = abi.CircuitDesc(n_gates=ng, n_vars=n_vars, lookup_len=65536)
        var = np.ascontiguousarray(var)
        for j in range(4):
            desc.var[j] = var[j].ctypes.data_as(abi.U32P)
            desc.table[j] = table[j].ctypes.data_as(abi.U64P)
        for k, name in enumerate(abi.DESC_SELECTORS):
            if name in cols:
                desc.sel[k] = cols[name].ctypes.data_as(abi.U64P)
        ctx = pnp.Context(0)
        ctx.preprocess(desc, device_ptrs=False)
        plan_s, infos = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            rc, info = ctx.load_solve_plan_lookup(ids.ctypes.data, len(ids), 0, 0, 0, 0, abi.SOLVE_LOOKUP, False)
            plan_s.append(time.perf_counter() - t0)
            if rc != 0:
                raise SystemExit(f"solve_time: no plan: {ctx.last_error()}")
            infos.append(bytes(info))
        if len(set(infos)) != 1 or info.n_solved + info.n_inputs != n_vars:
            raise SystemExit("solve_time: the plan differs between builds, or does not cover every variable")
        n_lookup, n_indexed = ctx.solve_lookup_entries()

        def solve():
            t0 = time.perf_counter()
            ctx.solve_assignment(inputs.ctypes.data, len(ids), False)
            return time.perf_counter() - t0, dict(ctx.stage_times())

        solve()
        ok, rep = ctx.check_solved([])
        if not ok:
            raise SystemExit(f"solve_time: the solution fails the check: {ctx.last_error()}")
        probe = sorted(set(range(0, units, max(1, units // 64))) | {units - 1})
        got_z = [to_int(l) for l in ctx.assignment_values(ids=[int(zs[k]) for k in probe])]
        if got_z != [to_int(palette_rows([int(expect[k])], pal)[0]) for k in probe]:
            raise SystemExit("solve_time: the solved XORs are not Python's")
        runs = [solve() for _ in range(reps)]
        ctx.kernel_timing(True)
        solve()
        levels_ms, _ = ctx.kernel_stats("solve_levels")
        ctx.kernel_timing(False)
        ctx.close()
        result["shapes"][shape_] = {
            "lookups": int(units), "lg": int(max(ng, 65536) - 1).bit_length(), "n_gates": int(ng), "n_vars": int(n_vars),
            "n_inputs": int(info.n_inputs), "n_solved": int(info.n_solved), "n_levels": int(info.n_levels),
            "max_width": int(info.max_width),
            "defined": {"arithmetic": int(info.n_solved) - int(n_lookup), "lookup": int(n_lookup)},
            "indexed_table_rows": int(n_indexed), "plan_bytes": int(info.plan_bytes),
            "layout_reproduces_the_composer": True, "solution_passes_check_solved": True, "xors_probed": len(probe),
            "plan_build_ms_runs": [round(1e3 * x, 2) for x in plan_s], "plan_build_ms": round(1e3 * median(plan_s), 2),
            "solve_ms_runs": [round(1e3 * t, 3) for t, _ in runs], "solve_ms": round(1e3 * median([t for t, _ in runs]), 3),
            "levels_kernels_ms": round(levels_ms, 3), "reps": reps,
        }
    result["host_build_s"] = round(build_s, 2)
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    out["lookup"] = result
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=15)
    ap.add_argument("--outputs", action="store_true",
                    help="the root row as an output of the plan, beside the present path (PI given)")
    ap.add_argument("--gates", action="store_true",
                    help="range and logic rows that define: a synthetic circuit of range checks and XORs on 2^lg")
    ap.add_argument("--lg", type=int, default=20, help="--gates: the domain")
    ap.add_argument("--ecc", action="store_true",
                    help="fixed-base and curve-addition rows that define: K 255-bit multiplications, K = 1 and 1024")
    ap.add_argument("--inverse", default="binary", choices=["binary", "fermat"],
                    help="--ecc: the inversion the loaded library was built with (the key the result is filed under)")
    ap.add_argument("--lookup", action="store_true",
                    help="lookup rows that define: byte XORs through a table, a wide shape and a deep chain")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = max(args.reps, 5)
    if args.out is None:
        name = ("solve_lookup_time.json" if args.lookup else "solve_ecc_time.json" if args.ecc else "solve_gates_time.json" if args.gates
                else "solve_outputs_time.json" if args.outputs else "solve_time.json")
        args.out = os.path.join(REPO, "profiles", name)
    if args.lookup:
        return main_lookup(args, reps)
    if args.ecc:
        return main_ecc(args, reps)
    if args.gates:
        return main_gates(args, reps)
    if args.outputs:
        return main_outputs(args, reps)

    from pnp import abi
    from pnp_testlib import R_MOD, fr_mont
    r = setup(args, with_root=True)
    ctx, ids, inputs, n_vars, root, root_var = r.ctx, r.ids, r.inputs, r.n_vars, r.root, r.root_var
    height, ng, D, build_s, cpu_tree_s, preprocess_s = r.height, r.ng, r.D, r.build_s, r.cpu_tree_s, r.preprocess_s
    pis = [(ng - 1, -root % R_MOD)]

    plan_s, infos = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        rc, info = ctx.load_solve_inputs(ids.ctypes.data, len(ids), False)
        plan_s.append(time.perf_counter() - t0)
        if rc != 0:
            raise SystemExit(f"solve_time: no plan: {ctx.last_error()}")
        infos.append(bytes(info))
    if len(set(infos)) != 1 or info.n_solved + info.n_inputs != n_vars:
        raise SystemExit("solve_time: the plan differs between builds, or does not cover every variable")

    def solve():
        t0 = time.perf_counter()
        ctx.solve_assignment(inputs.ctypes.data, len(ids), False, pis)
        return time.perf_counter() - t0, dict(ctx.stage_times())

    solve()
    addr, n = ctx.assignment_ptr()
    ok, rep = ctx.check_assignment(addr, n_vars, True, pis)
    if not ok:
        raise SystemExit(f"solve_time: the solution fails the check: {ctx.last_error()}")
    (limbs,) = ctx.assignment_values(ids=[root_var])
    if sum(int(w) << (64 * k) for k, w in enumerate(limbs)) != fr_mont(root):
        raise SystemExit("solve_time: the solution's root is not the CPU tree's")
    host_values = np.zeros((n_vars, 4), dtype=np.uint64)
    if ctx.lib.pnp_assignment_values(ctx.h, None, n_vars, host_values.ctypes.data) != 0:
        raise SystemExit("solve_time: " + ctx.last_error())

    def solve_and_prove():
        t0 = time.perf_counter()
        ctx.solve_assignment(inputs.ctypes.data, len(ids), False, pis)
        st = dict(ctx.stage_times())
        addr, n = ctx.assignment_ptr()
        p = ctx.prove_assignment(addr, n, True, pis)
        return abi.proof_to_bytes(p), time.perf_counter() - t0, st

    def upload_and_prove():
        t0 = time.perf_counter()
        p = ctx.prove_assignment(host_values.ctypes.data, n_vars, False, pis)
        return abi.proof_to_bytes(p), time.perf_counter() - t0, dict(ctx.stage_times())

    # warm-up: the first proof goes without the context's tables, which are then
    # built in the background (pnp_sync waits for them); one more of each path
    ref, _, _ = upload_and_prove()
    ctx.sync()
    proofs = [solve_and_prove()[0], upload_and_prove()[0]]
    ctx.sync()
    runs = {"solve_and_prove": [], "upload_and_prove": []}
    solve_stages = []
    for _ in range(reps):
        proof, wall, st = solve_and_prove()
        proofs.append(proof)
        runs["solve_and_prove"].append(wall)
        solve_stages.append(st)
        proof, wall, _ = upload_and_prove()
        proofs.append(proof)
        runs["upload_and_prove"].append(wall)
    solve_alone = [solve()[0] for _ in range(reps)]
    all_equal = all(p == ref for p in proofs)
    # the level kernels' own time: one more solve with the event timers on
    ctx.kernel_timing(True)
    solve()
    levels_ms, _ = ctx.kernel_stats("solve_levels")
    levels_bytes = ctx.kernel_bytes("solve_levels")
    ctx.kernel_timing(False)
    hbm = ctx.hbm_usage()["live"]
    ctx.close()

    med = {k: median(v) for k, v in runs.items()}
    out = {
        "height": height, "lg": D.bit_length() - 1, "n_gates": ng, "n_vars": n_vars, "n_inputs": int(info.n_inputs),
        "n_solved": int(info.n_solved), "n_levels": int(info.n_levels), "max_width": int(info.max_width),
        "plan_bytes": int(info.plan_bytes), "inputs_bytes": int(inputs.nbytes), "assignment_bytes": 32 * n_vars,
        "tiling_reproduces_merkle_circuit_6": True, "solution_passes_check_assignment": True,
        "solution_root_equals_cpu_tree": True, "plan_same_on_every_build": True,
        "plan_build_s_runs": [round(x, 4) for x in plan_s], "plan_build_s": round(median(plan_s), 4),
        "solve_s_runs": [round(x, 5) for x in solve_alone], "solve_s": round(median(solve_alone), 5),
        "solve_stage_ms_median": {k: round(median([st[k] for st in solve_stages]), 4)
                                  for k in ("solve_inputs", "solve_levels")},
        "levels_kernels_ms": round(levels_ms, 4), "levels_kernels_bytes": int(levels_bytes),
        "levels_kernels_gb_s": round(levels_bytes / (levels_ms * 1e-3) / 1e9, 1) if levels_ms > 0 else None,
        "reps_each": reps, "interleaved": True, "all_proofs_equal": bool(all_equal), "proofs_compared": len(proofs) + 1,
        "median_s": {k: round(v, 5) for k, v in med.items()},
        "wall_s_runs": {k: [round(x, 5) for x in v] for k, v in runs.items()},
        "solve_and_prove_over_upload_and_prove": round(med["solve_and_prove"] / med["upload_and_prove"], 4),
        "hbm_live_bytes_at_end": int(hbm),
        "host_side_s": {"build_instance": round(build_s, 2), "cpu_poseidon_tree": round(cpu_tree_s, 2),
                        "preprocess": round(preprocess_s, 3)},
    }
    if not all_equal:
        raise SystemExit("solve_time: the proofs differ")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
