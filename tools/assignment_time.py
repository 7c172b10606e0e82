#!/usr/bin/env python3
"""Time proofs from a host variable assignment against proofs from host
witness columns at the bench's size (one GPU process; run it once, under a
timeout of its own):

    timeout -k 10 900 python tools/assignment_time.py [--lg 22] [--out profiles/assignment_h15.json]

The instance is built the way tools/preprocess_time.py builds its own: the
HEIGHT = 15 Merkle circuit's shape (n_gates = 3,161,924 on D = 2^22) with a
seeded wire map, here one a witness satisfies, so that the proofs take the
prover's usual path (a quotient on 6 coset blocks).  Like the Merkle circuit's
rows (an affine map of three state wires into a fresh output wire), gate i is
a + b + d - c = 0 with c a fresh variable; the rows come in layers, the inputs
of a layer are outputs of the layer before at nearby rows (composer-built
circuits keep the ids of neighbouring rows close), a quarter of the input slots
hold variable 0 (the Merkle circuit's zero_var).  Every variable but the first
layer's inputs is used about three times as an input and once as an output, so
n_vars is about n_gates.

pnp_preprocess builds the key and leaves the wire map resident.  After the
warm-up (the first proofs build the context's tables) proofs from the four
host columns and q_lookup (pnp_prove_ex) alternate with proofs from the host
assignment (pnp_prove_assignment), --reps of each; all must be the same bytes.
Writes both medians, n_vars, the bytes uploaded per proof on either path, the
`inputs` stage of either path and the gather kernel's own time (HIP events,
one extra proof with pnp_kernel_timing on)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "zprize23-gpu-submission_amd"), os.path.join(REPO, "tests")]

R_MOD = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
R_FR = pow(2, 256, R_MOD)
LAYERS = 16
WINDOW = 32  # an input comes from at most this many rows away in the layer before


def limbs32(x: int) -> np.ndarray:
    return np.array([(x >> (32 * k)) & 0xFFFFFFFF for k in range(8)], dtype=np.uint64)


def add_mod(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """(x + y) mod r on (N, 4) u64 limb arrays of residues < r (any form:
    Montgomery addition is plain addition), in 32-bit limbs held in u64 lanes."""
    s = x.view(np.uint32).astype(np.uint64) + y.view(np.uint32).astype(np.uint64)  # (N, 8)
    mask = np.uint64(0xFFFFFFFF)
    c = np.zeros(len(s), dtype=np.uint64)
    for k in range(8):
        s[:, k] += c
        c = s[:, k] >> np.uint64(32)
        s[:, k] &= mask
    assert not c.any()  # x, y < r < 2^255
    r = limbs32(R_MOD)
    ge = np.ones(len(s), dtype=bool)  # s >= r, decided from the top limb down
    decided = np.zeros(len(s), dtype=bool)
    for k in range(7, -1, -1):
        gt, lt = s[:, k] > r[k], s[:, k] < r[k]
        ge = np.where(~decided & lt, False, ge)
        decided |= gt | lt
    borrow = np.zeros(len(s), dtype=np.uint64)
    d = s.copy()
    for k in range(8):
        t = d[:, k] + np.uint64(1 << 32) - r[k] - borrow
        borrow = np.uint64(1) - (t >> np.uint64(32))
        d[:, k] = t & mask
    s[ge] = d[ge]
    return np.ascontiguousarray(s.astype(np.uint32)).view(np.uint64).reshape(-1, 4)


def random_fr(rng, n):
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(2)  # < 2^254 < r: a valid residue
    return a


def build_instance(n_gates: int, seed: int):
    """(var (4, n_gates) u32, values (n_vars, 4) u64 Montgomery) of the layered
    circuit c = a + b + d: variable 0 is zero, then the first layer's inputs,
    then the output of gate i as variable n_in + 1 + i."""
    rng = np.random.default_rng(seed)
    per = (n_gates + LAYERS - 1) // LAYERS
    n_in = per
    n_vars = 1 + n_in + n_gates
    values = np.zeros((n_vars, 4), dtype=np.uint64)
    values[1:1 + n_in] = random_fr(rng, n_in)
    var = np.zeros((4, n_gates), dtype=np.uint32)
    var[2] = np.arange(1 + n_in, n_vars, dtype=np.uint32)
    lo_prev, cnt_prev = 1, n_in  # ids of the layer before
    for lo in range(0, n_gates, per):
        cnt = min(per, n_gates - lo)
        pos = np.arange(cnt, dtype=np.int64)
        for j in (0, 1, 3):
            src = (pos + rng.integers(-WINDOW, WINDOW + 1, size=cnt)) % cnt_prev + lo_prev
            src[rng.random(cnt) < 0.25] = 0
            var[j, lo:lo + cnt] = src.astype(np.uint32)
        a, b, d = (values[var[j, lo:lo + cnt].astype(np.int64)] for j in (0, 1, 3))
        values[1 + n_in + lo:1 + n_in + lo + cnt] = add_mod(add_mod(a, b), d)
        lo_prev, cnt_prev = 1 + n_in + lo, cnt
    return var, values


def const_column(v: int, n: int) -> np.ndarray:
    m = v * R_FR % R_MOD
    return np.tile(np.array([(m >> (64 * k)) & (2**64 - 1) for k in range(4)], dtype=np.uint64), (n, 1))


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=22)
    ap.add_argument("--gates", type=int, default=0, help="default: 3,161,924 scaled to the domain")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "assignment_h15.json"))
    args = ap.parse_args()
    D = 1 << args.lg
    n_gates = args.gates or (3161924 if args.lg == 22 else max(LAYERS, (D * 3161924) >> 22))
    reps = max(args.reps, 5)

    import torch
    import pnp
    from pnp import abi

    if not torch.cuda.is_available():
        raise SystemExit("assignment_time: no GPU (a measurement needs one; nothing is written)")
    t0 = time.perf_counter()
    var, values = build_instance(n_gates, args.seed)
    n_vars = values.shape[0]
    # the columns a host expands for pnp_prove_ex: values through the wire map
    t1 = time.perf_counter()
    cols = [np.ascontiguousarray(values[var[j].astype(np.int64)]) for j in range(4)]
    expand_s = time.perf_counter() - t1
    q_lookup = np.zeros((n_gates, 4), dtype=np.uint64)
    # a spot check of the instance in Python integers: c = a + b + d
    for i in (0, n_gates // 3, n_gates - 1):
        ints = [sum(int(cols[j][i, k]) << (64 * k) for k in range(4)) for j in range(4)]
        assert (ints[0] + ints[1] + ints[3] - ints[2]) % R_MOD == 0, i
    build_s = time.perf_counter() - t0

    sel = {"q_l": const_column(1, n_gates), "q_r": const_column(1, n_gates), "q_4": const_column(1, n_gates),
           "q_o": const_column(R_MOD - 1, n_gates), "q_arith": const_column(1, n_gates)}
    desc = abi.CircuitDesc(n_gates=n_gates, n_vars=n_vars, lookup_len=0)
    for j in range(4):
        desc.var[j] = var[j].ctypes.data_as(abi.U32P)
    for k, name in enumerate(abi.DESC_SELECTORS):
        if name in sel:
            desc.sel[k] = sel[name].ctypes.data_as(abi.U64P)
    circuit = abi.CircuitC(n=n_gates, lookup_len=0, intended_pi_pos=0, q_lookup=abi.ptr(q_lookup.ctypes.data),
                           pi=None, w_l=abi.ptr(cols[0].ctypes.data), w_r=abi.ptr(cols[1].ctypes.data),
                           w_o=abi.ptr(cols[2].ctypes.data), w_4=abi.ptr(cols[3].ctypes.data))
    pis = [(0, 0)]  # no public input (a zero value is dropped)

    ctx = pnp.Context(0)
    srs = torch.zeros((D, 12), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.srs(srs.data_ptr(), D, [5, 0, 0, 0])
    ctx.sync()
    ck = abi.CommitKeyC(powers_of_g=abi.ptr(srs.data_ptr()), powers_of_gamma_g=abi.ptr(srs.data_ptr()))
    ctx.load_commit_key(ck, D, device_ptrs=True)
    t0 = time.perf_counter()
    ctx.preprocess(desc, device_ptrs=False)
    preprocess_s = time.perf_counter() - t0

    def from_columns():
        t0 = time.perf_counter()
        p = ctx.prove_ex(circuit, False, pis)
        return abi.proof_to_bytes(p), time.perf_counter() - t0, dict(ctx.stage_times())

    def from_assignment():
        t0 = time.perf_counter()
        p = ctx.prove_assignment(values.ctypes.data, n_vars, False, pis)
        return abi.proof_to_bytes(p), time.perf_counter() - t0, dict(ctx.stage_times())

    # warm-up: the first proof goes without the context's tables, which are then
    # built in the background (pnp_sync waits for them); one more of each path
    ref, _, _ = from_columns()
    ctx.sync()
    proofs = [from_columns()[0], from_assignment()[0]]
    ctx.sync()
    runs = {"columns": [], "assignment": []}
    for _ in range(reps):
        for name, fn in (("columns", from_columns), ("assignment", from_assignment)):
            proof, wall, st = fn()
            proofs.append(proof)
            runs[name].append({"wall_s": wall, "inputs_ms": st["inputs"],
                               "h2d_bytes": int(st.get("inputs_h2d_bytes", 5 * 32 * n_gates))})
    all_equal = all(p == ref for p in proofs)
    # the gather kernel's own time: one more proof with the event timers on
    ctx.kernel_timing(True)
    proof, _, _ = from_assignment()
    ctx.sync()
    gather_ms, gather_launches = ctx.kernel_stats("gather_witness")
    ctx.kernel_timing(False)
    all_equal = all_equal and proof == ref
    ctx.close()

    med = {k: median([r["wall_s"] for r in v]) for k, v in runs.items()}
    out = {
        "lg": args.lg, "n_gates": n_gates, "n_vars": n_vars, "n_vars_per_gate": round(n_vars / n_gates, 4),
        "reps_each": reps, "interleaved": True, "all_proofs_equal": bool(all_equal),
        "proofs_compared": len(proofs) + 1,
        "median_s": {k: round(v, 5) for k, v in med.items()},
        "wall_s_runs": {k: [round(r["wall_s"], 5) for r in v] for k, v in runs.items()},
        "inputs_stage_ms_median": {k: round(median([r["inputs_ms"] for r in v]), 3) for k, v in runs.items()},
        "uploaded_bytes_per_proof": {k: v[0]["h2d_bytes"] for k, v in runs.items()},
        "gather_kernel_ms": round(gather_ms, 4), "gather_kernel_launches": gather_launches,
        "gather_bytes_moved": int(16 * n_gates + 4 * 32 * n_gates + 4 * 32 * D),
        "assignment_not_above_columns": bool(med["assignment"] <= med["columns"]),
        "host_side_s": {"build_instance": round(build_s, 3), "expand_columns_numpy": round(expand_s, 3),
                        "preprocess": round(preprocess_s, 3)},
        "instance": f"{LAYERS} layers of gates a + b + d - c = 0, inputs within {WINDOW} rows, 1/4 of them variable 0",
    }
    if not all_equal:
        raise SystemExit("assignment_time: the proofs differ")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
