#!/usr/bin/env python3
"""Time pnp_preprocess at the bench's size (one GPU process; run it once,
under a timeout of its own):

    timeout -k 10 900 python tools/preprocess_time.py [--lg 22] [--out profiles/preprocess_2e22.json]

n_gates = 3,161,924 on D = 2^22 (the HEIGHT = 15 Merkle circuit's shape), ten
non-zero selector columns of random field elements, a seeded wire map with a
quarter of all slots on variable 0 (the Merkle circuit's zero_var) and the rest
on variables used two to four times.  Preprocessing needs no satisfying
witness, so none is made.

Checks `next` (pnp_wire_sigma on the same wire map) against the numpy
reference of tests/test_preprocess_ref.py, then times pnp_wire_sigma alone
(warm-up, then --reps synchronous calls) and pnp_preprocess with the verifier
key (warm-up call, then --reps calls; per-stage host clocks between stream
synchronisations, pnp_last_stage_times).  Writes the per-stage milliseconds,
the PCIe bytes and the permutation's achieved bytes per second beside the
bytes its passes must move."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "zprize23-gpu-submission_amd"), os.path.join(REPO, "tests")]

NONZERO_SELECTORS = ("q_l", "q_r", "q_o", "q_4", "q_c", "q_hl", "q_hr", "q_h4", "q_arith", "q_m")


def wire_map(n_gates: int, seed: int):
    """(4, n_gates) u32 ids and n_vars: ~1/4 of the slots hold variable 0, the
    others variables used 2, 3 or 4 times, in random places."""
    rng = np.random.default_rng(seed)
    m = 4 * n_gates
    zero = rng.random(m) < 0.25
    rest = int(m - zero.sum())
    mult = rng.integers(2, 5, size=rest // 2 + 1)
    cut = int(np.searchsorted(np.cumsum(mult), rest, side="left")) + 1
    ids = np.repeat(np.arange(1, cut + 1, dtype=np.uint32), mult[:cut])[:rest]
    rng.shuffle(ids)
    flat = np.zeros(m, dtype=np.uint32)
    flat[~zero] = ids
    n_vars = int(flat.max()) + 1
    return np.ascontiguousarray(flat.reshape(n_gates, 4).T), n_vars


def random_fr(rng, n):
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(2)  # < 2^254 < r: a valid Montgomery residue
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=22)
    ap.add_argument("--gates", type=int, default=0, help="default: 3,161,924 scaled to the domain")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "preprocess_2e22.json"))
    args = ap.parse_args()
    D = 1 << args.lg
    n_gates = args.gates or (3161924 if args.lg == 22 else max(1, (D * 3161924) >> 22))

    import torch
    import pnp
    from pnp import abi
    from test_preprocess_ref import next_ref

    if not torch.cuda.is_available():
        raise SystemExit("preprocess_time: no GPU (a measurement needs one; nothing is written)")
    rng = np.random.default_rng(args.seed)
    var, n_vars = wire_map(n_gates, args.seed)
    t0 = time.perf_counter()
    exp_next = next_ref(var, D)
    numpy_ref_s = time.perf_counter() - t0
    sel = {name: random_fr(rng, n_gates) for name in NONZERO_SELECTORS}
    desc = abi.CircuitDesc(n_gates=n_gates, n_vars=n_vars, lookup_len=0)
    for j in range(4):
        desc.var[j] = var[j].ctypes.data_as(abi.U32P)
    for k, name in enumerate(abi.DESC_SELECTORS):
        if name in sel:
            desc.sel[k] = sel[name].ctypes.data_as(abi.U64P)

    ctx = pnp.Context(0)
    srs = torch.zeros((D, 12), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.srs(srs.data_ptr(), D, [5, 0, 0, 0])
    ctx.sync()
    ck = abi.CommitKeyC(powers_of_g=abi.ptr(srs.data_ptr()), powers_of_gamma_g=abi.ptr(srs.data_ptr()))
    ctx.load_commit_key(ck, D, device_ptrs=True)

    # ---- the permutation alone, device pointers
    dv = [torch.from_numpy(var[j].view(np.int32)).to("cuda") for j in range(4)]
    nxt = torch.zeros(4 * D, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in dv]
    ctx.wire_sigma(ptrs, n_gates, n_vars, args.lg, nxt.data_ptr(), None)  # warm-up
    got = nxt.cpu().numpy().view(np.uint32)
    next_ok = bool(np.array_equal(got, exp_next))
    perm_ms = []
    for _ in range(max(args.reps, 3)):
        t0 = time.perf_counter()
        ctx.wire_sigma(ptrs, n_gates, n_vars, args.lg, nxt.data_ptr(), None)
        perm_ms.append(1e3 * (time.perf_counter() - t0))
    del dv, nxt

    # ---- pnp_preprocess, host pointers, verifier key
    runs = []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        vk = ctx.preprocess(desc, device_ptrs=False, want_vk=True)
        wall = 1e3 * (time.perf_counter() - t0)
        st = dict(ctx.stage_times())
        st["wall"] = wall
        if rep:  # the first call builds the NTT tables and the SRS table
            runs.append(st)
        else:
            cold = st
    names = ("pre_upload", "pre_permutation", "pre_intt", "pre_derive", "pre_vk", "wall")
    stages = {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in names}
    perm_bytes = runs[0]["pre_permutation_bytes"]
    bits = max(n_vars - 1, 0).bit_length()
    m = 4 * n_gates
    perm_best = min(perm_ms)
    out = {
        "lg": args.lg, "n_gates": n_gates, "n_vars": n_vars, "slots": m, "zero_var_share": float((var == 0).mean()),
        "nonzero_selectors": len(NONZERO_SELECTORS), "reps": args.reps,
        "next_equals_numpy": next_ok, "numpy_reference_s": round(numpy_ref_s, 3),
        "stage_ms_median": {k: round(v, 3) for k, v in stages.items()},
        "stage_ms_runs": [{k: round(r[k], 3) for k in names} for r in runs],
        "first_call_ms": {k: round(cold[k], 3) for k in names},
        "pcie_bytes": int(runs[0]["pre_h2d_bytes"]),
        "permutation": {
            "digit_passes": (bits + 7) // 8, "pairs_per_pass": m,
            "bytes_must_move": int(perm_bytes),
            "wire_sigma_ms": [round(v, 3) for v in perm_ms],
            "achieved_GBps": round(perm_bytes / (perm_best * 1e-3) / 1e9, 1),
        },
        "derive_vs_coeff_load": {
            "derive_ms": round(stages["pre_derive"], 3),
            "parent_coeff_load_s": "0.098-0.109 (profiles/key_coeffs_v2_load_2e22.json, upload included)",
        },
        "vk_infinity": [n for n, c in zip(abi.VK_POLYS, vk.polys) if not any(c.x)],
    }
    ctx.close()
    if not next_ok:
        raise SystemExit("preprocess_time: next differs from the numpy reference")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
