#!/usr/bin/env python3
"""Time the satisfiability check beside the proof at the bench's size (one GPU
process; run it once, under a timeout of its own):

    timeout -k 10 900 python tools/check_time.py [--lg 22] [--out profiles/check_time.json]

The instance and the key are bench.py's own (bench.Synthetic, seed 1: the
reference's Poseidon Merkle circuit from pnp_synth_merkle, HEIGHT = lg - 7, 15
at 2^22; the full key and the SRS adopted in HBM).  pnp_synth_merkle yields
columns and sigmas, not a wire map, so the check is the columns form
(pnp_check_witness on the HBM columns) and copy constraints are not checked
(copy_checked = 0).

After the warm-up (the first proof goes without the context's tables, which
are then built in the background) checks alternate with proofs (pnp_prove),
--reps of each: every check must say PNP_OK, every proof must be the same
bytes.  Writes both medians, the check's stages, and the row kernels' own time
(HIP events, one extra check with pnp_kernel_timing on) with the bytes they
must read and the GB/s that makes."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "zprize23-gpu-submission_amd"), os.path.join(REPO, "tests")]

CHECK_STAGES = ("check_inputs", "check_rows_ntt", "check_rows", "check_lookup", "check_copy")


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "check_time.json"))
    args = ap.parse_args()
    reps = max(args.reps, 5)

    import torch
    import bench
    import pnp
    from pnp import abi

    if not torch.cuda.is_available():
        raise SystemExit("check_time: no GPU (a measurement needs one; nothing is written)")
    ctx = pnp.Context(0)
    t0 = time.perf_counter()
    syn = bench.Synthetic(ctx, args.lg, bench.HEIGHT15_GATES, seed=1, circuit="merkle")
    ctx.load_prover_key(syn.pk, syn.n, device_ptrs=True)
    ctx.load_commit_key(syn.ck, syn.n, device_ptrs=True)
    setup_s = time.perf_counter() - t0
    pis = [(int(syn.cs.intended_pi_pos), sum(int(syn.pi[k]) << (64 * k) for k in range(4)))]

    def prove():
        t0 = time.perf_counter()
        p = ctx.prove(syn.cs, device_ptrs=True)
        return abi.proof_to_bytes(p), time.perf_counter() - t0

    def check():
        t0 = time.perf_counter()
        ok, rep = ctx.check_witness(syn.cs, True, pis)
        wall = time.perf_counter() - t0
        if not ok or rep.violations or rep.copy_checked != 0:
            raise SystemExit(f"check_time: the bench's witness fails the check: {ctx.last_error()}")
        return wall, dict(ctx.stage_times())

    ref, _ = prove()
    ctx.sync()
    check()
    proofs = [prove()[0]]
    ctx.sync()
    runs = {"check": [], "prove": []}
    stages = []
    for _ in range(reps):
        wall, st = check()
        runs["check"].append(wall)
        stages.append(st)
        proof, wall = prove()
        proofs.append(proof)
        runs["prove"].append(wall)
    # the witness without its public input must fail, at the row that carries it
    ok, rep = ctx.check_witness(syn.cs, True, [])
    refused = (not ok) and rep.first_row == syn.cs.intended_pi_pos and rep.violations == 1
    # the row kernels' own time: one more check with the event timers on
    ctx.kernel_timing(True)
    check()
    rows_ms, rows_launches = ctx.kernel_stats("check_rows")
    rows_bytes = ctx.kernel_bytes("check_rows")
    ctx.kernel_timing(False)
    proofs.append(prove()[0])
    all_equal = all(p == ref for p in proofs)
    ctx.close()

    med = {k: median(v) for k, v in runs.items()}
    stage_med = {name: round(median([st[name] for st in stages]), 4) for name in CHECK_STAGES}
    out = {
        "lg": args.lg, "height": syn.height, "n_gates": syn.gates, "reps_each": reps, "interleaved": True,
        "form": "columns (HBM pointers), one public input", "copy_checked": 0,
        "all_checks_ok": True, "witness_without_its_public_input_refused_at_its_row": bool(refused),
        "all_proofs_equal": bool(all_equal), "proofs_compared": len(proofs) + 1,
        "median_s": {k: round(v, 5) for k, v in med.items()},
        "wall_s_runs": {k: [round(x, 5) for x in v] for k, v in runs.items()},
        "check_over_prove": round(med["check"] / med["prove"], 4),
        "check_stage_ms_median": stage_med,
        "transforms_share_of_check": round(stage_med["check_rows_ntt"] / sum(stage_med.values()), 3),
        "rows_kernel_ms": round(rows_ms, 4), "rows_kernel_launches": rows_launches,
        "rows_kernel_bytes": int(rows_bytes),
        "rows_kernel_gb_s": round(rows_bytes / (rows_ms * 1e-3) / 1e9, 1) if rows_ms > 0 else None,
        "setup_s": round(setup_s, 1),
    }
    if not all_equal:
        raise SystemExit("check_time: the proofs differ")
    if not refused:
        raise SystemExit("check_time: the witness without its public input was not refused at its row")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
