"""The launches of a solve, from the levels' widths alone.

pnp_load_solve_plan turns the plan's levels into launches with
SolvePlan::launch_runs (csrc/prover_key.h), a host function without a device
call: a level of more than 256 entries (a workgroup), arithmetic and gate
entries counted together, is a launch of its own, and consecutive narrower
levels share one.  tests/native/solve_runs.cpp calls it directly on the
widths given here; each run is (l0, l1, p0, p1, g0, g1, wide): the levels
[l0, l1), the arithmetic entries [p0, p1) and the gate entries [g0, g1).
The GPU tests of the solver cover the same function through the plan."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zprize23-gpu-submission_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# (levels as (arithmetic, gate) widths, the runs)
CASES = {
    "no levels": ([], []),
    "all narrow": ([(3, 0), (256, 0), (1, 0)], [(0, 3, 0, 260, 0, 0, 0)]),
    "one wide level": ([(257, 0)], [(0, 1, 0, 257, 0, 0, 1)]),
    "256 then 257 then 3": ([(256, 0), (257, 0), (3, 0)],
                            [(0, 1, 0, 256, 0, 0, 0), (1, 2, 256, 513, 0, 0, 1), (2, 3, 513, 516, 0, 0, 0)]),
    "wide only in sum": ([(200, 57)], [(0, 1, 0, 200, 0, 57, 1)]),
    "wide in sum between narrow": ([(5, 0), (200, 57), (200, 56), (1, 1)],
                                   [(0, 1, 0, 5, 0, 0, 0), (1, 2, 5, 205, 0, 57, 1), (2, 4, 205, 406, 57, 114, 0)]),
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("sr") / "solve_runs")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-Wall", "--offload-host-only", "-x", "hip", "-I", CSRC,
                    os.path.join(HERE, "native", "solve_runs.cpp"), "-o", out], check=True, timeout=300)
    return out


def test_launch_runs(exe):
    for name, (levels, runs) in CASES.items():
        args = ["%d+%d" % lv for lv in levels]
        out = subprocess.run([exe] + args, check=True, capture_output=True, text=True, timeout=60).stdout
        got = [tuple(int(x) for x in ln.split()) for ln in out.splitlines()]
        assert got == runs, name
