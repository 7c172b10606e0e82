"""The folded subtractions of csrc/field30s.cuh on the device, run alone.

tests/native/dev_arith_fold.hip (built by csrc/Makefile into lib/dev_arith_fold)
runs mul30s_sub and sqr30s_sub2 one lane per case, one launch each, on the whole
case list of tests/test_field30s_fold.py (the operand extremes, the subtrahend
limbs at +-2^29 with limb 12 at +-2^24, 1,000 random operands).  Every result
limb is compared with the Python model, which that file shows equal to the
renormalised subtraction of the product, and with plain integers.  The harness
and the file format are test_gpu_dev_arith's."""
import os
import subprocess

import pytest

import test_field30s as m30
import test_field30s_fold as fold
import test_gpu_dev_arith as da

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zprize23-gpu-submission_amd", "csrc")
BIN = os.path.join(HERE, "..", "zprize23-gpu-submission_amd", "lib", "dev_arith_fold")
Q, H = m30.Q, m30.H


def _props(name):
    def props(w, out):
        v = [m30.val(da.dec30(x)) for x in da.split(w, 13)]
        r = da.dec30(out)
        assert da.bal_ok(r)
        want = v[0] * v[1] * da.IR390 - v[2] if name == "mul30s_sub" else v[0] * v[0] * da.IR390 - v[1] - 2 * v[2]
        assert (m30.val(r) - want) % Q == 0
    return props


def suite():
    ops = {}
    for oid, name in ((1, "mul30s_sub"), (2, "sqr30s_sub2")):
        op = da.Op("field30s", name, oid, 39, 13, None, _props(name))
        for tag, *operands in fold.cases()[name]:
            op.add(tag, *operands)
        ops[name] = op
    return ops


def test_cases_hold_on_cpu():
    ops = suite()
    want = {name: [da.enc(r) for r in fold.expected()[name]] for name in ops}
    assert all(len(op.cases) >= 1121 for op in ops.values())
    assert da.failures(ops, want, want) == []  # the model alone meets the integers
    flat = da.array("I", [x for name in ops for e in want[name] for x in e]).tobytes()
    assert da.unpack_out(flat, ops) == want


@pytest.mark.gpu
def test_fold_device(tmp_path):
    ops = suite()
    if not os.path.exists(BIN):
        r = subprocess.run(["make", "-C", CSRC, "../lib/dev_arith_fold"], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and os.path.exists(BIN), f"lib/dev_arith_fold is missing and does not build:\n{r.stderr[-2000:]}"
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(fin, "wb") as f:
        f.write(da.pack(ops))
    r = subprocess.run([BIN, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"dev_arith_fold exited with {r.returncode}:\n{r.stderr[-2000:]}"
    with open(fout, "rb") as f:
        got = da.unpack_out(f.read(), ops)
    want = {name: [da.enc(x) for x in fold.expected()[name]] for name in ops}
    bad = da.failures(ops, got, want)
    assert not bad, f"{len(bad)} cases fail, the first: {bad[:8]}"
