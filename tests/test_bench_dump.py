"""bench.py --dump-outputs, CPU: a ProofC goes out as float32 arrays, one
value per byte, that give the proof's bytes back exactly; the writer refuses
more than its size limit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from pnp import abi  # noqa: E402
import bench  # noqa: E402


def _proof(seed):
    raw = np.random.default_rng(seed).integers(0, 256, size=C.sizeof(abi.ProofC), dtype=np.uint8).tobytes()
    return abi.ProofC.from_buffer_copy(raw), raw


def test_proof_arrays_round_trip(tmp_path):
    proof, raw = _proof(5)
    arrays = bench.proof_arrays(proof)
    assert arrays["commitments"].shape == (len(abi.PROOF_COMMITMENTS), 96)
    assert arrays["evaluations"].shape == (26, 32)
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    got = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in ("commitments", "evaluations")}
    assert all(a.dtype == np.float32 for a in got.values())
    back = b"".join(got[n].astype(np.uint8).tobytes() for n in ("commitments", "evaluations"))
    assert back == raw
    # a commitment's row is its x then y limbs, as CommitmentC lays them out
    assert got["commitments"][4].astype(np.uint8).tobytes() == bytes(proof.z_comm.x) + bytes(proof.z_comm.y)


def test_dump_refuses_over_the_limit(tmp_path):
    big = np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, dtype=np.float32)
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "big"), {"x": big})
    assert not (tmp_path / "big" / "x.npy").exists()
