"""The coset constants pnp_load_prover_key_coeffs writes into block layout,
on the host against Python integers, and the new entry point's CPU side.

csrc/coset_blocks.cuh holds the index map and the closed forms as host /
device functions; the key load's kernel (keyblocks.hip) and
tests/native/host_coset_blocks.cpp run the same source.  The program prints,
for lg_n in {3, 6}, every block m and every index j: the storage index and
lin, vh_inv, l1v in Montgomery form.  Here each line is compared exactly with
  point i = 8 j + m of the coset g w_8n^i (g = 7), stored at m n + brev(j),
  lin = g w_8n^i,  vh_inv = (lin^n - 1)^-1,  l1v = (n (lin - 1))^-1.
The GPU tests (test_gpu_key_coeffs.py) cover the same code end to end."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from pnp_testlib import FR_GEN, R_MOD, fr_mont, fr_root

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zprize23-gpu-submission_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("cb") / "host_coset_blocks")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-host-only", "-x", "hip", "-I", CSRC,
                    os.path.join(HERE, "native", "host_coset_blocks.cpp"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    return [ln.split() for ln in out.splitlines()]


def brev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


@pytest.mark.parametrize("lg", [3, 6])
def test_block_constants_and_index_map(lines, lg):
    n = 1 << lg
    rows = [ln for ln in lines if int(ln[0]) == lg]
    assert len(rows) == 8 * n
    w8n = fr_root(lg + 3)
    seen = set()
    for ln in rows:
        m, j, at = int(ln[1]), int(ln[2]), int(ln[3])
        lin, vh_inv, l1v = (int(x, 16) for x in ln[4:7])
        seen.add((m, j))
        x = FR_GEN * pow(w8n, 8 * j + m, R_MOD) % R_MOD
        assert at == m * n + brev(j, lg)
        assert lin == fr_mont(x)
        assert vh_inv == fr_mont(pow((pow(x, n, R_MOD) - 1) % R_MOD, -1, R_MOD))
        assert l1v == fr_mont(pow(n * (x - 1) % R_MOD, -1, R_MOD))
    assert seen == {(m, j) for m in range(8) for j in range(n)}


def test_library_exports_coeff_loader():
    """The symbol is exported and refuses bad arguments before any device
    work: a NULL context, a domain size that is no power of two."""
    import pnp
    from pnp import abi
    lib = pnp.load()
    assert hasattr(lib, "pnp_load_prover_key_coeffs")
    assert "pnp_load_prover_key_coeffs" in pnp.SYMBOLS
    assert callable(getattr(pnp.Context, "load_prover_key_coeffs", None))
    pk = abi.ProverKeyC()
    assert lib.pnp_load_prover_key_coeffs(None, C.byref(pk), 64, 0) == -1  # PNP_E_ARG
    fake = C.c_void_p(0x1000)  # never dereferenced: the size is refused first
    for d in (0, 3, 48, (1 << 10) + 1):
        assert lib.pnp_load_prover_key_coeffs(fake, C.byref(pk), d, 0) == -1
