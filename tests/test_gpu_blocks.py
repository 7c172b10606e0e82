"""Round 4's block-layout transforms (csrc/ntt.hip lde_blocks, intt_blocks,
t_combine_blocks, t_combine, to_blocks) through their operator forms, limb for
limb against tests/block_ref.py (held to its formulas by tests/test_block_ref.py).

Which kernels a case runs (ntt_core: n = 2^lg, nb blocks, tiles of 1024):

  lg 0, 1, 5, 6, any nb        small path: k_lde_twist / k_ntt_small / k_mul_table
  lg 7: nb 8     K = 7;  nb 6, 7             small path (nb n not whole tiles)
  lg 8: nb 8, 4  K = 8;  nb 6, 7             small path
  lg 9: nb 8, 6, 4, 2  K = 9;  nb 7, 1       small path
  lg 10: nb >= 2  K = 10;  nb 1              small path (one block, lg <= 10)
  lg 11  (6, 5)   lg 12  (6, 6)   lg 13  (7, 6)   lg 16  (8, 8)   lg 18  (9, 9)
                                             two passes, any nb

"K = k" is one k_ntt_pass4<k>: lde_blocks runs it as a DIF with the coset twist
fused in (`pre`), intt_blocks as a DIT with the block twist fused in (`post`).
Two passes (K1, K2): the DIF runs K1 first (with `pre`, lg_hlo = K2) and K2
last (lg_hlo = 0); the DIT runs K1 first (lg_hlo = 0) and K2 last (with `post`,
lg_hlo = K1).  So, over the cases below,

  DIF first pass, with `pre`:  K = 6 (lg 11, 12), 7 (lg 7, 13), 8 (lg 8, 16),
                               9 (lg 9), 10 (lg 10)
  DIF last pass of two:        K = 5 (lg 11), 6 (lg 12, 13), 8 (lg 16)
  DIT last pass, with `post`:  K = 5 (lg 11), 6 (lg 12, 13), 7 (lg 7), 8 (lg 8, 16),
                               9 (lg 9, 18), 10 (lg 10)
  DIT first pass of two:       K = 6 (lg 11, 12), 7 (lg 13), 8 (lg 16), 9 (lg 18)

K = 5 is only ever the second pass of lg 11 (the balanced split has no other
pass under 6 levels), so it has no DIF form with `pre` and no lg_hlo = 0 DIT
form.  The same kernels with the plain twiddle table (PNP_NTT_ROWS=0) run in
test_plain_twiddle_table's child process.

The kept cases: the lg sweep on the three block counts a proof uses, (0, 8),
(0, 6), (0, 7), and the sharded / redo shapes (6, 2), (4, 4), (2, 2), (5, 1) at
one lg of each class: 6 (small), 9 (K = 9, and small for one block), 10
(K = 10, and small for one block), 11 (two passes).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import block_ref as br
from block_gpu import check_lde_intt, gpu_intt_blocks, gpu_t_combine_blocks
from gpu_util import to_dev, from_dev, empty_dev
from pnp_testlib import REPO, oracle, vp, rand_fr_mont_arr

pytestmark = pytest.mark.gpu

LGS = [0, 1, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16]
SHAPES = [(0, 8), (0, 6), (0, 7), (6, 2), (4, 4), (2, 2), (5, 1)]
CASES = ([(lg, m0, nb) for lg in LGS for m0, nb in SHAPES[:3]]
         + [(lg, m0, nb) for lg in (6, 9, 10, 11) for m0, nb in SHAPES[3:]])


@pytest.fixture(scope="module")
def ctx():
    import pnp
    c = pnp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("lg,m0,nb", CASES)
def test_lde_and_intt_blocks(ctx, lg, m0, nb):
    """lde_blocks, plain and form29 (values times 32), and intt_blocks of its
    output: the intermediate Y against the formula up to 2^13, at 2^16 the
    round trip back to the coefficients."""
    check_lde_intt(ctx, lg, m0, nb)


def test_intt_blocks_2e18(ctx):
    """k_ntt_pass4<9, DIT> in both positions of a two-pass transform (lg_hlo = 0
    and 9, the latter with `post`), which no smaller size reaches: one block of
    2^18 arbitrary values against the formula."""
    lg, m0 = 18, 5
    blk = rand_fr_mont_arr(np.random.default_rng(18), 1 << lg)
    assert (gpu_intt_blocks(ctx, blk, lg, m0, 1) == br.ref_intt_blocks(blk, lg, m0, 1)).all()


@pytest.mark.parametrize("lg", [0, 1, 6, 9, 11])
def test_to_blocks(ctx, lg):
    """The permutation alone, on an arbitrary array of 8n values."""
    a8 = rand_fr_mont_arr(np.random.default_rng(70 + lg), 8 << lg)
    src = to_dev(a8)
    for m0, nb in SHAPES:
        out = empty_dev(nb << lg)
        ctx.to_blocks(src.data_ptr(), out.data_ptr(), lg, m0, nb)
        ctx.sync()
        assert (from_dev(out) == br.ref_to_blocks(a8, lg, m0, nb)).all(), (m0, nb)


def _blocks_of_poly(c: np.ndarray, lg: int) -> np.ndarray:
    """All 8 Y_m (8n, reference) of the polynomial with the coefficients c, deg < 8n"""
    n = 1 << lg
    e8 = np.zeros((8 * n, 4), dtype=np.uint64)
    e8[:len(c)] = c
    oracle().or_ntt(vp(e8), lg + 3, 0, 1)
    return br.ref_intt_blocks(br.ref_to_blocks(e8, lg, 0, 8), lg, 0, 8)


@pytest.mark.parametrize("nb", [6, 7, 8])
@pytest.mark.parametrize("lg", [5, 8, 11])
def test_t_combine_blocks(ctx, lg, nb):
    """Coefficients and chunk mask of a polynomial of degree < nb n from its
    first nb blocks (nb < 8: the missing blocks solved for), of one whose chunk
    3 is zero, and of the zero polynomial."""
    n = 1 << lg
    rng = np.random.default_rng(1000 * lg + nb)
    c = rand_fr_mont_arr(rng, nb * n)
    for zero_chunk in (None, 3):
        if zero_chunk is not None:
            c[zero_chunk * n:(zero_chunk + 1) * n] = 0
        Y8 = _blocks_of_poly(c, lg)
        exp, exp_nz = br.ref_t_combine(Y8, lg, nb)
        assert (exp == c).all()  # the formula returns the coefficients
        assert exp_nz == ((1 << nb) - 1 if zero_chunk is None else ((1 << nb) - 1) & ~(1 << zero_chunk))
        got, nz = gpu_t_combine_blocks(ctx, Y8[:nb * n], nb, lg)
        assert (got == exp).all(), zero_chunk
        assert nz == exp_nz, zero_chunk
    got, nz = gpu_t_combine_blocks(ctx, np.zeros((nb * n, 4), dtype=np.uint64), nb, lg)
    assert not got.any() and nz == 0


@pytest.mark.parametrize("q0,length", [(0, 683), (683, 683), (1366, 682)])
def test_t_combine_range(ctx, q0, length):
    """The three-rank split of 2^11 coefficient indices (lengths that are no
    multiple of the 256-thread block): every chunk's coefficients of the range
    and the mask, from all 8 blocks; chunk 5 is zero."""
    lg, n = 11, 1 << 11
    c = rand_fr_mont_arr(np.random.default_rng(2011), 8 * n)
    c[5 * n:6 * n] = 0
    Y8 = _blocks_of_poly(c, lg)
    exp, exp_nz = br.ref_t_combine(Y8, lg, 8, q0, length)
    assert (exp == np.concatenate([c[m1 * n + q0:m1 * n + q0 + length] for m1 in range(8)])).all()
    assert exp_nz == 0xFF & ~(1 << 5)
    Yr = np.concatenate([Y8[m * n + q0:m * n + q0 + length] for m in range(8)])
    d, out = to_dev(Yr), empty_dev(8 * length)
    nz = ctx.t_combine_range(d.data_ptr(), length, q0, out.data_ptr(), lg)
    assert (from_dev(out) == exp).all()
    assert nz == exp_nz


def test_operators_refuse_bad_arguments(ctx):
    """Each out-of-range argument of each wrapper is PNP_E_ARG before any
    launch (the buffers would hold the largest valid request at lg_n = 3)."""
    import pnp
    lg = 3
    a, b = empty_dev(8 << lg), empty_dev(8 << lg)
    A, B = a.data_ptr(), b.data_ptr()

    def refused(fn, *args):
        with pytest.raises(pnp.PnpError, match="PNP_E_ARG"):
            fn(*args)

    for m0, nb in [(-1, 2), (0, 0), (3, -1), (1, 8), (8, 1), (0, 9)]:
        refused(ctx.lde_blocks, A, B, lg, m0, nb)
        refused(ctx.to_blocks, A, B, lg, m0, nb)
        refused(ctx.intt_blocks, A, lg, m0, nb)
    refused(ctx.lde_blocks, A, B, 26, 0, 8)
    refused(ctx.to_blocks, A, B, 26, 0, 8)
    refused(ctx.intt_blocks, A, 26, 0, 8)
    refused(ctx.lde_blocks, 0, B, lg, 0, 8)
    refused(ctx.lde_blocks, A, 0, lg, 0, 8)
    refused(ctx.to_blocks, 0, B, lg, 0, 8)
    refused(ctx.to_blocks, A, 0, lg, 0, 8)
    refused(ctx.intt_blocks, 0, lg, 0, 8)
    for nb in (0, 5, 9, -6):
        refused(ctx.t_combine_blocks, A, nb, B, lg)
    refused(ctx.t_combine_blocks, A, 8, B, 26)
    refused(ctx.t_combine_blocks, 0, 8, B, lg)
    refused(ctx.t_combine_blocks, A, 8, 0, lg)
    for q0, length in [(0, 9), (8, 1), (9, 0), (5, 4), (1, 2**64 - 1)]:
        refused(ctx.t_combine_range, A, length, q0, B, lg)
    refused(ctx.t_combine_range, A, 8, 0, B, 26)
    refused(ctx.t_combine_range, 0, 8, 0, B, lg)
    refused(ctx.t_combine_range, A, 8, 0, 0, lg)
    lib = pnp.load()
    assert lib.pnp_t_combine_blocks(ctx.h, A, 8, B, lg, None) == -1
    assert lib.pnp_t_combine_range(ctx.h, A, 8, 0, B, lg, None) == -1
    assert lib.pnp_lde_blocks(None, A, B, lg, 0, 8, 0) == -1
    # and the context still works
    check_lde_intt(ctx, lg, 0, 8)


def test_plain_twiddle_table():
    """PNP_NTT_ROWS=0 (the plain twiddle table instead of the dense rows; read
    once per process, hence the child): pnp_ntt at 2^11 and 2^12 and the block
    transforms through every K of 5..10 against the same references."""
    worker = os.path.join(REPO, "tests", "ntt_rows_worker.py")
    r = subprocess.run([sys.executable, worker], env=dict(os.environ, PNP_NTT_ROWS="0"), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "ROWS_OFF_OK" in r.stdout
