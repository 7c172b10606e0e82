"""The GPU side of the block-transform and NTT comparisons, shared by
tests/test_gpu_blocks.py and its PNP_NTT_ROWS=0 child (tests/ntt_rows_worker.py).
Every device buffer is allocated here at the length include/pnp_plonk.h states
for its operator."""
import functools

import numpy as np

import block_ref as br
from gpu_util import to_dev, from_dev, empty_dev
from pnp_testlib import oracle, vp, rand_fr_mont_arr


@functools.lru_cache(maxsize=None)
def coeffs(lg: int) -> np.ndarray:
    """The n coefficients every block test of this lg starts from (read-only)."""
    c = rand_fr_mont_arr(np.random.default_rng(4000 + lg), 1 << lg)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def coset_values(lg: int) -> np.ndarray:
    """or_coset_lde8 of coeffs(lg): computed once, shared, read-only."""
    E = br.coset_lde8(coeffs(lg), lg)
    E.setflags(write=False)
    return E


def gpu_lde_blocks(ctx, c: np.ndarray, lg: int, m0: int, nb: int, form29: bool = False):
    """-> the device tensor of nb n elements"""
    src = to_dev(c)
    assert src.shape[0] == 1 << lg
    out = empty_dev(nb << lg)
    ctx.lde_blocks(src.data_ptr(), out.data_ptr(), lg, m0, nb, form29)
    ctx.sync()
    return out


def gpu_intt_blocks(ctx, blocks: np.ndarray, lg: int, m0: int, nb: int) -> np.ndarray:
    assert blocks.shape[0] == nb << lg
    d = to_dev(blocks)
    ctx.intt_blocks(d.data_ptr(), lg, m0, nb)
    ctx.sync()
    return from_dev(d)


def gpu_t_combine_blocks(ctx, Y: np.ndarray, nb: int, lg: int):
    assert Y.shape[0] == nb << lg
    d = to_dev(Y)
    out = empty_dev(nb << lg)
    nz = ctx.t_combine_blocks(d.data_ptr(), nb, out.data_ptr(), lg)
    return from_dev(out), nz


def check_lde_intt(ctx, lg: int, m0: int, nb: int, formula_max_lg: int = 13):
    """lde_blocks (plain and form29) against the reference, then intt_blocks of
    the plain blocks: against the formula up to formula_max_lg, above it the
    round trip through t_combine_blocks back to the coefficients (nb >= 6)."""
    c, E = coeffs(lg), coset_values(lg)
    n = 1 << lg
    exp = br.ref_lde_blocks(c, lg, m0, nb, E=E)
    got = from_dev(gpu_lde_blocks(ctx, c, lg, m0, nb))
    assert (got == exp).all(), ("lde_blocks", lg, m0, nb)
    got29 = from_dev(gpu_lde_blocks(ctx, c, lg, m0, nb, True))
    assert (got29 == br.ref_lde_blocks(c, lg, m0, nb, True, E=E)).all(), ("lde_blocks form29", lg, m0, nb)
    Y = gpu_intt_blocks(ctx, exp, lg, m0, nb)
    if lg <= formula_max_lg:
        assert (Y == br.ref_intt_blocks(exp, lg, m0, nb)).all(), ("intt_blocks", lg, m0, nb)
    else:
        assert m0 == 0 and nb >= 6
        back, nz = gpu_t_combine_blocks(ctx, Y, nb, lg)
        assert (back[:n] == c).all() and not back[n:].any() and nz == 1, ("round trip", lg, nb)


NTT_VARIANTS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def check_ntt(ctx, x: np.ndarray, lg: int, variants=NTT_VARIANTS, what=""):
    """pnp_ntt of x against or_ntt, bit for bit"""
    lib = oracle()
    for inverse, coset in variants:
        exp = x.copy()
        lib.or_ntt(vp(exp), lg, inverse, coset)
        d = to_dev(x)
        ctx.ntt(d.data_ptr(), lg, bool(inverse), bool(coset))
        assert (from_dev(d) == exp).all(), (what, lg, inverse, coset)
