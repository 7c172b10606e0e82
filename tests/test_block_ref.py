"""tests/block_ref.py held to itself (no GPU): the defining formulas of the
block transforms, as O(n^2) integer sums, return the coefficients they start
from; the oracle-backed array forms the GPU tests compare with agree with the
formulas; and the composite combine(intt(blocks(lde8(c)))) == c at 2^11."""
import numpy as np
import pytest

import block_ref as br
from pnp_testlib import R_MOD, fr_mont, ints_to_arr, oracle, rand_fr_mont_arr, vp


def _mont_arr(vals):
    return ints_to_arr([fr_mont(v) for v in vals])


def _rand_ints(rng, count):
    return [int(v) % R_MOD for v in br.to_obj(rng.integers(0, 2**64, size=(count, 4), dtype=np.uint64))]


def _pipeline_ints(c, lg):
    """coefficients -> E on the 8n coset -> natural blocks -> all 8 Y_m, in integers"""
    n = 1 << lg
    E = br.coset_evals_ints(c, lg)
    Y = [br.intt_block_ints([E[8 * j + m] for j in range(n)], lg, m) for m in range(8)]
    return E, Y


@pytest.mark.parametrize("nb", [6, 7, 8])
@pytest.mark.parametrize("lg", [3, 4, 5])
def test_formulas_return_the_coefficients(lg, nb):
    n = 1 << lg
    rng = np.random.default_rng(100 * lg + nb)
    c = _rand_ints(rng, nb * n)  # degree < nb n
    E, Y = _pipeline_ints(c, lg)
    # the coset values are the oracle's coset NTT of size 8n
    e8 = _mont_arr(c + [0] * (8 * n - len(c)))
    oracle().or_ntt(vp(e8), lg + 3, 0, 1)
    assert (e8 == _mont_arr(E)).all()
    out, nz = br.combine_ints(Y, lg, nb)
    assert out == c
    assert nz == (1 << nb) - 1
    # a coefficient range (the sharded form): the same numbers, chunk by chunk
    q0, length = n // 3, n - n // 3 - 1
    part, _ = br.combine_ints([y[q0:q0 + length] for y in Y], lg, 8, q0)
    full, _ = br.combine_ints(Y, lg, 8)
    assert part == [full[m1 * n + q0 + k] for m1 in range(8) for k in range(length)]
    # the array forms agree with the formulas
    blocks = br.ref_to_blocks(_mont_arr(E), lg, 0, 8)
    p = br.brev_index(lg)
    for m in range(8):
        assert (blocks[m * n + p] == _mont_arr([E[8 * j + m] for j in range(n)])).all()
    Y8 = br.ref_intt_blocks(blocks, lg, 0, 8)
    assert (Y8 == _mont_arr([v for y in Y for v in y])).all()
    for m0, k in [(2, 2), (5, 1), (4, 4)]:
        sub = br.ref_intt_blocks(blocks[m0 * n:(m0 + k) * n], lg, m0, k)
        assert (sub == Y8[m0 * n:(m0 + k) * n]).all()
    got, got_nz = br.ref_t_combine(Y8, lg, nb)
    assert (got == _mont_arr(c)).all() and got_nz == nz
    got, _ = br.ref_t_combine(Y8, lg, 8, q0, length)
    assert (got == _mont_arr(part)).all()


@pytest.mark.parametrize("lg", [0, 1, 4])
def test_lde_blocks_reference(lg):
    """ref_lde_blocks of n coefficients: the permuted direct evaluations, and
    32 times them (canonical) with form29."""
    n = 1 << lg
    rng = np.random.default_rng(lg)
    c = _rand_ints(rng, n)
    E = br.coset_evals_ints(c, lg)
    p = br.brev_index(lg)
    for m0, nb in [(0, 8), (6, 2), (5, 1)]:
        for f29 in (False, True):
            got = br.ref_lde_blocks(_mont_arr(c), lg, m0, nb, f29)
            for b in range(nb):
                exp = [E[8 * j + m0 + b] * (32 if f29 else 1) % R_MOD for j in range(n)]
                assert (got[b * n + p] == _mont_arr(exp)).all(), (m0, nb, f29, b)
    assert max(br.to_obj(br.ref_lde_blocks(_mont_arr(c), lg, 0, 8, True))) < R_MOD


def test_nz_mask_of_a_zero_chunk():
    lg, n = 4, 16
    rng = np.random.default_rng(9)
    c = _rand_ints(rng, 8 * n)
    c[3 * n:4 * n] = [0] * n
    _, Y = _pipeline_ints(c, lg)
    out, nz = br.combine_ints(Y, lg, 8)
    assert out == c and nz == 0xFF & ~(1 << 3)
    Y8 = _mont_arr([v for y in Y for v in y])
    got, got_nz = br.ref_t_combine(Y8, lg, 8)
    assert (got == _mont_arr(c)).all() and got_nz == nz
    zero, zero_nz = br.ref_t_combine(np.zeros((8 * n, 4), dtype=np.uint64), lg, 8)
    assert not zero.any() and zero_nz == 0


def test_composite_reference_2e11():
    """combine(intt(blocks(lde8(c)))) == c through the oracle at 2^11."""
    lg, n = 11, 1 << 11
    c = rand_fr_mont_arr(np.random.default_rng(11), n)
    blocks = br.ref_lde_blocks(c, lg, 0, 8)
    Y8 = br.ref_intt_blocks(blocks, lg, 0, 8)
    out, nz = br.ref_t_combine(Y8, lg, 8)
    assert (out[:n] == c).all() and not out[n:].any() and nz == 1
