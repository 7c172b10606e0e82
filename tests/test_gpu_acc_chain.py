"""The folded MSM after the products of csrc/field30s.cuh were put on one
accumulator chain (the carry of a column is the addend of the next column's
first multiply-add; no arithmetic changed): pnp_commit_ck and
pnp_commit_segments (B = 1 and B = 4) against the oracle's Pippenger
(oracle/g1.c or_commit), bit for bit, at 2^10 and 2^12 points, with the
production window (c = 20) and the window the size itself picks, over the
scalar families of tests/test_gpu_field30s.py: random scalars; every scalar
-1 = r - 1 (the sign and the top window); one value in every scalar (a heavy
bucket per window, k_merge_heavy29); equal and opposite points in one bucket
(ZZ = 0, the redo lanes).  And one proof at 2^10, byte for byte."""
import numpy as np
import pytest

from pnp_testlib import Inputs, oracle, vp, rand_fr_mont_arr, R_MOD, fr_mont
from gpu_util import to_dev
from pnp import abi

pytestmark = pytest.mark.gpu

Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
SIZES = [1 << 10, 1 << 12]
NMAX = 4 * SIZES[-1] + 7


@pytest.fixture(scope="module", params=["20", None], ids=["c20", "cdefault"])
def ctx(request):
    import pnp
    with pytest.MonkeyPatch.context() as mp:
        if request.param:
            mp.setenv("PNP_FOLD_C", request.param)  # read when the context is made
        c = pnp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def srs():
    rng = np.random.default_rng(31)
    pts = np.zeros((NMAX, 12), dtype=np.uint64)
    oracle().or_srs(vp(pts), NMAX, vp(rand_fr_mont_arr(rng, 1)))
    pts.setflags(write=False)
    return pts


def _fr(v):
    m = fr_mont(v % R_MOD)
    return np.array([(m >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


def _neg_point(p):
    y = sum(int(p[6 + i]) << (64 * i) for i in range(6))
    out = p.copy()
    out[6:] = [((Q - y) >> (64 * i)) & (2**64 - 1) for i in range(6)]
    return out


def _scalars(family, rng, n):
    if family == "random":
        return rand_fr_mont_arr(rng, n)
    if family == "minus_one":  # r - 1 in every scalar
        return np.repeat(_fr(R_MOD - 1)[None, :], n, axis=0)
    if family == "all_equal":  # one heavy bucket per window
        return np.repeat(rand_fr_mont_arr(rng, 1), n, axis=0)
    raise KeyError(family)


def _oracle_commit(pts, sc):
    exp = np.zeros(12, dtype=np.uint64)
    oracle().or_commit(vp(np.ascontiguousarray(pts)), vp(np.ascontiguousarray(sc)), len(sc), vp(exp))
    return exp


def _aff(c):
    return np.array(list(c.x) + list(c.y), dtype=np.uint64)


def _commit_ck(ctx, pts, sc):
    dp, ds = to_dev(pts), to_dev(sc)
    ctx.load_commit_key(abi.CommitKeyC(powers_of_g=abi.ptr(dp.data_ptr()), powers_of_gamma_g=abi.ptr(dp.data_ptr())),
                        len(pts), device_ptrs=True)
    return _aff(ctx.commit_ck(ds.data_ptr(), len(pts)))


def _check_all_entry_points(ctx, pts, n, make_scalars):
    """pnp_commit_ck over pts[:n], then the segmented batch over sub-ranges of
    pts at B = 1 and B = 4"""
    sc = make_scalars()
    assert (_commit_ck(ctx, pts[:n].copy(), sc) == _oracle_commit(pts[:n], sc)).all(), "pnp_commit_ck"
    dp = to_dev(pts)
    for offs in ([3], [0, n, 2 * n + 1, 3 * n + 7]):
        scs = [make_scalars() for _ in offs]
        ds = [to_dev(s) for s in scs]
        got = ctx.commit_segments(dp.data_ptr(), len(pts), offs, [d.data_ptr() for d in ds], n)
        for b, o in enumerate(offs):
            assert (_aff(got[b]) == _oracle_commit(pts[o:o + n], scs[b])).all(), ("pnp_commit_segments", offs, b)


@pytest.mark.parametrize("family", ["random", "minus_one", "all_equal"])
@pytest.mark.parametrize("n", SIZES)
def test_folded_msm_scalar_families(ctx, srs, n, family):
    rng = np.random.default_rng(2000 * n + len(family))
    _check_all_entry_points(ctx, srs[:4 * n + 7].copy(), n, lambda: _scalars(family, rng, n))


@pytest.mark.parametrize("n", SIZES)
def test_folded_msm_equal_and_opposite_points(ctx, srs, n):
    """P, P, -P, Q in every group of four points, under two scalar values:
    equal points meet in one bucket (a doubling inside a piece), opposite ones
    cancel there (ZZ = 0 mod q), and the lane is redone exactly."""
    rng = np.random.default_rng(9000 + n)
    pts = srs[:4 * n + 7].copy()
    vals = rand_fr_mont_arr(rng, 2)
    for i in range(0, len(pts) - 3, 4):
        pts[i + 1] = pts[i]
        pts[i + 2] = _neg_point(pts[i])
    _check_all_entry_points(ctx, pts, n, lambda: np.ascontiguousarray(vals[rng.integers(0, 2, size=n)]))
    sc = np.repeat(vals[:1], n, axis=0)  # the redo itself, counted: every point under one scalar
    ctx.kernel_timing(True)
    got = _commit_ck(ctx, pts[:n].copy(), sc)
    redone = ctx.kernel_bytes("msm_redo_lanes") + ctx.kernel_bytes("msm_exact_fallback")
    ctx.kernel_timing(False)
    assert (got == _oracle_commit(pts[:n], sc)).all()
    assert redone > 0


def test_proof_2e10_byte_equal():
    import pnp
    inp = Inputs(10, 31)
    exp = inp.oracle_proof()
    got = pnp.load().gen_proof(inp.circuit, inp.pk, inp.ck)
    assert abi.proof_to_bytes(got) == abi.proof_to_bytes(exp)
