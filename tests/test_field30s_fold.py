"""CPU model of the folded subtractions of csrc/field30s.cuh: mul30s_sub
(a b 2^-390 - d) and sqr30s_sub2 (a^2 2^-390 - d - 2 e), the product's column
loop with limb j of the subtrahend added to result column 13 + j, times -1
(-2), before that column is reduced, and limb 12 taken from what is left.  On
test_field30s's own accumulator (every partial sum asserted inside 64 bits)
and reduction column.

Checked: each routine gives, limb for limb, what the renormalised subtraction
of the product gave (sub30s(mul30s(a, b), d), sub30s(sub2_30s(sqr30s(a), d, e),
e)); the worst-case column from limb magnitudes alone stays under 2^63; the
mixed addition written with the folds (ec30s.cuh madd30s) equals
test_field30s.madd30s limb for limb along chains with both signs.  The case
lists are the ones the device routines run on in tests/test_gpu_field30s_fold.py."""
import functools
import random

import pytest

import test_field30s as m30
from test_field29 import _mulg

H, Q = m30.H, m30.Q
L = m30.limbs


def _sub_in(*ops):
    for d in ops:
        assert all(abs(x) <= H for x in d[:12]), "subtrahend limb out of range"
        m30.i32(d[12])


def mul30s_sub(a, b, d, peak=None):
    """mul30s_sub of field30s.cuh"""
    m30._in(a, b)
    _sub_in(d)
    m, r, acc = [0] * 13, [0] * 13, m30.Acc()
    for k in range(25):
        for i in range(max(0, k - 12), min(k, 12) + 1):
            acc.mad(a[i], b[k - i])
        if k >= 13:
            acc.mad(d[k - 13], -1)
        acc.set(m30.reduce_col(k, acc, m, r))
    r[12] = m30.i32(m30.i32(acc.v) - d[12])
    if peak is not None:
        peak.append(acc.peak)
    return r


def sqr30s_sub2(a, d, e, peak=None):
    """sqr30s_sub2 of field30s.cuh"""
    m30._in(a)
    _sub_in(d, e)
    a2 = [m30.i32(2 * x) for x in a]
    m, r, acc = [0] * 13, [0] * 13, m30.Acc()
    for k in range(25):
        for i in range(max(0, k - 12), 13):
            if 2 * i < k:
                acc.mad(a[i], a2[k - i])
        if k % 2 == 0:
            acc.mad(a[k // 2], a[k // 2])
        if k >= 13:
            acc.mad(d[k - 13], -1)
            acc.mad(e[k - 13], -2)
        acc.set(m30.reduce_col(k, acc, m, r))
    r[12] = m30.i32(m30.i32(m30.i32(acc.v) - d[12]) - m30.i32(2 * e[12]))
    if peak is not None:
        peak.append(acc.peak)
    return r


def mul_then_sub(a, b, d):
    """what madd30s did before the fold"""
    return m30.sub30s(m30.mul30s(a, b), d)


def sqr_then_sub2(a, d, e):
    return m30.sub30s(m30.sub2_30s(m30.sqr30s(a), d, e), e)


def madd30s_fold(p, x2, y2):
    """madd30s of ec30s.cuh; returns the intermediates too"""
    X, Y, ZZ, ZZZ = p
    P, R = mul30s_sub(x2, ZZ, X), mul30s_sub(y2, ZZZ, Y)
    pp = m30.sqr30s(P)
    ppp = m30.mul30s(P, pp)
    q = m30.mul30s(X, pp)
    x3 = sqr30s_sub2(R, ppp, q)
    y3 = m30.mul2_30s(R, m30.sub30s(q, x3), Y, m30.neg30s(ppp))
    return (x3, y3, m30.mul30s(ZZ, pp), m30.mul30s(ZZZ, ppp)), (P, R)


# ---------------------------------------------------------------- the cases
def sub_extremes():
    """subtrahends with every limb 0..11 at +-2^29 (one sign, and alternating)
    and limb 12 at +-2^24"""
    out = []
    for top in (2**24, -2**24):
        out += [[s] * 12 + [top] for s in (H, -H)]
        out += [[s if i % 2 else -s for i in range(12)] + [top] for s in (H, -H)]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """{routine: [(tag, a, b, d) or (tag, a, d, e)]}: the operand extremes of
    test_field30s against each other and against the subtrahend extremes, the
    subtrahend extremes against every operand extreme, 1,000 random operands
    below 2^385"""
    rnd = random.Random(301)
    r385 = lambda: L(rnd.randrange(-2**385 + 1, 2**385))  # noqa: E731
    ext = [L(v) for v in m30._extremes()]
    sx = sub_extremes()
    n = len(ext)
    mul, sqr = [], []
    for i, a in enumerate(ext):
        for j, b in enumerate(ext):
            mul.append((f"extreme{i}x{j}-extreme{(i + j + 2) % n}", a, b, ext[(i + j + 2) % n]))
            mul.append((f"extreme{i}x{j}-sub{(i + j) % 8}", a, b, sx[(i + j) % 8]))
            sqr.append((f"extreme{i}-extreme{j}-2extreme{(i + j + 2) % n}", a, b, ext[(i + j + 2) % n]))
        for k, d in enumerate(sx):
            mul.append((f"extreme{i}x{(i + 5) % n}-sub{k}", a, ext[(i + 5) % n], d))
            mul.append((f"random_x_extreme{i}-sub{k}", r385(), a, d))
            for k2, e in enumerate(sx):
                sqr.append((f"extreme{i}-sub{k}-2sub{k2}", a, d, e))
    for k, d in enumerate(sx):
        for k2, e in enumerate(sx):
            sqr.append((f"random-sub{k}-2sub{k2}", r385(), d, e))
    for _ in range(1000):
        mul.append(("random", r385(), r385(), r385()))
        sqr.append(("random", r385(), r385(), r385()))
    return {"mul30s_sub": mul, "sqr30s_sub2": sqr}


MODEL = {"mul30s_sub": mul30s_sub, "sqr30s_sub2": sqr30s_sub2}
UNFOLDED = {"mul30s_sub": mul_then_sub, "sqr30s_sub2": sqr_then_sub2}


@functools.lru_cache(maxsize=None)
def expected():
    """the model's result of every case, computed once"""
    return {name: [MODEL[name](*c[1:]) for c in cs] for name, cs in cases().items()}


# ---------------------------------------------------------------- tests
def test_case_lists():
    cs = cases()
    for name in MODEL:
        tags = [c[0] for c in cs[name]]
        assert sum(t == "random" for t in tags) == 1000
        assert sum(t.startswith("extreme") for t in tags) >= 121
        assert any("sub" in t for t in tags)
        for c in cs[name]:
            assert all(abs(m30.val(o)) < 2**385 for o in c[1:]), c[0]
    for d in sub_extremes():
        assert all(abs(x) == H for x in d[:12]) and abs(d[12]) == 2**24
    assert len({tuple(d) for d in sub_extremes()}) == 8


@pytest.mark.parametrize("name", sorted(MODEL))
def test_fold_equals_renormalised_subtraction(name):
    ir = pow(m30.R390, -1, Q)
    for (tag, *ops), r in zip(cases()[name], expected()[name]):
        assert r == UNFOLDED[name](*ops), tag
        assert all(-H <= x < H for x in r[:12]), tag
        v = [m30.val(o) for o in ops]
        want = v[0] * v[1] * ir - v[2] if name == "mul30s_sub" else v[0] * v[0] * ir - v[1] - 2 * v[2]
        assert (m30.val(r) - want) % Q == 0, tag
        bound = 2**381 + abs(v[2]) if name == "mul30s_sub" else 2**381 + abs(v[1]) + 2 * abs(v[2])
        assert abs(m30.val(r)) < bound, tag


def _column_bounds(kind):
    """test_field30s._column_bounds with the fold terms: every operand limb,
    every m_i, every limb of q and of the subtrahends taken as 2^29, all terms
    with one sign; a result column takes 2^29 (mul30s_sub) or 3 2^29
    (sqr30s_sub2) more"""
    peak, carry = 0, 0
    for k in range(25):
        n = k + 1 if k < 13 else 25 - k
        red = (min(k, 13) - max(0, k - 12)) + (1 if k < 13 else 0)
        if kind == "mul_sub":
            ops = n * H * H + (H if k >= 13 else 0)
        else:
            ops = (n // 2) * H * (2 * H) + (H * H if k % 2 == 0 else 0) + (3 * H if k >= 13 else 0)
        peak = max(peak, carry + ops + red * H * H)
        carry = ((carry + ops + red * H * H) >> 30) + 1
        peak = max(peak, carry)
    return peak


def test_worst_case_columns():
    for kind in ("mul_sub", "sqr_sub2"):
        assert _column_bounds(kind) < 2**63, kind
    # the counts the header states: 13 + 13 products (the square: 27) of 2^58, a
    # carry below 2^34, fold terms of at most 3 2^29
    assert _column_bounds("mul_sub") <= 26 * 2**58 + 2**34 + H
    assert _column_bounds("sqr_sub2") <= 27 * 2**58 + 2**34 + 3 * H
    # and the model itself (asserting every partial sum) at the limb extremes,
    # all signs, the top limbs at +-2^29 too: the columns must still hold
    alt = [H if i % 2 else -H for i in range(13)]
    for sa in (-H, H):
        for sb in (-H, H):
            for sd in (-H, H):
                a, b, d = [sa] * 13, [sb] * 13, [sd] * 13
                pk = []
                assert mul30s_sub(a, b, d, pk) == mul_then_sub(a, b, d)
                assert pk[0] <= _column_bounds("mul_sub")
                pk = []
                assert sqr30s_sub2(a, b, d, pk) == sqr_then_sub2(a, b, d)
                assert pk[0] <= _column_bounds("sqr_sub2")
                assert mul30s_sub(alt, a, d) == mul_then_sub(alt, a, d)
                assert sqr30s_sub2(alt, b, d) == sqr_then_sub2(alt, b, d)


@pytest.mark.parametrize("seed", [5, 6])
def test_madd_chain_equals_unfolded(seed):
    rnd = random.Random(seed)
    pts = [_mulg(rnd.randrange(1, 2**64)) for _ in range(32)]
    tab = lambda v: m30.to_f30s(v * 2**384 % Q)  # noqa: E731  the table's form
    acc = (tab(pts[0][0]), tab(pts[0][1]), m30.C["F30S_ONE"], m30.C["F30S_ONE"])
    signs = set()
    for x, y in pts[1:]:
        ym = tab(y)
        neg = rnd.random() < 0.5
        signs.add(neg)
        if neg:
            ym = m30.neg30s(ym)
        X, Y, ZZ, ZZZ = acc
        want = m30.madd30s(acc, tab(x), ym)
        acc, (P, R) = madd30s_fold(acc, tab(x), ym)
        assert tuple(acc) == tuple(want)  # x3, y3, zz, zzz
        assert P == m30.sub30s(m30.mul30s(tab(x), ZZ), X) and R == m30.sub30s(m30.mul30s(ym, ZZZ), Y)
    assert signs == {True, False}
