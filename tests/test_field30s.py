"""CPU model of the signed radix-2^30 Fq arithmetic of csrc/field30s.cuh (the
mixed addition of the MSM bucket accumulation): every routine restated in
Python limb for limb, with the signed 64-bit column accumulator and the 32-bit
limb sums asserted at every step; the worst-case column sums from limb
magnitudes alone (not from random inputs); an interval analysis of the mixed
addition; agreement with plain modular arithmetic; the table and piece forms.
This file checks the Python model; the compiled device routines themselves run
on the same edge lists in tests/test_gpu_dev_arith.py (tests/native/
dev_arith.hip), limb for limb against this model."""
import os
import random
import re

import pytest

from test_field29 import G1X, G1Y, aff_add, _mulg, from_m as from_m29

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(HERE, "..", "zprize23-gpu-submission_amd", "csrc", "f30s_consts.inc")
Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
H = 1 << 29
R390 = 1 << 390


def _consts():
    txt = open(INC).read()
    arrs = {m.group(1): [int(x) for x in m.group(2).split(",")]
            for m in re.finditer(r"(F30S_\w+)\[13\] = \{([^}]*)\}", txt)}
    return arrs, int(re.search(r"F30S_QINV = (-?\d+);", txt).group(1))


C, QINV = _consts()
QL = C["F30S_Q"]


def val(l):
    return sum(x << (30 * i) for i, x in enumerate(l))


def limbs(v):
    """balanced limbs of any integer, the top one taking what is left"""
    out = []
    for _ in range(12):
        l = bal30(v)
        out.append(l)
        v = (v - l) >> 30
    return out + [v]


def i32(x):
    assert -2**31 <= x < 2**31, "32-bit limb sum overflows"
    return x


def bal30(x):
    x &= (1 << 30) - 1
    return x - (1 << 30) if x >= H else x


class Acc:
    """the signed 64-bit column accumulator: every partial sum checked"""

    def __init__(self):
        self.v, self.peak = 0, 0

    def mad(self, a, b):
        assert abs(a) <= 2**30 and abs(b) <= 2**30
        self.set(self.v + a * b)

    def set(self, v):
        assert -2**63 <= v < 2**63, "column accumulator overflows"
        self.v, self.peak = v, max(self.peak, abs(v))


def carry30(v):
    return (v + H) >> 30


def reduce_col(k, acc, m, r):
    """reduce_col30s: returns the carry into column k + 1"""
    for i in range(max(0, k - 12), min(k, 13)):
        acc.mad(m[i], QL[k - i])
    if k < 13:
        m[k] = bal30((acc.v & 0xFFFFFFFF) * (QINV & 0xFFFFFFFF))
        acc.mad(m[k], QL[0])
        assert acc.v & ((1 << 30) - 1) == 0
        return acc.v >> 30
    r[k - 13] = bal30(acc.v)
    return carry30(acc.v)


def _in(*ops):
    for a in ops:
        assert all(abs(x) <= H for x in a), "product input limb out of range"


def mul30s(a, b, peak=None):
    _in(a, b)
    m, r, acc = [0] * 13, [0] * 13, Acc()
    for k in range(25):
        for i in range(max(0, k - 12), min(k, 12) + 1):
            acc.mad(a[i], b[k - i])
        acc.set(reduce_col(k, acc, m, r))
    r[12] = i32(acc.v)
    if peak is not None:
        peak.append(acc.peak)
    return r


def sqr30s(a, peak=None):
    _in(a)
    a2 = [i32(2 * x) for x in a]
    m, r, acc = [0] * 13, [0] * 13, Acc()
    for k in range(25):
        for i in range(max(0, k - 12), 13):
            if 2 * i < k:
                acc.mad(a[i], a2[k - i])
        if k % 2 == 0:
            acc.mad(a[k // 2], a[k // 2])
        acc.set(reduce_col(k, acc, m, r))
    r[12] = i32(acc.v)
    if peak is not None:
        peak.append(acc.peak)
    return r


def heavy(k):
    return 3 * (k + 1 if k < 13 else 25 - k) > 31


def mul2_30s(a, b, c, d, peak=None):
    _in(a, b, c, d)
    m, r, acc = [0] * 13, [0] * 13, Acc()
    for k in range(25):
        for i in range(max(0, k - 12), min(k, 12) + 1):
            acc.mad(a[i], b[k - i])
            acc.mad(c[i], d[k - i])
        if heavy(k):
            hi = carry30(acc.v)
            acc.set(bal30(acc.v))
            acc.set(reduce_col(k, acc, m, r) + hi)
        else:
            acc.set(reduce_col(k, acc, m, r))
    r[12] = i32(acc.v)
    if peak is not None:
        peak.append(acc.peak)
    return r


def norm30s(t, three=False):
    r, c = [0] * 13, 0
    for i in range(12):
        assert abs(t[i]) <= (3 if three else 2) * H
        s = i32(t[i] + c)
        r[i] = bal30(s)
        c = (s >> 30) + ((s >> 29) & 1) if three else i32(s + H) >> 30
    r[12] = i32(t[12] + c)
    assert val(r) == val(t)
    return r


def sub30s(a, b):
    return norm30s([i32(x - y) for x, y in zip(a, b)])


def sub2_30s(a, b, c):
    return norm30s([i32(i32(x - y) - z) for x, y, z in zip(a, b, c)], True)


def neg30s(a):
    return [-x for x in a]


def lift30s(r):
    u, c = [0] * 13, 0
    for i in range(12):
        t = i32(r[i] + QL[i] + c)
        u[i], c = t & 0x3FFFFFFF, t >> 30
    u[12] = i32(r[12] + QL[12] + c)
    assert u[12] >= 0 and sum(x << (30 * i) for i, x in enumerate(u)) == val(r) + Q
    return u


def to_f29(a):
    """R390 F30s -> raw R406 F29 (14 limbs < 2^29, value < 2q)"""
    u = lift30s(mul30s(a, C["F30S_C406"])) + [0]
    out = []
    for j in range(14):
        w, sh = divmod(29 * j, 30)
        out.append(((u[w] | (u[w + 1] << 30)) >> sh) & 0x1FFFFFFF)
    return out


def to_fq32(a):
    """R390 F30s -> canonical R384 integer (12 x 32-bit words, reduced once)"""
    u = lift30s(mul30s(a, C["F30S_C384"])) + [0, 0]
    v = 0
    for w in range(12):
        j, sh = divmod(32 * w, 30)
        x = (u[j] >> sh) | (u[j + 1] << (30 - sh)) | ((u[j + 2] << (60 - sh)) if 60 - sh < 32 else 0)
        v |= (x & 0xFFFFFFFF) << (32 * w)
    return v - Q if v >= Q else v


def to_f30s(v):
    """canonical R384 integer -> R390 F30s"""
    assert 0 <= v < Q
    t, c = [0] * 13, 0
    for j in range(13):
        u = ((v >> (30 * j)) & 0x3FFFFFFF) + c
        t[j] = bal30(u) if j < 12 else u
        c = (u + H) >> 30
    assert val(t) == v
    return mul30s(t, C["F30S_C396"])


def to_m(v):
    return limbs(v * R390 % Q)


def from_m(l):
    return val(l) * pow(R390, -1, Q) % Q


# ---------------------------------------------------------------- constants
def test_constants():
    assert val(QL) == Q and all(-H <= x < H for x in QL[:12])
    assert (QINV * Q) % 2**30 == 2**30 - 1 and -H <= QINV < H
    assert val(C["F30S_ONE"]) == R390 % Q
    for name, e in (("F30S_C384", 384), ("F30S_C396", 396), ("F30S_C406", 406)):
        assert val(C[name]) == 2**e % Q
        assert all(-H <= x < H for x in C[name][:12])


# ---------------------------------------------------------------- column bounds
def _column_bounds(kind):
    """Largest possible |accumulator| of each routine from magnitudes alone:
    every operand limb, every m_i and every limb of q taken as 2^29 (doubled
    limbs of the square as 2^30), all products with one sign."""
    peak, carry = 0, 0
    for k in range(25):
        n = k + 1 if k < 13 else 25 - k  # operand products in the column
        red = (min(k, 13) - max(0, k - 12)) + (1 if k < 13 else 0)
        if kind == "mul":
            ops = n * H * H
        elif kind == "mul2":
            ops = 2 * n * H * H
        else:  # cross terms once against a doubled limb, the square on even k
            ops = (n // 2) * H * (2 * H) + (H * H if k % 2 == 0 else 0)
        if kind == "mul2" and heavy(k):
            peak = max(peak, carry + ops)
            hi = ((carry + ops) >> 30) + 1
            peak = max(peak, H + red * H * H)
            carry = ((H + red * H * H) >> 30) + 1 + hi
        else:
            peak = max(peak, carry + ops + red * H * H)
            carry = ((carry + ops + red * H * H) >> 30) + 1
        peak = max(peak, carry)
    return peak


def test_worst_case_columns():
    for kind in ("mul", "sqr", "mul2"):
        assert _column_bounds(kind) < 2**63, kind
    # the two-product form needs its mid-column carry: without it 39 products
    assert 39 * H * H > 2**63
    # and the model itself (asserting every partial sum) at the limb extremes,
    # all signs: the top limb at +-2^29 too (beyond the value range the results
    # are exact for, the columns must still hold)
    for sa in (-H, H):
        for sb in (-H, H):
            a, b = [sa] * 13, [sb] * 13
            pk = []
            mul30s(a, b, pk)
            sqr30s(a, pk)
            mul2_30s(a, b, a, b, pk)
            mul2_30s(a, b, neg30s(a), neg30s(b), pk)
            assert max(pk) <= _column_bounds("mul2")
    alt = [H if i % 2 else -H for i in range(13)]
    mul2_30s(alt, alt, alt, alt)
    sqr30s(alt)


# ---------------------------------------------------------------- exactness
def _extremes():
    top = 2**385 - 1
    out = [0, 1, -1, top, -top, Q, -Q, val([-H] * 12 + [2**24]), val([H - 1] * 12 + [-2**24])]
    out += [val([H if i % 2 else -H for i in range(12)] + [s * 2**24]) for s in (1, -1)]
    return out


def test_mul_exact_and_bounded():
    rnd = random.Random(1)
    ir = pow(R390, -1, Q)
    cases = [(a, b) for a in _extremes() for b in _extremes()]
    cases += [(rnd.randrange(-2**385, 2**385), rnd.randrange(-2**385, 2**385)) for _ in range(300)]
    for a, b in cases:
        la, lb = limbs(a), limbs(b)
        assert val(la) == a
        r = mul30s(la, lb)
        assert (val(r) - a * b * ir) % Q == 0 and abs(val(r)) < 2**381
        assert all(-H <= x < H for x in r[:12])
        assert val(sqr30s(la)) == val(mul30s(la, la))
        c, d = rnd.randrange(-2**385, 2**385), rnd.randrange(-2**385, 2**385)
        t = mul2_30s(la, lb, limbs(c), limbs(d))
        # two products of < 2^770: 2^381 + q/2 (the mixed addition's operands are
        # smaller, test_madd_intervals)
        assert (val(t) - (a * b + c * d) * ir) % Q == 0 and abs(val(t)) < 2**382


def test_sub_neg():
    rnd = random.Random(2)
    for _ in range(200):
        a, b, c = (limbs(rnd.randrange(-2**385, 2**385)) for _ in range(3))
        assert val(sub30s(a, b)) == val(a) - val(b)
        assert val(sub2_30s(a, b, c)) == val(a) - val(b) - val(c)
        assert val(neg30s(a)) == -val(a)
    lo, hi = [-H] * 12 + [0], [H] * 12 + [0]  # hi: a negated limb may be 2^29
    for a, b, c in ((lo, hi, hi), (hi, lo, lo), (lo, lo, lo), (hi, hi, hi)):
        r = sub2_30s(a, b, c)
        assert all(-H <= x < H for x in r[:12])
        sub30s(a, b)


# ---------------------------------------------------------------- conversions
def test_table_form_round_trip():
    rnd = random.Random(3)
    for x in [0, 1, Q - 1, Q // 2, Q // 2 + 1] + [rnd.randrange(Q) for _ in range(100)]:
        canon = x * 2**384 % Q  # what the key holds (field.cuh R384 form)
        t = to_f30s(canon)
        assert abs(val(t)) < 2**381 and all(-H <= l < H for l in t[:12])
        assert from_m(t) == x
        assert to_fq32(t) == canon
        assert to_fq32(neg30s(t)) == (-canon) % Q


def test_piece_form():
    rnd = random.Random(4)
    vals = [0, Q, -Q, 2 * Q, 2**383 - 1, -(2**383 - 1)] + [rnd.randrange(-2**383, 2**383) for _ in range(100)]
    for v in vals:
        p = to_f29(limbs(v))
        assert all(0 <= l < 2**29 for l in p)
        pv = sum(l << (29 * i) for i, l in enumerate(p))
        assert 0 < pv < 2 * Q < 2**382  # a product output of ec29.cuh
        assert from_m29(p) == from_m(limbs(v))
        if v % Q == 0:
            assert pv == Q  # zero29 tests 0, q, 2q limb for limb


# ---------------------------------------------------------------- mixed addition
def madd30s(p, x2, y2):
    """madd30s of ec30s.cuh"""
    X, Y, ZZ, ZZZ = p
    u2, s2 = mul30s(x2, ZZ), mul30s(y2, ZZZ)
    P, R = sub30s(u2, X), sub30s(s2, Y)
    pp = sqr30s(P)
    ppp = mul30s(P, pp)
    q = mul30s(X, pp)
    x3 = sub30s(sub2_30s(sqr30s(R), ppp, q), q)
    y3 = mul2_30s(R, sub30s(q, x3), Y, neg30s(ppp))
    for v in (u2, s2, pp, ppp, q, y3):
        assert abs(val(v)) < 2**381
    for v in (P, R, x3, sub30s(q, x3)):
        assert abs(val(v)) < 2**385
    return x3, y3, mul30s(ZZ, pp), mul30s(ZZZ, ppp)


def test_madd_intervals():
    """Magnitude bounds through the formula, by induction: a product of
    |a| <= A, |b| <= B is at most (A B + M q) / 2^390 with |M| <= 2^29 sum
    2^(30 i).  If the accumulator holds |X| < 2^383 and |Y|, |ZZ|, |ZZZ| <
    2^381, every product input stays inside the range the model is exact for
    (< 2^385) and the new accumulator holds the same bounds again, so they
    hold after any number of additions."""
    M = H * sum(1 << (30 * i) for i in range(13))

    def prod(a, b, c=0, d=0):
        assert max(a, b, c, d) < 2**385
        return -(-(a * b + c * d + M * Q) // R390)

    T = prod(Q, Q)  # a table coordinate: to_f30s of a canonical value by C396 < q
    assert T < 2**381 and Q < 2**381  # a fresh accumulator: the point, ZZ = ZZZ = ONE < q
    X, Y, ZZ, ZZZ = 2**383, 2**381, 2**381, 2**381
    u2, s2 = prod(T, ZZ), prod(T, ZZZ)
    P, R = u2 + X, s2 + Y
    pp = prod(P, P)
    ppp, q = prod(P, pp), prod(X, pp)
    x3 = prod(R, R) + ppp + 2 * q
    y3 = prod(R, q + x3, Y, ppp)
    assert max(u2, s2, pp, ppp, q) < 2**381
    assert x3 < X and max(y3, prod(ZZ, pp), prod(ZZZ, ppp)) < 2**381
    # a piece leaves through to_f29 / to_fq32: |C| < q, result inside (-q, q)
    assert prod(X, Q) < Q


@pytest.mark.parametrize("seed", [3, 4])
def test_madd_chain(seed):
    rnd = random.Random(seed)
    pts = [_mulg(rnd.randrange(1, 2**64)) for _ in range(24)]
    ref = pts[0]
    tab = lambda v: to_f30s(v * 2**384 % Q)  # noqa: E731  the table's form
    acc = (tab(pts[0][0]), tab(pts[0][1]), C["F30S_ONE"], C["F30S_ONE"])
    for x, y in pts[1:]:
        ym = tab(y)
        if rnd.random() < 0.5:
            ym, y = neg30s(ym), (-y) % Q
        acc = madd30s(acc, tab(x), ym)
        ref = aff_add(ref, (x, y))
    X, Y, ZZ, ZZZ = (from_m29(to_f29(v)) for v in acc)  # as the piece is stored
    assert X * pow(ZZ, -1, Q) % Q == ref[0]
    assert Y * pow(ZZZ, -1, Q) % Q == ref[1]
    # equal points make ZZ = 0 mod q, which the stored piece shows as q
    x, y = pts[5]
    one = (tab(x), tab(y), C["F30S_ONE"], C["F30S_ONE"])
    dbl = madd30s(one, tab(x), tab(y))
    assert sum(l << (29 * i) for i, l in enumerate(to_f29(dbl[2]))) == Q
    opp = madd30s(one, tab(x), neg30s(tab(y)))
    assert sum(l << (29 * i) for i, l in enumerate(to_f29(opp[2]))) == Q
