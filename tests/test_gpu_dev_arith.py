"""The device field and curve routines themselves, run alone at the limb edges.

tests/native/dev_arith.hip (built by csrc/Makefile into lib/dev_arith) runs each
device routine of field30s.cuh, ec30s.cuh, field29.cuh, ec29.cuh, fr29.cuh and
the device halves of field.cuh and ec.cuh, one kernel per routine and one lane
per case, on operands read from a file.  The cases are the edge lists of the
Python models (test_field30s, test_field29, test_fr29: imported, not restated)
and a few more: limbs at +-2^29, carries that ripple through every limb, exact
multiples of q, three-term limb sums at 3 2^29, the top R29 limb at 2^32 - 1,
values next to the moduli.  Every result word is compared, exactly, with

  1. plain Python integers (congruence with the right Montgomery factor, the
     exact value where the routine is canonical, the affine sum for points),
  2. the output contract the header documents (limb ranges, value bounds),
  3. the limb-for-limb model where one exists (all of F30s, F29, R29, the
     radix-2^29 point formulas); the canonical routines have one exact answer,
     which the integers give.

test_cases_hold_on_cpu runs every case through the models (their asserts live)
and the integer checks without a GPU: the inputs are inside every contract and
the reference alone satisfies 1 and 2.  The GPU tests run the same cases, all of
them, through one harness process."""
import functools
import os
import random
import subprocess
from array import array

import pytest

import test_field29 as m29
import test_field30s as m30
import test_fr29 as mr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zprize23-gpu-submission_amd", "csrc")
BIN = os.path.join(HERE, "..", "zprize23-gpu-submission_amd", "lib", "dev_arith")

Q, R = m30.Q, mr.R
H = m30.H
M32 = 0xFFFFFFFF
M29 = m29.M29
IR390, IR406 = pow(m30.R390, -1, Q), pow(m29.R406, -1, Q)
C30, C29, CR = m30.C, m29.C, mr.C
CHAIN_MAX = 24


# ---------------------------------------------------------------- words
def s32(w):
    return w - (1 << 32) if w >> 31 else w


def dec30(w):
    return [s32(x) for x in w]


def enc(l):
    assert all(-2**31 <= x < 2**32 for x in l)
    return [x & M32 for x in l]


def words(v, n):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & M32 for i in range(n)]


def unwords(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def split(w, n):
    return [w[i:i + n] for i in range(0, len(w), n)]


class Op:
    """one device routine: its id and widths in tests/native/dev_arith.hip, its
    cases (tag, operand words), the expected result words (limb model or exact
    integers) and the integer / contract checks on a result"""

    def __init__(self, header, name, oid, wi, wo, model, props):
        self.header, self.name, self.oid, self.wi, self.wo = header, name, oid, wi, wo
        self.model, self.props, self.cases = model, props, []

    def add(self, tag, *operands):
        w = [x for o in operands for x in o]
        assert len(w) == self.wi, (self.name, tag, len(w))
        self.cases.append((tag, enc(w)))


# ================================================================ field30s.cuh
def in385(*ops):
    return all(abs(m30.val(a)) < 2**385 for a in ops)


def bal_ok(l):
    return all(-H <= x < H for x in l[:12])


def _p_prod30(n, bound):
    def props(w, out):
        ops, r = [dec30(x) for x in split(w, 13)], dec30(out)
        assert bal_ok(r)
        if in385(*ops):  # beyond it (a top limb at +-2^29) only the model speaks
            v = [m30.val(a) for a in ops]
            want = v[0] * v[0] if n == 1 else v[0] * v[1] + (v[2] * v[3] if n == 4 else 0)
            assert (m30.val(r) - want * IR390) % Q == 0
            assert abs(m30.val(r)) < bound
    return props


def _p_lin30(f):
    def props(w, out):
        ops, r = [dec30(x) for x in split(w, 13)], dec30(out)
        assert m30.val(r) == f(*[m30.val(a) for a in ops])
        assert all(-H <= x <= H for x in r[:12]) if len(ops) == 1 else bal_ok(r)
    return props


def _m_to_f30s(w):
    t = m30.to_f30s(unwords(w))
    return enc(t) + words(m30.to_fq32(t), 12) + words(m30.to_fq32(m30.neg30s(t)), 12)


def _p_to_f30s(w, out):
    canon, t = unwords(w), dec30(out[:13])
    assert abs(m30.val(t)) < 2**381 and bal_ok(t)
    assert m30.from_m(t) == canon * pow(2**384, -1, Q) % Q
    assert unwords(out[13:25]) == canon and unwords(out[25:37]) == (-canon) % Q


def _p_f30s_to_fq32(w, out):
    assert unwords(out) == m30.val(dec30(w)) * 2**384 * IR390 % Q


def _p_to_f29(w, out):
    v = m30.val(dec30(w))
    assert all(0 <= l < 2**29 for l in out)
    assert 0 < m29.val(out) < 2 * Q
    assert m29.from_m(out) == v * IR390 % Q
    if v % Q == 0:
        assert out == m29.limbs(Q)  # zero29 tests 0, q, 2q limb for limb


def zero29(l):
    return l in (m29.limbs(0), m29.limbs(Q), m29.limbs(2 * Q))


def _p_zero29(w, out):
    assert m29.val(w) < 2**382 and all(x < 2**29 for x in w)  # a product output or F29_ONE
    assert out == [int(m29.val(w) % Q == 0)]


def _chain_entries(w):
    n = w[0]
    assert 1 <= n <= CHAIN_MAX
    return [(dec30(e[:13]), dec30(e[13:])) for e in split(w[1:], 26)[:n]]


def _m_chain(w):
    ent = _chain_entries(w)
    acc = (ent[0][0], ent[0][1], C30["F30S_ONE"], C30["F30S_ONE"])
    for x, y in ent[1:]:
        acc = m30.madd30s(acc, x, y)
    p = [m30.to_f29(c) for c in acc]
    return p[0] + p[1] + p[2] + p[3] + [int(not zero29(p[2])), 0, 0, 0]


def _p_chain(w, out):
    pts = [(m30.from_m(x), m30.from_m(y)) for x, y in _chain_entries(w)]
    ref, degenerate = pts[0], False
    for p in pts[1:]:
        if degenerate or p[0] == ref[0]:
            degenerate = True  # an equal or opposite step: ZZ = 0 mod q from there on
        else:
            ref = m29.aff_add(ref, p)
    X, Y, ZZ, ZZZ = split(out[:56], 14)
    assert all(0 <= l < 2**29 for l in out[:56]) and out[57:] == [0, 0, 0]
    if degenerate:
        assert out[56] == 0 and ZZ == m29.limbs(Q)
    else:
        assert out[56] == 1
        assert m29.from_m(X) * pow(m29.from_m(ZZ), -1, Q) % Q == ref[0]
        assert m29.from_m(Y) * pow(m29.from_m(ZZZ), -1, Q) % Q == ref[1]


COLUMN12_PAST_2E63 = (
    ([-536870912, -536870912, 536870912, -536867878, 536870284, 536870792, 536870909, 536870912, 535482366,
      -536870774, 536856764, -536869652, 536870911],
     [536870912, -536870912, 533236764, -536869229, 536870912, 536870912, 535283630, 536860225, 536346074,
      -536870912, 536720553, -536805376, -536870912],
     [536870912, -536870912, 536870912, 536870912, -536870912, -536870315, -536784780, 536870897, 536346624,
      -536870250, 535181686, 536869198, -536870912],
     [-536870912, 536870912, 536870912, -536870912, 536870912, 536854371, -536847476, -536870656, -536608036,
      536867560, 536863387, -536869026, 536870912]),
    ([-536870912, -536870912, 536870912, -536867878, 536870284, 536870792, 536870909, 536870912, 535482366,
      -536870710, 536857401, -536870650, 536870912],
     [536870912, -536870912, 533236764, -536869229, 536870912, 536870912, 535283630, 536860225, 536870362,
      -536870912, 535050445, -536870912, -536870912],
     [536870912, -536870912, 536870912, 536870912, -536870912, -536870315, -536784780, 536870897, 536412160,
      -536853878, 536398604, 536870908, -536870912],
     [-536870912, 536870912, 536870912, -536870912, 536870912, 536854371, -536847476, -536870656, -536837412,
      536867536, 536867759, -536869978, 536870912]),
)


def tab30(v):
    """an affine coordinate in the folded table's form"""
    return m30.to_f30s(v * 2**384 % Q)


def _cases_f30s(ops):
    rnd = random.Random(101)
    L = m30.limbs
    r385 = lambda: L(rnd.randrange(-2**385 + 1, 2**385))  # noqa: E731
    ext = [L(v) for v in m30._extremes()]
    worst = [[s] * 13 for s in (-H, H)]
    alt = [H if i % 2 else -H for i in range(13)]
    big = [[s * H] * 12 + [2**25 - 1] for s in (1, -1)] + [[s * H] * 12 + [-(2**25 - 1)] for s in (1, -1)]
    mul, sqr, mul2 = ops["mul30s"], ops["sqr30s"], ops["mul2_30s"]
    for i, a in enumerate(ext):
        for j, b in enumerate(ext):
            mul.add(f"extreme{i}x{j}", a, b)
            c, d = ext[(i + 3) % 11], ext[(j + 7) % 11]
            mul2.add(f"extreme{i}x{j}+{(i + 3) % 11}x{(j + 7) % 11}", a, b, c, d)
            mul2.add(f"extreme{i}x{j}+random", a, b, r385(), r385())
        sqr.add(f"extreme{i}", a)
    for a in worst:
        sqr.add(f"all{a[0]:+d}", a)
        for b in worst:
            mul.add(f"all{a[0]:+d}x{b[0]:+d}", a, b)
            mul2.add(f"all{a[0]:+d}x{b[0]:+d}twice", a, b, a, b)
            mul2.add(f"all{a[0]:+d}x{b[0]:+d}+negated", a, b, m30.neg30s(a), m30.neg30s(b))
    alts = [("alternating", alt), ("-alternating", m30.neg30s(alt))]
    for ta, a in alts:
        sqr.add(ta, a)
        for tb, b in alts + [(f"all{w[0]:+d}", w) for w in worst]:
            for x, y, tag in ((a, b, f"{ta}x{tb}"), (b, a, f"{tb}x{ta}")):
                mul.add(tag, x, y)
                mul2.add(f"{tag}twice", x, y, x, y)
                mul2.add(f"{tag}+negated", x, y, m30.neg30s(x), m30.neg30s(y))
    for i, a in enumerate(big):
        sqr.add(f"largest{i}", a)
        for j, b in enumerate(big):
            mul.add(f"largest{i}x{j}", a, b)
            for k in range(4):
                mul2.add(f"largest{i}x{j}+{k}x{(i + k) % 4}", a, b, big[k], big[(i + k) % 4])
            mul2.add(f"largest{i}x{j}+negated", a, b, m30.neg30s(a), m30.neg30s(b))
    # column 12 of a b + c d with every limb next to +-2^29, the 26 operand
    # products of one sign and the twelve m_i lined up with the limbs of q: the
    # column's products alone sum past 2^63 (1.00002 and 1.000005 times), which
    # the carry taken out in mid-column is for (found by a local search over
    # such operands; no sign pattern of exact +-2^29 limbs gets there)
    for n, quad in enumerate(COLUMN12_PAST_2E63):
        mul2.add(f"column12_past_2e63_{n}", *quad)
        mul.add(f"column12_past_2e63_{n}:ab", quad[0], quad[1])
        mul.add(f"column12_past_2e63_{n}:cd", quad[2], quad[3])
    for _ in range(300):
        mul.add("random", r385(), r385())
        sqr.add("random", r385())
        mul2.add("random", r385(), r385(), r385(), r385())

    lo, hi = [-H] * 12 + [0], [H] * 12 + [0]  # hi: a negated limb may be 2^29
    name = {id(lo): "lo", id(hi): "hi"}
    for a in (lo, hi):
        ops["neg30s"].add(name[id(a)], a)
        for b in (lo, hi):
            ops["sub30s"].add(f"{name[id(a)]}-{name[id(b)]}", a, b)
            for c in (lo, hi):  # a - b - c: limb sums of +-3 2^29 with the carry
                ops["sub2_30s"].add(f"{name[id(a)]}-{name[id(b)]}-{name[id(c)]}", a, b, c)
    for i, a in enumerate(ext):
        ops["neg30s"].add(f"extreme{i}", a)
        ops["sub30s"].add(f"extreme{i}-{(i + 4) % 11}", a, ext[(i + 4) % 11])
        ops["sub2_30s"].add(f"extreme{i}-{(i + 4) % 11}-{(i + 9) % 11}", a, ext[(i + 4) % 11], ext[(i + 9) % 11])
    for _ in range(200):
        ops["neg30s"].add("random", r385())
        ops["sub30s"].add("random", r385(), r385())
        ops["sub2_30s"].add("random", r385(), r385(), r385())

    win = lambda x: sum(x << (30 * i) for i in range(12))  # noqa: E731
    tf = ops["to_f30s"]
    for tag, x in (("x=0", 0), ("x=1", 1), ("x=q-1", Q - 1), ("x=q//2", Q // 2), ("x=q//2+1", Q // 2 + 1)):
        tf.add(tag, words(x * 2**384 % Q, 12))
    for tag, v in (("windows_3fffffff", win(0x3FFFFFFF)), ("windows_2e29", win(H)), ("windows_2e29-1", win(H - 1)),
                   ("windows_3fffffff_top", win(0x3FFFFFFF) + (((Q >> 360) - 1) << 360)),
                   ("0", 0), ("1", 1), ("q-1", Q - 1)):
        tf.add(tag, words(v, 12))
    for _ in range(100):
        tf.add("random", words(rnd.randrange(Q), 12))

    piece = [("0", 0), ("2e383-1", 2**383 - 1), ("-(2e383-1)", -(2**383 - 1))]
    piece += [(f"{k}q", k * Q) for k in range(-2, 4) if k]
    piece += [("q+1", Q + 1), ("q-1", Q - 1), ("-q+1", 1 - Q), ("1", 1), ("-1", -1)]
    piece += [("random", rnd.randrange(-2**383 + 1, 2**383)) for _ in range(100)]
    for tag, v in piece:
        ops["f30s_to_fq32"].add(tag, L(v))
        ops["to_f29"].add(tag, L(v))

    ch = ops["chain30s"]

    def chain(tag, ent):
        pad = [[0] * 13, [0] * 13]
        ch.add(tag, [len(ent)], *[c for e in ent + [pad] * (CHAIN_MAX - len(ent)) for c in e])

    for seed in (3, 4):  # the chains of test_field30s.test_madd_chain
        r2 = random.Random(seed)
        pts = [m29._mulg(r2.randrange(1, 2**64)) for _ in range(24)]
        ent = [[tab30(pts[0][0]), tab30(pts[0][1])]]
        for x, y in pts[1:]:
            ym = tab30(y)
            ent.append([tab30(x), m30.neg30s(ym) if r2.random() < 0.5 else ym])
        chain(f"chain{seed}", ent)
        for n in (1, 2, 3, 23):
            chain(f"chain{seed}[:{n}]", ent[:n])
        (x, y), (x2, y2) = pts[5], pts[6]
        a, b = [tab30(x), tab30(y)], [tab30(x2), tab30(y2)]
        s = m29.aff_add((x, y), (x2, y2))
        chain(f"doubling{seed}", [a, a])
        chain(f"opposite{seed}", [a, [a[0], m30.neg30s(a[1])]])
        chain(f"doubling_late{seed}", [a, b, [tab30(s[0]), tab30(s[1])]])
        chain(f"opposite_late{seed}", [a, b, [tab30(s[0]), tab30(Q - s[1])]])
        chain(f"doubling_then_more{seed}", [a, a, b] + ent[8:12])


# ================================================================ field29.cuh
def _p_prod29(n):
    def props(w, out):
        v = [m29.val(x) for x in split(w, 14)]
        want = v[0] * v[0] if n == 1 else v[0] * v[1] + (v[2] * v[3] if n == 4 else 0)
        assert all(0 <= l < 2**29 for l in out) and (m29.val(out) - want * IR406) % Q == 0
        if all(x < 2**391 for x in v):  # beyond it (limb 13 at 2^29 - 1) the columns still hold, the bound need not
            assert m29.val(out) < 2**382
    return props


def neg29(b, K):
    return m29.sub29([0] * 14, b, K)


def _p_sub29(K, neg=False):
    def props(w, out):
        v = [m29.val(x) for x in split(w, 14)]
        assert m29.val(out) == (0 if neg else v[0]) + m29.val(K) - v[-1]
        assert all(0 <= l < 2**29 for l in out[:13]) and 0 <= out[13] <= M32
    return props


def unpack29(l):
    v = m29.val(l)
    assert v < 2 * Q and all(x < 2**29 for x in l)
    return words(v - Q if v >= Q else v, 12)


def _m_f29_to_fq32(w):
    return unpack29(m29.mul29(w, C29["F29_C384"]))


def _m_from_fq32(w):
    assert unwords(w) < Q
    return m29.mul29(m29.limbs(unwords(w)), C29["F29_C428"])


def _p_from_fq32(w, out):
    assert all(0 <= l < 2**29 for l in out) and m29.val(out) < 2 * Q
    assert (m29.val(out) - unwords(w) * 2**22) % Q == 0


def _cases_f29(ops):
    rnd = random.Random(102)
    L = m29.limbs
    r391 = lambda: L(rnd.randrange(2**391))  # noqa: E731
    top = L(2**391 - 1)
    single = [[M29 if j == i else 0 for j in range(14)] for i in range(14)]
    mul, sqr, mul2 = ops["mul29"], ops["sqr29"], ops["mul2_29"]
    mul.add("top_x_top", top, top)
    mul.add("top_x_random", top, r391())
    mul.add("random_x_top", r391(), top)
    mul.add("0_x_top", L(0), top)
    sqr.add("top", top)
    sqr.add("0", L(0))
    mul2.add("top_everywhere", top, top, top, top)
    for k in range(4):
        o = [r391() for _ in range(4)]
        o[k] = top
        mul2.add(f"top_in_slot{k}", *o)
    for i, s in enumerate(single):
        mul.add(f"limb{i}_x_top", s, top)
        mul.add(f"top_x_limb{i}", top, s)
        mul.add(f"limb{i}_x_limb{13 - i}", s, single[13 - i])
        mul.add(f"limb{i}_x_random", s, r391())
        sqr.add(f"limb{i}", s)
        mul2.add(f"limb{i}_top_top_limb{i}", s, top, top, s)
        mul2.add(f"limb{i}_limb{13 - i}_random", s, single[13 - i], r391(), r391())
    for _ in range(300):
        mul.add("random", r391(), r391())
        sqr.add("random", r391())
        mul2.add("random", r391(), r391(), r391(), r391())

    for k, e in (("ka", 386), ("kb", 389)):
        K = C29[f"F29_K{k[1].upper()}"]
        bs = [("0", 0), ("1", 1), ("max", 2**e - 1), ("2e377", 2**377), ("2e377-1", 2**377 - 1)]
        bs += [("random", rnd.randrange(2**e)) for _ in range(30)]
        for tb, b in bs:
            ops[f"neg29_{k}"].add(f"b={tb}", L(b))
            for ta, a in (("0", 0), ("max", 2**389 - 1), ("random", rnd.randrange(2**389))):
                ops[f"sub29_{k}"].add("random" if (ta, tb) == ("random", "random") else f"a={ta},b={tb}", L(a), L(b))
        assert m29.val(K) >= 2**e

    ints = [("0", 0), ("1", 1), ("2e384-1", 2**384 - 1), ("q-1", Q - 1), ("q", Q), ("2q-1", 2 * Q - 1)]
    ints += [(f"bit{b}", 1 << b) for b in sorted(set(range(0, 384, 29)) | set(range(0, 384, 32)))]
    ints += [("random", rnd.randrange(2**384)) for _ in range(50)]
    for tag, v in ints:
        ops["repack29"].add(tag, words(v, 12))
    for tag, v in [("0", 0), ("1", 1), ("q-1", Q - 1), ("q", Q), ("q+1", Q + 1), ("2q-1", 2 * Q - 1)] + \
            [("random", rnd.randrange(2 * Q)) for _ in range(50)]:
        ops["unpack29"].add(tag, L(v))
    for tag, a in [("top", top), ("0", L(0)), ("one", C29["F29_ONE"])] + [(f"{k}q", L(k * Q)) for k in (1, 2, 3)] + \
            [(f"limb{i}", s) for i, s in enumerate(single)] + [("random", r391()) for _ in range(50)]:
        ops["f29_to_fq32"].add(tag, a)
    for tag, v in [("0", 0), ("1", 1), ("q-1", Q - 1), ("q/2", Q // 2), ("low_words_ffffffff", (Q >> 352 << 352) - 1)] + \
            [("random", rnd.randrange(Q)) for _ in range(50)]:
        ops["from_fq32"].add(tag, words(v, 12))


# ================================================================ ec29.cuh
def _aff29(p):
    return m29._aff(p)


def _m_xadd29_inf(w):
    p, q = split(w[:56], 14), split(w[56:], 14)
    if zero29(p[2]):
        return [x for c in q for x in c] + [0]
    if zero29(q[2]):
        return [x for c in p for x in c] + [0]
    r = m29.xadd29(p, q)
    return [x for c in r for x in c] + [int(zero29(r[2]))]


def _p_xadd29_inf(w, out):
    p, q = split(w[:56], 14), split(w[56:], 14)
    if zero29(p[2]) or zero29(q[2]):  # the other operand as it is
        assert out == (w[56:] if zero29(p[2]) else w[:56]) + [0]
        return
    a, b = _aff29(p), _aff29(q)
    if a[0] == b[0]:  # equal or opposite: reported, the result is redone elsewhere
        assert out[56] == 1
        return
    assert out[56] == 0 and _aff29(split(out[:56], 14)) == m29.aff_add(a, b)
    X, Y, ZZ, ZZZ = split(out[:56], 14)
    assert m29.val(X) < 2**389 and m29.val(Y) < 2**382 and m29.val(ZZ) < 2**382 and m29.val(ZZZ) < 2**382


def _m_xdbl29_inf(w):
    p = split(w, 14)
    return w if zero29(p[2]) else [x for c in m29.xdbl29(p) for x in c]


def _p_xdbl29_inf(w, out):
    p = split(w, 14)
    if zero29(p[2]):
        assert out == w
        return
    assert _aff29(split(out, 14)) == m29._dbl_aff(_aff29(p))
    assert m29.val(out[:14]) < 2**389 and all(m29.val(c) < 2**382 for c in split(out[14:], 14))


def _m_to32(w):
    return [x for c in split(w, 14) for x in _m_f29_to_fq32(c)]


def _p_to32(w, out):
    for c, o in zip(split(w, 14), split(out, 12)):
        assert unwords(o) == m29.val(c) * 2**384 * IR406 % Q


def _m_from32(w):
    c = split(w, 12)
    return [0] * 56 if unwords(c[2]) == 0 else [x for v in c for x in _m_from_fq32(v)]


def _p_from32(w, out):
    if unwords(w[24:36]) == 0:
        assert out == [0] * 56
        return
    for c, o in zip(split(w, 12), split(out, 14)):
        _p_from_fq32(c, o)


def point29(k, z, lx=0, ly=0, neg=False):
    """k G as (x z^2, y z^3, z^2, z^3) in the R406 form, X and Y lifted by
    multiples of q (stored coordinates are < 2^389), ZZ and ZZZ as mul29 leaves
    them"""
    x, y = m29._mulg(k)
    if neg:
        y = Q - y
    zl = m29.to_m(z)
    zz = m29.mul29(zl, zl)
    zzz = m29.mul29(zz, zl)
    X, Y = x * z * z * m29.R406 % Q + lx * Q, y * z**3 * m29.R406 % Q + ly * Q
    assert X < 2**389 and Y < 2**389
    return m29.limbs(X) + m29.limbs(Y) + zz + zzz


def _cases_ec29(ops):
    rnd = random.Random(103)
    L = m29.limbs
    z = ops["zero29"]
    qb = L(Q)
    for tag, v in (("0", 0), ("q", Q), ("2q", 2 * Q), ("q+1", Q + 1), ("q-1", Q - 1), ("2q+1", 2 * Q + 1),
                   ("2q-1", 2 * Q - 1), ("1", 1), ("2e382-1", 2**382 - 1)):
        z.add(tag, L(v))
    z.add("one", C29["F29_ONE"])
    for i in range(14):
        for base, name in ((Q, "q"), (2 * Q, "2q")):
            l = L(base)
            l[i] ^= 1 << ((5 * i + 3) % (29 if i < 13 else 4))
            z.add(f"{name}_flip_limb{i}", l)
        l = [0] * 14
        l[i] = 1 << ((7 * i) % (29 if i < 13 else 4))
        z.add(f"0_flip_limb{i}", l)
    for _ in range(20):
        z.add("random", L(rnd.randrange(2**382)))

    ks = [rnd.randrange(1, 2**64) for _ in range(6)]
    zr = lambda: rnd.randrange(1, Q)  # noqa: E731
    lifts = [(0, 0), (1, 0), (0, 1), (300, 300), (100, 7), (299, 1)]
    P = [point29(k, zr(), *lifts[i]) for i, k in enumerate(ks)]
    inf0 = [0] * 56
    infq = point29(ks[0], zr(), 300, 300)[:28] + qb + L(2 * Q)  # ZZ = q limb for limb: infinity too
    inf2q = point29(ks[1], zr())[:28] + L(2 * Q) + qb
    xa, xd, t32 = ops["xadd29_inf"], ops["xdbl29_inf"], ops["to32"]
    for i, p in enumerate(P):
        for j, q in enumerate(P):
            if i != j:
                xa.add(f"P{i}+P{j}", p, q)
        xa.add(f"P{i}+P{i}", p, p)
        xa.add(f"P{i}+P{i}_other_z", p, point29(ks[i], zr(), 17, 250))
        xa.add(f"P{i}+(-P{i})", p, point29(ks[i], zr(), 3, 300, neg=True))
        xa.add(f"P{i}+(-P{i})_same_z", p, p[:14] + L(301 * Q - m29.val(p[14:28])) + p[28:])
        for tn, n in (("inf0", inf0), ("infq", infq), ("inf2q", inf2q)):
            xa.add(f"P{i}+{tn}", p, n)
            xa.add(f"{tn}+P{i}", n, p)
        xd.add(f"2P{i}", p)
        t32.add(f"P{i}", p)
    for tn, n in (("inf0", inf0), ("infq", infq), ("inf2q", inf2q)):
        xd.add(tn, n)
        for tm, m in (("inf0", inf0), ("infq", infq)):
            xa.add(f"{tn}+{tm}", n, m)
    t32.add("inf0", inf0)
    t32.add("top", *[L(2**389 - 1)] * 2, *[L(2**382 - 1)] * 2)
    # sums and doubles as operands again: X as the three subtractions leave it
    for i in range(3):
        s = _m_xadd29_inf(P[i] + P[i + 1])[:56]
        d = _m_xdbl29_inf(P[i + 2])
        xa.add(f"(P{i}+P{i + 1})+2P{i + 2}", s, d)
        xd.add(f"2(P{i}+P{i + 1})", s)
        t32.add(f"P{i}+P{i + 1}", s)

    f32 = ops["from32"]
    for i, k in enumerate(ks):
        f32.add(f"P{i}", point32(k, zr() if i else 1))
    f32.add("inf", words(2**384 % Q, 12) * 2 + [0] * 24)
    f32.add("inf_junk_xy", point32(ks[0], 5)[:24] + [0] * 12 + words(7, 12))
    f32.add("q-1", *[words(Q - 1, 12)] * 4)


# ================================================================ fr29.cuh
def norm_r29(l):
    return mr.norm_ok(l)


def r29_from_words(w):
    return mr.from_fr(unwords(w))


def _m_r29_to_words(w):
    v = mr.val(w)
    assert norm_r29(w) and v < 2**256
    return words(v, 8)


def _p_r29_lin(f):
    def props(w, out):
        assert norm_r29(out) and mr.val(out) == f(*[mr.val(x) for x in split(w[:18], 9)], *w[18:])
    return props


def _p_r29_prod(n):
    def props(w, out):
        v = [mr.val(x) for x in split(w, 9)]
        want = v[0] * v[1] + (v[2] * v[3] if n == 4 else 0)
        assert norm_r29(out) and (mr.val(out) - want * pow(2, -261, R)) % R == 0
        assert mr.val(out) < want // 2**261 + R + 1
    return props


def _p_r29_canon(w, out):
    assert norm_r29(out) and mr.val(out) == mr.val(w) % R


def _cases_r29(ops):
    rnd = random.Random(104)
    L = mr.limbs
    conv = [("0", 0), ("2e256-1", 2**256 - 1), ("r-1", R - 1)]
    conv += [(f"bit{b}", 1 << b) for b in sorted(set(range(0, 256, 29)) | set(range(0, 256, 32)))]
    conv += [(f"bit{b}-1", (1 << b) - 1) for b in sorted(set(range(29, 256, 29)) | set(range(32, 256, 32)))]
    conv += [("random", rnd.randrange(2**256)) for _ in range(50)]
    for tag, v in conv:
        ops["r29_from_words"].add(tag, words(v, 8))
        ops["r29_to_words"].add(tag, L(v))

    avals = [("0", 0), ("1", 1), ("2e261-1", 2**261 - 1), ("2e263-1", 2**263 - 1), ("low_limbs_full", 2**232 - 1)]
    for ta, a in avals + [("random", rnd.randrange(2**263)) for _ in range(20)]:
        for tb, b in avals + [("random", rnd.randrange(2**263))]:
            ops["r29_add"].add("random" if ta == tb == "random" else f"{ta}+{tb}", L(a), L(b))
        for tb, b in [("0", 0), ("1", 1), ("4r-1", 4 * R - 1), ("r", R), ("random", rnd.randrange(4 * R))]:
            ops["r29_sub_kdit"].add("random" if ta == tb == "random" else f"{ta}-{tb}", L(a), L(b))
        for row in (0, 7):
            K = R << (row + 1)
            for tb, b in [("0", 0), ("1", 1), ("K-1", K - 1), ("K/2", K // 2), ("random", rnd.randrange(K))]:
                ops["r29_sub_kdif"].add("random" if ta == tb == "random" else f"row{row}:{ta}-{tb}",
                                        L(a), L(b), [row])

    top = 2**261 - 1
    pv = [("0", 0), ("1", 1), ("r-1", R - 1), ("r", R), ("2e261-1", top), ("2e232", 2**232), ("low_limbs_full", 2**232 - 1)]
    pv += [(f"limb{i}", M29 << (29 * i)) for i in range(9)]
    for ta, a in pv:
        for tb, b in pv:
            ops["r29_mul"].add(f"{ta}x{tb}", L(a), L(b))
    for ta, a in pv:
        ops["r29_mul2"].add(f"{ta}x2e261-1_twice", L(a), L(top), L(top), L(a))
        ops["r29_mul2"].add(f"{ta}x{ta}+random", L(a), L(a), L(rnd.randrange(top)), L(rnd.randrange(top)))
    for _ in range(300):
        ops["r29_mul"].add("random", L(rnd.randrange(2**261)), L(rnd.randrange(2**261)))
        ops["r29_mul2"].add("random", *[L(rnd.randrange(2**261)) for _ in range(4)])

    cv = [(str(i), v) for i, v in enumerate([0, 1, R - 1, R, R + 1, 2 * R, 3 * R - 1, 2**262, 2**264 - 1, 255 * R,
                                             256 * R - 1])]
    cv = [(f"canon_edge{t}", v) for t, v in cv]
    for k in (1, 2, 3, 255, 256):
        cv += [(f"{k}r{'%+d' % d if d else ''}", k * R + d) for d in (-1, 0, 1) if k * R + d < 2**264]
    for tag, v in cv + [("random", rnd.randrange(2**264)) for _ in range(300)]:
        ops["r29_canon"].add(tag, L(v))
    ops["r29_canon"].add("top_limb_ffffffff_low_full", [M29] * 8 + [M32])
    ops["r29_canon"].add("top_limb_ffffffff_low_0", [0] * 8 + [M32])
    ops["r29_canon"].add("top_limb_0_low_full", [M29] * 8 + [0])


# ================================================================ field.cuh
def _fp_ops(ops, header, pfx, base, p, n):
    Rm = 1 << (32 * n)
    ir = pow(Rm, -1, p)
    un = lambda f: (lambda w: words(f(unwords(w)) % p, n))  # noqa: E731
    bi = lambda f: (lambda w: words(f(unwords(w[:n]), unwords(w[n:])) % p, n))  # noqa: E731

    def props(w, out):
        assert all(unwords(x) < p for x in split(w, n)) and unwords(out) < p

    table = [("add", 2, bi(lambda a, b: a + b)), ("sub", 2, bi(lambda a, b: a - b)), ("neg", 1, un(lambda a: -a)),
             ("dbl", 1, un(lambda a: 2 * a)), ("mul", 2, bi(lambda a, b: a * b * ir)), ("sqr", 1, un(lambda a: a * a * ir)),
             ("inverse", 1, un(lambda a: pow(a, -1, p) * Rm * Rm if a else 0)), ("to_mont", 1, un(lambda a: a * Rm)),
             ("from_mont", 1, un(lambda a: a * ir))]
    for i, (name, k, model) in enumerate(table):
        ops[pfx + name] = Op(header, pfx + name, base + i, k * n, n, model, props)


def _cases_fp(ops, pfx, p, n, seed):
    rnd = random.Random(seed)
    Rm = 1 << (32 * n)
    sp = [("0", 0), ("1", 1), ("p-1", p - 1), ("p-2", p - 2), ("(p-1)/2", (p - 1) // 2), ("(p+1)/2", (p + 1) // 2),
          ("R", Rm % p), ("R2", Rm * Rm % p), ("low_words_ffffffff", (p >> (32 * (n - 1)) << (32 * (n - 1))) - 1)]
    W = lambda v: words(v, n)  # noqa: E731
    for name in ("neg", "dbl", "sqr", "to_mont", "from_mont"):
        for t, v in sp + [("random", rnd.randrange(p)) for _ in range(50)]:
            ops[pfx + name].add(t, W(v))
    for t, v in sp + [("random", rnd.randrange(p)) for _ in range(6)]:
        ops[pfx + "inverse"].add(t, W(v))
    pairs = [(f"{ta},{tb}", a, b) for ta, a in sp for tb, b in sp]
    for _ in range(10):
        a = rnd.randrange(1, p)
        b = rnd.randrange(a, p)
        pairs += [("a+b=p", a, p - a), ("a+b=p-1", a, p - 1 - a), ("a<b", a, b), ("a=b", a, a), ("a+b=p+1", a, p + 1 - a)]
    pairs += [("random", rnd.randrange(p), rnd.randrange(p)) for _ in range(200)]
    for name in ("add", "sub", "mul"):
        for t, a, b in pairs:
            ops[pfx + name].add(t, W(a), W(b))


def _cases_fr_mul2(op, p):
    rnd = random.Random(106)
    Rm = 1 << 256
    sp = [0, 1, p - 1, p - 2, (p - 1) // 2, Rm % p, (p >> 224 << 224) - 1]
    op.add("p-1_everywhere", *[words(p - 1, 8)] * 4)
    for i, a in enumerate(sp):
        for j, b in enumerate(sp):
            op.add(f"special{i}x{j}+p-1_squared", words(a, 8), words(b, 8), words(p - 1, 8), words(p - 1, 8))
            op.add(f"special{i}x{j}+special{j}x{i}", words(a, 8), words(b, 8), words(b, 8), words(a, 8))
    for _ in range(10):  # a b + c d = 0: a b + (p - a) b
        a, b = rnd.randrange(p), rnd.randrange(p)
        op.add("ab+(p-a)b", words(a, 8), words(b, 8), words(p - a, 8), words(b, 8))
    for _ in range(200):
        op.add("random", *[words(rnd.randrange(p), 8) for _ in range(4)])


# ================================================================ ec.cuh
RQ = 2**384 % Q
IRQ = pow(2**384, -1, Q)


def point32(k, z, neg=False):
    """k G as canonical Montgomery (R = 2^384) XYZZ words"""
    x, y = m29._mulg(k)
    if neg:
        y = Q - y
    return [w for v in (x * z * z, y * z**3, z * z, z**3) for w in words(v * RQ % Q, 12)]


def _pl(w):  # Montgomery words -> plain coordinates
    return [unwords(c) * IRQ % Q for c in split(w, 12)]


def _mw(c):  # plain coordinates -> Montgomery words
    return [w for v in c for w in words(v % Q * RQ % Q, 12)]


INF32 = (1, 1, 0, 0)


def ec_dbl(p):
    X, Y, ZZ, ZZZ = p
    if ZZ == 0:
        return p
    u = 2 * Y % Q
    v = u * u % Q
    w = u * v % Q
    s = X * v % Q
    m = 3 * X * X % Q
    x3 = (m * m - 2 * s) % Q
    return x3, (m * (s - x3) - w * Y) % Q, v * ZZ % Q, w * ZZZ % Q


def ec_add(p, q):
    if p[2] == 0:
        return q
    if q[2] == 0:
        return p
    u1, u2, s1, s2 = p[0] * q[2] % Q, q[0] * p[2] % Q, p[1] * q[3] % Q, q[1] * p[3] % Q
    P, Rr = (u2 - u1) % Q, (s2 - s1) % Q
    if P == 0:
        return ec_dbl(p) if Rr == 0 else INF32
    pp = P * P % Q
    ppp, qq = P * pp % Q, u1 * pp % Q
    x3 = (Rr * Rr - ppp - 2 * qq) % Q
    return x3, (Rr * (qq - x3) - s1 * ppp) % Q, p[2] * q[2] * pp % Q, p[3] * q[3] * ppp % Q


def ec_madd(p, x2, y2):
    if p[2] == 0:
        return x2, y2, 1, 1
    if (x2 * p[2] - p[0]) % Q == 0 and (y2 * p[3] - p[1]) % Q == 0:
        return ec_dbl((x2, y2, 1, 1))
    return ec_add(p, (x2, y2, 1, 1))


def _aff32(c):
    return None if c[2] == 0 else (c[0] * pow(c[2], -1, Q) % Q, c[1] * pow(c[3], -1, Q) % Q)


def _ec_sum(a, b):
    if a is None or b is None:
        return b if a is None else a
    if a[0] == b[0]:
        return m29._dbl_aff(a) if a[1] == b[1] else None
    return m29.aff_add(a, b)


def _p_ec(kind):
    def props(w, out):
        assert all(unwords(c) < Q for c in split(w + out, 12))
        a = _aff32(_pl(w[:48]))
        b = a if kind == "dbl" else (tuple(_pl(w[48:72])) if kind == "madd" else _aff32(_pl(w[48:])))
        assert _aff32(_pl(out)) == _ec_sum(a, b)
    return props


def _cases_ec(ops):
    rnd = random.Random(105)
    ks = [rnd.randrange(1, 2**64) for _ in range(6)]
    zr = lambda: rnd.randrange(1, Q)  # noqa: E731
    P = [point32(k, zr() if i else 1) for i, k in enumerate(ks)]
    aff = [_mw(m29._mulg(k)) for k in ks]
    infs = [("inf", _mw(INF32)), ("inf_junk_xy", point32(ks[0], 5)[:24] + [0] * 24)]
    add, madd, dbl = ops["ec_add"], ops["ec_madd"], ops["ec_dbl"]
    for i, p in enumerate(P):
        for j, q in enumerate(P):
            if i != j:
                add.add(f"P{i}+P{j}", p, q)
                madd.add(f"P{i}+P{j}", p, aff[j])
        add.add(f"P{i}+P{i}", p, p)
        add.add(f"P{i}+P{i}_other_z", p, point32(ks[i], zr()))
        add.add(f"P{i}+(-P{i})", p, point32(ks[i], zr(), neg=True))
        madd.add(f"P{i}+P{i}", p, aff[i])
        madd.add(f"P{i}+(-P{i})", p, _mw((lambda x, y: (x, Q - y))(*m29._mulg(ks[i]))))
        for tn, n in infs:
            add.add(f"P{i}+{tn}", p, n)
            add.add(f"{tn}+P{i}", n, p)
            madd.add(f"{tn}+P{i}", n, aff[i])
        dbl.add(f"2P{i}", p)
    for tn, n in infs:
        dbl.add(tn, n)
        for tm, m in infs:
            add.add(f"{tn}+{tm}", n, m)


# ================================================================ the suite
@functools.lru_cache(maxsize=None)
def suite():
    ops = {}

    def op(header, name, oid, wi, wo, model, props):
        ops[name] = Op(header, name, oid, wi, wo, model, props)

    # the models by name, looked up when called
    f30 = lambda f: (lambda w: enc(getattr(m30, f)(*[dec30(x) for x in split(w, 13)])))  # noqa: E731
    h = "field30s"
    op(h, "mul30s", 1, 26, 13, f30("mul30s"), _p_prod30(2, 2**381))
    op(h, "sqr30s", 2, 13, 13, f30("sqr30s"), _p_prod30(1, 2**381))
    op(h, "mul2_30s", 3, 52, 13, f30("mul2_30s"), _p_prod30(4, 2**382))
    op(h, "sub30s", 4, 26, 13, f30("sub30s"), _p_lin30(lambda a, b: a - b))
    op(h, "sub2_30s", 5, 39, 13, f30("sub2_30s"), _p_lin30(lambda a, b, c: a - b - c))
    op(h, "neg30s", 6, 13, 13, f30("neg30s"), _p_lin30(lambda a: -a))
    op(h, "to_f30s", 7, 12, 37, _m_to_f30s, _p_to_f30s)
    op(h, "f30s_to_fq32", 8, 13, 12, lambda w: words(m30.to_fq32(dec30(w)), 12), _p_f30s_to_fq32)
    op(h, "to_f29", 9, 13, 14, lambda w: m30.to_f29(dec30(w)), _p_to_f29)
    op("ec30s", "chain30s", 10, 1 + 26 * CHAIN_MAX, 60, _m_chain, _p_chain)

    f29 = lambda f: (lambda w: f(*split(w, 14)))  # noqa: E731
    KA, KB = C29["F29_KA"], C29["F29_KB"]
    h = "field29"
    op(h, "mul29", 11, 28, 14, f29(lambda a, b: m29.mul29(a, b)), _p_prod29(2))
    op(h, "sqr29", 12, 14, 14, f29(lambda a: m29.sqr29(a)), _p_prod29(1))
    op(h, "mul2_29", 13, 56, 14, f29(lambda a, b, c, d: m29.mul2_29(a, b, c, d)), _p_prod29(4))
    op(h, "sub29_ka", 14, 28, 14, f29(lambda a, b: m29.sub29(a, b, KA)), _p_sub29(KA))
    op(h, "sub29_kb", 15, 28, 14, f29(lambda a, b: m29.sub29(a, b, KB)), _p_sub29(KB))
    op(h, "neg29_ka", 16, 14, 14, lambda w: neg29(w, KA), _p_sub29(KA, True))
    op(h, "neg29_kb", 17, 14, 14, lambda w: neg29(w, KB), _p_sub29(KB, True))
    op(h, "repack29", 18, 12, 14, lambda w: m29.limbs(unwords(w)), lambda w, o: None)
    op(h, "unpack29", 19, 14, 12, lambda w: unpack29(w), lambda w, o: None)
    op(h, "f29_to_fq32", 20, 14, 12, lambda w: _m_f29_to_fq32(w), lambda w, o: _p_to32(w, o))
    op(h, "from_fq32", 21, 12, 14, _m_from_fq32, _p_from_fq32)
    h = "ec29"
    op(h, "zero29", 22, 14, 1, lambda w: [int(zero29(w))], _p_zero29)
    op(h, "xadd29_inf", 23, 112, 57, _m_xadd29_inf, _p_xadd29_inf)
    op(h, "xdbl29_inf", 24, 56, 56, _m_xdbl29_inf, _p_xdbl29_inf)
    op(h, "to32", 25, 56, 48, _m_to32, _p_to32)
    op(h, "from32", 26, 48, 56, _m_from32, _p_from32)

    r2 = lambda f: (lambda w: f(*split(w, 9)))  # noqa: E731
    h = "fr29"
    op(h, "r29_from_words", 27, 8, 9, lambda w: r29_from_words(w), lambda w, o: None)
    op(h, "r29_to_words", 28, 9, 8, _m_r29_to_words, lambda w, o: None)
    op(h, "r29_add", 29, 18, 9, r2(lambda a, b: mr.add(a, b)), _p_r29_lin(lambda a, b: a + b))
    op(h, "r29_sub_kdit", 30, 18, 9, r2(lambda a, b: mr.sub(a, b, CR["R29_KDIT"])), _p_r29_lin(lambda a, b: a + 4 * R - b))
    op(h, "r29_sub_kdif", 31, 19, 9, lambda w: mr.sub(w[:9], w[9:18], CR["KDIF"][w[18]]),
       _p_r29_lin(lambda a, b, row: a + (R << (row + 1)) - b))
    op(h, "r29_mul", 32, 18, 9, r2(lambda a, b: mr._mul_in(a, b)), _p_r29_prod(2))
    op(h, "r29_mul2", 33, 36, 9, r2(lambda a, b, c, d: mr.mul2(a, b, c, d)), _p_r29_prod(4))
    op(h, "r29_canon", 34, 9, 9, lambda w: mr.canon(w), _p_r29_canon)

    _fp_ops(ops, "field", "fr_", 40, R, 8)
    ir = pow(2**256, -1, R)
    ops["fr_mul2"] = Op("field", "fr_mul2", 49, 32, 8,
                        lambda w: words((lambda a, b, c, d: (a * b + c * d) * ir % R)(*[unwords(x) for x in split(w, 8)]), 8),
                        ops["fr_mul"].props)
    _fp_ops(ops, "field", "fq_", 50, Q, 12)
    h = "ec"
    op(h, "ec_add", 60, 96, 48, lambda w: _mw(ec_add(_pl(w[:48]), _pl(w[48:]))), _p_ec("add"))
    op(h, "ec_madd", 61, 72, 48, lambda w: _mw(ec_madd(_pl(w[:48]), *_pl(w[48:]))), _p_ec("madd"))
    op(h, "ec_dbl", 62, 48, 48, lambda w: _mw(ec_dbl(_pl(w))), _p_ec("dbl"))

    _cases_f30s(ops)
    _cases_f29(ops)
    _cases_ec29(ops)
    _cases_r29(ops)
    _cases_fp(ops, "fr_", R, 8, 107)
    _cases_fp(ops, "fq_", Q, 12, 108)
    _cases_fr_mul2(ops["fr_mul2"], R)
    _cases_ec(ops)
    return ops


HEADERS = ("field30s", "ec30s", "field29", "ec29", "fr29", "field", "ec")


@functools.lru_cache(maxsize=None)
def expected():
    """the result words of every case by the limb models (asserts live) and the
    integers, computed once"""
    return {name: [op.model(w) for _, w in op.cases] for name, op in suite().items()}


def pack(ops):
    a = array("I")
    assert a.itemsize == 4
    for op in ops.values():
        a.extend([op.oid, len(op.cases), op.wi, op.wo])
        for _, w in op.cases:
            a.extend(w)
    return a.tobytes()


def unpack_in(blob, ops):
    """the case file read back: {op id: (cases, words in, words out, operand words)}"""
    a = array("I")
    a.frombytes(blob)
    out, pos = {}, 0
    while pos < len(a):
        oid, n, wi, wo = a[pos:pos + 4]
        out[oid] = (n, wi, wo, split(list(a[pos + 4:pos + 4 + n * wi]), wi))
        pos += 4 + n * wi
    assert pos == len(a)
    return out


def unpack_out(blob, ops):
    a = array("I")
    a.frombytes(blob)
    assert len(a) == sum(len(op.cases) * op.wo for op in ops.values()), "the harness wrote another number of words"
    out, pos = {}, 0
    for name, op in ops.items():
        n = len(op.cases) * op.wo
        out[name] = split(list(a[pos:pos + n]), op.wo)
        pos += n
    return out


def failures(ops, got, want, header=None):
    """(op, case number, tag, what) of every case whose result misses a check"""
    bad = []
    for name, op in ops.items():
        if header and op.header != header:
            continue
        assert len(got[name]) == len(op.cases) == len(want[name])
        for i, ((tag, w), o, e) in enumerate(zip(op.cases, got[name], want[name])):
            assert len(o) == op.wo
            try:
                op.props(w, o)
            except (AssertionError, ValueError) as err:  # ValueError: no inverse of a ZZ that should have one
                bad.append((name, i, tag, f"integers / contract: {err!r}"))
                continue
            if o != e:
                bad.append((name, i, tag, "differs from the model"))
    return bad


# ================================================================ CPU
def test_cases_hold_on_cpu():
    ops, want = suite(), expected()  # the models' own asserts ran on every case
    assert sorted(set(op.header for op in ops.values())) == sorted(HEADERS)
    assert len(set(op.oid for op in ops.values())) == len(ops)
    for name, op in ops.items():
        assert op.cases, name
        assert all(len(e) == op.wo and all(0 <= x <= M32 for x in e) for e in want[name]), name
    for name in ("mul30s", "sqr30s", "mul2_30s", "mul29", "sqr29", "mul2_29", "r29_mul", "r29_mul2"):
        assert len(ops[name].cases) >= 300, name
    assert failures(ops, want, want) == []  # the reference alone meets the integers and the contract
    blob = pack(ops)
    back = unpack_in(blob, ops)
    assert list(back) == [op.oid for op in ops.values()]
    for op in ops.values():
        assert back[op.oid] == (len(op.cases), op.wi, op.wo, [w for _, w in op.cases]), op.name
    flat = array("I", [x for name in ops for e in want[name] for x in e]).tobytes()
    assert unpack_out(flat, ops) == want
    # the limb lists the cases must hold, by name
    tags = {name: {t for t, _ in op.cases} for name, op in ops.items()}
    assert sum(t.startswith("extreme") for t in tags["mul30s"]) == 121
    assert {"hi-lo-lo", "lo-hi-hi", "lo-lo-lo", "hi-hi-hi"} <= tags["sub2_30s"]
    assert {"windows_3fffffff", "windows_2e29", "windows_2e29-1"} <= tags["to_f30s"]
    assert {f"{k}q" for k in (-2, -1, 1, 2, 3)} | {"0", "2e383-1", "-(2e383-1)"} <= tags["to_f29"]
    assert {"q", "2q", "0"} <= tags["zero29"] and "top_limb_ffffffff_low_full" in tags["r29_canon"]


# ================================================================ GPU
@pytest.fixture(scope="module")
def device_results(tmp_path_factory):
    """every case of every op through ONE run of lib/dev_arith"""
    ops = suite()
    if not os.path.exists(BIN):
        r = subprocess.run(["make", "-C", CSRC, "../lib/dev_arith"], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and os.path.exists(BIN), f"lib/dev_arith is missing and does not build:\n{r.stderr[-2000:]}"
    d = tmp_path_factory.mktemp("dev_arith")
    fin, fout = str(d / "cases.bin"), str(d / "results.bin")
    with open(fin, "wb") as f:
        f.write(pack(ops))
    r = subprocess.run([BIN, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"dev_arith exited with {r.returncode}:\n{r.stderr[-2000:]}"
    with open(fout, "rb") as f:
        return unpack_out(f.read(), ops)


def _check(device_results, header):
    ops = suite()
    assert any(op.header == header for op in ops.values())
    bad = failures(ops, device_results, expected(), header)
    assert not bad, f"{len(bad)} cases fail, the first: {bad[:8]}"


@pytest.mark.gpu
def test_field30s_device(device_results):
    _check(device_results, "field30s")


@pytest.mark.gpu
def test_ec30s_device(device_results):
    _check(device_results, "ec30s")


@pytest.mark.gpu
def test_field29_device(device_results):
    _check(device_results, "field29")


@pytest.mark.gpu
def test_ec29_device(device_results):
    _check(device_results, "ec29")


@pytest.mark.gpu
def test_fr29_device(device_results):
    _check(device_results, "fr29")


@pytest.mark.gpu
def test_field_device(device_results):
    _check(device_results, "field")


@pytest.mark.gpu
def test_ec_device(device_results):
    _check(device_results, "ec")
