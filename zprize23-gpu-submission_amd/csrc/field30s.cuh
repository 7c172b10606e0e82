// field30s.cuh — BLS12-381 Fq in SIGNED radix 2^30 (13 limbs), for the mixed
// addition of the MSM bucket accumulation on gfx950.
//
// Why: the accumulation is bound by its v_mad_u64_u32 count (field29.cuh: 392
// per product).  13 limbs need 169 + 169 = 338 multiply-adds, but unsigned
// 30-bit limbs overflow one 64-bit column (26 products of < 2^60) and the two
// accumulators that cures it with ran 0.80x (tools/ubench_fq30.hip).  With
// limbs balanced in [-2^29, 2^29) a product is <= 2^58 in magnitude, a column
// of 26 products and its carry stays below 2^63, and the product is 338 bare
// v_mad_i64_i32 in ONE signed accumulator: 1.09x the products/s of mul29 on the
// whole chip (tools/ubench_fq30s.hip, profiles/fq30s_ubench.txt).
//
// Representation: value V = sum l_i 2^(30 i), l_0..l_11 in [-2^29, 2^29] (the
// closed upper end admits a negated limb), l_12 whatever is left; Montgomery
// with R = 2^390, NOT reduced and signed: a product of |inputs| < 2^385 is
// (a b + M q) 2^-390 with |M| < 2^389, so |result| < 2^380 + q/2 < 2^381.
// Subtraction is limb-wise with the carries renormalised (no lifted multiples
// of q); negation is 13 limb negations.  The bounds of the mixed addition are
// tracked in madd30s (ec30s.cuh) and checked by tests/test_field30s.py against
// a Python model.
//
// One accumulator chain: in the source the carry of column k is the addend of
// column k + 1's first multiply-add.  Left alone, the compiler reorders a
// column's sum: it starts the operand products from zero, keeps the carry on a
// second register pair and joins the two with a 64-bit add the source does not
// contain (25 a product).  Two things together keep the source's order
// (tools/ubench_fq30s.hip, profiles/acc_chain_ubench.txt, profiles/
// acc_chain_isa.txt): the carry handed to the next column goes through an empty
// asm (pin30s), and every partial sum is named in an assumption (mad30s), which
// gives it a second use, so the sums of a column are not merged into one
// expression.  Neither emits an instruction; the compiler pads some of the asm
// statements with an s_nop 0.  Every column still sums the same terms in the
// same order as before, so the bounds stated at each product cover every
// partial sum, and the assumption (a sum is not -2^63) follows from them.
#pragma once
#include "field29.cuh"
#include "f30s_consts.inc"

namespace pnp {

struct F30s {
    int32_t l[13];
};

// low 30 bits of x as a balanced limb in [-2^29, 2^29) (v_bfe_i32)
__device__ __forceinline__ int32_t bal30(uint32_t x) { return (int32_t)(x << 2) >> 2; }
// acc + a b, one v_mad_i64_i32; |acc + a b| < 2^63 by the column bounds below
__device__ __forceinline__ int64_t mad30s(int32_t a, int32_t b, int64_t acc) {
    acc += (int64_t)a * b;
    __builtin_assume(acc != INT64_MIN);
    return acc;
}
// the value as it is, but opaque to the compiler: what is added to it later
// cannot be reassociated with what was added before
__device__ __forceinline__ int64_t pin30s(int64_t acc) {
    asm volatile("" : "+v"(acc));
    return acc;
}
// what a column hands to the next once its balanced low limb is taken out
__device__ __forceinline__ int64_t carry30(int64_t acc) { return (acc + (1 << 29)) >> 30; }

// one column of the Montgomery reduction: the products m_i q_(k-i) so far,
// then (k < 13) the new m_k, which clears the low 30 bits, or (k >= 13) the
// result limb; returns the carry into column k + 1, which the caller pins
__device__ __forceinline__ int64_t reduce_col30s(int k, int64_t acc, int32_t *m, F30s &r) {
#pragma unroll
    for (int i = (k > 12 ? k - 12 : 0); i < (k < 13 ? k : 13); i++) acc = mad30s(m[i], F30S_Q[k - i], acc);
    if (k < 13) {
        m[k] = bal30((uint32_t)acc * (uint32_t)F30S_QINV);
        return mad30s(m[k], F30S_Q[0], acc) >> 30;  // exact: the low 30 bits are 0
    }
    r.l[k - 13] = bal30((uint32_t)acc);
    return carry30(acc);
}

// Montgomery product a b 2^-390 (product scanning, one signed accumulator);
// a column holds <= 13 + 13 products of <= 2^58 and a carry < 2^34
__device__ __forceinline__ F30s mul30s(const F30s &a, const F30s &b) {
    int32_t m[13];
    F30s r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 25; k++) {
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); i <= (k < 12 ? k : 12); i++) acc = mad30s(a.l[i], b.l[k - i], acc);
        acc = pin30s(reduce_col30s(k, acc, m, r));
    }
    r.l[12] = (int32_t)acc;
    return r;
}

// Montgomery square: the cross products a_i a_j (i < j) once, against the
// doubled limb 2 a_j (<= 2^30): a column holds <= 6 products of <= 2^59, one
// square and <= 13 + 1 reduction products of <= 2^58 — 27 2^58 < 2^63.
// 91 + 169 multiply-adds instead of 169 + 169.
__device__ __forceinline__ F30s sqr30s(const F30s &a) {
    int32_t m[13], a2[13];
#pragma unroll
    for (int i = 0; i < 13; i++) a2[i] = a.l[i] * 2;
    F30s r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 25; k++) {
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); 2 * i < k; i++) acc = mad30s(a.l[i], a2[k - i], acc);
        if ((k & 1) == 0) acc = mad30s(a.l[k / 2], a.l[k / 2], acc);
        acc = pin30s(reduce_col30s(k, acc, m, r));
    }
    r.l[12] = (int32_t)acc;
    return r;
}

// A subtraction folded into the product it follows.  The reduction walks the
// result columns 13..24 on the accumulator and takes a balanced limb out of
// each, so a term added to column 13 + j is added to the result at weight
// 2^(30 j): the subtrahend's limb j goes in there, times -1 (or -2), with one
// multiply-add, and the chain normalises the difference for nothing; limb 12
// is subtracted from what is left.  The m_k are fixed by columns 0..12, which
// the fold does not touch, and balanced limbs 0..11 with limb 12 taking the
// rest are unique, so the result has the 13 limbs of sub30s(mul30s(a, b), d).
// The factor must be opaque (an SGPR the compiler cannot see through): a
// visible -1 becomes a sign extension and a 64-bit subtract with borrow, 3
// instructions a limb instead of one v_mad_i64_i32.
// The subtrahend: limbs 0..11 of <= 2^29, any limb 12 that fits 32 bits with
// the result's (here |x|, |y|, |ppp|, |q| < 2^384: limb 12 below 2^24).
__device__ __forceinline__ int32_t opaque30s(int32_t c) {
    asm volatile("" : "+s"(c));
    return c;
}

// a b 2^-390 - d.  A result column holds <= 13 + 13 products of <= 2^58, a
// carry < 2^34 and one fold term of <= 2^29: under 2^63.
// 338 + 12 multiply-adds; |result| < 2^381 + |d|.
__device__ __forceinline__ F30s mul30s_sub(const F30s &a, const F30s &b, const F30s &d) {
    const int32_t m1 = opaque30s(-1);
    int32_t m[13];
    F30s r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 25; k++) {
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); i <= (k < 12 ? k : 12); i++) acc = mad30s(a.l[i], b.l[k - i], acc);
        if (k >= 13) acc = mad30s(d.l[k - 13], m1, acc);
        acc = pin30s(reduce_col30s(k, acc, m, r));
    }
    r.l[12] = (int32_t)acc - d.l[12];
    return r;
}

// a^2 2^-390 - d - 2 e.  A result column holds the <= 27 2^58 of sqr30s, a
// carry < 2^34 and fold terms of <= 3 2^29: under 2^63.
// 260 + 24 multiply-adds; |result| < 2^381 + |d| + 2 |e|.
__device__ __forceinline__ F30s sqr30s_sub2(const F30s &a, const F30s &d, const F30s &e) {
    const int32_t m1 = opaque30s(-1), m2 = opaque30s(-2);
    int32_t m[13], a2[13];
#pragma unroll
    for (int i = 0; i < 13; i++) a2[i] = a.l[i] * 2;
    F30s r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 25; k++) {
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); 2 * i < k; i++) acc = mad30s(a.l[i], a2[k - i], acc);
        if ((k & 1) == 0) acc = mad30s(a.l[k / 2], a.l[k / 2], acc);
        if (k >= 13) {
            acc = mad30s(d.l[k - 13], m1, acc);
            acc = mad30s(e.l[k - 13], m2, acc);
        }
        acc = pin30s(reduce_col30s(k, acc, m, r));
    }
    r.l[12] = (int32_t)acc - d.l[12] - 2 * e.l[12];
    return r;
}

// a b + c d with ONE Montgomery reduction, (a b + c d) 2^-390.  Column k
// holds 2 n + n (+ 1) products of <= 2^58, n = min(k + 1, 25 - k): up to 39 in
// the middle, which does not fit 63 bits.  In the columns of more than 31
// products (k = 10..14) the carry of the 2 n operand products (<= 26 2^58) is
// taken out before the reduction products go in, and handed to column k + 1
// with theirs; the low limb the reduction starts from is pinned like a carry.
// 338 + 169 multiply-adds against the 676 of two mul30s.
// |result| < (|a b| + |c d|) 2^-390 + q/2: < 2^382 for inputs < 2^385.
__device__ __forceinline__ F30s mul2_30s(const F30s &a, const F30s &b, const F30s &c, const F30s &d) {
    int32_t m[13];
    F30s r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 25; k++) {
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); i <= (k < 12 ? k : 12); i++) {
            acc = mad30s(a.l[i], b.l[k - i], acc);
            acc = mad30s(c.l[i], d.l[k - i], acc);
        }
        if (3 * (k < 13 ? k + 1 : 25 - k) > 31) {
            const int64_t hi = carry30(acc);
            acc = reduce_col30s(k, (int64_t)bal30((uint32_t)acc), m, r) + hi;
        } else {
            acc = pin30s(reduce_col30s(k, acc, m, r));
        }
    }
    r.l[12] = (int32_t)acc;
    return r;
}

// carries of limb sums renormalised to balanced limbs.  Two limbs of
// <= 2^29: |t_i + c| <= 2^30 + 1, and the carry is (s + 2^29) >> 30.  THREE
// limbs can reach 3 2^29 with the carry, where s + 2^29 is 2^31: the carry is
// then taken as floor(s / 2^30) + bit 29 of s, which never leaves 32 bits.
template <bool THREE>
__device__ __forceinline__ F30s norm30s(const int32_t *t) {
    F30s r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const int32_t s = t[i] + c;
        r.l[i] = bal30((uint32_t)s);
        c = THREE ? (s >> 30) + ((s >> 29) & 1) : (s + (1 << 29)) >> 30;
    }
    r.l[12] = t[12] + c;
    return r;
}
// a - b
__device__ __forceinline__ F30s sub30s(const F30s &a, const F30s &b) {
    int32_t t[13];
#pragma unroll
    for (int i = 0; i < 13; i++) t[i] = a.l[i] - b.l[i];
    return norm30s<false>(t);
}
// a - b - c
__device__ __forceinline__ F30s sub2_30s(const F30s &a, const F30s &b, const F30s &c) {
    int32_t t[13];
#pragma unroll
    for (int i = 0; i < 13; i++) t[i] = a.l[i] - b.l[i] - c.l[i];
    return norm30s<true>(t);
}
// -a: limbs in (-2^29, 2^29], still <= 2^29 in magnitude
__device__ __forceinline__ F30s neg30s(const F30s &a) {
    F30s r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = -a.l[i];
    return r;
}

__device__ __forceinline__ F30s const30s(const int32_t *c) {
    F30s r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = c[i];
    return r;
}

// ---- conversions ----------------------------------------------------------
// a product output r (|r| < q) as the non-negative integer r + q < 2q in 13
// unsigned limbs, the top one taking what is left; r = 0 mod q comes out as q
__device__ __forceinline__ void lift30s(const F30s &r, uint32_t *u) {
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const int32_t t = r.l[i] + F30S_Q[i] + c;
        u[i] = (uint32_t)t & 0x3FFFFFFFu;
        c = t >> 30;
    }
    u[12] = (uint32_t)(r.l[12] + F30S_Q[12] + c);
}

// R390-form F30s (|a| < 2^383) -> raw R406-form F29, < 2q with normalised
// limbs (the form of a product output in ec29.cuh; 0 mod q comes out as q,
// which zero29 knows): one product by a constant, then 13 x 30 -> 14 x 29 bits
__device__ __forceinline__ F29 to_f29(const F30s &a) {
    uint32_t u[13];
    lift30s(mul30s(a, const30s(F30S_C406)), u);
    F29 r;
#pragma unroll
    for (int j = 0; j < 14; j++) {
        const int bit = 29 * j, w = bit / 30, sh = bit % 30;
        uint64_t x = u[w];
        if (w + 1 < 13) x |= (uint64_t)u[w + 1] << 30;
        r.l[j] = (uint32_t)(x >> sh) & F29_M;
    }
    return r;
}

// R390-form F30s (|a| < 2^383) -> R384-form canonical Fq (12 x 32-bit limbs)
__device__ __forceinline__ Fq to_fq32(const F30s &a) {
    uint32_t u[13];
    lift30s(mul30s(a, const30s(F30S_C384)), u);
    Fq r;
#pragma unroll
    for (int w = 0; w < 12; w++) {
        const int bit = 32 * w, j = bit / 30, sh = bit % 30;
        uint64_t x = (uint64_t)u[j] >> sh;
        if (j + 1 < 13) x |= (uint64_t)u[j + 1] << (30 - sh);
        if (j + 2 < 13 && 60 - sh < 32) x |= (uint64_t)u[j + 2] << (60 - sh);
        r.v[w] = (uint32_t)x;
    }
    reduce_once(r);
    return r;
}

// R384-form Fq (canonical) -> R390-form F30s, |result| < 2^381
__device__ __forceinline__ F30s to_f30s(const Fq &a) {
    F30s t;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 13; j++) {
        const int bit = 30 * j, w = bit >> 5, sh = bit & 31;
        uint64_t x = a.v[w];
        if (w + 1 < 12) x |= (uint64_t)a.v[w + 1] << 32;
        const uint32_t u = ((uint32_t)(x >> sh) & 0x3FFFFFFFu) + c;  // <= 2^30
        t.l[j] = j < 12 ? bal30(u) : (int32_t)u;
        c = (u + (1u << 29)) >> 30;
    }
    return mul30s(t, const30s(F30S_C396));
}

// a table line: x, y as 13 limbs each (104 B of the 128-B line)
__device__ __forceinline__ F30s load30s(const uint32_t *p) {
    F30s r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = (int32_t)p[i];
    return r;
}

}  // namespace pnp
