// Microbenchmark: throughput of the Fq Montgomery product on the whole chip,
// radix 2^29 unsigned (field29.cuh, 392 v_mad_u64_u32) against 13 SIGNED
// 30-bit limbs, balanced in [-2^29, 2^29), R = 2^390: 338 v_mad_i64_i32 in ONE
// signed 64-bit column accumulator (26 products of <= 2^58 are < 2^63, so the
// two accumulators of tools/ubench_fq30.hip are not needed).  Same launch
// shape and method as tools/ubench_fq30.hip: random operands, every CU busy,
// best of 5, so the clock the chip holds under the load is part of the result.
// The signed product is checked first: the host's copy of the function
// against integer arithmetic mod q, then 256 lanes' chains on the GPU against
// the host's (check() below).
//
// CHAIN variants (mul<C>, sqr<C>, mul2<C>): the compiler starts every column's
// operand products from zero, keeps the carry of the reduction on a second
// register pair and joins the two with one 64-bit add per column that the
// source does not contain.  C = 1: an empty asm on the accumulator between two
// columns (pin()) makes the carry opaque; C = 2: the same, and every partial
// sum is named in an assumption (mad()).  k_mul30s<C> times the plain product,
// k_mix30s<C> the mix of one mixed addition (6 products, 2 squares, one
// a b + c d with one reduction).
//
// FOLD (k_madd30s<C, F>): the whole mixed addition, products and subtractions.
// F = 0: the three subtractions from a fresh product (U2 - X, S2 - Y,
// R^2 - PPP - 2 Q) limb-wise with the carries renormalised; F = 1: folded into
// that product's reduction, one multiply-add a limb (mul_sub, sqr_sub2).  The
// two give the same limbs, which check() compares on the host.
//   hipcc -O3 --offload-arch=gfx950 -I<csrc> ubench_fq30s.hip -o ubench_fq30s
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "field29.cuh"
using namespace pnp;

namespace f30s {
// q in balanced limbs, sum Q[i] 2^(30 i) = q
__host__ __device__ constexpr int32_t qlimb(int i) {
    constexpr int32_t Q[13] = {-21845,    -402915328, 356515836,  -352321620, -252304353, 55215067, 288093811,
                               316751073, -321428361, 517541167, -375082566, -91332614,  1704210};
    return Q[i];
}
constexpr uint32_t QINV = 0xfffcfffdu;  // -q^-1 mod 2^30, sign-extended (-196611)
struct F30 {
    int32_t l[13];
};
// low 30 bits of x as a balanced limb in [-2^29, 2^29)
__host__ __device__ __forceinline__ int32_t bal30(uint32_t x) { return (int32_t)(x << 2) >> 2; }
// CHAIN 2: every partial sum is also named in an assumption (true: a column
// stays below 2^63), which gives it a second use, so the sums of a column are
// not merged into one expression and reordered while the assumptions live
template <int CHAIN = 0>
__host__ __device__ __forceinline__ int64_t mad(int32_t a, int32_t b, int64_t acc) {
    acc += (int64_t)a * b;
#ifdef __HIP_DEVICE_COMPILE__
    if (CHAIN == 2) __builtin_assume(acc != INT64_MIN);
#endif
    return acc;
}
__host__ __device__ __forceinline__ int64_t carry(int64_t acc) { return (acc + (1 << 29)) >> 30; }
// CHAIN: the value is opaque to the compiler from here on, so the additions
// before and after it cannot be reassociated (device only; emits nothing)
template <int CHAIN>
__host__ __device__ __forceinline__ int64_t pin(int64_t acc) {
#ifdef __HIP_DEVICE_COMPILE__
    if (CHAIN) asm volatile("" : "+v"(acc));
#endif
    return acc;
}
// one column of the reduction: returns the carry into column k + 1
template <int CHAIN>
__host__ __device__ __forceinline__ int64_t reduce_col(int k, int64_t acc, int32_t *m, int32_t *r) {
#pragma unroll
    for (int i = (k > 12 ? k - 12 : 0); i < (k < 13 ? k : 13); i++) acc = mad<CHAIN>(m[i], qlimb(k - i), acc);
    if (k < 13) {
        m[k] = bal30((uint32_t)acc * QINV);
        return mad<CHAIN>(m[k], qlimb(0), acc) >> 30;  // low 30 bits become 0
    }
    r[k - 13] = bal30((uint32_t)acc);
    return carry(acc);
}
// a b 2^-390 (mod q), |a|, |b| < 2^385 -> |r| < 2^381; r.l[0..11] balanced
template <int CHAIN = 0>
__host__ __device__ __forceinline__ F30 mul(const F30 &a, const F30 &b) {
    int32_t m[13];
    F30 r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 25; k++) {
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); i <= (k < 12 ? k : 12); i++) acc = mad<CHAIN>(a.l[i], b.l[k - i], acc);
        acc = pin<CHAIN>(reduce_col<CHAIN>(k, acc, m, r.l));
    }
    r.l[12] = (int32_t)acc;
    return r;
}
// a^2 2^-390: the cross products once, against the doubled limb
template <int CHAIN = 0>
__host__ __device__ __forceinline__ F30 sqr(const F30 &a) {
    int32_t m[13], a2[13];
#pragma unroll
    for (int i = 0; i < 13; i++) a2[i] = a.l[i] * 2;
    F30 r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 25; k++) {
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); 2 * i < k; i++) acc = mad<CHAIN>(a.l[i], a2[k - i], acc);
        if ((k & 1) == 0) acc = mad<CHAIN>(a.l[k / 2], a.l[k / 2], acc);
        acc = pin<CHAIN>(reduce_col<CHAIN>(k, acc, m, r.l));
    }
    r.l[12] = (int32_t)acc;
    return r;
}
// (a b + c d) 2^-390 with one reduction; in the columns of more than 31
// products (k = 10..14) the operand products' carry is taken out early
template <int CHAIN = 0>
__host__ __device__ __forceinline__ F30 mul2(const F30 &a, const F30 &b, const F30 &c, const F30 &d) {
    int32_t m[13];
    F30 r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 25; k++) {
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); i <= (k < 12 ? k : 12); i++) {
            acc = mad<CHAIN>(a.l[i], b.l[k - i], acc);
            acc = mad<CHAIN>(c.l[i], d.l[k - i], acc);
        }
        if (3 * (k < 13 ? k + 1 : 25 - k) > 31) {
            const int64_t hi = carry(acc);
            acc = pin<CHAIN>(reduce_col<CHAIN>(k, pin<CHAIN>((int64_t)bal30((uint32_t)acc)), m, r.l) + hi);
        } else {
            acc = pin<CHAIN>(reduce_col<CHAIN>(k, acc, m, r.l));
        }
    }
    r.l[12] = (int32_t)acc;
    return r;
}
// ---- the subtractions of the mixed addition (field30s.cuh), and the FOLD of
// the three that follow a fresh product into that product's reduction: limb j
// of the subtrahend goes into result column 13 + j, times an opaque -1 (-2),
// one multiply-add each; the chain normalises the difference
template <bool THREE>
__host__ __device__ __forceinline__ F30 norm(const int32_t *t) {
    F30 r;
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
__host__ __device__ __forceinline__ F30 sub(const F30 &a, const F30 &b) {
    int32_t t[13];
#pragma unroll
    for (int i = 0; i < 13; i++) t[i] = a.l[i] - b.l[i];
    return norm<false>(t);
}
__host__ __device__ __forceinline__ F30 sub2(const F30 &a, const F30 &b, const F30 &c) {
    int32_t t[13];
#pragma unroll
    for (int i = 0; i < 13; i++) t[i] = a.l[i] - b.l[i] - c.l[i];
    return norm<true>(t);
}
__host__ __device__ __forceinline__ F30 neg(const F30 &a) {
    F30 r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = -a.l[i];
    return r;
}
// a constant the compiler cannot see through (device only; emits nothing)
__host__ __device__ __forceinline__ int32_t opaque(int32_t c) {
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+s"(c));
#endif
    return c;
}
// a b 2^-390 - d
template <int CHAIN = 0>
__host__ __device__ __forceinline__ F30 mul_sub(const F30 &a, const F30 &b, const F30 &d) {
    const int32_t m1 = opaque(-1);
    int32_t m[13];
    F30 r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 25; k++) {
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); i <= (k < 12 ? k : 12); i++) acc = mad<CHAIN>(a.l[i], b.l[k - i], acc);
        if (k >= 13) acc = mad<CHAIN>(d.l[k - 13], m1, acc);
        acc = pin<CHAIN>(reduce_col<CHAIN>(k, acc, m, r.l));
    }
    r.l[12] = (int32_t)acc - d.l[12];
    return r;
}
// a^2 2^-390 - d - 2 e
template <int CHAIN = 0>
__host__ __device__ __forceinline__ F30 sqr_sub2(const F30 &a, const F30 &d, const F30 &e) {
    const int32_t m1 = opaque(-1), m2 = opaque(-2);
    int32_t m[13], a2[13];
#pragma unroll
    for (int i = 0; i < 13; i++) a2[i] = a.l[i] * 2;
    F30 r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 25; k++) {
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); 2 * i < k; i++) acc = mad<CHAIN>(a.l[i], a2[k - i], acc);
        if ((k & 1) == 0) acc = mad<CHAIN>(a.l[k / 2], a.l[k / 2], acc);
        if (k >= 13) {
            acc = mad<CHAIN>(d.l[k - 13], m1, acc);
            acc = mad<CHAIN>(e.l[k - 13], m2, acc);
        }
        acc = pin<CHAIN>(reduce_col<CHAIN>(k, acc, m, r.l));
    }
    r.l[12] = (int32_t)acc - d.l[12] - 2 * e.l[12];
    return r;
}
}  // namespace f30s

__global__ __launch_bounds__(256) void k_mul29(uint32_t *out, int L, uint32_t seed) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    F29 a, b, c, d;
    uint32_t h = seed ^ (t * 0x9E3779B9u);
    for (int i = 0; i < 14; i++) {
        h = h * 1664525u + 1013904223u; a.l[i] = h & F29_M;
        h = h * 1664525u + 1013904223u; b.l[i] = h & F29_M;
        h = h * 1664525u + 1013904223u; c.l[i] = h & F29_M;
        h = h * 1664525u + 1013904223u; d.l[i] = h & F29_M;
    }
    a.l[13] &= 0xFFFFFF; b.l[13] &= 0xFFFFFF; c.l[13] &= 0xFFFFFF; d.l[13] &= 0xFFFFFF;
#pragma unroll 1
    for (int i = 0; i < L; i++) {
        a = mul29(a, b); c = mul29(c, d); b = mul29(b, c); d = mul29(d, a);
    }
    uint32_t x = 0;
    for (int i = 0; i < 14; i++) x ^= a.l[i] ^ b.l[i] ^ c.l[i] ^ d.l[i];
    out[t] = x;
}

// the four operands of lane t: balanced limbs, top limb < 2^21 in magnitude
__host__ __device__ inline void seed30s(uint32_t t, uint32_t seed, f30s::F30 &a, f30s::F30 &b, f30s::F30 &c,
                                        f30s::F30 &d) {
    uint32_t h = seed ^ (t * 0x9E3779B9u);
    for (int i = 0; i < 13; i++) {
        h = h * 1664525u + 1013904223u; a.l[i] = f30s::bal30(h >> 2);
        h = h * 1664525u + 1013904223u; b.l[i] = f30s::bal30(h >> 2);
        h = h * 1664525u + 1013904223u; c.l[i] = f30s::bal30(h >> 2);
        h = h * 1664525u + 1013904223u; d.l[i] = f30s::bal30(h >> 2);
    }
    a.l[12] >>= 8; b.l[12] >>= 8; c.l[12] >>= 8; d.l[12] >>= 8;
}
template <int CHAIN = 0>
__host__ __device__ inline void chain30s(int L, f30s::F30 &a, f30s::F30 &b, f30s::F30 &c, f30s::F30 &d) {
#pragma unroll 1
    for (int i = 0; i < L; i++) {
        a = f30s::mul<CHAIN>(a, b); c = f30s::mul<CHAIN>(c, d); b = f30s::mul<CHAIN>(b, c); d = f30s::mul<CHAIN>(d, a);
    }
}
// the nine products of one mixed addition: 6 mul, 2 sqr, 1 mul2 (3,055
// multiply-adds), chained through the four values so that nothing is dead;
// every output is < 2^382, inside the products' input bound of 2^385
template <int CHAIN = 0>
__host__ __device__ inline void mix30s(int L, f30s::F30 &a, f30s::F30 &b, f30s::F30 &c, f30s::F30 &d) {
#pragma unroll 1
    for (int i = 0; i < L; i++) {
        f30s::F30 u = f30s::mul<CHAIN>(a, c), s = f30s::mul<CHAIN>(b, d);
        f30s::F30 pp = f30s::sqr<CHAIN>(u);
        f30s::F30 ppp = f30s::mul<CHAIN>(u, pp), q = f30s::mul<CHAIN>(a, pp);
        a = f30s::sqr<CHAIN>(s);
        b = f30s::mul2<CHAIN>(s, q, b, ppp);
        c = f30s::mul<CHAIN>(c, pp);
        d = f30s::mul<CHAIN>(d, ppp);
    }
}
// the whole mixed addition (ec30s.cuh madd30s) on (X, Y, ZZ, ZZZ) = (a, b, c, d),
// the lane's first (a, b) added again in every step (|x2|, |y2| < 2^381, the
// bounds of madd30s hold).  FOLD 0: the three subtractions from a fresh product
// renormalised limb by limb, as sub() and sub2() do; FOLD 1: folded into that
// product's reduction.  Both give the same 52 limbs (check() below).
template <int CHAIN, int FOLD>
__host__ __device__ inline void madd30s(int L, f30s::F30 &a, f30s::F30 &b, f30s::F30 &c, f30s::F30 &d) {
    using namespace f30s;
    const F30 x2 = a, y2 = b;
#pragma unroll 1
    for (int i = 0; i < L; i++) {
        const F30 P = FOLD ? mul_sub<CHAIN>(x2, c, a) : sub(mul<CHAIN>(x2, c), a);
        const F30 R = FOLD ? mul_sub<CHAIN>(y2, d, b) : sub(mul<CHAIN>(y2, d), b);
        const F30 pp = sqr<CHAIN>(P);
        const F30 ppp = mul<CHAIN>(P, pp), q = mul<CHAIN>(a, pp);
        const F30 x3 = FOLD ? sqr_sub2<CHAIN>(R, ppp, q) : sub(sub2(sqr<CHAIN>(R), ppp, q), q);
        b = mul2<CHAIN>(R, sub(q, x3), b, neg(ppp));
        c = mul<CHAIN>(c, pp);
        d = mul<CHAIN>(d, ppp);
        a = x3;
    }
}

template <int CHAIN>
__global__ __launch_bounds__(256) void k_mul30s(uint32_t *out, int L, uint32_t seed) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    f30s::F30 a, b, c, d;
    seed30s(t, seed, a, b, c, d);
    chain30s<CHAIN>(L, a, b, c, d);
    uint32_t x = 0;
    for (int i = 0; i < 13; i++) x ^= (uint32_t)(a.l[i] ^ b.l[i] ^ c.l[i] ^ d.l[i]);
    out[t] = x;
}
template <int CHAIN>
__global__ __launch_bounds__(256) void k_mix30s(uint32_t *out, int L, uint32_t seed) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    f30s::F30 a, b, c, d;
    seed30s(t, seed, a, b, c, d);
    mix30s<CHAIN>(L, a, b, c, d);
    uint32_t x = 0;
    for (int i = 0; i < 13; i++) x ^= (uint32_t)(a.l[i] ^ b.l[i] ^ c.l[i] ^ d.l[i]);
    out[t] = x;
}
template <int CHAIN, int FOLD>
__global__ __launch_bounds__(256) void k_madd30s(uint32_t *out, int L, uint32_t seed) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    f30s::F30 a, b, c, d;
    seed30s(t, seed, a, b, c, d);
    madd30s<CHAIN, FOLD>(L, a, b, c, d);
    uint32_t x = 0;
    for (int i = 0; i < 13; i++) x ^= (uint32_t)(a.l[i] ^ b.l[i] ^ c.l[i] ^ d.l[i]);
    out[t] = x;
}

// ---- host check of the signed product ------------------------------------
// r = a b 2^-390 (mod q) means r 2^390 - a b = 0 (mod q): the 780-bit integer
// is formed in 30-bit limbs and divided by q bit by bit.
static bool divisible_by_q(std::vector<int64_t> v) {  // v: signed limbs radix 2^30, little endian
    static const uint64_t QW[7] = {0xb9feffffffffaaabull, 0x1eabfffeb153ffffull, 0x6730d2a0f6b0f624ull,
                                   0x64774b84f38512bfull, 0x4b1ba7b6434bacd7ull, 0x1a0111ea397fe69aull, 0};
    // normalise the limbs; a negative integer is negated (divisibility does not depend on the sign)
    int64_t c = 0;
    for (auto &x : v) { x += c; c = x >> 30; x &= 0x3FFFFFFF; }
    if (c < 0) {  // negate: two's complement over the limbs
        int64_t b = 1;
        for (auto &x : v) { x = (~x & 0x3FFFFFFF) + b; b = x >> 30; x &= 0x3FFFFFFF; }
        c = ~c + b;
    }
    v.push_back(c);
    const int nb = 30 * (int)v.size();
    std::vector<uint8_t> bits(nb);
    for (int i = 0; i < nb; i++) bits[i] = (v[i / 30] >> (i % 30)) & 1;
    // remainder in 7 x 64-bit words, shift-and-subtract from the top bit
    uint64_t rem[7] = {0};
    for (int i = nb - 1; i >= 0; i--) {
        for (int w = 6; w > 0; w--) rem[w] = (rem[w] << 1) | (rem[w - 1] >> 63);
        rem[0] = (rem[0] << 1) | bits[i];
        bool ge = true;
        for (int w = 6; w >= 0; w--)
            if (rem[w] != QW[w]) { ge = rem[w] > QW[w]; break; }
        if (ge) {
            uint64_t bw = 0;
            for (int w = 0; w < 7; w++) {
                const uint64_t s = rem[w] - QW[w] - bw;
                bw = (rem[w] < QW[w] + bw) || (QW[w] + bw < bw);
                rem[w] = s;
            }
        }
    }
    for (int w = 0; w < 7; w++)
        if (rem[w]) return false;
    return true;
}
// r = (a b + c d) 2^-390 (mod q), c = nullptr: r = a b 2^-390
static bool check_result(const f30s::F30 &r, const f30s::F30 &a, const f30s::F30 &b, const f30s::F30 *c = nullptr,
                         const f30s::F30 *d = nullptr) {
    std::vector<int64_t> v(27, 0);  // r 2^390 - a b - c d, columns of <= 26 products < 2^58 and one limb
    for (int i = 0; i < 13; i++) v[13 + i] += r.l[i];
    for (int i = 0; i < 13; i++)
        for (int j = 0; j < 13; j++) {
            v[i + j] -= (int64_t)a.l[i] * b.l[j];
            if (c) v[i + j] -= (int64_t)c->l[i] * d->l[j];
        }
    for (int i = 0; i < 12; i++)
        if (r.l[i] < -(1 << 29) || r.l[i] >= (1 << 29)) return false;
    return divisible_by_q(v);
}
static bool check_product(const f30s::F30 &a, const f30s::F30 &b) {
    return check_result(f30s::mul(a, b), a, b) && check_result(f30s::sqr(a), a, a) &&
           check_result(f30s::mul2(a, b, b, a), a, b, &b, &a);
}
static bool check(uint32_t *dout) {
    f30s::F30 a, b, c, d;
    int bad = 0;
    for (uint32_t t = 0; t < 64; t++) {
        seed30s(t, 99u, a, b, c, d);
        for (int i = 0; i < 8; i++) {
            bad += !check_product(a, b); a = f30s::mul(a, b);
            bad += !check_product(c, d); c = f30s::mul(c, d);
            bad += !check_product(b, c); b = f30s::mul(b, c);
            bad += !check_product(d, a); d = f30s::mul(d, a);
        }
    }
    for (int s = 0; s < 4; s++) {  // every limb at an end of its range
        for (int i = 0; i < 13; i++) {
            a.l[i] = (s & 1) ? -(1 << 29) : (1 << 29) - 1;
            b.l[i] = (s & 2) ? -(1 << 29) : (1 << 29) - 1;
        }
        a.l[12] >>= 5; b.l[12] >>= 5;  // |value| < 2^385
        bad += !check_product(a, b);
    }
    printf("signed products (mul, sqr, mul2) against integer arithmetic mod q on the host: %s\n",
           bad ? "MISMATCH" : "ok");
    {  // the folded subtractions against the renormalised ones, every limb, after each of 8 steps
        int fb = 0;
        for (uint32_t t = 0; t < 64; t++) {
            f30s::F30 e, f, g, h;
            seed30s(t, 99u, a, b, c, d);
            e = a; f = b; g = c; h = d;
            for (int i = 0; i < 8; i++) {
                madd30s<0, 0>(1, a, b, c, d);
                madd30s<0, 1>(1, e, f, g, h);
                fb += memcmp(&a, &e, sizeof a) || memcmp(&b, &f, sizeof b) || memcmp(&c, &g, sizeof c) ||
                      memcmp(&d, &h, sizeof d);
            }
        }
        printf("mixed addition with the folded subtractions against the renormalised, limb for limb, on the host: %s\n",
               fb ? "MISMATCH" : "ok");
        bad += fb;
    }
    if (dout) {  // the GPU's chains of lanes 0..255, plain and CHAIN, against the host's
        for (int v = 0; v < 8; v++) {
            if (v == 0) hipLaunchKernelGGL(k_mul30s<0>, dim3(1), dim3(256), 0, 0, dout, 3, 5u);
            if (v == 1) hipLaunchKernelGGL(k_mul30s<1>, dim3(1), dim3(256), 0, 0, dout, 3, 5u);
            if (v == 2) hipLaunchKernelGGL(k_mul30s<2>, dim3(1), dim3(256), 0, 0, dout, 3, 5u);
            if (v == 3) hipLaunchKernelGGL(k_mix30s<0>, dim3(1), dim3(256), 0, 0, dout, 3, 5u);
            if (v == 4) hipLaunchKernelGGL(k_mix30s<1>, dim3(1), dim3(256), 0, 0, dout, 3, 5u);
            if (v == 5) hipLaunchKernelGGL(k_mix30s<2>, dim3(1), dim3(256), 0, 0, dout, 3, 5u);
            if (v == 6) hipLaunchKernelGGL((k_madd30s<2, 0>), dim3(1), dim3(256), 0, 0, dout, 3, 5u);
            if (v == 7) hipLaunchKernelGGL((k_madd30s<2, 1>), dim3(1), dim3(256), 0, 0, dout, 3, 5u);
            uint32_t g[256];
            if (hipMemcpy(g, dout, sizeof g, hipMemcpyDeviceToHost) != hipSuccess) return false;
            int gb = 0;
            for (uint32_t t = 0; t < 256; t++) {
                seed30s(t, 5u, a, b, c, d);
                if (v < 3) chain30s(3, a, b, c, d);
                else if (v < 6) mix30s(3, a, b, c, d);
                else madd30s<0, 0>(3, a, b, c, d);
                uint32_t x = 0;
                for (int i = 0; i < 13; i++) x ^= (uint32_t)(a.l[i] ^ b.l[i] ^ c.l[i] ^ d.l[i]);
                gb += x != g[t];
            }
            printf("GPU %s, CHAIN %d, against the host's, 256 lanes: %s\n",
                   v < 3 ? "mul chain" : v < 6 ? "mixed-addition mix" : v == 6 ? "mixed addition" : "mixed addition, folded",
                   v < 6 ? v % 3 : 2, gb ? "MISMATCH" : "ok");
            bad += gb;
        }
    }
    return bad == 0;
}

template <typename K>
static double run(K kern, const char *name, uint32_t *dout, uint32_t threads, int L, double per_iter = 4.0) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipLaunchKernelGGL(kern, dim3(threads / 256), dim3(256), 0, 0, dout, 4, 1u);
    hipDeviceSynchronize();
    float best = 1e30f, worst = 0;
    for (int rep = 0; rep < 5; rep++) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(kern, dim3(threads / 256), dim3(256), 0, 0, dout, L, 7u + rep);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
        if (ms > worst) worst = ms;
    }
    hipFuncAttributes fa;
    hipFuncGetAttributes(&fa, (const void *)kern);
    const double prods = per_iter * L * threads;
    printf("%-10s best %8.3f ms  worst %8.3f ms  %7.2f G products/s  (%d VGPRs)\n", name, best, worst,
           prods / best / 1e6, fa.numRegs);
    return prods / best / 1e6;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--host-check")) return check(nullptr) ? 0 : 1;
    const uint32_t threads = 1u << 20;
    const int L = 256;
    uint32_t *dout;
    if (hipMalloc(&dout, threads * 4) != hipSuccess) return 2;
    if (!check(dout)) return 1;
    double a[3], b[3][3], m[3][3], f[2][3];
    const double mix = 3055.0 / 338.0;  // a mix iteration is 3,055 multiply-adds: counted as 3055 / 338 products
    for (int i = 0; i < 3; i++) {
        a[i] = run(k_mul29, "mul29", dout, threads, L);
        b[0][i] = run(k_mul30s<0>, "mul30s", dout, threads, L);
        b[1][i] = run(k_mul30s<1>, "mul30s/c1", dout, threads, L);
        b[2][i] = run(k_mul30s<2>, "mul30s/c2", dout, threads, L);
        m[0][i] = run(k_mix30s<0>, "mix30s", dout, threads, L / 2, mix);
        m[1][i] = run(k_mix30s<1>, "mix30s/c1", dout, threads, L / 2, mix);
        m[2][i] = run(k_mix30s<2>, "mix30s/c2", dout, threads, L / 2, mix);
        // the whole mixed addition, its products counted as the mix's: renormalised and folded subtractions
        f[0][i] = run(k_madd30s<2, 0>, "madd30s", dout, threads, L / 2, mix);
        f[1][i] = run(k_madd30s<2, 1>, "madd30s/f", dout, threads, L / 2, mix);
    }
    for (int i = 0; i < 3; i++) printf("ratio mul30s / mul29 = %.3f\n", b[0][i] / a[i]);
    for (int c = 1; c < 3; c++)
        for (int i = 0; i < 3; i++)
            printf("ratio CHAIN %d / plain: mul30s %.4f  mix30s %.4f\n", c, b[c][i] / b[0][i], m[c][i] / m[0][i]);
    for (int i = 0; i < 3; i++) printf("ratio folded / renormalised subtractions: madd30s %.4f\n", f[1][i] / f[0][i]);
    return 0;
}
