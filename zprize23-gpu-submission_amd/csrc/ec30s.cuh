// ec30s.cuh — the G1 XYZZ mixed addition in signed radix 2^30 (field30s.cuh)
// of the MSM bucket accumulation (msm.hip k_accumulate29), and the way a piece
// leaves it: parked in its slot as it is, converted in place to the raw
// radix-2^29 form of ec29.cuh.  A header of its own so that the device routines
// can be run alone on chosen operands (tests/native/dev_arith.hip).
#pragma once
#include "ec29.cuh"
#include "field30s.cuh"

namespace pnp {

struct Xyzz30s {
    F30s x, y, zz, zzz;
};
// P += (x2, y2), madd-2008-s.  Bounds (see field30s.cuh; the interval
// analysis of tests/test_field30s.py): x2, y2 and every product output are
// < 2^381 in magnitude, X3 = R^2 - PPP - 2 Q < 2^383, P = U2 - X < 2^383.4,
// R = S2 - Y < 2^382, Q - X3 < 2^383.4 — every product input < 2^385, and Y3
// (one reduction of two products < 2^766 + 2^762) < 2^381 again.  No equal /
// opposite / infinity cases: those make ZZ = 0 mod q, detected per piece.
// 6 mul30s + 2 sqr30s + mul2_30s = 6 338 + 2 260 + 507 = 3,055 multiply-adds
// (the radix-2^29 form: 6 392 + 2 301 + 588 = 3,542), and 12 + 12 + 24 = 48
// more for the three subtractions from a fresh product (U2 - X, S2 - Y,
// R^2 - PPP - 2 Q), folded into that product's reduction (mul30s_sub,
// sqr30s_sub2): 3,103.  The results have the limbs the renormalised
// subtractions gave, so the bounds above are what they were.
__device__ __forceinline__ void madd30s(Xyzz30s &p, const F30s &x2, const F30s &y2) {
    F30s P = mul30s_sub(x2, p.zz, p.x);
    F30s R = mul30s_sub(y2, p.zzz, p.y);
    F30s pp = sqr30s(P);
    F30s ppp = mul30s(P, pp);
    F30s q = mul30s(p.x, pp);
    F30s x3 = sqr30s_sub2(R, ppp, q);
    // Y3 = R (Q - X3) - Y PPP as R (Q - X3) + Y (-PPP), one reduction
    F30s y3 = mul2_30s(R, sub30s(q, x3), p.y, neg30s(ppp));
    p.zz = mul30s(p.zz, pp);
    p.zzz = mul30s(p.zzz, ppp);
    p.x = x3;
    p.y = y3;
}
// Pieces leave the accumulation in raw radix-2^29 form (56 u32 per XYZZ
// point, 4 x 14 limbs, ec29.cuh) and stay in it through the merge and the
// reduction tree (msm_reduce.hip); only the roots are converted to R384.
// The accumulator is in F30s form, so each coordinate of a piece is converted
// (to_f29: one product by a constant and a repack, 4 x 338 multiply-adds a
// piece against the 3,055 of an addition, on the ~1.3% of entries that end a
// piece: ~0.6%).  Not where the piece ends: a bucket ends in some lane of a
// wave in about every second step of its loop, and the whole wave would wait
// for that lane's four products.  The loop leaves the piece in its slot as it
// is (park30s: 52 of the slot's 56 u32), and the lane converts its slots in
// place when its segment is done (store29 over the same walk of the buckets).
__device__ __forceinline__ void park30s(uint32_t *dst, const Xyzz30s &p) {
    uint32_t w[52];
#pragma unroll
    for (int i = 0; i < 13; i++) {
        w[i] = (uint32_t)p.x.l[i];
        w[13 + i] = (uint32_t)p.y.l[i];
        w[26 + i] = (uint32_t)p.zz.l[i];
        w[39 + i] = (uint32_t)p.zzz.l[i];
    }
    uint4 *q = reinterpret_cast<uint4 *>(dst);
#pragma unroll
    for (int c = 0; c < 13; c++) q[c] = make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
}
// parked F30s piece -> raw F29 piece, in place; false when ZZ = 0 mod q (a
// degenerate step in the piece)
__device__ __forceinline__ bool store29(uint32_t *dst) {
    uint32_t w[52];
    const uint4 *q = reinterpret_cast<const uint4 *>(dst);
#pragma unroll
    for (int c = 0; c < 13; c++) {
        const uint4 v = q[c];
        w[4 * c] = v.x;
        w[4 * c + 1] = v.y;
        w[4 * c + 2] = v.z;
        w[4 * c + 3] = v.w;
    }
    Xyzz30s p;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        p.x.l[i] = (int32_t)w[i];
        p.y.l[i] = (int32_t)w[13 + i];
        p.zz.l[i] = (int32_t)w[26 + i];
        p.zzz.l[i] = (int32_t)w[39 + i];
    }
    const F29 zz = to_f29(p.zz);
    store_f29(dst, to_f29(p.x));
    store_f29(dst + 14, to_f29(p.y));
    store_f29(dst + 28, zz);
    store_f29(dst + 42, to_f29(p.zzz));
    return !zero29(zz);
}

}  // namespace pnp
