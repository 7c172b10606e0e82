// coset_blocks.cuh — the 8n-coset constants of a prover key in closed form,
// addressed in block-bitrev layout (ntt.hip lde_blocks): point i = 8 j + m of
// the coset x_i = g w_8n^i (g = 7) is stored at b n + brev(j), m = m0 + b.
//   lin    = x_i              = (g w_8n^m) w_n^j
//   vh_inv = (x_i^n - 1)^-1   = (g^n w_8^m - 1)^-1      one value per block
//   l1v    = L_1(x_i) / Z_H(x_i) = (D (lin - 1))^-1
// The index map and the per-block constants are host / device functions: the
// key load's kernel (keyblocks.hip) and tests/native/host_coset_blocks.cpp
// run the same source.
#pragma once
#include "field.cuh"

namespace pnp {

struct CosetBlockConsts {
    Fr c[8];       // g w_8n^m: the first point of block m
    Fr vh_inv[8];  // (g^n w_8^m - 1)^-1
    Fr w_n;        // w_8n^8, the generator of the order-n subgroup
    Fr d;          // the domain size n (Montgomery form)
    uint32_t lg_n;
};

PNP_HD uint32_t coset_brev(uint32_t x, uint32_t bits) {
    uint32_t r = 0;
    for (uint32_t k = 0; k < bits; k++) r |= ((x >> k) & 1u) << (bits - 1 - k);
    return r;
}
// where block b (of the blocks m0 .. held) keeps index j of its residue class
PNP_HD uint64_t coset_block_index(const CosetBlockConsts &K, int b, uint32_t j) {
    return ((uint64_t)b << K.lg_n) + coset_brev(j, K.lg_n);
}
// lin and the denominator of l1v (l1v = l1_den^-1) at index j of block m,
// given wj = w_n^j (shared by the eight blocks)
PNP_HD void coset_block_point(const CosetBlockConsts &K, int m, const Fr &wj, Fr &lin, Fr &l1_den) {
    lin = K.c[m] * wj;
    l1_den = K.d * (lin - Fr::one());
}

// host: the constants of domain 2^lg_n
inline CosetBlockConsts coset_block_consts(uint32_t lg_n) {
    const uint64_t root32[4] = {13381757501831005802ULL, 6564924994866501612ULL, 789602057691799140ULL,
                                6625830629041353339ULL};
    const Fr r32 = from_u64_limbs<FrP>(root32);
    const uint64_t n = 1ULL << lg_n;
    const Fr w8n = pow_u64(r32, 1ULL << (32 - (lg_n + 3))), w8 = pow_u64(r32, 1ULL << 29);
    Fr seven = Fr::zero(), nf = Fr::zero();
    seven.v[0] = 7;
    nf.v[0] = (uint32_t)n;
    nf.v[1] = (uint32_t)(n >> 32);
    const Fr g = to_mont(seven);
    CosetBlockConsts K;
    K.lg_n = lg_n;
    K.w_n = pow_u64(w8n, 8);
    K.d = to_mont(nf);
    Fr cm = g, vm = pow_u64(g, n);
    for (int m = 0; m < 8; m++) {
        K.c[m] = cm;
        K.vh_inv[m] = inverse(vm - Fr::one());
        cm = cm * w8n;
        vm = vm * w8;
    }
    return K;
}

}  // namespace pnp
