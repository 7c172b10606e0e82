// keyblocks.hip — key-load kernels of pnp_load_prover_key_coeffs: the coset
// constants (lin, v_h^-1, the denominators of l1v) written straight into
// block-bitrev layout from their closed forms (coset_blocks.cuh), with no
// natural-order 8n array in between, and the gather that reads single points
// back out of that layout (the v1 symbol's sampled check).
#include "pnp_internal.h"
#include "coset_blocks.cuh"

namespace pnp {

// One thread per storage index p of a block: j = brev(p), so a wavefront
// stores 64 consecutive 32-byte elements (two 16-byte stores per lane) in
// every array of every block, and w_n^j (the ~2 lg n products) is shared by
// the nb blocks.  Any of the outputs may be nullptr.
__global__ __launch_bounds__(256) void k_coset_blocks_(CosetBlockConsts K, int m0, int nb, uint64_t *lin,
                                                       uint64_t *lin32, uint64_t *vh_inv, uint64_t *l1_den) {
    const uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (p >> K.lg_n) return;
    const uint32_t j = coset_brev((uint32_t)p, K.lg_n);
    const Fr wj = pow_u64(K.w_n, j);
    for (int b = 0; b < nb; b++) {
        const int m = m0 + b;
        const uint64_t at = coset_block_index(K, b, j);  // = b n + p
        Fr x, den;
        coset_block_point(K, m, wj, x, den);
        if (lin) store_fr(lin, at, x);
        if (lin32) {  // the 2^261 form of k_quotient29: five modular doublings (k_to_form29)
            Fr y = x;
#pragma unroll
            for (int k = 0; k < 5; k++) y = y + y;
            store_fr(lin32, at, y);
        }
        if (vh_inv) store_fr(vh_inv, at, K.vh_inv[m]);
        if (l1_den) store_fr(l1_den, at, den);
    }
}

void k_coset_blocks(uint32_t lg_n, int m0, int nb, uint64_t *lin, uint64_t *lin32, uint64_t *vh_inv,
                    uint64_t *l1_den, hipStream_t s) {
    if (lg_n > 25 || m0 < 0 || nb < 1 || m0 + nb > 8) {
        set_error("coset blocks [%d, %d) of domain 2^%u", m0, m0 + nb, lg_n);
        throw Error(PNP_E_ARG);
    }
    const uint64_t n = 1ULL << lg_n;
    hipLaunchKernelGGL(k_coset_blocks_, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s,
                       coset_block_consts(lg_n), m0, nb, lin, lin32, vh_inv, l1_den);
    PNP_HIP(hipGetLastError());
}

// out[k] = the value at natural index idx[k] = 8 j + m of the 8n coset, read
// from blocks m0 .. m0 + nb - 1 in block-bitrev layout; zero for a block that
// is not held (the caller skips those)
__global__ void k_gather_blocks_(const uint64_t *blk, uint32_t lg_n, int m0, int nb, const uint64_t *idx,
                                 uint32_t cnt, uint64_t *out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    const uint64_t i = idx[k];
    const int b = (int)(i & 7) - m0;
    Fr v = Fr::zero();
    if (b >= 0 && b < nb && (i >> 3) >> lg_n == 0)
        v = load_fr(blk, ((uint64_t)b << lg_n) + coset_brev((uint32_t)(i >> 3), lg_n));
    store_fr(out, k, v);
}

void k_gather_blocks(const uint64_t *blk, uint32_t lg_n, int m0, int nb, const uint64_t *d_idx, uint32_t cnt,
                     uint64_t *d_out, hipStream_t s) {
    if (!cnt) return;
    hipLaunchKernelGGL(k_gather_blocks_, dim3((cnt + 255) / 256), dim3(256), 0, s, blk, lg_n, m0, nb, d_idx, cnt,
                       d_out);
    PNP_HIP(hipGetLastError());
}

}  // namespace pnp
