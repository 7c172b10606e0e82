// The closed forms and the index map of csrc/coset_blocks.cuh on the host (the
// key load's kernel, keyblocks.hip, runs the same source on the device):
// for lg_n in {3, 6}, every block m and every index j, one line
//   "<lg_n> <m> <j> <storage index> lin vh_inv l1v"   (hex, Montgomery form)
// with all eight blocks held (m0 = 0), for tests/test_host_coset_blocks.py to
// check with Python integers.
#include "coset_blocks.cuh"
#include <cstdio>

using namespace pnp;

static void hex(const Fr &a) {
    printf(" ");
    for (int i = 7; i >= 0; i--) printf("%08x", a.v[i]);
}
int main() {
    for (uint32_t lg : {3u, 6u}) {
        const CosetBlockConsts K = coset_block_consts(lg);
        for (int m = 0; m < 8; m++)
            for (uint32_t j = 0; j < (1u << lg); j++) {
                Fr lin, den;
                coset_block_point(K, m, pow_u64(K.w_n, j), lin, den);
                printf("%u %d %u %llu", lg, m, j, (unsigned long long)coset_block_index(K, m, j));
                hex(lin), hex(K.vh_inv[m]), hex(inverse(den));
                printf("\n");
            }
    }
    return 0;
}
