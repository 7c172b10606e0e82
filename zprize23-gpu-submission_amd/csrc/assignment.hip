// assignment.hip — the witness columns from a variable assignment on gfx950.
//
// A composer holds one value per variable and a wire map var[j][i] (the
// variable in wire j of gate i).  The prover's four witness columns are
//   w_j[i] = values[var_j[i]],  i < n_gates;   0,  n_gates <= i < D,
// which the ZK-Garage prover builds on the CPU by four passes of
// variables[&w_x[i]] over a HashMap (prover.rs:197-216) followed by pad_poly.
// Here: one launch over the D rows of the domain, straight into the prover's
// padded witness buffers (no separate zero fill of the padding rows).
//
//   k_gather_witness  a lane a row: four coalesced u32 id loads, four
//                     independent 32-byte gathers (ids of neighbouring rows are
//                     near each other in composer-built circuits, so the
//                     gathers of a wave share cache lines), four store_fr.
//                     No atomics, no LDS.
//   k_first_diff      the first (row, wire) at which four columns differ from
//                     four others (pnp_load_wire_map: the sigmas of a wire map
//                     against the resident key's).
#include "pnp_internal.h"

namespace pnp {

namespace {

inline uint32_t nblk(uint64_t threads, uint32_t bs = 256) { return (uint32_t)((threads + bs - 1) / bs); }

struct GatherArgs {
    const uint32_t *var[4];
    uint64_t *w[4];
};

// An id >= n_vars (the loaders refuse such maps) reads as zero: the kernel
// never reads outside `values`.
__global__ __launch_bounds__(256) void k_gather_witness_(GatherArgs a, const uint64_t *__restrict__ values,
                                                          uint64_t n_gates, uint64_t n_vars, uint64_t D) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= D) return;
    Fr v[4];
    if (i < n_gates) {
        uint32_t id[4];
#pragma unroll
        for (int j = 0; j < 4; j++) id[j] = a.var[j][i];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = id[j] < n_vars ? load_fr(values, id[j]) : Fr::zero();
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = Fr::zero();
    }
#pragma unroll
    for (int j = 0; j < 4; j++) store_fr(a.w[j], i, v[j]);
}

struct DiffArgs {
    const uint64_t *a[4], *b[4];
};

// *first = min over differing (wire j, row i) of 4 i + j (unchanged when none)
__global__ __launch_bounds__(256) void k_first_diff_(DiffArgs c, uint32_t lg, unsigned long long *first) {
    const uint64_t D = 1ULL << lg;
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= 4 * D) return;
    const uint32_t j = (uint32_t)(t >> lg);
    const uint64_t i = t & (D - 1);
    if (!(load_fr(c.a[j], i) == load_fr(c.b[j], i))) atomicMin(first, (unsigned long long)(4 * i + j));
}

}  // namespace

void k_gather_witness(const uint32_t *const d_var[4], uint64_t n_gates, const uint64_t *d_values, uint64_t n_vars,
                      uint32_t lg, uint64_t *const d_w[4], hipStream_t s) {
    const uint64_t D = 1ULL << lg;
    GatherArgs a{{d_var[0], d_var[1], d_var[2], d_var[3]}, {d_w[0], d_w[1], d_w[2], d_w[3]}};
    hipLaunchKernelGGL(k_gather_witness_, dim3(nblk(D)), dim3(256), 0, s, a, d_values, n_gates, n_vars, D);
    PNP_HIP(hipGetLastError());
}

uint64_t k_first_diff4(const uint64_t *const a[4], const uint64_t *const b[4], uint32_t lg, DevBuf &scratch,
                       hipStream_t s) {
    scratch.reserve(8);
    unsigned long long *first = static_cast<unsigned long long *>(scratch.p);
    PNP_HIP(hipMemsetAsync(first, 0xff, 8, s));
    DiffArgs c{{a[0], a[1], a[2], a[3]}, {b[0], b[1], b[2], b[3]}};
    hipLaunchKernelGGL(k_first_diff_, dim3(nblk(4ULL << lg)), dim3(256), 0, s, c, lg, first);
    PNP_HIP(hipGetLastError());
    unsigned long long h = 0;
    PNP_HIP(hipMemcpyAsync(&h, first, 8, hipMemcpyDeviceToHost, s));
    PNP_HIP(hipStreamSynchronize(s));
    return h;
}

}  // namespace pnp
