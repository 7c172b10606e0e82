// dev_arith_fold — runs the folded subtractions of csrc/field30s.cuh
// (mul30s_sub, sqr30s_sub2) alone, one routine per kernel and one lane per
// case, on operands read from a file (tests/test_gpu_field30s_fold.py writes it
// and checks what comes back).  A program of its own beside dev_arith, with
// that program's file format:
//
//   dev_arith_fold IN OUT
//
// IN is a sequence of blocks of u32 words: op id, case count, words in per
// case, words out per case, then the operand words of every case.  OUT gets
// the result words of every block in the same order.  Operands are loaded from
// global memory, so no routine sees a compile-time constant; nothing is checked
// here.  Any HIP error ends the program with a non-zero status before anything
// more is launched.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "field30s.cuh"

using namespace pnp;

__device__ __forceinline__ void st30(uint32_t *o, const F30s &a) {
#pragma unroll
    for (int i = 0; i < 13; i++) o[i] = (uint32_t)a.l[i];
}

// ---- the ops: words in, words out, the routine on one case
struct o_mul30s_sub {
    static constexpr uint32_t WI = 39, WO = 13;
    static __device__ __forceinline__ void run(const uint32_t *in, uint32_t *out) {
        st30(out, mul30s_sub(load30s(in), load30s(in + 13), load30s(in + 26)));
    }
};
struct o_sqr30s_sub2 {
    static constexpr uint32_t WI = 39, WO = 13;
    static __device__ __forceinline__ void run(const uint32_t *in, uint32_t *out) {
        st30(out, sqr30s_sub2(load30s(in), load30s(in + 13), load30s(in + 26)));
    }
};

template <class O>
__global__ __launch_bounds__(64) void k_op(const uint32_t *in, uint32_t *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) O::run(in + (uint64_t)i * O::WI, out + (uint64_t)i * O::WO);
}

struct OpEntry {
    uint32_t id, wi, wo;
    void (*launch)(const uint32_t *, uint32_t *, uint32_t);
};
template <class O>
static void launch(const uint32_t *in, uint32_t *out, uint32_t n) {
    k_op<O><<<(n + 63) / 64, 64>>>(in, out, n);
}
// the ids are the ones tests/test_gpu_field30s_fold.py names
static const OpEntry OPS[] = {
    {1, o_mul30s_sub::WI, o_mul30s_sub::WO, launch<o_mul30s_sub>},
    {2, o_sqr30s_sub2::WI, o_sqr30s_sub2::WO, launch<o_sqr30s_sub2>},
};

static void die(const char *what, hipError_t e) {
    fprintf(stderr, "dev_arith_fold: %s: %s\n", what, hipGetErrorString(e));
    exit(1);
}
#define HIP(call)                              \
    do {                                       \
        const hipError_t e_ = (call);          \
        if (e_ != hipSuccess) die(#call, e_);  \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: dev_arith_fold IN OUT\n");
        return 2;
    }
    std::vector<uint32_t> in;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) {
            perror(argv[1]);
            return 2;
        }
        fseek(f, 0, SEEK_END);
        const long sz = ftell(f);
        fseek(f, 0, SEEK_SET);
        if (sz < 0 || sz % 4 != 0) {
            fprintf(stderr, "dev_arith_fold: %s is not a whole number of words\n", argv[1]);
            return 2;
        }
        in.resize((size_t)sz / 4);
        if (!in.empty() && fread(in.data(), 4, in.size(), f) != in.size()) {
            fprintf(stderr, "dev_arith_fold: short read of %s\n", argv[1]);
            return 2;
        }
        fclose(f);
    }
    std::vector<uint32_t> out;
    size_t pos = 0;
    while (pos < in.size()) {
        if (in.size() - pos < 4) {
            fprintf(stderr, "dev_arith_fold: truncated block header at word %zu\n", pos);
            return 2;
        }
        const uint32_t id = in[pos], n = in[pos + 1], wi = in[pos + 2], wo = in[pos + 3];
        pos += 4;
        const OpEntry *op = nullptr;
        for (const OpEntry &e : OPS)
            if (e.id == id) op = &e;
        // the kernels index by their own widths: a block must state the same
        if (!op || wi != op->wi || wo != op->wo || n > (1u << 20) || (uint64_t)n * wi > in.size() - pos) {
            fprintf(stderr, "dev_arith_fold: bad block (op %u, %u cases, %u in, %u out) at word %zu\n", id, n, wi,
                    wo, pos - 4);
            return 2;
        }
        const size_t nin = (size_t)n * wi, nout = (size_t)n * wo, at = out.size();
        out.resize(at + nout);
        if (n) {
            uint32_t *din = nullptr, *dout = nullptr;
            HIP(hipMalloc(&din, nin * 4));
            HIP(hipMalloc(&dout, nout * 4));
            HIP(hipMemcpy(din, in.data() + pos, nin * 4, hipMemcpyHostToDevice));
            HIP(hipMemset(dout, 0, nout * 4));
            op->launch(din, dout, n);
            HIP(hipGetLastError());
            HIP(hipDeviceSynchronize());
            HIP(hipMemcpy(out.data() + at, dout, nout * 4, hipMemcpyDeviceToHost));
            HIP(hipFree(din));
            HIP(hipFree(dout));
        }
        pos += nin;
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f) {
        perror(argv[2]);
        return 2;
    }
    if (!out.empty() && fwrite(out.data(), 4, out.size(), f) != out.size()) {
        fprintf(stderr, "dev_arith_fold: short write of %s\n", argv[2]);
        return 2;
    }
    if (fclose(f) != 0) {
        perror(argv[2]);
        return 2;
    }
    return 0;
}
