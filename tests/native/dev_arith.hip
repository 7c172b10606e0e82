// dev_arith — runs the device field and curve routines of csrc/ alone, one
// routine per kernel and one lane per case, on operands read from a file
// (tests/test_gpu_dev_arith.py writes it and checks what comes back).
//
//   dev_arith IN OUT
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

#include "field.cuh"
#include "ec.cuh"
#include "field29.cuh"
#include "ec29.cuh"
#include "field30s.cuh"
#include "ec30s.cuh"
#include "fr29.cuh"

using namespace pnp;

#define CHAIN_MAX 24

// ---- operands in and out, one word at a time
__device__ __forceinline__ F30s ld30(const uint32_t *p) { return load30s(p); }
__device__ __forceinline__ void st30(uint32_t *o, const F30s &a) {
#pragma unroll
    for (int i = 0; i < 13; i++) o[i] = (uint32_t)a.l[i];
}
__device__ __forceinline__ F29 ld29(const uint32_t *p) {
    F29 r;
#pragma unroll
    for (int i = 0; i < 14; i++) r.l[i] = p[i];
    return r;
}
__device__ __forceinline__ void st29(uint32_t *o, const F29 &a) {
#pragma unroll
    for (int i = 0; i < 14; i++) o[i] = a.l[i];
}
template <class F>
__device__ __forceinline__ F ldp(const uint32_t *p) {
    F r;
#pragma unroll
    for (int i = 0; i < F::N; i++) r.v[i] = p[i];
    return r;
}
template <class F>
__device__ __forceinline__ void stp(uint32_t *o, const F &a) {
#pragma unroll
    for (int i = 0; i < F::N; i++) o[i] = a.v[i];
}
__device__ __forceinline__ R29 ldr(const uint32_t *p) { return r29_load(p, 0); }
__device__ __forceinline__ void str(uint32_t *o, const R29 &a) {
#pragma unroll
    for (int i = 0; i < 9; i++) o[i] = a.l[i];
}
__device__ __forceinline__ Xyzz29 ldx29(const uint32_t *p) {
    Xyzz29 r;
    r.x = ld29(p);
    r.y = ld29(p + 14);
    r.zz = ld29(p + 28);
    r.zzz = ld29(p + 42);
    return r;
}
__device__ __forceinline__ void stx29(uint32_t *o, const Xyzz29 &a) {
    st29(o, a.x);
    st29(o + 14, a.y);
    st29(o + 28, a.zz);
    st29(o + 42, a.zzz);
}
__device__ __forceinline__ Xyzz ldx(const uint32_t *p) {
    Xyzz r;
    r.x = ldp<Fq>(p);
    r.y = ldp<Fq>(p + 12);
    r.zz = ldp<Fq>(p + 24);
    r.zzz = ldp<Fq>(p + 36);
    return r;
}
__device__ __forceinline__ void stx(uint32_t *o, const Xyzz &a) {
    stp(o, a.x);
    stp(o + 12, a.y);
    stp(o + 24, a.zz);
    stp(o + 36, a.zzz);
}

// ---- the ops: words in, words out, the routine on one case
#define OP(name, wi, wo)                                                      \
    struct name {                                                             \
        static constexpr uint32_t WI = wi, WO = wo;                           \
        static __device__ __forceinline__ void run(const uint32_t *in, uint32_t *out); \
    };                                                                        \
    __device__ __forceinline__ void name::run(const uint32_t *in, uint32_t *out)

// field30s.cuh
OP(o_mul30s, 26, 13) { st30(out, mul30s(ld30(in), ld30(in + 13))); }
OP(o_sqr30s, 13, 13) { st30(out, sqr30s(ld30(in))); }
OP(o_mul2_30s, 52, 13) { st30(out, mul2_30s(ld30(in), ld30(in + 13), ld30(in + 26), ld30(in + 39))); }
OP(o_sub30s, 26, 13) { st30(out, sub30s(ld30(in), ld30(in + 13))); }
OP(o_sub2_30s, 39, 13) { st30(out, sub2_30s(ld30(in), ld30(in + 13), ld30(in + 26))); }
OP(o_neg30s, 13, 13) { st30(out, neg30s(ld30(in))); }
// the table form, then back: to_fq32 of it and of its negation
OP(o_to_f30s, 12, 37) {
    const F30s t = to_f30s(ldp<Fq>(in));
    st30(out, t);
    stp(out + 13, to_fq32(t));
    stp(out + 25, to_fq32(neg30s(t)));
}
OP(o_f30s_to_fq32, 13, 12) { stp(out, to_fq32(ld30(in))); }
OP(o_to_f29, 13, 14) { st29(out, to_f29(ld30(in))); }
// ec30s.cuh: in = chain length, then CHAIN_MAX table-form (x, y); the first
// point starts the accumulator, the others are added; the piece is parked in
// the case's 56-word slot and converted in place; word 56 = store29's result
OP(o_chain30s, 1 + 26 * CHAIN_MAX, 60) {
    uint32_t len = in[0];
    len = len < 1 ? 1 : (len > CHAIN_MAX ? CHAIN_MAX : len);
    Xyzz30s acc;
    acc.x = ld30(in + 1);
    acc.y = ld30(in + 14);
    acc.zz = acc.zzz = const30s(F30S_ONE);
#pragma unroll 1
    for (uint32_t j = 1; j < len; j++) madd30s(acc, ld30(in + 1 + 26 * j), ld30(in + 14 + 26 * j));
    park30s(out, acc);
    const bool ok = store29(out);
    out[56] = ok ? 1u : 0u;
    out[57] = out[58] = out[59] = 0u;
}

// field29.cuh
OP(o_mul29, 28, 14) { st29(out, mul29(ld29(in), ld29(in + 14))); }
OP(o_sqr29, 14, 14) { st29(out, sqr29(ld29(in))); }
OP(o_mul2_29, 56, 14) { st29(out, mul2_29(ld29(in), ld29(in + 14), ld29(in + 28), ld29(in + 42))); }
OP(o_sub29_ka, 28, 14) { st29(out, sub29(ld29(in), ld29(in + 14), F29_KA)); }
OP(o_sub29_kb, 28, 14) { st29(out, sub29(ld29(in), ld29(in + 14), F29_KB)); }
OP(o_neg29_ka, 14, 14) { st29(out, neg29(ld29(in), F29_KA)); }
OP(o_neg29_kb, 14, 14) { st29(out, neg29(ld29(in), F29_KB)); }
OP(o_repack29, 12, 14) { st29(out, repack29(ldp<Fq>(in).v)); }
OP(o_unpack29, 14, 12) { stp(out, unpack29(ld29(in))); }
OP(o_f29_to_fq32, 14, 12) { stp(out, to_fq32(ld29(in))); }
OP(o_from_fq32, 12, 14) { st29(out, from_fq32(ldp<Fq>(in))); }

// ec29.cuh
OP(o_zero29, 14, 1) { out[0] = zero29(ld29(in)) ? 1u : 0u; }
OP(o_xadd29_inf, 112, 57) {
    uint32_t exc = 0;
    stx29(out, xadd29_inf(ldx29(in), ldx29(in + 56), &exc));
    out[56] = exc;
}
OP(o_xdbl29_inf, 56, 56) { stx29(out, xdbl29_inf(ldx29(in))); }
OP(o_to32, 56, 48) { stx(out, to32(ldx29(in))); }
OP(o_from32, 48, 56) { stx29(out, from32(ldx(in))); }

// fr29.cuh
OP(o_r29_from_words, 8, 9) { str(out, r29_from_words(ldp<Fr>(in).v)); }
OP(o_r29_to_words, 9, 8) {
    Fr w;
    r29_to_words(ldr(in), w.v);
    stp(out, w);
}
OP(o_r29_add, 18, 9) { str(out, r29_add(ldr(in), ldr(in + 9))); }
OP(o_r29_sub_kdit, 18, 9) { str(out, r29_sub(ldr(in), ldr(in + 9), R29_KDIT)); }
// word 18 = the row of R29_KDIF
OP(o_r29_sub_kdif, 19, 9) { str(out, r29_sub(ldr(in), ldr(in + 9), R29_KDIF[in[18] & 7u])); }
OP(o_r29_mul, 18, 9) { str(out, r29_mul(ldr(in), ldr(in + 9))); }
OP(o_r29_mul2, 36, 9) { str(out, r29_mul2(ldr(in), ldr(in + 9), ldr(in + 18), ldr(in + 27))); }
OP(o_r29_canon, 9, 9) { str(out, r29_canon(ldr(in))); }

// field.cuh on the device
#define FP_OPS(T, pfx, n)                                                                        \
    OP(pfx##add, 2 * n, n) { stp(out, ldp<T>(in) + ldp<T>(in + n)); }                             \
    OP(pfx##sub, 2 * n, n) { stp(out, ldp<T>(in) - ldp<T>(in + n)); }                             \
    OP(pfx##neg, n, n) { stp(out, neg(ldp<T>(in))); }                                             \
    OP(pfx##dbl, n, n) { stp(out, dbl(ldp<T>(in))); }                                             \
    OP(pfx##mul, 2 * n, n) { stp(out, ldp<T>(in) * ldp<T>(in + n)); }                             \
    OP(pfx##sqr, n, n) { stp(out, sqr(ldp<T>(in))); }                                             \
    OP(pfx##inverse, n, n) { stp(out, inverse(ldp<T>(in))); }                                     \
    OP(pfx##to_mont, n, n) { stp(out, to_mont(ldp<T>(in))); }                                     \
    OP(pfx##from_mont, n, n) { stp(out, from_mont(ldp<T>(in))); }
FP_OPS(Fr, o_fr_, 8)
FP_OPS(Fq, o_fq_, 12)
OP(o_fr_mul2, 32, 8) { stp(out, fr_mul2(ldp<Fr>(in), ldp<Fr>(in + 8), ldp<Fr>(in + 16), ldp<Fr>(in + 24))); }

// ec.cuh on the device
OP(o_ec_add, 96, 48) { stx(out, add(ldx(in), ldx(in + 48))); }
OP(o_ec_madd, 72, 48) { stx(out, madd(ldx(in), ldp<Fq>(in + 48), ldp<Fq>(in + 60))); }
OP(o_ec_dbl, 48, 48) { stx(out, dbl(ldx(in))); }

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
#define ENTRY(id, O) {id, O::WI, O::WO, launch<O>}
#define FP_ENTRIES(base, pfx)                                                                      \
    ENTRY(base + 0, pfx##add), ENTRY(base + 1, pfx##sub), ENTRY(base + 2, pfx##neg),               \
        ENTRY(base + 3, pfx##dbl), ENTRY(base + 4, pfx##mul), ENTRY(base + 5, pfx##sqr),           \
        ENTRY(base + 6, pfx##inverse), ENTRY(base + 7, pfx##to_mont), ENTRY(base + 8, pfx##from_mont)
// the ids are the ones tests/test_gpu_dev_arith.py names
static const OpEntry OPS[] = {
    ENTRY(1, o_mul30s), ENTRY(2, o_sqr30s), ENTRY(3, o_mul2_30s), ENTRY(4, o_sub30s), ENTRY(5, o_sub2_30s),
    ENTRY(6, o_neg30s), ENTRY(7, o_to_f30s), ENTRY(8, o_f30s_to_fq32), ENTRY(9, o_to_f29), ENTRY(10, o_chain30s),
    ENTRY(11, o_mul29), ENTRY(12, o_sqr29), ENTRY(13, o_mul2_29), ENTRY(14, o_sub29_ka), ENTRY(15, o_sub29_kb),
    ENTRY(16, o_neg29_ka), ENTRY(17, o_neg29_kb), ENTRY(18, o_repack29), ENTRY(19, o_unpack29),
    ENTRY(20, o_f29_to_fq32), ENTRY(21, o_from_fq32),
    ENTRY(22, o_zero29), ENTRY(23, o_xadd29_inf), ENTRY(24, o_xdbl29_inf), ENTRY(25, o_to32), ENTRY(26, o_from32),
    ENTRY(27, o_r29_from_words), ENTRY(28, o_r29_to_words), ENTRY(29, o_r29_add), ENTRY(30, o_r29_sub_kdit),
    ENTRY(31, o_r29_sub_kdif), ENTRY(32, o_r29_mul), ENTRY(33, o_r29_mul2), ENTRY(34, o_r29_canon),
    FP_ENTRIES(40, o_fr_), ENTRY(49, o_fr_mul2), FP_ENTRIES(50, o_fq_),
    ENTRY(60, o_ec_add), ENTRY(61, o_ec_madd), ENTRY(62, o_ec_dbl),
};

static void die(const char *what, hipError_t e) {
    fprintf(stderr, "dev_arith: %s: %s\n", what, hipGetErrorString(e));
    exit(1);
}
#define HIP(call)                              \
    do {                                       \
        const hipError_t e_ = (call);          \
        if (e_ != hipSuccess) die(#call, e_);  \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: dev_arith IN OUT\n");
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
            fprintf(stderr, "dev_arith: %s is not a whole number of words\n", argv[1]);
            return 2;
        }
        in.resize((size_t)sz / 4);
        if (!in.empty() && fread(in.data(), 4, in.size(), f) != in.size()) {
            fprintf(stderr, "dev_arith: short read of %s\n", argv[1]);
            return 2;
        }
        fclose(f);
    }
    std::vector<uint32_t> out;
    size_t pos = 0;
    while (pos < in.size()) {
        if (in.size() - pos < 4) {
            fprintf(stderr, "dev_arith: truncated block header at word %zu\n", pos);
            return 2;
        }
        const uint32_t id = in[pos], n = in[pos + 1], wi = in[pos + 2], wo = in[pos + 3];
        pos += 4;
        const OpEntry *op = nullptr;
        for (const OpEntry &e : OPS)
            if (e.id == id) op = &e;
        // the kernels index by their own widths: a block must state the same
        if (!op || wi != op->wi || wo != op->wo || n > (1u << 20) || (uint64_t)n * wi > in.size() - pos) {
            fprintf(stderr, "dev_arith: bad block (op %u, %u cases, %u in, %u out) at word %zu\n", id, n, wi, wo,
                    pos - 4);
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
        fprintf(stderr, "dev_arith: short write of %s\n", argv[2]);
        return 2;
    }
    if (fclose(f) != 0) {
        perror(argv[2]);
        return 2;
    }
    return 0;
}
