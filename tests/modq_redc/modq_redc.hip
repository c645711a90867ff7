// The ModQ Montgomery reduction through q + 1 (csrc/field.h: redc_limbs / redc_digit, M::low_ones) next to the generic reduction it replaces, on raw limbs.
// ModQGeneric is ModQ with low_ones = false: the templates of field.h instantiate the generic code for it -- every term m_i * q_j, the quotient digit times n0 --
// exactly as they do for ModT and ModN.  Each record runs every one-lane product routine and the wide reduction through BOTH; tests/test_modq_redc_host.py
// demands the same limb vectors from the two (not merely congruent ones: proof bytes depend on the limbs) and checks them with Python integers.
// One source, two compilers, as tests/raw_limbs:
//   g++ -x c++ -std=c++17 -DZK_HOST_BUILD -I zkp-ecdsa_amd/csrc modq_redc.hip      host executable
//   hipcc --offload-arch=gfx950 -std=c++17 -I zkp-ecdsa_amd/csrc modq_redc.hip     device executable: one record per lane
// usage: modq_redc IN OUT.  Every field a little-endian uint32.
//   header  'MQRD' (0x4452514d), n, 0, 0
//   record  40 words: a[9], b[9], T[18], sq, 0, 0, 0       (sq: 0 squares a, 1 squares b -- the operand whose magnitude admits a square)
//   output  per record 2 x 54 words, new then generic: a*b (limbs_mont_mul), a*b and b*a (limbs_mont_mul_n<2>), x^2 (limbs_mont_sqr), a*b (limbs_mont_mul_rows),
//           T / R (redc_wide)
#include "field.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

#define MQ_MAGIC 0x4452514du
#define MQ_IN 40
#define MQ_HALF 54
#define MQ_OUT (2 * MQ_HALF)

struct ModQGeneric : ModQ {
    static constexpr bool low_ones = false;
};
static_assert(ModQ::low_ones && ModQ::n0 == 1 && !ModT::low_ones && !ModN::low_ones, "the trait of consts_gen.h");

template <class M>
ZK_DEV void mq_half(const uint32_t* in, uint32_t* out) {
    uint32_t a[NLIMB], b[NLIMB], o[NLIMB], T[2 * NLIMB];
    for (int i = 0; i < NLIMB; i++) a[i] = in[i], b[i] = in[NLIMB + i];
    for (int i = 0; i < 2 * NLIMB; i++) T[i] = in[2 * NLIMB + i];
    limbs_mont_mul<M>(o, a, b);
    for (int i = 0; i < NLIMB; i++) out[i] = o[i];
    uint32_t a2[2][NLIMB], b2[2][NLIMB], o2[2][NLIMB];
    for (int i = 0; i < NLIMB; i++) a2[0][i] = a[i], b2[0][i] = b[i], a2[1][i] = b[i], b2[1][i] = a[i];
    limbs_mont_mul_n<M, 2>(o2, a2, b2);
    for (int i = 0; i < NLIMB; i++) out[NLIMB + i] = o2[0][i], out[2 * NLIMB + i] = o2[1][i];
    limbs_mont_sqr<M>(o, in[4 * NLIMB] ? b : a);
    for (int i = 0; i < NLIMB; i++) out[3 * NLIMB + i] = o[i];
    limbs_mont_mul_rows<M>(o, a, b);
    for (int i = 0; i < NLIMB; i++) out[4 * NLIMB + i] = o[i];
    const Fe<M, 2> r = redc_wide<M>(T);
    for (int i = 0; i < NLIMB; i++) out[5 * NLIMB + i] = r.l[i];
}
ZK_DEV void mq_record(const uint32_t* in, uint32_t* out) {
    mq_half<ModQ>(in, out);
    mq_half<ModQGeneric>(in, out + MQ_HALF);
}

#ifndef ZK_HOST_BUILD
__global__ void __launch_bounds__(64) k_mq(const uint32_t* in, uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) mq_record(in + (size_t)i * MQ_IN, out + (size_t)i * MQ_OUT);
}
#define MQ_HIP(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "modq_redc: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)
#endif

int main(int argc, char** argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fprintf(stderr, "modq_redc: cannot read %s\n", argv[1]), 2;
    uint32_t hdr[4];
    if (fread(hdr, 4, 4, f) != 4 || hdr[0] != MQ_MAGIC) return fprintf(stderr, "modq_redc: bad header\n"), 2;
    const uint32_t n = hdr[1];
    if (n == 0 || n > (1u << 20)) return fprintf(stderr, "modq_redc: bad record count\n"), 2;
    std::vector<uint32_t> in((size_t)n * MQ_IN), out((size_t)n * MQ_OUT, 0u);
    if (fread(in.data(), 4, in.size(), f) != in.size() || fgetc(f) != EOF) return fprintf(stderr, "modq_redc: the file's length does not match its header\n"), 2;
    fclose(f);
#ifdef ZK_HOST_BUILD
    for (uint32_t i = 0; i < n; i++) mq_record(in.data() + (size_t)i * MQ_IN, out.data() + (size_t)i * MQ_OUT);
#else
    uint32_t *d_in = nullptr, *d_out = nullptr;
    MQ_HIP(hipMalloc(&d_in, 4 * in.size()));
    MQ_HIP(hipMalloc(&d_out, 4 * out.size()));
    MQ_HIP(hipMemcpy(d_in, in.data(), 4 * in.size(), hipMemcpyHostToDevice));
    MQ_HIP(hipMemset(d_out, 0, 4 * out.size()));
    hipLaunchKernelGGL(k_mq, dim3((n + 63) / 64), dim3(64), 0, 0, d_in, d_out, n);
    MQ_HIP(hipGetLastError());
    MQ_HIP(hipDeviceSynchronize());
    MQ_HIP(hipMemcpy(out.data(), d_out, 4 * out.size(), hipMemcpyDeviceToHost));
    MQ_HIP(hipFree(d_in));
    MQ_HIP(hipFree(d_out));
#endif
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f) != 0) return fprintf(stderr, "modq_redc: cannot write %s\n", argv[2]), 2;
    return 0;
}
