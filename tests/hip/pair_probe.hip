// Device probe for pair_response (gpu-physics-engine_amd/csrc/k_pair.h): runs the collide kernels' pair arithmetic
// on records read from a file, 64 records per wave, and writes what each lane computed.  Built and driven by
// tests/test_gpu_pair_math.py, which compares the output with an IEEE binary32 restatement of the oracle's pair.
//
//   pair_probe <in.bin> <out.bin>
//   in:  n records of 8 x 32-bit words: p1x p1y p2x p2y r1 r2 stiffness active (u32, 0 or 1); n % 64 == 0
//   out: n records of 11 x 32-bit words:
//        p1x p1y p2x p2y hit      pair_response<true>(active, p1, p2, r1, r2) -- both particles, hit bit
//        ax ay hit_a              pair_response<false>(active, p1, p2, r1, r2) -- p1's half (the lower lane)
//        bx by hit_b              pair_response<false>(active, p2, p1, r2, r1) -- p2's half (the upper lane)
// `plain` and `careful` are computed from the call's own particle, as the lane-group kernels do.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "gpe_internal.h"
#include "k_pair.h"

#define CHECK(x)                                                                         \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) {                                                          \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(2);                                                                     \
        }                                                                                \
    } while (0)

constexpr int kIn = 8, kOut = 11;

__global__ void __launch_bounds__(256) probe(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, const uint32_t n)
{
    using namespace gpe;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;         // n % 64 == 0: every wave is whole or absent
    if (i >= n) return;                                               // (wave-uniform)
    const uint32_t *r = in + (size_t)i * kIn;
    const f32x2 p1 = {__uint_as_float(r[0]), __uint_as_float(r[1])};
    const f32x2 p2 = {__uint_as_float(r[2]), __uint_as_float(r[3])};
    const float r1 = __uint_as_float(r[4]), r2 = __uint_as_float(r[5]), stiffness = __uint_as_float(r[6]);
    const uint64_t active = ballot64(r[7] != 0u);

    f32x2 b1 = p1, b2 = p2;
    const uint64_t hit = pair_response<true>(active, b1, b2, r1, r2, plain_radius_lanes(r1), stiffness);
    f32x2 a = p1;                                                     // the lower particle's lane
    const uint64_t hit_a = pair_response<false>(active, a, p2, r1, r2, plain_radius_lanes(r1), stiffness, ~0ull,
                                                neg_zero_lanes(p1));
    f32x2 b = p2;                                                     // the upper particle's lane
    const uint64_t hit_b = pair_response<false>(active, b, p1, r2, r1, plain_radius_lanes(r2), stiffness, 0ull,
                                                neg_zero_lanes(p2));

    uint32_t *o = out + (size_t)i * kOut;
    const uint64_t me = 1ull << lane_id();
    o[0] = __float_as_uint(b1.x); o[1] = __float_as_uint(b1.y);
    o[2] = __float_as_uint(b2.x); o[3] = __float_as_uint(b2.y);
    o[4] = (hit & me) ? 1u : 0u;
    o[5] = __float_as_uint(a.x); o[6] = __float_as_uint(a.y);
    o[7] = (hit_a & me) ? 1u : 0u;
    o[8] = __float_as_uint(b.x); o[9] = __float_as_uint(b.y);
    o[10] = (hit_b & me) ? 1u : 0u;
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s <in.bin> <out.bin>\n", argv[0]);
        return 1;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % (long)(kIn * 4 * 64) != 0) {
        fprintf(stderr, "%s: %ld bytes is not a whole number of 64-record waves\n", argv[1], bytes);
        return 1;
    }
    const uint32_t n = (uint32_t)(bytes / (kIn * 4));
    std::vector<uint32_t> in((size_t)n * kIn), out((size_t)n * kOut);
    if (fread(in.data(), 4, in.size(), f) != in.size()) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);

    uint32_t *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc(&d_in, in.size() * 4));
    CHECK(hipMalloc(&d_out, out.size() * 4));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xFF, out.size() * 4));
    probe<<<(n + 255) / 256, 256>>>(d_in, d_out, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));

    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 1; }
    if (fwrite(out.data(), 4, out.size(), g) != out.size()) { fprintf(stderr, "short write\n"); return 1; }
    fclose(g);
    printf("pair_probe: %u records\n", n);
    return 0;
}
