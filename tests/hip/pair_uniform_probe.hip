// Device probe for the UNIFORM form of pair_response (gpu-physics-engine_amd/csrc/k_pair.h): the form the direct-slot tiles
// run while every particle has one ordinary radius.  Same records and output as pair_probe.hip; the radii of the records
// are not read -- the one radius of the launch comes from the command line, as the kernels get theirs from the host, and
// UniformRadii is formed from it once per lane as the tiles form it once per tile.  Built and driven by
// tests/test_gpu_pair_math_uniform.py, which compares the output with the IEEE binary32 restatement of the oracle's pair
// at r1 == r2 == that radius.
//
//   pair_uniform_probe <in.bin> <out.bin> <radius bits, hex>
//   in:  n records of 8 x 32-bit words: p1x p1y p2x p2y (r1 r2: ignored) stiffness active (u32, 0 or 1); n % 64 == 0
//   out: n records of 11 x 32-bit words:
//        p1x p1y p2x p2y hit      pair_response<true>(active, p1, p2, U) -- both particles, hit bit
//        ax ay hit_a              pair_response<false>(active, p1, p2, U) -- p1's half (the lower lane)
//        bx by hit_b              pair_response<false>(active, p2, p1, U) -- p2's half (the upper lane)
// `careful` is computed from the call's own particle, as the lane-group kernels do.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

__global__ void __launch_bounds__(256) probe(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, const uint32_t n,
                                            const float radius)
{
    using namespace gpe;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;         // n % 64 == 0: every wave is whole or absent
    if (i >= n) return;                                               // (wave-uniform)
    const uint32_t *r = in + (size_t)i * kIn;
    const f32x2 p1 = {__uint_as_float(r[0]), __uint_as_float(r[1])};
    const f32x2 p2 = {__uint_as_float(r[2]), __uint_as_float(r[3])};
    const float stiffness = __uint_as_float(r[6]);
    const uint64_t active = ballot64(r[7] != 0u);
    const UniformRadii U = uniform_radii(radius);

    f32x2 b1 = p1, b2 = p2;
    const uint64_t hit = pair_response<true>(active, b1, b2, U, stiffness);
    f32x2 a = p1;                                                     // the lower particle's lane
    const uint64_t hit_a = pair_response<false>(active, a, p2, U, stiffness, ~0ull, neg_zero_lanes(p1));
    f32x2 b = p2;                                                     // the upper particle's lane
    const uint64_t hit_b = pair_response<false>(active, b, p1, U, stiffness, 0ull, neg_zero_lanes(p2));

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
    if (argc != 4) {
        fprintf(stderr, "usage: %s <in.bin> <out.bin> <radius bits, hex>\n", argv[0]);
        return 1;
    }
    const uint32_t radius_bits = (uint32_t)strtoul(argv[3], nullptr, 16);
    float radius;
    memcpy(&radius, &radius_bits, sizeof(radius));
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
    probe<<<(n + 255) / 256, 256>>>(d_in, d_out, n, radius);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));

    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 1; }
    if (fwrite(out.data(), 4, out.size(), g) != out.size()) { fprintf(stderr, "short write\n"); return 1; }
    fclose(g);
    printf("pair_uniform_probe: %u records, radius %a\n", n, (double)radius);
    return 0;
}
