// Device probe for cell membership and the Verlet step: runs neighbour_overlap_mask (gpu-physics-engine_amd/csrc/
// k_cells.h, the NATIVE hash kernel's form), cell_coord / is_obj_in_cell and verlet_one (gpe_internal.h, the compat
// kernels' forms and every write-back's integration) on records read from a file, 64 records per wave, and writes what
// each lane computed.  Built and driven by tests/test_gpu_cell_math.py, which compares the output with an IEEE binary32
// restatement of the oracle's.
//
//   cell_probe cells <in.bin> <out.bin>
//   in:  n records of 4 x 32-bit words: px py r cell_size; n % 64 == 0
//   out: n records of 4 x 32-bit words:
//        cx cy          cell_coord(px, cell_size), cell_coord(py, cell_size)
//        mask_native    neighbour_overlap_mask(p, r, cx, cy, cell_size)
//        mask_compat    the same 8 bits from is_obj_in_cell(px, py, r * r, cx + x, cy + y, cell_size) in the reference's
//                       scan order (y outer, x inner, centre skipped; the add wraps as u32, as the oracle's does)
//
//   cell_probe verlet <in.bin> <out.bin>
//   in:  n records of 14 x 32-bit words: cx cy qx qy r dt_squared world_w world_h acc_x acc_y mouse_pressed (u32)
//        mouse_x mouse_y mouse_strength; n % 64 == 0
//   out: n records of 2 x 32-bit words: nx ny from verlet_one
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "gpe_internal.h"
#include "k_cells.h"

#define CHECK(x)                                                                         \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) {                                                          \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(2);                                                                     \
        }                                                                                \
    } while (0)

constexpr int kCellsIn = 4, kCellsOut = 4, kVerletIn = 14, kVerletOut = 2;

__global__ void __launch_bounds__(256) probe_cells(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, const uint32_t n)
{
    using namespace gpe;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;         // n % 64 == 0: every wave is whole or absent
    if (i >= n) return;
    const uint32_t *r = in + (size_t)i * kCellsIn;
    const float px = __uint_as_float(r[0]), py = __uint_as_float(r[1]), rad = __uint_as_float(r[2]);
    const float cs = __uint_as_float(r[3]);
    const int32_t cx = cell_coord(px, cs), cy = cell_coord(py, cs);
    const uint32_t native = neighbour_overlap_mask(make_float2(px, py), rad, cx, cy, cs);
    const float sq_radius = rad * rad;
    uint32_t compat = 0;
    int k = 0;
#pragma unroll
    for (int y = -1; y <= 1; ++y) {
#pragma unroll
        for (int x = -1; x <= 1; ++x) {
            if (x == 0 && y == 0) continue;
            const int32_t nx = (int32_t)((uint32_t)cx + (uint32_t)x);
            const int32_t ny = (int32_t)((uint32_t)cy + (uint32_t)y);
            compat |= is_obj_in_cell(px, py, sq_radius, nx, ny, cs) ? (1u << k) : 0u;
            ++k;
        }
    }
    uint32_t *o = out + (size_t)i * kCellsOut;
    o[0] = (uint32_t)cx; o[1] = (uint32_t)cy; o[2] = native; o[3] = compat;
}

__global__ void __launch_bounds__(256) probe_verlet(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, const uint32_t n)
{
    using namespace gpe;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *r = in + (size_t)i * kVerletIn;
    VerletParams P;
    P.dt_squared = __uint_as_float(r[5]);
    P.world_w = __uint_as_float(r[6]); P.world_h = __uint_as_float(r[7]);
    P.acc_x = __uint_as_float(r[8]); P.acc_y = __uint_as_float(r[9]);
    P.mouse_pressed = r[10];
    P.mouse_x = __uint_as_float(r[11]); P.mouse_y = __uint_as_float(r[12]); P.mouse_strength = __uint_as_float(r[13]);
    float nx, ny;
    verlet_one(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3]),
               __uint_as_float(r[4]), P, nx, ny);
    uint32_t *o = out + (size_t)i * kVerletOut;
    o[0] = __float_as_uint(nx); o[1] = __float_as_uint(ny);
}

int main(int argc, char **argv)
{
    const bool cells = argc == 4 && !strcmp(argv[1], "cells"), verlet = argc == 4 && !strcmp(argv[1], "verlet");
    if (!cells && !verlet) {
        fprintf(stderr, "usage: %s cells|verlet <in.bin> <out.bin>\n", argv[0]);
        return 1;
    }
    const int k_in = cells ? kCellsIn : kVerletIn, k_out = cells ? kCellsOut : kVerletOut;
    FILE *f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % (long)(k_in * 4 * 64) != 0) {
        fprintf(stderr, "%s: %ld bytes is not a whole number of 64-record waves\n", argv[2], bytes);
        return 1;
    }
    const uint32_t n = (uint32_t)(bytes / (k_in * 4));
    std::vector<uint32_t> in((size_t)n * k_in), out((size_t)n * k_out);
    if (fread(in.data(), 4, in.size(), f) != in.size()) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);

    uint32_t *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc(&d_in, in.size() * 4));
    CHECK(hipMalloc(&d_out, out.size() * 4));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xFF, out.size() * 4));
    if (cells) probe_cells<<<(n + 255) / 256, 256>>>(d_in, d_out, n);
    else probe_verlet<<<(n + 255) / 256, 256>>>(d_in, d_out, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));

    FILE *g = fopen(argv[3], "wb");
    if (!g) { perror(argv[3]); return 1; }
    if (fwrite(out.data(), 4, out.size(), g) != out.size()) { fprintf(stderr, "short write\n"); return 1; }
    fclose(g);
    printf("cell_probe %s: %u records\n", argv[1], n);
    return 0;
}
