// stamp_boundary.hip -- what does one timestamp at a launch boundary cost on an in-order stream that carries a 5 us
// kernel between boundaries?  Three forms: hipEventRecord; a one-thread kernel that stores wall_clock64() (the 100 MHz
// counter hipEventElapsedTime reports in); the same store by thread 0 of workgroup 0 of the kernel that starts there.
//   hipcc --offload-arch=gfx950 -O3 -o stamp_boundary stamp_boundary.hip && ./stamp_boundary
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <chrono>

#define OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorName(e_)); return 1; } } while (0)
constexpr int kBoundaries = 400, kRounds = 5;

__global__ void k_busy(unsigned long long *slot, unsigned ticks)      // slot != nullptr: the stamp rides along
{
    const unsigned long long t0 = wall_clock64();
    if (slot && blockIdx.x == 0 && threadIdx.x == 0) *slot = t0;
    while (wall_clock64() - t0 < ticks) {}
}
__global__ void k_stamp(unsigned long long *slot) { *slot = wall_clock64(); }

int main()
{
    hipStream_t s;
    unsigned long long *slots;
    hipEvent_t ev[kBoundaries];
    OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    OK(hipMalloc((void **)&slots, kBoundaries * sizeof(*slots)));
    for (hipEvent_t &e : ev) OK(hipEventCreate(&e));
    const char *names[4] = {"no boundary", "hipEventRecord", "one-thread stamp kernel", "stamp in the next kernel"};
    double best[4][2];
    for (int form = 0; form < 4; ++form) {
        best[form][0] = best[form][1] = 1e30;
        for (int r = 0; r < kRounds + 1; ++r) {                       // (the first round warms up)
            OK(hipStreamSynchronize(s));
            const auto t0 = std::chrono::steady_clock::now();
            for (int i = 0; i < kBoundaries; ++i) {
                if (form == 1) OK(hipEventRecord(ev[i], s));
                if (form == 2) k_stamp<<<1, 1, 0, s>>>(slots + i);
                k_busy<<<256, 256, 0, s>>>(form == 3 ? slots + i : nullptr, 500u);
            }
            const auto t1 = std::chrono::steady_clock::now();
            OK(hipStreamSynchronize(s));
            const auto t2 = std::chrono::steady_clock::now();
            const double host = std::chrono::duration<double, std::micro>(t1 - t0).count() / kBoundaries;
            const double all = std::chrono::duration<double, std::micro>(t2 - t0).count() / kBoundaries;
            if (r > 0 && all < best[form][1]) { best[form][0] = host; best[form][1] = all; }
        }
        printf("%-26s %7.2f us per boundary + kernel (host enqueue %5.2f us)  extra over no boundary %6.2f us\n", names[form],
               best[form][1], best[form][0], best[form][1] - best[0][1]);
    }
    OK(hipGetLastError());
    return 0;
}
