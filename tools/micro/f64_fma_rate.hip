// f64_fma_rate.hip -- what the chip sustains in dependent-free f64 vector FMAs (development micro-benchmark; tools/raycast_cost.py
// runs it to put the brute-force ray cast's f64 arithmetic next to the chip's rate).
//   hipcc --offload-arch=gfx950 -O3 tools/micro/f64_fma_rate.hip -o tools/micro/bin/f64_fma_rate && tools/micro/bin/f64_fma_rate
// Every lane runs kIters x 8 independent fma(x, a, b) chains; the grid is swept so that the best occupancy shows.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
constexpr int kIters = 4096, kChains = 8;

__global__ __launch_bounds__(256) void k_fma64(double* out, double a, double b) {
    double x[kChains];
    for (int i = 0; i < kChains; i++) x[i] = threadIdx.x * 1e-3 + i;
    for (int it = 0; it < kIters; it++) {
#pragma unroll
        for (int i = 0; i < kChains; i++) x[i] = __builtin_fma(x[i], a, b);
    }
    double s = 0;
    for (int i = 0; i < kChains; i++) s += x[i];
    out[static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x] = s;
}

int main() {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { fprintf(stderr, "no HIP device\n"); return 1; }
    const int cus = prop.multiProcessorCount;
    const int max_blocks = cus * 16;
    double* out = nullptr;
    if (hipMalloc(&out, static_cast<size_t>(max_blocks) * 256 * sizeof(double)) != hipSuccess) return 1;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    double best = 0.0;
    for (int per_cu : {2, 4, 8, 16}) {
        const int blocks = cus * per_cu;
        std::vector<float> ms;
        for (int rep = 0; rep < 7; rep++) {
            (void)hipEventRecord(e0, nullptr);
            hipLaunchKernelGGL(k_fma64, dim3(blocks), dim3(256), 0, nullptr, out, 0.999999, 1e-9);
            (void)hipEventRecord(e1, nullptr);
            if (hipEventSynchronize(e1) != hipSuccess) return 1;
            float t = 0; (void)hipEventElapsedTime(&t, e0, e1);
            if (rep >= 2) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        const double fma = static_cast<double>(blocks) * 256 * kIters * kChains / (ms[ms.size() / 2] * 1e-3);
        printf("f64 fma loop: %d CUs, %2d workgroups of 256 per CU: %.3f ms, %.3g f64 FMA/s = %.3g f64 flop/s\n", cus, per_cu, ms[ms.size() / 2], fma, 2 * fma);
        best = std::max(best, fma);
    }
    printf("f64 fma loop best: %.4g f64 FMA/s (%.4g f64 operations/s counting an FMA as two)\n", best, 2 * best);
    (void)hipFree(out);
    return 0;
}
