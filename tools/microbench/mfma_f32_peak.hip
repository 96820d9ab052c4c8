// What the matrix pipe sustains chip-wide on v_mfma_f32_16x16x4_f32 (2 waves per SIMD, four independent accumulators per
// wave, operands of moderate magnitude in registers) -- the ceiling the fp32 scorers' compute side is measured against
// (tools/bench_maxsim_batch.py --mfma-f32-tflops).
//   hipcc --offload-arch=gfx950 -O3 mfma_f32_peak.hip -o mfma_f32_peak
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256, 2) void k(float* out, int iters, float seed) {
    const int lane = threadIdx.x & 63;
    float a[4], b[4];
    for (int j = 0; j < 4; ++j) {
        a[j] = 0.5f + 0.001f * (float)((lane * 7 + j * 13) & 63) + seed;
        b[j] = 0.25f - 0.001f * (float)((lane * 5 + j * 11) & 63);
    }
    f32x4 acc[4];
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[(r + t) & 3], b[t], acc[t], 0, 0, 0);
        }
    }
    float s = 0.f;
    for (int t = 0; t < 4; ++t) s += acc[t][0] + acc[t][1] + acc[t][2] + acc[t][3];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

int main() {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no GPU\n"); return 1; }
    const int blocks = prop.multiProcessorCount * 2, iters = 20000;
    float* out = nullptr;
    if (hipMalloc(&out, sizeof(float) * blocks * 256) != hipSuccess) return 1;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    for (int rep = 0; rep < 4; ++rep) {                   // the first is the warm-up
        (void)hipEventRecord(e0, nullptr);
        hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, nullptr, out, iters, 0.f);
        (void)hipEventRecord(e1, nullptr);
        if (hipEventSynchronize(e1) != hipSuccess) return 1;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        const double flop = 2.0 * 16 * 16 * 4 * 32.0 * iters * 4.0 * blocks;      // per MFMA x MFMAs per iteration x waves
        printf("v_mfma_f32_16x16x4_f32 rep %d  %8.3f ms  %7.1f TFLOP/s\n", rep, ms, flop / ms / 1e9);
    }
    (void)hipFree(out);
    return 0;
}
