// The bare v_mfma_scale_f32_16x16x128_f8f6f4, MXFP8 (E4M3) and MXFP4 (E2M1) rows against MXFP8 tokens, apart from the dense
// MaxSim kernel (this file includes nothing of the library):
//   error  single MFMAs from a zero accumulator on random 16 x 128 blocks with a random E8M0 scale per (row, block of 32),
//          against the float64 dot of the decoded operands.  Printed: the largest |got - exact| / sum_k |a_k b_k| over all
//          256 entries of every trial, as a power of two -- the unit u of the instruction's adder that the bound of
//          tests/test_gpu_maxsim_batch_mx.py assumes (u = 2^-23 unless this says more).  Two draws: every non-NaN code
//          (magnitudes log-uniform over the format, scale bytes 120..134), and codes of the top two binades under scale bytes
//          118..122 (what quantised unit-norm embeddings look like: every block's amax sits in the top binade).
//   rate   what the matrix pipe sustains chip-wide on the instruction (2 waves per SIMD, four independent accumulators, operands
//          in registers), the ceiling the all-pairs form of the dense kernel is measured against (profiles/maxsim_batch_mx.md).
// Operand layout as the dense kernel's exact test pins it: lane (r, g) = (lane % 16, lane / 16); an 8-bit operand holds
// k = 16 g .. 16 g + 15 in registers 0-3 and k = 64 + 16 g .. in registers 4-7; a 4-bit operand k = 32 g .. 32 g + 31 in registers
// 0-3, element 2 i in the low nibble of byte i; block b is scaled by byte 0 of lane group b's scale register; accumulator entry
// i of lane (r, g) is row 4 g + i, column r.
//   hipcc --offload-arch=gfx950 -O3 mfma_scale_mx.hip -o mfma_scale_mx && ./mfma_scale_mx
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// One wave per trial.  A: rows (16, AB bytes) with AB = 128 (E4M3) or 64 (E2M1); B: tokens (16, 128); SA, SB: (16, 4) scale bytes;
// out (16 rows, 16 tokens).
template <bool E2M1>
__global__ __launch_bounds__(64) void one_mfma(const unsigned char* A, const unsigned char* B, const unsigned char* SA,
                                               const unsigned char* SB, float* out) {
    constexpr int AB = E2M1 ? 64 : 128;
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const size_t t = blockIdx.x;
    const int* pa = reinterpret_cast<const int*>(A + (t * 16 + r) * AB + 16 * g);
    const int* pb = reinterpret_cast<const int*>(B + (t * 16 + r) * 128 + 16 * g);
    i32x8 a = {}, b;
    for (int j = 0; j < 4; ++j) {
        a[j] = pa[j];
        if (!E2M1) a[4 + j] = pa[16 + j];
        b[j] = pb[j];
        b[4 + j] = pb[16 + j];
    }
    const int sa = SA[(t * 16 + r) * 4 + g], sb = SB[(t * 16 + r) * 4 + g];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, E2M1 ? 4 : 0, 0, 0, sa, 0, sb);
    for (int i = 0; i < 4; ++i) out[t * 256 + (4 * g + i) * 16 + r] = acc[i];
}

template <bool E2M1>
__global__ __launch_bounds__(256, 2) void stream_mfma(float* out, int iters, unsigned seed) {
    const int lane = threadIdx.x & 63;
    i32x8 a[2] = {}, b[2];
    for (int q = 0; q < 2; ++q)
        for (int j = 0; j < 8; ++j) {               // E4M3 bytes below 2 in magnitude (no NaN code); any nibble is a finite E2M1
            if (!E2M1 || j < 4) a[q][j] = (int)((((lane + 1) * 2654435761u * (j + 1 + 8 * q) + seed) & (E2M1 ? 0xffffffffu : 0xbfbfbfbfu)));
            b[q][j] = (int)(((lane + 7) * 40503u * (j + 3 + 8 * q) + seed) & 0xbfbfbfbfu);
        }
    f32x4 acc[4];
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int rep = 0; rep < 3; ++rep) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[t & 1], b[t >> 1], acc[t], E2M1 ? 4 : 0, 0, 0, 127, 0, 127);
        }
    }
    float s = 0.f;
    for (int t = 0; t < 4; ++t) for (int j = 0; j < 4; ++j) s += acc[t][j];
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 24);
}
static double e4m3(unsigned c) {
    const int e = c >> 3 & 15, m = c & 7;
    const double v = e ? std::ldexp(1.0 + m / 8.0, e - 7) : std::ldexp(m / 8.0, -6);
    return c & 0x80 ? -v : v;
}
static double e2m1(unsigned c) {
    static const double mag[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
    return c & 8 ? -mag[c & 7] : mag[c & 7];
}
static unsigned draw_e4m3(int top) {      // 0: every non-NaN code; 1: the top two binades; 2: every normal code and zero
    unsigned c;
    do c = rnd() & 0xff; while ((c & 0x7f) == 0x7f);
    if (top == 2 && (c & 0x78) == 0) c &= 0x80;
    if (top == 1) c = (c & 0x87) | ((14 + (rnd() & 1)) << 3), c -= (c & 0x7f) == 0x7f;   // binades 2^7, 2^8; 0x7F -> 0x7E (448)
    return c;
}
static unsigned draw_e2m1(int top) { return top == 1 ? (rnd() & 8) | (4 + (rnd() & 3)) : rnd() & 15; }

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

template <bool E2M1>
int error_run(const char* name, int top, int slo, int shi, int trials) {
    constexpr int AB = E2M1 ? 64 : 128;
    std::vector<unsigned char> A((size_t)trials * 16 * AB), B((size_t)trials * 16 * 128), SA((size_t)trials * 64), SB((size_t)trials * 64);
    std::vector<float> out((size_t)trials * 256);
    for (auto& x : B) x = (unsigned char)draw_e4m3(top);
    for (auto& x : A) x = E2M1 ? (unsigned char)(draw_e2m1(top) | draw_e2m1(top) << 4) : (unsigned char)draw_e4m3(top);
    for (auto& x : SA) x = (unsigned char)(slo + rnd() % (shi - slo + 1));
    for (auto& x : SB) x = (unsigned char)(slo + rnd() % (shi - slo + 1));
    unsigned char *dA, *dB, *dSA, *dSB;
    float* dout;
    CHECK(hipMalloc(&dA, A.size())); CHECK(hipMalloc(&dB, B.size())); CHECK(hipMalloc(&dSA, SA.size())); CHECK(hipMalloc(&dSB, SB.size()));
    CHECK(hipMalloc(&dout, out.size() * 4));
    CHECK(hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice)); CHECK(hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dSA, SA.data(), SA.size(), hipMemcpyHostToDevice)); CHECK(hipMemcpy(dSB, SB.data(), SB.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(one_mfma<E2M1>, dim3(trials), dim3(64), 0, 0, dA, dB, dSA, dSB, dout);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
    double worst = 0.0, worst_res = 0.0;       // in units of sum |a b|; and of the result's own magnitude
    long exact_entries = 0;
    for (int t = 0; t < trials; ++t)
        for (int r = 0; r < 16; ++r)
            for (int c = 0; c < 16; ++c) {
                double dot = 0.0, mag = 0.0;
                for (int k = 0; k < 128; ++k) {
                    const unsigned char ab = A[((size_t)t * 16 + r) * AB + (E2M1 ? k >> 1 : k)];
                    const double av = E2M1 ? e2m1(k & 1 ? ab >> 4 : ab & 15) : e4m3(ab);
                    const double p = std::ldexp(av, SA[((size_t)t * 16 + r) * 4 + k / 32] - 127) *
                                     std::ldexp(e4m3(B[((size_t)t * 16 + c) * 128 + k]), SB[((size_t)t * 16 + c) * 4 + k / 32] - 127);
                    dot += p;
                    mag += std::fabs(p);
                }
                const double err = std::fabs((double)out[(size_t)t * 256 + r * 16 + c] - dot);
                exact_entries += err == 0.0;
                if (mag > 0.0 && err / mag > worst) worst = err / mag;
                if (dot != 0.0 && err / std::fabs(dot) > worst_res) worst_res = err / std::fabs(dot);
            }
    printf("error %-36s %6d MFMAs: max |got - exact| / sum|a b| = %.4e = 2^%.2f   (/ |exact| = 2^%.2f; %ld of %ld entries exact)\n", name, trials,
           worst, worst > 0 ? std::log2(worst) : -INFINITY, worst_res > 0 ? std::log2(worst_res) : -INFINITY, exact_entries, (long)trials * 256);
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dSA); (void)hipFree(dSB); (void)hipFree(dout);
    return 0;
}

template <bool E2M1>
int rate_run(const char* name, float* out, int grid) {
    const int iters = 4000;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    double best = 0.0, sum = 0.0;
    for (int rep = 0; rep < 4; ++rep) {            // rep 0 warms up
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(stream_mfma<E2M1>, dim3(grid), dim3(256), 0, 0, out, iters, 1u + rep);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        const double tf = (double)grid * 4 * iters * 12 * 65536.0 / ms / 1e9;
        if (rep) { sum += tf; if (tf > best) best = tf; }
    }
    printf("rate  %-34s %7.0f TFLOP/s mean of 3, best %7.0f\n", name, sum / 3, best);
    return 0;
}

int main() {
    int rc = 0;
    rc |= error_run<false>("E4M3 x E4M3, every code, 120..134", false, 120, 134, 2048);
    rc |= error_run<false>("E4M3 x E4M3, every code, 125..130", false, 125, 130, 2048);
    rc |= error_run<false>("E4M3 x E4M3, every code, 127", false, 127, 127, 2048);
    rc |= error_run<false>("E4M3 x E4M3, normal codes, 127", 2, 127, 127, 2048);
    rc |= error_run<false>("E4M3 x E4M3, normal codes, 120..134", 2, 120, 134, 2048);
    rc |= error_run<false>("E4M3 x E4M3, top binades, 118..122", true, 118, 122, 2048);
    rc |= error_run<false>("E4M3 x E4M3, top binades, 120..134", true, 120, 134, 2048);
    rc |= error_run<true>("E2M1 x E4M3, every code, 120..134", false, 120, 134, 2048);
    rc |= error_run<true>("E2M1 x E4M3, every code, 127", false, 127, 127, 2048);
    rc |= error_run<true>("E2M1 x E4M3, normal codes, 127", 2, 127, 127, 2048);
    rc |= error_run<true>("E2M1 x E4M3, top binades, 118..122", true, 118, 122, 2048);
    rc |= error_run<true>("E2M1 x E4M3, top binades, 120..134", true, 120, 134, 2048);
    if (rc) return rc;
    float* out;
    CHECK(hipMalloc(&out, sizeof(float) * 2048 * 256));
    rc |= rate_run<false>("E4M3 x E4M3, 2 waves per SIMD", out, 2048);
    rc |= rate_run<true>("E2M1 x E4M3, 2 waves per SIMD", out, 2048);
    (void)hipFree(out);
    return rc;
}
