// dense.hip -- MaxSim of un-indexed passages for a query batch (include/colbert_hip.h: clb_maxsim_batch*): the scorer between
// the encoder's device outputs, with no index and no handle.  Kernels: dense_kernels.hpp (fp32 embeddings, the oracle's bits),
// dense_half_kernels.hpp (fp16 / bf16 embeddings: clb_maxsim_batch_half*).
#include <algorithm>

#include "dense_half_kernels.hpp"

using namespace clb;

namespace {

inline int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

int check_shape(int64_t dim, int64_t T, int64_t B, int64_t n_D, int64_t N) {
    if (dim % 4 != 0 || dim < 4 || dim > 1024)
        return fail(CLB_EUNSUPPORTED, "maxsim_batch serves dim %% 4 == 0, 4 <= dim <= 1024 (dim = %lld): score one query at a time with clb_maxsim", (long long)dim);
    if (T < 1 || T > 128)
        return fail(CLB_EUNSUPPORTED, "maxsim_batch serves 1 <= T <= 128 (T = %lld): score one query at a time with clb_maxsim", (long long)T);
    if (B < 1 || N < 0 || n_D < 0) return fail(CLB_EARGUMENT, "maxsim_batch: B >= 1, N >= 0 and n_D >= 0 are required");
    return CLB_OK;
}

// How a launch is cut: G passages and QB queries per work-group, nw waves of 16 rows, and the dynamic LDS that takes.
struct DensePlan {
    int G, QB, nw;
    unsigned gx, gy;
    size_t lds;
};
DensePlan plan_dense(int dim, int T, int64_t B, int64_t N, bool owned) {
    DensePlan p;
    const int TP = T | 1;
    const int g_target = (int)std::min<int64_t>(kDenseMaxGroup, std::max<int64_t>(1, (N + 2047) / 2048));   // >= ~2048 work-groups first
    p.QB = owned ? 1 : (int)std::min<int64_t>(B, std::max(1, kDensePmWords / TP));
    p.G = std::max(1, std::min(g_target, kDensePmWords / (TP * p.QB)));
    p.nw = dim <= 512 ? 4 : 2;
    p.gx = (unsigned)((N + p.G - 1) / p.G);
    p.gy = owned ? 1u : (unsigned)((B + p.QB - 1) / p.QB);
    p.lds = kDenseHeadBytes + ((size_t)p.QB * p.G * TP * 4 + 15) / 16 * 16 + (size_t)4 * 16 * p.nw * dense_row_stride(dim);
    return p;
}

// What a host call checks before it uploads anything: the doclens against n_D, the owners against the batch.
int check_host_lists(const int64_t* doclens, int64_t N, int64_t n_D, const int32_t* owner, int64_t B) {
    int64_t total = 0;
    for (int64_t j = 0; j < N; ++j) {
        if (doclens[j] < 0) return fail(CLB_EARGUMENT, "maxsim_batch: passage %lld has a negative doclen", (long long)j);
        total += doclens[j];
    }
    if (total != n_D)  // ranking.jl:71-74
        return fail(CLB_EDIMENSION, "The total number of embeddings for pids does not match with the dimension of D!");
    for (int64_t j = 0; j < N; ++j)
        if (doclens[j] == 0) return fail(CLB_EARGUMENT, "reducing over an empty collection is not allowed (passage %lld has no embeddings)", (long long)j);
    if (owner)
        for (int64_t j = 0; j < N; ++j)
            if (owner[j] < 0 || owner[j] >= B) return fail(CLB_EBOUNDS, "passage %lld: owner %d outside 0..%lld", (long long)j, (int)owner[j], (long long)(B - 1));
    return CLB_OK;
}

// ---- 16-bit embeddings (dense_half_kernels.hpp) ----------------------------------------------------------------------------
int check_half(int q_type, int d_type, int64_t dim, int64_t T, int64_t B, int64_t n_D, int64_t N) {
    if ((d_type != CLB_F16 && d_type != CLB_BF16) || (q_type != CLB_F32 && q_type != d_type))
        return fail(CLB_EUNSUPPORTED, "maxsim_batch_half serves D in fp16 or bf16 and Q in fp32 or D's type (q_type = %d, d_type = %d)", q_type, d_type);
    if (dim % 8 != 0 || dim < 8 || dim > 1024)
        return fail(CLB_EUNSUPPORTED, "maxsim_batch_half serves dim %% 8 == 0, 8 <= dim <= 1024 (dim = %lld)", (long long)dim);
    if (T < 1 || T > 128) return fail(CLB_EUNSUPPORTED, "maxsim_batch_half serves 1 <= T <= 128 (T = %lld)", (long long)T);
    if (B < 1 || N < 0 || n_D < 0) return fail(CLB_EARGUMENT, "maxsim_batch_half: B >= 1, N >= 0 and n_D >= 0 are required");
    return CLB_OK;
}

// plan_dense's G, QB and grid; waves of 32 rows and the 16-bit rows' LDS footprint
DensePlan plan_dense_half(int dim, int T, int64_t B, int64_t N, bool owned) {
    DensePlan p = plan_dense(dim, T, B, N, owned);
    p.lds = kDenseHeadBytes + ((size_t)p.QB * p.G * (T | 1) * 4 + 15) / 16 * 16 + (size_t)2 * kDenseHalfWaveRows * p.nw * dense_half_row_stride(dim);
    return p;
}

template <typename H>
int launch_half(const void* d_Q, bool q_f32, int dim, int T, int64_t B, const void* d_D, const int64_t* d_off, int64_t N,
                const int32_t* d_owner, float* d_scores, void* d_qh, hipStream_t st) {
    const bool owned = d_owner != nullptr;
    const DensePlan p = plan_dense_half(dim, T, B, N, owned);
    if (q_f32) {                                            // Q~ = Q rounded to nearest-even, behind the offsets in the work buffer
        const int64_t n8 = B * T * dim / 8;
        hipLaunchKernelGGL(dense_round_kernel<H>, dim3((unsigned)std::min<int64_t>((n8 + 255) / 256, 4096)), dim3(256), 0, st,
                           (const float4*)d_Q, n8, (dense_u32x4*)d_qh);
    }
    auto kern = dim == 128 ? dense_maxsim_half_kernel<H, 4> : dense_maxsim_half_kernel<H, 0>;
    if (p.lds > 64 * 1024) allow_dynamic_lds(reinterpret_cast<const void*>(kern), 160 * 1024);
    hipLaunchKernelGGL(kern, dim3(p.gx, p.gy), dim3(64 * p.nw), p.lds, st, (const uint16_t*)(q_f32 ? d_qh : d_Q), dim, T, (int)B,
                       (const uint16_t*)d_D, d_off, N, d_owner, p.G, p.QB, d_scores);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

}  // namespace

extern "C" {

int64_t clb_maxsim_batch_work_bytes(int64_t N, int64_t B, int64_t T) {
    (void)B; (void)T;                                   // the scratch is the clamped offsets: per-pair maxima never leave LDS
    return align256((int64_t)sizeof(int64_t) * (std::max<int64_t>(N, 0) + 1));
}

int clb_maxsim_batch_device(int device, const float* d_Q, int64_t dim, int64_t T, int64_t B, const float* d_D, int64_t n_D,
                            const int64_t* d_doclens, int64_t N, const int32_t* d_owner, float* d_scores, void* d_work,
                            int64_t work_bytes, void* hip_stream) {
    CLB_TRY(check_shape(dim, T, B, n_D, N));
    if (N == 0) return CLB_OK;
    if (!d_Q || !d_doclens || !d_scores || !d_work || (!d_D && n_D > 0)) return fail(CLB_EARGUMENT, "maxsim_batch: null argument");
    if ((uintptr_t)d_D % 16 || (uintptr_t)d_work % 8) return fail(CLB_EARGUMENT, "maxsim_batch: D must be 16-byte aligned and the work buffer 8-byte aligned");
    if (work_bytes < clb_maxsim_batch_work_bytes(N, B, T))
        return fail(CLB_EARGUMENT, "maxsim_batch: work buffer of %lld bytes, clb_maxsim_batch_work_bytes asks for %lld", (long long)work_bytes,
                    (long long)clb_maxsim_batch_work_bytes(N, B, T));
    const bool owned = d_owner != nullptr;
    const DensePlan p = plan_dense((int)dim, (int)T, B, N, owned);
    if (p.gy > 65535u || (N + p.G - 1) / p.G > 0x7fffffffLL) return fail(CLB_EUNSUPPORTED, "maxsim_batch: B = %lld, N = %lld exceed one launch", (long long)B, (long long)N);
    CLB_TRY(use_device(device));
    hipStream_t st = (hipStream_t)hip_stream;
    int64_t* d_off = reinterpret_cast<int64_t*>(d_work);
    hipLaunchKernelGGL(dense_offsets_kernel, dim3(1), dim3(1024), 0, st, d_doclens, N, n_D, d_off);
    auto kern = dim == 128 ? dense_maxsim_kernel<32> : dense_maxsim_kernel<0>;
    if (p.lds > 64 * 1024) allow_dynamic_lds(reinterpret_cast<const void*>(kern), 160 * 1024);
    hipLaunchKernelGGL(kern, dim3(p.gx, p.gy), dim3(64 * p.nw), p.lds, st, d_Q, (int)dim, (int)T, (int)B, d_D, (const int64_t*)d_off, N,
                       d_owner, p.G, p.QB, d_scores);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

int clb_maxsim_batch(int device, const float* Q, int64_t dim, int64_t T, int64_t B, const float* D, int64_t n_D,
                     const int64_t* doclens, int64_t N, const int32_t* owner, float* scores) {
    CLB_TRY(check_shape(dim, T, B, n_D, N));
    if (N > 0 && (!doclens || !scores || !Q)) return fail(CLB_EARGUMENT, "maxsim_batch: null argument");
    CLB_TRY(check_host_lists(doclens, N, n_D, owner, B));
    CLB_TRY(use_device(device));
    if (N == 0) return CLB_OK;
    hipStream_t st = nullptr;
    CLB_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const int64_t n_scores = owner ? N : N * B, wb = clb_maxsim_batch_work_bytes(N, B, T);
    DevBuf dQ, dD, dL, dO, dS, dW;
    int rc = upload(dQ, Q, sizeof(float) * dim * T * B, st);
    if (!rc) rc = upload(dD, D, sizeof(float) * dim * n_D, st);
    if (!rc) rc = upload(dL, doclens, sizeof(int64_t) * N, st);
    if (!rc && owner) rc = upload(dO, owner, sizeof(int32_t) * N, st);
    if (!rc) rc = dS.alloc(sizeof(float) * n_scores);
    if (!rc) rc = dW.alloc((size_t)wb);
    if (!rc)
        rc = clb_maxsim_batch_device(device, dQ.as<float>(), dim, T, B, dD.as<float>(), n_D, dL.as<int64_t>(), N,
                                     owner ? dO.as<int32_t>() : nullptr, dS.as<float>(), dW.p, wb, st);
    if (!rc && hipMemcpyAsync(scores, dS.p, sizeof(float) * n_scores, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = fail(CLB_EHIP, "maxsim_batch: copying the scores back failed");
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(CLB_EHIP, "maxsim_batch: hipStreamSynchronize failed");
    (void)hipStreamDestroy(st);
    return rc;
}

int64_t clb_maxsim_batch_half_work_bytes(int64_t N, int64_t B, int64_t T, int64_t dim) {
    const int64_t q = std::max<int64_t>(B, 0) * std::max<int64_t>(T, 0) * std::max<int64_t>(dim, 0);   // Q~, when Q arrives in fp32
    return clb_maxsim_batch_work_bytes(N, B, T) + align256(2 * q);
}

int clb_maxsim_batch_half_device(int device, const void* d_Q, int q_type, int64_t dim, int64_t T, int64_t B, const void* d_D,
                                 int d_type, int64_t n_D, const int64_t* d_doclens, int64_t N, const int32_t* d_owner,
                                 float* d_scores, void* d_work, int64_t work_bytes, void* hip_stream) {
    CLB_TRY(check_half(q_type, d_type, dim, T, B, n_D, N));
    if (N == 0) return CLB_OK;
    if (!d_Q || !d_doclens || !d_scores || !d_work || (!d_D && n_D > 0)) return fail(CLB_EARGUMENT, "maxsim_batch_half: null argument");
    if ((uintptr_t)d_D % 16 || (uintptr_t)d_Q % 16 || (uintptr_t)d_work % 16)
        return fail(CLB_EARGUMENT, "maxsim_batch_half: Q, D and the work buffer must be 16-byte aligned");
    if (work_bytes < clb_maxsim_batch_half_work_bytes(N, B, T, dim))
        return fail(CLB_EARGUMENT, "maxsim_batch_half: work buffer of %lld bytes, clb_maxsim_batch_half_work_bytes asks for %lld",
                    (long long)work_bytes, (long long)clb_maxsim_batch_half_work_bytes(N, B, T, dim));
    const DensePlan p = plan_dense_half((int)dim, (int)T, B, N, d_owner != nullptr);
    if (p.gy > 65535u || (N + p.G - 1) / p.G > 0x7fffffffLL)
        return fail(CLB_EUNSUPPORTED, "maxsim_batch_half: B = %lld, N = %lld exceed one launch", (long long)B, (long long)N);
    CLB_TRY(use_device(device));
    hipStream_t st = (hipStream_t)hip_stream;
    int64_t* d_off = reinterpret_cast<int64_t*>(d_work);
    void* d_qh = reinterpret_cast<unsigned char*>(d_work) + clb_maxsim_batch_work_bytes(N, B, T);
    hipLaunchKernelGGL(dense_offsets_kernel, dim3(1), dim3(1024), 0, st, d_doclens, N, n_D, d_off);
    return (d_type == CLB_F16 ? launch_half<DenseF16> : launch_half<DenseBF16>)(d_Q, q_type == CLB_F32, (int)dim, (int)T, B, d_D, d_off, N,
                                                                                 d_owner, d_scores, d_qh, st);
}

int clb_maxsim_batch_half(int device, const void* Q, int q_type, int64_t dim, int64_t T, int64_t B, const void* D, int d_type,
                          int64_t n_D, const int64_t* doclens, int64_t N, const int32_t* owner, float* scores) {
    CLB_TRY(check_half(q_type, d_type, dim, T, B, n_D, N));
    if (N > 0 && (!doclens || !scores || !Q)) return fail(CLB_EARGUMENT, "maxsim_batch_half: null argument");
    CLB_TRY(check_host_lists(doclens, N, n_D, owner, B));
    CLB_TRY(use_device(device));
    if (N == 0) return CLB_OK;
    hipStream_t st = nullptr;
    CLB_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const int64_t n_scores = owner ? N : N * B, wb = clb_maxsim_batch_half_work_bytes(N, B, T, dim);
    DevBuf dQ, dD, dL, dO, dS, dW;
    int rc = upload(dQ, Q, (size_t)(q_type == CLB_F32 ? 4 : 2) * dim * T * B, st);
    if (!rc) rc = upload(dD, D, (size_t)2 * dim * n_D, st);
    if (!rc) rc = upload(dL, doclens, sizeof(int64_t) * N, st);
    if (!rc && owner) rc = upload(dO, owner, sizeof(int32_t) * N, st);
    if (!rc) rc = dS.alloc(sizeof(float) * n_scores);
    if (!rc) rc = dW.alloc((size_t)wb);
    if (!rc)
        rc = clb_maxsim_batch_half_device(device, dQ.p, q_type, dim, T, B, dD.p, d_type, n_D, dL.as<int64_t>(), N,
                                          owner ? dO.as<int32_t>() : nullptr, dS.as<float>(), dW.p, wb, st);
    if (!rc && hipMemcpyAsync(scores, dS.p, sizeof(float) * n_scores, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = fail(CLB_EHIP, "maxsim_batch_half: copying the scores back failed");
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(CLB_EHIP, "maxsim_batch_half: hipStreamSynchronize failed");
    (void)hipStreamDestroy(st);
    return rc;
}

}  // extern "C"
