// dense.hip -- MaxSim of un-indexed passages for a query batch (include/colbert_hip.h: clb_maxsim_batch*): the scorer between
// the encoder's device outputs, with no index and no handle.  Kernels: dense_kernels.hpp (fp32 embeddings, the oracle's bits),
// dense_half_kernels.hpp (fp16 / bf16 embeddings: clb_maxsim_batch_half*), dense_i8_kernels.hpp (int8 embeddings with one scale
// each: clb_maxsim_batch_i8*, clb_quantize_rows*).
#include <algorithm>
#include <cmath>

#include "dense_half_kernels.hpp"
#include "dense_i8_kernels.hpp"

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

// ---- int8 embeddings with one fp32 scale each (dense_i8_kernels.hpp) --------------------------------------------------------
int check_i8_dim(const char* who, int64_t dim) {
    if (dim % 16 != 0 || dim < 16 || dim > 1024)
        return fail(CLB_EUNSUPPORTED, "%s serves dim %% 16 == 0, 16 <= dim <= 1024 (dim = %lld)", who, (long long)dim);
    return CLB_OK;
}

int check_i8(int q_type, int64_t dim, int64_t T, int64_t B, int64_t n_D, int64_t N) {
    if (q_type != CLB_F32 && q_type != CLB_I8)
        return fail(CLB_EUNSUPPORTED, "maxsim_batch_i8 serves Q in fp32 or int8 (q_type = %d)", q_type);
    CLB_TRY(check_i8_dim("maxsim_batch_i8", dim));
    if (T < 1 || T > 128) return fail(CLB_EUNSUPPORTED, "maxsim_batch_i8 serves 1 <= T <= 128 (T = %lld)", (long long)T);
    if (B < 1 || N < 0 || n_D < 0) return fail(CLB_EARGUMENT, "maxsim_batch_i8: B >= 1, N >= 0 and n_D >= 0 are required");
    return CLB_OK;
}

// one finite scale >= 0 per embedding
int check_scales(const char* who, const char* what, const float* s, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(s[i]) || s[i] < 0.f)
            return fail(CLB_EARGUMENT, "%s: the scale of %s embedding %lld is %g: finite and >= 0 is required", who, what, (long long)i, (double)s[i]);
    return CLB_OK;
}

// plan_dense's G, QB and grid; waves of 64 rows, the int8 rows' and their scales' LDS footprint behind this kernel's own head
DensePlan plan_dense_i8(int dim, int T, int64_t B, int64_t N, bool owned) {
    DensePlan p = plan_dense(dim, T, B, N, owned);
    p.lds = kDenseI8HeadBytes + ((size_t)p.QB * p.G * (T | 1) * 4 + 15) / 16 * 16 + (size_t)16 * kDenseI8WaveTiles * p.nw * (dense_i8_row_stride(dim) + 4);
    return p;
}

void launch_quantize(const float* d_X, int dim, int64_t n, int8_t* d_X8, float* d_scale, hipStream_t st) {
    hipLaunchKernelGGL(dense_quantize_kernel, dim3((unsigned)std::min<int64_t>((n + 3) / 4, 8192)), dim3(256), 0, st, d_X, dim, n, d_X8, d_scale);
}

// Where the work buffer keeps a query quantised in the call: behind the offsets, values then scales.
struct I8Work {
    int64_t off_bytes, q_bytes, s_bytes;
    I8Work(int64_t N, int64_t B, int64_t T, int64_t dim) {
        const int64_t bt = std::max<int64_t>(B, 0) * std::max<int64_t>(T, 0);
        off_bytes = align256((int64_t)sizeof(int64_t) * (std::max<int64_t>(N, 0) + 1));
        q_bytes = align256(bt * std::max<int64_t>(dim, 0));
        s_bytes = align256(4 * bt);
    }
};

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

int clb_quantize_rows_device(int device, const float* d_X, int64_t dim, int64_t n, int8_t* d_X8, float* d_scale, void* hip_stream) {
    CLB_TRY(check_i8_dim("quantize_rows", dim));
    if (n < 0) return fail(CLB_EARGUMENT, "quantize_rows: n >= 0 is required");
    if (n == 0) return CLB_OK;
    if (!d_X || !d_X8 || !d_scale) return fail(CLB_EARGUMENT, "quantize_rows: null argument");
    if ((uintptr_t)d_X % 16 || (uintptr_t)d_X8 % 16) return fail(CLB_EARGUMENT, "quantize_rows: X and X8 must be 16-byte aligned");
    CLB_TRY(use_device(device));
    launch_quantize(d_X, (int)dim, n, d_X8, d_scale, (hipStream_t)hip_stream);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

int clb_quantize_rows(int device, const float* X, int64_t dim, int64_t n, int8_t* X8, float* scale) {
    CLB_TRY(check_i8_dim("quantize_rows", dim));
    if (n < 0 || (n > 0 && (!X || !X8 || !scale))) return fail(CLB_EARGUMENT, "quantize_rows: n >= 0 and non-null buffers are required");
    for (int64_t e = 0; e < n; ++e)
        for (int64_t k = 0; k < dim; ++k)
            if (!std::isfinite(X[e * dim + k])) return fail(CLB_EARGUMENT, "quantize_rows: embedding %lld holds a non-finite value", (long long)e);
    CLB_TRY(use_device(device));
    if (n == 0) return CLB_OK;
    hipStream_t st = nullptr;
    CLB_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    DevBuf dX, d8, dS;
    int rc = upload(dX, X, sizeof(float) * dim * n, st);
    if (!rc) rc = d8.alloc((size_t)dim * n);
    if (!rc) rc = dS.alloc(sizeof(float) * n);
    if (!rc) rc = clb_quantize_rows_device(device, dX.as<float>(), dim, n, d8.as<int8_t>(), dS.as<float>(), st);
    if (!rc && (hipMemcpyAsync(X8, d8.p, (size_t)dim * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipMemcpyAsync(scale, dS.p, sizeof(float) * n, hipMemcpyDeviceToHost, st) != hipSuccess))
        rc = fail(CLB_EHIP, "quantize_rows: copying the result back failed");
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(CLB_EHIP, "quantize_rows: hipStreamSynchronize failed");
    (void)hipStreamDestroy(st);
    return rc;
}

int64_t clb_maxsim_batch_i8_work_bytes(int64_t N, int64_t B, int64_t T, int64_t dim) {
    const I8Work w(N, B, T, dim);                       // the offsets; Q8 and its scales, when Q arrives in fp32
    return w.off_bytes + w.q_bytes + w.s_bytes;
}

int clb_maxsim_batch_i8_device(int device, const void* d_Q, int q_type, const float* d_qscale, int64_t dim, int64_t T, int64_t B,
                               const int8_t* d_D8, const float* d_dscale, int64_t n_D, const int64_t* d_doclens, int64_t N,
                               const int32_t* d_owner, float* d_scores, void* d_work, int64_t work_bytes, void* hip_stream) {
    CLB_TRY(check_i8(q_type, dim, T, B, n_D, N));
    if (N == 0) return CLB_OK;
    if (!d_Q || !d_doclens || !d_scores || !d_work || ((!d_D8 || !d_dscale) && n_D > 0) || (q_type == CLB_I8 && !d_qscale))
        return fail(CLB_EARGUMENT, "maxsim_batch_i8: null argument");
    if ((uintptr_t)d_D8 % 16 || (uintptr_t)d_Q % 16 || (uintptr_t)d_work % 16)
        return fail(CLB_EARGUMENT, "maxsim_batch_i8: Q, D8 and the work buffer must be 16-byte aligned");
    const I8Work wk(N, B, T, dim);
    if (work_bytes < wk.off_bytes + wk.q_bytes + wk.s_bytes)
        return fail(CLB_EARGUMENT, "maxsim_batch_i8: work buffer of %lld bytes, clb_maxsim_batch_i8_work_bytes asks for %lld",
                    (long long)work_bytes, (long long)(wk.off_bytes + wk.q_bytes + wk.s_bytes));
    const DensePlan p = plan_dense_i8((int)dim, (int)T, B, N, d_owner != nullptr);
    if (p.gy > 65535u || (N + p.G - 1) / p.G > 0x7fffffffLL)
        return fail(CLB_EUNSUPPORTED, "maxsim_batch_i8: B = %lld, N = %lld exceed one launch", (long long)B, (long long)N);
    CLB_TRY(use_device(device));
    hipStream_t st = (hipStream_t)hip_stream;
    int64_t* d_off = reinterpret_cast<int64_t*>(d_work);
    const int8_t* d_q8 = reinterpret_cast<const int8_t*>(d_Q);
    if (q_type == CLB_F32) {                                // Q8 and its scales behind the offsets in the work buffer
        int8_t* q8 = reinterpret_cast<int8_t*>(d_work) + wk.off_bytes;
        float* qs = reinterpret_cast<float*>(q8 + wk.q_bytes);
        launch_quantize(reinterpret_cast<const float*>(d_Q), (int)dim, B * T, q8, qs, st);
        d_q8 = q8;
        d_qscale = qs;
    }
    hipLaunchKernelGGL(dense_offsets_kernel, dim3(1), dim3(1024), 0, st, d_doclens, N, n_D, d_off);
    auto kern = dim == 128 ? dense_maxsim_i8_kernel<2, kDenseI8WaveTiles> : dense_maxsim_i8_kernel<0, kDenseI8WaveTiles>;
    if (p.lds > 64 * 1024) allow_dynamic_lds(reinterpret_cast<const void*>(kern), 160 * 1024);
    hipLaunchKernelGGL(kern, dim3(p.gx, p.gy), dim3(64 * p.nw), p.lds, st, d_q8, d_qscale, (int)dim, (int)T, (int)B, d_D8, d_dscale,
                       (const int64_t*)d_off, N, d_owner, p.G, p.QB, d_scores);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

int clb_maxsim_batch_i8(int device, const void* Q, int q_type, const float* qscale, int64_t dim, int64_t T, int64_t B,
                        const int8_t* D8, const float* dscale, int64_t n_D, const int64_t* doclens, int64_t N, const int32_t* owner,
                        float* scores) {
    CLB_TRY(check_i8(q_type, dim, T, B, n_D, N));
    if (N > 0 && (!doclens || !scores || !Q || (q_type == CLB_I8 && !qscale) || (n_D > 0 && (!D8 || !dscale))))
        return fail(CLB_EARGUMENT, "maxsim_batch_i8: null argument");
    if (N > 0 && q_type == CLB_I8) CLB_TRY(check_scales("maxsim_batch_i8", "query", qscale, B * T));
    if (N > 0) CLB_TRY(check_scales("maxsim_batch_i8", "passage", dscale, n_D));
    CLB_TRY(check_host_lists(doclens, N, n_D, owner, B));
    CLB_TRY(use_device(device));
    if (N == 0) return CLB_OK;
    hipStream_t st = nullptr;
    CLB_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const int64_t n_scores = owner ? N : N * B, wb = clb_maxsim_batch_i8_work_bytes(N, B, T, dim);
    DevBuf dQ, dQs, dD, dDs, dL, dO, dS, dW;
    int rc = upload(dQ, Q, (size_t)(q_type == CLB_F32 ? 4 : 1) * dim * T * B, st);
    if (!rc && q_type == CLB_I8) rc = upload(dQs, qscale, sizeof(float) * T * B, st);
    if (!rc) rc = upload(dD, D8, (size_t)dim * n_D, st);
    if (!rc) rc = upload(dDs, dscale, sizeof(float) * n_D, st);
    if (!rc) rc = upload(dL, doclens, sizeof(int64_t) * N, st);
    if (!rc && owner) rc = upload(dO, owner, sizeof(int32_t) * N, st);
    if (!rc) rc = dS.alloc(sizeof(float) * n_scores);
    if (!rc) rc = dW.alloc((size_t)wb);
    if (!rc)
        rc = clb_maxsim_batch_i8_device(device, dQ.p, q_type, dQs.as<float>(), dim, T, B, dD.as<int8_t>(), dDs.as<float>(), n_D,
                                        dL.as<int64_t>(), N, owner ? dO.as<int32_t>() : nullptr, dS.as<float>(), dW.p, wb, st);
    if (!rc && hipMemcpyAsync(scores, dS.p, sizeof(float) * n_scores, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = fail(CLB_EHIP, "maxsim_batch_i8: copying the scores back failed");
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(CLB_EHIP, "maxsim_batch_i8: hipStreamSynchronize failed");
    (void)hipStreamDestroy(st);
    return rc;
}

}  // extern "C"
