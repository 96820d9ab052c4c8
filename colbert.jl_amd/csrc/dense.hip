// dense.hip -- MaxSim of un-indexed passages for a query batch (include/colbert_hip.h: clb_maxsim_batch*): the scorer between
// the encoder's device outputs, with no index and no handle.  One kernel frame (dense_kernels.hpp) for seven embedding formats
// (dense_formats.hpp): fp32 (clb_maxsim_batch*, the oracle's bits), fp16 / bf16 (clb_maxsim_batch_half*), int8 with one scale
// each (clb_maxsim_batch_i8*, clb_quantize_rows*), MXFP8 / MXFP4 with one scale byte per block of 32 (clb_maxsim_batch_mx*,
// clb_quantize_mx*), one sign bit per dimension with one scale each against int8 queries (clb_maxsim_batch_b1*,
// clb_binarize_rows*); one device path and one host-array path behind the ten entry points, and the same device path behind
// clb_maxsim_store_device, which scores passages listed by id where they lie in a resident store (any of the seven formats).
#include <algorithm>
#include <cmath>

#include "dense_formats.hpp"

using namespace clb;

namespace {

inline int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

// What the host needs of a format F: its sizes, its LDS layout, its kernels.  One per type of D: CLB_F32 .. CLB_MXFP4, CLB_B1.
typedef void (*DenseKernel)(const void*, const void*, int, int, int, const void*, const void*, const int64_t*, int64_t, const int32_t*,
                            int, int, float*);
typedef void (*DenseStoreKernel)(const void*, const void*, int, int, int, const void*, const void*, const int64_t*, int64_t, const int32_t*,
                                 int, int, float*, DenseStore);
struct DenseFormat {
    int dim_multiple;                                   // dim is a multiple of one fragment's elements
    bool scaled, has_scales;                            // one fp32 scale per embedding (applied around the product); any scales at all
    int (*row_bytes)(int dim);                          // one embedding of D, of Q in D's family, and its scales
    int (*q_bytes)(int dim);
    int (*scale_bytes)(int dim);
    DenseLayout (*layout)(int dim, int T, int QB, int G, int nw, bool owned, bool listed);
    DenseKernel k128, kany;                             // both operands in registers at dim 128; any served dim
    DenseStoreKernel s128, sany;                        // the same two, passages listed by id in a resident store
};
template <typename F>
DenseFormat dense_format() {
    return {F::kDimMultiple, F::kScaled, F::kHasScales, F::row_bytes, F::q_bytes, F::scale_bytes, dense_layout<F>,
            dense_maxsim_kernel<F, 128 / F::kK>, dense_maxsim_kernel<F, 0>, dense_maxsim_kernel<F, 128 / F::kK, DenseStore>,
            dense_maxsim_kernel<F, 0, DenseStore>};
}
bool is_format(int d_type) { return (d_type >= CLB_F32 && d_type <= CLB_MXFP4) || d_type == CLB_B1; }
const DenseFormat& format_of(int d_type) {                // (d_type: is_format)
    static const DenseFormat f[7] = {dense_format<DenseF32>(), dense_format<DenseF16>(), dense_format<DenseBF16>(), dense_format<DenseI8>(),
                                     dense_format<DenseMXFP8>(), dense_format<DenseMXFP4>(), dense_format<DenseB1>()};
    return f[d_type == CLB_B1 ? 6 : d_type];
}

// One call, as every entry point states it.  Q and D are device arrays in run_dense_device, host arrays in run_dense_host.
struct DenseCall {
    const char* who;                                    // the name its messages carry: maxsim_batch, maxsim_batch_half, maxsim_batch_i8, _mx, _b1
    int family;                                         // the entry point's: CLB_F32, CLB_F16 (D in either 16-bit type), CLB_I8, CLB_MXFP8 (either MX), CLB_B1
    int q_type, d_type;
    const void* Q;
    const void* qscale;
    const void* D;
    const void* dscale;
    int64_t dim, T, B, n_D, N;
    const int64_t* doclens;
    const int32_t* owner;
    float* scores;
    void* work = nullptr;
    int64_t work_bytes = 0;
    hipStream_t st = nullptr;
    // a listed call (clb_maxsim_store_device): D / dscale / n_D are the store and its rows, doclens the store's offsets [P + 1],
    // pids [N] the entries to score
    bool listed = false;
    const int64_t* pids = nullptr;
    int64_t P = 0;
};

int check_dim(const char* who, int m, int64_t dim, const char* advice) {
    if (dim % m != 0 || dim < m || dim > 1024)
        return fail(CLB_EUNSUPPORTED, "%s serves dim %% %d == 0, %d <= dim <= 1024 (dim = %lld)%s", who, m, m, (long long)dim, advice);
    return CLB_OK;
}

int check_shape(const DenseCall& c) {
    const char* advice = c.family == CLB_F32 ? ": score one query at a time with clb_maxsim" : "";
    if (c.family == CLB_F32 && c.q_type != CLB_F32) return fail(CLB_EUNSUPPORTED, "%s serves fp32 D with Q in fp32 (q_type = %d)", c.who, c.q_type);
    if ((c.family == CLB_I8 || c.family == CLB_B1) && c.q_type != CLB_F32 && c.q_type != CLB_I8)
        return fail(CLB_EUNSUPPORTED, "%s serves Q in fp32 or int8 (q_type = %d)", c.who, c.q_type);
    if (c.family == CLB_F16 && ((c.d_type != CLB_F16 && c.d_type != CLB_BF16) || (c.q_type != CLB_F32 && c.q_type != c.d_type)))
        return fail(CLB_EUNSUPPORTED, "%s serves D in fp16 or bf16 and Q in fp32 or D's type (q_type = %d, d_type = %d)", c.who, c.q_type, c.d_type);
    if (c.family == CLB_MXFP8 && ((c.d_type != CLB_MXFP8 && c.d_type != CLB_MXFP4) || (c.q_type != CLB_F32 && c.q_type != CLB_MXFP8)))
        return fail(CLB_EUNSUPPORTED, "%s serves D in CLB_MXFP8 or CLB_MXFP4 and Q in fp32 or CLB_MXFP8 (q_type = %d, format = %d)", c.who, c.q_type, c.d_type);
    CLB_TRY(check_dim(c.who, format_of(c.d_type).dim_multiple, c.dim, advice));
    if (c.T < 1 || c.T > 128) return fail(CLB_EUNSUPPORTED, "%s serves 1 <= T <= 128 (T = %lld)%s", c.who, (long long)c.T, advice);
    if (c.B < 1 || c.N < 0 || c.n_D < 0) return fail(CLB_EARGUMENT, "%s: B >= 1, N >= 0 and n_D >= 0 are required", c.who);
    if (c.P < 0) return fail(CLB_EARGUMENT, "%s: P >= 0 is required", c.who);
    return CLB_OK;
}

// How a launch is cut: G passages and QB queries per work-group, nw waves, and the dynamic LDS that takes (dense_layout).
struct DensePlan {
    int G, QB, nw;
    unsigned gx, gy;
    size_t lds;
};
DensePlan plan_dense(const DenseFormat& f, int dim, int T, int64_t B, int64_t N, bool owned, bool listed) {
    DensePlan p;
    const int TP = T | 1;
    const int g_target = (int)std::min<int64_t>(kDenseMaxGroup, std::max<int64_t>(1, (N + 2047) / 2048));   // >= ~2048 work-groups first
    p.QB = owned ? 1 : (int)std::min<int64_t>(B, std::max(1, kDensePmWords / TP));
    p.G = std::max(1, std::min(g_target, kDensePmWords / (TP * p.QB)));
    p.nw = dim <= 512 ? 4 : 2;
    p.gx = (unsigned)((N + p.G - 1) / p.G);
    p.gy = owned ? 1u : (unsigned)((B + p.QB - 1) / p.QB);
    p.lds = f.layout(dim, T, p.QB, p.G, p.nw, owned, listed).total;
    return p;
}

// The work buffer: the clamped offsets (per-pair maxima never leave LDS); behind them, when Q arrives in fp32 and D does not
// hold fp32, Q in D's format and -- a scaled format -- its scales.  A listed call has no offsets of its own (the kernel derives
// them from the store's): its buffer is the converted Q alone, and 16 bytes at the least, so that it is never empty.
struct DenseWork {
    int64_t off_bytes, q_bytes, s_bytes;
    DenseWork(int d_type, int64_t N, int64_t B, int64_t T, int64_t dim, bool listed = false) {
        const DenseFormat& f = format_of(d_type);
        const int64_t bt = std::max<int64_t>(B, 0) * std::max<int64_t>(T, 0);
        off_bytes = listed ? 0 : align256((int64_t)sizeof(int64_t) * (std::max<int64_t>(N, 0) + 1));
        const int d = (int)std::min<int64_t>(std::max<int64_t>(dim, 0), 1 << 24);   // the formats size by int; a dim past 2^24 is unserved whatever this returns
        q_bytes = d_type == CLB_F32 ? 0 : align256(f.q_bytes(d) * bt);
        s_bytes = f.has_scales ? align256(f.scale_bytes(d) * bt) : 0;
    }
    int64_t total() const { return std::max<int64_t>(off_bytes + q_bytes + s_bytes, 16); }
};

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

// one finite scale >= 0 per embedding
int check_scales(const char* who, const char* what, const float* s, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(s[i]) || s[i] < 0.f)
            return fail(CLB_EARGUMENT, "%s: the scale of %s embedding %lld is %g: finite and >= 0 is required", who, what, (long long)i, (double)s[i]);
    return CLB_OK;
}

// X into the values and scales of `format`: CLB_I8, CLB_B1 (one fp32 scale per embedding), CLB_MXFP8 / CLB_MXFP4 (one byte per block)
void launch_quantize(int format, const float* d_X, int dim, int64_t n, void* d_V, void* d_scale, hipStream_t st) {
    const dim3 grid((unsigned)std::min<int64_t>((n + 3) / 4, 8192)), block(256);
    if (format == CLB_I8)
        hipLaunchKernelGGL(dense_quantize_kernel, grid, block, 0, st, d_X, dim, n, (int8_t*)d_V, (float*)d_scale);
    else if (format == CLB_B1)
        hipLaunchKernelGGL(dense_binarize_kernel, grid, block, 0, st, d_X, dim, n, (unsigned char*)d_V, (float*)d_scale);
    else
        hipLaunchKernelGGL(format == CLB_MXFP4 ? dense_quantize_mx_kernel<true> : dense_quantize_mx_kernel<false>, grid, block, 0, st, d_X, dim, n,
                           (unsigned char*)d_V, (unsigned char*)d_scale);
}


// Every device entry point: checks, the work buffer's slices, the offsets, Q into D's format if it arrived in fp32, the kernel.
int run_dense_device(int device, const DenseCall& c) {
    CLB_TRY(check_shape(c));
    const DenseFormat& f = format_of(c.d_type);
    const bool q_f32 = c.q_type == CLB_F32, fp32 = c.d_type == CLB_F32;
    if (c.N == 0) return CLB_OK;
    if (!c.Q || !c.doclens || (c.listed && !c.pids) || !c.scores || !c.work || ((!c.D || (f.has_scales && !c.dscale)) && c.n_D > 0) || (f.has_scales && !q_f32 && !c.qscale))
        return fail(CLB_EARGUMENT, "%s: null argument", c.who);
    if (fp32) {                                             // fp32 queries are read in dwords, the work buffer holds offsets only
        if ((uintptr_t)c.D % 16 || (uintptr_t)c.work % 8)
            return fail(CLB_EARGUMENT, "%s: D must be 16-byte aligned and the work buffer 8-byte aligned", c.who);
    } else if ((uintptr_t)c.D % 16 || (uintptr_t)c.Q % 16 || (uintptr_t)c.work % 16) {
        return fail(CLB_EARGUMENT, "%s: Q, %s and the work buffer must be 16-byte aligned", c.who, f.scaled ? "D8" : "D");
    } else if (f.has_scales && !f.scaled && f.scale_bytes((int)c.dim) % 4 == 0 && (uintptr_t)c.dscale % 4) {
        return fail(CLB_EARGUMENT, "%s: the passages' scale bytes must be 4-byte aligned when dim %% 128 == 0", c.who);
    }
    const DenseWork wk(c.d_type, c.N, c.B, c.T, c.dim, c.listed);
    if (c.work_bytes < wk.total())
        return fail(CLB_EARGUMENT, "%s: work buffer of %lld bytes, clb_%s_work_bytes asks for %lld", c.who, (long long)c.work_bytes, c.who,
                    (long long)wk.total());
    const int dim = (int)c.dim, T = (int)c.T;
    const DensePlan p = plan_dense(f, dim, T, c.B, c.N, c.owner != nullptr, c.listed);
    if (p.gy > 65535u || (c.N + p.G - 1) / p.G > 0x7fffffffLL)
        return fail(CLB_EUNSUPPORTED, "%s: B = %lld, N = %lld exceed one launch", c.who, (long long)c.B, (long long)c.N);
    CLB_TRY(use_device(device));
    int64_t* d_off = reinterpret_cast<int64_t*>(c.work);
    unsigned char* d_qf = reinterpret_cast<unsigned char*>(c.work) + wk.off_bytes;     // Q in D's family's query format, then its scales
    unsigned char* d_qs = d_qf + wk.q_bytes;
    const bool convert = q_f32 && !fp32;
    // The order of the two launches ahead of the kernel is each format's own, as captured graphs hold it: a format with scales
    // quantises Q before the offsets (an MX family's query is MXFP8 whatever D holds), a 16-bit format rounds it after them.
    if (convert && f.has_scales)
        launch_quantize(f.scaled ? CLB_I8 : CLB_MXFP8, reinterpret_cast<const float*>(c.Q), dim, c.B * c.T, d_qf, d_qs, c.st);
    if (!c.listed) hipLaunchKernelGGL(dense_offsets_kernel, dim3(1), dim3(1024), 0, c.st, c.doclens, c.N, c.n_D, d_off);
    if (convert && !f.has_scales) {                         // Q~ = Q rounded to nearest-even
        const int64_t n8 = c.B * c.T * c.dim / 8;
        hipLaunchKernelGGL(c.d_type == CLB_F16 ? dense_round_kernel<DenseF16> : dense_round_kernel<DenseBF16>,
                           dim3((unsigned)std::min<int64_t>((n8 + 255) / 256, 4096)), dim3(256), 0, c.st, (const float4*)c.Q, n8, (dense_u32x4*)d_qf);
    }
    const void* q = convert ? (const void*)d_qf : c.Q;
    const void* qs = convert && f.has_scales ? (const void*)d_qs : c.qscale;
    if (c.listed) {                                         // the store's own offsets: no scan, this is the call's only other launch
        const DenseStoreKernel kern = dim == 128 ? f.s128 : f.sany;
        if (p.lds > 64 * 1024) allow_dynamic_lds(reinterpret_cast<const void*>(kern), 160 * 1024);
        hipLaunchKernelGGL(kern, dim3(p.gx, p.gy), dim3(64 * p.nw), p.lds, c.st, q, qs, dim, T, (int)c.B, c.D, c.dscale, c.doclens, c.N, c.owner,
                           p.G, p.QB, c.scores, DenseStore{c.pids, c.P, c.n_D});
    } else {
        const DenseKernel kern = dim == 128 ? f.k128 : f.kany;
        if (p.lds > 64 * 1024) allow_dynamic_lds(reinterpret_cast<const void*>(kern), 160 * 1024);
        hipLaunchKernelGGL(kern, dim3(p.gx, p.gy), dim3(64 * p.nw), p.lds, c.st, q, qs, dim, T, (int)c.B, c.D, c.dscale, (const int64_t*)d_off, c.N,
                           c.owner, p.G, p.QB, c.scores);
    }
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

// Every host-array entry point: what a host call checks first, then upload, allocate, the device path, copy back, synchronise.
int run_dense_host(int device, const DenseCall& h) {
    CLB_TRY(check_shape(h));
    const DenseFormat& f = format_of(h.d_type);
    const bool q_f32 = h.q_type == CLB_F32;
    if (h.N > 0 && (!h.doclens || !h.scores || !h.Q || (f.has_scales && ((!q_f32 && !h.qscale) || (h.n_D > 0 && (!h.D || !h.dscale))))))
        return fail(CLB_EARGUMENT, "%s: null argument", h.who);
    if (f.scaled && h.N > 0 && !q_f32) CLB_TRY(check_scales(h.who, "query", (const float*)h.qscale, h.B * h.T));
    if (f.scaled && h.N > 0) CLB_TRY(check_scales(h.who, "passage", (const float*)h.dscale, h.n_D));
    CLB_TRY(check_host_lists(h.doclens, h.N, h.n_D, h.owner, h.B));
    CLB_TRY(use_device(device));
    if (h.N == 0) return CLB_OK;
    hipStream_t st = nullptr;
    CLB_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const int64_t n_scores = h.owner ? h.N : h.N * h.B, wb = DenseWork(h.d_type, h.N, h.B, h.T, h.dim).total();
    const bool qs_given = f.has_scales && !q_f32;
    const int dim = (int)h.dim;
    DevBuf dQ, dQs, dD, dDs, dL, dO, dS, dW;
    int rc = upload(dQ, h.Q, (size_t)(q_f32 ? 4 * dim : f.q_bytes(dim)) * h.T * h.B, st);
    if (!rc && qs_given) rc = upload(dQs, h.qscale, (size_t)f.scale_bytes(dim) * h.T * h.B, st);
    if (!rc) rc = upload(dD, h.D, (size_t)f.row_bytes(dim) * h.n_D, st);
    if (!rc && f.has_scales) rc = upload(dDs, h.dscale, (size_t)f.scale_bytes(dim) * h.n_D, st);
    if (!rc) rc = upload(dL, h.doclens, sizeof(int64_t) * h.N, st);
    if (!rc && h.owner) rc = upload(dO, h.owner, sizeof(int32_t) * h.N, st);
    if (!rc) rc = dS.alloc(sizeof(float) * n_scores);
    if (!rc) rc = dW.alloc((size_t)wb);
    if (!rc) {
        DenseCall c = h;
        c.Q = dQ.p, c.qscale = dQs.p, c.D = dD.p, c.dscale = dDs.p, c.doclens = dL.as<int64_t>();
        c.owner = h.owner ? dO.as<int32_t>() : nullptr, c.scores = dS.as<float>(), c.work = dW.p, c.work_bytes = wb, c.st = st;
        rc = run_dense_device(device, c);
    }
    if (!rc && hipMemcpyAsync(h.scores, dS.p, sizeof(float) * n_scores, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = fail(CLB_EHIP, "%s: copying the scores back failed", h.who);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(CLB_EHIP, "%s: hipStreamSynchronize failed", h.who);
    (void)hipStreamDestroy(st);
    return rc;
}

}  // namespace

extern "C" {

int64_t clb_maxsim_batch_work_bytes(int64_t N, int64_t B, int64_t T) { return DenseWork(CLB_F32, N, B, T, 0).total(); }

int64_t clb_maxsim_batch_half_work_bytes(int64_t N, int64_t B, int64_t T, int64_t dim) { return DenseWork(CLB_F16, N, B, T, dim).total(); }

int64_t clb_maxsim_batch_i8_work_bytes(int64_t N, int64_t B, int64_t T, int64_t dim) { return DenseWork(CLB_I8, N, B, T, dim).total(); }

int clb_maxsim_batch_device(int device, const float* d_Q, int64_t dim, int64_t T, int64_t B, const float* d_D, int64_t n_D,
                            const int64_t* d_doclens, int64_t N, const int32_t* d_owner, float* d_scores, void* d_work,
                            int64_t work_bytes, void* hip_stream) {
    return run_dense_device(device, {"maxsim_batch", CLB_F32, CLB_F32, CLB_F32, d_Q, nullptr, d_D, nullptr, dim, T, B, n_D, N, d_doclens, d_owner,
                                     d_scores, d_work, work_bytes, (hipStream_t)hip_stream});
}

int clb_maxsim_batch(int device, const float* Q, int64_t dim, int64_t T, int64_t B, const float* D, int64_t n_D,
                     const int64_t* doclens, int64_t N, const int32_t* owner, float* scores) {
    return run_dense_host(device, {"maxsim_batch", CLB_F32, CLB_F32, CLB_F32, Q, nullptr, D, nullptr, dim, T, B, n_D, N, doclens, owner, scores});
}

int clb_maxsim_batch_half_device(int device, const void* d_Q, int q_type, int64_t dim, int64_t T, int64_t B, const void* d_D,
                                 int d_type, int64_t n_D, const int64_t* d_doclens, int64_t N, const int32_t* d_owner,
                                 float* d_scores, void* d_work, int64_t work_bytes, void* hip_stream) {
    return run_dense_device(device, {"maxsim_batch_half", CLB_F16, q_type, d_type, d_Q, nullptr, d_D, nullptr, dim, T, B, n_D, N, d_doclens,
                                     d_owner, d_scores, d_work, work_bytes, (hipStream_t)hip_stream});
}

int clb_maxsim_batch_half(int device, const void* Q, int q_type, int64_t dim, int64_t T, int64_t B, const void* D, int d_type,
                          int64_t n_D, const int64_t* doclens, int64_t N, const int32_t* owner, float* scores) {
    return run_dense_host(device, {"maxsim_batch_half", CLB_F16, q_type, d_type, Q, nullptr, D, nullptr, dim, T, B, n_D, N, doclens, owner,
                                   scores});
}

int clb_maxsim_batch_i8_device(int device, const void* d_Q, int q_type, const float* d_qscale, int64_t dim, int64_t T, int64_t B,
                               const int8_t* d_D8, const float* d_dscale, int64_t n_D, const int64_t* d_doclens, int64_t N,
                               const int32_t* d_owner, float* d_scores, void* d_work, int64_t work_bytes, void* hip_stream) {
    return run_dense_device(device, {"maxsim_batch_i8", CLB_I8, q_type, CLB_I8, d_Q, d_qscale, d_D8, d_dscale, dim, T, B, n_D, N, d_doclens, d_owner,
                                     d_scores, d_work, work_bytes, (hipStream_t)hip_stream});
}

int clb_maxsim_batch_i8(int device, const void* Q, int q_type, const float* qscale, int64_t dim, int64_t T, int64_t B,
                        const int8_t* D8, const float* dscale, int64_t n_D, const int64_t* doclens, int64_t N, const int32_t* owner,
                        float* scores) {
    return run_dense_host(device, {"maxsim_batch_i8", CLB_I8, q_type, CLB_I8, Q, qscale, D8, dscale, dim, T, B, n_D, N, doclens, owner, scores});
}

int64_t clb_maxsim_batch_b1_work_bytes(int64_t N, int64_t B, int64_t T, int64_t dim) { return DenseWork(CLB_B1, N, B, T, dim).total(); }

int clb_maxsim_batch_b1_device(int device, const void* d_Q, int q_type, const float* d_qscale, int64_t dim, int64_t T, int64_t B,
                               const uint8_t* d_D1, const float* d_dscale, int64_t n_D, const int64_t* d_doclens, int64_t N,
                               const int32_t* d_owner, float* d_scores, void* d_work, int64_t work_bytes, void* hip_stream) {
    return run_dense_device(device, {"maxsim_batch_b1", CLB_B1, q_type, CLB_B1, d_Q, d_qscale, d_D1, d_dscale, dim, T, B, n_D, N, d_doclens, d_owner,
                                     d_scores, d_work, work_bytes, (hipStream_t)hip_stream});
}

int clb_maxsim_batch_b1(int device, const void* Q, int q_type, const float* qscale, int64_t dim, int64_t T, int64_t B,
                        const uint8_t* D1, const float* dscale, int64_t n_D, const int64_t* doclens, int64_t N, const int32_t* owner,
                        float* scores) {
    return run_dense_host(device, {"maxsim_batch_b1", CLB_B1, q_type, CLB_B1, Q, qscale, D1, dscale, dim, T, B, n_D, N, doclens, owner, scores});
}

// one size for both passage formats: what the work buffer holds beside the offsets is the QUERY, MXFP8 either way (DenseMX's
// q_bytes and scale_bytes do not depend on E2M1), so sizing by CLB_MXFP8 here equals run_dense_device's sizing by the passages' format
int64_t clb_maxsim_batch_mx_work_bytes(int64_t N, int64_t B, int64_t T, int64_t dim) { return DenseWork(CLB_MXFP8, N, B, T, dim).total(); }

int clb_maxsim_batch_mx_device(int device, const void* d_Q, int q_type, const uint8_t* d_qscale, int64_t dim, int64_t T, int64_t B,
                               const uint8_t* d_D, const uint8_t* d_dscale, int format, int64_t n_D, const int64_t* d_doclens, int64_t N,
                               const int32_t* d_owner, float* d_scores, void* d_work, int64_t work_bytes, void* hip_stream) {
    return run_dense_device(device, {"maxsim_batch_mx", CLB_MXFP8, q_type, format, d_Q, d_qscale, d_D, d_dscale, dim, T, B, n_D, N, d_doclens,
                                     d_owner, d_scores, d_work, work_bytes, (hipStream_t)hip_stream});
}

int clb_maxsim_batch_mx(int device, const void* Q, int q_type, const uint8_t* qscale, int64_t dim, int64_t T, int64_t B, const uint8_t* D,
                        const uint8_t* dscale, int format, int64_t n_D, const int64_t* doclens, int64_t N, const int32_t* owner,
                        float* scores) {
    return run_dense_host(device, {"maxsim_batch_mx", CLB_MXFP8, q_type, format, Q, qscale, D, dscale, dim, T, B, n_D, N, doclens, owner, scores});
}

// The listed call: one entry point for the seven formats, the family being what the contiguous call of d_type belongs to.
static int family_of(int d_type) { return d_type == CLB_BF16 ? CLB_F16 : d_type == CLB_MXFP4 ? CLB_MXFP8 : d_type; }

int64_t clb_maxsim_store_work_bytes(int64_t N, int64_t B, int64_t T, int64_t dim, int d_type) {
    return DenseWork(is_format(d_type) ? d_type : CLB_F32, N, B, T, dim, true).total();
}

int clb_maxsim_store_device(int device, const void* d_Q, int q_type, const void* d_qscale, int64_t dim, int64_t T, int64_t B,
                            const void* d_store, const void* d_store_scale, int d_type, int64_t n_rows, const int64_t* d_store_off,
                            int64_t P, const int64_t* d_pids, int64_t N, const int32_t* d_owner, float* d_scores, void* d_work,
                            int64_t work_bytes, void* hip_stream) {
    if (!is_format(d_type)) return fail(CLB_EUNSUPPORTED, "maxsim_store serves d_type CLB_F32 .. CLB_MXFP4 and CLB_B1 (d_type = %d)", d_type);
    DenseCall c{"maxsim_store", family_of(d_type), q_type, d_type, d_Q, d_qscale, d_store, d_store_scale, dim, T, B, n_rows, N, d_store_off,
                d_owner, d_scores, d_work, work_bytes, (hipStream_t)hip_stream};
    c.listed = true, c.pids = d_pids, c.P = P;
    return run_dense_device(device, c);
}

static int check_mx_format(int format) {
    if (format != CLB_MXFP8 && format != CLB_MXFP4) return fail(CLB_EUNSUPPORTED, "quantize_mx serves CLB_MXFP8 and CLB_MXFP4 (format = %d)", format);
    return CLB_OK;
}

int clb_quantize_mx_device(int device, const float* d_X, int64_t dim, int64_t n, int format, uint8_t* d_V, uint8_t* d_scale, void* hip_stream) {
    CLB_TRY(check_mx_format(format));
    CLB_TRY(check_dim("quantize_mx", 32, dim, ""));
    if (n < 0) return fail(CLB_EARGUMENT, "quantize_mx: n >= 0 is required");
    if (n == 0) return CLB_OK;
    if (!d_X || !d_V || !d_scale) return fail(CLB_EARGUMENT, "quantize_mx: null argument");
    if ((uintptr_t)d_X % 16 || (uintptr_t)d_V % 4) return fail(CLB_EARGUMENT, "quantize_mx: X must be 16-byte and the values 4-byte aligned");
    CLB_TRY(use_device(device));
    launch_quantize(format, d_X, (int)dim, n, d_V, d_scale, (hipStream_t)hip_stream);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

int clb_quantize_mx(int device, const float* X, int64_t dim, int64_t n, int format, uint8_t* V, uint8_t* scale) {
    CLB_TRY(check_mx_format(format));
    CLB_TRY(check_dim("quantize_mx", 32, dim, ""));
    if (n < 0 || (n > 0 && (!X || !V || !scale))) return fail(CLB_EARGUMENT, "quantize_mx: n >= 0 and non-null buffers are required");
    for (int64_t e = 0; e < n; ++e)
        for (int64_t k = 0; k < dim; ++k)
            if (!std::isfinite(X[e * dim + k])) return fail(CLB_EARGUMENT, "quantize_mx: embedding %lld holds a non-finite value", (long long)e);
    CLB_TRY(use_device(device));
    if (n == 0) return CLB_OK;
    const size_t v_bytes = (size_t)(format == CLB_MXFP4 ? dim / 2 : dim) * n, s_bytes = (size_t)(dim / 32) * n;
    hipStream_t st = nullptr;
    CLB_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    DevBuf dX, dV, dS;
    int rc = upload(dX, X, sizeof(float) * dim * n, st);
    if (!rc) rc = dV.alloc(v_bytes);
    if (!rc) rc = dS.alloc(s_bytes);
    if (!rc) rc = clb_quantize_mx_device(device, dX.as<float>(), dim, n, format, dV.as<uint8_t>(), dS.as<uint8_t>(), st);
    if (!rc && (hipMemcpyAsync(V, dV.p, v_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipMemcpyAsync(scale, dS.p, s_bytes, hipMemcpyDeviceToHost, st) != hipSuccess))
        rc = fail(CLB_EHIP, "quantize_mx: copying the result back failed");
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(CLB_EHIP, "quantize_mx: hipStreamSynchronize failed");
    (void)hipStreamDestroy(st);
    return rc;
}

int clb_binarize_rows_device(int device, const float* d_X, int64_t dim, int64_t n, uint8_t* d_V, float* d_scale, void* hip_stream) {
    CLB_TRY(check_dim("binarize_rows", 128, dim, ""));
    if (n < 0) return fail(CLB_EARGUMENT, "binarize_rows: n >= 0 is required");
    if (n == 0) return CLB_OK;
    if (!d_X || !d_V || !d_scale) return fail(CLB_EARGUMENT, "binarize_rows: null argument");
    if ((uintptr_t)d_X % 16 || (uintptr_t)d_V % 16) return fail(CLB_EARGUMENT, "binarize_rows: X and the bits must be 16-byte aligned");
    CLB_TRY(use_device(device));
    launch_quantize(CLB_B1, d_X, (int)dim, n, d_V, d_scale, (hipStream_t)hip_stream);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

int clb_binarize_rows(int device, const float* X, int64_t dim, int64_t n, uint8_t* V, float* scale) {
    CLB_TRY(check_dim("binarize_rows", 128, dim, ""));
    if (n < 0 || (n > 0 && (!X || !V || !scale))) return fail(CLB_EARGUMENT, "binarize_rows: n >= 0 and non-null buffers are required");
    for (int64_t e = 0; e < n; ++e)
        for (int64_t k = 0; k < dim; ++k)
            if (!std::isfinite(X[e * dim + k])) return fail(CLB_EARGUMENT, "binarize_rows: embedding %lld holds a non-finite value", (long long)e);
    CLB_TRY(use_device(device));
    if (n == 0) return CLB_OK;
    const size_t v_bytes = (size_t)(dim / 8) * n;
    hipStream_t st = nullptr;
    CLB_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    DevBuf dX, dV, dS;
    int rc = upload(dX, X, sizeof(float) * dim * n, st);
    if (!rc) rc = dV.alloc(v_bytes);
    if (!rc) rc = dS.alloc(sizeof(float) * n);
    if (!rc) rc = clb_binarize_rows_device(device, dX.as<float>(), dim, n, dV.as<uint8_t>(), dS.as<float>(), st);
    if (!rc && (hipMemcpyAsync(V, dV.p, v_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipMemcpyAsync(scale, dS.p, sizeof(float) * n, hipMemcpyDeviceToHost, st) != hipSuccess))
        rc = fail(CLB_EHIP, "binarize_rows: copying the result back failed");
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(CLB_EHIP, "binarize_rows: hipStreamSynchronize failed");
    (void)hipStreamDestroy(st);
    return rc;
}

int clb_quantize_rows_device(int device, const float* d_X, int64_t dim, int64_t n, int8_t* d_X8, float* d_scale, void* hip_stream) {
    CLB_TRY(check_dim("quantize_rows", 16, dim, ""));
    if (n < 0) return fail(CLB_EARGUMENT, "quantize_rows: n >= 0 is required");
    if (n == 0) return CLB_OK;
    if (!d_X || !d_X8 || !d_scale) return fail(CLB_EARGUMENT, "quantize_rows: null argument");
    if ((uintptr_t)d_X % 16 || (uintptr_t)d_X8 % 16) return fail(CLB_EARGUMENT, "quantize_rows: X and X8 must be 16-byte aligned");
    CLB_TRY(use_device(device));
    launch_quantize(CLB_I8, d_X, (int)dim, n, d_X8, d_scale, (hipStream_t)hip_stream);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

int clb_quantize_rows(int device, const float* X, int64_t dim, int64_t n, int8_t* X8, float* scale) {
    CLB_TRY(check_dim("quantize_rows", 16, dim, ""));
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

}  // extern "C"
