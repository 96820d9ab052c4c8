// dense_kernels.hpp -- MaxSim of un-indexed passages for a batch of queries (gfx950): fp32 embeddings in, fp32 scores out,
// bit-identical to the CPU oracle's maxsim (ranking.jl:69-86).
//   dot     v_mfma_f32_16x16x4_f32 with k walked in ascending order = the canonical d-ascending fmaf chain
//           (search_kernels.hpp, generic_kernels.hpp): embeddings are tile rows, query tokens are tile columns
//   max     exact and order-free, so partial maxima of a passage combine in any order (LDS atomic max on order keys)
//   sum     acc = 0; acc = acc + max_t for t ascending: one serial chain per (passage, query)
//
// Work split.  A work-group owns G consecutive PASSAGES (so its rows are consecutive and cut at passage boundaries) and, in
// the all-pairs form, a block of QB queries.  It walks its rows in steps of 16 rows per wave: a step is brought from global
// memory into LDS once with 16-byte loads (rows are contiguous, so the loads are dense), in rows padded to a stride = 4
// mod 64 floats so that the MFMA A-operand reads -- lane (r, g) reads dim 4 s + g of row r -- touch 64 different banks.  At
// dim 128 a wave then keeps its 16 rows as 32 VGPRs of A operand and re-uses them for every token tile of every query of
// the block; the B operand of a token tile (16 tokens x 128 dims) is 32 VGPRs read from the query block.  Other dims walk
// k at run time, the A operand read from LDS.
// Segmentation.  Every row of a step knows its passage (s_rowp; -1 past the end of the group).  A tile whose 16 rows lie in
// one passage reduces in registers (3 fmax, 2 shuffles) and issues one LDS atomic per token; a tile that straddles passages
// issues one per (row, token), to the row's own passage -- a neighbour's row never reaches a maximum.  In the owned form a
// wave multiplies a tile once per RUN of consecutive passages with the same owner.
// Long passages span several steps and several waves of their work-group: their partial maxima meet in the same LDS words.
// Safety.  The offsets are a clamped scan (negative doclen = 0, every offset <= n_D), so no row at or past n_D is read; an
// owner outside 0..B-1 multiplies nothing.  A (passage, query) that received no row keeps -Inf in every token and sums to -Inf.
#pragma once
#include "common.hpp"

namespace clb {

typedef float dense_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kDenseMaxGroup = 16;         // passages per work-group, at most
constexpr int kDensePmWords = 4096;        // LDS words of per-(query, passage, token) maxima per work-group
constexpr int kDenseHeadBytes = 1024;      // s_off (17 x 8) | s_rowp at 256 (<= 128 x 4) | s_own at 768 (16 x 4)

__host__ __device__ inline int dense_row_stride(int dim) { return dim + (68 - dim % 64) % 64; }   // = 4 mod 64

// offsets[j] = min(n_D, sum of max(0, min(doclens[i], n_D)) for i < j), j = 0..N.  One work-group; 4096 doclens per round.
static __global__ __launch_bounds__(1024) void dense_offsets_kernel(const int64_t* __restrict__ doclens, int64_t N, int64_t n_D,
                                                                    int64_t* __restrict__ off) {
    __shared__ int64_t wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < N; base += 4096) {
        int64_t v[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = base + 4 * tid + k;
            int64_t x = i < N ? doclens[i] : 0;
            x = x < 0 ? 0 : (x > n_D ? n_D : x);
            v[k] = x;
            s += x;
        }
        int64_t incl = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        int64_t before = 0, total = 0;
        for (int i = 0; i < 16; ++i) {
            const int64_t x = wsum[i];
            if (i < w) before += x;
            total += x;
        }
        int64_t run = carry + before + (incl - s);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = base + 4 * tid + k;
            if (i < N) off[i] = run < n_D ? run : n_D;
            run += v[k];
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) off[N] = carry < n_D ? carry : n_D;
}

// One 16 x 16 tile's maxima into the LDS words of the passages pa..pb (local numbers): pm[rowp * TP + t].
// Accumulator layout: lane (r = token column, g) holds the rows 4 g + i, i = 0..3.
__device__ __forceinline__ void dense_tile_max(const dense_f32x4 acc, const int* __restrict__ rowp16, int pa, int pb, bool tok_ok,
                                               uint32_t* __restrict__ pm, int TP, int tcol, int g) {
    const int p_first = rowp16[0], p_last = rowp16[15];
    if (p_first == p_last) {                       // (wave-uniform) the whole tile is one passage: p_first >= 0, no row is past the end
        if (p_first < pa || p_first > pb) return;
        float m = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3]));
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        if (g == 0 && tok_ok) atomicMax(&pm[p_first * TP + tcol], f32_order_key(m));
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = rowp16[4 * g + i];
        if (p >= pa && p <= pb && tok_ok) atomicMax(&pm[p * TP + tcol], f32_order_key(acc[i]));
    }
}

// The group's offsets and owners into the LDS head and every maximum to -Inf; the barrier after it is the caller's.
__device__ __forceinline__ void dense_group_begin(int64_t* __restrict__ s_off, int* __restrict__ s_own, uint32_t* __restrict__ s_pm,
                                                  const int64_t* __restrict__ off, const int32_t* __restrict__ owner, int64_t p0,
                                                  int np, int pm_words) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    for (int i = tid; i <= np; i += nthr) s_off[i] = off[p0 + i];
    for (int i = tid; i < np; i += nthr) s_own[i] = owner ? owner[p0 + i] : 0;
    const uint32_t key_ninf = f32_order_key(kNegInf);
    for (int i = tid; i < pm_words; i += nthr) s_pm[i] = key_ninf;
}

// The passage of every row of the step of CH rows that begins at row c: the last p with off[p] <= row; -1 past n_rows.
__device__ __forceinline__ void dense_step_passages(const int64_t* __restrict__ s_off, int* __restrict__ s_rowp, int64_t c, int n_rows,
                                                    int CH, int np) {
    for (int i = threadIdx.x; i < CH; i += blockDim.x) {
        int p = -1;
        if (i < n_rows) {
            const int64_t e = c + i;
            int a = 0, b = np;                          // s_off[a] <= e < s_off[b]
            while (b - a > 1) {
                const int m = (a + b) >> 1;
                if (s_off[m] <= e) a = m; else b = m;
            }
            p = a;
        }
        s_rowp[i] = p;
    }
}

// one ordered fp32 sum per (query, passage): acc = 0; acc = acc + max_t, t ascending (ranking.jl:83)
__device__ __forceinline__ void dense_sum_maxima(const uint32_t* __restrict__ s_pm, int nq, int np, int G, int TP, int T, bool owned,
                                                 int64_t p0, int q0, int64_t N, float* __restrict__ scores) {
    for (int i = threadIdx.x; i < nq * np; i += blockDim.x) {
        const int ql = i / np, p = i - ql * np;
        const uint32_t* pm = s_pm + (ql * G + p) * TP;
        float acc = 0.f;
        for (int t = 0; t < T; ++t) acc = acc + f32_from_order_key(pm[t]);
        scores[owned ? p0 + p : (int64_t)(q0 + ql) * N + p0 + p] = acc;
    }
}

// KS = dim / 4 when the A and B operands live in registers (dim 128: KS 32), 0 = any dim, k walked at run time.
// grid (ceil(N / G), owned ? 1 : ceil(B / QB)); block 64 * nw, nw waves of 16 rows each;
// dynamic LDS = kDenseHeadBytes + 4 * (owned ? 1 : QB) * G * (T | 1) rounded up to 16 + 4 * 16 nw * dense_row_stride(dim).
template <int KS>
static __global__ __launch_bounds__(256) void dense_maxsim_kernel(const float* __restrict__ Q, int dim, int T, int B,
                                                                  const float* __restrict__ D, const int64_t* __restrict__ off,
                                                                  int64_t N, const int32_t* __restrict__ owner, int G, int QB,
                                                                  float* __restrict__ scores) {
    extern __shared__ __align__(16) unsigned char dense_smem[];
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int CH = (nthr >> 6) * 16;                       // rows per step of the work-group
    const int stride = dense_row_stride(dim), TP = T | 1, ks = dim >> 2, dim4 = dim >> 2;
    const bool owned = owner != nullptr;
    const int64_t p0 = (int64_t)blockIdx.x * G;
    const int np = (int)(N - p0 < G ? N - p0 : G);
    const int q0 = owned ? 0 : (int)blockIdx.y * QB;
    const int nq = owned ? 1 : (B - q0 < QB ? B - q0 : QB);
    int64_t* s_off = reinterpret_cast<int64_t*>(dense_smem);
    int* s_rowp = reinterpret_cast<int*>(dense_smem + 256);
    int* s_own = reinterpret_cast<int*>(dense_smem + 768);
    uint32_t* s_pm = reinterpret_cast<uint32_t*>(dense_smem + kDenseHeadBytes);
    const int pm_words = (owned ? 1 : QB) * G * TP;
    float* s_d = reinterpret_cast<float*>(dense_smem + kDenseHeadBytes + ((size_t)pm_words * 4 + 15) / 16 * 16);

    dense_group_begin(s_off, s_own, s_pm, off, owner, p0, np, pm_words);
    __syncthreads();
    const int64_t lo = s_off[0], hi = s_off[np];

    for (int64_t c = lo; c < hi; c += CH) {
        const int n_rows = (int)(hi - c < CH ? hi - c : CH);
        // the step's rows, dense 16-byte loads (D + c * dim is 16-byte aligned: dim % 4 == 0), into padded LDS rows
        const float4* src = reinterpret_cast<const float4*>(D + c * dim);
        for (int i = tid; i < n_rows * dim4; i += nthr) {
            const int row = i / dim4, c4 = i - row * dim4;
            *reinterpret_cast<float4*>(s_d + row * stride + 4 * c4) = src[i];
        }
        dense_step_passages(s_off, s_rowp, c, n_rows, CH, np);
        __syncthreads();

        const int rb = 16 * w;                              // this wave's rows of the step
        if (rb < n_rows) {
            const int* rowp16 = s_rowp + rb;
            const float* arow = s_d + (rb + r) * stride + g;
            float a[KS > 0 ? KS : 1];
            if (KS > 0) {
#pragma unroll
                for (int s = 0; s < KS; ++s) a[s] = arow[4 * s];
            }
            const int last = (rb + 16 < n_rows ? rb + 16 : n_rows) - 1;
            const int pf = __builtin_amdgcn_readfirstlane(s_rowp[rb]), pl = __builtin_amdgcn_readfirstlane(s_rowp[last]);
            // runs of passages that one query scores: the whole span per query (all pairs), or the stretches of equal owner
            int pa = owned ? pf : 0, ql = 0;
            while (owned ? pa <= pl : ql < nq) {
                int pb, q;
                bool run_ok = true;
                if (owned) {
                    q = __builtin_amdgcn_readfirstlane(s_own[pa]);
                    pb = pa;
                    while (pb < pl && __builtin_amdgcn_readfirstlane(s_own[pb + 1]) == q) ++pb;
                    run_ok = q >= 0 && q < B;              // an owner outside the batch reads no query: its passages stay at -Inf
                } else {
                    q = q0 + ql;
                    pb = np - 1;
                }
                if (run_ok) {
                    uint32_t* pm = s_pm + (owned ? 0 : ql * G * TP);
                    for (int t0 = 0; t0 < T; t0 += 16) {
                        const int t = t0 + r;
                        const bool tok_ok = t < T;
                        const float* qrow = Q + ((size_t)q * T + (tok_ok ? t : T - 1)) * dim + g;   // B operand: lane (col r, k g)
                        dense_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                        if (KS > 0) {
                            float bq[KS > 0 ? KS : 1];
#pragma unroll
                            for (int s = 0; s < KS; ++s) bq[s] = qrow[4 * s];
#pragma unroll
                            for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], bq[s], acc, 0, 0, 0);
                        } else {
                            for (int s = 0; s < ks; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * s], qrow[4 * s], acc, 0, 0, 0);
                        }
                        dense_tile_max(acc, rowp16, pa, pb, tok_ok, pm, TP, t, g);
                    }
                }
                if (owned) pa = pb + 1; else ++ql;
            }
        }
        __syncthreads();                                    // the step's rows and passages are read; the next step overwrites them
    }

    dense_sum_maxima(s_pm, nq, np, G, TP, T, owned, p0, q0, N, scores);
}

}  // namespace clb
