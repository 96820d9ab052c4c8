// dense_half_kernels.hpp -- MaxSim of un-indexed passages on fp16 / bf16 embeddings (gfx950): 16-bit operands in, fp32 scores out.
//   dot     v_mfma_f32_16x16x32_f16 / _bf16: 32 exact products per instruction, summed in fp32 on the matrix pipe, the K-blocks
//           of 32 in ascending order from +0.  NOT the oracle's fmaf chain: the claim is a derived bound against float64
//           (DESIGN 4.2a), and that a pair's bits do not depend on where its rows fall: one row x one token is one column of
//           one accumulator entry through the same instructions, whatever else the tile holds.
//   max/sum as dense_kernels.hpp: exact order-free maxima on order keys in LDS, one ordered fp32 sum per (query, passage).
// Taken from dense_kernels.hpp as they are: dense_offsets_kernel, the LDS head (s_off | s_rowp | s_own) and the maxima behind
// it, dense_group_begin / dense_step_passages / dense_tile_max / dense_sum_maxima.  The 16 x 16 accumulator layout is the
// fp32 instruction's (lane (col r, g) holds rows 4 g + i), so segmentation, owners and the no-fault contract carry over.
//
// What is new.
// Q operand.  The kernel reads 16-bit queries only.  fp32 queries are rounded to nearest-even by dense_round_kernel into the
// caller's work buffer first (one launch, no allocation).  Lane (r, g) of a token tile's B operand holds k = 32 kb + 8 g .. + 7
// of token r: one 16-byte load per K-block, four at dim 128, against 32 dword loads in the fp32 kernel.
// Q residency.  At KB > 0 and T <= 32 the query's one or two token tiles (2 x KB x 4 = 32 VGPRs at dim 128) are loaded when a
// wave meets a query it does not hold and kept across owner runs, steps and -- in the all-pairs form, while the block holds
// one query -- the whole work-group; a block of several queries reloads per (step, query), 8 MFMAs behind 4 loads.  T > 32
// and KB = 0 read each token tile where it is used (not the tuned case).
// A operand and LDS.  A step's rows go global -> LDS once with 16-byte loads and LDS -> registers with ds_read_b128: lane
// (r, g) reads the 8 halves at byte 64 kb + 16 g of row r.  Row stride: 2 dim bytes padded so that stride / 16 is odd (dim
// 128: 272 bytes).  The 16 lanes of one g then read 16 different 16-byte columns of the 256 bytes the 64 banks span, so a
// group of 16 consecutive lanes -- what one pass of a 128-bit read serves -- is conflict-free (so is any 8 consecutive
// lanes; a pass that mixed lanes of different g would not be, and which lanes share a pass has not been measured).  The
// global -> LDS stores are consecutive 16-byte columns with one skipped per row: conflict-free as well.
// Rows per wave: 32.  A 16-row tile at dim 128 is 16 VGPRs of A, so a wave keeps two row tiles (32 VGPRs) and multiplies both
// by every B operand: 8 MFMAs per 4 B loads.  A 4-wave step is 128 rows = 34 KB of LDS at dim 128 (what 64 fp32 rows cost),
// beside the 1 KB head and at most 16 KB of maxima: three work-groups per CU in the all-pairs form as before, four in the
// owned form.  16 rows per wave has not been built or measured against it.  A row tile whose passages lie outside the run
// (owned form) is not multiplied.
// K tail.  dim % 8 == 0, so a lane's 8 halves lie wholly inside the row or wholly past it; past it both operands are zero
// registers (nothing is read), and zeros add exact zeros.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): KB = 4, fp16 and bf16 alike: 118 VGPRs, no AGPRs, no scratch,
// no spills, 4 waves per SIMD -- above the 3 (all pairs) or 4 (owned) work-groups of 4 waves per CU that the LDS allows, so
// registers do not lower the occupancy and 32 rows per wave stands.  KB = 0: 48 VGPRs, no spills.
// Safety: as dense_kernels.hpp -- clamped offsets (no row at or past n_D is read), an owner outside 0..B-1 multiplies nothing,
// a token column past T reads token T - 1 and reaches no maximum, rows past the step's end reach no maximum.
#pragma once
#include "dense_kernels.hpp"

namespace clb {

typedef uint32_t dense_u32x4 __attribute__((ext_vector_type(4)));   // 8 halves: one lane's share of a K-block of one operand

constexpr int kDenseHalfWaveRows = 32;

__host__ __device__ inline int dense_half_row_stride(int dim) { return dim % 16 == 0 ? dim + 8 : dim; }   // halves; stride / 8 odd

// The two 16-bit formats: the MFMA that multiplies them and the round-to-nearest-even from fp32 (NaN stays a quiet NaN).
struct DenseF16 {
    typedef _Float16 v8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ dense_f32x4 mfma(dense_u32x4 a, dense_u32x4 b, dense_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ uint32_t round(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }
};
struct DenseBF16 {
    typedef __bf16 v8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ dense_f32x4 mfma(dense_u32x4 a, dense_u32x4 b, dense_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ uint32_t round(float x) {
        const uint32_t u = __float_as_uint(x);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    }
};

// out[i] = round-to-nearest-even(in[i]) as H, 8 elements per thread and turn: n8 = n / 8, in and out 16-byte aligned.
template <typename H>
static __global__ __launch_bounds__(256) void dense_round_kernel(const float4* __restrict__ in, int64_t n8, dense_u32x4* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 x = in[2 * i], y = in[2 * i + 1];
        dense_u32x4 o;
        o[0] = H::round(x.x) | H::round(x.y) << 16;
        o[1] = H::round(x.z) | H::round(x.w) << 16;
        o[2] = H::round(y.x) | H::round(y.y) << 16;
        o[3] = H::round(y.z) | H::round(y.w) << 16;
        out[i] = o;
    }
}

// One token tile against a wave's one or two row tiles, KB K-blocks from registers, and its maxima.
template <typename H, int KB>
__device__ __forceinline__ void dense_half_tile(const dense_u32x4* a0, const dense_u32x4* a1, const dense_u32x4* b, bool do0, bool do1,
                                                const int* __restrict__ rowp, int pa, int pb, bool tok_ok, uint32_t* __restrict__ pm,
                                                int TP, int t, int g) {
    dense_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if (do0) {
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) acc0 = H::mfma(a0[kb], b[kb], acc0);
    }
    if (do1) {
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) acc1 = H::mfma(a1[kb], b[kb], acc1);
    }
    if (do0) dense_tile_max(acc0, rowp, pa, pb, tok_ok, pm, TP, t, g);
    if (do1) dense_tile_max(acc1, rowp + 16, pa, pb, tok_ok, pm, TP, t, g);
}

// H = DenseF16 / DenseBF16.  KB = dim / 32 K-blocks of both operands in registers (dim 128: KB 4); 0 = any dim, K walked at
// run time with the operands read where they lie.  Qh (dim, T, B) and D (dim, n_D) hold 16-bit elements, both 16-byte aligned.
// grid (ceil(N / G), owned ? 1 : ceil(B / QB)); block 64 * nw, nw waves of 32 rows each;
// dynamic LDS = kDenseHeadBytes + 4 * (owned ? 1 : QB) * G * (T | 1) rounded up to 16 + 2 * 32 nw * dense_half_row_stride(dim).
template <typename H, int KB>
static __global__ __launch_bounds__(256) void dense_maxsim_half_kernel(const uint16_t* __restrict__ Qh, int dim, int T, int B,
                                                                       const uint16_t* __restrict__ D, const int64_t* __restrict__ off,
                                                                       int64_t N, const int32_t* __restrict__ owner, int G, int QB,
                                                                       float* __restrict__ scores) {
    extern __shared__ __align__(16) unsigned char dense_smem[];
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int CH = (nthr >> 6) * kDenseHalfWaveRows;       // rows per step of the work-group
    const int stride = 2 * dense_half_row_stride(dim), TP = T | 1, dim8 = dim >> 3, nkb = (dim + 31) >> 5;   // stride in bytes
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
    unsigned char* s_d = dense_smem + kDenseHeadBytes + ((size_t)pm_words * 4 + 15) / 16 * 16;

    dense_group_begin(s_off, s_own, s_pm, off, owner, p0, np, pm_words);
    __syncthreads();
    const int64_t lo = s_off[0], hi = s_off[np];

    const dense_u32x4 zero = {0u, 0u, 0u, 0u};
    const bool resident = KB > 0 && T <= 32;
    dense_u32x4 bq[2][KB > 0 ? KB : 1];                    // the resident query's token tiles (resident only)
    int q_res = -1;                                        // (wave-uniform) the query they hold
    // lane (r, g)'s share of K-block kb of token t of query q, t clamped to the last token
    auto q_frag = [&](int q, int t, int kb) {
        return *reinterpret_cast<const dense_u32x4*>(Qh + ((size_t)q * T + (t < T ? t : T - 1)) * dim + 32 * kb + 8 * g);
    };

    for (int64_t c = lo; c < hi; c += CH) {
        const int n_rows = (int)(hi - c < CH ? hi - c : CH);
        // the step's rows, dense 16-byte loads (D + c * dim is 16-byte aligned: dim % 8 == 0), into padded LDS rows
        const dense_u32x4* src = reinterpret_cast<const dense_u32x4*>(D + c * dim);
        for (int i = tid; i < n_rows * dim8; i += nthr) {
            const int row = i / dim8, c8 = i - row * dim8;
            *reinterpret_cast<dense_u32x4*>(s_d + row * stride + 16 * c8) = src[i];
        }
        dense_step_passages(s_off, s_rowp, c, n_rows, CH, np);
        __syncthreads();

        const int rb = kDenseHalfWaveRows * w;              // this wave's rows of the step: the tiles rb .. + 15 and rb + 16 .. + 31
        if (rb < n_rows) {
            const bool two = rb + 16 < n_rows;
            const int* rowp = s_rowp + rb;
            const unsigned char* arow = s_d + (rb + r) * stride + 16 * g;
            dense_u32x4 a0[KB > 0 ? KB : 1], a1[KB > 0 ? KB : 1];
            if (KB > 0) {
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) {
                    a0[kb] = *reinterpret_cast<const dense_u32x4*>(arow + 64 * kb);
                    a1[kb] = two ? *reinterpret_cast<const dense_u32x4*>(arow + 16 * stride + 64 * kb) : zero;
                }
            }
            const int last = (rb + kDenseHalfWaveRows < n_rows ? rb + kDenseHalfWaveRows : n_rows) - 1;
            const int pf = __builtin_amdgcn_readfirstlane(s_rowp[rb]), pl = __builtin_amdgcn_readfirstlane(s_rowp[last]);
            const int pm0 = __builtin_amdgcn_readfirstlane(s_rowp[two ? rb + 15 : last]);    // the last passage of the first tile
            const int pf1 = __builtin_amdgcn_readfirstlane(s_rowp[two ? rb + 16 : last]);    // the first passage of the second
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
                    const bool do0 = pa <= pm0, do1 = two && pb >= pf1;      // (wave-uniform) the tile holds a row of the run
                    if (resident) {
                        if (q != q_res) {
#pragma unroll
                            for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                                for (int kb = 0; kb < KB; ++kb) bq[tt][kb] = 16 * tt < T ? q_frag(q, 16 * tt + r, kb) : zero;
                            }
                            q_res = q;
                        }
#pragma unroll
                        for (int tt = 0; tt < 2; ++tt)
                            if (16 * tt < T)
                                dense_half_tile<H, KB>(a0, a1, bq[tt], do0, do1, rowp, pa, pb, 16 * tt + r < T, pm, TP, 16 * tt + r, g);
                    } else if (KB > 0) {
                        for (int t0 = 0; t0 < T; t0 += 16) {
                            dense_u32x4 bt[KB > 0 ? KB : 1];
#pragma unroll
                            for (int kb = 0; kb < KB; ++kb) bt[kb] = q_frag(q, t0 + r, kb);
                            dense_half_tile<H, KB>(a0, a1, bt, do0, do1, rowp, pa, pb, t0 + r < T, pm, TP, t0 + r, g);
                        }
                    } else {
                        for (int t0 = 0; t0 < T; t0 += 16) {
                            dense_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                            for (int kb = 0; kb < nkb; ++kb) {
                                const bool k_ok = 32 * kb + 8 * g < dim;        // past the row: zeros, nothing read
                                const dense_u32x4 b = k_ok ? q_frag(q, t0 + r, kb) : zero;
                                if (do0) acc0 = H::mfma(k_ok ? *reinterpret_cast<const dense_u32x4*>(arow + 64 * kb) : zero, b, acc0);
                                if (do1) acc1 = H::mfma(k_ok ? *reinterpret_cast<const dense_u32x4*>(arow + 16 * stride + 64 * kb) : zero, b, acc1);
                            }
                            if (do0) dense_tile_max(acc0, rowp, pa, pb, t0 + r < T, pm, TP, t0 + r, g);
                            if (do1) dense_tile_max(acc1, rowp + 16, pa, pb, t0 + r < T, pm, TP, t0 + r, g);
                        }
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
