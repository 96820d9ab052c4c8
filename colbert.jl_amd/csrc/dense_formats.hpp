// dense_formats.hpp -- the embedding formats of the dense MaxSim kernel (dense_kernels.hpp: dense_maxsim_kernel<F, KB>) and the
// kernels that bring fp32 queries into a format (dense_round_kernel, dense_quantize_kernel).  A format F supplies
//   kElem, Frag       bytes per element; one lane's share of a K-block of one operand (K = kK = 4 sizeof(Frag) / kElem elements)
//   kRowTiles         16-row tiles a wave keeps and multiplies by every B operand
//   kResident         whether a query of T <= 32 stays in registers (dense_kernels.hpp)
//   kScaled           one fp32 scale per embedding: row scales staged in LDS per step, query scales applied in the sum
//   kHeadBytes, kOwnAt, kRowpAt   the LDS head: s_off (17 x 8) at 0, s_own (16 x 4), s_rowp (one int per row of a 4-wave step)
//   row_stride(dim)   bytes from one LDS row to the next
//   Acc, mfma         the accumulator and the instruction; epilogue(acc, ds): the accumulator as fp32, ds = its four rows' scales
//
// fp32 (DenseF32): v_mfma_f32_16x16x4_f32 with k walked in ascending order = the canonical d-ascending fmaf chain
// (search_kernels.hpp, generic_kernels.hpp), so every score has the bits of the CPU oracle's maxsim (ranking.jl:69-86).  Lane
// (r, g) reads dim 4 s + g of row r: one float per K-block, 32 K-blocks at dim 128.  Rows padded to a stride = 4 mod 64 floats
// so that these reads touch 64 different banks.  At dim 128 a wave keeps its 16 rows as 32 VGPRs of A operand; the B operand of a
// token tile is 32 VGPRs more, read per (run, token tile) with dword loads (Q need only be 4-byte aligned): a resident query
// would be 64, so there is none.  Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; profiles/dense_refactor.md has
// every instantiation): KB = 32: 66 VGPRs, no AGPRs, no scratch, no spills, 7 waves per SIMD -- above the 3 (all pairs) or 4
// (owned) work-groups of 4 waves per CU that the LDS allows.  KB = 0: 29 VGPRs.
//
// fp16 / bf16 (DenseF16, DenseBF16): v_mfma_f32_16x16x32_f16 / _bf16: 32 exact products per instruction, summed in fp32 on the
// matrix pipe.  NOT the oracle's fmaf chain: the claim is a derived bound against float64, and that a pair's
// bits do not depend on where its rows fall: one row x one token is one column of one accumulator entry through the same
// instructions, whatever else the tile holds.  The kernel reads 16-bit queries only; fp32 queries are rounded to nearest-even
// by dense_round_kernel into the caller's work buffer first (one launch, no allocation).  Lane (r, g) holds the 8 halves at
// byte 64 kb + 16 g: one 16-byte global load (Q) or ds_read_b128 (D) per K-block, four at dim 128.  Row stride (Dense16ByteFrag):
// the row's bytes padded so that stride / 16 is odd (dim 128: 272 bytes).  The 16 lanes of one g then read 16 different
// 16-byte columns of the 256 bytes the 64 banks span, so a group of 16 consecutive lanes -- what one pass of a 128-bit read
// serves -- is conflict-free (so is any 8 consecutive lanes; a pass that mixed lanes of different g would not be, and which
// lanes share a pass has not been measured).  The global -> LDS stores are consecutive 16-byte columns with one skipped per
// row: conflict-free as well.  Rows per wave: 32.  A 16-row tile at dim 128 is 16 VGPRs of A, so a wave keeps two row tiles
// (32 VGPRs) beside the resident query's two token tiles (32 VGPRs) and multiplies both by every B operand: 8 MFMAs per 4 B
// loads.  A 4-wave step is 128 rows = 34 KB of LDS at dim 128 (what 64 fp32 rows cost), beside the 1 KB head and at most 16 KB
// of maxima: three work-groups per CU in the all-pairs form, four in the owned form.  16 rows per wave has not been built or
// measured against it.  Registers at KB = 4, fp16 and bf16 alike: 108 VGPRs, no AGPRs, no scratch, no VGPR spills, 5 SGPRs parked
// in lanes of a VGPR (no memory traffic), 4 waves per SIMD -- above the 3 or 4 work-groups of 4 waves per CU that the LDS
// allows, so registers do not lower the occupancy and 32 rows per wave stands.  KB = 0: 40 VGPRs, no spills.
//
// int8 with one fp32 scale per embedding (DenseI8): v_mfma_i32_16x16x64_i8: 64 exact products per instruction, summed in
// int32.  Integer addition is exact and order-free and |i| <= 1024 * 128 * 128 = 2^24, so float(i) is exact as well; every
// score is bit-identical to a plain restatement: m_t = max over the passage's rows of fl32(ds[r] * float(i)),
// one multiply per accumulator entry (the epilogue), and acc = fl32(acc + fl32(qs[t] * m_t)).  The QUERY scale waits until
// after the maximum: qs[t] >= 0 and fp32 multiplication is monotone, so it selects the same row, and it costs one multiply
// per token instead of one per entry.  Lane (r, g) holds the 16 bytes at 64 kb + 16 g.  At dim 128 a 16-row tile is 2 K-blocks
// = 8 VGPRs, so a wave keeps 4 row tiles (64 rows, 32 VGPRs) beside the resident query's two token tiles (16 VGPRs) and
// issues 2 MFMAs per (row tile, token tile).  A step of 4 waves x 64 rows needs 256 row-to-passage entries, twice what the
// other formats' 1 KB head reserves, so this format's head is 1280 bytes.  The step's row scales (4 B per row) lie behind
// the rows, and lane (r, g) reads the four scales of the rows 4 g .. 4 g + 3 of a tile -- its accumulator entries' rows -- in
// one 16-byte read.  A 4-wave step at dim 128: 256 rows x 144 B + 1 KB of scales = 37 KB, what the 16-bit format's 128 rows
// cost.  With two MFMAs per tile the epilogue (v_cvt_f32_i32 and a multiply on four entries), not the matrix pipe, is the
// likely limit of the all-pairs form (read from the code, not profiled; profiles/maxsim_batch_int8.md has the times).
// Registers at KB = 2: 106 VGPRs, no AGPRs, no scratch, no VGPR spills, 4 waves per SIMD -- the 3 (all pairs) or 4 (owned)
// work-groups of 4 waves per CU that the LDS allows, so registers do not lower the occupancy.  The scalar side is full: 25
// SGPRs (loop-invariant pointers and saved exec masks) are parked in lanes of one VGPR (v_writelane in the prologue,
// v_readlane where used) -- SGPR spills in the report, no memory traffic; they have not been removed.  2 row tiles per wave
// (half the step's LDS, so more work-groups per CU in the owned form) has not been measured against 4.  KB = 0: 69 VGPRs, 11
// SGPRs in lanes.  In the register path (KB > 0) the frame finishes a row tile -- chain, epilogue, maxima -- before it starts
// the next: all chains first costs this format 16 more VGPRs and measured 2 % (owned) to 5 % (all pairs) slower
// (profiles/dense_refactor.md).
#pragma once
#include "dense_kernels.hpp"

namespace clb {

typedef uint32_t dense_u32x4 __attribute__((ext_vector_type(4)));   // 8 halves: one lane's share of a K-block of one operand
typedef int dense_i32x4 __attribute__((ext_vector_type(4)));        // 16 int8: one lane's share of a K-block; or one accumulator

struct DenseF32 {
    typedef float Frag;
    typedef dense_f32x4 Acc;
    static constexpr int kElem = 4, kK = 4, kRowTiles = 1, kHeadBytes = 1024, kOwnAt = 768, kRowpAt = 256;
    static constexpr bool kResident = false, kScaled = false;
    __host__ __device__ static int row_stride(int dim) { return 4 * (dim + (68 - dim % 64) % 64); }   // = 4 mod 64 floats
    static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ dense_f32x4 epilogue(Acc acc, float4) { return acc; }
};

// What the formats with 16-byte fragments share: a resident query, and rows padded so that stride / 16 is odd.
struct Dense16ByteFrag {
    static constexpr bool kResident = true;
    __host__ __device__ static int padded(int row_bytes) { return row_bytes % 32 == 0 ? row_bytes + 16 : row_bytes; }
};

// The two 16-bit formats: the MFMA that multiplies them and the round-to-nearest-even from fp32 (NaN stays a quiet NaN).
struct Dense16Bit : Dense16ByteFrag {
    typedef dense_u32x4 Frag;
    typedef dense_f32x4 Acc;
    static constexpr int kElem = 2, kK = 32, kRowTiles = 2, kHeadBytes = 1024, kOwnAt = 768, kRowpAt = 256;
    static constexpr bool kScaled = false;
    __host__ __device__ static int row_stride(int dim) { return padded(2 * dim); }
    static __device__ __forceinline__ dense_f32x4 epilogue(Acc acc, float4) { return acc; }
};
struct DenseF16 : Dense16Bit {
    typedef _Float16 v8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ dense_f32x4 mfma(dense_u32x4 a, dense_u32x4 b, dense_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ uint32_t round(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }
};
struct DenseBF16 : Dense16Bit {
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

struct DenseI8 : Dense16ByteFrag {
    typedef dense_i32x4 Frag;
    typedef dense_i32x4 Acc;
    static constexpr int kElem = 1, kK = 64, kRowTiles = 4, kHeadBytes = 1280, kOwnAt = 192, kRowpAt = 256;
    static constexpr bool kScaled = true;
    __host__ __device__ static int row_stride(int dim) { return padded(dim); }
    static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
    // the int32 sums to fp32 (exact), each times its row's scale
    static __device__ __forceinline__ dense_f32x4 epilogue(Acc acc, float4 ds) {
        return dense_f32x4{ds.x * (float)acc[0], ds.y * (float)acc[1], ds.z * (float)acc[2], ds.w * (float)acc[3]};
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

// X (dim, n) fp32 -> X8 (dim, n) int8 and scale [n]: s = fl32(amax / 127), q_k = clamp(rint(fl32(x_k / s)), -127, 127); s == 0
// gives zeros.  One wave per embedding, grid-stride; the row (dim <= 1024, dim % 16 == 0) is read once with float4 loads into
// at most 4 registers per lane and written as packed dwords; no LDS.  A non-finite input gives defined, meaningless numbers
// (v_max_f32 drops a NaN, the clamp bounds whatever the division gives).  X and X8 16-byte aligned.
static __global__ __launch_bounds__(256) void dense_quantize_kernel(const float* __restrict__ X, int dim, int64_t n,
                                                                    int8_t* __restrict__ X8, float* __restrict__ scale) {
    const int lane = threadIdx.x & 63, dim4 = dim >> 2;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t e = wave; e < n; e += n_waves) {
        const float4* src = reinterpret_cast<const float4*>(X + e * dim);
        float4 v[4];
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            v[j] = c < dim4 ? src[c] : make_float4(0.f, 0.f, 0.f, 0.f);
            amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v[j].x), fabsf(v[j].y)), fmaxf(fabsf(v[j].z), fabsf(v[j].w))));
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) amax = fmaxf(amax, __shfl_xor(amax, d, 64));
        const float s = amax / 127.f;
        uint32_t* dst = reinterpret_cast<uint32_t*>(X8 + e * dim);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            if (c >= dim4) continue;
            const float x[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            uint32_t word = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int qi = s == 0.f ? 0 : (int)fminf(fmaxf(rintf(x[i] / s), -127.f), 127.f);
                word |= (uint32_t)(qi & 0xff) << (8 * i);
            }
            dst[c] = word;
        }
        if (lane == 0) scale[e] = s;
    }
}

}  // namespace clb
