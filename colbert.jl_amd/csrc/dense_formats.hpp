// dense_formats.hpp -- the embedding formats of the dense MaxSim kernel (dense_kernels.hpp: dense_maxsim_kernel<F, KB>) and the
// kernels that bring fp32 embeddings into a format (dense_round_kernel, dense_quantize_kernel, dense_quantize_mx_kernel,
// dense_binarize_kernel).  A format
// F supplies
//   Frag, QFrag       one lane's share of a K-block (kK elements) of a row and of a query token: kFragBytes / kQFragBytes of values
//   load_row, load_q  lane group g's fragment of a K-block, given the lane's first byte of it (the K-block's + kLaneBytes g), the
//                     lane's scale byte and the bytes the row still holds from the K-block's start
//   row_bytes(dim), q_bytes(dim), scale_bytes(dim), kDimMultiple   one embedding of D, of Q, its scales; what dim is a multiple of
//   kRowTiles         16-row tiles a wave keeps and multiplies by every B operand
//   kResident         whether a query of T <= 32 stays in registers (dense_kernels.hpp)
//   kScaled           one fp32 scale per embedding: row scales staged in LDS per step, query scales applied in the sum
//   kHasScales        any scales at all (kScaled, or block scales inside the fragments): staged behind the step's rows
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
//
// 1-bit sign rows against int8 queries (DenseB1): one bit per dimension and one fp32 scale per row, 16 + 4 B at dim 128.  gfx950
// has no 1-bit matrix instruction, and needs none: a sign is +-1 and +-1 is an int8, so the row is widened in registers and
// everything from the MFMA on -- v_mfma_i32_16x16x64_i8, the epilogue, the scales, the query side, the bit-exact restatement --
// is DenseI8's (|i| <= 1024 * 127 < 2^24).  Only load_row is new: lane (r, g) reads the 16 bits at k = 64 kb + 16 g of its row
// (kFragBytes = kLaneBytes = 2 stored bytes; Frag is the widened 16 int8).
// The widening, chosen from the instruction count: 14 VALU per 16 bits, counted in the ISA -- v_not and v_lshl once (so that
// every nibble is the high nibble of some byte), then per dword v_perm (replicate that byte), v_and 0x80402010 (byte j keeps its
// own bit) and v_perm again, which reads the four bytes as SELECTORS into a constant: 0 selects 0x01, a selector >= 0x0d is the
// constant 0xff, so a set bit becomes +1 and a clear one -1 with no arithmetic on the bytes at all.  Against it: bfe, multiply by
// 0x00204081, mask, then 0 / 1 -> -1 / +1 is 16 to 20; feeding bytes 0 / 2 and seeding the accumulator with -sum_k q8[k, t]
// saves the last step (12) but needs the sum per token tile -- two more MFMAs per (run, token tile) wherever the query is not
// resident -- and a seed hook in the frame for 2 instructions per 16 bits; a nibble table in LDS is two dependent LDS reads per
// 16 bits with random bank conflicts.  The widening runs once per row tile and step at dim 128 (KB = 2: 8 x 14 = 112 VALU per wave
// and step, the A operand then resident for every token tile of every query), per K-block at other dims.
// LDS: rows at padded(dim / 8) bytes -- 16 at dim 128, 48 at dim 256 and 384.  The 64 lanes of a read take 2 bytes each at
// 16 r + 8 kb + 2 g: at dim 128 the 16 rows of a tile are 256 contiguous bytes, one per bank group of 4, and the lanes g = 0, 1
// (2, 3) of a row share a dword, which is a broadcast: 32 dwords in 32 banks, conflict-free.  At a 48-byte stride row r starts
// at bank 12 r mod 64, sixteen different multiples of 4: conflict-free as well (an unpadded 32 bytes would put rows r and r + 8
// on the same bank).  A 4-wave step at dim 128 is 256 rows x 16 B = 4 KB + 1 KB of scales, against int8's 37 KB; with the 1280-byte
// head and at most 16 KB of maxima a work-group needs 8.3 KB (owned, T = 32) to 22.3 KB, so the LDS allows 19 (owned) to 7 (all
// pairs) work-groups per CU -- and registers, not LDS, now set the occupancy: 106 VGPRs = 4 waves per SIMD = 4 work-groups of 4
// waves per CU, where int8 had 3 or 4 from its LDS.  4 row tiles per wave stands: it is the most the frame's packed first / last
// passage scalars hold, the A operand is int8's 32 VGPRs, and fewer tiles would not raise the occupancy the registers set.
// Decided from the code, not timed: the bank picture, 4 tiles against 2, and the widening routes against each other.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / SGPRs in VGPR lanes / waves per SIMD; no AGPRs, no
// scratch, no VGPR spills): KB = 2: 106 / 27 / 4, KB = 0: 74 / 11 / 6; listed KB = 2: 105 / 27 / 4, KB = 0: 73 / 13 / 6.  Every
// other instantiation's figures are what they were.  Measured (profiles/maxsim_batch_b1.md): 1.8x int8 in the owned form, 1.3x in
// all pairs, and 2 % / 9 % SLOWER than MXFP4 at a third of its bytes -- at 9 % of the read rate the owned form is bound by issue
// slots, not bytes: two MFMAs, four v_cvt_f32_i32 and four multiplies per tile where MXFP4 has one MFMA and no epilogue.
// Quantiser (dense_binarize_kernel): a float4 is a nibble, 8 lanes' nibbles are OR-ed into a dword with 3 shuffles; no LDS.
//
// MX block-scaled (DenseMX<E2M1>: MXFP8 / MXFP4 passages, MXFP8 queries): v_mfma_scale_f32_16x16x128_f8f6f4 multiplies 128
// elements and applies one E8M0 scale per block of 32 of each operand inside the product, so there is no epilogue multiply and
// no query scale in the sum; A (rows, cbsz) and B (tokens, blgp) formats are independent.  At dim 128 a (row tile, token tile)
// is ONE MFMA.  Layout, pinned by the exact test (tests/test_gpu_maxsim_batch_mx.py; a first build that gave every lane 32
// consecutive E4M3 elements scored half of each block under another block's scale): an 8-bit operand is two halves of 64 --
// lane (r, g) holds k = 16 g .. 16 g + 15 in registers 0-3 and k = 64 + 16 g .. in registers 4-7, two 16-byte reads 64 bytes
// apart --, a 4-bit operand is k = 32 g .. 32 g + 31 in registers 0-3, one 16-byte read; block b's scale is the byte lane group
// b supplies, so lane (r, g) reads scale byte g of its row whatever values it holds.  A piece past the row's end is zero
// registers, a scale past it byte 127, neither read: dim % 32 == 0 suffices.  Rows per wave: 64 for both formats.  At dim 128
// an MXFP8 row tile is 8 VGPRs + 1 scale, an MXFP4 one 4 + 1; the resident query 16 + 2.  128 rows per wave was the other
// candidate for MXFP4 (8 tiles = 40 VGPRs): not built -- the frame packs a wave's first and last passage per tile into one
// 32-bit scalar each (4 tiles), the step's row-to-passage table would double, and 64 rows keep the owned step at 20 KB of LDS
// (256 rows x 80 B) + 1 KB of scales, so LDS allows 7 work-groups per CU where 40 KB would allow 3.  MXFP8: 256 x 144 B + 1 KB =
// 37 KB, the int8 figures.  LDS rows at an odd number of 16-byte columns (144 / 80 B at dim 128), dim / 32 scale bytes per row
// behind them (one dword per row at dim 128, staged in dwords; in bytes at other dims), where int8 keeps its fp32 scales.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage): MXFP8 KB = 1: 102 VGPRs, 4 waves per SIMD; KB = 0: 84, 5.  MXFP4
// KB = 1: 87 VGPRs, 5 waves; KB = 0: 81, 5.  No AGPRs, no scratch, no VGPR spills; 53 (KB = 1) / 30 scalar values parked in
// VGPR lanes, as for int8, not removed.  With one MFMA per tile, the tile's maximum (3 fmax, 2 shuffles, one LDS atomic per
// token) is what the all-pairs form spends its issue slots on (read from the code; DESIGN 4.2a says what was considered).
// Quantiser (dense_quantize_mx_kernel): plain integer / exact-fp32 code, not the hardware converts -- their saturation and
// subnormal rounding were not measured against the numpy statement, and the integer form is the same code on host and device.
//
// Listed variant (dense_maxsim_kernel<F, KB, DenseStore>: passages by id in a resident store).  kShiftAt: where the head keeps the
// entries' 16 x 8 store shifts -- behind s_own in the 1 KB heads; the 1280-byte heads have no room, so kListedHeadExtra = 128 more
// bytes, for this variant only.  Registers, same flags (VGPRs / SGPRs in lanes / waves per SIMD; no AGPRs, no scratch, no VGPR
// spills anywhere): fp32 KB = 32: 66 / 0 / 7, KB = 0: 29 / 0 / 8; fp16 and bf16 KB = 4: 108 / 3 / 4, KB = 0: 40 / 0 / 8; int8 KB = 2:
// 105 / 25 / 4, KB = 0: 71 / 11 / 7; MXFP8 KB = 1: 101 / 37 / 4, KB = 0: 83 / 14 / 5; MXFP4 KB = 1: 85 / 38 / 5, KB = 0: 79 / 14 / 6 --
// no occupancy below its unlisted twin's, whose figures (int8 KB = 0 today: 73 VGPRs, 13 in lanes, 6 waves) did not move.
#pragma once
#include "dense_kernels.hpp"

namespace clb {

typedef uint32_t dense_u32x4 __attribute__((ext_vector_type(4)));   // 8 halves: one lane's share of a K-block of one operand
typedef int dense_i32x4 __attribute__((ext_vector_type(4)));        // 16 int8: one lane's share of a K-block; or one accumulator

// What the formats whose two operands hold the same elements, ELEM bytes each, share: one fragment type, read as it lies.
template <typename FRAG, int ELEM>
struct DensePlain {
    typedef FRAG Frag;
    typedef FRAG QFrag;
    static constexpr int kElem = ELEM, kFragBytes = (int)sizeof(FRAG), kQFragBytes = (int)sizeof(FRAG), kLaneBytes = (int)sizeof(FRAG), kQLaneBytes = (int)sizeof(FRAG);
    static constexpr int kDimMultiple = ELEM < 4 ? 16 / ELEM : 4;
    __host__ __device__ static int row_bytes(int dim) { return ELEM * dim; }
    __host__ __device__ static int q_bytes(int dim) { return ELEM * dim; }
    // lane group g's fragment of a K-block, v already at it (its g-th); zeros, nothing read, where the row holds fewer than `left` bytes
    static __device__ __forceinline__ FRAG load_row(const unsigned char* v, const unsigned char*, int g, int left) {
        return (int)sizeof(FRAG) * g < left ? *reinterpret_cast<const FRAG*>(v) : FRAG{};
    }
    static __device__ __forceinline__ FRAG load_q(const unsigned char* v, const unsigned char* s, int g, int left) { return load_row(v, s, g, left); }
};

struct DenseF32 : DensePlain<float, 4> {
    typedef dense_f32x4 Acc;
    static constexpr int kK = 4, kRowTiles = 1, kHeadBytes = 1024, kOwnAt = 768, kRowpAt = 256, kShiftAt = 832, kListedHeadExtra = 0;
    static constexpr bool kResident = false, kScaled = false, kHasScales = false;
    __host__ __device__ static int scale_bytes(int) { return 0; }
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
struct Dense16Bit : Dense16ByteFrag, DensePlain<dense_u32x4, 2> {
    typedef dense_f32x4 Acc;
    static constexpr int kK = 32, kRowTiles = 2, kHeadBytes = 1024, kOwnAt = 768, kRowpAt = 256, kShiftAt = 832, kListedHeadExtra = 0;
    static constexpr bool kScaled = false, kHasScales = false;
    __host__ __device__ static int scale_bytes(int) { return 0; }
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

struct DenseI8 : Dense16ByteFrag, DensePlain<dense_i32x4, 1> {
    typedef dense_i32x4 Acc;
    static constexpr int kK = 64, kRowTiles = 4, kHeadBytes = 1280, kOwnAt = 192, kRowpAt = 256, kShiftAt = 1280, kListedHeadExtra = 128;
    static constexpr bool kScaled = true, kHasScales = true;
    __host__ __device__ static int scale_bytes(int) { return 4; }
    __host__ __device__ static int row_stride(int dim) { return padded(dim); }
    static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
    // the int32 sums to fp32 (exact), each times its row's scale
    static __device__ __forceinline__ dense_f32x4 epilogue(Acc acc, float4 ds) {
        return dense_f32x4{ds.x * (float)acc[0], ds.y * (float)acc[1], ds.z * (float)acc[2], ds.w * (float)acc[3]};
    }
};

// 1-bit sign rows against int8 queries: the row is stored as bits (2 bytes per lane and K-block) and widened to the int8
// fragment of +-1 that DenseI8's MFMA, epilogue and scales take; the query side is DenseI8's as it stands.
struct DenseB1 : Dense16ByteFrag {
    typedef dense_i32x4 Frag;                            // the WIDENED row fragment: 16 int8 of +-1
    typedef dense_i32x4 QFrag;
    typedef dense_i32x4 Acc;
    static constexpr int kK = 64, kRowTiles = 4, kHeadBytes = 1280, kOwnAt = 192, kRowpAt = 256, kShiftAt = 1280, kListedHeadExtra = 128, kDimMultiple = 128;
    static constexpr int kFragBytes = 2, kQFragBytes = 16, kLaneBytes = 2, kQLaneBytes = 16;
    static constexpr bool kScaled = true, kHasScales = true;
    __host__ __device__ static int row_bytes(int dim) { return dim >> 3; }
    __host__ __device__ static int q_bytes(int dim) { return dim; }
    __host__ __device__ static int scale_bytes(int) { return 4; }
    __host__ __device__ static int row_stride(int dim) { return padded(dim >> 3); }
    // The 16 bits at v (k = 64 kb + 16 g .. + 15, least significant first) as 16 int8: bit 1 -> +1, bit 0 -> -1.  The bits are
    // inverted once and a copy shifted by 4, so that every group of 4 is the HIGH nibble of some byte; per dword that byte is
    // replicated (v_perm), each copy keeps its own bit (0x10 << j in byte j), and a second v_perm reads the result as
    // selectors: 0 takes byte 0 of the table (0x01), anything >= 0x0d is the constant 0xff.
    static __device__ __forceinline__ Frag load_row(const unsigned char* v, const unsigned char*, int, int) {
        const uint32_t hn = ~(uint32_t)*reinterpret_cast<const uint16_t*>(v), hs = hn << 4;
        const uint32_t src[4] = {hs, hn, hs, hn};
        Frag f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t rep = __builtin_amdgcn_perm(src[i], src[i], i < 2 ? 0x00000000u : 0x01010101u);
            f[i] = (int)__builtin_amdgcn_perm(0x01010101u, 0x01010101u, rep & 0x80402010u);
        }
        return f;
    }
    static __device__ __forceinline__ QFrag load_q(const unsigned char* v, const unsigned char* s, int g, int left) { return DenseI8::load_q(v, s, g, left); }
    static __device__ __forceinline__ Acc mfma(Frag a, QFrag b, Acc c) { return DenseI8::mfma(a, b, c); }
    static __device__ __forceinline__ dense_f32x4 epilogue(Acc acc, float4 ds) { return DenseI8::epilogue(acc, ds); }
};

// MX block-scaled embeddings (OCP MX v1.0): passages MXFP8 (E4M3) or MXFP4 (E2M1), queries always MXFP8, one E8M0 scale byte
// per block of 32 elements.  A fragment is one block -- N16 16-byte columns of values and the block's scale byte, which
// the instruction takes from the lane that holds the block; the zero fragment is zero values under scale byte 127.
template <int N16>
struct DenseMXFrag {
    dense_u32x4 v[N16] = {};
    uint32_t s = 127;
};
template <bool E2M1>
struct DenseMX : Dense16ByteFrag {
    typedef DenseMXFrag<E2M1 ? 1 : 2> Frag;
    typedef DenseMXFrag<2> QFrag;
    typedef dense_f32x4 Acc;
    typedef int v8 __attribute__((ext_vector_type(8)));
    static constexpr int kK = 128, kRowTiles = 4, kHeadBytes = 1280, kOwnAt = 192, kRowpAt = 256, kShiftAt = 1280, kListedHeadExtra = 128, kDimMultiple = 32;
    static constexpr int kFragBytes = E2M1 ? 16 : 32, kQFragBytes = 32, kLaneBytes = 16, kQLaneBytes = 16;
    static constexpr bool kScaled = false, kHasScales = true;     // no fp32 scale, no epilogue multiply: the scales are in the product
    __host__ __device__ static int row_bytes(int dim) { return E2M1 ? dim >> 1 : dim; }
    __host__ __device__ static int q_bytes(int dim) { return dim; }
    __host__ __device__ static int scale_bytes(int dim) { return dim >> 5; }
    __host__ __device__ static int row_stride(int dim) { return padded(row_bytes(dim)); }
    // Lane group g's share of a K-block of 128 elements: v = the K-block's values + 16 g, s = its four scale bytes + g.  The
    // instruction reads an 8-bit operand as two halves of 64: registers 0-3 are k = 16 g .. 16 g + 15, registers 4-7
    // k = 64 + 16 g .. 64 + 16 g + 15 (measured: profiles/maxsim_batch_mx.md), a 4-bit operand as k = 32 g .. 32 g + 31; and it
    // scales block b = k / 32 by the byte lane group b supplies, so the lane's scale operand is byte g whatever values it holds.
    // `left`: the value bytes the row holds from v on; a 16-byte piece or a scale byte past them is zero / 127 and is not read.
    template <int N16>
    static __device__ __forceinline__ DenseMXFrag<N16> load(const unsigned char* v, const unsigned char* s, int g, int left) {
        DenseMXFrag<N16> f;
#pragma unroll
        for (int i = 0; i < N16; ++i)
            if (64 * i + 16 * g < left) f.v[i] = *reinterpret_cast<const dense_u32x4*>(v + 64 * i);
        if (16 * N16 * g < left) f.s = s[0];
        return f;
    }
    static __device__ __forceinline__ Frag load_row(const unsigned char* v, const unsigned char* s, int g, int left) { return load<E2M1 ? 1 : 2>(v, s, g, left); }
    static __device__ __forceinline__ QFrag load_q(const unsigned char* v, const unsigned char* s, int g, int left) { return load<2>(v, s, g, left); }
    template <int N16>
    static __device__ __forceinline__ v8 operand(const DenseMXFrag<N16>& f) {
        const dense_u32x4 hi = N16 == 2 ? f.v[N16 - 1] : dense_u32x4{};      // an E2M1 operand is the first four registers
        return v8{(int)f.v[0][0], (int)f.v[0][1], (int)f.v[0][2], (int)f.v[0][3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    }
    // A = the rows in their format (cbsz: 0 E4M3, 4 E2M1), B = the tokens in E4M3 (blgp 0); each lane's scale in its byte 0
    static __device__ __forceinline__ Acc mfma(const Frag& a, const QFrag& b, Acc c) {
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(operand(a), operand(b), c, E2M1 ? 4 : 0, 0, 0, (int)a.s, 0, (int)b.s);
    }
    static __device__ __forceinline__ dense_f32x4 epilogue(Acc acc, float4) { return acc; }
};
typedef DenseMX<false> DenseMXFP8;
typedef DenseMX<true> DenseMXFP4;

// The element code of y, a value already divided by its block's scale: round to nearest-even onto the format's grid (E4M3:
// 3 mantissa bits, least normal 2^-6, largest 448; E2M1: 1 bit, 1, 6), saturating; the sign is kept, a NaN gives the largest
// magnitude, and no NaN code comes out.  Every step is exact but the one rintf, so host and device agree bit for bit.
template <bool E2M1>
__host__ __device__ inline uint32_t dense_mx_encode(float y) {
    constexpr int M = E2M1 ? 1 : 3, EMIN = E2M1 ? 0 : -6, BIAS = E2M1 ? 1 : 7;
    auto pow2 = [](int k) { return __builtin_bit_cast(float, (uint32_t)(k + 127) << 23); };
    const float a = fminf(fabsf(y), E2M1 ? 6.f : 448.f);
    const int ea = (int)(__builtin_bit_cast(uint32_t, a) >> 23) - 127;
    const int eq = (ea > EMIN ? ea : EMIN) - M;                        // the grid's step at a is 2^eq
    const float r = rintf(a * pow2(-eq)) * pow2(eq);
    const uint32_t rb = __builtin_bit_cast(uint32_t, r);
    const int er = (int)(rb >> 23) - 127;
    const uint32_t mag = er < EMIN ? (uint32_t)(r * pow2(M - EMIN)) : ((uint32_t)(er + BIAS) << M | (rb >> (23 - M) & ((1u << M) - 1)));
    return (__builtin_bit_cast(uint32_t, y) >> 31) << (E2M1 ? 3 : 7) | mag;
}

// X (dim, n) fp32 -> MX values V ((dim, n) bytes, or (dim / 2, n) for E2M1: element 2 i in the low nibble of byte i) and scale
// bytes S (dim / 32, n), per block of 32: byte = max(0, E - emax) with E the biased fp32 exponent of the block's amax (= e + 127,
// e = max(-127, ilogb(amax) - emax); emax = 8 / 2), 127 for amax == 0; element = dense_mx_encode(x * 2^-e), the product exact.
// One wave per embedding, grid-stride; the row (dim <= 1024, dim % 32 == 0) is read once with float4 loads into at most 4
// registers per lane; a block is the 8 float4 of 8 consecutive lanes, so its maximum is a 3-step butterfly among them; the
// values leave as one dword (one half-word for E2M1) per lane and load, the scale byte from the block's first lane; no LDS.
// A non-finite input gives defined, meaningless numbers (v_max_f32 drops a NaN, an infinite amax gives byte 255 - emax, the
// encoder saturates).  X 16-byte aligned.
template <bool E2M1>
static __global__ __launch_bounds__(256) void dense_quantize_mx_kernel(const float* __restrict__ X, int dim, int64_t n,
                                                                       unsigned char* __restrict__ V, unsigned char* __restrict__ S) {
    constexpr int EMAX = E2M1 ? 2 : 8;
    const int lane = threadIdx.x & 63, dim4 = dim >> 2, nblk = dim >> 5;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t e = wave; e < n; e += n_waves) {
        const float4* src = reinterpret_cast<const float4*>(X + e * dim);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;                                // (c < dim4 is uniform over a block's 8 lanes)
            const float4 v = c < dim4 ? src[c] : make_float4(0.f, 0.f, 0.f, 0.f);
            float amax = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
#pragma unroll
            for (int d = 1; d < 8; d <<= 1) amax = fmaxf(amax, __shfl_xor(amax, d, 64));
            if (c >= dim4) continue;
            const int E = (int)(__float_as_uint(amax) >> 23);
            const int byte = amax == 0.f ? 127 : (E > EMAX ? E - EMAX : 0);
            const float inv = __uint_as_float((uint32_t)(254 - byte) << 23);      // 2^-e
            const uint32_t c0 = dense_mx_encode<E2M1>(v.x * inv), c1 = dense_mx_encode<E2M1>(v.y * inv);
            const uint32_t c2 = dense_mx_encode<E2M1>(v.z * inv), c3 = dense_mx_encode<E2M1>(v.w * inv);
            if constexpr (E2M1)
                reinterpret_cast<uint16_t*>(V + e * (dim >> 1))[c] = (uint16_t)(c0 | c1 << 4 | c2 << 8 | c3 << 12);
            else
                reinterpret_cast<uint32_t*>(V + e * dim)[c] = c0 | c1 << 8 | c2 << 16 | c3 << 24;
            if ((lane & 7) == 0) S[e * nblk + (c >> 3)] = (unsigned char)byte;
        }
    }
}

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

// X (dim, n) fp32 -> sign bits V (dim / 8, n) -- bit k & 7 of byte k >> 3 is x_k >= 0, so -0.0 gives 1 and a NaN 0 -- and scale
// [n]: s = (sum_k |x_k|) / dim, the least-squares scale of a sign code, summed in fp32 (each lane its own elements, then a
// butterfly).  One wave per embedding, grid-stride; the row (dim <= 1024, dim % 128 == 0) is read once with float4 loads.  A
// float4 is one nibble; a dword of V is the nibbles of 8 consecutive lanes, OR-ed together in 3 shuffle steps (dim / 4 is a
// multiple of 32, so the 8 lanes are all inside the row or all past it) and written by the first of them; no LDS.  A non-finite
// input gives defined, meaningless numbers.  X 16-byte, V 4-byte aligned.
static __global__ __launch_bounds__(256) void dense_binarize_kernel(const float* __restrict__ X, int dim, int64_t n,
                                                                    unsigned char* __restrict__ V, float* __restrict__ scale) {
    const int lane = threadIdx.x & 63, dim4 = dim >> 2;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t e = wave; e < n; e += n_waves) {
        const float4* src = reinterpret_cast<const float4*>(X + e * dim);
        uint32_t* dst = reinterpret_cast<uint32_t*>(V + e * (dim >> 3));
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            const float4 v = c < dim4 ? src[c] : make_float4(0.f, 0.f, 0.f, 0.f);
            sum += (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w));
            uint32_t word = ((uint32_t)(v.x >= 0.f) | (uint32_t)(v.y >= 0.f) << 1 | (uint32_t)(v.z >= 0.f) << 2 | (uint32_t)(v.w >= 0.f) << 3) << (4 * (lane & 7));
#pragma unroll
            for (int d = 1; d < 8; d <<= 1) word |= (uint32_t)__shfl_xor((int)word, d, 64);
            if (c < dim4 && (lane & 7) == 0) dst[c >> 3] = word;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) sum += __shfl_xor(sum, d, 64);
        if (lane == 0) scale[e] = sum / (float)dim;
    }
}

}  // namespace clb
