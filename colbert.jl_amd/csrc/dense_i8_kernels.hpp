// dense_i8_kernels.hpp -- MaxSim of un-indexed passages on int8 embeddings with one fp32 scale each (gfx950): fp32 scores out,
// bit-identical to a plain restatement:
//   dot     i(t, r) = sum_k q8[k, t] d8[k, r] by v_mfma_i32_16x16x64_i8: 64 exact products per instruction, summed in int32.
//           Integer addition is exact and order-free and |i| <= 1024 * 128 * 128 = 2^24, so float(i) is exact as well: the
//           only requirement on the operand layout is that A and B give a lane the same k.
//   max     m_t = max over the passage's rows of fl32(ds[r] * float(i)): one multiply per accumulator entry, then the exact
//           order-free maxima of dense_kernels.hpp.  The QUERY scale waits until after the maximum: qs[t] >= 0 and fp32
//           multiplication is monotone, so it selects the same row, and it costs one multiply per token instead of one per entry.
//   sum     acc = 0; acc = fl32(acc + fl32(qs[t] * m_t)) for t ascending (dense_i8_sum_maxima).  A (query, passage) that
//           received no row is -Inf by its offsets and owner, before any multiplication: qs[t] == 0 cannot turn it into a NaN.
// Taken from dense_kernels.hpp as they are: dense_offsets_kernel, dense_group_begin, dense_step_passages, dense_tile_max.  The
// 16 x 16 accumulator layout is the fp32 instruction's (lane (col r, g) holds rows 4 g + i), so segmentation, owner runs and the
// no-fault contract carry over from the 16-bit kernel; what differs is everything around the multiply.
//
// Operands.  Lane (r, g) of K-block kb holds the 16 consecutive bytes at 64 kb + 16 g of row (A) or token (B) r: one 16-byte
// global load (Q) or ds_read_b128 (D).  At dim 128 a 16-row tile is 2 K-blocks = 8 VGPRs, half of the 16-bit kernel's, so a
// wave keeps RT = 4 row tiles (64 rows, 32 VGPRs) beside the resident query's two token tiles (T <= 32: 16 VGPRs) and issues
// 2 MFMAs per (row tile, token tile).  Q residency, owner runs and the skip of row tiles outside a run are the 16-bit kernel's.
// K tail.  dim % 16 == 0, so a lane's 16 bytes lie wholly inside the row or wholly past it; past it both operands are zero
// registers and nothing is read (KB = 0 only; KB = 2 has no tail).
// LDS.  Head: s_off (17 x 8) | s_own at 192 (16 x 4) | s_rowp at 256 (256 x 4) = kDenseI8HeadBytes -- a step of 4 waves x 64
// rows needs 256 row-to-passage entries, twice what kDenseHeadBytes reserves, so this kernel lays out its own head and the
// other kernels keep theirs.  Then the maxima, then the step: rows global -> LDS once with 16-byte loads at a stride of dim
// bytes padded so that stride / 16 is odd (dim 128: 144), the 16-bit kernel's conflict-free rule for the b128 reads of 16
// consecutive lanes; the step's row scales (4 B per row) lie behind the rows, and lane (r, g) reads the four scales of the
// rows 4 g .. 4 g + 3 of a tile -- its accumulator entries' rows -- in one 16-byte read.  A 4-wave step at dim 128: 256 rows x
// 144 B + 1 KB of scales = 37 KB, what the 16-bit kernel's 128 rows cost.
// Tile epilogue.  v_cvt_f32_i32 on the four entries, one multiply each by the row's scale, dense_tile_max.  With two MFMAs per
// tile this epilogue, not the matrix pipe, is the likely limit of the all-pairs form (read from the code, not profiled;
// profiles/maxsim_batch_int8.md has the times).
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see the figures at dense_maxsim_i8_kernel below.
// Safety, all by construction: clamped offsets, so no row at or past n_D is read -- neither its bytes nor its scale; an owner
// outside 0..B-1 multiplies nothing and reads no query scale; a token column past T reads token T - 1 and reaches no
// maximum; rows past the step's end (whatever the LDS holds there) reach no maximum; no allocation, no host wait.
#pragma once
#include "dense_kernels.hpp"

namespace clb {

typedef int dense_i32x4 __attribute__((ext_vector_type(4)));   // 16 int8: one lane's share of a K-block; or one accumulator

constexpr int kDenseI8WaveTiles = 4;       // row tiles of 16 per wave: 64 rows
constexpr int kDenseI8HeadBytes = 1280;    // s_off (17 x 8) | s_own at 192 (16 x 4) | s_rowp at 256 (<= 256 x 4)

__host__ __device__ inline int dense_i8_row_stride(int dim) { return dim % 32 == 0 ? dim + 16 : dim; }   // bytes; stride / 16 odd

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

// One 16 x 16 tile: its int32 sums to fp32 (exact), each times its row's scale, and its maxima.
__device__ __forceinline__ void dense_i8_tile_max(const dense_i32x4 acc, const float4 ds, const int* __restrict__ rowp16, int pa, int pb,
                                                  bool tok_ok, uint32_t* __restrict__ pm, int TP, int t, int g) {
    const dense_f32x4 m = {ds.x * (float)acc[0], ds.y * (float)acc[1], ds.z * (float)acc[2], ds.w * (float)acc[3]};
    dense_tile_max(m, rowp16, pa, pb, tok_ok, pm, TP, t, g);
}

// One token tile (KB K-blocks in registers) against a wave's RT row tiles: 2 MFMAs and one epilogue per row tile of the run.
template <int KB, int RT>
__device__ __forceinline__ void dense_i8_tiles(const dense_i32x4 (*a)[KB], const dense_i32x4* b, const float4* ds, int on,
                                               const int* __restrict__ rowp, int pa, int pb, bool tok_ok, uint32_t* __restrict__ pm,
                                               int TP, int t, int g) {
#pragma unroll
    for (int j = 0; j < RT; ++j) {
        if (!(on >> j & 1)) continue;                      // (wave-uniform)
        dense_i32x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[j][kb], b[kb], acc, 0, 0, 0);
        dense_i8_tile_max(acc, ds[j], rowp + 16 * j, pa, pb, tok_ok, pm, TP, t, g);
    }
}

// acc = 0; acc = acc + qs[t] * max_t, t ascending, per (query, passage); -Inf where the pair received no row: an empty
// (clamped) passage, or an owner outside the batch -- whose query scales are not read.
__device__ __forceinline__ void dense_i8_sum_maxima(const uint32_t* __restrict__ s_pm, const int64_t* __restrict__ s_off,
                                                    const int* __restrict__ s_own, const float* __restrict__ qscale, int nq, int np,
                                                    int G, int TP, int T, int B, bool owned, int64_t p0, int q0, int64_t N,
                                                    float* __restrict__ scores) {
    for (int i = threadIdx.x; i < nq * np; i += blockDim.x) {
        const int ql = i / np, p = i - ql * np;
        const int q = owned ? s_own[p] : q0 + ql;
        float acc = kNegInf;
        if (s_off[p + 1] > s_off[p] && q >= 0 && q < B) {
            const uint32_t* pm = s_pm + (ql * G + p) * TP;
            const float* qs = qscale + (size_t)q * T;
            acc = 0.f;
            for (int t = 0; t < T; ++t) acc = acc + qs[t] * f32_from_order_key(pm[t]);
        }
        scores[owned ? p0 + p : (int64_t)(q0 + ql) * N + p0 + p] = acc;
    }
}

// KB = dim / 64 K-blocks of both operands in registers (dim 128: KB 2); 0 = any served dim, K walked at run time with the
// operands read where they lie.  RT row tiles (16 RT rows) per wave.  Q8 (dim, T, B) and D8 (dim, n_D) int8, both 16-byte
// aligned; qscale (T, B) and dscale [n_D] fp32.
// grid (ceil(N / G), owned ? 1 : ceil(B / QB)); block 64 * nw;
// dynamic LDS = kDenseI8HeadBytes + 4 * (owned ? 1 : QB) * G * (T | 1) rounded up to 16 + 16 RT nw * (dense_i8_row_stride(dim) + 4).
// Registers (gfx950, -Rpass-analysis=kernel-resource-usage): KB = 2, RT = 4: 106 VGPRs, no AGPRs, no scratch, no VGPR spills,
// 4 waves per SIMD -- the 3 (all pairs) or 4 (owned) work-groups of 4 waves per CU that the LDS allows, so registers do not
// lower the occupancy.  The scalar side is full: 25 SGPRs (loop-invariant pointers and saved exec masks) are parked in lanes
// of one VGPR (v_writelane in the prologue, v_readlane where used) -- SGPR spills in the report, no memory traffic; they have
// not been removed.  RT = 2 (32 rows per wave: half the step's LDS, so more work-groups per CU in the owned form) has not
// been measured against RT = 4.  KB = 0: 69 VGPRs, 11 SGPRs in lanes.
template <int KB, int RT>
static __global__ __launch_bounds__(256) void dense_maxsim_i8_kernel(const int8_t* __restrict__ Q8, const float* __restrict__ qscale,
                                                                     int dim, int T, int B, const int8_t* __restrict__ D8,
                                                                     const float* __restrict__ dscale, const int64_t* __restrict__ off,
                                                                     int64_t N, const int32_t* __restrict__ owner, int G, int QB,
                                                                     float* __restrict__ scores) {
    extern __shared__ __align__(16) unsigned char dense_smem[];
    constexpr int KR = KB > 0 ? KB : 1, WR = 16 * RT;
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar, so that what hangs on the wave's rows is wave-uniform to the compiler
    const int CH = (nthr >> 6) * WR;                      // rows per step of the work-group
    const int stride = dense_i8_row_stride(dim), TP = T | 1, dim16 = dim >> 4, nkb = (dim + 63) >> 6;
    const bool owned = owner != nullptr;
    const int64_t p0 = (int64_t)blockIdx.x * G;
    const int np = (int)(N - p0 < G ? N - p0 : G);
    const int q0 = owned ? 0 : (int)blockIdx.y * QB;
    const int nq = owned ? 1 : (B - q0 < QB ? B - q0 : QB);
    int64_t* s_off = reinterpret_cast<int64_t*>(dense_smem);
    int* s_own = reinterpret_cast<int*>(dense_smem + 192);
    int* s_rowp = reinterpret_cast<int*>(dense_smem + 256);
    uint32_t* s_pm = reinterpret_cast<uint32_t*>(dense_smem + kDenseI8HeadBytes);
    const int pm_words = (owned ? 1 : QB) * G * TP;
    unsigned char* s_d = dense_smem + kDenseI8HeadBytes + ((size_t)pm_words * 4 + 15) / 16 * 16;
    float* s_ds = reinterpret_cast<float*>(s_d + (size_t)CH * stride);     // the step's row scales (CH * stride is a multiple of 16)

    dense_group_begin(s_off, s_own, s_pm, off, owner, p0, np, pm_words);
    __syncthreads();
    const int64_t lo = s_off[0], hi = s_off[np];

    const dense_i32x4 zero = {0, 0, 0, 0};
    const bool resident = KB > 0 && T <= 32;
    dense_i32x4 bq[2][KR];                                 // the resident query's token tiles (resident only)
    int q_res = -1;                                        // (wave-uniform) the query they hold
    // lane (r, g)'s share of K-block kb of token t of query q, t clamped to the last token
    auto q_frag = [&](int q, int t, int kb) {
        return *reinterpret_cast<const dense_i32x4*>(Q8 + ((size_t)q * T + (t < T ? t : T - 1)) * dim + 64 * kb + 16 * g);
    };

    for (int64_t c = lo; c < hi; c += CH) {
        const int n_rows = (int)(hi - c < CH ? hi - c : CH);
        // the step's rows, dense 16-byte loads (D8 + c * dim is 16-byte aligned: dim % 16 == 0), into padded LDS rows; their scales
        const dense_i32x4* src = reinterpret_cast<const dense_i32x4*>(D8 + c * dim);
        for (int i = tid; i < n_rows * dim16; i += nthr) {
            const int row = i / dim16, c16 = i - row * dim16;
            *reinterpret_cast<dense_i32x4*>(s_d + row * stride + 16 * c16) = src[i];
        }
        for (int i = tid; i < n_rows; i += nthr) s_ds[i] = dscale[c + i];
        dense_step_passages(s_off, s_rowp, c, n_rows, CH, np);
        __syncthreads();

        const int rb = WR * w;                              // this wave's rows of the step: RT tiles of 16
        if (rb < n_rows) {
            const int* rowp = s_rowp + rb;
            const unsigned char* arow = s_d + (rb + r) * stride + 16 * g;
            dense_i32x4 a[RT][KR];
            float4 ds[RT];
            uint32_t tf = 0, tl = 0;                        // (wave-uniform) byte j: tile j's first and last passage (< 16); none: first > last
#pragma unroll
            for (int j = 0; j < RT; ++j) {
                const bool live = rb + 16 * j < n_rows;
                const int end = rb + 16 * j + 15 < n_rows ? rb + 16 * j + 15 : n_rows - 1;
                tf |= (uint32_t)(live ? __builtin_amdgcn_readfirstlane(s_rowp[rb + 16 * j]) : 1) << (8 * j);
                tl |= (uint32_t)(live ? __builtin_amdgcn_readfirstlane(s_rowp[end]) : 0) << (8 * j);
                ds[j] = live ? *reinterpret_cast<const float4*>(s_ds + rb + 16 * j + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (KB > 0) {
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb) a[j][kb] = live ? *reinterpret_cast<const dense_i32x4*>(arow + 16 * j * stride + 64 * kb) : zero;
                }
            }
            const int last = (rb + WR < n_rows ? rb + WR : n_rows) - 1;
            const int pf = (int)(tf & 255u), pl =__builtin_amdgcn_readfirstlane(s_rowp[last]);
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
                    int on = 0;                            // (wave-uniform) bit j: tile j holds a row of the run
#pragma unroll
                    for (int j = 0; j < RT; ++j) {
                        const int f = (int)(tf >> (8 * j) & 255u), l = (int)(tl >> (8 * j) & 255u);
                        on |= (int)(f <= pb && l >= pa && f <= l) << j;
                    }
                    if (resident) {
                        if (q != q_res) {
#pragma unroll
                            for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                                for (int kb = 0; kb < KR; ++kb) bq[tt][kb] = 16 * tt < T ? q_frag(q, 16 * tt + r, kb) : zero;
                            }
                            q_res = q;
                        }
#pragma unroll
                        for (int tt = 0; tt < 2; ++tt)
                            if (16 * tt < T) dense_i8_tiles<KR, RT>(a, bq[tt], ds, on, rowp, pa, pb, 16 * tt + r < T, pm, TP, 16 * tt + r, g);
                    } else if (KB > 0) {
                        for (int t0 = 0; t0 < T; t0 += 16) {
                            dense_i32x4 bt[KR];
#pragma unroll
                            for (int kb = 0; kb < KR; ++kb) bt[kb] = q_frag(q, t0 + r, kb);
                            dense_i8_tiles<KR, RT>(a, bt, ds, on, rowp, pa, pb, t0 + r < T, pm, TP, t0 + r, g);
                        }
                    } else {
                        for (int t0 = 0; t0 < T; t0 += 16) {
                            dense_i32x4 acc[RT];
#pragma unroll
                            for (int j = 0; j < RT; ++j) acc[j] = zero;
                            for (int kb = 0; kb < nkb; ++kb) {
                                const bool k_ok = 64 * kb + 16 * g < dim;        // past the row: zeros, nothing read
                                const dense_i32x4 b = k_ok ? q_frag(q, t0 + r, kb) : zero;
#pragma unroll
                                for (int j = 0; j < RT; ++j)
                                    if (on >> j & 1)
                                        acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                                            k_ok ? *reinterpret_cast<const dense_i32x4*>(arow + 16 * j * stride + 64 * kb) : zero, b, acc[j], 0, 0, 0);
                            }
#pragma unroll
                            for (int j = 0; j < RT; ++j)
                                if (on >> j & 1) dense_i8_tile_max(acc[j], ds[j], rowp + 16 * j, pa, pb, t0 + r < T, pm, TP, t0 + r, g);
                        }
                    }
                }
                if (owned) pa = pb + 1; else ++ql;
            }
        }
        __syncthreads();                                    // the step's rows, scales and passages are read; the next step overwrites them
    }

    dense_i8_sum_maxima(s_pm, s_off, s_own, qscale, nq, np, G, TP, T, B, owned, p0, q0, N, scores);
}

}  // namespace clb
