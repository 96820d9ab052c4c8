// dense_kernels.hpp -- MaxSim of un-indexed passages for a batch of queries (gfx950): the one kernel frame of every
// embedding format, fp32 scores out.  A format (dense_formats.hpp) supplies its fragment types and how one is read (rows and
// query tokens each their own: their element formats may differ, and a fragment may carry a block scale), its MFMA, its tile
// epilogue, its LDS row stride, scale bytes and head; everything below exists once.
//   dot     one MFMA per K-block, the K-blocks in ascending order from +0: embeddings are tile rows, query tokens are tile
//           columns.  Lane (r, g) holds, of K-block kb of row or token r, the FRAG consecutive elements at K kb + FRAG g --
//           one fragment of F::kFragBytes (rows) or F::kQFragBytes (tokens) bytes, K = 4 FRAG -- and the same k in the A and
//           the B operand; lane group g's bytes begin F::kLaneBytes g (rows) / F::kQLaneBytes g (tokens) into the K-block, and a
//           format may widen what it read (1-bit rows: 2 stored bytes become the 16 int8 of the register fragment).  Where a format's instruction orders K otherwise it says so in its load (F::load_row, F::load_q: the
//           lane's first byte of the K-block, lane group g and the bytes the row still holds from the K-block's start).  The accumulator
//           layout is the same for every format: lane (col r, g) holds the rows 4 g + i, i = 0..3.
//   max     exact and order-free, so partial maxima of a passage combine in any order (LDS atomic max on order keys)
//   sum     one serial chain per (passage, query), t ascending (dense_sum_maxima)
//
// Work split.  A work-group owns G consecutive PASSAGES (so its rows are consecutive and cut at passage boundaries) and, in
// the all-pairs form, a block of QB queries.  It walks its rows in steps of 16 RT rows per wave (RT row tiles: F::kRowTiles):
// a step is brought from global memory into LDS once with 16-byte loads (rows are contiguous, so the loads are dense), in
// rows padded to the format's stride so that the A-operand reads are conflict-free.  At dim 128 (KB > 0) a wave keeps its
// RT row tiles as registers of A operand and re-uses them for every token tile of every query of the block; other dims
// (KB = 0) walk K at run time, both operands read where they lie.
// Q residency (F::kResident, KB > 0, T <= 32).  The query's one or two token tiles are loaded when a wave meets a query it does
// not hold and kept across owner runs, steps and -- in the all-pairs form, while the block holds one query -- the whole
// work-group; a block of several queries reloads per (step, query).  Otherwise each token tile is read where it is used.
// Segmentation.  Every row of a step knows its passage (s_rowp; -1 past the end of the group).  A tile whose 16 rows lie in
// one passage reduces in registers (3 fmax, 2 shuffles) and issues one LDS atomic per token; a tile that straddles passages
// issues one per (row, token), to the row's own passage -- a neighbour's row never reaches a maximum.  In the owned form a
// wave multiplies a tile once per RUN of consecutive passages with the same owner, and only the row tiles that hold a row
// of the run.
// Long passages span several steps and several waves of their work-group: their partial maxima meet in the same LDS words.
// K tail.  dim is a multiple of the elements of one 16-byte piece of a fragment, so a piece lies wholly inside the row or
// wholly past it; past it both operands hold zeros (nothing is read, neither values nor scale), and zeros add exact zeros
// (KB = 0 only).
// Safety, all by construction and stated here once: the offsets are a clamped scan (negative doclen = 0, every offset <= n_D),
// so no row at or past n_D is read -- neither its elements nor its scale; an owner outside 0..B-1 multiplies nothing and
// reads no query scale; a token column past T reads token T - 1 and reaches no maximum; rows past the step's end (whatever
// the LDS holds there) reach no maximum.  A (passage, query) that received no row keeps -Inf in every token and sums to -Inf.
// No allocation, no host wait.
#pragma once
#include "common.hpp"

namespace clb {

typedef float dense_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kDenseMaxGroup = 16;         // passages per work-group, at most
constexpr int kDensePmWords = 4096;        // LDS words of per-(query, passage, token) maxima per work-group
constexpr int kDenseWholeRow = 1 << 30;    // "bytes left in the row" where the K-block lies wholly inside it

// The dynamic LDS of one launch, in bytes from its start: the head (s_off at 0, 17 x 8; s_own and s_rowp where the format puts
// them), the maxima, the step's rows at `stride` bytes each, the step's row scales (F::scale_bytes(dim) per row).  The kernel carves its
// LDS by it and the host asks for `total`.  listed (the by-id variant): the head also holds the entries' 16 x 8 store shifts at
// F::kShiftAt, F::kListedHeadExtra bytes longer where the format's own head has no room for them; the unlisted layout is untouched.
struct DenseLayout {
    int stride, step_rows, pm_words;
    size_t pm, rows, scales, total;
};
template <typename F>
__host__ __device__ inline DenseLayout dense_layout(int dim, int T, int QB, int G, int nw, bool owned, bool listed = false) {
    DenseLayout l;
    l.stride = F::row_stride(dim);
    l.step_rows = 16 * F::kRowTiles * nw;
    l.pm_words = (owned ? 1 : QB) * G * (T | 1);
    l.pm = F::kHeadBytes + (listed ? F::kListedHeadExtra : 0);
    l.rows = l.pm + ((size_t)l.pm_words * 4 + 15) / 16 * 16;
    l.scales = l.rows + (size_t)l.step_rows * l.stride;     // a multiple of 16: the stride is
    l.total = l.scales + (size_t)F::scale_bytes(dim) * l.step_rows;
    return l;
}

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

// What the listed variant of the kernel takes beside the frame's arguments: the entries to score and the store's extent.
struct DenseStore {
    const int64_t* pids;   // [N] stored passages, 0-based; outside 0..P-1: no rows
    int64_t P, n_store;    // stored passages (off holds P + 1 offsets) and stored rows
};
__device__ __forceinline__ DenseStore dense_store_of() { return DenseStore{nullptr, 0, 0}; }
__device__ __forceinline__ DenseStore dense_store_of(DenseStore s) { return s; }

// The group's offsets and owners into the LDS head and every maximum to -Inf; the barrier after it is the caller's.
// LISTED: the group is np <= 16 entries of a pid list and `off` the STORE's offsets [P + 1].  Lane i of wave 0 reads pid i and
// clamps its range -- a pid outside 0..P-1 is an empty range at 0; start = clamp(off[pid], 0, n_store), end = clamp(off[pid + 1],
// start, n_store), all before any row address is formed --; the local offsets are the prefix sum of the lengths (four shuffle
// steps, no barrier of its own), and s_shift[i] = start - s_off[i]: local row e of entry i is store row e + s_shift[i] < end.
template <bool LISTED>
__device__ __forceinline__ void dense_group_begin(int64_t* __restrict__ s_off, int* __restrict__ s_own, uint32_t* __restrict__ s_pm,
                                                  const int64_t* __restrict__ off, const int32_t* __restrict__ owner, int64_t p0,
                                                  int np, int pm_words, int64_t* __restrict__ s_shift, const int64_t* __restrict__ pids,
                                                  int64_t P, int64_t n_store) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    if constexpr (LISTED) {
        if (tid < 64) {
            int64_t start = 0, len = 0;
            if (tid < np) {
                const int64_t pid = pids[p0 + tid];
                if (pid >= 0 && pid < P) {
                    const int64_t a = off[pid], b = off[pid + 1];
                    start = a < 0 ? 0 : (a > n_store ? n_store : a);
                    len = (b < start ? start : (b > n_store ? n_store : b)) - start;
                }
            }
            int64_t incl = len;
#pragma unroll
            for (int d = 1; d < kDenseMaxGroup; d <<= 1) {
                const int64_t o = __shfl_up(incl, d, 64);
                if (tid >= d) incl += o;
            }
            if (tid == 0) s_off[0] = 0;
            if (tid < np) {
                s_off[tid + 1] = incl;
                s_shift[tid] = start - (incl - len);
            }
        }
    } else {
        for (int i = tid; i <= np; i += nthr) s_off[i] = off[p0 + i];
    }
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

// One ordered fp32 sum per (query, passage): acc = 0; acc = acc + max_t, t ascending (ranking.jl:83).  A scaled format:
// acc = acc + qs[t] * max_t, and -Inf where the pair received no row -- an empty (clamped) passage, or an owner outside the
// batch, whose query scales are not read -- before any multiplication: qs[t] == 0 cannot turn it into a NaN.
template <typename F>
__device__ __forceinline__ void dense_sum_maxima(const uint32_t* __restrict__ s_pm, const int64_t* __restrict__ s_off,
                                                 const int* __restrict__ s_own, const void* __restrict__ qscale, int nq, int np,
                                                 int G, int TP, int T, int B, bool owned, int64_t p0, int q0, int64_t N,
                                                 float* __restrict__ scores) {
    for (int i = threadIdx.x; i < nq * np; i += blockDim.x) {
        const int ql = i / np, p = i - ql * np;
        const uint32_t* pm = s_pm + (ql * G + p) * TP;
        float acc = 0.f;
        if constexpr (F::kScaled) {
            const int q = owned ? s_own[p] : q0 + ql;
            if (s_off[p + 1] > s_off[p] && q >= 0 && q < B) {
                const float* qs = static_cast<const float*>(qscale) + (size_t)q * T;
                for (int t = 0; t < T; ++t) acc = acc + qs[t] * f32_from_order_key(pm[t]);
            } else {
                acc = kNegInf;
            }
        } else {
            for (int t = 0; t < T; ++t) acc = acc + f32_from_order_key(pm[t]);
        }
        scores[owned ? p0 + p : (int64_t)(q0 + ql) * N + p0 + p] = acc;
    }
}

// One token tile against a wave's RT row tiles, those that hold a row of the run (bit j of `on`, wave-uniform).  KB > 0: KB
// K-blocks of both operands from registers (a, b), tile after tile: its MFMA chain, its epilogue, its maxima.  KB = 0: K walked
// at run time for all row tiles at once, A read from the LDS rows at arow, B once per K-block from the token at qtok (this
// lane's share of its row and token, F::kLaneBytes g bytes into K-block 0; asc and qsc: the lane's scale byte of K-block 0,
// nsb bytes per row, null for a format without block scales), then the epilogues and maxima.
template <typename F, int KB>
__device__ __forceinline__ void dense_tiles(const typename F::Frag (*a)[KB > 0 ? KB : 1], const typename F::QFrag* b,
                                            const unsigned char* arow, int stride, const unsigned char* asc, int nsb,
                                            const unsigned char* qtok, const unsigned char* qsc, int dim, const float4* ds,
                                            int on, const int* __restrict__ rowp, int pa, int pb, bool tok_ok,
                                            uint32_t* __restrict__ pm, int TP, int t, int g) {
    typedef typename F::Frag Frag;
    typedef typename F::QFrag QFrag;
    constexpr int RT = F::kRowTiles, FB = F::kFragBytes, QFB = F::kQFragBytes;
    if constexpr (KB > 0) {
#pragma unroll
        for (int j = 0; j < RT; ++j) {
            if (!(on >> j & 1)) continue;
            typename F::Acc acc = {};
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) acc = F::mfma(a[j][kb], b[kb], acc);
            dense_tile_max(F::epilogue(acc, ds[j]), rowp + 16 * j, pa, pb, tok_ok, pm, TP, t, g);
        }
    } else {
        constexpr bool tail = 4 * FB > 16;                  // a K-block is wider than the 16-byte column dim is a multiple of
        const int row_bytes = F::row_bytes(dim), q_bytes = F::q_bytes(dim), nkb = (row_bytes + 4 * FB - 1) / (4 * FB);
        typename F::Acc acc[RT];
#pragma unroll
        for (int j = 0; j < RT; ++j) acc[j] = typename F::Acc{};
        for (int kb = 0; kb < nkb; ++kb) {
            // what the row and the token still hold from this K-block on: past it a fragment is zeros and nothing is read
            const int left = tail ? row_bytes - 4 * FB * kb : kDenseWholeRow, qleft = tail ? q_bytes - 4 * QFB * kb : kDenseWholeRow;
            const QFrag bk = F::load_q(qtok + 4 * QFB * kb, qsc + 4 * kb, g, qleft);
#pragma unroll
            for (int j = 0; j < RT; ++j)
                if (on >> j & 1)
                    acc[j] = F::mfma(F::load_row(arow + 16 * j * stride + 4 * FB * kb, asc + 16 * j * nsb + 4 * kb, g, left), bk, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < RT; ++j)
            if (on >> j & 1) dense_tile_max(F::epilogue(acc[j], ds[j]), rowp + 16 * j, pa, pb, tok_ok, pm, TP, t, g);
    }
}

// F = the format (dense_formats.hpp).  KB = dim / F::kK K-blocks of both operands in registers (dim 128); 0 = any served dim.
// Q (dim, T, B) and D (dim, n_D) hold F's elements, D 16-byte aligned and Q aligned to 16 bytes or a fragment, whichever is
// less; qscale (T, B) and dscale [n_D]: F::scale_bytes(dim) bytes per embedding (one fp32, or one byte per block of 32), read
// by a format that has scales only.
// grid (ceil(N / G), owned ? 1 : ceil(B / QB)); block 64 * nw; dynamic LDS = dense_layout<F>(dim, T, QB, G, nw, owned, LISTED).total.
// LISTED (a DenseStore as the last argument): D and dscale are a resident store of n_store rows, `off` its offsets [P + 1] and the N
// passages are the entries of `pids`: a work-group owns G consecutive ENTRIES.  Its prologue turns them into local offsets
// (dense_group_begin), so everything from the row-to-passage map on runs on local row numbers as it does unlisted; only the
// step's load differs: local row e of entry p is store row e + s_shift[p], one row at a time -- still dense 16-byte columns, its
// scales per row --, and since a row's entry must be known before its address the map is resolved first, behind a barrier of
// its own (the alternative, a search of the 17 LDS offsets inside the load loop, repeats the four dependent LDS reads once per
// 16-byte column -- 8 to 32 times a row at dim 128 -- and puts them in front of every global load; the map is needed anyway.
// Chosen from the code; the two were not timed against each other).
// STORE: nothing (unlisted: the kernel's arguments are those above and no more), or one DenseStore (LISTED).
template <typename F, int KB, typename... STORE>
static __global__ __launch_bounds__(256) void dense_maxsim_kernel(const void* __restrict__ Qv, const void* __restrict__ qscale, int dim,
                                                                  int T, int B, const void* __restrict__ Dv,
                                                                  const void* __restrict__ dscale, const int64_t* __restrict__ off,
                                                                  int64_t N, const int32_t* __restrict__ owner, int G, int QB,
                                                                  float* __restrict__ scores, STORE... store) {
    constexpr bool LISTED = sizeof...(STORE) > 0;
    const DenseStore st = dense_store_of(store...);
    extern __shared__ __align__(16) unsigned char dense_smem[];
    typedef typename F::Frag Frag;
    typedef typename F::QFrag QFrag;
    typedef uint32_t col16 __attribute__((ext_vector_type(4)));                  // one 16-byte column of a row
    constexpr int RT = F::kRowTiles, WR = 16 * RT, KR = KB > 0 ? KB : 1, FB = F::kFragBytes, QFB = F::kQFragBytes;
    const unsigned char* Q = static_cast<const unsigned char*>(Qv);
    const unsigned char* D = static_cast<const unsigned char*>(Dv);
    const unsigned char* QS = static_cast<const unsigned char*>(qscale);
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar, so that what hangs on the wave's rows is wave-uniform to the compiler
    const bool owned = owner != nullptr;
    const DenseLayout L = dense_layout<F>(dim, T, QB, G, nthr >> 6, owned, LISTED);
    const int CH = L.step_rows, stride = L.stride, TP = T | 1, cols = F::row_bytes(dim) >> 4;   // rows per step; 16-byte columns per row
    const int nsb = F::scale_bytes(dim);                                         // scale bytes per embedding
    constexpr bool BS = F::kHasScales && !F::kScaled;                            // block scales inside the fragments: else no scale pointer lives
    const int fsb = BS ? nsb : 0;
    const int64_t p0 = (int64_t)blockIdx.x * G;
    const int np = (int)(N - p0 < G ? N - p0 : G);
    const int q0 = owned ? 0 : (int)blockIdx.y * QB;
    const int nq = owned ? 1 : (B - q0 < QB ? B - q0 : QB);
    int64_t* s_off = reinterpret_cast<int64_t*>(dense_smem);
    int* s_own = reinterpret_cast<int*>(dense_smem + F::kOwnAt);
    int* s_rowp = reinterpret_cast<int*>(dense_smem + F::kRowpAt);
    int64_t* s_shift = reinterpret_cast<int64_t*>(dense_smem + F::kShiftAt);   // (LISTED only)
    uint32_t* s_pm = reinterpret_cast<uint32_t*>(dense_smem + L.pm);
    unsigned char* s_d = dense_smem + L.rows;
    unsigned char* s_sc = dense_smem + L.scales;                                // the step's row scales, nsb bytes per row
    float* s_ds = reinterpret_cast<float*>(s_sc);                               // (a format with one fp32 scale per row)

    dense_group_begin<LISTED>(s_off, s_own, s_pm, off, owner, p0, np, L.pm_words, s_shift, st.pids, st.P, st.n_store);
    __syncthreads();
    const int64_t lo = s_off[0], hi = s_off[np];

    const Frag zero = {};
    const QFrag qzero = {};
    const bool resident = F::kResident && KB > 0 && T <= 32;
    QFrag bq[2][KR];                                       // the resident query's token tiles (resident only)
    int q_res = -1;                                        // (wave-uniform) the query they hold
    // K-block 0 of token t of query q, t clamped to the last token; K-block kb lies 4 QFB kb bytes on.  q_sc: the same for its
    // block scales, K-block kb 4 bytes on (a format whose fragments carry one)
    auto q_tok = [&](int q, int t) { return Q + ((size_t)q * T + (t < T ? t : T - 1)) * F::q_bytes(dim) + F::kQLaneBytes * g; };
    auto q_sc = [&](int q, int t) { return BS ? QS + ((size_t)q * T + (t < T ? t : T - 1)) * nsb + g : nullptr; };

    for (int64_t c = lo; c < hi; c += CH) {
        const int n_rows = (int)(hi - c < CH ? hi - c : CH);
        if constexpr (LISTED) {
            // every row's entry first, then the row from where the store keeps it: 16-byte columns of one row are consecutive,
            // rows are not; its scales per row, in dwords where a row's are whole dwords, no row's but those read
            dense_step_passages(s_off, s_rowp, c, n_rows, CH, np);
            __syncthreads();
            auto store_row = [&](int row) { return c + row + s_shift[s_rowp[row]]; };
            for (int i = tid; i < n_rows * cols; i += nthr) {
                const int row = i / cols, col = i - row * cols;
                *reinterpret_cast<col16*>(s_d + row * stride + 16 * col) = reinterpret_cast<const col16*>(D + store_row(row) * F::row_bytes(dim))[col];
            }
            if constexpr (F::kHasScales) {
                const unsigned char* ssrc = static_cast<const unsigned char*>(dscale);
                if (nsb % 4 == 0) {
                    const int nsw = nsb >> 2;
                    for (int i = tid; i < n_rows * nsw; i += nthr) {
                        const int row = i / nsw;
                        reinterpret_cast<uint32_t*>(s_sc)[i] = reinterpret_cast<const uint32_t*>(ssrc + store_row(row) * nsb)[i - row * nsw];
                    }
                } else {
                    for (int i = tid; i < n_rows * nsb; i += nthr) {
                        const int row = i / nsb;
                        s_sc[i] = ssrc[store_row(row) * nsb + (i - row * nsb)];
                    }
                }
            }
        } else {
            // the step's rows, dense 16-byte loads (D + c rows is 16-byte aligned), into padded LDS rows; their scales -- those of
            // the rows read, no others -- in dwords where a row's are whole dwords (then dscale + c rows is 4-byte aligned)
            const col16* src = reinterpret_cast<const col16*>(D + c * F::row_bytes(dim));
            for (int i = tid; i < n_rows * cols; i += nthr) {
                const int row = i / cols, col = i - row * cols;
                *reinterpret_cast<col16*>(s_d + row * stride + 16 * col) = src[i];
            }
            if constexpr (F::kHasScales) {
                const unsigned char* ssrc = static_cast<const unsigned char*>(dscale) + c * nsb;
                if (nsb % 4 == 0) {
                    for (int i = tid; i < n_rows * (nsb >> 2); i += nthr) reinterpret_cast<uint32_t*>(s_sc)[i] = reinterpret_cast<const uint32_t*>(ssrc)[i];
                } else {
                    for (int i = tid; i < n_rows * nsb; i += nthr) s_sc[i] = ssrc[i];
                }
            }
            dense_step_passages(s_off, s_rowp, c, n_rows, CH, np);
        }
        __syncthreads();

        const int rb = WR * w;                             // this wave's rows of the step: RT tiles of 16
        if (rb < n_rows) {
            const int* rowp = s_rowp + rb;
            const unsigned char* arow = s_d + (rb + r) * stride + F::kLaneBytes * g;   // this lane's share of its row of tile 0, and its scale byte
            const unsigned char* asc = BS ? s_sc + (rb + r) * nsb + g : nullptr;
            Frag a[RT][KR];
            float4 ds[RT];
            uint32_t tf = 0, tl = 0;                        // (wave-uniform) byte j: tile j's first and last passage (< 16); none: first > last
#pragma unroll
            for (int j = 0; j < RT; ++j) {
                const bool live = rb + 16 * j < n_rows;
                const int end = rb + 16 * j + 15 < n_rows ? rb + 16 * j + 15 : n_rows - 1;
                tf |= (uint32_t)(live ? __builtin_amdgcn_readfirstlane(s_rowp[rb + 16 * j]) : 1) << (8 * j);
                tl |= (uint32_t)(live ? __builtin_amdgcn_readfirstlane(s_rowp[end]) : 0) << (8 * j);
                ds[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (F::kScaled)                   // the scales of the rows 4 g .. 4 g + 3 of the tile: this lane's accumulator entries
                    if (live) ds[j] = *reinterpret_cast<const float4*>(s_ds + rb + 16 * j + 4 * g);
                if (KB > 0) {
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb)
                        a[j][kb] = live ? F::load_row(arow + 16 * j * stride + 4 * FB * kb, asc + 16 * j * fsb + 4 * kb, g, kDenseWholeRow) : zero;
                }
            }
            const int last = (rb + WR < n_rows ? rb + WR : n_rows) - 1;
            const int pf = (int)(tf & 255u), pl = __builtin_amdgcn_readfirstlane(s_rowp[last]);
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
                    int on = RT == 1;                      // (wave-uniform) bit j: tile j holds a row of the run; a wave's only tile always does
                    if constexpr (RT > 1) {
#pragma unroll
                        for (int j = 0; j < RT; ++j) {
                            const int f = (int)(tf >> (8 * j) & 255u), l = (int)(tl >> (8 * j) & 255u);
                            on |= (int)(f <= pb && l >= pa && f <= l) << j;
                        }
                    }
                    if (resident) {
                        if (q != q_res) {
#pragma unroll
                            for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                                for (int kb = 0; kb < KR; ++kb)
                                    bq[tt][kb] = 16 * tt < T ? F::load_q(q_tok(q, 16 * tt + r) + 4 * QFB * kb, q_sc(q, 16 * tt + r) + 4 * kb, g, kDenseWholeRow) : qzero;
                            }
                            q_res = q;
                        }
#pragma unroll
                        for (int tt = 0; tt < 2; ++tt)
                            if (16 * tt < T)
                                dense_tiles<F, KB>(a, bq[tt], arow, stride, asc, fsb, nullptr, nullptr, dim, ds, on, rowp, pa, pb, 16 * tt + r < T, pm,
                                                   TP, 16 * tt + r, g);
                    } else {
                        for (int t0 = 0; t0 < T; t0 += 16) {
                            const unsigned char* qtok = q_tok(q, t0 + r);
                            const unsigned char* qsc = q_sc(q, t0 + r);
                            QFrag bt[KR];
                            if (KB > 0) {
#pragma unroll
                                for (int kb = 0; kb < KB; ++kb) bt[kb] = F::load_q(qtok + 4 * QFB * kb, qsc + 4 * kb, g, kDenseWholeRow);
                            }
                            dense_tiles<F, KB>(a, bt, arow, stride, asc, fsb, qtok, qsc, dim, ds, on, rowp, pa, pb, t0 + r < T, pm, TP, t0 + r, g);
                        }
                    }
                }
                if (owned) pa = pb + 1; else ++ql;
            }
        }
        __syncthreads();                                    // the step's rows, scales and passages are read; the next step overwrites them
    }

    dense_sum_maxima<F>(s_pm, s_off, s_own, qscale, nq, np, G, TP, T, B, owned, p0, q0, N, scores);
}

}  // namespace clb
