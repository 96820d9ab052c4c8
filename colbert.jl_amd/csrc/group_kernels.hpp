// group_kernels.hpp -- grouped search: rank documents by their best passage (no counterpart in the reference; the
// "collapse" of Elasticsearch / Vespa).  A grouping maps every local passage to the dense 0-based index of its group,
// non-decreasing in pid, so the passages of one group are consecutive pids -- and, the candidates of a query being an
// ascending pid list (bitmap_emit_kernel), consecutive entries of every candidate list.  "Best passage per group" is
// therefore a run reduction over that list: no sort, no hash, no atomics.
#pragma once
#include "search_kernels.hpp"

namespace clb {

constexpr int kGroupChunk = 8;                      // entries a thread owns per tile
constexpr int kGroupTile = 1024 * kGroupChunk;      // entries of one tile of the collapse

// S7g-a.  The run reduction of ONE query per work-group.  The entries are the query's `nlist[b]` listed slots (two-pass
// mode after the selection) or, with list == nullptr, its ncand[b] candidate slots 0, 1, ...; the group of an entry is
// gid[cand[slot]].  Slots ascend with the entry, pids with the slot, groups with the pid: equal groups are one run.
// For every run, in run order, glist[b][r] = the slot of the run's largest score, the FIRST such entry among equal
// scores (scores compare by their order key, as the top-k kernels compare them), and nglist[b] = the number of runs.
//
// An entry travels as one 64-bit word, order key << 32 | ~slot: the larger word is the better score and, among equal
// scores, the lower slot = the earlier entry; 0 is "nothing" (no slot is 2^32 - 1).  Combining two stretches of a run is
// then max().  Tiles of kGroupTile entries; in a tile thread t owns the `chunk` consecutive entries from t * chunk on
// (chunk = kGroupChunk in a full tile, the last tile spreads what is left over all threads):
//   1. it loads them and publishes the group of its last entry; an entry is a HEAD when its group differs from the
//      entry before it (for a thread's first entry: its left neighbour's last, for the tile's first entry: the last
//      of the tile before);
//   2. it reduces its chunk in registers to (number of heads, best of the stretch behind its last head -- the whole
//      chunk when it has none); a block-wide scan of the counts gives the index of every run, a block-wide SEGMENTED
//      max-scan of the stretches (a head cuts the carry) gives every thread the best of the open run as it reaches its
//      first entry.  Both scans: shuffles inside a wave, one LDS word per wave across the sixteen waves;
//   3. it walks its chunk again from that carry: at every head the run that ends there is final and its slot is stored.
// The run open at the end of a tile is carried into the next one in registers (every thread computes the same value);
// the last run is written after the last tile.  Writes: one word per RUN.  grid = B, block = 1024.
static __global__ __launch_bounds__(1024) void group_collapse_kernel(const float* __restrict__ scores,
                                                                    const uint32_t* __restrict__ cand,
                                                                    const int* __restrict__ ncand,
                                                                    const int* __restrict__ list /*optional*/,
                                                                    const int* __restrict__ nlist,
                                                                    const uint32_t* __restrict__ gid, size_t cand_cap,
                                                                    int* __restrict__ glist, int* __restrict__ nglist) {
    __shared__ uint32_t sh_last[1024];                 // group of every thread's last entry
    __shared__ unsigned long long sh_v[16];            // per wave: the stretch behind the wave's last head
    __shared__ int sh_f[16], sh_c[16];                 // per wave: has a head / number of heads
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = list ? nlist[b] : ncand[b];
    const float* sc = scores + (size_t)b * cand_cap;
    const uint32_t* cnd = cand + (size_t)b * cand_cap;
    const int* lst = list ? list + (size_t)b * cand_cap : nullptr;
    int* out = glist + (size_t)b * cand_cap;
    constexpr uint32_t kNoGroup = 0xffffffffu;         // a group index is below n_docs < 2^31
    unsigned long long carry = 0ull;                   // best of the run open at the tile's start (uniform)
    uint32_t prev_tile = kNoGroup;                     // group of the entry before the tile (read by thread 0 only)
    int nruns = 0;                                     // heads so far (uniform)
    for (int base = 0; base < n; base += kGroupTile) {
        const int left = n - base;
        const int chunk = left >= kGroupTile ? kGroupChunk : (left + 1023) >> 10;     // uniform
        const int i0 = base + tid * chunk;
        unsigned long long e[kGroupChunk];
        uint32_t g[kGroupChunk];
#pragma unroll
        for (int c = 0; c < kGroupChunk; ++c) {
            const int i = i0 + c;
            const bool valid = c < chunk && i < n;
            const int slot = valid ? (lst ? lst[i] : i) : 0;
            g[c] = valid ? gid[cnd[slot]] : kNoGroup;
            e[c] = valid ? ((unsigned long long)f32_order_key(sc[slot]) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)slot)
                         : 0ull;
        }
        // the group of the thread's last valid entry (valid entries are a prefix of the chunk, and of the tile)
        uint32_t last = kNoGroup;
#pragma unroll
        for (int c = 0; c < kGroupChunk; ++c) last = g[c] != kNoGroup ? g[c] : last;
        sh_last[tid] = last;
        __syncthreads();
        uint32_t prev = tid > 0 ? sh_last[tid - 1] : prev_tile;
        if (tid == 0) prev_tile = sh_last[1023];       // only a full tile has a successor
        // 2. heads, and the stretch behind the last head
        uint32_t heads = 0u;                           // bit c: entry c is a head
        unsigned long long tail = 0ull;
#pragma unroll
        for (int c = 0; c < kGroupChunk; ++c) {
            const bool valid = g[c] != kNoGroup;
            const bool head = valid && g[c] != prev;
            heads |= head ? (1u << c) : 0u;
            tail = head ? e[c] : (e[c] > tail ? e[c] : tail);      // an invalid entry is 0: it changes nothing
            prev = valid ? g[c] : prev;
        }
        const int nh = __popc(heads);
        int xc = nh, xf = nh > 0;
        unsigned long long xv = tail;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int yc = __shfl_up(xc, o, 64), yf = __shfl_up(xf, o, 64);
            const unsigned long long yv = __shfl_up(xv, o, 64);
            if (lane >= o) {
                xc += yc;
                if (!xf) xv = yv > xv ? yv : xv;       // no head up to here: the stretch reaches further left
                xf |= yf;
            }
        }
        if (lane == 63) { sh_c[wave] = xc; sh_f[wave] = xf; sh_v[wave] = xv; }
        // what the lanes before this one leave open, inside the wave
        int ef = __shfl_up(xf, 1, 64);
        unsigned long long ev = __shfl_up(xv, 1, 64);
        if (lane == 0) { ef = 0; ev = 0ull; }
        __syncthreads();
        int runs_before = nruns + xc - nh;             // heads before this thread's first entry
        unsigned long long open = carry;               // the open run as the thread's wave begins ...
        unsigned long long open_all = carry;
        int heads_all = 0;
        for (int w2 = 0; w2 < 16; ++w2) {
            const unsigned long long v = sh_v[w2];
            open_all = sh_f[w2] ? v : (v > open_all ? v : open_all);
            heads_all += sh_c[w2];
            if (w2 + 1 == wave) open = open_all;
            if (w2 < wave) runs_before += sh_c[w2];
        }
        unsigned long long acc = ef ? ev : (ev > open ? ev : open);    // ... and as the thread itself does
        // 3. the runs that end inside the chunk
        int r = runs_before - 1;                       // index of the open run (-1: the list begins here)
#pragma unroll
        for (int c = 0; c < kGroupChunk; ++c) {
            if ((heads >> c) & 1u) {
                if (r >= 0) out[r] = (int)(0xffffffffu - (uint32_t)(acc & 0xffffffffull));
                ++r;
                acc = e[c];
            } else {
                acc = e[c] > acc ? e[c] : acc;
            }
        }
        carry = open_all;
        nruns += heads_all;
    }
    if (tid == 0) {
        if (nruns > 0) out[nruns - 1] = (int)(0xffffffffu - (uint32_t)(carry & 0xffffffffull));
        nglist[b] = nruns;
    }
}

// S7g-b.  tau_g[b] = a lower bound, to 2^-16 of the key range, of the k-th largest of scores[glist[b][i]], i < nglist[b]
// (the k-th best GROUP by approximate score), -inf when the query has fewer than k groups: the external threshold the
// unchanged selection kernels cut at (select_margin_kernel / wide_* with tau_in).  Any lower bound of the k-th value
// keeps the proof of the two-pass mode -- it only lists more (select_margin_kernel's coarse_tau).  grid = B, block = 1024.
static __global__ __launch_bounds__(1024) void group_tau_kernel(const float* __restrict__ scores,
                                                               const int* __restrict__ glist,
                                                               const int* __restrict__ nglist, int k, size_t cand_cap,
                                                               float* __restrict__ tau_g) {
    __shared__ __attribute__((aligned(16))) int hist[256];
    __shared__ uint32_t s_prefix, s_kmin, s_kmax;
    __shared__ int s_remaining;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = nglist[b];
    if (n < k) {                                       // uniform over the block
        if (tid == 0) tau_g[b] = kNegInf;
        return;
    }
    const float* sc = scores + (size_t)b * cand_cap;
    const int* lst = glist + (size_t)b * cand_cap;
    const int chunk = (n + 1023) >> 10;
#define CLB_SEL_FOR_EACH(...)                                                                   \
    for (int c = 0; c < chunk; ++c) {                                                           \
        const int i_ = c * 1024 + tid;                                                          \
        const bool valid = i_ < n;                                                              \
        const uint32_t key = valid ? f32_order_key(sc[lst[i_]]) : 0u;                           \
        __VA_ARGS__                                                                             \
    }
    if (tid == 0) { s_prefix = 0u; s_remaining = k; }
    __syncthreads();
    CLB_RADIX_SELECT_N(2)
#undef CLB_SEL_FOR_EACH
    if (tid == 0) tau_g[b] = f32_from_order_key(s_prefix);
}

// ---- load time: the dense group index of every passage from the caller's ids -----------------------------------------
// flag[i] = 1 where passage i begins a group (ids[i] != ids[i - 1]), 0 for passage 0: the library's exclusive scan over
// n + 1 inputs (flag[n] = 0 is the pad slot it reads) leaves the sums of flag[0 .. i - 1]; the group of passage i is that
// sum plus flag[i], and the number of groups is 1 + the total (n > 0).
static __global__ __launch_bounds__(256) void grouping_flags_kernel(const int64_t* __restrict__ ids, int64_t n,
                                                                   uint32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    flag[i] = (i > 0 && i < n && ids[i] != ids[i - 1]) ? 1u : 0u;
}
static __global__ __launch_bounds__(256) void grouping_index_kernel(const uint32_t* __restrict__ flag,
                                                                   const uint32_t* __restrict__ before, int64_t n,
                                                                   uint32_t* __restrict__ gid) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) gid[i] = before[i] + flag[i];
}

}  // namespace clb
