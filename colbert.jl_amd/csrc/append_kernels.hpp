// append_kernels.hpp -- device side of clb_searcher_append (search.hip): the inverted lists of a grown index are the old
// lists with the new passages' entries behind them, list by list.  No counterpart in the reference (its index is built once:
// _build_ivf, collection_indexer.jl:349-353, is what the merged lists must equal).
#pragma once
#include "common.hpp"

namespace clb {

// Per NEW embedding e (0-based among the appended ones, codes already 0-based and checked): its local passage id, by binary
// search in the appended passages' own offsets `off` (n_new + 1 entries, off[0] = 0) plus pid_base = the passages the handle
// held before, and one count in the histogram of the new codes.  hist has K + 1 entries, zeroed (the scan wants the pad).
static __global__ __launch_bounds__(256) void append_hist_pid_kernel(const uint32_t* __restrict__ codes0,
                                                                    const uint32_t* __restrict__ off, int64_t n_emb,
                                                                    int n_new, uint32_t pid_base,
                                                                    uint32_t* __restrict__ hist, uint32_t* __restrict__ pids) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_emb) return;
    int lo = 0, hi = n_new;  // largest p with off[p] <= e
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)off[mid] <= e) lo = mid; else hi = mid;
    }
    pids[e] = pid_base + (uint32_t)lo;
    atomicAdd(&hist[codes0[e]], 1u);
}

// new_off[c] = old_off[c] + add_off[c], c = 0 .. K: where list c starts in the merged array
static __global__ void append_offsets_kernel(const uint32_t* __restrict__ old_off, const uint32_t* __restrict__ add_off,
                                             int n, uint32_t* __restrict__ new_off) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) new_off[c] = old_off[c] + add_off[c];
}

// The merge.  A flat grid over the OUTPUT: entry j of the merged array belongs to the list c with new_off[c] <= j <
// new_off[c + 1]; at rank r = j - new_off[c] it is old entry old_off[c] + r while r is below the old length, and entry
// add_off[c] + r - old_len of the (code, embedding)-sorted new entries after that.  Every output is written exactly once,
// consecutive lanes write consecutive words and -- inside a list segment -- read consecutive words; an empty old or new
// segment is never visited because no j maps to it.  A tile of kMergeTile outputs finds the lists of its first and last
// entry once (two full binary searches in new_off, K + 1 words that stay in L2) and every entry then searches only between
// those two: at 1 M passages a list holds ~900 entries, so a tile spans two or three lists and the per-entry search is one or
// two steps.  Work per tile is equal whatever the list lengths are, which a wave-per-list mapping cannot give on a topical
// index (lengths from 0 to tens of thousands) or for a small append (K waves launched to move a few entries each).
// grid = min(tiles, any cap), block = 256; tiles are taken grid-stride.
constexpr int kMergeItems = 8;
constexpr int kMergeTile = 256 * kMergeItems;

static __global__ __launch_bounds__(256) void ivf_merge_kernel(const uint32_t* __restrict__ old_off,
                                                              const uint32_t* __restrict__ add_off,
                                                              const uint32_t* __restrict__ new_off,
                                                              const uint32_t* __restrict__ old_pid,
                                                              const uint32_t* __restrict__ add_pid, int K, int64_t n_total,
                                                              uint32_t* __restrict__ out) {
    __shared__ int s_c[2];
    const int64_t tiles = (n_total + kMergeTile - 1) / kMergeTile;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t j0 = tile * kMergeTile;
        const int64_t j1 = (j0 + kMergeTile < n_total ? j0 + kMergeTile : n_total) - 1;
        if (threadIdx.x < 2) {
            const int64_t j = threadIdx.x == 0 ? j0 : j1;
            int lo = 0, hi = K;      // new_off[lo] <= j < new_off[hi]  (new_off[0] = 0, new_off[K] = n_total)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)new_off[mid] <= j) lo = mid; else hi = mid;
            }
            s_c[threadIdx.x] = lo;
        }
        __syncthreads();
        const int c_lo = s_c[0], c_hi = s_c[1];
#pragma unroll
        for (int i = 0; i < kMergeItems; ++i) {
            const int64_t j = j0 + (int64_t)i * 256 + threadIdx.x;
            if (j > j1) break;
            int lo = c_lo, hi = c_hi + 1;       // new_off[c_lo] <= j0 <= j <= j1 < new_off[c_hi + 1]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)new_off[mid] <= j) lo = mid; else hi = mid;
            }
            const uint32_t r = (uint32_t)j - new_off[lo];
            const uint32_t o0 = old_off[lo], old_len = old_off[lo + 1] - o0;
            out[j] = r < old_len ? old_pid[o0 + r] : add_pid[add_off[lo] + (r - old_len)];
        }
        __syncthreads();        // s_c is rewritten by the next tile
    }
}

}  // namespace clb
