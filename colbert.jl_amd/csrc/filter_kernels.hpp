// filter_kernels.hpp -- composing filters on the device (S3f; no counterpart in the reference: its filter_fn is a host
// closure).  A clb_filter is one bitmap, ceil(n_docs / 32) u32 words, bit i of word j = local passage 32 j + i.  The three
// kernels here write the words of a FRESH bitmap from operands that are already resident -- other filters (set algebra), a
// clb_prior (an attribute range), an older filter (its extension after an append) -- and leave the tail bits and the
// population to filter_count_kernel (search_kernels.hpp), which every way of making a filter ends in.
// Each moves at most (operands + 1) n_docs / 8 bytes, 4 n_docs for the range: at a million passages the launch and the one
// read-back of the count are the whole cost, so accesses are coalesced and nothing else is done about speed.
#pragma once
#include "common.hpp"

namespace clb {

// The operand words of filter_combine_kernel, by value in the kernel arguments as FilterArgs carries the handles of a search:
// no table on the device, no upload.  Entries n .. are unused.
struct FilterOperands {
    const uint32_t* bits[CLB_MAX_FILTER_OPERANDS];
    int n;
};

// Set algebra, one lane per output word w < W: AND / OR over all operands, ANDNOT operand 0 minus the union of the others,
// NOT the complement of operand 0.  NOT sets the bits past n_docs in the last word: filter_count_kernel clears them.
// An operand may be named more than once, and may be in use by searches in flight: operands are only read, `out` is no
// operand.  grid = ceil(W / 256), block = 256.
static __global__ __launch_bounds__(256) void filter_combine_kernel(FilterOperands ops, int op, int W, uint32_t* __restrict__ out) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= W) return;
    uint32_t x = ops.bits[0][w];
    if (op == CLB_FILTER_OP_NOT) {
        x = ~x;
    } else if (op == CLB_FILTER_OP_AND) {
        for (int i = 1; i < ops.n; ++i) x &= ops.bits[i][w];
    } else {
        uint32_t rest = 0;
        for (int i = 1; i < ops.n; ++i) rest |= ops.bits[i][w];
        x = op == CLB_FILTER_OP_OR ? (x | rest) : (x & ~rest);
    }
    out[w] = x;
}

// An attribute range, one lane per passage: passage p is in when (lo_open ? v > lo : v >= lo) && (hi_open ? v < hi : v <= hi)
// for its value v, IEEE comparisons on the stored fp32 (-0 equals +0; a prior holds no NaN).  A lane past n_docs votes false.
// The 64 votes of a wave are words 2 g and 2 g + 1 of the bitmap (g the wave's index in the grid); lane 0 stores them, the
// second only where it exists (W may be odd).  Waves own disjoint words: no atomics.  grid = ceil(n_docs / 256), block = 256.
static __global__ __launch_bounds__(256) void filter_range_kernel(const float* __restrict__ values, int n_docs, float lo, float hi,
                                                                  int lo_open, int hi_open, int W, uint32_t* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool in = false;
    if (p < (int64_t)n_docs) {
        const float v = values[p];
        in = (lo_open ? v > lo : v >= lo) && (hi_open ? v < hi : v <= hi);
    }
    const unsigned long long votes = __ballot(in);
    if ((threadIdx.x & 63) == 0) {
        const int64_t w = p >> 5;            // p is a multiple of 64 here
        if (w < W) out[w] = (uint32_t)votes;
        if (w + 1 < W) out[w + 1] = (uint32_t)(votes >> 32);
    }
}

// A filter of n_old passages as one of n_new >= n_old, one lane per word w < W_new of the NEW bitmap: the words wholly below
// n_old are copied, the word that holds passage n_old keeps its bits below it and takes `fill` (0 or ~0) above, later words
// are `fill`.  (The old bitmap has no bit past n_old, but that is not relied on.)  grid = ceil(W_new / 256), block = 256.
static __global__ __launch_bounds__(256) void filter_extend_kernel(const uint32_t* __restrict__ old_bits, int n_old, uint32_t fill,
                                                                   int W_new, uint32_t* __restrict__ out) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= W_new) return;
    const int full = n_old >> 5, rem = n_old & 31;      // whole old words; old passages in the word after them
    uint32_t x = fill;
    if (w < full) {
        x = old_bits[w];
    } else if (w == full && rem) {
        const uint32_t low = (1u << rem) - 1u;
        x = (old_bits[w] & low) | (fill & ~low);
    }
    out[w] = x;
}

}  // namespace clb
