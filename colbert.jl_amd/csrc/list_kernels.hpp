// list_kernels.hpp -- re-rank given passages: the candidate set of a query is a pid list the caller hands over (no counterpart
// in the reference; the rescore of a first-stage retriever's results).  One block of int64 pids per batch, row b of stride L
// the list of query b, and one length per query, both in device memory and read in stream order: a captured graph holds
// their ADDRESSES, so the next batch's lists are written into the same buffers and the graph replayed.  Entries are pids as
// search returns them (1-based, pid_offset added), in any order, duplicates allowed.
// Two kernels.  list_mark_kernel takes the place of the centroid-list marking: it sets the bit of every listed passage of
// this handle in the query's row of the slot's candidate bitmap, and the compaction that follows (bitmap_count_kernel /
// bitmap_emit_kernel with the handle's live bitmap as every query's filter word) makes the ascending, de-duplicated
// candidate list without the passages that hold no embeddings -- exactly the list a CLB_FILTER_ALL filter of the same pids
// gives.  list_scores_kernel, behind the exact scores, carries every candidate's score back to the positions it was listed at.
// With list priors (one fp32 value per list position, the additive term of prior_kernels.hpp per query AND passage) a third,
// list_slot_kernel behind the compaction, leaves the lowest list position of every candidate slot: the boost reads the value
// there, so of a duplicate's values the first counts, on every route and in every launch order.
// Nothing here can raise: a length is clamped to 0..L and a pid outside the handle's range is skipped (another shard's pid,
// as filter_mark_kernel<true> skips it); the host route checks both before any device work.
#pragma once
#include "search_kernels.hpp"

namespace clb {

// the length of query b's list as the kernels read it
__device__ __forceinline__ int list_len(const int64_t* __restrict__ lens, int b, int L) {
    const int64_t n = lens[b];
    return n < 0 ? 0 : n > (int64_t)L ? L : (int)n;
}
// the local 0-based passage of a listed pid, or -1 when the pid is not this handle's (pid > pid_offset >= 0: no overflow)
__device__ __forceinline__ int list_local(int64_t pid, int64_t pid_offset, int n_docs) {
    return pid > pid_offset && pid - pid_offset <= (int64_t)n_docs ? (int)(pid - pid_offset - 1) : -1;
}

// L1: one thread per list position.  bitmap: the rows of the launch's queries ([B][W]), zero on entry -- bitmap_emit_kernel
// clears every word that was marked.  A list is a few thousand entries: their atomics are nothing beside the 1.25 M of an IVF
// marking that mark_count_kernel exists to avoid.  grid = (ceil(L / 256), B), block = 256.
static __global__ __launch_bounds__(256) void list_mark_kernel(const int64_t* __restrict__ pids, const int64_t* __restrict__ lens,
                                                               int L, int64_t pid_offset, int n_docs,
                                                               uint32_t* __restrict__ bitmap, int W) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= list_len(lens, b, L)) return;
    const int p = list_local(pids[(size_t)b * L + i], pid_offset, n_docs);
    if (p < 0) return;
    atomicOr(&bitmap[(size_t)b * W + (p >> 5)], 1u << (p & 31));
}

// the slot of local passage p among a query's n ascending candidates c, or -1
__device__ __forceinline__ int list_slot(const uint32_t* __restrict__ c, int n, int p) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (c[mid] < (uint32_t)p) lo = mid + 1; else hi = mid;
    }
    return lo < n && c[lo] == (uint32_t)p ? lo : -1;
}
// the number of candidate slots of query b as the kernels read it
__device__ __forceinline__ int list_ncand(const int* __restrict__ ncand, int b, size_t cand_cap) {
    return (int)min((size_t)max(ncand[b], 0), cand_cap);
}

// L2: one thread per list position, behind the exact scores of ALL candidates (with a prior: the boosted ones).  The
// candidates of a query are an ascending list of local pids (cand, ncand entries): a binary search finds the listed
// passage's slot, whose score goes to out[b][i] -- every occurrence of a duplicate finds the same slot.  -Inf for a position
// past the length, a pid outside the handle's range and a passage that is no candidate (it holds no embeddings).
// grid = (ceil(L / 256), B), block = 256.
static __global__ __launch_bounds__(256) void list_scores_kernel(const int64_t* __restrict__ pids, const int64_t* __restrict__ lens,
                                                                 int L, int64_t pid_offset, int n_docs,
                                                                 const uint32_t* __restrict__ cand, const int* __restrict__ ncand,
                                                                 const float* __restrict__ scores, size_t cand_cap,
                                                                 float* __restrict__ out) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L) return;
    float v = kNegInf;
    if (i < list_len(lens, b, L)) {
        const int p = list_local(pids[(size_t)b * L + i], pid_offset, n_docs);
        if (p >= 0) {
            const int slot = list_slot(cand + (size_t)b * cand_cap, list_ncand(ncand, b, cand_cap), p);
            if (slot >= 0) v = scores[(size_t)b * cand_cap + slot];
        }
    }
    out[(size_t)b * L + i] = v;
}

// the fill in front of L3: slot_pos[i] = INT_MAX ("no position yet") for the n words the launch's queries can reach.  A
// kernel, like fill_pad_kernel, not a memset: it is ordered against its neighbours like every other launch of the search,
// on a stream and as a node of a captured graph.  grid = ceil(n / 256), block = 256.
static __global__ __launch_bounds__(256) void list_slot_fill_kernel(int* __restrict__ slot_pos, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) slot_pos[i] = 0x7fffffff;
}

// L3 (list priors): one thread per list position, behind the compaction.  slot_pos[b][slot] (row stride pos_stride, INT_MAX
// on entry) becomes the LOWEST position i < len that lists the slot's passage: the position whose value is the passage's
// term.  Every candidate came from the list, so every slot receives a position; a position past the length, a pid outside
// the handle's range and a passage that is no candidate touch nothing -- their values are never read.  A slot index at or
// past pos_stride cannot arise (a listed query has at most min(L, n_docs) candidates) and is skipped.
// grid = (ceil(L / 256), B), block = 256.
static __global__ __launch_bounds__(256) void list_slot_kernel(const int64_t* __restrict__ pids, const int64_t* __restrict__ lens,
                                                               int L, int64_t pid_offset, int n_docs,
                                                               const uint32_t* __restrict__ cand, const int* __restrict__ ncand,
                                                               size_t cand_cap, int* __restrict__ slot_pos, size_t pos_stride) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= list_len(lens, b, L)) return;
    const int p = list_local(pids[(size_t)b * L + i], pid_offset, n_docs);
    if (p < 0) return;
    const int slot = list_slot(cand + (size_t)b * cand_cap, list_ncand(ncand, b, cand_cap), p);
    if (slot < 0 || (size_t)slot >= pos_stride) return;
    atomicMin(&slot_pos[(size_t)b * pos_stride + slot], i);
}

}  // namespace clb
