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
            const uint32_t* c = cand + (size_t)b * cand_cap;
            int lo = 0, hi = (int)min((size_t)max(ncand[b], 0), cand_cap);
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (c[mid] < (uint32_t)p) lo = mid + 1; else hi = mid;
            }
            const int n = (int)min((size_t)max(ncand[b], 0), cand_cap);
            if (lo < n && c[lo] == (uint32_t)p) v = scores[(size_t)b * cand_cap + lo];
        }
    }
    out[(size_t)b * L + i] = v;
}

}  // namespace clb
