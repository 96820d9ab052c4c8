// remove_kernels.hpp -- device side of clb_searcher_remove (search.hip): the rows and the inverted lists of a reduced index
// are the old ones with the removed passages' entries taken out, everything else in its old order.  No counterpart in the
// reference (its index is built once; upstream ColBERT: IndexUpdater.remove).  The set of removed passages arrives as a
// passage bitmap in the layout of a clb_filter (filter_mark_kernel, search_kernels.hpp): a SET bit means removed.
#pragma once
#include "common.hpp"

namespace clb {

__device__ __forceinline__ bool removed_bit(const uint32_t* __restrict__ bits, uint32_t p) { return (bits[p >> 5] >> (p & 31)) & 1u; }

// what the host reads back of the new passage lengths, in one copy
struct RemoveCounts {
    uint32_t removed;   // passages that lose at least one embedding
    uint32_t longest;   // the longest passage that stays
};

// len[p] = removed(p) ? 0 : doc_off[p + 1] - doc_off[p], p = 0 .. n_docs - 1, and len[n_docs] = 0 (the scan's pad).
// One atomic per wave and counter: the wave's sum / maximum first.
static __global__ __launch_bounds__(256) void remove_lengths_kernel(const uint32_t* __restrict__ doc_off,
                                                                   const uint32_t* __restrict__ bits, int n_docs,
                                                                   uint32_t* __restrict__ len, RemoveCounts* __restrict__ counts) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    uint32_t gone = 0, keep = 0;
    if (p < n_docs) {
        const uint32_t l = doc_off[p + 1] - doc_off[p];
        if (removed_bit(bits, (uint32_t)p)) gone = l > 0; else keep = l;
        len[p] = keep;
    } else if (p == n_docs) {
        len[p] = 0;
    }
    for (int d = 32; d > 0; d >>= 1) {
        gone += __shfl_xor(gone, d);
        keep = max(keep, (uint32_t)__shfl_xor(keep, d));
    }
    if ((threadIdx.x & 63) == 0) {
        if (gone) atomicAdd(&counts->removed, gone);
        if (keep) atomicMax(&counts->longest, keep);
    }
}

// The rows.  A flat grid over the OUTPUT rows: row j of the reduced index belongs to the passage p with new_off[p] <= j <
// new_off[p + 1] (the LAST p with new_off[p] <= j: the empty passages in front of it share its offset) and is the old row
// old_off[p] + (j - new_off[p]): rows keep their order inside a passage, so create's per-passage code order survives.  A tile
// of kRemoveTile rows finds the passages of its first and last row once (two full binary searches in new_off, as
// ivf_merge_kernel does in the list offsets) and every row then searches between those two; the source rows of the tile are
// kept in LDS.  The residual rows are then copied as ONE run of pieces per tile: consecutive lanes write consecutive pieces
// (Piece = 16 bytes on the tuned path, where a row is 16 * nbits bytes; 4 or 1 byte for the general path's other sizes).
// Every output row is written exactly once; the zero padding behind the last row is the host's (alloc_padded_rows).
// grid = min(tiles, any cap), block = 256; tiles are taken grid-stride.
constexpr int kRemoveItems = 8;
constexpr int kRemoveTile = 256 * kRemoveItems;

template <class Piece>
static __global__ __launch_bounds__(256) void remove_rows_kernel(const uint32_t* __restrict__ old_off,
                                                                const uint32_t* __restrict__ new_off, int n_docs,
                                                                int64_t n_rows, const uint32_t* __restrict__ codes_src,
                                                                const Piece* __restrict__ res_src, int pieces,
                                                                uint32_t* __restrict__ codes_dst, Piece* __restrict__ res_dst) {
    __shared__ int s_p[2];
    __shared__ uint32_t s_src[kRemoveTile];
    const int64_t tiles = (n_rows + kRemoveTile - 1) / kRemoveTile;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t j0 = tile * kRemoveTile;
        const int64_t j1 = (j0 + kRemoveTile < n_rows ? j0 + kRemoveTile : n_rows) - 1;
        if (threadIdx.x < 2) {
            const int64_t j = threadIdx.x == 0 ? j0 : j1;
            int lo = 0, hi = n_docs;      // new_off[lo] <= j < new_off[hi]  (new_off[0] = 0, new_off[n_docs] = n_rows)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)new_off[mid] <= j) lo = mid; else hi = mid;
            }
            s_p[threadIdx.x] = lo;
        }
        __syncthreads();
        const int p_lo = s_p[0], p_hi = s_p[1];
#pragma unroll
        for (int i = 0; i < kRemoveItems; ++i) {
            const int r = i * 256 + threadIdx.x;
            const int64_t j = j0 + r;
            if (j > j1) break;
            int lo = p_lo, hi = p_hi + 1;       // new_off[p_lo] <= j0 <= j <= j1 < new_off[p_hi + 1]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)new_off[mid] <= j) lo = mid; else hi = mid;
            }
            const uint32_t src = old_off[lo] + ((uint32_t)j - new_off[lo]);
            s_src[r] = src;
            codes_dst[j] = codes_src[src];
        }
        __syncthreads();
        const int n_pieces = (int)(j1 - j0 + 1) * pieces;       // at most 2048 rows of at most dim / 8 * 8 bytes
        Piece* dst = res_dst + (size_t)j0 * pieces;
        for (int i = threadIdx.x; i < n_pieces; i += 256) {
            const int r = i / pieces;
            dst[i] = res_src[(size_t)s_src[r] * pieces + (i - r * pieces)];
        }
        __syncthreads();        // s_p and s_src are rewritten by the next tile
    }
}

// The inverted lists.  flag[j] = 1 when entry j's passage stays, j = 0 .. n - 1, and flag[n] = 0 (the scan's pad) ...
static __global__ __launch_bounds__(256) void ivf_keep_flags_kernel(const uint32_t* __restrict__ ivf_pid,
                                                                   const uint32_t* __restrict__ bits, int64_t n,
                                                                   uint32_t* __restrict__ flag) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) flag[j] = removed_bit(bits, ivf_pid[j]) ? 0u : 1u;
    else if (j == n) flag[j] = 0u;
}
// ... pos = the exclusive scan of flag (n + 1 entries, pos[n] = the entries that stay): a kept entry moves to pos[j].  The
// order of the kept entries is unchanged, inside every list and across the lists: no sort.
static __global__ __launch_bounds__(256) void ivf_compact_kernel(const uint32_t* __restrict__ ivf_pid,
                                                                const uint32_t* __restrict__ pos, int64_t n,
                                                                uint32_t* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t at = pos[j];
    if (pos[j + 1] != at) out[at] = ivf_pid[j];
}
// new_off[c] = pos[old_off[c]], c = 0 .. K: the kept entries in front of list c
static __global__ void ivf_compact_offsets_kernel(const uint32_t* __restrict__ old_off, const uint32_t* __restrict__ pos,
                                                  int n, uint32_t* __restrict__ new_off) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) new_off[c] = pos[old_off[c]];
}

}  // namespace clb
