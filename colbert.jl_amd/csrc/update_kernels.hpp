// update_kernels.hpp -- device side of clb_searcher_update (search.hip): the rows and the inverted lists of an index in which
// some passages have new content are the old ones with those passages' entries taken out and the new entries put where a
// fresh build of the changed index would put them.  No counterpart in the reference (its index is built once); upstream
// ColBERT's IndexUpdater has remove and add only.  The set of replaced passages arrives as a passage bitmap in the layout
// of a clb_filter (filter_mark_kernel, search_kernels.hpp; read with removed_bit, remove_kernels.hpp): a SET bit means
// replaced.  Beside it stands slot[p], read only where the bit is set: the position of passage p in the caller's list, whose
// new rows are stage_off[slot] .. stage_off[slot + 1] - 1 of the staged new rows.
#pragma once
#include "common.hpp"
#include "remove_kernels.hpp"

namespace clb {

// slot[pids[i] - pid_offset - 1] = i.  The host has refused pids outside the handle and pids named twice: every word is
// written by one thread; the range is checked again because the word is an address.
static __global__ __launch_bounds__(256) void update_slots_kernel(const int64_t* __restrict__ pids, int64_t n, int64_t pid_offset,
                                                                  int n_docs, uint32_t* __restrict__ slot) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pids[i] - pid_offset - 1;
    if (p >= 0 && p < (int64_t)n_docs) slot[p] = (uint32_t)i;
}

// what the host reads back of the new passage lengths, in one copy
struct UpdateCounts {
    uint32_t changed;               // replaced passages whose old or new length is not zero
    uint32_t longest;               // the longest passage of the changed index
    unsigned long long dropped;     // the rows the replaced passages held before
};

// len[p] = replaced(p) ? the new length : doc_off[p + 1] - doc_off[p], p = 0 .. n_docs - 1, and len[n_docs] = 0 (the scan's
// pad).  One atomic per wave and counter: the wave's sum / maximum first.
static __global__ __launch_bounds__(256) void update_lengths_kernel(const uint32_t* __restrict__ doc_off,
                                                                    const uint32_t* __restrict__ bits,
                                                                    const uint32_t* __restrict__ slot,
                                                                    const uint32_t* __restrict__ stage_off, int n_docs,
                                                                    uint32_t* __restrict__ len, UpdateCounts* __restrict__ counts) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    uint32_t changed = 0, longest = 0, dropped = 0;
    if (p < n_docs) {
        longest = doc_off[p + 1] - doc_off[p];
        if (removed_bit(bits, (uint32_t)p)) {
            const uint32_t i = slot[p];
            dropped = longest;
            longest = stage_off[i + 1] - stage_off[i];
            changed = (dropped | longest) != 0;
        }
        len[p] = longest;
    } else if (p == n_docs) {
        len[p] = 0;
    }
    unsigned long long dropped_wave = dropped;
    for (int d = 32; d > 0; d >>= 1) {
        changed += __shfl_xor(changed, d);
        longest = max(longest, (uint32_t)__shfl_xor(longest, d));
        dropped_wave += __shfl_xor(dropped_wave, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (changed) atomicAdd(&counts->changed, changed);
        if (longest) atomicMax(&counts->longest, longest);
        if (dropped_wave) atomicAdd(&counts->dropped, dropped_wave);
    }
}

// The rows.  A flat grid over the OUTPUT rows, tiled and searched exactly as remove_rows_kernel does: row j of the changed
// index belongs to the LAST passage p with new_off[p] <= j, at rank r = j - new_off[p] inside it.  Its source is staged row
// stage_off[slot[p]] + r when p is replaced -- the staging buffer holds the new rows in create's per-passage code order on the
// tuned path, as given on the general path -- and old row old_off[p] + r when it is not: a kept passage keeps its rows in
// their order.  The tile's sources go to LDS (s_src: the row; s_new: one bit per row of the tile, set = staged) and the
// residual rows are copied as ONE run of pieces per tile, consecutive lanes writing consecutive pieces (Piece as in
// remove_rows_kernel).  Every output row is written exactly once; the zero padding behind the last row is the host's
// (alloc_padded_rows).  grid = min(tiles, any cap), block = 256; tiles are taken grid-stride.
constexpr int kSpliceItems = 8;
constexpr int kSpliceTile = 256 * kSpliceItems;

template <class Piece>
static __global__ __launch_bounds__(256) void splice_rows_kernel(
    const uint32_t* __restrict__ old_off, const uint32_t* __restrict__ new_off, const uint32_t* __restrict__ bits,
    const uint32_t* __restrict__ slot, const uint32_t* __restrict__ stage_off, int n_docs, int64_t n_rows,
    const uint32_t* __restrict__ codes_old, const Piece* __restrict__ res_old, const uint32_t* __restrict__ codes_stage,
    const Piece* __restrict__ res_stage, int pieces, uint32_t* __restrict__ codes_dst, Piece* __restrict__ res_dst) {
    __shared__ int s_p[2];
    __shared__ uint32_t s_src[kSpliceTile];
    __shared__ uint32_t s_new[kSpliceTile / 32];
    const int64_t tiles = (n_rows + kSpliceTile - 1) / kSpliceTile;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t j0 = tile * kSpliceTile;
        const int64_t j1 = (j0 + kSpliceTile < n_rows ? j0 + kSpliceTile : n_rows) - 1;
        if (threadIdx.x < 2) {
            const int64_t j = threadIdx.x == 0 ? j0 : j1;
            int lo = 0, hi = n_docs;      // new_off[lo] <= j < new_off[hi]  (new_off[0] = 0, new_off[n_docs] = n_rows)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)new_off[mid] <= j) lo = mid; else hi = mid;
            }
            s_p[threadIdx.x] = lo;
        }
        if (threadIdx.x < kSpliceTile / 32) s_new[threadIdx.x] = 0u;
        __syncthreads();
        const int p_lo = s_p[0], p_hi = s_p[1];
#pragma unroll
        for (int i = 0; i < kSpliceItems; ++i) {
            const int r = i * 256 + threadIdx.x;
            const int64_t j = j0 + r;
            if (j > j1) break;
            int lo = p_lo, hi = p_hi + 1;       // new_off[p_lo] <= j0 <= j <= j1 < new_off[p_hi + 1]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)new_off[mid] <= j) lo = mid; else hi = mid;
            }
            const uint32_t rank = (uint32_t)j - new_off[lo];
            uint32_t src;
            if (removed_bit(bits, (uint32_t)lo)) {
                src = stage_off[slot[lo]] + rank;
                atomicOr(&s_new[r >> 5], 1u << (r & 31));
                codes_dst[j] = codes_stage[src];
            } else {
                src = old_off[lo] + rank;
                codes_dst[j] = codes_old[src];
            }
            s_src[r] = src;
        }
        __syncthreads();
        const int n_pieces = (int)(j1 - j0 + 1) * pieces;       // at most 2048 rows of at most dim / 8 * 8 bytes
        Piece* dst = res_dst + (size_t)j0 * pieces;
        for (int i = threadIdx.x; i < n_pieces; i += 256) {
            const int r = i / pieces;
            const Piece* src = ((s_new[r >> 5] >> (r & 31)) & 1u) ? res_stage : res_old;
            dst[i] = src[(size_t)s_src[r] * pieces + (i - r * pieces)];
        }
        __syncthreads();        // s_p, s_src and s_new are rewritten by the next tile
    }
}

// The inverted lists.  Per NEW embedding e (in the caller's order, codes already 0-based and checked): the local passage it
// belongs to -- the last entry i of the caller's list with stage_off[i] <= e, then pids[i] -- and one count in the histogram
// of the new codes.  hist has K + 1 entries, zeroed (the scan wants the pad).
static __global__ __launch_bounds__(256) void update_hist_pid_kernel(const uint32_t* __restrict__ codes0,
                                                                     const uint32_t* __restrict__ stage_off,
                                                                     const int64_t* __restrict__ pids, int64_t pid_offset,
                                                                     int64_t n_emb, int n, uint32_t* __restrict__ hist,
                                                                     uint32_t* __restrict__ pid_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_emb) return;
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)stage_off[mid] <= e) lo = mid; else hi = mid;
    }
    pid_out[e] = (uint32_t)(pids[lo] - pid_offset - 1);
    atomicAdd(&hist[codes0[e]], 1u);
}

// new_off[c] = pos[old_off[c]] + add_off[c], c = 0 .. K: the kept old entries and the new entries in front of list c
static __global__ void ivf_splice_offsets_kernel(const uint32_t* __restrict__ old_off, const uint32_t* __restrict__ pos,
                                                 const uint32_t* __restrict__ add_off, int n, uint32_t* __restrict__ new_off) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) new_off[c] = pos[old_off[c]] + add_off[c];
}

// The merge, on a handle whose lists hold non-decreasing pids.  A passage is wholly kept or wholly replaced, so no pid comes
// from both sides and the changed list of centroid c is the merge by pid of its kept old entries (pos: the exclusive scan of
// the keep flags, n_old + 1 entries, as in a removal) and the new entries with code c (add_code / add_pid: the new entries
// sorted by (code, pid), n_add of them; add_off: the scan of their histogram).  Every entry computes its own destination:
//   kept old entry j of list c  ->  pos[j] + add_off[c] + |{new entries of c with a smaller pid}|
//   new entry i, of list c      ->  pos[first old entry of list c whose pid is not smaller] + i
// (i counts the new entries of the lists before c and those of c in front of it; pos[..] the kept entries of the lists before
// c and those of c with a smaller pid -- a replaced passage's own old entries are not kept and do not move pos).  A flat grid
// over the n_old old entries, then over the n_add new ones, in tiles of kSpliceTile.  An old tile finds the lists of its
// first and last entry once (two full binary searches in old_off, K + 1 words that stay in L2) and every entry then searches
// between those two; a new entry reads its list from add_code.  The searches by pid run over one list segment each.
// Every output entry is written exactly once.  grid = min(tiles, any cap), block = 256; tiles are taken grid-stride.
static __global__ __launch_bounds__(256) void ivf_splice_kernel(const uint32_t* __restrict__ old_off,
                                                                const uint32_t* __restrict__ old_pid,
                                                                const uint32_t* __restrict__ pos, int64_t n_old,
                                                                const uint32_t* __restrict__ add_off,
                                                                const uint32_t* __restrict__ add_code,
                                                                const uint32_t* __restrict__ add_pid, int64_t n_add, int K,
                                                                uint32_t* __restrict__ out) {
    __shared__ int s_c[2];
    const int64_t tiles_old = (n_old + kSpliceTile - 1) / kSpliceTile;
    const int64_t tiles = tiles_old + (n_add + kSpliceTile - 1) / kSpliceTile;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if (tile >= tiles_old) {        // new entries (the whole block takes this branch)
            const int64_t i0 = (tile - tiles_old) * kSpliceTile;
#pragma unroll
            for (int t = 0; t < kSpliceItems; ++t) {
                const int64_t i = i0 + (int64_t)t * 256 + threadIdx.x;
                if (i >= n_add) break;
                const uint32_t c = add_code[i], pid = add_pid[i];
                uint32_t lo = old_off[c], hi = old_off[c + 1];      // the first entry in [lo, hi) with old_pid >= pid, or hi
                while (lo < hi) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (old_pid[mid] < pid) lo = mid + 1; else hi = mid;
                }
                out[(int64_t)pos[lo] + i] = pid;
            }
            continue;
        }
        const int64_t j0 = tile * kSpliceTile;
        const int64_t j1 = (j0 + kSpliceTile < n_old ? j0 + kSpliceTile : n_old) - 1;
        if (threadIdx.x < 2) {
            const int64_t j = threadIdx.x == 0 ? j0 : j1;
            int lo = 0, hi = K;      // old_off[lo] <= j < old_off[hi]  (old_off[0] = 0, old_off[K] = n_old)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)old_off[mid] <= j) lo = mid; else hi = mid;
            }
            s_c[threadIdx.x] = lo;
        }
        __syncthreads();
        const int c_lo = s_c[0], c_hi = s_c[1];
#pragma unroll
        for (int t = 0; t < kSpliceItems; ++t) {
            const int64_t j = j0 + (int64_t)t * 256 + threadIdx.x;
            if (j > j1) break;
            const uint32_t at = pos[j];
            if (pos[j + 1] == at) continue;     // a replaced passage's entry
            int lo = c_lo, hi = c_hi + 1;       // old_off[c_lo] <= j0 <= j <= j1 < old_off[c_hi + 1]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)old_off[mid] <= j) lo = mid; else hi = mid;
            }
            const uint32_t pid = old_pid[j], a0 = add_off[lo];
            uint32_t a = a0, b = add_off[lo + 1];       // the first new entry of the list in [a, b) with add_pid >= pid, or b
            while (a < b) {
                const uint32_t mid = a + ((b - a) >> 1);
                if (add_pid[mid] < pid) a = mid + 1; else b = mid;
            }
            out[(int64_t)at + a] = pid;         // a = add_off[c] + the new entries of the list with a smaller pid
        }
        __syncthreads();        // s_c is rewritten by the next tile
    }
}

}  // namespace clb
