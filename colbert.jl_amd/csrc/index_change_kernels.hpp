// index_change_kernels.hpp -- device side of clb_searcher_append, clb_searcher_remove and clb_searcher_update (search.hip): the
// rows and the inverted lists of a changed index are the old ones with the removed or replaced passages' entries taken out and
// the new entries put where a fresh build of the changed index would put them, everything else in its old order.  No
// counterpart in the reference (its index is built once: _build_ivf, collection_indexer.jl:349-353, is what the changed lists
// must equal); upstream ColBERT's IndexUpdater has remove and add only.
// The set of removed or replaced passages arrives as a passage bitmap in the layout of a clb_filter (filter_mark_kernel,
// search_kernels.hpp): a SET bit means removed or replaced.  Beside it stands, for an update, slot[p], read only where the bit
// is set: the position of passage p in the caller's list, whose new rows are stage_off[slot] .. stage_off[slot + 1] - 1 of the
// staged new rows.  A removal has neither staged rows nor slots: every named passage's new length is zero (STAGED = false).
#pragma once
#include "common.hpp"

namespace clb {

__device__ __forceinline__ bool removed_bit(const uint32_t* __restrict__ bits, uint32_t p) { return (bits[p >> 5] >> (p & 31)) & 1u; }

// the last i in [lo, hi) with off[i] <= j, given off[lo] <= j: the segment of item j (the empty segments in front of it share
// its offset)
__device__ __forceinline__ int last_at_or_below(const uint32_t* __restrict__ off, int lo, int hi, int64_t j) {
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)off[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// The flat kernels below work in tiles of kTile consecutive items (output rows, list entries), taken grid-stride by blocks of
// 256.  A tile finds the segments of its first and last item once -- two full binary searches in off (n_seg + 1 offsets,
// off[0] = 0, off[n_seg] = the items), by threads 0 and 1, through s_seg -- and every item then searches only between those
// two.  Ends with a barrier; the caller barriers again before the next tile rewrites s_seg.
constexpr int kTileItems = 8;
constexpr int kTile = 256 * kTileItems;

__device__ __forceinline__ void tile_segments(const uint32_t* __restrict__ off, int n_seg, int64_t j0, int64_t j1, int* s_seg,
                                              int& seg_lo, int& seg_hi) {
    if (threadIdx.x < 2) s_seg[threadIdx.x] = last_at_or_below(off, 0, n_seg, threadIdx.x == 0 ? j0 : j1);
    __syncthreads();
    seg_lo = s_seg[0];
    seg_hi = s_seg[1];
}

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
struct ChangeCounts {
    uint32_t changed;               // named passages whose old or new length is not zero (a removal: that lose an embedding)
    uint32_t longest;               // the longest passage of the changed index
    unsigned long long dropped;     // STAGED only: the rows the named passages held before (the changed index must fit a shard)
};

// len[p] = named(p) ? the new length (STAGED; zero otherwise) : doc_off[p + 1] - doc_off[p], p = 0 .. n_docs - 1, and
// len[n_docs] = 0 (the scan's pad).  One atomic per wave and counter: the wave's sum / maximum first.
template <bool STAGED>
static __global__ __launch_bounds__(256) void change_lengths_kernel(const uint32_t* __restrict__ doc_off,
                                                                    const uint32_t* __restrict__ bits,
                                                                    const uint32_t* __restrict__ slot,
                                                                    const uint32_t* __restrict__ stage_off, int n_docs,
                                                                    uint32_t* __restrict__ len, ChangeCounts* __restrict__ counts) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    uint32_t changed = 0, longest = 0;
    unsigned long long dropped = 0;
    if (p < n_docs) {
        longest = doc_off[p + 1] - doc_off[p];
        if (removed_bit(bits, (uint32_t)p)) {
            const uint32_t old_len = longest;
            longest = 0;
            if constexpr (STAGED) {
                const uint32_t i = slot[p];
                longest = stage_off[i + 1] - stage_off[i];
                dropped = old_len;
            }
            changed = (old_len | longest) != 0;
        }
        len[p] = longest;
    } else if (p == n_docs) {
        len[p] = 0;
    }
    for (int d = 32; d > 0; d >>= 1) {
        changed += __shfl_xor(changed, d);
        longest = max(longest, (uint32_t)__shfl_xor(longest, d));
        if constexpr (STAGED) dropped += __shfl_xor(dropped, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (changed) atomicAdd(&counts->changed, changed);
        if (longest) atomicMax(&counts->longest, longest);
        if (dropped) atomicAdd(&counts->dropped, dropped);
    }
}

// The rows.  A flat grid over the OUTPUT rows: row j of the changed index belongs to the passage p with new_off[p] <= j <
// new_off[p + 1] (the LAST p with new_off[p] <= j: the empty passages in front of it share its offset), at rank r = j -
// new_off[p] inside it.  Its source is staged row stage_off[slot[p]] + r when p is replaced -- the staging buffer holds the new
// rows in create's per-passage code order on the tuned path, as given on the general path -- and old row old_off[p] + r when it
// is not: rows keep their order inside a kept passage, so create's per-passage code order survives.  Without staged rows
// (STAGED = false, a removal) a named passage has no output row and every source is an old row: no bitmap, slot or stage_off
// is read.  A tile of kTile rows finds its passages with tile_segments, as ivf_merge_kernel does in the list offsets; the
// tile's sources go to LDS (s_src: the row; s_new, STAGED only: one bit per row of the tile, set = staged).  The residual rows
// are then copied as ONE run of pieces per tile: consecutive lanes write consecutive pieces (Piece = 16 bytes on the tuned
// path, where a row is 16 * nbits bytes; 4 or 1 byte for the general path's other sizes).  Every output row is written exactly
// once; the zero padding behind the last row is the host's (alloc_padded_rows).
// grid = min(tiles, any cap), block = 256; tiles are taken grid-stride.
template <class Piece, bool STAGED>
static __global__ __launch_bounds__(256) void splice_rows_kernel(
    const uint32_t* __restrict__ old_off, const uint32_t* __restrict__ new_off, const uint32_t* __restrict__ bits,
    const uint32_t* __restrict__ slot, const uint32_t* __restrict__ stage_off, int n_docs, int64_t n_rows,
    const uint32_t* __restrict__ codes_old, const Piece* __restrict__ res_old, const uint32_t* __restrict__ codes_stage,
    const Piece* __restrict__ res_stage, int pieces, uint32_t* __restrict__ codes_dst, Piece* __restrict__ res_dst) {
    __shared__ int s_p[2];
    __shared__ uint32_t s_src[kTile];
    __shared__ uint32_t s_new[STAGED ? kTile / 32 : 1];
    const int64_t tiles = (n_rows + kTile - 1) / kTile;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t j0 = tile * kTile;
        const int64_t j1 = (j0 + kTile < n_rows ? j0 + kTile : n_rows) - 1;
        if constexpr (STAGED) {
            if (threadIdx.x < kTile / 32) s_new[threadIdx.x] = 0u;
        }
        int p_lo, p_hi;
        tile_segments(new_off, n_docs, j0, j1, s_p, p_lo, p_hi);
#pragma unroll
        for (int i = 0; i < kTileItems; ++i) {
            const int r = i * 256 + threadIdx.x;
            const int64_t j = j0 + r;
            if (j > j1) break;
            const int p = last_at_or_below(new_off, p_lo, p_hi + 1, j);     // new_off[p_lo] <= j0 <= j <= j1 < new_off[p_hi + 1]
            const uint32_t rank = (uint32_t)j - new_off[p];
            uint32_t src = old_off[p] + rank;
            bool staged = false;
            if constexpr (STAGED) staged = removed_bit(bits, (uint32_t)p);
            if (staged) {
                src = stage_off[slot[p]] + rank;
                atomicOr(&s_new[r >> 5], 1u << (r & 31));
                codes_dst[j] = codes_stage[src];
            } else {
                codes_dst[j] = codes_old[src];
            }
            s_src[r] = src;
        }
        __syncthreads();
        const int n_pieces = (int)(j1 - j0 + 1) * pieces;       // at most 2048 rows of at most dim / 8 * 8 bytes
        Piece* dst = res_dst + (size_t)j0 * pieces;
        for (int i = threadIdx.x; i < n_pieces; i += 256) {
            const int r = i / pieces;
            const Piece* src = res_old;
            if constexpr (STAGED) {
                if ((s_new[r >> 5] >> (r & 31)) & 1u) src = res_stage;
            }
            dst[i] = src[(size_t)s_src[r] * pieces + (i - r * pieces)];
        }
        __syncthreads();        // s_p, s_src and s_new are rewritten by the next tile
    }
}

// The inverted lists: the new entries.  Per NEW embedding e (in the caller's order, codes already 0-based and checked): the
// local passage it belongs to and one count in the histogram of the new codes.  The passage: the last entry i of the caller's
// n passages with off[i] <= e (their own n + 1 offsets among the new embeddings, off[0] = 0), then pid_base + i -- an append,
// pid_base = the passages the handle held before -- when pids is null and pids[i] - pid_offset - 1 when it is not (an update).
// hist has K + 1 entries, zeroed (the scan wants the pad).
static __global__ __launch_bounds__(256) void hist_pid_kernel(const uint32_t* __restrict__ codes0, const uint32_t* __restrict__ off,
                                                              const int64_t* __restrict__ pids, int64_t pid_offset,
                                                              uint32_t pid_base, int64_t n_emb, int n,
                                                              uint32_t* __restrict__ hist, uint32_t* __restrict__ pid_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_emb) return;
    const int i = last_at_or_below(off, 0, n, e);
    pid_out[e] = pids ? (uint32_t)(pids[i] - pid_offset - 1) : pid_base + (uint32_t)i;
    atomicAdd(&hist[codes0[e]], 1u);
}

// Where list c starts in the changed array, c = 0 .. K: new_off[c] = kept(old_off[c]) + add_off[c].  kept(j) = pos[j], the
// kept entries in front of old entry j (KEPT), and j itself when every old entry stays (an append's merge); add_off[c], the new
// entries in front of list c (ADD), is absent from a compaction.
template <bool KEPT, bool ADD>
static __global__ void list_offsets_kernel(const uint32_t* __restrict__ old_off, const uint32_t* __restrict__ pos,
                                           const uint32_t* __restrict__ add_off, int n, uint32_t* __restrict__ new_off) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    uint32_t at = old_off[c];
    if constexpr (KEPT) at = pos[at];
    if constexpr (ADD) at += add_off[c];
    new_off[c] = at;
}

// The merge of an append.  A flat grid over the OUTPUT: entry j of the merged array belongs to the list c with new_off[c] <= j <
// new_off[c + 1]; at rank r = j - new_off[c] it is old entry old_off[c] + r while r is below the old length, and entry
// add_off[c] + r - old_len of the (code, embedding)-sorted new entries after that.  Every output is written exactly once,
// consecutive lanes write consecutive words and -- inside a list segment -- read consecutive words; an empty old or new
// segment is never visited because no j maps to it.  A tile of kTile outputs finds the lists of its first and last
// entry once (tile_segments in new_off, K + 1 words that stay in L2) and every entry then searches only between
// those two: at 1 M passages a list holds ~900 entries, so a tile spans two or three lists and the per-entry search is one or
// two steps.  Work per tile is equal whatever the list lengths are, which a wave-per-list mapping cannot give on a topical
// index (lengths from 0 to tens of thousands) or for a small append (K waves launched to move a few entries each).
// grid = min(tiles, any cap), block = 256; tiles are taken grid-stride.
static __global__ __launch_bounds__(256) void ivf_merge_kernel(const uint32_t* __restrict__ old_off,
                                                              const uint32_t* __restrict__ add_off,
                                                              const uint32_t* __restrict__ new_off,
                                                              const uint32_t* __restrict__ old_pid,
                                                              const uint32_t* __restrict__ add_pid, int K, int64_t n_total,
                                                              uint32_t* __restrict__ out) {
    __shared__ int s_c[2];
    const int64_t tiles = (n_total + kTile - 1) / kTile;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t j0 = tile * kTile;
        const int64_t j1 = (j0 + kTile < n_total ? j0 + kTile : n_total) - 1;
        int c_lo, c_hi;
        tile_segments(new_off, K, j0, j1, s_c, c_lo, c_hi);
#pragma unroll
        for (int i = 0; i < kTileItems; ++i) {
            const int64_t j = j0 + (int64_t)i * 256 + threadIdx.x;
            if (j > j1) break;
            const int c = last_at_or_below(new_off, c_lo, c_hi + 1, j);     // new_off[c_lo] <= j0 <= j <= j1 < new_off[c_hi + 1]
            const uint32_t r = (uint32_t)j - new_off[c];
            const uint32_t o0 = old_off[c], old_len = old_off[c + 1] - o0;
            out[j] = r < old_len ? old_pid[o0 + r] : add_pid[add_off[c] + (r - old_len)];
        }
        __syncthreads();        // s_c is rewritten by the next tile
    }
}

// The compaction of a removal.  flag[j] = 1 when entry j's passage stays, j = 0 .. n - 1, and flag[n] = 0 (the scan's pad) ...
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

// The merge of an update, on a handle whose lists hold non-decreasing pids.  A passage is wholly kept or wholly replaced, so no
// pid comes from both sides and the changed list of centroid c is the merge by pid of its kept old entries (pos: the exclusive
// scan of the keep flags, n_old + 1 entries, as in a removal) and the new entries with code c (add_code / add_pid: the new
// entries sorted by (code, pid), n_add of them; add_off: the scan of their histogram).  Every entry computes its own
// destination:
//   kept old entry j of list c  ->  pos[j] + add_off[c] + |{new entries of c with a smaller pid}|
//   new entry i, of list c      ->  pos[first old entry of list c whose pid is not smaller] + i
// (i counts the new entries of the lists before c and those of c in front of it; pos[..] the kept entries of the lists before
// c and those of c with a smaller pid -- a replaced passage's own old entries are not kept and do not move pos).  A flat grid
// over the n_old old entries, then over the n_add new ones, in tiles of kTile.  An old tile finds the lists of its
// first and last entry once (tile_segments in old_off, K + 1 words that stay in L2) and every entry then searches
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
    const int64_t tiles_old = (n_old + kTile - 1) / kTile;
    const int64_t tiles = tiles_old + (n_add + kTile - 1) / kTile;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if (tile >= tiles_old) {        // new entries (the whole block takes this branch)
            const int64_t i0 = (tile - tiles_old) * kTile;
#pragma unroll
            for (int t = 0; t < kTileItems; ++t) {
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
        const int64_t j0 = tile * kTile;
        const int64_t j1 = (j0 + kTile < n_old ? j0 + kTile : n_old) - 1;
        int c_lo, c_hi;
        tile_segments(old_off, K, j0, j1, s_c, c_lo, c_hi);
#pragma unroll
        for (int t = 0; t < kTileItems; ++t) {
            const int64_t j = j0 + (int64_t)t * 256 + threadIdx.x;
            if (j > j1) break;
            const uint32_t at = pos[j];
            if (pos[j + 1] == at) continue;     // a replaced passage's entry
            const int c = last_at_or_below(old_off, c_lo, c_hi + 1, j);     // old_off[c_lo] <= j0 <= j <= j1 < old_off[c_hi + 1]
            const uint32_t pid = old_pid[j], a0 = add_off[c];
            uint32_t a = a0, b = add_off[c + 1];        // the first new entry of the list in [a, b) with add_pid >= pid, or b
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
