// group_kernels.hpp -- grouped search: rank documents by their best passage (no counterpart in the reference; the
// "collapse" of Elasticsearch / Vespa).  A grouping maps every local passage to the dense 0-based index of its group,
// non-decreasing in pid, so the passages of one group are consecutive pids -- and, the candidates of a query being an
// ascending pid list (bitmap_emit_kernel), consecutive entries of every candidate list.  "Best passage per group" is
// therefore a run reduction over that list: no sort, no hash, no atomics.
// Across the shards of a group (second half of this file) a group may lie on both sides of a cut: the shards then name it by
// one global index, the threshold and the merge count it once.
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
//
// run_max_tiles is that reduction for the n entries of one query, by all 1 024 threads of a work-group, shared with the
// m-th best of every run (group_extend_kernel): `load(i, &g, &e)` gives entry i its group and its word,
// `out.run(r, best)` takes the final word of run r (every run once, by one thread), `out.entry(i, r)` the run index of
// entry i.  Returns the number of runs (every thread the same).
struct RunScanShared {
    uint32_t last[1024];                // group of every thread's last entry
    unsigned long long v[16];           // per wave: the stretch behind the wave's last head
    int f[16], c[16];                   // per wave: has a head / number of heads
};
template <class Load, class Out>
__device__ __forceinline__ int run_max_tiles(int n, RunScanShared& sh, Load load, Out out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
            g[c] = kNoGroup;
            e[c] = 0ull;
            if (c < chunk && i < n) load(i, &g[c], &e[c]);
        }
        // the group of the thread's last valid entry (valid entries are a prefix of the chunk, and of the tile)
        uint32_t last = kNoGroup;
#pragma unroll
        for (int c = 0; c < kGroupChunk; ++c) last = g[c] != kNoGroup ? g[c] : last;
        sh.last[tid] = last;
        __syncthreads();
        uint32_t prev = tid > 0 ? sh.last[tid - 1] : prev_tile;
        if (tid == 0) prev_tile = sh.last[1023];       // only a full tile has a successor
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
        if (lane == 63) { sh.c[wave] = xc; sh.f[wave] = xf; sh.v[wave] = xv; }
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
            const unsigned long long v = sh.v[w2];
            open_all = sh.f[w2] ? v : (v > open_all ? v : open_all);
            heads_all += sh.c[w2];
            if (w2 + 1 == wave) open = open_all;
            if (w2 < wave) runs_before += sh.c[w2];
        }
        unsigned long long acc = ef ? ev : (ev > open ? ev : open);    // ... and as the thread itself does
        // 3. the runs that end inside the chunk
        int r = runs_before - 1;                       // index of the open run (-1: the list begins here)
#pragma unroll
        for (int c = 0; c < kGroupChunk; ++c) {
            if ((heads >> c) & 1u) {
                if (r >= 0) out.run(r, acc);
                ++r;
                acc = e[c];
            } else {
                acc = e[c] > acc ? e[c] : acc;
            }
            if (g[c] != kNoGroup) out.entry(i0 + c, r);
        }
        carry = open_all;
        nruns += heads_all;
    }
    if (tid == 0 && nruns > 0) out.run(nruns - 1, carry);
    return nruns;
}

// the word of a slot: order key << 32 | ~slot
__device__ __forceinline__ unsigned long long slot_word(float score, int slot) {
    return ((unsigned long long)f32_order_key(score) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)slot);
}
__device__ __forceinline__ int word_slot(unsigned long long w) { return (int)(0xffffffffu - (uint32_t)(w & 0xffffffffull)); }
__device__ __forceinline__ float word_score(unsigned long long w) { return f32_from_order_key((uint32_t)(w >> 32)); }

static __global__ __launch_bounds__(1024) void group_collapse_kernel(const float* __restrict__ scores,
                                                                    const uint32_t* __restrict__ cand,
                                                                    const int* __restrict__ ncand,
                                                                    const int* __restrict__ list /*optional*/,
                                                                    const int* __restrict__ nlist,
                                                                    const uint32_t* __restrict__ gid, size_t cand_cap,
                                                                    int* __restrict__ glist, int* __restrict__ nglist) {
    __shared__ RunScanShared sh;
    const int b = blockIdx.x;
    const int n = list ? nlist[b] : ncand[b];
    const float* sc = scores + (size_t)b * cand_cap;
    const uint32_t* cnd = cand + (size_t)b * cand_cap;
    const int* lst = list ? list + (size_t)b * cand_cap : nullptr;
    struct Out {
        int* out;
        __device__ void run(int r, unsigned long long best) const { out[r] = word_slot(best); }
        __device__ void entry(int, int) const {}
    } out{glist + (size_t)b * cand_cap};
    const int nruns = run_max_tiles(n, sh, [&](int i, uint32_t* g, unsigned long long* e) {
        const int slot = lst ? lst[i] : i;
        *g = gid[cnd[slot]];
        *e = slot_word(sc[slot], slot);
    }, out);
    if (threadIdx.x == 0) nglist[b] = nruns;
}

// S7g-e (hits of a grouped search, per_group = m > 1; two-pass mode, behind the selection).  The list of the selection is
// L0 = {slot : !(a[slot] < thr)}, thr = tau - 2 eps from thresh[b] = {tau, eps} exactly as margin_threshold forms it (-inf:
// everything is listed, and this kernel only copies).  It is extended by the passages that can be one of the m best of a
// listed group:  xlist = L0 + {slot : its run has a member in L0 and !(a[slot] < a_m - 2 eps)},
// a_m = the m-th largest approximate score of the run among ALL the query's candidates (a run shorter than m: all of it),
// slots ascending, xnlist[b] their number.
// The m-th largest of every run at once, whatever the run lengths: m rounds of the run reduction of the collapse over the
// query's candidates.  Round 0 leaves cut[r] = the largest word of run r -- or kDeadRun when that score is below thr: the
// run has no member in L0 -- and runidx[slot] = r; round i > 0 reduces the words BELOW cut[run] and leaves the next
// largest (0: the run has no more entries; a dead run stays dead).  Words are distinct, so i rounds remove exactly the i
// largest.  cut[r] of a round is written at the head of run r + 1, behind the two barriers of a tile in which or before
// which every entry of run r has been loaded: the rounds work in place.  grid = B, block = 1024.
constexpr unsigned long long kDeadRun = ~0ull;
static __global__ __launch_bounds__(1024) void group_extend_kernel(const float* __restrict__ scores,
                                                                  const uint32_t* __restrict__ cand,
                                                                  const int* __restrict__ ncand,
                                                                  const uint32_t* __restrict__ gid,
                                                                  const float* __restrict__ thresh, int m, size_t cand_cap,
                                                                  unsigned long long* cut, int* runidx,
                                                                  int* __restrict__ xlist, int* __restrict__ xnlist) {
    __shared__ RunScanShared sh;
    __shared__ int sh_scan[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = ncand[b];
    n = n < 0 ? 0 : ((size_t)n > cand_cap ? (int)cand_cap : n);
    const float* sc = scores + (size_t)b * cand_cap;
    const uint32_t* cnd = cand + (size_t)b * cand_cap;
    unsigned long long* ct = cut + (size_t)b * cand_cap;
    int* ri = runidx + (size_t)b * cand_cap;
    int* out = xlist + (size_t)b * cand_cap;
    const float tau = thresh[2 * b], eps = thresh[2 * b + 1];
    const float thr = tau == kNegInf ? kNegInf : tau - 2.f * eps;
    if (thr == kNegInf) {                              // uniform: an unsafe query, or one with fewer than k groups
        for (int i = tid; i < n; i += 1024) out[i] = i;
        if (tid == 0) xnlist[b] = n;
        return;
    }
    struct First {
        unsigned long long* ct; int* ri; float thr;
        __device__ void run(int r, unsigned long long best) const { ct[r] = !(word_score(best) < thr) ? best : kDeadRun; }
        __device__ void entry(int i, int r) const { ri[i] = r; }
    };
    struct Next {
        unsigned long long* ct;
        __device__ void run(int r, unsigned long long best) const { ct[r] = best; }
        __device__ void entry(int, int) const {}
    };
    run_max_tiles(n, sh, [&](int i, uint32_t* g, unsigned long long* e) {
        *g = gid[cnd[i]];
        *e = slot_word(sc[i], i);
    }, First{ct, ri, thr});
    __syncthreads();
    for (int round = 1; round < m; ++round) {
        run_max_tiles(n, sh, [&](int i, uint32_t* g, unsigned long long* e) {
            const int r = ri[i];
            const unsigned long long c = ct[r], w = slot_word(sc[i], i);
            *g = (uint32_t)r;
            *e = c == kDeadRun ? kDeadRun : (w < c ? w : 0ull);
        }, Next{ct});
        __syncthreads();
    }
    // the ordered union: thread t owns the slots [t * chunk, (t + 1) * chunk), one block-wide scan of the counts places them
    const float two_eps = 2.f * eps;
    auto take = [&](int i) {
        const float a = sc[i];
        if (!(a < thr)) return true;
        const unsigned long long c = ct[ri[i]];
        return c != kDeadRun && (c == 0ull || !(a < word_score(c) - two_eps));
    };
    const int chunk = (n + 1023) >> 10;
    const int lo = min(tid * chunk, n), hi = min(lo + chunk, n);
    int cnt = 0;
    for (int i = lo; i < hi; ++i) cnt += take(i) ? 1 : 0;
    int xv = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(xv, o, 64);
        if (lane >= o) xv += y;
    }
    if (lane == 63) sh_scan[wave] = xv;
    __syncthreads();
    int wbase = 0, tot = 0;
    for (int w2 = 0; w2 < 16; ++w2) {
        const int sv = sh_scan[w2];
        if (w2 < wave) wbase += sv;
        tot += sv;
    }
    int pos = wbase + xv - cnt;
    for (int i = lo; i < hi; ++i)
        if (take(i)) out[pos++] = i;
    if (tid == 0) xnlist[b] = tot;
}

// S7g-f (hits of a grouped search, behind the top-k).  One wave per result (b, j): top_pids[b][j] is the representative of
// the j-th group (0: a padded row -- all padding).  Its group's run in the exact-scored set -- the re-scored list (list /
// nlist, slots ascending) or, with list == nullptr, all ncand[b] candidates -- is found by two binary searches on the group
// index, which is non-decreasing along the set; out[b][j][0 .. m) = the m largest words of the run, largest first (score
// order key descending, slot ascending: entry 0 is the representative itself), as pid and score, padded with (0, -inf).
// Entry i is the largest word below entry i - 1: m sweeps of the run by the wave, the first 64 entries kept in registers.
// grid = ceil(nq * k / 4), block = 256.
static __global__ __launch_bounds__(256) void group_hits_kernel(const float* __restrict__ scores,
                                                               const uint32_t* __restrict__ cand,
                                                               const int* __restrict__ ncand,
                                                               const int* __restrict__ list /*optional*/,
                                                               const int* __restrict__ nlist,
                                                               const uint32_t* __restrict__ gid, int64_t n_docs,
                                                               const int64_t* __restrict__ top_pids, int nq, int k, int m,
                                                               size_t cand_cap, int64_t pid_offset,
                                                               int64_t* __restrict__ out_pids, float* __restrict__ out_scores) {
    const int lane = threadIdx.x & 63;
    const int64_t res = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (res >= (int64_t)nq * k) return;                // uniform over the wave
    const int b = (int)(res / k);
    int64_t* op = out_pids + (size_t)res * m;
    float* os = out_scores + (size_t)res * m;
    const int64_t local = top_pids[res] - pid_offset - 1;
    int n = list ? nlist[b] : ncand[b];
    n = n < 0 ? 0 : ((size_t)n > cand_cap ? (int)cand_cap : n);
    if (top_pids[res] <= 0 || local < 0 || local >= n_docs || n == 0) {
        for (int i = lane; i < m; i += 64) { op[i] = 0; os[i] = kNegInf; }
        return;
    }
    const float* sc = scores + (size_t)b * cand_cap;
    const uint32_t* cnd = cand + (size_t)b * cand_cap;
    const int* lst = list ? list + (size_t)b * cand_cap : nullptr;
    const uint32_t g = gid[local];
    auto group_at = [&](int p) { return gid[cnd[lst ? lst[p] : p]]; };
    int lo = 0, hi = n;                                // first entry of a group >= g
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (group_at(mid) < g) lo = mid + 1; else hi = mid;
    }
    const int first = lo;
    hi = n;                                            // first entry of a group > g
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (group_at(mid) <= g) lo = mid + 1; else hi = mid;
    }
    const int end = lo;
    unsigned long long w0 = 0ull;                      // the lane's entry among the run's first 64
    if (first + lane < end) {
        const int slot = lst ? lst[first + lane] : first + lane;
        w0 = slot_word(sc[slot], slot);
    }
    unsigned long long prev = ~0ull;
    for (int i = 0; i < m; ++i) {
        unsigned long long best = w0 < prev ? w0 : 0ull;
        for (int p = first + 64 + lane; p < end; p += 64) {
            const int slot = lst ? lst[p] : p;
            const unsigned long long w = slot_word(sc[slot], slot);
            best = (w < prev && w > best) ? w : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long y = __shfl_xor(best, o, 64);
            best = y > best ? y : best;
        }
        if (lane == 0) {
            const int slot = word_slot(best);
            op[i] = best ? (int64_t)cnd[slot] + pid_offset + 1 : 0;
            os[i] = best ? sc[slot] : kNegInf;
        }
        prev = best;                                   // 0 once the run is exhausted: nothing is below it
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

// ---- grouped search across a shard group -----------------------------------------------------------------------------
// A shard's grouping is made from its slice of the group ids; group_base is the GLOBAL dense index of the group of the
// shard's first passage, so the global index of local passage p is group_base + gid[p].  Shards are contiguous pid ranges
// and groups are contiguous too: a group that lies on two shards is the LAST group of the one and the FIRST of the other
// (a group over three shards: the only group of the middle one).  Among the records a shard publishes for one query --
// distinct groups, one record each -- only the record with the lowest and the one with the highest group index can
// therefore meet the same index in another shard's records: at most two "boundary records" per shard and query, found
// by one wave per shard and resolved against each other in LDS.
constexpr int kMaxGroupShards = 256;                // lists whose boundary records one work-group holds (2 each)

// The lowest and the highest valid (>= 0) group index among g[0 .. k) and where they stand, by one wave; -1 when the list
// has no valid record.  Every lane returns the same positions.
__device__ __forceinline__ void wave_list_edges(const int64_t* __restrict__ g, int k, int lane, int* at_lo, int* at_hi) {
    long long glo = 0, ghi = 0;
    int ilo = -1, ihi = -1;
    for (int i = lane; i < k; i += 64) {
        const long long v = g[i];
        if (v < 0) continue;
        if (ilo < 0 || v < glo) { glo = v; ilo = i; }
        if (ihi < 0 || v > ghi) { ghi = v; ihi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long a = __shfl_xor(glo, o, 64), c = __shfl_xor(ghi, o, 64);
        const int ai = __shfl_xor(ilo, o, 64), ci = __shfl_xor(ihi, o, 64);
        if (ai >= 0 && (ilo < 0 || a < glo || (a == glo && ai < ilo))) { glo = a; ilo = ai; }
        if (ci >= 0 && (ihi < 0 || c > ghi || (c == ghi && ci < ihi))) { ghi = c; ihi = ci; }
    }
    *at_lo = ilo;
    *at_hi = ihi;
}

// The boundary records of one query's gathered lists all_top / all_gid [n_shards][B][k], for the 1024 threads of a work-group:
// e_at[2 l], e_at[2 l + 1] = the positions (in the query's n_shards * k records) of list l's records with the lowest and the
// highest valid group index, -1 where there is none; e_dead = 1 for a boundary record that loses to another of the same group
// (the larger score wins, the earlier record among equal ones).  The caller synchronises before it reads e_dead.
__device__ __forceinline__ void group_boundary_records(const float* __restrict__ all_top, const int64_t* __restrict__ all_gid,
                                                       int n_shards, int B, int b, int k, long long* e_gid, uint32_t* e_key,
                                                       int* e_at, int* e_dead) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int l = wave; l < n_shards; l += 16) {
        const size_t base = ((size_t)l * B + b) * k;
        int lo, hi;
        wave_list_edges(all_gid + base, k, lane, &lo, &hi);
        if (lane == 0) {
            if (hi == lo) hi = -1;                     // one valid record: one boundary record
            e_at[2 * l] = lo < 0 ? -1 : l * k + lo;
            e_at[2 * l + 1] = hi < 0 ? -1 : l * k + hi;
            e_gid[2 * l] = lo < 0 ? -1 : all_gid[base + lo];
            e_gid[2 * l + 1] = hi < 0 ? -1 : all_gid[base + hi];
            e_key[2 * l] = lo < 0 ? 0u : f32_order_key(all_top[base + lo]);
            e_key[2 * l + 1] = hi < 0 ? 0u : f32_order_key(all_top[base + hi]);
        }
    }
    __syncthreads();
    for (int t = tid; t < 2 * n_shards; t += 1024) {
        int dead = 0;
        if (e_at[t] >= 0)
            for (int j = 0; j < 2 * n_shards; ++j)
                dead |= j != t && e_at[j] >= 0 && e_gid[j] == e_gid[t] && (e_key[j] > e_key[t] || (e_key[j] == e_key[t] && j < t));
        e_dead[t] = dead;
    }
}

// S7g-c (phase 1 of the grouped two-phase search).  Of the query's groups -- glist[b][r] = the slot of the best approximate
// score of run r, nglist[b] runs (group_collapse_kernel over all candidates) -- the k with the largest score: out_top[b][i]
// the score, out_gid[b][i] the GLOBAL group index, in no particular order, padded with (-inf, -1).  Among scores equal to
// the k-th largest any may be taken: they are equal values, and the threshold phase 2 derives from them is a lower bound
// of the k-th best group whichever groups they name.  grid = B, block = 1024.
static __global__ __launch_bounds__(1024) void group_local_top_kernel(const float* __restrict__ scores,
                                                                     const uint32_t* __restrict__ cand,
                                                                     const int* __restrict__ glist,
                                                                     const int* __restrict__ nglist,
                                                                     const uint32_t* __restrict__ gid, int64_t group_base,
                                                                     int k, size_t cand_cap, float* __restrict__ out_top,
                                                                     int64_t* __restrict__ out_gid) {
    __shared__ __attribute__((aligned(16))) int hist[256];
    __shared__ uint32_t s_prefix, s_kmin, s_kmax;
    __shared__ int s_remaining, s_gt, s_eq;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = nglist[b];
    const float* sc = scores + (size_t)b * cand_cap;
    const uint32_t* cnd = cand + (size_t)b * cand_cap;
    const int* lst = glist + (size_t)b * cand_cap;
    float* o = out_top + (size_t)b * k;
    int64_t* og = out_gid + (size_t)b * k;
    if (n <= k) {                                      // uniform over the block: every group, then the padding
        for (int i = tid; i < k; i += 1024) {
            const int slot = i < n ? lst[i] : 0;
            o[i] = i < n ? sc[slot] : kNegInf;
            og[i] = i < n ? group_base + (int64_t)gid[cnd[slot]] : (int64_t)-1;
        }
        return;
    }
    const int chunk = (n + 1023) >> 10;
#define CLB_SEL_FOR_EACH(...)                                                                   \
    for (int c = 0; c < chunk; ++c) {                                                           \
        const int i_ = c * 1024 + tid;                                                          \
        const bool valid = i_ < n;                                                              \
        const uint32_t key = valid ? f32_order_key(sc[lst[i_]]) : 0u;                           \
        __VA_ARGS__                                                                             \
    }
    if (tid == 0) { s_prefix = 0u; s_remaining = k; s_gt = 0; s_eq = 0; }
    __syncthreads();
    CLB_RADIX_SELECT()
#undef CLB_SEL_FOR_EACH
    __syncthreads();
    const uint32_t tau = s_prefix;
    const int need_eq = s_remaining;                   // of the scores == tau, as many as the k places leave
    const int n_gt = k - need_eq;                      // scores > tau
    for (int i = tid; i < n; i += 1024) {
        const int slot = lst[i];
        const float v = sc[slot];
        const uint32_t key = f32_order_key(v);
        int pos = -1;
        if (key > tau) {
            pos = atomicAdd(&s_gt, 1);
        } else if (key == tau) {
            const int e = atomicAdd(&s_eq, 1);
            pos = e < need_eq ? n_gt + e : -1;
        }
        if (pos >= 0 && pos < k) {
            o[pos] = v;
            og[pos] = group_base + (int64_t)gid[cnd[slot]];
        }
    }
}

// S7g-d (phase 2).  tau[b] = the k-th largest score over the DISTINCT group indices of the gathered records
// all_top / all_gid [n_shards][B][k]: a repeated index counts once, with its largest score; -inf when fewer than k
// distinct finite records exist.  Records with index -1 (padding), and the boundary records that lose to a record of the
// same group, take part as -inf; the select over the n_shards * k keys is the radix-select core, run to the last bit.
// n_shards <= kMaxGroupShards.  grid = B, block = 1024.
static __global__ __launch_bounds__(1024) void group_global_tau_kernel(const float* __restrict__ all_top,
                                                                      const int64_t* __restrict__ all_gid, int n_shards,
                                                                      int B, int k, float* __restrict__ tau_glob) {
    __shared__ __attribute__((aligned(16))) int hist[256];
    __shared__ uint32_t s_prefix, s_kmin, s_kmax;
    __shared__ int s_remaining;
    __shared__ long long e_gid[2 * kMaxGroupShards];
    __shared__ uint32_t e_key[2 * kMaxGroupShards];
    __shared__ int e_at[2 * kMaxGroupShards];          // position in the query's n_shards * k records, -1: no such record
    __shared__ int e_dead[2 * kMaxGroupShards];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = n_shards * k;
    group_boundary_records(all_top, all_gid, n_shards, B, b, k, e_gid, e_key, e_at, e_dead);
    if (tid == 0) { s_prefix = 0u; s_remaining = k; }
    __syncthreads();
    const uint32_t neg_key = f32_order_key(kNegInf);
    const int chunk = (n + 1023) >> 10;
#define CLB_SEL_FOR_EACH(...)                                                                   \
    for (int c = 0; c < chunk; ++c) {                                                           \
        const int i_ = c * 1024 + tid;                                                          \
        const bool valid = i_ < n;                                                              \
        uint32_t key = 0u;                                                                      \
        if (valid) {                                                                            \
            const int l_ = i_ / k;                                                              \
            const size_t at_ = ((size_t)l_ * B + b) * k + (i_ - l_ * k);                        \
            const bool gone_ = all_gid[at_] < 0 || (e_at[2 * l_] == i_ && e_dead[2 * l_]) ||    \
                               (e_at[2 * l_ + 1] == i_ && e_dead[2 * l_ + 1]);                  \
            key = gone_ ? neg_key : f32_order_key(all_top[at_]);                                \
        }                                                                                       \
        __VA_ARGS__                                                                             \
    }
    CLB_RADIX_SELECT()
#undef CLB_SEL_FOR_EACH
    if (tid == 0) tau_glob[b] = f32_from_order_key(s_prefix);
}

// After a grouped search on a shard: out_gids[b][i] = the GLOBAL group index of result pid out_pids[b][i] (-1 for the
// pid-0 padding), and edge_gids[b] = the global group index of the query's lowest-pid and highest-pid candidate (the slot's
// candidate list is ascending in pid), (-1, -1) for a query without candidates: what the merge across the shards needs to
// find a group that two shards both returned, and to count a group that straddles a cut once.
// grid = ceil(max(B * k, B) / 256), block = 256.
static __global__ __launch_bounds__(256) void group_result_kernel(const int64_t* __restrict__ out_pids, int B, int k,
                                                                 int64_t pid_offset, const uint32_t* __restrict__ gid,
                                                                 int64_t n_docs, int64_t group_base,
                                                                 const uint32_t* __restrict__ cand, const int* __restrict__ ncand,
                                                                 size_t cand_cap, int64_t* __restrict__ out_gids,
                                                                 int64_t* __restrict__ edge_gids) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)B * k) {
        const int64_t local = out_pids[i] - pid_offset - 1;
        out_gids[i] = (out_pids[i] > 0 && local >= 0 && local < n_docs) ? group_base + (int64_t)gid[local] : (int64_t)-1;
    }
    if (i < B) {
        int n = ncand[i];
        n = n < 0 ? 0 : ((size_t)n > cand_cap ? (int)cand_cap : n);
        const uint32_t* cnd = cand + (size_t)i * cand_cap;
        edge_gids[2 * i] = n > 0 ? group_base + (int64_t)gid[cnd[0]] : (int64_t)-1;
        edge_gids[2 * i + 1] = n > 0 ? group_base + (int64_t)gid[cnd[n - 1]] : (int64_t)-1;
    }
}

// The merge of the shards' grouped top-k lists: merge_topk_kernel with one record per GROUP.  in: [n_lists][B][k] records
// (pid, score, global group index) sorted by (score desc, pid asc), padded with (0, -inf, -1), the groups of one list
// distinct.  Of the records of one group only the first in that order survives; a survivor's place is its rank in the
// plain merge minus the dead records ranked before it.  The dead are boundary records (at most 2 n_lists of them), so
// every work-group finds them again -- one wave per list -- and keeps them in LDS.  Work-group (0, b) also writes
// out_n_cand[b] = the sum of the lists' candidate-group counts minus the lists whose first edge group equals the last edge
// group of the nearest list before it that has candidates: a group that straddles cuts is counted once, however many
// shards it spans.  Strides as in merge_topk_kernel, in elements.  n_lists <= kMaxGroupShards.
// grid = (ceil(n_lists * k / 256), B), block = 256; the output is filled with padding beforehand (fill_pad_kernel).
// All three comparisons below go through rec_before (search_kernels.hpp), which orders scores by their order keys: -0.0 below +0.0.
static __global__ __launch_bounds__(256) void merge_topk_grouped_kernel(
    const int64_t* __restrict__ pids, const float* __restrict__ scores, const int64_t* __restrict__ gids, int k, int n_lists,
    int B, size_t pid_stride, size_t score_stride, size_t gid_stride, const int64_t* __restrict__ n_cand_lists,
    size_t n_cand_stride, const int64_t* __restrict__ edge_gids, size_t edge_stride, int64_t* __restrict__ out_pids,
    float* __restrict__ out_scores, int64_t* __restrict__ out_n_cand) {
    __shared__ long long e_gid[2 * kMaxGroupShards], e_pid[2 * kMaxGroupShards];
    __shared__ float e_sc[2 * kMaxGroupShards];
    __shared__ int e_at[2 * kMaxGroupShards], e_dead[2 * kMaxGroupShards];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int l = wave; l < n_lists; l += 4) {
        int lo, hi;
        wave_list_edges(gids + (size_t)l * gid_stride + (size_t)b * k, k, lane, &lo, &hi);
        if (lane == 0) {
            if (hi == lo) hi = -1;
            const int at[2] = {lo, hi};
            for (int h = 0; h < 2; ++h) {
                const int a = at[h];
                const int64_t p = a < 0 ? 0 : pids[(size_t)l * pid_stride + (size_t)b * k + a];
                e_at[2 * l + h] = (a < 0 || p <= 0) ? -1 : l * k + a;
                e_pid[2 * l + h] = p;
                e_gid[2 * l + h] = a < 0 ? -1 : gids[(size_t)l * gid_stride + (size_t)b * k + a];
                e_sc[2 * l + h] = a < 0 ? kNegInf : scores[(size_t)l * score_stride + (size_t)b * k + a];
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < 2 * n_lists; t += 256) {
        int dead = 0;
        if (e_at[t] >= 0)
            for (int j = 0; j < 2 * n_lists; ++j)
                dead |= j != t && e_at[j] >= 0 && e_gid[j] == e_gid[t] && rec_before(e_sc[j], e_pid[j], e_sc[t], e_pid[t]);
        e_dead[t] = dead;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) {
        int64_t total = 0, prev_last = -1;
        for (int l = 0; l < n_lists; ++l) {
            total += n_cand_lists[(size_t)l * n_cand_stride + b];
            const int64_t first = edge_gids[(size_t)l * edge_stride + 2 * (size_t)b];
            const int64_t last = edge_gids[(size_t)l * edge_stride + 2 * (size_t)b + 1];
            if (first < 0) continue;                   // a list without candidates
            if (first == prev_last) total -= 1;
            prev_last = last;
        }
        out_n_cand[b] = total;
    }
    const int idx = blockIdx.x * blockDim.x + tid;
    if (idx >= n_lists * k) return;
    const int l = idx / k, i = idx % k;
    const int64_t p = pids[(size_t)l * pid_stride + (size_t)b * k + i];
    const float s = scores[(size_t)l * score_stride + (size_t)b * k + i];
    if (p <= 0) return;  // padding
    if ((e_at[2 * l] == idx && e_dead[2 * l]) || (e_at[2 * l + 1] == idx && e_dead[2 * l + 1])) return;
    int rank = i;
    for (int l2 = 0; l2 < n_lists; ++l2) {
        if (l2 == l) continue;
        const int64_t* pl = pids + (size_t)l2 * pid_stride + (size_t)b * k;
        const float* sl = scores + (size_t)l2 * score_stride + (size_t)b * k;
        int lo = 0, hi = k;  // number of records of list l2 that come before (s, p)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int64_t p2 = pl[mid];
            const float s2 = sl[mid];
            if (p2 > 0 && rec_before(s2, p2, s, p)) lo = mid + 1; else hi = mid;
        }
        rank += lo;
    }
    for (int j = 0; j < 2 * n_lists; ++j)
        rank -= (e_at[j] >= 0 && e_dead[j] && rec_before(e_sc[j], (int64_t)e_pid[j], s, p)) ? 1 : 0;
    if (rank < k) {
        out_pids[(size_t)b * k + rank] = p;
        out_scores[(size_t)b * k + rank] = s;
    }
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
