// search.hip -- the Searcher handle and the search entry points of the C ABI (include/colbert_hip.h).
// Replaces: struct Searcher / Searcher(index_path) (src/searching.jl:1-91) and search() after the
// encoder (src/searching.jl:102-127), retrieve/gather/maxsim (src/search/ranking.jl).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>

#include "approx_kernels.hpp"
#include "after_kernels.hpp"
#include "filter_kernels.hpp"
#include "generic_kernels.hpp"
#include "group_kernels.hpp"
#include "index_change_kernels.hpp"
#include "list_kernels.hpp"
#include "prior_kernels.hpp"
#include "search_kernels.hpp"
#include "sort.hpp"

using namespace clb;

namespace {

enum KernelId {
    KID_CENTROID_SCORES = 0,
    KID_TOPN,
    KID_MARK,
    KID_COMPACT,
    KID_SCORE_EXACT,
    KID_SCORE_APPROX,
    KID_SELECT,
    KID_ROWS,
    KID_TOPK,
    KID_COUNT
};
const char* kKernelNames[KID_COUNT] = {"centroid_scores", "top_nprobe", "mark_candidates", "compact_candidates",
                                       "score_exact",     "score_approx", "select_margin", "rescore_rows",
                                       "topk"};

struct Prof {
    bool on = false;        // HIP-event timing of every kernel
    bool counters = false;  // additionally count the work of each batch (one extra kernel per batch)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending[KID_COUNT];
    std::vector<hipEvent_t> pool;
    // end event of the previous timed kernel: the next timed kernel on the same stream starts from it instead of
    // recording its own start (half the event records per batch).  Cleared wherever untimed work is enqueued.
    hipEvent_t chain = nullptr;
    hipStream_t chain_stream = nullptr;
    double total_ms[KID_COUNT] = {0};
    int64_t launches[KID_COUNT] = {0};
    bool failed = false;    // an event could not be created: that kernel goes untimed, clb_profile_read reports it
    hipEvent_t get() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { failed = true; return nullptr; }
        return e;
    }
};

}  // namespace

// A resident passage filter (include/colbert_hip.h): one bitmap in the layout of the candidate bitmap.  It owns its words
// and remembers its searcher by serial number only, so it may outlive the searcher (clb_filter_destroy then just frees).
struct clb_filter {
    uint64_t owner = 0;         // clb_searcher::serial of the searcher it was made for
    int device = 0;
    int64_t n_docs = 0, count = 0;
    DevBuf bits;                // u32 [ceil(n_docs / 32)]
};

// A resident passage grouping (include/colbert_hip.h): the dense 0-based group index of every local passage, non-decreasing
// in pid.  Like a clb_filter it owns its words and remembers its searcher by serial number only.
struct clb_grouping {
    uint64_t owner = 0;         // clb_searcher::serial of the searcher it was made for
    int device = 0;
    int64_t n_docs = 0, count = 0;
    DevBuf gid;                 // u32 [n_docs]
};

// A resident score prior (include/colbert_hip.h): one finite fp32 value per local passage.  Like a clb_grouping it owns its
// values and remembers its searcher by serial number only.
struct clb_prior {
    uint64_t owner = 0;         // clb_searcher::serial of the searcher it was made for
    int device = 0;
    int64_t n_docs = 0;
    float max_abs = 0.f;        // max |value|: a call's weight must keep |weight| * max_abs below FLT_MAX (check_prior)
    DevBuf values;              // fp32 [n_docs]
};

// Per-batch workspace (everything a batch of queries needs besides the resident index).
struct Workspace {
    int64_t Bcap = 0, Tcap = 0, npcap = 0, kcap = 0;
    int64_t Ttuned = 0;         // largest query length <= 128 this slot has seen (what the tuned-path buffers are sized for)
    size_t cand_cap = 0;
    int W = 0, nblk_bitmap = 0, topn_blocks = 0;
    bool x1_table = false;      // the score table in cells_q came from the single-fp16-product kernel: the bound carries its terms
    bool have_range = false;    // tscale holds this batch's measured score ranges (the batched centroid kernel ran)
    bool cell8 = false;         // pass 1 gathers from cells8: 32-byte rows of 8-bit cells requantised from cells_q by tscale
    size_t filt_cap = 0;        // largest filter population a CLB_FILTER_ALL call has asked this slot to hold (cand_cap covers it)
    size_t ivf_cap = 0;         // cand_cap before filt_cap was taken into account: the most candidates the IVF lists can give
    // two-phase sharded search: what clb_search_shard_phase1 left behind (phase 2 must continue exactly that batch)
    struct { bool valid = false; const float* dQ = nullptr; int64_t T = 0, B = 0, nprobe = 0, k = 0; void* stream = nullptr;
             size_t filt_now = 0; const clb_grouping* grp = nullptr; int64_t group_base = 0;
             const clb_prior* prior = nullptr; float weight = 0.f; } pending;
    // filt_now: Batch::filt_now of phase 1 -- phase 2 selects over the same candidates; grp / group_base: the grouping operands of
    // a grouped phase 1 (clb_search_shard_phase1_grouped_slot) -- phase 2 must be the grouped call with the same ones; prior /
    // weight: those of a phase 1 with a prior (clb_search_shard_phase1_prior_slot) -- phase 2 must be the prior call with the same
    // single-exchange grouped sharded search: the last whole search on this slot was a grouped one of B <= 64 queries (one
    // sub-batch, so its candidate lists are still here) -- clb_search_result_groups_slot reads the edge groups from them
    struct { bool valid = false; int64_t B = 0, k = 0, generation = 0; const clb_grouping* grp = nullptr; void* stream = nullptr; } grouped_done;
    DevBuf Qdev, cells, cells_q, partial, sel, bitmap, blocksum, ncand, cand, cand_hdr, scores, list, nlist, thresh,
        outp, outs, flags, stats, redo, rowmask, eps_pair, tokmax, tau_glob, wsel, bounds, tscale, rangep, cells8;
    // grouped search (group_kernels.hpp), sized once a call has passed a grouping: the best slot of every group among all
    // candidates (grp_list / grp_n: grp_n is the query's group count) and among the re-scored passages of the two-pass mode
    // (grp_list2 / grp_n2), and the threshold at the k-th best group
    bool grouped = false;
    DevBuf grp_list, grp_n, grp_list2, grp_n2, grp_tau;
    // hits of a grouped search (per_group = m > 1), sized once a call has asked for them: the largest m so far (outp / outs
    // then hold B k mcap entries), the top-k the hits are read from (hit_p / hit_s, [B][k]) and, in the two-pass mode, the
    // state of group_extend_kernel (hit_cut / hit_run) with the extended list it leaves (hit_list / hit_n)
    int64_t mcap = 0;
    DevBuf hit_p, hit_s, hit_cut, hit_run, hit_list, hit_n;
    // search with a prior (prior_kernels.hpp), sized once a call has passed one: per query the threshold of the boosted
    // selection (prior_tau[b]) and the largest boosted approximate score by magnitude (prior_tau[Bcap + b])
    bool prior = false;
    DevBuf prior_tau;
    // search after a cursor (after_kernels.hpp), sized once a call has passed one: the slots after_filter_kernel keeps and
    // their number, the threshold of after_cut_kernel, and the host route's copy of the cursors
    bool after = false;
    DevBuf after_list, after_n, after_tau, after_cur_s, after_cur_p;
    // candidate lists (list_kernels.hpp) on the host route, sized by the first listed call: the sub-batch's rows of the pid
    // block, its lengths and, when the call asks for them, its list scores
    DevBuf lst_pids, lst_lens, lst_scores;
    // ... with list priors (one value per list position), sized once a call has passed them: on the host route the sub-batch's
    // rows of the value block (lst_prior), and on every route the lowest list position of every candidate slot (slot_pos,
    // list_slot_kernel), 4 bytes per query and candidate of the slot's capacity
    bool list_prior = false;
    DevBuf lst_prior, slot_pos;
    DevBuf g_cells, g_keys, g_keys2, g_vals, g_vals2, g_scratch, g_sort_tmp;   // general-shape path (generic_kernels.hpp)
};

constexpr int kWorkspaceSlots = 4;

struct clb_searcher {
    int device = 0;
    uint64_t serial = 0;       // unique per handle of this process: what a clb_filter remembers of its searcher
    int64_t dim = 0, K = 0, n_docs = 0, n_emb = 0, pid_offset = 0;
    int nbits = 0;
    int mode = 0;
    int wide_select = -1;      // selection by kWideBlocks work-groups per query: -1 by candidate capacity, 0 never, 1 always
    bool approx_ok = false;
    bool bounds_synced = false;   // clb_searcher_set_bound_consts has been called: the error bound is the shard group's, not this shard's
    bool ivf_sorted = false;   // every IVF list holds non-decreasing passage ids (mark_count_kernel<true> needs it)
    bool generic = false;      // dim != 128 or nbits == 8: every query takes the general-shape path
    int64_t max_doclen = 0;
    hipStream_t stream = nullptr;
    // resident index (HBM)
    DevBuf centroids;   // fp32 [K][128]
    DevBuf weights;     // fp32 [2^nbits]
    DevBuf codes0;      // u32 [n_emb], 0-based
    DevBuf residuals;   // u8 [n_emb][16*nbits]
    DevBuf doc_off;     // u32 [n_docs+1]
    DevBuf live;        // u32 [ceil(n_docs / 32)]: the passages that hold embeddings, in a filter's layout (FilterArgs::live)
    DevBuf ivf_off;     // u32 [K+1]
    DevBuf ivf_pid;     // u32 [n_emb] local passage ids grouped by centroid
    DevBuf codeinv;     // u32 [n_emb]: code | quantised inv_norm, the one word pass 1 streams per embedding (two-pass mode)
    int cbits = 0;      // bits of the code field
    float inv_lo = 0.f, inv_step = 0.f;
    DevBuf cent_hi, cent_lo;  // bf16 [K][128] split of the centroids (bf16x3 centroid scoring)
    DevBuf cent_f16;          // fp16 [K][128]: the one operand of the single-product score table (batches of 16+ queries)
    float dc_f16 = 0.f;       // max ||c - fp16(c)|| over the centroids; approx_consts.dc_max carries it only for tables made from cent_f16
    int s1_x1 = -1;           // 16+ queries: score table from ONE fp16 product (to_f16_kernel's comment)?  1 yes, 0 three bf16 products,
                              // -1 by the handle's role: yes on a shard of a group (bounds_synced: the centroid stage is replicated on every
                              // shard while the pass-2 rows its wider bound adds are divided among them), no on a single GPU, where
                              // -0.020 ms on the centroid kernel meets +0.01-0.02 ms on pass 2 (profiles/r05_experiments.md)
    int gather_lds = 0; // pass 1: score rows through LDS-DMA, four adjacent lanes per row (0: the per-lane VGPR gather); set at load
    double code_adjacency = 0.0;   // fraction of consecutive embeddings that share a 128-B line of the score table
    int cell8 = -1;     // batches of 16+ queries: score rows as 32 bytes of 8-bit cells?  1 yes, 0 / -1 (default) fp16 rows.  On the
                        // shards of a group every shard's bound must cover every shard's table: set it alike on all shards
    ApproxConsts approx_consts{};
    std::vector<uint32_t> ivf_len_sorted;  // descending, for the candidate-capacity bound
    Workspace ws[kWorkspaceSlots];   // per-batch scratch, grown on demand (ensure_workspace); slots 1..: further batches in flight
    Prof prof;
    int64_t last_cand_docs = 0, last_cand_embs = 0, last_resc_docs = 0, last_resc_embs = 0;
    int64_t index_bytes = 0;
    int64_t generation = 0;    // clb_searcher_append / clb_searcher_remove calls that changed the handle
};

namespace {

// One sub-batch as run_search and its helpers are asked to run it.  It lives on the caller's stack: what belongs to a call
// never outlives it in the Workspace.
struct Batch {
    const float* dQ = nullptr;  // [B][T][dim] on the device
    int B = 0, T = 0, nprobe = 0, k = 0;
    int64_t* d_out_pids = nullptr; float* d_out_scores = nullptr; int64_t* d_n_cand = nullptr;
    // filtered search: the handles of the sub-batch (a HOST array, one entry per query, nullptr = unfiltered; nullptr
    // altogether when no query of the sub-batch is filtered: it then launches the unfiltered kernels), their scope, and
    // the largest filter population of the CLB_FILTER_ALL call this sub-batch belongs to when one of ITS queries is
    // filtered (0 otherwise: its candidates are the IVF lists')
    const clb_filter* const* filt = nullptr;
    int filt_all = 0;
    size_t filt_now = 0;
    const clb_grouping* grp = nullptr;      // grouped search: one grouping for the whole batch (checked by check_grouping)
    // ... with hits (per_group = m > 1; 0: none): d_out_pids / d_out_scores are the slot's hit_p / hit_s, the m best
    // passages of every result go to d_hit_pids / d_hit_scores [B][k][m]
    int per_group = 0;
    int64_t* d_hit_pids = nullptr; float* d_hit_scores = nullptr;
    // search with a prior: one prior and one weight for the whole batch (checked by check_prior); nullptr: none, and the
    // sub-batch launches exactly what it launches without one
    const clb_prior* prior = nullptr;
    float prior_weight = 1.f;
    // search after a cursor: the sub-batch's cursors on the device, [B] each; nullptr: none, and the sub-batch launches
    // exactly what it launches without them
    const float* d_after_s = nullptr; const int64_t* d_after_p = nullptr;
    // candidate lists: the sub-batch's rows of the pid block ([B][list_stride]) and its lengths ([B]) on the device -- they ARE
    // its candidate sets (nullptr: none, and the sub-batch launches exactly what it launches without them) -- and the list
    // scores it is to leave ([B][list_stride], or nullptr): asking for them makes the call a single exact pass
    const int64_t* d_list_pids = nullptr; const int64_t* d_list_lens = nullptr;
    int64_t list_stride = 0;
    float* d_list_scores = nullptr;
    // ... with list priors: the sub-batch's rows of the value block ([B][list_stride]) on the device, beside d_list_pids; the
    // additive term of candidate p is prior_weight * the value at p's lowest list position (nullptr: none, and the sub-batch
    // launches exactly what it launches without them).  Never together with `prior`: a call has one additive term
    const float* d_list_prior = nullptr;
    bool stats_keep = false;    // the 2nd, 3rd ... sub-batch of one call: the work counters accumulate over the call
    int phase = 0, n_shards = 0;    // two-phase sharded search (run_search)
    float* d_local_top = nullptr; const float* d_all_top = nullptr;
    // ... with a grouping (grp): the global index of the shard's first group, the group indices that travel with the scores
    // between the phases, and what the grouped merge needs of phase 2's result (group_result_kernel)
    int64_t group_base = 0;
    int64_t* d_local_gid = nullptr; const int64_t* d_all_gid = nullptr;
    int64_t* d_out_gids = nullptr; int64_t* d_edge_gids = nullptr;
    // ... with a prior (prior): the largest boosted approximate score by magnitude, per query, that travels with the scores
    float* d_local_mabs = nullptr; const float* d_all_mabs = nullptr;
};
Batch make_batch(const float* dQ, int64_t B, int64_t T, int64_t nprobe, int64_t k) {
    Batch q;
    q.dQ = dQ; q.B = (int)B; q.T = (int)T; q.nprobe = (int)nprobe; q.k = (int)k;
    return q;
}

// Does this sub-batch run as the two-pass pipeline?  By the handle's mode -- except a call that asks for list scores, which
// needs the exact score of EVERY candidate and so runs as the single exact pass (the two are identical by construction).
inline bool two_pass_mode(const clb_searcher* s, const Batch& q) {
    return s->mode == 1 && s->approx_ok && q.T <= 32 && !q.d_list_scores;
}

struct Timed {
    clb_searcher* s;
    int id;                 // a KernelId; negative: the scope times nothing and leaves the event chain alone
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    Timed(clb_searcher* s_, int id_, hipStream_t st_) : s(s_), id(id_), st(st_) {
        if (s->prof.on && id >= 0) {
            if (s->prof.chain && s->prof.chain_stream == st) {
                a = s->prof.chain;
            } else {
                a = s->prof.get();
                if (a && hipEventRecord(a, st) != hipSuccess) { s->prof.pool.push_back(a); a = nullptr; s->prof.failed = true; }
            }
            b = a ? s->prof.get() : nullptr;
        }
    }
    ~Timed() {
        if (!s->prof.on || id < 0) return;
        if (a && b && hipEventRecord(b, st) == hipSuccess) {
            s->prof.pending[id].push_back({a, b});
            s->prof.chain = b;
            s->prof.chain_stream = st;
        } else {                       // untimed launch: the next timed kernel records its own start
            s->prof.failed = true;
            s->prof.chain = nullptr;
        }
    }
};

// token tiles of 32 for the cells table: Tpad in {32, 64, 128} so that it divides the 256-thread scan
inline int token_tiles(int64_t T) { return T <= 32 ? 1 : T <= 64 ? 2 : 4; }
// entries per token of the selection buffer: the top-nprobe kernels come in widths 2, 8 and 32; beyond that a sort selects
inline int64_t padded_nprobe(int64_t nprobe) { return nprobe <= 2 ? 2 : nprobe <= 8 ? 8 : nprobe <= 32 ? 32 : nprobe; }

// 8-bit score rows for this handle's batches of 16+ queries?
// (round 6: only when asked for -- measured end to end the format loses on all four workloads, profiles/r06_experiments.md)
inline bool cell8_rows(const clb_searcher* s) { return s->cell8 == 1 && s->approx_ok; }

// the score table of this handle's batches of 16+ queries from ONE fp16 product (clb_searcher::s1_x1)?
inline bool single_product_table(const clb_searcher* s) {
    return (s->s1_x1 == 1 || (s->s1_x1 < 0 && s->bounds_synced)) && s->cent_f16.p && s->dc_f16 > 0.f;
}

// Pass 1's gather form by the index's own code statistics (derive_index_tables): LDS-DMA when neighbouring embeddings
// seldom share a line of the score table -- and only when the query's score table (64 B per centroid) does not fit the
// 4-MB L2 of an XCD: with a resident table the two forms are equal within 2 % (built index, K = 32 768: 0.663 / 0.668 ms)
inline int default_gather_lds(const clb_searcher* s) { return s->code_adjacency < 0.2 && s->K * 64 > ((int64_t)4 << 20); }

// the top-k kernel sorts up to kMaxTopK 8-byte keys in LDS: beyond 64 KB the attribute has to be raised
void allow_large_topk_lds() {
    allow_dynamic_lds(reinterpret_cast<const void*>(topk_kernel), (int)(sizeof(unsigned long long) * kMaxTopK));
}

constexpr int64_t kSubBatch = 64;      // queries per pass of the single-call search entry points (see for_sub_batches)

int next_pow2(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// filt_count: the largest filter population of a CLB_FILTER_ALL call (0 otherwise) -- such a query's candidates are its
// filter's passages, however few the IVF lists would give
int ensure_workspace_sized(clb_searcher* s, Workspace& w, int64_t B, int64_t T, int64_t nprobe, int64_t k, size_t filt_count,
                           bool grouped, int64_t per_group, bool prior, bool after, bool list_prior) {
    const int64_t t_tuned = T <= 128 ? T : 0;       // queries of up to 128 tokens take the tuned (or batched general) kernels
    if (B <= w.Bcap && T <= w.Tcap && t_tuned <= w.Ttuned && nprobe <= w.npcap && k <= w.kcap && filt_count <= w.filt_cap &&
        (!grouped || w.grouped) && per_group <= w.mcap && (!prior || w.prior) && (!after || w.after) && (!list_prior || w.list_prior))
        return CLB_OK;
    CLB_HIP(hipDeviceSynchronize());       // buffers may be in use on any of the caller's streams
    B = std::max(B, w.Bcap); T = std::max(T, w.Tcap);
    nprobe = std::max(nprobe, w.npcap); k = std::max(k, w.kcap);
    per_group = std::max(per_group, w.mcap);
    // T is the LARGEST query length this slot has seen; the buffers of the tuned kernels (the fp32 / fp16 score tables:
    // B K Tpad entries, 2 GB at B = 32, K = 131 072) are sized for the largest query of UP TO 128 tokens it has seen --
    // a longer query (per-query general path, which touches none of them) neither allocates them for 128 tokens nor
    // leaves a later short query without them
    const int64_t Ttuned = std::max(w.Ttuned, t_tuned);
    const int64_t Tpad = token_tiles(std::max<int64_t>(Ttuned, 1)) * 32;
    // candidates of one query <= sum of the T*nprobe longest IVF lists (and <= n_docs)
    size_t lists = (size_t)std::min<int64_t>(T * nprobe, s->K);
    size_t cap = 0;
    for (size_t i = 0; i < lists; ++i) cap += s->ivf_len_sorted[i];
    cap = std::min<size_t>(cap, (size_t)s->n_docs);
    w.ivf_cap = (std::max<size_t>(cap, 1) + 3) & ~(size_t)3;
    cap = std::max<size_t>(cap, std::max(filt_count, w.filt_cap));      // <= n_docs: a filter's population
    cap = std::max<size_t>(cap, 1);
    w.cand_cap = (cap + 3) & ~(size_t)3;
    w.W = (int)((s->n_docs + 31) / 32);
    w.nblk_bitmap = (w.W + kScanBlock * kWordsPerThread - 1) / (kScanBlock * kWordsPerThread);
    w.topn_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(256, s->K / 512));
    const int64_t NPs = padded_nprobe(nprobe);
    const bool general = s->generic;
    CLB_TRY(w.Qdev.ensure(sizeof(float) * B * T * s->dim));
    // the fp32 T x K score matrix is only materialised by the unfused S1/S2 path (nprobe > 2 or T > 32)
    // (the general-shape path scores its centroids into the same matrix whenever its batched kernels apply)
    const bool general_batched = general && s->dim % 4 == 0 && s->dim <= 256;
    if (Ttuned > 0 && ((!general && !(nprobe <= 2 && Ttuned <= 32)) || general_batched))
        CLB_TRY(w.cells.ensure(sizeof(float) * B * s->K * Tpad));
    if (Ttuned > 0 && (!general || general_batched))
        CLB_TRY(w.partial.ensure(sizeof(ValIdx) * B * w.topn_blocks * Tpad * std::min<int64_t>(NPs, 32)));
    CLB_TRY(w.sel.ensure(sizeof(int) * B * std::max<int64_t>(Tpad, T) * NPs));
    const size_t bm_bytes = sizeof(uint32_t) * (size_t)B * w.W;
    const bool bm_new = bm_bytes > w.bitmap.bytes || !w.bitmap.p;
    CLB_TRY(w.bitmap.ensure(bm_bytes));
    if (bm_new) CLB_HIP(hipMemsetAsync(w.bitmap.p, 0, w.bitmap.bytes, s->stream));
    CLB_TRY(w.blocksum.ensure(sizeof(int) * B * w.nblk_bitmap));
    CLB_TRY(w.ncand.ensure(sizeof(int) * B));
    CLB_TRY(w.cand.ensure(sizeof(uint32_t) * B * w.cand_cap));
    {   // slice boundaries of every selected list (mark_count_kernel<true>, shards of more than 16 slices)
        const size_t nsl = ((size_t)w.nblk_bitmap + kMarkSliceBlocks - 1) / kMarkSliceBlocks;
        const size_t nbig = ((size_t)w.nblk_bitmap + kMarkSliceBlocksBig - 1) / kMarkSliceBlocksBig;
        if (nsl > 16) CLB_TRY(w.bounds.ensure(sizeof(uint32_t) * B * T * nprobe * (nbig + 1)));
    }
    CLB_TRY(w.cand_hdr.ensure(sizeof(uint2) * B * w.cand_cap));
    CLB_TRY(w.scores.ensure(sizeof(float) * B * w.cand_cap));
    CLB_TRY(w.list.ensure(sizeof(int) * B * w.cand_cap));
    CLB_TRY(w.nlist.ensure(sizeof(int) * B));
    CLB_TRY(w.thresh.ensure(sizeof(float) * B * 2));
    CLB_TRY(w.outp.ensure(sizeof(int64_t) * B * k * std::max<int64_t>(per_group, 1)));
    CLB_TRY(w.outs.ensure(sizeof(float) * B * k * std::max<int64_t>(per_group, 1)));
    CLB_TRY(w.flags.ensure(sizeof(int) * B));
    if (!w.stats.p) {
        CLB_TRY(w.stats.ensure(sizeof(unsigned long long) * 8));
        CLB_HIP(hipMemset(w.stats.p, 0, sizeof(unsigned long long) * 8));
    }
    if (s->approx_ok && Ttuned > 0) {
        CLB_TRY(w.cells_q.ensure(approx_cells_bytes(B, s->K, Tpad)));
        CLB_TRY(w.rowmask.ensure(sizeof(unsigned long long) * 8 * B * w.cand_cap));   // [b][list position][token half][4]
        CLB_TRY(w.eps_pair.ensure(sizeof(float) * B));
        CLB_TRY(w.tokmax.ensure(sizeof(uint16_t) * 32 * B * w.cand_cap));
    }
    if (grouped || w.grouped) {     // a slot that has served a grouped call keeps these in step with its other buffers
        CLB_TRY(w.grp_list.ensure(sizeof(int) * B * w.cand_cap));
        CLB_TRY(w.grp_n.ensure(sizeof(int) * B));
        CLB_TRY(w.grp_tau.ensure(sizeof(float) * B));
        if (s->approx_ok) {
            CLB_TRY(w.grp_list2.ensure(sizeof(int) * B * w.cand_cap));
            CLB_TRY(w.grp_n2.ensure(sizeof(int) * B));
        }
        w.grouped = true;
    }
    if (per_group > 0) {            // ... and one that has returned hits, these
        CLB_TRY(w.hit_p.ensure(sizeof(int64_t) * B * k));
        CLB_TRY(w.hit_s.ensure(sizeof(float) * B * k));
        if (s->approx_ok) {
            CLB_TRY(w.hit_cut.ensure(sizeof(unsigned long long) * B * w.cand_cap));
            CLB_TRY(w.hit_run.ensure(sizeof(int) * B * w.cand_cap));
            CLB_TRY(w.hit_list.ensure(sizeof(int) * B * w.cand_cap));
            CLB_TRY(w.hit_n.ensure(sizeof(int) * B));
        }
    }
    if (prior || w.prior || list_prior || w.list_prior) {   // ... and one that has searched with a prior or list priors, this
        CLB_TRY(w.prior_tau.ensure(sizeof(float) * 2 * B));
        w.prior = true;
    }
    if (list_prior || w.list_prior) {   // ... and one that has searched with list priors, this as well
        CLB_TRY(w.slot_pos.ensure(sizeof(int) * B * w.cand_cap));
        w.list_prior = true;
    }
    if (after || w.after) {         // ... and one that has searched after a cursor, these
        CLB_TRY(w.after_list.ensure(sizeof(int) * B * w.cand_cap));
        CLB_TRY(w.after_n.ensure(sizeof(int) * B));
        CLB_TRY(w.after_tau.ensure(sizeof(float) * B));
        CLB_TRY(w.after_cur_s.ensure(sizeof(float) * B));
        CLB_TRY(w.after_cur_p.ensure(sizeof(int64_t) * B));
        w.after = true;
    }
    w.Bcap = B; w.Tcap = T; w.Ttuned = Ttuned; w.npcap = nprobe; w.kcap = k; w.mcap = per_group;
    w.filt_cap = std::max(w.filt_cap, filt_count);
    CLB_HIP(hipStreamSynchronize(s->stream));
    return CLB_OK;
}

int ensure_workspace(clb_searcher* s, Workspace& w, int64_t B, int64_t T, int64_t nprobe, int64_t k, size_t filt_count = 0,
                     bool grouped = false, int64_t per_group = 0, bool prior = false, bool after = false, bool list_prior = false) {
    const int rc = ensure_workspace_sized(s, w, B, T, nprobe, k, filt_count, grouped, per_group, prior, after, list_prior);
    if (rc) {
        w.Bcap = 0;       // some buffers may have grown and others not: the next call sizes all of them again
        // a candidate set the size of a filter that does not fit is this call's own request, not a fault of the device
        if (rc == CLB_ENOMEM && filt_count > w.filt_cap)
            return fail(CLB_EUNSUPPORTED, "no room for the candidate buffers of a filter of %zu passages (CLB_FILTER_ALL, %lld "
                                          "queries per pass): %s", filt_count, (long long)B, std::string(last_error()).c_str());
    }
    return rc;
}

template <int NP>
void launch_topn(clb_searcher* s, Workspace& w, hipStream_t st, int B, int Tpad) {
    hipLaunchKernelGGL(topn_partial_kernel<NP>, dim3(w.topn_blocks, B), dim3(256), 0, st,
                       w.cells.as<float>(), w.partial.as<ValIdx>(), (int)s->K, Tpad);
    hipLaunchKernelGGL(topn_final_kernel<NP>, dim3(B), dim3(Tpad), 0, st, w.partial.as<ValIdx>(),
                       w.sel.as<int>(), w.topn_blocks, Tpad);
}

template <int NBITS>
void launch_score_exact(clb_searcher* s, Workspace& w, hipStream_t st, const float* dQ, int B, int T, const int* list,
                        const int* nlist, int grid_x) {
    hipLaunchKernelGGL(score_exact_kernel<NBITS>, dim3(grid_x, B), dim3(256), 0, st, s->centroids.as<float>(),
                       s->weights.as<float>(), s->codes0.as<uint32_t>(), s->residuals.as<uint8_t>(),
                       w.cand_hdr.as<uint2>(), dQ, w.ncand.as<int>(), w.scores.as<float>(), T, w.cand_cap, list,
                       nlist);
}

int select_by_sort(clb_searcher* s, Workspace& w, hipStream_t st, const float* cells, size_t stride_t, size_t stride_c,
                   int T, int nprobe, int NP, int* sel_b);

// S2 from the fp32 score matrix w.cells ([b][centroid][Tpad]): the top nprobe centroids of every token of B queries to w.sel
int select_top_nprobe(clb_searcher* s, Workspace& w, hipStream_t st, int B, int T, int Tpad, int nprobe) {
    const int NPs = (int)padded_nprobe(nprobe);
    if (NPs == 2) launch_topn<2>(s, w, st, B, Tpad);
    else if (NPs == 8) launch_topn<8>(s, w, st, B, Tpad);
    else if (NPs == 32) launch_topn<32>(s, w, st, B, Tpad);
    else   // nprobe > 32: stable sort of every token's K scores (one query at a time)
        for (int b = 0; b < B; ++b)
            CLB_TRY(select_by_sort(s, w, st, w.cells.as<float>() + (size_t)b * s->K * Tpad, 1, (size_t)Tpad, T, nprobe, NPs,
                                   w.sel.as<int>() + (size_t)b * Tpad * NPs));
    return CLB_OK;
}

int mark_and_compact(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, int b0, int B, int Tpad, int NPs, bool timed);

// Candidate generation S1-S3 for the queries of q on stream st; leaves cand/ncand on the device.
int run_retrieve(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q) {
    const float* dQ = q.dQ;
    const int B = q.B, T = q.T, nprobe = q.nprobe;
    const int TT = token_tiles(T), Tpad = TT * 32;
    const int n_tiles = (int)((s->K + 31) / 32);
    const bool want_half = two_pass_mode(s, q);
    w.x1_table = false;
    w.have_range = false;
    w.cell8 = false;
    if (nprobe <= 2 && T <= 32) {
        // fused S1+S2: no fp32 score matrix; fp16 pairs only when pass 1 will gather them
        // batches of 8+ queries share each staged centroid tile between 8 queries (centroid_top_bf16x3_mq_kernel)
        // (from 6 queries: the shared-tile kernel with two idle query slots, 0.047 ms, beats six or seven per-query passes
        // over the table, 0.06-0.07 ms)
        const bool mq = B >= 6;
        const int groups = (B + kMqQueries - 1) / kMqQueries;
        int gx = mq ? std::max(1, std::min(n_tiles, std::min(256, std::max(512 / groups, 16))))
                          : std::max(1, std::min(n_tiles / 2 + 1, std::min(256, std::max(1024 / std::max(1, B), 16))));
        // 16+ queries and a score table to write: two teams of four waves per work-group, 16 queries per staged tile
        // (centroid_top_bf16x3_teams_kernel); one 8-wave work-group per CU
        const bool teams = mq && want_half && B >= kTeamQueries;
        const int team_groups = (B + kTeamQueries - 1) / kTeamQueries;
        if (teams) gx = std::max(1, std::min(n_tiles, std::min(256, std::max(256 / team_groups, 16))));
        const bool x1 = teams && single_product_table(s);
        w.x1_table = x1;
        w.cell8 = teams && cell8_rows(s);
        w.have_range = w.cell8;
        if (w.cell8) {
            CLB_TRY(w.tscale.ensure(sizeof(float4) * 32 * B));
            CLB_TRY(w.rangep.ensure(sizeof(float2) * 32 * B * gx));
            CLB_TRY(w.cells8.ensure((size_t)B * s->K * 32));
        }
        const int nslots = mq ? gx * 2 : gx * 4;
        CLB_TRY(w.partial.ensure(sizeof(ValIdx) * (size_t)B * nslots * 32 * kTopPartial));
        if (w.redo.bytes < sizeof(int) * B) {          // cumulative fallback counter (statistics only)
            CLB_TRY(w.redo.ensure(sizeof(int) * B));
            CLB_HIP(hipMemsetAsync(w.redo.p, 0, w.redo.bytes, st));
        }
        {
            Timed t(s, KID_CENTROID_SCORES, st);
            const size_t lds_b16 = 2 * 2 * 32 * kRowBytes16;
            if (teams) {
                // 66 KB of dynamic LDS: above the 64-KB default limit of a launch
                auto kern = x1 ? (w.cell8 ? centroid_top_bf16x3_teams_kernel<true, true> : centroid_top_bf16x3_teams_kernel<true, false>)
                               : (w.cell8 ? centroid_top_bf16x3_teams_kernel<false, true> : centroid_top_bf16x3_teams_kernel<false, false>);
                allow_dynamic_lds(reinterpret_cast<const void*>(kern), 2 * 2 * 32 * kRowBytes16 + 8 * 4096);
                hipLaunchKernelGGL(kern, dim3(gx, team_groups), dim3(512), lds_b16 + 8 * 4096, st,
                                   x1 ? s->cent_f16.as<uint16_t>() : s->cent_hi.as<uint16_t>(),
                                   x1 ? (const uint16_t*)nullptr : (const uint16_t*)s->cent_lo.as<uint16_t>(), dQ,
                                   w.partial.as<ValIdx>(), w.cells_q.as<uint32_t>(), (int)s->K, T, B, n_tiles,
                                   w.rangep.as<float2>());
                if (w.cell8) {     // 8-bit rows: every token's measured score range, then the table rewritten by it
                    hipLaunchKernelGGL(token_range_kernel, dim3(B), dim3(1024), 0, st, (const float2*)w.rangep.as<float2>(), gx, T,
                                       w.tscale.as<float4>());
                    hipLaunchKernelGGL(requantise_cells_kernel, dim3(std::max(1, 2048 / B), B), dim3(256), 0, st,
                                       (const uint32_t*)w.cells_q.as<uint32_t>(), (const float4*)w.tscale.as<float4>(),
                                       w.cells8.as<uint32_t>(), (int)s->K);
                }
            } else if (mq && want_half)
                hipLaunchKernelGGL(centroid_top_bf16x3_mq_kernel<true>, dim3(gx, groups), dim3(256), lds_b16 + 4 * 2048, st,
                                   s->cent_hi.as<uint16_t>(), s->cent_lo.as<uint16_t>(), dQ,
                                   w.partial.as<ValIdx>(), w.cells_q.as<uint32_t>(), (int)s->K, T, B, n_tiles);
            else if (mq)
                hipLaunchKernelGGL(centroid_top_bf16x3_mq_kernel<false>, dim3(gx, groups), dim3(256), lds_b16, st,
                                   s->cent_hi.as<uint16_t>(), s->cent_lo.as<uint16_t>(), dQ,
                                   w.partial.as<ValIdx>(), (uint32_t*)nullptr, (int)s->K, T, B, n_tiles);
            else if (want_half)
                hipLaunchKernelGGL(centroid_top_bf16x3_kernel<true>, dim3(gx, B), dim3(128), lds_b16 + 2 * 2048, st,
                                   s->cent_hi.as<uint16_t>(), s->cent_lo.as<uint16_t>(), dQ,
                                   w.partial.as<ValIdx>(), w.cells_q.as<uint32_t>(), (int)s->K, T, n_tiles);
            else
                hipLaunchKernelGGL(centroid_top_bf16x3_kernel<false>, dim3(gx, B), dim3(128), lds_b16, st,
                                   s->cent_hi.as<uint16_t>(), s->cent_lo.as<uint16_t>(), dQ,
                                   w.partial.as<ValIdx>(), (uint32_t*)nullptr, (int)s->K, T, n_tiles);
        }
        {
            Timed t(s, KID_TOPN, st);
            hipLaunchKernelGGL(top_refine_kernel, dim3(32, B), dim3(64), 0, st, w.partial.as<ValIdx>(),
                               s->centroids.as<float>(), dQ, T, (int)s->K, nslots, s->approx_consts.cn_max,
                               w.sel.as<int>(), w.redo.as<int>(), x1 ? s->dc_f16 : 0.f);
        }
    } else {
        {
            Timed t(s, KID_CENTROID_SCORES, st);
            const int gx = std::max(1, std::min(n_tiles / 2 + 1, 2048 / std::max(1, B * TT)));
            hipLaunchKernelGGL(centroid_scores_kernel, dim3(gx, B * TT), dim3(128),
                               2 * 32 * kCentTileStride * sizeof(float), st, s->centroids.as<float>(), dQ,
                               w.cells.as<float>(), (int)s->K, T, TT, n_tiles);
        }
        {
            Timed t(s, KID_TOPN, st);
            CLB_TRY(select_top_nprobe(s, w, st, B, T, Tpad, nprobe));
        }
        s->prof.chain = nullptr;   // untimed conversion below
        if (want_half)
            hipLaunchKernelGGL(cells_to_half_kernel, dim3(std::max(1, 1024 / B), B), dim3(256), 0, st,
                               w.cells.as<float>(), w.cells_q.as<uint32_t>(), (int)s->K);
    }
    return mark_and_compact(s, w, st, q, 0, B, Tpad, (int)padded_nprobe(nprobe), /*timed=*/true);
}

// the filter operand of queries b0 .. b0 + n - 1 of the sub-batch: query b0 is entry 0, as a launch over those queries counts
FilterArgs filter_args(const clb_searcher* s, const Batch& q, int b0, int n) {
    FilterArgs fa{};
    fa.live = s->live.as<uint32_t>();
    for (int i = 0; i < n && i < kFilterQueries; ++i) fa.bits[i] = q.filt[b0 + i] ? q.filt[b0 + i]->bits.as<uint32_t>() : nullptr;
    fa.all = q.filt_all;
    return fa;
}

// S3: the union of the selected IVF lists as an ascending pid list + passage headers, for the B queries from b0 on
// (w.sel, entries 0 .. B - 1 of Tpad x NPs -> cand, cand_hdr, ncand of queries b0 ...); shared by the tuned and the
// general-shape path, whose per-query loop calls it one query at a time and untimed
// FILT: some query of the launch carries a filter (S3f) -- the same launches with the filter operand; false: the
// unfiltered kernels, launched as ever
template <bool FILT>
int mark_and_compact_impl(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, int b0, int B, int Tpad, int NPs,
                          bool timed) {
    static_assert(kScanBlock * kWordsPerThread == 1024, "mark_count_kernel writes 1024-word count blocks");
    static_assert(kSubBatch <= kFilterQueries, "the filter handles of a sub-batch travel in one kernel argument block");
    FilterOperand<FILT> fa{};
    if constexpr (FILT) fa = filter_args(s, q, b0, B);
    const int T = q.T, nprobe = q.nprobe;
    uint32_t* bitmap = w.bitmap.as<uint32_t>() + (size_t)b0 * w.W;
    int* blocksum = w.blocksum.as<int>() + (size_t)b0 * w.nblk_bitmap;
    uint32_t* cand = w.cand.as<uint32_t>() + (size_t)b0 * w.cand_cap;
    uint2* cand_hdr = w.cand_hdr.as<uint2>() + (size_t)b0 * w.cand_cap;
    int* ncand = w.ncand.as<int>() + b0;
    const int nslices = (w.nblk_bitmap + kMarkSliceBlocks - 1) / kMarkSliceBlocks;
    const int nslices_big = (w.nblk_bitmap + kMarkSliceBlocksBig - 1) / kMarkSliceBlocksBig;
    // every slice re-reads the query's lists: beyond 16 slices (2 M passages per shard) that costs more than the atomics
    // it saves -- unless the lists are sorted by passage id: then slice_bounds_kernel cuts every list at the slice
    // boundaries first (binary searches) and larger slices keep the number of work-groups down.  For a few queries the
    // 64 one-list work-groups of the atomic path finish sooner (one query: 8 us against 27)
    const bool sliced = (nslices <= 16 || s->ivf_sorted) && B >= 8;
    {
        Timed t(s, timed ? KID_MARK : -1, st);
        if (sliced && nslices <= 16)     // mark + per-block counts, the bitmap slice of a work-group in LDS (no global atomics)
            hipLaunchKernelGGL((mark_count_kernel<false, kMarkSliceBlocks, FILT>), dim3(nslices, B), dim3(1024), 0, st, w.sel.as<int>(),
                               s->ivf_off.as<uint32_t>(), s->ivf_pid.as<uint32_t>(), bitmap, blocksum, T, Tpad, NPs, nprobe, w.W,
                               w.nblk_bitmap, (const uint32_t*)nullptr, fa);
        else if (sliced) {
            const int nb = T * nprobe * (nslices_big + 1);
            hipLaunchKernelGGL(slice_bounds_kernel, dim3((nb + 255) / 256, B), dim3(256), 0, st, w.sel.as<int>(),
                               s->ivf_off.as<uint32_t>(), s->ivf_pid.as<uint32_t>(), T, Tpad, NPs, nprobe, nslices_big,
                               (uint32_t)(kMarkSliceBlocksBig * 1024 * 32), w.bounds.as<uint32_t>());
            hipLaunchKernelGGL((mark_count_kernel<true, kMarkSliceBlocksBig, FILT>), dim3(nslices_big, B), dim3(1024), 0, st,
                               w.sel.as<int>(), s->ivf_off.as<uint32_t>(), s->ivf_pid.as<uint32_t>(), bitmap, blocksum, T, Tpad,
                               NPs, nprobe, w.W, w.nblk_bitmap, (const uint32_t*)w.bounds.as<uint32_t>(), fa);
        } else
            hipLaunchKernelGGL(mark_candidates_kernel<FILT>, dim3(T * nprobe, B), dim3(256), 0, st, w.sel.as<int>(),
                               s->ivf_off.as<uint32_t>(), s->ivf_pid.as<uint32_t>(), bitmap, T, Tpad, NPs, nprobe, w.W, fa);
    }
    {
        Timed t(s, timed ? KID_COMPACT : -1, st);
        if (!sliced)
            hipLaunchKernelGGL(bitmap_count_kernel<FILT>, dim3(w.nblk_bitmap, B), dim3(kScanBlock), 0, st, bitmap, blocksum, w.W, fa);
        // after the sliced marking the bitmap already holds marked AND filter: only a filter that IS the candidate set
        // (CLB_FILTER_ALL) still has to reach the emit kernel
        if (FILT && (!sliced || q.filt_all))
            hipLaunchKernelGGL(bitmap_emit_kernel<FILT>, dim3(w.nblk_bitmap, B), dim3(kScanBlock), 0, st, bitmap, blocksum, cand,
                               s->doc_off.as<uint32_t>(), cand_hdr, w.W, w.cand_cap, ncand, fa);
        else
            hipLaunchKernelGGL(bitmap_emit_kernel<false>, dim3(w.nblk_bitmap, B), dim3(kScanBlock), 0, st, bitmap, blocksum, cand,
                               s->doc_off.as<uint32_t>(), cand_hdr, w.W, w.cand_cap, ncand);
    }
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

// entries per query of slot_pos in a call with list priors: the most candidates a listed query can have (filt_now =
// min(list_stride, n_docs) <= cand_cap), so that the fill in front of list_slot_kernel touches no more than the lists can reach
inline size_t slot_pos_stride(const Batch& q) { return (std::max<size_t>(q.filt_now, 1) + 3) & ~(size_t)3; }

// S3l: the candidates of the B queries from b0 on are the caller's lists (list_kernels.hpp) -- the listed passages go into
// the candidate bitmap, and the compaction reads it through the handle's live bitmap as every query's filter word
// (CLB_FILTER_CANDIDATES: marked AND filter), which drops the passages without embeddings as CLB_FILTER_ALL drops them
int list_and_compact(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, int b0, int B, bool timed) {
    FilterArgs fa{};
    fa.live = s->live.as<uint32_t>();
    for (int i = 0; i < B && i < kFilterQueries; ++i) fa.bits[i] = fa.live;
    fa.all = 0;
    const int L = (int)q.list_stride;
    uint32_t* bitmap = w.bitmap.as<uint32_t>() + (size_t)b0 * w.W;
    int* blocksum = w.blocksum.as<int>() + (size_t)b0 * w.nblk_bitmap;
    {
        Timed t(s, timed ? KID_MARK : -1, st);
        hipLaunchKernelGGL(list_mark_kernel, dim3((L + 255) / 256, B), dim3(256), 0, st, q.d_list_pids + (size_t)b0 * L,
                           q.d_list_lens + b0, L, s->pid_offset, (int)s->n_docs, bitmap, w.W);
    }
    {
        Timed t(s, timed ? KID_COMPACT : -1, st);
        hipLaunchKernelGGL(bitmap_count_kernel<true>, dim3(w.nblk_bitmap, B), dim3(kScanBlock), 0, st, bitmap, blocksum, w.W, fa);
        hipLaunchKernelGGL(bitmap_emit_kernel<true>, dim3(w.nblk_bitmap, B), dim3(kScanBlock), 0, st, bitmap, blocksum,
                           w.cand.as<uint32_t>() + (size_t)b0 * w.cand_cap, s->doc_off.as<uint32_t>(),
                           w.cand_hdr.as<uint2>() + (size_t)b0 * w.cand_cap, w.W, w.cand_cap, w.ncand.as<int>() + b0, fa);
    }
    if (q.d_list_prior) {
        // with list priors: the lowest list position of every candidate slot (list_slot_kernel), which the boosts read the
        // values through.  A listed query has at most filt_now candidates: only that many slots of a row are filled and read
        Timed t(s, timed ? KID_COMPACT : -1, st);
        const size_t ps = slot_pos_stride(q);
        int* slot_pos = w.slot_pos.as<int>() + (size_t)b0 * ps;
        hipLaunchKernelGGL(list_slot_fill_kernel, dim3((unsigned)(((size_t)B * ps + 255) / 256)), dim3(256), 0, st, slot_pos,
                           (size_t)B * ps);
        hipLaunchKernelGGL(list_slot_kernel, dim3((L + 255) / 256, B), dim3(256), 0, st, q.d_list_pids + (size_t)b0 * L,
                           q.d_list_lens + b0, L, s->pid_offset, (int)s->n_docs, w.cand.as<uint32_t>() + (size_t)b0 * w.cand_cap,
                           w.ncand.as<int>() + b0, w.cand_cap, slot_pos, ps);
    }
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

int mark_and_compact(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, int b0, int B, int Tpad, int NPs, bool timed) {
    if (q.d_list_pids) return list_and_compact(s, w, st, q, b0, B, timed);
    bool filt = false;
    for (int b = b0; q.filt && b < b0 + B; ++b) filt |= q.filt[b] != nullptr;
    return filt ? mark_and_compact_impl<true>(s, w, st, q, b0, B, Tpad, NPs, timed)
                : mark_and_compact_impl<false>(s, w, st, q, b0, B, Tpad, NPs, timed);
}

int check_search_args(const clb_searcher* s, int64_t T, int64_t B, int64_t nprobe, int64_t k) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (T < 1) return fail(CLB_EARGUMENT, "query length must be >= 1");
    if (B < 1) return fail(CLB_EARGUMENT, "batch size must be >= 1");
    if (nprobe < 1 || nprobe > s->K) return fail(CLB_EBOUNDS, "nprobe=%lld outside 1..K=%lld (partialsortperm)", (long long)nprobe, (long long)s->K);
    if (k < 1) return fail(CLB_EBOUNDS, "k must be >= 1");
    if (T * nprobe > (int64_t)0x7fffffff / 4 || T * s->K > (int64_t)0x7fffffff) return fail(CLB_EUNSUPPORTED, "T * K too large");
    return CLB_OK;
}

// ---- general-shape pieces (generic_kernels.hpp) --------------------------------------------------------------
// top-nprobe of every token of ONE query by a stable sort of the T x K scores; sel_b: [T][NP] (0-based centroid ids)
int select_by_sort(clb_searcher* s, Workspace& w, hipStream_t st, const float* cells, size_t stride_t, size_t stride_c,
                   int T, int nprobe, int NP, int* sel_b) {
    const size_t n = (size_t)T * s->K;
    CLB_TRY(w.g_keys.ensure(sizeof(uint64_t) * n));
    CLB_TRY(w.g_keys2.ensure(sizeof(uint64_t) * n));
    CLB_TRY(w.g_vals.ensure(sizeof(uint32_t) * n));
    CLB_TRY(w.g_vals2.ensure(sizeof(uint32_t) * n));
    hipLaunchKernelGGL(generic_sel_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cells, stride_t,
                       stride_c, (int)s->K, T, w.g_keys.as<unsigned long long>(), w.g_vals.as<uint32_t>());
    CLB_TRY(sort_pairs_u64(w.g_keys.as<uint64_t>(), w.g_keys2.as<uint64_t>(), w.g_vals.as<uint32_t>(),
                           w.g_vals2.as<uint32_t>(), n, st, &w.g_sort_tmp));
    hipLaunchKernelGGL(generic_sel_extract_kernel, dim3((unsigned)((T * nprobe + 255) / 256)), dim3(256), 0, st,
                       w.g_vals2.as<uint32_t>(), (int)s->K, T, nprobe, NP, sel_b);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

// the count a search reports as n_cand: the query's candidates, or with a grouping the groups among them
inline const int* reported_count(const Workspace& w, const Batch& q) { return q.grp ? w.grp_n.as<int>() : w.ncand.as<int>(); }

// top-k of ONE query by a full stable sort (k above the single-work-group sort of topk_kernel).  The count stays on the
// device: the sort runs over the slot's candidate capacity with the positions past the count keyed to the end, the
// emit kernel writes the short-result flag and the candidate count; rocPRIM's temporary storage lives in the workspace
// slot (g_sort_tmp, sized on first use), so the sort is only enqueued -- no allocation and no host synchronisation per
// query.  The price of keeping the count on the device: the sort covers cand_cap keys, not the query's own count.
int topk_by_sort(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, int b, const int* list, const int* nlist) {
    const int k = q.k;
    const int cap = (int)w.cand_cap;
    const float* sc = w.scores.as<float>() + (size_t)b * w.cand_cap;
    const int* lst = list ? list + (size_t)b * w.cand_cap : nullptr;
    const int* n_ptr = list ? nlist + b : w.ncand.as<int>() + b;
    CLB_TRY(w.g_keys.ensure(sizeof(uint64_t) * std::max(cap, 1)));
    CLB_TRY(w.g_keys2.ensure(sizeof(uint64_t) * std::max(cap, 1)));
    hipLaunchKernelGGL(generic_topk_keys_kernel, dim3((cap + 255) / 256), dim3(256), 0, st, sc, lst, n_ptr, cap,
                       w.g_keys.as<unsigned long long>());
    CLB_TRY(sort_keys_u64(w.g_keys.as<uint64_t>(), w.g_keys2.as<uint64_t>(), (size_t)cap, st, &w.g_sort_tmp));
    hipLaunchKernelGGL(generic_topk_emit_kernel, dim3((std::max(k, 1) + 255) / 256), dim3(256), 0, st,
                       w.g_keys2.as<unsigned long long>(), sc, w.cand.as<uint32_t>() + (size_t)b * w.cand_cap, lst, n_ptr,
                       reported_count(w, q) + b, k, s->pid_offset, q.d_out_pids + (size_t)b * k, q.d_out_scores + (size_t)b * k,
                       w.flags.as<int>() + b, q.d_n_cand ? q.d_n_cand + b : nullptr);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

// S7g-a for queries b0 .. b0 + n - 1 (group_collapse_kernel): the best slot of every group among the listed slots (list /
// nlist, [B][cand_cap] / [B]) or, with list == nullptr, among all candidates, to out_list / out_n of the same layout
void launch_collapse(Workspace& w, hipStream_t st, const Batch& q, int b0, int n, const int* list, const int* nlist,
                     int* out_list, int* out_n) {
    hipLaunchKernelGGL(group_collapse_kernel, dim3(n), dim3(1024), 0, st, w.scores.as<float>() + (size_t)b0 * w.cand_cap,
                       w.cand.as<uint32_t>() + (size_t)b0 * w.cand_cap, w.ncand.as<int>() + b0,
                       list ? list + (size_t)b0 * w.cand_cap : nullptr, list ? nlist + b0 : nullptr, q.grp->gid.as<uint32_t>(),
                       w.cand_cap, out_list + (size_t)b0 * w.cand_cap, out_n + b0);
}

// the global group index of every result pid and the edge groups of every query's candidate list (group_result_kernel)
void launch_result_groups(const clb_searcher* s, Workspace& w, hipStream_t st, const clb_grouping* g, int64_t group_base,
                          const int64_t* d_pids, int B, int k, int64_t* d_out_gids, int64_t* d_edge_gids) {
    const int64_t n = std::max<int64_t>((int64_t)B * k, B);
    hipLaunchKernelGGL(group_result_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_pids, B, k, s->pid_offset,
                       g->gid.as<uint32_t>(), s->n_docs, group_base, w.cand.as<uint32_t>(), w.ncand.as<int>(), w.cand_cap,
                       d_out_gids, d_edge_gids);
}

// S7g-f for queries b0 .. b0 + n - 1 of a call with hits (group_hits_kernel; nothing otherwise): the per_group best passages
// of every result among the exact-scored set -- the re-scored list (list / nlist) or, with list == nullptr, all candidates
void launch_hits(const clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, int b0, int n, const int* list,
                 const int* nlist) {
    if (q.per_group <= 0) return;
    const int64_t waves = (int64_t)n * q.k;
    hipLaunchKernelGGL(group_hits_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st,
                       w.scores.as<float>() + (size_t)b0 * w.cand_cap, w.cand.as<uint32_t>() + (size_t)b0 * w.cand_cap,
                       w.ncand.as<int>() + b0, list ? list + (size_t)b0 * w.cand_cap : nullptr, list ? nlist + b0 : nullptr,
                       q.grp->gid.as<uint32_t>(), s->n_docs, q.d_out_pids + (size_t)b0 * q.k, n, q.k, q.per_group, w.cand_cap,
                       s->pid_offset, q.d_hit_pids + (size_t)b0 * q.k * q.per_group, q.d_hit_scores + (size_t)b0 * q.k * q.per_group);
}

// S7 for queries b0 .. b0 + n - 1: the single-work-group select + sort of topk_kernel, one work-group per query, or for
// k above it a full stable sort per query.  list / nlist: the two-pass mode's re-scored passages ([B][cand_cap] / [B]) or
// nullptr; ranked: topk_rank_kernel has already written the queries with short lists
int launch_topk(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, int b0, int n, const int* list, const int* nlist,
                int ranked) {
    if (q.k > kMaxTopK) {
        for (int b = b0; b < b0 + n; ++b) CLB_TRY(topk_by_sort(s, w, st, q, b, list, nlist));
        return CLB_OK;
    }
    const int kpow2 = next_pow2(q.k);
    allow_large_topk_lds();
    hipLaunchKernelGGL(topk_kernel, dim3(n), dim3(1024), sizeof(unsigned long long) * kpow2, st,
                       w.scores.as<float>() + (size_t)b0 * w.cand_cap, w.cand.as<uint32_t>() + (size_t)b0 * w.cand_cap,
                       reported_count(w, q) + b0, list ? list + (size_t)b0 * w.cand_cap : nullptr, list ? nlist + b0 : nullptr, q.k, kpow2,
                       w.cand_cap, s->pid_offset, q.d_out_pids + (size_t)b0 * q.k, q.d_out_scores + (size_t)b0 * q.k,
                       w.flags.as<int>() + b0, q.d_n_cand ? q.d_n_cand + b0 : nullptr, ranked);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

// P1 for queries b0 .. b0 + n - 1 of a call with a prior (prior_boost_kernel; nothing otherwise): the scores of the listed
// slots (list / nlist) or, with list == nullptr, of all candidates become score + weight * value; mabs: prior_tau's M, or nullptr
// With list priors (q.d_list_prior, never together with q.prior) the same kernel reads the term of a slot from the query's row
// of the value block, at the position list_slot_kernel left in slot_pos.
void launch_boost(Workspace& w, hipStream_t st, const Batch& q, int b0, int n, const int* list, const int* nlist, float* mabs) {
    if (!q.prior && !q.d_list_prior) return;
    float* scores = w.scores.as<float>() + (size_t)b0 * w.cand_cap;
    const uint32_t* cand = w.cand.as<uint32_t>() + (size_t)b0 * w.cand_cap;
    const int* l = list ? list + (size_t)b0 * w.cand_cap : nullptr;
    const int* nl = list ? nlist + b0 : nullptr;
    if (q.prior) {
        hipLaunchKernelGGL(prior_boost_kernel<false>, dim3(n), dim3(1024), 0, st, scores, cand, w.ncand.as<int>() + b0, l, nl,
                           PriorTerm{q.prior->values.as<float>(), nullptr, 0, 0}, q.prior_weight, w.cand_cap,
                           mabs ? mabs + b0 : nullptr);
        return;
    }
    const size_t ps = slot_pos_stride(q);
    hipLaunchKernelGGL(prior_boost_kernel<true>, dim3(n), dim3(1024), 0, st, scores, cand, w.ncand.as<int>() + b0, l, nl,
                       PriorTerm{q.d_list_prior + (size_t)b0 * q.list_stride, w.slot_pos.as<int>() + (size_t)b0 * ps,
                                 (int)q.list_stride, ps},
                       q.prior_weight, w.cand_cap, mabs ? mabs + b0 : nullptr);
}

// A2 for queries b0 .. b0 + n - 1 of a call with cursors (after_filter_kernel): of the listed slots (list / nlist) or, with
// list == nullptr, of all candidates, those after the query's cursor go to the slot's after_list / after_n, which the top-k
// forms then rank.  The cursor arrays of q belong to the sub-batch, as list / nlist do.
void launch_after(const clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, int b0, int n, const int* list,
                  const int* nlist) {
    hipLaunchKernelGGL(after_filter_kernel, dim3(n), dim3(1024), 0, st, w.scores.as<float>() + (size_t)b0 * w.cand_cap,
                       w.cand.as<uint32_t>() + (size_t)b0 * w.cand_cap, w.ncand.as<int>() + b0,
                       list ? list + (size_t)b0 * w.cand_cap : nullptr, list ? nlist + b0 : nullptr, q.d_after_s + b0,
                       q.d_after_p + b0, w.cand_cap, s->pid_offset, w.after_list.as<int>() + (size_t)b0 * w.cand_cap,
                       w.after_n.as<int>() + b0);
}

// L2 for queries b0 .. b0 + n - 1 of a call that asks for list scores (list_scores_kernel; nothing otherwise), behind the
// exact scores of all their candidates and the boost of a prior
void launch_list_scores(const clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, int b0, int n) {
    if (!q.d_list_scores) return;
    const int L = (int)q.list_stride;
    hipLaunchKernelGGL(list_scores_kernel, dim3((L + 255) / 256, n), dim3(256), 0, st, q.d_list_pids + (size_t)b0 * L,
                       q.d_list_lens + b0, L, s->pid_offset, (int)s->n_docs, w.cand.as<uint32_t>() + (size_t)b0 * w.cand_cap,
                       w.ncand.as<int>() + b0, w.scores.as<float>() + (size_t)b0 * w.cand_cap, w.cand_cap,
                       q.d_list_scores + (size_t)b0 * L);
}

// S7 of the general-shape path for queries b0 .. b0 + n - 1, the exact scores of all their candidates in place (with a
// prior: boosted first; with cursors: the candidates after them) -- with a grouping: one collapse, then the top-k forms
// rank its list
int topk_of(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, int b0, int n) {
    launch_boost(w, st, q, b0, n, nullptr, nullptr, nullptr);
    launch_list_scores(s, w, st, q, b0, n);
    if (q.d_after_s) {
        launch_after(s, w, st, q, b0, n, nullptr, nullptr);
        return launch_topk(s, w, st, q, b0, n, w.after_list.as<int>(), w.after_n.as<int>(), 0);
    }
    if (!q.grp) return launch_topk(s, w, st, q, b0, n, nullptr, nullptr, 0);
    launch_collapse(w, st, q, b0, n, nullptr, nullptr, w.grp_list.as<int>(), w.grp_n.as<int>());
    CLB_TRY(launch_topk(s, w, st, q, b0, n, w.grp_list.as<int>(), w.grp_n.as<int>(), 0));
    launch_hits(s, w, st, q, b0, n, nullptr, nullptr);
    return CLB_OK;
}

// S1-S3 of query b of the sub-batch on the general-shape path: leaves cand / cand_hdr / ncand of slot b
int run_retrieve_general(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, int b) {
    const int T = q.T, nprobe = q.nprobe;
    CLB_TRY(w.g_cells.ensure(sizeof(float) * (size_t)T * s->K));
    hipLaunchKernelGGL(generic_cells_kernel, dim3((unsigned)((s->K + 127) / 128), T), dim3(128), sizeof(float) * s->dim, st,
                       s->centroids.as<float>(), q.dQ + (size_t)b * T * s->dim, (int)s->dim, (int)s->K, w.g_cells.as<float>());
    // one query at a time: slot 0 of the selection buffer, rows of nprobe entries for T tokens
    CLB_TRY(select_by_sort(s, w, st, w.g_cells.as<float>(), (size_t)s->K, 1, T, nprobe, nprobe, w.sel.as<int>()));
    return mark_and_compact(s, w, st, q, b, 1, /*Tpad=*/T, /*NPs=*/nprobe, /*timed=*/false);
}

// S1..S3 of B queries on the general-shape path when the shape allows the batched kernels: fp32-MFMA centroid scores in
// the tuned path's [b][centroid][Tpad] layout, then the tuned path's own selection, marking and compaction
bool general_batched_ok(const clb_searcher* s, int T) { return s->dim % 4 == 0 && s->dim <= 256 && T <= 128; }

int run_retrieve_general_batched(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q) {
    const int Tpad = token_tiles(q.T) * 32;
    auto cells_kernel = s->dim <= 128 ? generic_cells_mfma_kernel<32> : generic_cells_mfma_kernel<64>;
    hipLaunchKernelGGL(cells_kernel, dim3((unsigned)((s->K + 63) / 64), (unsigned)q.B), dim3(256), 0, st, s->centroids.as<float>(),
                       q.dQ, (int)s->dim, (int)s->K, q.T, Tpad, w.cells.as<float>());
    CLB_TRY(select_top_nprobe(s, w, st, q.B, q.T, Tpad, q.nprobe));
    return mark_and_compact(s, w, st, q, 0, q.B, Tpad, (int)padded_nprobe(q.nprobe), /*timed=*/true);
}

// the whole search of B queries on the general-shape path (exact scoring only)
int run_search_general(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q) {
    const float* dQ = q.dQ;
    const int B = q.B, T = q.T;
    s->prof.chain = nullptr;
    if (general_batched_ok(s, T)) {
        // batched: every stage is one launch for the B queries (the loop below: ~12 launches per query, the scoring
        // kernel a chain of dependent loads)
        CLB_TRY(run_retrieve_general_batched(s, w, st, q));
        const dim3 grid((unsigned)std::max(64, 2048 / std::max(1, B)), (unsigned)B);
        const size_t lds = sizeof(float) * (((size_t)1 << s->nbits) + (size_t)T * (s->dim + 1));   // <= 133 KB (T 128, dim 256)
        if (lds > 64 * 1024) {
            allow_dynamic_lds(reinterpret_cast<const void*>(generic_score_mfma_fast_kernel<32>), (int)lds);
            allow_dynamic_lds(reinterpret_cast<const void*>(generic_score_mfma_fast_kernel<64>), (int)lds);
        }
        auto score_kernel = s->dim <= 128 ? generic_score_mfma_fast_kernel<32> : generic_score_mfma_fast_kernel<64>;
        hipLaunchKernelGGL(score_kernel, grid, dim3(256), lds, st, s->centroids.as<float>(), s->weights.as<float>(),
                           s->codes0.as<uint32_t>(), s->residuals.as<uint8_t>(), w.cand_hdr.as<uint2>(), w.ncand.as<int>(), dQ,
                           (int)s->dim, s->nbits, T, w.cand_cap, w.scores.as<float>());
        CLB_HIP(hipGetLastError());
        return topk_of(s, w, st, q, 0, B);
    }
    const int grid = 1024;
    const size_t max_len = (size_t)std::max<int64_t>(s->max_doclen, 1);
    CLB_TRY(w.g_scratch.ensure(sizeof(float) * grid * max_len * s->dim));
    for (int b = 0; b < B; ++b) {
        CLB_TRY(run_retrieve_general(s, w, st, q, b));
        if (T <= 16 * kGenericMaxTokenGroups && s->dim % 4 == 0)
            // fp32 MFMA, one wave per passage (the canonical arithmetic of the scalar kernel, bit for bit)
            hipLaunchKernelGGL(generic_score_mfma_kernel, dim3(grid), dim3(256), sizeof(float) * ((size_t)1 << s->nbits), st,
                               s->centroids.as<float>(), s->weights.as<float>(), s->codes0.as<uint32_t>(),
                               s->residuals.as<uint8_t>(), w.cand_hdr.as<uint2>() + (size_t)b * w.cand_cap,
                               w.ncand.as<int>() + b, dQ + (size_t)b * T * s->dim, (int)s->dim, s->nbits, T,
                               w.scores.as<float>() + (size_t)b * w.cand_cap);
        else
            hipLaunchKernelGGL(generic_score_kernel, dim3(grid), dim3(256), sizeof(float) * T, st, s->centroids.as<float>(),
                               s->weights.as<float>(), s->codes0.as<uint32_t>(), s->residuals.as<uint8_t>(),
                               w.cand_hdr.as<uint2>() + (size_t)b * w.cand_cap, w.ncand.as<int>() + b,
                               dQ + (size_t)b * T * s->dim, (int)s->dim, s->nbits, T, w.g_scratch.as<float>(), max_len,
                               w.scores.as<float>() + (size_t)b * w.cand_cap);
        CLB_HIP(hipGetLastError());
        CLB_TRY(topk_of(s, w, st, q, b, 1));
    }
    return CLB_OK;
}

// tau and the list {approx >= tau - 2 eps} of every query of the batch (two-pass mode).  One work-group per query keeps
// up to 32 768 candidates in registers; shards whose queries can have several times that (candidate capacity >= 131 072:
// roughly 3 M passages and up) take the wide selection -- kWideBlocks work-groups per query, one launch per radix pass.
constexpr size_t kWideSelectCap = 131072;

// Pass 1 over every candidate of the batch: the gather form by the index's code statistics, the row format by the batch's table
void launch_pass1(clb_searcher* s, Workspace& w, hipStream_t st, const float* dQ, dim3 grid, int B, int T) {
    auto kern = w.cell8 ? (s->gather_lds ? score_approx32_kernel<false, 1, true> : score_approx32_kernel<false, 0, true>)
                        : (s->gather_lds ? score_approx32_kernel<false, 1, false> : score_approx32_kernel<false, 0, false>);
    hipLaunchKernelGGL(kern, grid, dim3(kApproxThreads), 0, st, s->weights.as<float>(),
                       s->codeinv.as<uint32_t>(), s->residuals.as<uint8_t>(), s->cbits, s->inv_lo, s->inv_step, dQ,
                       w.cell8 ? w.cells8.as<uint32_t>() : w.cells_q.as<uint32_t>(), w.cand_hdr.as<uint2>(), w.ncand.as<int>(),
                       w.scores.as<float>(), (int)s->K, T, B, w.cand_cap, w.tokmax.as<uint16_t>(), (const int*)nullptr,
                       (const int*)nullptr, (const float*)nullptr, (unsigned long long*)nullptr,
                       (const float4*)w.tscale.as<float4>());
}
// The centroid side of the single-product score table in the error bound: when this batch's table was made that way -- and,
// on a shard of a group, whenever a shard MAY make its tables that way (the threshold tau comes from every shard's
// approximate scores, so one bound has to cover them all; set clb_searcher_set_centroid_products alike on all shards).
inline float bound_dc(const clb_searcher* s, const Workspace& w) {
    return (w.x1_table || (s->bounds_synced && s->s1_x1 != 0 && s->cent_f16.p)) ? s->dc_f16 : 0.f;
}
// What every kernel that evaluates the error bound of this batch takes: the handle's constants with that centroid term, the
// score ranges the batched centroid kernel measured (or none) and the row format of the score table
struct BoundOperands { ApproxConsts ac; const float4* tscale; int cell8; };
inline BoundOperands bound_operands(const clb_searcher* s, const Workspace& w) {
    ApproxConsts ac = s->approx_consts;
    ac.dc_max = bound_dc(s, w);
    return {ac, w.have_range ? (const float4*)w.tscale.as<float4>() : (const float4*)nullptr, w.cell8 ? 1 : 0};
}
int launch_select(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q, const float* tau_in, bool coarse_tau = false) {
    const float* dQ = q.dQ;
    const int B = q.B, T = q.T, k = q.k;
    // by the most candidates a query of THIS sub-batch can have: a slot that once grew for a large CLB_FILTER_ALL set
    // goes on selecting its unfiltered batches as before
    const size_t most = std::max(w.ivf_cap, q.filt_now);
    const bool wide = s->wide_select == 1 || (s->wide_select < 0 && most >= kWideSelectCap);
    const BoundOperands bo = bound_operands(s, w);
    if (!wide) {
        hipLaunchKernelGGL(select_margin_kernel, dim3(B), dim3(1024), 0, st, w.scores.as<float>(), w.ncand.as<int>(), dQ, T, k,
                           w.cand_cap, bo.ac, w.list.as<int>(), w.nlist.as<int>(), w.thresh.as<float>(),
                           w.eps_pair.as<float>(), tau_in, coarse_tau ? 1 : 0, bo.tscale, bo.cell8);
        return CLB_OK;
    }
    CLB_TRY(w.wsel.ensure(sizeof(WideSel) * B));
    CLB_HIP(hipMemsetAsync(w.wsel.p, 0, sizeof(WideSel) * B, st));
    const dim3 grid(kWideBlocks, B);
    hipLaunchKernelGGL(wide_minmax_kernel, grid, dim3(1024), 0, st, w.scores.as<float>(), w.ncand.as<int>(), dQ, T, w.cand_cap,
                       bo.ac, w.wsel.as<WideSel>(), w.eps_pair.as<float>(), bo.tscale, bo.cell8);
    if (!tau_in)
        for (int pass = 0; pass < 4; ++pass)
            hipLaunchKernelGGL(wide_hist_kernel, grid, dim3(1024), 0, st, w.scores.as<float>(), w.ncand.as<int>(), k, w.cand_cap,
                               w.wsel.as<WideSel>(), pass);
    hipLaunchKernelGGL(wide_count_kernel, grid, dim3(1024), 0, st, w.scores.as<float>(), w.ncand.as<int>(), k, w.cand_cap,
                       w.wsel.as<WideSel>(), tau_in);
    hipLaunchKernelGGL(wide_emit_kernel, grid, dim3(1024), 0, st, w.scores.as<float>(), w.ncand.as<int>(), k, w.cand_cap,
                       (const WideSel*)w.wsel.as<WideSel>(), tau_in, w.list.as<int>(), w.nlist.as<int>(), w.thresh.as<float>());
    return CLB_OK;
}

// The whole search for the B device-resident queries of q, enqueued on st.
// phase 0: the whole search.  Sharded search in two calls (clb_search_shard_phase1/2, two-pass mode only):
// phase 1 = candidate generation, pass 1, local selection, and the shard's k largest approximate scores per query
// to `d_local_top`; phase 2 = global tau from the gathered scores `d_all_top` ([n_shards][B][k]), selection at that
// tau, pass 2, top-k.  Phase 2 continues on the workspace phase 1 left behind.
// With a grouping (q.grp) the phases exchange GROUPS: phase 1 publishes the best approximate score and the global index of the
// shard's k best groups (d_local_top / d_local_gid), phase 2 cuts at the k-th best DISTINCT group of the gathered records and
// adds what the grouped merge needs to its result (d_out_gids / d_edge_gids).
// With a prior (q.prior) in the phases: phase 1 boosts every candidate's approximate score first and publishes, beside the k
// largest BOOSTED scores (or groups), the largest of them by magnitude (d_local_mabs); phase 2 cuts at the gathered threshold
// lowered by the rounding slack at the largest magnitude of ALL shards (d_all_mabs, prior_global_tau_kernel) and boosts the
// re-scored list in front of the ranking, as phase 0 does.
int run_search(clb_searcher* s, Workspace& w, hipStream_t st, const Batch& q) {
    const float* dQ = q.dQ;
    const int B = q.B, T = q.T, k = q.k, phase = q.phase;
    const bool two_pass = two_pass_mode(s, q);
    if (phase != 0 && !two_pass) return fail(CLB_EUNSUPPORTED, "the two-phase sharded search needs the two-pass mode");
    if (s->generic || T > 128) return run_search_general(s, w, st, q);
    s->prof.chain = nullptr;           // the first timed kernel of a call records its own start
    if (phase == 2) {
        CLB_TRY(w.tau_glob.ensure(sizeof(float) * B));
        if (q.prior) {  // the k-th largest BOOSTED score (the k-th best group's) over the shards, lowered by the rounding slack at
                        // the largest magnitude any shard saw (prior_global_tau_kernel)
            const BoundOperands bo = bound_operands(s, w);
            hipLaunchKernelGGL(prior_global_tau_kernel, dim3(B), dim3(1024), 0, st, q.d_all_top, q.d_all_gid, q.d_all_mabs,
                               q.n_shards, B, k, (const float*)nullptr, dQ, T, bo.ac, bo.tscale, bo.cell8, w.tau_glob.as<float>());
        } else if (q.grp)      // the k-th best GROUP over the shards: a group that straddles a cut counts once
            hipLaunchKernelGGL(group_global_tau_kernel, dim3(B), dim3(1024), 0, st, q.d_all_top, q.d_all_gid, q.n_shards, B, k,
                               w.tau_glob.as<float>());
        else
            hipLaunchKernelGGL(global_tau_kernel, dim3(B), dim3(1024), 0, st, q.d_all_top, q.n_shards, B, k, w.tau_glob.as<float>());
        Timed t(s, KID_SELECT, st);
        CLB_TRY(launch_select(s, w, st, q, (const float*)w.tau_glob.as<float>()));
    } else {
        CLB_TRY(run_retrieve(s, w, st, q));
        if (s->prof.counters) {
            // one set of counters per CALL: the sub-batches of a large batch add onto those of the sub-batches before them
            if (!q.stats_keep) CLB_HIP(hipMemsetAsync(w.stats.p, 0, sizeof(unsigned long long) * 8, st));
            s->prof.chain = nullptr;
        }
        if (two_pass) {
            {
                Timed t(s, KID_SCORE_APPROX, st);
                constexpr int kWgPerGroup = 32;   // x 8 XCD groups: one 12-wave work-group per CU
                // Grid: XCD-affine 1-D launch (all work-groups of an XCD share one query's score table in L2) for
                // large candidate sets; for small ones (a shard of a multi-GPU run: < ~6 k candidate passages per
                // query, estimated from the mean IVF list) a (G, B) launch whose few waves per query each get a long
                // run of passages -- the pipeline fill otherwise dominates.
                const double est_cand = 0.5 * T * q.nprobe * (double)s->n_emb / (double)std::max<int64_t>(1, s->K);
                // work-groups per query of the (G, B) launch (0 = the 1-D launch): enough to fill the chip for small batches,
                // eight for large ones (measured at 4 and 8 shards, B = 8 ... 256: one or two per query cost 12 % of the pass
                // at B = 256, sixteen and more cost as much at B = 32)
                const int gxq = est_cand < 6000.0 ? std::max(8, 256 / B) : 0;
                const dim3 approx_grid = gxq > 0 && B > 1 ? dim3(gxq, B) : dim3(8 * kWgPerGroup);
                launch_pass1(s, w, st, dQ, approx_grid, B, T);
            }
            if ((q.prior || q.d_list_prior) && phase == 0) {
                // with a prior or list priors (the whole search): the selection cuts on the BOOSTED approximate scores, at their
                // k-th largest -- with a grouping the k-th best group's -- lowered by the rounding slack (prior_tau_kernel, DESIGN
                // section 5)
                Timed t(s, KID_SELECT, st);
                float* ptau = w.prior_tau.as<float>();
                float* mabs = ptau + w.Bcap;
                launch_boost(w, st, q, 0, B, nullptr, nullptr, mabs);
                if (q.grp) launch_collapse(w, st, q, 0, B, nullptr, nullptr, w.grp_list.as<int>(), w.grp_n.as<int>());
                const BoundOperands bo = bound_operands(s, w);
                hipLaunchKernelGGL(prior_tau_kernel, dim3(B), dim3(1024), 0, st, w.scores.as<float>(), w.ncand.as<int>(),
                                   q.grp ? (const int*)w.grp_list.as<int>() : (const int*)nullptr,
                                   q.grp ? (const int*)w.grp_n.as<int>() : (const int*)nullptr, k, w.cand_cap, (const float*)mabs,
                                   dQ, T, bo.ac, bo.tscale, bo.cell8, ptau);
                CLB_TRY(launch_select(s, w, st, q, (const float*)ptau));
            } else if (q.d_after_s) {
                // with cursors (phase 0 only): the cut sits at the k-th largest approximate score of the candidates that are
                // SURELY after the cursor, and those surely before it leave the selection (after_cut_kernel)
                Timed t(s, KID_SELECT, st);
                const BoundOperands bo = bound_operands(s, w);
                hipLaunchKernelGGL(after_cut_kernel, dim3(B), dim3(1024), 0, st, w.scores.as<float>(), w.ncand.as<int>(), k,
                                   w.cand_cap, q.d_after_s, dQ, T, bo.ac, bo.tscale, bo.cell8, w.after_tau.as<float>());
                CLB_TRY(launch_select(s, w, st, q, (const float*)w.after_tau.as<float>()));
            } else {
                Timed t(s, KID_SELECT, st);
                // phase 1 with a prior: everything below works on A = fl(a + pi), and the shard's largest |A| travels with it
                if (phase == 1) launch_boost(w, st, q, 0, B, nullptr, nullptr, q.d_local_mabs);
                if (q.grp && phase == 1) {
                    // grouped phase 1: the shard's k best groups by approximate score, with their global indices; the
                    // selection waits for the threshold of phase 2
                    launch_collapse(w, st, q, 0, B, nullptr, nullptr, w.grp_list.as<int>(), w.grp_n.as<int>());
                    hipLaunchKernelGGL(group_local_top_kernel, dim3(B), dim3(1024), 0, st, w.scores.as<float>(),
                                       w.cand.as<uint32_t>(), w.grp_list.as<int>(), w.grp_n.as<int>(), q.grp->gid.as<uint32_t>(),
                                       q.group_base, k, w.cand_cap, q.d_local_top, q.d_local_gid);
                    CLB_HIP(hipGetLastError());
                    return CLB_OK;
                }
                if (q.grp) {
                    // grouped: the cut is at the k-th best GROUP by approximate score -- the best
                    // approximate score of every group, their k-th largest, and the unchanged selection at that tau
                    launch_collapse(w, st, q, 0, B, nullptr, nullptr, w.grp_list.as<int>(), w.grp_n.as<int>());
                    hipLaunchKernelGGL(group_tau_kernel, dim3(B), dim3(1024), 0, st, w.scores.as<float>(), w.grp_list.as<int>(),
                                       w.grp_n.as<int>(), k, w.cand_cap, w.grp_tau.as<float>());
                    CLB_TRY(launch_select(s, w, st, q, (const float*)w.grp_tau.as<float>()));
                    // hits: the list grows by the passages that can be among the per_group best of a listed group
                    if (q.per_group > 0)
                        hipLaunchKernelGGL(group_extend_kernel, dim3(B), dim3(1024), 0, st, w.scores.as<float>(),
                                           w.cand.as<uint32_t>(), w.ncand.as<int>(), q.grp->gid.as<uint32_t>(),
                                           w.thresh.as<float>(), q.per_group, w.cand_cap, w.hit_cut.as<unsigned long long>(),
                                           w.hit_run.as<int>(), w.hit_list.as<int>(), w.hit_n.as<int>());
                } else
                    CLB_TRY(launch_select(s, w, st, q, nullptr, /*coarse_tau=*/phase == 0));
            }
        }
    }
    // two-pass mode: only the selected passages go on
    const bool extended = two_pass && q.grp && q.per_group > 0 && phase == 0;     // group_extend_kernel has left its own list
    const int* list = two_pass ? (extended ? w.hit_list.as<int>() : w.list.as<int>()) : nullptr;
    const int* nlist = two_pass ? (extended ? w.hit_n.as<int>() : w.nlist.as<int>()) : nullptr;
    if (phase == 1) {
        hipLaunchKernelGGL(local_top_kernel, dim3(B), dim3(1024), 0, st, w.scores.as<float>(), list, nlist,
                           w.thresh.as<float>(), k, w.cand_cap, q.d_local_top);
        CLB_HIP(hipGetLastError());
        return CLB_OK;
    }
    const bool subset = list != nullptr;   // two-pass mode: re-score only the rows that matter
    if (subset) {
        Timed t(s, KID_ROWS, st);
        // the pass-1 pipeline again, over the listed passages only: marks the rows that can hold a token maximum
        constexpr int kRowsGx = 256;
        const dim3 rows_grid = B > 1 ? dim3(std::max(1, kRowsGx / B), B) : dim3(8 * 32);
        // (the row sweep keeps the VGPR gather: its ~1 200 passages per query are faster with it on every workload measured)
        auto rows_kernel = w.cell8 ? score_approx32_kernel<true, 0, true> : score_approx32_kernel<true, 0, false>;
        hipLaunchKernelGGL(rows_kernel, rows_grid, dim3(kApproxThreads), 0, st, s->weights.as<float>(),
                           s->codeinv.as<uint32_t>(), s->residuals.as<uint8_t>(), s->cbits, s->inv_lo, s->inv_step, dQ,
                           w.cell8 ? w.cells8.as<uint32_t>() : w.cells_q.as<uint32_t>(), w.cand_hdr.as<uint2>(), w.ncand.as<int>(),
                           w.scores.as<float>(), (int)s->K, T, B, w.cand_cap, w.tokmax.as<uint16_t>(), list, nlist,
                           w.eps_pair.as<float>(), w.rowmask.as<unsigned long long>(), (const float4*)w.tscale.as<float4>());
    }
    {
        Timed t(s, KID_SCORE_EXACT, st);
        const int gx = list ? std::max(1, 1024 / B) : std::max(1, 2048 / B);
        constexpr int kFlatGx = 768;   // one resident round at 3 work-groups per CU
        if (subset)
            hipLaunchKernelGGL(score_exact_flat_kernel, dim3(std::max(1, kFlatGx / B), B), dim3(256), 0, st, s->centroids.as<float>(),
                               s->weights.as<float>(), s->codes0.as<uint32_t>(), s->residuals.as<uint8_t>(),
                               w.cand_hdr.as<uint2>(), dQ, w.scores.as<float>(), T, w.cand_cap, list, nlist,
                               w.rowmask.as<unsigned long long>());
        else
            switch (s->nbits) {
                case 1: launch_score_exact<1>(s, w, st, dQ, B, T, list, nlist, gx); break;
                case 2: launch_score_exact<2>(s, w, st, dQ, B, T, list, nlist, gx); break;
                case 4: launch_score_exact<4>(s, w, st, dQ, B, T, list, nlist, gx); break;
                default: return fail(CLB_EUNSUPPORTED, "nbits=%d not supported by the HIP search path", s->nbits);
            }
    }
    // what S7 ranks: the re-scored passages (two-pass mode) or all candidates -- with a grouping, the best of every group
    // among them by exact score (two-pass mode: grp_n, the group count of ALL candidates, stays what the call reports)
    const int* tlist = list;
    const int* tnlist = nlist;
    auto collapse_exact = [&]() {
        launch_boost(w, st, q, 0, B, list, nlist, nullptr);     // with a prior: the exact scores become E = e + weight * value
        launch_list_scores(s, w, st, q, 0, B);                  // (a call with list scores is the exact pass: list == nullptr)
        if (q.d_after_s) {      // with cursors (never with a grouping): only what lies after them is ranked
            launch_after(s, w, st, q, 0, B, list, nlist);
            tlist = w.after_list.as<int>(); tnlist = w.after_n.as<int>();
        }
        if (!q.grp) return;
        int* gl = list ? w.grp_list2.as<int>() : w.grp_list.as<int>();
        int* gn = list ? w.grp_n2.as<int>() : w.grp_n.as<int>();
        launch_collapse(w, st, q, 0, B, list, nlist, gl, gn);
        tlist = gl; tnlist = gn;
    };
    if (k <= kMaxTopK) {
        Timed t(s, KID_TOPK, st);
        collapse_exact();
        // two-pass mode: the ~1.2 k listed passages of a query are ranked by kRankBlocks work-groups (no sorting network);
        // a query whose list is longer than kRankMax falls through to the one-work-group select + sort
        const int ranked = tlist != nullptr;
        if (ranked)
            hipLaunchKernelGGL(topk_rank_kernel, dim3(kRankBlocks, B), dim3(1024), 0, st, w.scores.as<float>(),
                               w.cand.as<uint32_t>(), reported_count(w, q), tlist, tnlist, k, w.cand_cap, s->pid_offset,
                               q.d_out_pids, q.d_out_scores, w.flags.as<int>(), q.d_n_cand);
        CLB_TRY(launch_topk(s, w, st, q, 0, B, tlist, tnlist, ranked));
    } else {      // k above the single-work-group sort: a full stable sort per query, untimed
        s->prof.chain = nullptr;
        collapse_exact();
        CLB_TRY(launch_topk(s, w, st, q, 0, B, tlist, tnlist, 0));
    }
    if (q.grp) launch_hits(s, w, st, q, 0, B, list, nlist);
    if (q.grp && q.d_out_gids) launch_result_groups(s, w, st, q.grp, q.group_base, q.d_out_pids, B, k, q.d_out_gids, q.d_edge_gids);
    if (s->prof.counters) {
        hipLaunchKernelGGL(batch_stats_kernel, dim3(32, B), dim3(256), 0, st, w.cand.as<uint32_t>(),
                           w.ncand.as<int>(), list, nlist, s->doc_off.as<uint32_t>(), w.cand_cap,
                           w.stats.as<unsigned long long>(),
                           subset ? w.rowmask.as<unsigned long long>() : (const unsigned long long*)nullptr, T);
    }
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

// the filters of a request (a host array of B handles, or nullptr): every one must be this searcher's; *filt_count = the largest
// population a CLB_FILTER_ALL search has to hold as a candidate set (a host value: sizing the workspace needs no read-back)
int check_filters(const clb_searcher* s, const clb_filter* const* filters, int64_t B, int scope, size_t* filt_count) {
    *filt_count = 0;
    if (scope != CLB_FILTER_CANDIDATES && scope != CLB_FILTER_ALL)
        return fail(CLB_EARGUMENT, "scope must be CLB_FILTER_CANDIDATES (0) or CLB_FILTER_ALL (1), got %d", scope);
    if (!filters) return CLB_OK;
    for (int64_t b = 0; b < B; ++b) {
        const clb_filter* f = filters[b];
        if (!f) continue;
        if (f->owner != s->serial)
            return fail(CLB_EARGUMENT, "the filter of query %lld was made for another searcher", (long long)b);
        if (f->n_docs != s->n_docs)       // its bitmap has the old length
            return fail(CLB_EARGUMENT, "the filter of query %lld: filter made before an append; make another", (long long)b);
        if (scope == CLB_FILTER_ALL) *filt_count = std::max(*filt_count, (size_t)f->count);
    }
    return CLB_OK;
}

// the prior of a request (or nullptr) and its weight, which check_request has found finite: the prior must be this searcher's,
// made for the passages it holds now, and weight * value must be finite for every value
int check_prior(const clb_searcher* s, const clb_prior* p, float weight) {
    if (!p) return CLB_OK;
    if (p->owner != s->serial) return fail(CLB_EARGUMENT, "the prior was made for another searcher");
    if (p->n_docs != s->n_docs)     // its table has the old length
        return fail(CLB_EARGUMENT, "prior made before an append; make another");
    if (!(std::fabs((double)weight) * (double)p->max_abs < (double)FLT_MAX))
        return fail(CLB_EARGUMENT, "prior_weight %g times the prior's largest |value| %g is not below FLT_MAX", (double)weight,
                    (double)p->max_abs);
    return CLB_OK;
}

// the grouping of a request (or nullptr): it must be this searcher's, made for the passages it holds now
int check_grouping(const clb_searcher* s, const clb_grouping* g) {
    if (!g) return CLB_OK;
    if (g->owner != s->serial) return fail(CLB_EARGUMENT, "the grouping was made for another searcher");
    if (g->n_docs != s->n_docs)     // its table has the old length
        return fail(CLB_EARGUMENT, "grouping made before an append; make another");
    return CLB_OK;
}

int bad_per_group(int64_t per_group) {
    return fail(CLB_EARGUMENT, "per_group must be 1..%d, got %lld", CLB_MAX_PER_GROUP, (long long)per_group);
}
int hits_without_grouping() { return fail(CLB_EARGUMENT, "grouping is null: per_group needs a grouping"); }

// The four ways a request reaches run_search: they differ in where the cursor arrays live (host / device memory) and in the
// fields they offer (the phases of a shard group take no hits and no cursors, phase 2 no filters)
enum class Route { host, device, phase1, phase2 };

// hits per result of a request: one hit per result is the representative, exactly the grouped search
inline int64_t request_hits(const clb_search_request& r) { return r.per_group > 1 ? r.per_group : 0; }

// EVERY rule of a search request and of the sizes of its call, in the order the entry points have always answered: first
// what needs no searcher -- the struct itself, the per_group range, a finite weight, the cursor pair, the combinations that
// are not offered, NaN cursors where the host can see them, the fields of the candidate lists -- then the handle and the sizes
// (check_search_args), the route's buffers, the listed pids where the host can see them and phase 1's group_base, then what is
// bound to the searcher (filters, grouping, prior) and the batch limit of a filtered phase 1.  *filt_count as check_filters
// gives it, or with candidate lists the most candidates one of them can give.
// route_buffers(): the route's own refusals of its plain parameters (the exchange buffers of a phase), answered where they
// always were -- directly behind the sizes.
template <class RouteBuffers>
int check_request(const clb_searcher* s, const clb_search_request* r, int64_t T, int64_t B, int64_t nprobe, int64_t k, Route route,
                  size_t* filt_count, RouteBuffers route_buffers) {
    *filt_count = 0;
    if (!r) return fail(CLB_EARGUMENT, "the search request is null");
    if (r->struct_bytes != (int64_t)sizeof(clb_search_request))
        return fail(CLB_EARGUMENT, "struct_bytes of the search request is %lld, not sizeof(clb_search_request) = %zu",
                    (long long)r->struct_bytes, sizeof(clb_search_request));
    if (r->per_group < 0 || r->per_group > CLB_MAX_PER_GROUP) return bad_per_group(r->per_group);
    if (r->per_group && !r->grouping) return hits_without_grouping();
    if ((r->prior || r->list_prior) && !std::isfinite(r->prior_weight))
        return fail(CLB_EARGUMENT, "prior_weight must be finite, got %g", (double)r->prior_weight);
    if ((r->after_scores == nullptr) != (r->after_pids == nullptr))
        return fail(CLB_EARGUMENT, "after_scores and after_pids must both be given or both be null");
    const bool after = r->after_scores != nullptr, phases = route == Route::phase1 || route == Route::phase2;
    if (r->list_prior && r->prior)          // one additive term per call
        return fail(CLB_EUNSUPPORTED, "list priors together with a prior are not supported: a call has one additive term");
    if (r->list_prior && r->per_group > 1)  // as with a prior: the extended list is built from approximate MaxSim scores
        return fail(CLB_EUNSUPPORTED, "per_group together with list priors is not supported: the hits of a grouped search take "
                                      "no additive term");
    if (after && r->list_prior) return fail(CLB_EUNSUPPORTED, "cursors together with list priors are not supported");
    if (r->prior && r->per_group > 1)       // group_extend_kernel builds the extended list from approximate MaxSim scores
        return fail(CLB_EUNSUPPORTED, "per_group together with a prior is not supported: the hits of a grouped search take no prior");
    if (after && r->grouping)               // a cursor continues the ranking of PASSAGES by MaxSim
        return fail(CLB_EUNSUPPORTED, "cursors together with a grouping are not supported");
    if (after && r->prior) return fail(CLB_EUNSUPPORTED, "cursors together with a prior are not supported");
    if (phases && r->per_group > 1) return fail(CLB_EUNSUPPORTED, "the phase calls of a shard group take no per_group");
    if (phases && after) return fail(CLB_EUNSUPPORTED, "the phase calls of a shard group take no cursors");
    if (route == Route::phase2 && r->filters)
        return fail(CLB_EARGUMENT, "phase 2 takes no filters: it continues on the candidates phase 1 left on the slot");
    for (int64_t b = 0; route == Route::host && after && b < B; ++b)
        if (std::isnan(r->after_scores[b])) return fail(CLB_EARGUMENT, "the cursor score of query %lld is NaN", (long long)b);
    // candidate lists: the pair, the stride, and the two places they are not offered; on the host route every length
    if ((r->list_pids == nullptr) != (r->list_lens == nullptr))
        return fail(CLB_EARGUMENT, "list_pids and list_lens must both be given or both be null");
    const bool listed = r->list_pids != nullptr;
    if (!listed && r->list_scores) return fail(CLB_EARGUMENT, "list_scores without candidate lists (list_pids / list_lens)");
    if (!listed && r->list_prior) return fail(CLB_EARGUMENT, "list_prior without candidate lists (list_pids / list_lens)");
    if (listed && (r->list_stride < 1 || r->list_stride > (int64_t)0x7fffffff))
        return fail(CLB_EARGUMENT, "list_stride must be 1..2^31-1, got %lld", (long long)r->list_stride);
    for (int64_t b = 0; listed && r->filters && b < B; ++b)
        if (r->filters[b])                  // a list IS the candidate set
            return fail(CLB_EUNSUPPORTED, "candidate lists together with filters are not supported");
    if (phases && listed) return fail(CLB_EUNSUPPORTED, "the phase calls of a shard group take no candidate lists");
    for (int64_t b = 0; route == Route::host && listed && b < B; ++b)
        if (r->list_lens[b] < 0 || r->list_lens[b] > r->list_stride)
            return fail(CLB_EARGUMENT, "the candidate list of query %lld has length %lld, outside 0..list_stride=%lld", (long long)b,
                        (long long)r->list_lens[b], (long long)r->list_stride);
    // ... and every list prior the call can read: finite, and finite when multiplied by the weight (clb_prior's two rules)
    if (route == Route::host && listed && r->list_prior) {
        float vmax = 0.f;
        for (int64_t b = 0; b < B; ++b)
            for (int64_t i = 0; i < r->list_lens[b]; ++i) {
                const float v = r->list_prior[b * r->list_stride + i];
                if (!std::isfinite(v))
                    return fail(CLB_EARGUMENT, "the list prior of query %lld, position %lld is not a finite number", (long long)b,
                                (long long)i);
                vmax = std::max(vmax, std::fabs(v));
            }
        if (!(std::fabs((double)r->prior_weight) * (double)vmax < (double)FLT_MAX))
            return fail(CLB_EARGUMENT, "prior_weight %g times the largest listed |value| %g is not below FLT_MAX",
                        (double)r->prior_weight, (double)vmax);
    }
    CLB_TRY(check_search_args(s, T, B, nprobe, k));
    CLB_TRY(route_buffers());
    // ... and, where the host can see them, every listed pid against the handle's range (the device route skips such a pid)
    for (int64_t b = 0; route == Route::host && listed && b < B; ++b)
        for (int64_t i = 0; i < r->list_lens[b]; ++i) {
            const int64_t pid = r->list_pids[b * r->list_stride + i];
            if (pid <= s->pid_offset || pid - s->pid_offset > s->n_docs)
                return fail(CLB_EBOUNDS, "candidate list of query %lld, position %lld: pid %lld outside %lld..%lld", (long long)b,
                            (long long)i, (long long)pid, (long long)s->pid_offset + 1, (long long)(s->pid_offset + s->n_docs));
        }
    if (route == Route::phase1 && r->grouping && r->group_base < 0)
        return fail(CLB_EARGUMENT, "group_base must be >= 0, got %lld", (long long)r->group_base);
    CLB_TRY(check_filters(s, r->filters, B, r->scope, filt_count));
    CLB_TRY(check_grouping(s, r->grouping));
    CLB_TRY(check_prior(s, r->prior, r->prior_weight));
    // a listed query has at most min(list_stride, n_docs) candidates: a host value, like a filter's population
    if (listed) *filt_count = (size_t)std::min<int64_t>(r->list_stride, s->n_docs);
    if (route == Route::phase1) {
        bool filtered = false;
        for (int64_t b = 0; r->filters && b < B; ++b) filtered |= r->filters[b] != nullptr;
        // the whole batch stays on the slot for phase 2, and the filter handles of a launch travel in one argument block
        if (filtered && B > kFilterQueries)
            return fail(CLB_EUNSUPPORTED, "a filtered clb_search_shard_phase1 takes at most %d queries per call, got %lld: split the batch",
                        kFilterQueries, (long long)B);
    }
    return CLB_OK;
}

// The sub-batch of queries b0 .. b0 + B - 1 of a call that carries the request r (checked by check_request, which gave
// filt_count), with everything of r that every route hands to run_search alike: the sub-batch's slice of the handle array --
// nullptr when none of its queries is filtered --, the grouping with its base and hits, the prior with its weight, the stride
// of the candidate lists.  The cursors and the list arrays stay with the route: it knows where they live.
Batch make_batch(const float* dQ, int64_t B, int64_t T, int64_t nprobe, int64_t k, const clb_search_request& r, int64_t b0,
                 size_t filt_count) {
    Batch q = make_batch(dQ, B, T, nprobe, k);
    q.filt_all = r.scope == CLB_FILTER_ALL;
    for (int64_t b = b0; r.filters && b < b0 + q.B; ++b)
        if (r.filters[b]) q.filt = r.filters + b0;
    q.filt_now = (q.filt && q.filt_all) || r.list_pids ? filt_count : 0;
    q.list_stride = r.list_pids ? r.list_stride : 0;
    q.grp = r.grouping; q.group_base = r.group_base; q.per_group = (int)request_hits(r);
    q.prior = r.prior; q.prior_weight = r.prior_weight;
    return q;
}

// the workspace of a slot of the *_slot entry points, with the searcher's device made current
int slot_workspace(clb_searcher* s, int slot, Workspace** w) {
    if (slot < 0 || slot >= kWorkspaceSlots) return fail(CLB_EARGUMENT, "workspace slot must be 0..%d", kWorkspaceSlots - 1);
    CLB_TRY(use_device(s->device));
    *w = &s->ws[slot];
    return CLB_OK;
}

// A large batch runs as sub-batches of kSubBatch queries, back to back on one stream and on one slot's scratch:
// every query carries an 8-MB fp16 score table (K = 131 072), and from ~64 queries on the tables of a batch outgrow
// the 256-MB Infinity Cache before pass 1 reads them (measured: 29.4 k queries/s at 64, 27.8 k at 256 in one piece);
// the centroid kernel shares a staged tile between 16 queries whatever the batch, so nothing is lost above that.
// (The two-phase sharded calls keep the whole batch: phase 2 continues on the scratch of phase 1.)
// run_one(b0, q): points q at the queries, cursors and outputs of the sub-batch that starts at query b0 and runs it.  q
// arrives as make_batch fills it from the request (every sub-batch carries the grouping and the prior), with stats_keep set
template <class RunOne>
int for_sub_batches(clb_searcher* s, Workspace& w, int64_t T, int64_t B, int64_t nprobe, int64_t k, const clb_search_request& r,
                    size_t filt_count, RunOne run_one) {
    w.pending.valid = false;
    w.grouped_done.valid = false;
    for (int64_t b0 = 0; b0 < B; b0 += kSubBatch) {
        Batch q = make_batch(nullptr, std::min<int64_t>(kSubBatch, B - b0), T, nprobe, k, r, b0, filt_count);
        CLB_TRY(ensure_workspace(s, w, q.B, T, nprobe, k, filt_count, r.grouping != nullptr, q.per_group, r.prior != nullptr,
                                 r.after_scores != nullptr, r.list_prior != nullptr));
        q.stats_keep = b0 > 0;
        CLB_TRY(run_one(b0, q));
    }
    return CLB_OK;
}

// ---- shared by clb_searcher_create, clb_searcher_append and clb_searcher_remove: the steps that check, order and write a
// batch of rows, and the tables a handle derives from its resident index ---------------------------------------------

using FilterPtr = std::unique_ptr<clb_filter, decltype(&clb_filter_destroy)>;

int check_shard_limits(int64_t n_emb, int64_t n_docs) {
    if (n_emb >= (int64_t)0xffffffffll || n_docs >= (int64_t)0x7fffffffll)
        return fail(CLB_EUNSUPPORTED, "a shard holds at most 2^32-1 embeddings / 2^31-1 passages");
    return CLB_OK;
}

struct Offsets {
    std::vector<uint32_t> off;      // off[i] = lens[0] + ... + lens[i - 1], i = 0 .. n
    int64_t total = 0, longest = 0;
};
// -> the position of the first negative length, or -1
int64_t running_offsets(const int64_t* lens, int64_t n, Offsets* o) {
    o->off.resize((size_t)n + 1);
    for (int64_t i = 0; i < n; ++i) {
        if (lens[i] < 0) return i;
        o->off[i] = (uint32_t)o->total;
        o->total += lens[i];
        o->longest = std::max(o->longest, lens[i]);
    }
    o->off[n] = (uint32_t)o->total;
    return -1;
}
// the offsets of n passages among their own n_emb embeddings (the reference's DimensionMismatch in _cids_to_eids!,
// ranking.jl:9-12); noun: what the message calls a passage of this batch
int passage_offsets(const int64_t* doclens, int64_t n, int64_t n_emb, const char* noun, Offsets* o) {
    const int64_t bad = running_offsets(doclens, n, o);
    if (bad >= 0) return fail(CLB_EARGUMENT, "negative doclen at %s %lld", noun, (long long)(bad + 1));
    if (o->total != n_emb)
        return fail(CLB_EDIMENSION, "sum(doclens)=%lld must equal the number of embeddings %lld", (long long)o->total, (long long)n_emb);
    return CLB_OK;
}

// One word that kernels report through (an error mask, a count): zeroed on the stream, read into `value` once the stream is done
template <class T>
struct DevWord {
    DevBuf buf;
    T value{};
    T* ptr() const { return buf.as<T>(); }
    int init(hipStream_t st) {
        CLB_TRY(buf.alloc(sizeof(T)));
        CLB_HIP(hipMemsetAsync(buf.p, 0, sizeof(T), st));
        return CLB_OK;
    }
    int read(hipStream_t st) {
        CLB_HIP(hipMemcpyAsync(&value, buf.p, sizeof(T), hipMemcpyDeviceToHost, st));
        CLB_HIP(hipStreamSynchronize(st));
        CLB_HIP(hipGetLastError());
        return CLB_OK;
    }
};
// the bits of an ingest's error word (ivf_to_pid_kernel, codes_to_zero_based_kernel, ivf_lists_sorted_kernel)
enum { kErrIvfId = 1, kErrCode = 2, kErrUnsortedList = 4 };

// the caller's 1-based codes as 0-based words in `dst`, a buffer of the library's (the caller's array is never written);
// a code outside 1..K raises kErrCode in *err (decompress's DomainError, residual.jl:766-768)
int stage_codes(hipStream_t st, const uint32_t* codes, hipMemcpyKind kind, int64_t n, int64_t K, uint32_t* dst, int* err) {
    if (n == 0) return CLB_OK;
    CLB_HIP(hipMemcpyAsync(dst, codes, sizeof(uint32_t) * n, kind, st));
    hipLaunchKernelGGL(codes_to_zero_based_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, n, (uint32_t)K, err);
    return CLB_OK;
}
int bad_codes() { return fail(CLB_EDOMAIN, "All the codes must be in the valid range of centroid IDs!"); }

// codes and residual rows of n embeddings, padded by one step of zero rows (dummy steps read embeddings 0 .. kStepRows-1
// even of a tiny index); rows 0 .. n - 1 are the caller's to write
int alloc_padded_rows(hipStream_t st, int64_t n, size_t row_bytes, DevBuf* codes, DevBuf* res) {
    CLB_TRY(codes->alloc(sizeof(uint32_t) * (n + kStepRows)));
    CLB_TRY(res->alloc(row_bytes * (n + kStepRows)));
    CLB_HIP(hipMemsetAsync(codes->as<uint32_t>() + n, 0, sizeof(uint32_t) * kStepRows, st));
    CLB_HIP(hipMemsetAsync(res->as<uint8_t>() + row_bytes * n, 0, row_bytes * kStepRows, st));
    return CLB_OK;
}

// Order every passage's embeddings by centroid code (results cannot change: MaxSim maximises over a passage's embeddings;
// row masks, headers and the IVF are positional or per passage).  Equal and neighbouring codes then sit in adjacent lanes
// of a pass-1 step: their 64-byte score rows coalesce into fewer, larger requests.
// The n_emb > 0 source rows (0-based codes; residual rows of row_bytes, a multiple of 16, 16-byte aligned) belong to n_docs
// passages at offsets_dev (n_docs + 1 offsets among these rows); all n_emb rows of codes_dst / res_dst are written.
// Padding is the caller's.  Waits for the stream: the scratch is gone on return.
int order_rows_by_code(hipStream_t st, const uint32_t* codes_src, const uint32_t* offsets_dev, int64_t n_emb, int64_t n_docs,
                       const uint8_t* res_src, size_t row_bytes, uint32_t* codes_dst, uint8_t* res_dst) {
    DevBuf keys, keys2, vals, perm;
    CLB_TRY(keys.alloc(sizeof(uint64_t) * n_emb));
    CLB_TRY(keys2.alloc(sizeof(uint64_t) * n_emb));
    CLB_TRY(vals.alloc(sizeof(uint32_t) * n_emb));
    CLB_TRY(perm.alloc(sizeof(uint32_t) * n_emb));
    const dim3 blocks((unsigned)((n_emb + 255) / 256));
    hipLaunchKernelGGL(passage_code_keys_kernel, blocks, dim3(256), 0, st, codes_src, offsets_dev, n_emb, (int)n_docs,
                       keys.as<unsigned long long>(), vals.as<uint32_t>());
    CLB_TRY(sort_pairs_u64(keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(), perm.as<uint32_t>(), (size_t)n_emb, st));
    hipLaunchKernelGGL(permute_codes_kernel, blocks, dim3(256), 0, st, perm.as<uint32_t>(), codes_src, codes_dst, n_emb);
    const int pieces = (int)(row_bytes / 16);
    hipLaunchKernelGGL(permute_rows16_kernel, dim3((unsigned)((n_emb * pieces + 255) / 256)), dim3(256), 0, st, perm.as<uint32_t>(),
                       reinterpret_cast<const uint4*>(res_src), reinterpret_cast<uint4*>(res_dst), n_emb, pieces);
    CLB_HIP(hipGetLastError());
    CLB_HIP(hipStreamSynchronize(st));
    return CLB_OK;
}

// the bitmap of the passages that hold embeddings (clb_searcher::live) from n_docs + 1 passage offsets on the device
int build_live_bitmap(hipStream_t st, const uint32_t* doc_off, int64_t n_docs, DevBuf* live) {
    const int64_t W = (n_docs + 31) / 32;
    CLB_TRY(live->alloc(sizeof(uint32_t) * (size_t)W));
    if (W > 0) hipLaunchKernelGGL(passage_live_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, doc_off, (int)n_docs,
                                  live->as<uint32_t>());
    return CLB_OK;
}

// the list lengths, descending, from the host copy of ivf_off (K + 1 entries): the candidate-capacity bound
std::vector<uint32_t> sorted_list_lengths(const std::vector<uint32_t>& ivf_off) {
    std::vector<uint32_t> len(ivf_off.size() - 1);
    for (size_t c = 0; c + 1 < ivf_off.size(); ++c) len[c] = ivf_off[c + 1] - ivf_off[c];
    std::sort(len.begin(), len.end(), std::greater<uint32_t>());
    return len;
}

int64_t resident_bytes(const clb_searcher* s) {
    return (int64_t)(s->centroids.bytes + s->weights.bytes + s->codes0.bytes + s->residuals.bytes + s->doc_off.bytes +
                     s->ivf_off.bytes + s->ivf_pid.bytes + s->codeinv.bytes + s->live.bytes);
}

// Statistics and tables of the tuned path over a whole index (codes0 / residuals as the handle stores them, padded by
// kStepRows).  Derived beside the handle and installed in one step, so that a failure leaves the handle as it was.
struct IndexTables {
    double code_adjacency = 0.0;
    ApproxConsts consts{};
    float inv_lo = 0.f, inv_step = 0.f;
    DevBuf codeinv;
};

int derive_index_tables(const clb_searcher* s, const uint32_t* codes0, const uint8_t* residuals, int64_t n_emb, IndexTables* t) {
    {   // Pass 1's gather form, by the index's own code statistics: when neighbouring embeddings of a passage often share
        // a 128-byte line of the score table (id-adjacent codes: the L1 merges those requests of the per-lane VGPR
        // gather) the VGPR form is faster (1 M topical passages: 0.67 against 0.76 ms per batch); when they do not
        // (uniform codes, a k-means-built index) the LDS-DMA form is (uniform: 1.47 against 1.61 ms)
        DevWord<unsigned long long> adj;
        const int64_t n_sample = std::min<int64_t>(n_emb, (int64_t)1 << 24);
        CLB_TRY(adj.init(s->stream));
        if (n_sample > 1)
            hipLaunchKernelGGL(code_adjacency_kernel, dim3(1024), dim3(256), 0, s->stream, codes0, n_sample, adj.ptr());
        CLB_TRY(adj.read(s->stream));
        t->code_adjacency = n_sample > 1 ? (double)adj.value / (double)(n_sample - 1) : 0.0;
    }
    if (s->approx_ok) {
        CLB_TRY(t->codeinv.alloc(sizeof(uint32_t) * (n_emb + kStepRows)));
        CLB_HIP(hipMemsetAsync(t->codeinv.p, 0, t->codeinv.bytes, s->stream));
    }
    return build_approx_tables(s->stream, s->centroids.as<float>(), s->weights.as<float>(), codes0, residuals, n_emb, (int)s->K,
                               s->approx_ok ? t->codeinv.as<uint32_t>() : nullptr, s->cbits, 1 << s->nbits, &t->consts,
                               &t->inv_lo, &t->inv_step);
}

inline void swap_buf(DevBuf& a, DevBuf& b) { std::swap(a.p, b.p); std::swap(a.bytes, b.bytes); }

// the six constants of the error bound that shards share, in the order of the C ABI (clb_searcher_get_bound_consts);
// dc_max travels beside them (clb_searcher::dc_f16)
constexpr float ApproxConsts::* kBoundConsts[6] = {&ApproxConsts::cn_max, &ApproxConsts::rn_max, &ApproxConsts::inv_max,
                                                   &ApproxConsts::rb_max, &ApproxConsts::dw_rn,  &ApproxConsts::inv_qerr};
void bound_consts_to_abi(const ApproxConsts& a, float* c) { for (int i = 0; i < 6; ++i) c[i] = a.*kBoundConsts[i]; }
// element-wise maximum: a shard group's bound is never lowered
void raise_bound_consts(ApproxConsts& a, const float* c) {
    for (int i = 0; i < 6; ++i) a.*kBoundConsts[i] = std::max(a.*kBoundConsts[i], c[i]);
}

// keep_max: the handle's bound constants are a shard group's (bounds_synced) -- like `set`, an append or a removal never
// lowers one
void install_index_tables(clb_searcher* s, IndexTables& t, bool keep_max = false) {
    s->code_adjacency = t.code_adjacency;
    s->gather_lds = default_gather_lds(s);
    swap_buf(s->codeinv, t.codeinv);
    s->inv_lo = t.inv_lo; s->inv_step = t.inv_step;
    float old[6];
    bound_consts_to_abi(s->approx_consts, old);
    s->approx_consts = t.consts;
    // the fp16 side's error lives beside the consts: a table made by the three-product kernels (fewer than 16 queries) keeps
    // the tighter bound.  Infinite (a centroid component beyond the fp16 range): the single-product kernel is never chosen.
    s->dc_f16 = std::isfinite(s->approx_consts.dc_max) ? s->approx_consts.dc_max : 0.f;
    s->approx_consts.dc_max = 0.f;
    if (keep_max) raise_bound_consts(s->approx_consts, old);
    s->index_bytes = resident_bytes(s);
}

// ---- index changes: clb_searcher_append, clb_searcher_remove, clb_searcher_update (index_change_kernels.hpp) ----------------
// What a change builds BESIDE the handle's arrays: the per-embedding and per-passage arrays and the inverted lists of the
// changed index, its counts and -- filled by commit_index_change -- the host copy of the list offsets and the approximate-pass
// tables.  commit_index_change swaps all of it in after the last device work has been waited for: any return before that
// leaves the handle untouched.
struct IndexChange {
    DevBuf codes0, residuals, doc_off, live, ivf_off, ivf_pid;
    IndexTables tables;
    std::vector<uint32_t> h_ivf_off;        // K + 1 list offsets
    int64_t n_docs = 0, n_emb = 0, max_doclen = 0;
};

// the first device step of a change, after the arguments have been checked on the host
int begin_index_change(const clb_searcher* s) {
    CLB_TRY(use_device(s->device));
    CLB_HIP(hipDeviceSynchronize());      // searches of this handle and whatever wrote the caller's device arrays
    return CLB_OK;
}

int check_pid_range(const clb_searcher* s, const int64_t* pids, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (pids[i] <= s->pid_offset || pids[i] > s->pid_offset + s->n_docs)
            return fail(CLB_EBOUNDS, "pid %lld (entry %lld) outside %lld..%lld", (long long)pids[i], (long long)i,
                        (long long)(s->pid_offset + 1), (long long)(s->pid_offset + s->n_docs));
    return CLB_OK;
}

// The n_emb > 0 new rows of n passages, where the change reads them: codes_dst / res_dst, the tail of the grown arrays for an
// append and a staging pair for an update.  codes_in: their 0-based, checked codes on the device; off_dev: the passages' n + 1
// offsets among them.  The tuned path gives them create's per-passage code order over the new rows alone (old passages keep
// theirs); the general path keeps the caller's order.
int stage_new_rows(const clb_searcher* s, const uint32_t* codes_in, const uint32_t* off_dev, int64_t n_emb, int64_t n,
                   const uint8_t* residuals, bool on_device, uint32_t* codes_dst, uint8_t* res_dst) {
    const hipStream_t st = s->stream;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t rows = (size_t)(s->dim / 8 * s->nbits);
    if (s->generic) {
        CLB_HIP(hipMemcpyAsync(codes_dst, codes_in, sizeof(uint32_t) * n_emb, hipMemcpyDeviceToDevice, st));
        CLB_HIP(hipMemcpyAsync(res_dst, residuals, rows * n_emb, kind, st));
        return CLB_OK;
    }
    DevBuf res_in;
    if (!on_device || ((uintptr_t)residuals & 15)) {        // the row permutation reads 16-byte pieces
        CLB_TRY(res_in.alloc(rows * n_emb));
        CLB_HIP(hipMemcpyAsync(res_in.p, residuals, rows * n_emb, kind, st));
        residuals = res_in.as<uint8_t>();
    }
    return order_rows_by_code(st, codes_in, off_dev, n_emb, n, residuals, rows, codes_dst, res_dst);
}

// the n named passages as a bitmap in a filter's layout (a SET bit: named; naming one twice is the caller's to refuse); a pid
// outside the handle raises *err.  d_pids: the pids on the device -- read *err before it and the host array go away.
int mark_passages(const clb_searcher* s, const int64_t* pids, int64_t n, DevBuf* d_pids, DevBuf* bits, int* err) {
    CLB_TRY(upload(*d_pids, pids, sizeof(int64_t) * n, s->stream));
    CLB_TRY(bits->alloc(sizeof(uint32_t) * (size_t)((s->n_docs + 31) / 32)));
    CLB_HIP(hipMemsetAsync(bits->p, 0, bits->bytes, s->stream));
    hipLaunchKernelGGL(filter_mark_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, d_pids->as<int64_t>(), n,
                       s->pid_offset, (int)s->n_docs, bits->as<uint32_t>(), err);
    return CLB_OK;
}

// pos (n_emb + 1 entries): the entries of the handle's inverted lists in front of each one whose passage is not named
int scan_kept_entries(const clb_searcher* s, const uint32_t* named, DevBuf* pos) {
    DevBuf flag;
    CLB_TRY(flag.alloc(sizeof(uint32_t) * (s->n_emb + 1)));
    CLB_TRY(pos->alloc(sizeof(uint32_t) * (s->n_emb + 1)));
    hipLaunchKernelGGL(ivf_keep_flags_kernel, dim3((unsigned)((s->n_emb + 1 + 255) / 256)), dim3(256), 0, s->stream,
                       s->ivf_pid.as<uint32_t>(), named, s->n_emb, flag.as<uint32_t>());
    return exclusive_scan_u32(flag.as<uint32_t>(), pos->as<uint32_t>(), (size_t)s->n_emb, s->stream);     // waits: flag may go
}

// the kept entries in their old order and the offsets of their lists, from the same scan: no sort
int compact_lists(const clb_searcher* s, const DevBuf& pos, int64_t n_kept, DevBuf* off, DevBuf* pid) {
    CLB_TRY(off->alloc(sizeof(uint32_t) * (s->K + 1)));
    CLB_TRY(pid->alloc(sizeof(uint32_t) * n_kept));
    hipLaunchKernelGGL(ivf_compact_kernel, dim3((unsigned)((s->n_emb + 1 + 255) / 256)), dim3(256), 0, s->stream,
                       s->ivf_pid.as<uint32_t>(), pos.as<uint32_t>(), s->n_emb, pid->as<uint32_t>());
    hipLaunchKernelGGL((list_offsets_kernel<true, false>), dim3((unsigned)((s->K + 1 + 255) / 256)), dim3(256), 0, s->stream,
                       s->ivf_off.as<uint32_t>(), pos.as<uint32_t>(), (const uint32_t*)nullptr, (int)(s->K + 1), off->as<uint32_t>());
    return CLB_OK;
}

// The inverted-list entries of n_emb new embeddings: the scan of the histogram of their codes (off, K + 1 entries) and their
// local pids in list order (pid; code beside them).  codes_in / off_dev as in stage_new_rows; the passages are d_pids (the
// caller's pids on the device) or, without them, pid_base onwards.  One stable sort by code gives the (code, embedding) order
// of a fresh build when the pids ascend with the embeddings (an append); by_pid sorts by pid first, so that every list's new
// entries hold non-decreasing pids whatever the caller's order is (an update).  Waits for the stream.
struct NewEntries {
    DevBuf off, code, pid;
};
int sort_new_entries(const clb_searcher* s, const uint32_t* codes_in, const uint32_t* off_dev, int64_t n, const int64_t* d_pids,
                     int64_t pid_base, int64_t n_emb, bool by_pid, NewEntries* e) {
    const hipStream_t st = s->stream;
    DevBuf hist, pid_in, pid2, code2;
    CLB_TRY(hist.alloc(sizeof(uint32_t) * (s->K + 1)));
    CLB_TRY(pid_in.alloc(sizeof(uint32_t) * n_emb));
    CLB_TRY(e->off.alloc(sizeof(uint32_t) * (s->K + 1)));
    CLB_TRY(e->code.alloc(sizeof(uint32_t) * n_emb));
    CLB_TRY(e->pid.alloc(sizeof(uint32_t) * n_emb));
    CLB_HIP(hipMemsetAsync(hist.p, 0, hist.bytes, st));
    if (n_emb > 0)
        hipLaunchKernelGGL(hist_pid_kernel, dim3((unsigned)((n_emb + 255) / 256)), dim3(256), 0, st, codes_in, off_dev, d_pids,
                           s->pid_offset, (uint32_t)pid_base, n_emb, (int)n, hist.as<uint32_t>(), pid_in.as<uint32_t>());
    CLB_TRY(exclusive_scan_u32(hist.as<uint32_t>(), e->off.as<uint32_t>(), (size_t)s->K, st));
    int pid_bits = 1, code_bits = 1;
    while (((int64_t)1 << pid_bits) < s->n_docs) ++pid_bits;
    while (((int64_t)1 << code_bits) < s->K) ++code_bits;
    const uint32_t *codes = codes_in, *pids = pid_in.as<uint32_t>();
    if (by_pid) {
        CLB_TRY(pid2.alloc(sizeof(uint32_t) * n_emb));
        CLB_TRY(code2.alloc(sizeof(uint32_t) * n_emb));
        CLB_TRY(sort_pairs_u32(pids, pid2.as<uint32_t>(), codes, code2.as<uint32_t>(), (size_t)n_emb, pid_bits, st));
        codes = code2.as<uint32_t>(); pids = pid2.as<uint32_t>();
    }
    return sort_pairs_u32(codes, e->code.as<uint32_t>(), pids, e->pid.as<uint32_t>(), (size_t)n_emb, code_bits, st);
}

// c's lists: those of old_off / old_pid (K lists, c->n_emb - the new entries) with e's new entries behind them, list by list
int merge_lists(const clb_searcher* s, const uint32_t* old_off, const uint32_t* old_pid, const NewEntries& e, IndexChange* c) {
    CLB_TRY(c->ivf_off.alloc(sizeof(uint32_t) * (s->K + 1)));
    CLB_TRY(c->ivf_pid.alloc(sizeof(uint32_t) * c->n_emb));
    hipLaunchKernelGGL((list_offsets_kernel<false, true>), dim3((unsigned)((s->K + 1 + 255) / 256)), dim3(256), 0, s->stream, old_off,
                       (const uint32_t*)nullptr, e.off.as<uint32_t>(), (int)(s->K + 1), c->ivf_off.as<uint32_t>());
    const int64_t tiles = (c->n_emb + kTile - 1) / kTile;
    if (tiles > 0)
        hipLaunchKernelGGL(ivf_merge_kernel, dim3((unsigned)std::min<int64_t>(tiles, 8192)), dim3(256), 0, s->stream, old_off,
                           e.off.as<uint32_t>(), c->ivf_off.as<uint32_t>(), old_pid, e.pid.as<uint32_t>(), (int)s->K, c->n_emb,
                           c->ivf_pid.as<uint32_t>());
    return CLB_OK;
}

// f(Piece{}) with the widest piece that a residual row of row_bytes is a whole number of
template <class F>
void with_piece(size_t row_bytes, F&& f) {
    if (row_bytes % 16 == 0) f(uint4{});
    else if (row_bytes % 4 == 0) f(uint32_t{});
    else f(uint8_t{});
}

// The end of a change, once everything of `c` but the tables has been enqueued: checks the lists, derives what the handle
// keeps of the changed index, waits, and only then touches the handle.
int commit_index_change(clb_searcher* s, IndexChange& c) {
    const hipStream_t st = s->stream;
    CLB_HIP(hipGetLastError());
    c.h_ivf_off.resize((size_t)s->K + 1);
    CLB_HIP(hipMemcpyAsync(c.h_ivf_off.data(), c.ivf_off.p, sizeof(uint32_t) * (s->K + 1), hipMemcpyDeviceToHost, st));
    CLB_HIP(hipStreamSynchronize(st));
    if ((int64_t)c.h_ivf_off[s->K] != c.n_emb)
        return fail(CLB_EHIP, "the changed inverted lists hold %lld entries, expected %lld", (long long)c.h_ivf_off[s->K],
                    (long long)c.n_emb);
    // code | inv_norm words and bound constants: one streaming pass over the whole changed index -- inv_norm is quantised over
    // the index's own range, which a new row may widen and a dropped row may narrow
    if (!s->generic) CLB_TRY(derive_index_tables(s, c.codes0.as<uint32_t>(), c.residuals.as<uint8_t>(), c.n_emb, &c.tables));
    CLB_HIP(hipStreamSynchronize(st));
    CLB_HIP(hipGetLastError());

    // ---- nothing below can fail ----
    swap_buf(s->codes0, c.codes0); swap_buf(s->residuals, c.residuals); swap_buf(s->doc_off, c.doc_off);
    swap_buf(s->ivf_off, c.ivf_off); swap_buf(s->ivf_pid, c.ivf_pid); swap_buf(s->live, c.live);
    s->n_docs = c.n_docs; s->n_emb = c.n_emb; s->max_doclen = c.max_doclen;
    s->ivf_len_sorted = sorted_list_lengths(c.h_ivf_off);
    if (s->generic) s->index_bytes = resident_bytes(s);
    else install_index_tables(s, c.tables, s->bounds_synced);
    for (auto& w : s->ws) {       // sized for the old index: the next ensure_workspace sizes every buffer again
        w.Bcap = 0;
        w.filt_cap = 0;           // populations of filters that no longer fit the handle
        w.bitmap.release();       // its rows had the old word count
        w.pending.valid = false;
    }
    ++s->generation;
    return CLB_OK;
}

// clb_searcher_remove and clb_searcher_update / _device after their host checks: the n passages `pids` lose their rows and, with
// `add`, get the add->total new ones that it delimits in the caller's order (codes, residuals).  Without new rows -- a removal, or
// an update to all-empty content -- no row is staged and the lists are only compacted.  *n_changed: the named passages whose
// old or new length is not zero; none: the handle stays as it is, generation included.
int replace_passages(clb_searcher* s, int64_t n, const int64_t* pids, const Offsets* add, const uint32_t* codes,
                     const uint8_t* residuals, bool on_device, int64_t* n_changed) {
    const int64_t n_old = s->n_emb, n_docs = s->n_docs, K = s->K, n_add = add ? add->total : 0;
    const bool staged = n_add > 0;
    CLB_TRY(begin_index_change(s));
    const hipStream_t st = s->stream;
    const size_t rows = (size_t)(s->dim / 8 * s->nbits);
    IndexChange c;
    DevWord<ChangeCounts> counts;
    {   // the scratch of the call
        // the new codes, 0-based and checked, in a buffer of the call's own; the named passages as a bitmap and their place in
        // the caller's list; the lengths of the changed index
        DevBuf codes_in, d_pids, stage_off, named, slot, len;
        DevWord<int> err;
        CLB_TRY(err.init(st));
        CLB_TRY(counts.init(st));
        CLB_TRY(mark_passages(s, pids, n, &d_pids, &named, err.ptr()));
        if (staged) {
            CLB_TRY(codes_in.alloc(sizeof(uint32_t) * n_add));
            CLB_TRY(stage_codes(st, codes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, n_add, K,
                                codes_in.as<uint32_t>(), err.ptr()));
            CLB_TRY(upload(stage_off, add->off.data(), sizeof(uint32_t) * add->off.size(), st));
            CLB_TRY(slot.alloc(sizeof(uint32_t) * n_docs));
            hipLaunchKernelGGL(update_slots_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_pids.as<int64_t>(), n,
                               s->pid_offset, (int)n_docs, slot.as<uint32_t>());
        }
        CLB_TRY(len.alloc(sizeof(uint32_t) * (n_docs + 1)));
        CLB_TRY(c.doc_off.alloc(sizeof(uint32_t) * (n_docs + 1)));
        const auto lengths_kernel = staged ? change_lengths_kernel<true> : change_lengths_kernel<false>;
        hipLaunchKernelGGL(lengths_kernel, dim3((unsigned)((n_docs + 1 + 255) / 256)), dim3(256), 0, st, s->doc_off.as<uint32_t>(),
                           named.as<uint32_t>(), slot.as<uint32_t>(), stage_off.as<uint32_t>(), (int)n_docs, len.as<uint32_t>(),
                           counts.ptr());
        CLB_TRY(err.read(st));                // ... before the host arrays go away
        CLB_TRY(counts.read(st));
        if (err.value & kErrCode) return bad_codes();
        if (err.value) return fail(CLB_EBOUNDS, "a pid outside the searcher's passages");
        if (staged) CLB_TRY(check_shard_limits(n_old - (int64_t)counts.value.dropped + n_add, n_docs));
        if (counts.value.changed == 0) return CLB_OK;       // every named passage was empty and stays empty
        uint32_t n_rows = 0;
        CLB_TRY(exclusive_scan_u32(len.as<uint32_t>(), c.doc_off.as<uint32_t>(), (size_t)n_docs, st));
        CLB_HIP(hipMemcpyAsync(&n_rows, c.doc_off.as<uint32_t>() + n_docs, sizeof n_rows, hipMemcpyDeviceToHost, st));
        CLB_HIP(hipStreamSynchronize(st));
        c.n_docs = n_docs; c.n_emb = n_rows; c.max_doclen = counts.value.longest;
        CLB_TRY(build_live_bitmap(st, c.doc_off.as<uint32_t>(), n_docs, &c.live));

        // one splice of the kept rows and the staged new ones, and the zero padding of one step
        DevBuf codes_staged, res_staged;
        if (staged) {
            CLB_TRY(codes_staged.alloc(sizeof(uint32_t) * n_add));
            CLB_TRY(res_staged.alloc(rows * n_add));
            CLB_TRY(stage_new_rows(s, codes_in.as<uint32_t>(), stage_off.as<uint32_t>(), n_add, n, residuals, on_device,
                                   codes_staged.as<uint32_t>(), res_staged.as<uint8_t>()));
        }
        CLB_TRY(alloc_padded_rows(st, c.n_emb, rows, &c.codes0, &c.residuals));
        const int64_t row_tiles = (c.n_emb + kTile - 1) / kTile;
        if (row_tiles > 0)
            with_piece(rows, [&](auto piece) {
                using Piece = decltype(piece);
                const auto rows_kernel = staged ? splice_rows_kernel<Piece, true> : splice_rows_kernel<Piece, false>;
                hipLaunchKernelGGL(rows_kernel, dim3((unsigned)std::min<int64_t>(row_tiles, 8192)), dim3(256), 0, st, s->doc_off.as<uint32_t>(),
                                   c.doc_off.as<uint32_t>(), named.as<uint32_t>(), slot.as<uint32_t>(), stage_off.as<uint32_t>(),
                                   (int)n_docs, c.n_emb, s->codes0.as<uint32_t>(), s->residuals.as<Piece>(),
                                   codes_staged.as<uint32_t>(), res_staged.as<Piece>(), (int)(rows / sizeof(Piece)),
                                   c.codes0.as<uint32_t>(), c.residuals.as<Piece>());
            });

        // the inverted lists.  Kept entries: a flag per old entry and its scan.  Without new entries one scatter of the entries
        // that stay, in their old order.  With them, on lists that hold non-decreasing pids, one pass puts both where a fresh
        // build would; on lists in the caller's own order the kept entries stay in that order (the same compaction) and the
        // new ones go behind them list by list (an append's merge): the lists stay unsorted.
        DevBuf pos, kept_off, kept_pid;
        NewEntries e;
        CLB_TRY(scan_kept_entries(s, named.as<uint32_t>(), &pos));
        if (!staged) {
            CLB_TRY(compact_lists(s, pos, c.n_emb, &c.ivf_off, &c.ivf_pid));
        } else {
            CLB_TRY(sort_new_entries(s, codes_in.as<uint32_t>(), stage_off.as<uint32_t>(), n, d_pids.as<int64_t>(), 0, n_add, true, &e));
            if (s->ivf_sorted) {
                CLB_TRY(c.ivf_off.alloc(sizeof(uint32_t) * (K + 1)));
                CLB_TRY(c.ivf_pid.alloc(sizeof(uint32_t) * c.n_emb));
                hipLaunchKernelGGL((list_offsets_kernel<true, true>), dim3((unsigned)((K + 1 + 255) / 256)), dim3(256), 0, st,
                                   s->ivf_off.as<uint32_t>(), pos.as<uint32_t>(), e.off.as<uint32_t>(), (int)(K + 1),
                                   c.ivf_off.as<uint32_t>());
                const int64_t tiles = (n_old + kTile - 1) / kTile + (n_add + kTile - 1) / kTile;
                hipLaunchKernelGGL(ivf_splice_kernel, dim3((unsigned)std::min<int64_t>(tiles, 8192)), dim3(256), 0, st,
                                   s->ivf_off.as<uint32_t>(), s->ivf_pid.as<uint32_t>(), pos.as<uint32_t>(), n_old, e.off.as<uint32_t>(),
                                   e.code.as<uint32_t>(), e.pid.as<uint32_t>(), n_add, (int)K, c.ivf_pid.as<uint32_t>());
            } else {
                CLB_TRY(compact_lists(s, pos, c.n_emb - n_add, &kept_off, &kept_pid));
                CLB_TRY(merge_lists(s, kept_off.as<uint32_t>(), kept_pid.as<uint32_t>(), e, &c));
            }
        }
        CLB_HIP(hipStreamSynchronize(st));      // the scratch goes away here
    }
    CLB_TRY(commit_index_change(s, c));
    if (n_changed) *n_changed = counts.value.changed;
    return CLB_OK;
}

}  // namespace

extern "C" {

const char* clb_version(void) { return "colbert_hip 0.1 (gfx950)"; }
const char* clb_last_error(void) { return clb::last_error().c_str(); }
int clb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// `big_on_device`: centroids, codes, residuals and ivf are device pointers on `device` (an index that was built there:
// clb_codec_compress_device / clb_build_ivf_device); the per-passage and per-centroid lengths are host arrays either way.
// The handle is owned until the last step has succeeded: any failure frees everything and leaves *out null.
static int searcher_create_impl(int device, int64_t dim, int nbits, int64_t K, const float* centroids,
                                const float* bucket_weights, int64_t n_docs, const int64_t* doclens, int64_t n_emb,
                                const uint32_t* codes, const uint8_t* residuals, const int64_t* ivf,
                                const int64_t* ivf_lengths, int64_t pid_offset, bool big_on_device, clb_searcher** out) {
    const hipMemcpyKind big_kind = big_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (!out) return fail(CLB_EARGUMENT, "out is null");
    *out = nullptr;
    if (dim < 8 || dim % 8 != 0) return fail(CLB_EDOMAIN, "dim should be a multiple of 8!");          // residual.jl:763-768
    if (nbits != 1 && nbits != 2 && nbits != 4 && nbits != 8)
        return fail(CLB_EUNSUPPORTED, "the HIP codec supports nbits in {1,2,4,8} (got %d)", nbits);
    if (K < 1 || n_docs < 0 || n_emb < 0) return fail(CLB_EARGUMENT, "negative or empty sizes");
    CLB_TRY(check_shard_limits(n_emb, n_docs));
    Offsets docs, lists;
    CLB_TRY(passage_offsets(doclens, n_docs, n_emb, "passage", &docs));
    if (running_offsets(ivf_lengths, K, &lists) >= 0) return fail(CLB_EARGUMENT, "negative ivf length");
    if (lists.total != n_emb) return fail(CLB_EDIMENSION, "length(ivf) must be equal to sum(ivf_lengths)!");
    CLB_TRY(use_device(device));

    static std::atomic<uint64_t> next_serial{1};
    std::unique_ptr<clb_searcher, decltype(&clb_searcher_destroy)> owned(new clb_searcher(), clb_searcher_destroy);
    clb_searcher* s = owned.get();
    s->serial = next_serial.fetch_add(1);
    s->device = device; s->dim = dim; s->nbits = nbits; s->K = K; s->n_docs = n_docs; s->n_emb = n_emb;
    s->pid_offset = pid_offset;
    s->generic = !(dim == kDim && nbits <= 4);     // the tuned kernels are built for dim 128, nbits 1/2/4
    s->max_doclen = docs.longest;
    CLB_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    const hipStream_t st = s->stream;
    s->ivf_len_sorted = sorted_list_lengths(lists.off);

    const size_t rows = (size_t)(dim / 8 * nbits);
    CLB_TRY(s->centroids.alloc(sizeof(float) * dim * K));
    CLB_HIP(hipMemcpyAsync(s->centroids.p, centroids, sizeof(float) * dim * K, big_kind, st));
    CLB_TRY(upload(s->weights, bucket_weights, sizeof(float) * ((size_t)1 << nbits), st));
    CLB_TRY(alloc_padded_rows(st, n_emb, rows, &s->codes0, &s->residuals));
    CLB_HIP(hipMemcpyAsync(s->residuals.p, residuals, rows * n_emb, big_kind, st));
    CLB_TRY(upload(s->doc_off, docs.off.data(), sizeof(uint32_t) * docs.off.size(), st));
    CLB_TRY(build_live_bitmap(st, s->doc_off.as<uint32_t>(), n_docs, &s->live));
    CLB_TRY(upload(s->ivf_off, lists.off.data(), sizeof(uint32_t) * lists.off.size(), st));
    CLB_TRY(s->ivf_pid.alloc(sizeof(uint32_t) * n_emb));
    DevBuf ivf_raw;
    DevWord<int> err;       // the three device checks share one word and one read-back
    CLB_TRY(ivf_raw.alloc(sizeof(int64_t) * n_emb));
    CLB_TRY(err.init(st));
    CLB_TRY(stage_codes(st, codes, big_kind, n_emb, K, s->codes0.as<uint32_t>(), err.ptr()));
    if (n_emb > 0) {
        CLB_HIP(hipMemcpyAsync(ivf_raw.p, ivf, sizeof(int64_t) * n_emb, big_kind, st));
        hipLaunchKernelGGL(ivf_to_pid_kernel, dim3((unsigned)((n_emb + 255) / 256)), dim3(256), 0, st, ivf_raw.as<int64_t>(),
                           s->doc_off.as<uint32_t>(), s->ivf_pid.as<uint32_t>(), n_emb, (int)n_docs, err.ptr());
        hipLaunchKernelGGL(ivf_lists_sorted_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, st,
                           s->ivf_off.as<uint32_t>(), s->ivf_pid.as<uint32_t>(), (int)K, err.ptr());
    }
    CLB_TRY(err.read(st));
    if (err.value & kErrIvfId) return fail(CLB_EBOUNDS, "ivf holds embedding ids outside 1..n_emb");
    if (err.value & kErrCode) return bad_codes();
    s->ivf_sorted = !(err.value & kErrUnsortedList);

    if (s->generic) {       // the general-shape path keeps the caller's row order and needs no tables
        s->index_bytes = resident_bytes(s);
        *out = owned.release();
        return CLB_OK;
    }
    if (n_emb > 0) {
        DevBuf codes_new, res_new;
        CLB_TRY(alloc_padded_rows(st, n_emb, rows, &codes_new, &res_new));
        CLB_TRY(order_rows_by_code(st, s->codes0.as<uint32_t>(), s->doc_off.as<uint32_t>(), n_emb, n_docs,
                                   s->residuals.as<uint8_t>(), rows, codes_new.as<uint32_t>(), res_new.as<uint8_t>()));
        swap_buf(s->codes0, codes_new); swap_buf(s->residuals, res_new);
    }
    // bf16 hi/lo split of the centroids for the bf16x3 centroid scoring, and their fp16 image
    const int64_t nel = dim * K;
    CLB_TRY(s->cent_hi.alloc(sizeof(uint16_t) * nel));
    CLB_TRY(s->cent_lo.alloc(sizeof(uint16_t) * nel));
    CLB_TRY(s->cent_f16.alloc(sizeof(uint16_t) * nel));
    hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, st,
                       s->centroids.as<float>(), s->cent_hi.as<uint16_t>(), s->cent_lo.as<uint16_t>(), nel);
    hipLaunchKernelGGL(to_f16_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, st,
                       s->centroids.as<float>(), s->cent_f16.as<uint16_t>(), nel);
    s->cbits = 1;
    while (((int64_t)1 << s->cbits) < K) ++s->cbits;
    // the packed word leaves 32 - cbits bits for inv_norm: at least 12 (K <= 2^20), otherwise exact mode only
    s->approx_ok = approx_supported((int)dim, nbits) && s->cbits <= 20;
    IndexTables tables;
    CLB_TRY(derive_index_tables(s, s->codes0.as<uint32_t>(), s->residuals.as<uint8_t>(), n_emb, &tables));
    install_index_tables(s, tables);
    s->mode = s->approx_ok ? 1 : 0;
    *out = owned.release();
    return CLB_OK;
}

int clb_searcher_create(int device, int64_t dim, int nbits, int64_t K, const float* centroids,
                        const float* bucket_weights, int64_t n_docs, const int64_t* doclens, int64_t n_emb,
                        const uint32_t* codes, const uint8_t* residuals, const int64_t* ivf,
                        const int64_t* ivf_lengths, int64_t pid_offset, clb_searcher** out) {
    return searcher_create_impl(device, dim, nbits, K, centroids, bucket_weights, n_docs, doclens, n_emb, codes, residuals,
                                ivf, ivf_lengths, pid_offset, false, out);
}

int clb_searcher_create_device(int device, int64_t dim, int nbits, int64_t K, const float* d_centroids,
                               const float* bucket_weights, int64_t n_docs, const int64_t* doclens, int64_t n_emb,
                               const uint32_t* d_codes, const uint8_t* d_residuals, const int64_t* d_ivf,
                               const int64_t* ivf_lengths, int64_t pid_offset, clb_searcher** out) {
    return searcher_create_impl(device, dim, nbits, K, d_centroids, bucket_weights, n_docs, doclens, n_emb, d_codes,
                                d_residuals, d_ivf, ivf_lengths, pid_offset, true, out);
}

int clb_searcher_destroy(clb_searcher* s) {
    if (!s) return CLB_OK;
    (void)hipSetDevice(s->device);
    if (s->stream) {
        (void)hipStreamSynchronize(s->stream);
        for (auto& v : s->prof.pending)
            for (auto& pr : v) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        for (auto e : s->prof.pool) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(s->stream);
    }
    delete s;
    return CLB_OK;
}

// clb_searcher_append / _device (include/colbert_hip.h).  The old rows move with plain device copies and the new ones go
// behind them; the inverted lists are the old lists with the new entries behind them, list by list.
static int searcher_append_impl(clb_searcher* s, int64_t n_new, const int64_t* doclens, int64_t n_new_emb,
                                const uint32_t* codes, const uint8_t* residuals, bool on_device) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (n_new < 0 || n_new_emb < 0) return fail(CLB_EARGUMENT, "negative sizes");
    if ((n_new > 0 && !doclens) || (n_new_emb > 0 && (!codes || !residuals))) return fail(CLB_EARGUMENT, "null argument");
    Offsets add;            // the appended passages among the appended embeddings
    CLB_TRY(passage_offsets(doclens, n_new, n_new_emb, "appended passage", &add));
    if (n_new == 0) return CLB_OK;
    const int64_t n_old = s->n_emb, d_old = s->n_docs;
    IndexChange c;
    c.n_docs = d_old + n_new; c.n_emb = n_old + n_new_emb; c.max_doclen = std::max<int64_t>(s->max_doclen, add.longest);
    CLB_TRY(check_shard_limits(c.n_emb, c.n_docs));
    CLB_TRY(begin_index_change(s));
    const hipStream_t st = s->stream;
    const size_t rows = (size_t)(s->dim / 8 * s->nbits);
    {   // the scratch of the call
        // the new codes, 0-based and checked, in a buffer of the call's own
        DevBuf codes_in, new_off_d;
        DevWord<int> err;
        CLB_TRY(codes_in.alloc(sizeof(uint32_t) * n_new_emb));
        CLB_TRY(err.init(st));
        CLB_TRY(stage_codes(st, codes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, n_new_emb, s->K,
                            codes_in.as<uint32_t>(), err.ptr()));
        CLB_TRY(err.read(st));
        if (err.value & kErrCode) return bad_codes();

        // grown per-embedding and per-passage arrays: the old rows, the new rows behind them, the zero padding of one step
        CLB_TRY(alloc_padded_rows(st, c.n_emb, rows, &c.codes0, &c.residuals));
        CLB_TRY(c.doc_off.alloc(sizeof(uint32_t) * (c.n_docs + 1)));
        CLB_TRY(upload(new_off_d, add.off.data(), sizeof(uint32_t) * add.off.size(), st));
        CLB_HIP(hipMemcpyAsync(c.codes0.p, s->codes0.p, sizeof(uint32_t) * n_old, hipMemcpyDeviceToDevice, st));
        CLB_HIP(hipMemcpyAsync(c.residuals.p, s->residuals.p, rows * n_old, hipMemcpyDeviceToDevice, st));
        CLB_HIP(hipMemcpyAsync(c.doc_off.p, s->doc_off.p, sizeof(uint32_t) * (d_old + 1), hipMemcpyDeviceToDevice, st));
        std::vector<uint32_t> off_tail((size_t)n_new);
        for (int64_t p = 0; p < n_new; ++p) off_tail[p] = (uint32_t)(n_old + add.off[p + 1]);
        CLB_HIP(hipMemcpyAsync(c.doc_off.as<uint32_t>() + d_old + 1, off_tail.data(), sizeof(uint32_t) * n_new, hipMemcpyHostToDevice, st));
        CLB_TRY(build_live_bitmap(st, c.doc_off.as<uint32_t>(), c.n_docs, &c.live));
        if (n_new_emb > 0)
            CLB_TRY(stage_new_rows(s, codes_in.as<uint32_t>(), new_off_d.as<uint32_t>(), n_new_emb, n_new, residuals, on_device,
                                   c.codes0.as<uint32_t>() + n_old, c.residuals.as<uint8_t>() + rows * n_old));

        // the inverted lists: the new entries in the (code, embedding) order of a fresh build, one merge
        NewEntries e;
        CLB_TRY(sort_new_entries(s, codes_in.as<uint32_t>(), new_off_d.as<uint32_t>(), n_new, nullptr, d_old, n_new_emb, false, &e));
        CLB_TRY(merge_lists(s, s->ivf_off.as<uint32_t>(), s->ivf_pid.as<uint32_t>(), e, &c));
        CLB_HIP(hipStreamSynchronize(st));      // the scratch goes away here
    }
    return commit_index_change(s, c);
}

int clb_searcher_append(clb_searcher* s, int64_t n_new, const int64_t* doclens, int64_t n_new_emb, const uint32_t* codes,
                        const uint8_t* residuals) {
    return searcher_append_impl(s, n_new, doclens, n_new_emb, codes, residuals, false);
}
int clb_searcher_append_device(clb_searcher* s, int64_t n_new, const int64_t* doclens, int64_t n_new_emb,
                               const uint32_t* d_codes, const uint8_t* d_residuals, void* hip_stream) {
    (void)hip_stream;     // the call waits for the whole device on entry, the work of that stream included
    return searcher_append_impl(s, n_new, doclens, n_new_emb, d_codes, d_residuals, true);
}

// clb_searcher_remove (include/colbert_hip.h): replace_passages without new content.  A pid may be named twice.
int clb_searcher_remove(clb_searcher* s, const int64_t* pids, int64_t n, int64_t* n_removed) {
    if (n_removed) *n_removed = 0;
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (n < 0 || (n > 0 && !pids)) return fail(CLB_EARGUMENT, "pids is null or n < 0");
    CLB_TRY(check_pid_range(s, pids, n));
    if (n == 0 || s->n_emb == 0) return CLB_OK;       // no pid named, or every named passage is empty already
    return replace_passages(s, n, pids, nullptr, nullptr, nullptr, false, n_removed);
}

// clb_searcher_update / _device (include/colbert_hip.h): replace_passages with one new content per named passage
static int searcher_update_impl(clb_searcher* s, int64_t n, const int64_t* pids, const int64_t* doclens, int64_t n_new_emb,
                                const uint32_t* codes, const uint8_t* residuals, bool on_device, int64_t* n_changed) {
    if (n_changed) *n_changed = 0;
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (n < 0 || n_new_emb < 0) return fail(CLB_EARGUMENT, "negative sizes");
    if ((n > 0 && (!pids || !doclens)) || (n_new_emb > 0 && (!codes || !residuals))) return fail(CLB_EARGUMENT, "null argument");
    Offsets add;            // the named passages among the new embeddings
    CLB_TRY(passage_offsets(doclens, n, n_new_emb, "replaced passage", &add));
    CLB_TRY(check_pid_range(s, pids, n));
    {   // a pid named twice: which of its two contents is meant?
        std::vector<int64_t> sorted(pids, pids + n);
        std::sort(sorted.begin(), sorted.end());
        const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
        if (twice != sorted.end())
            return fail(CLB_EARGUMENT, "pid %lld is named twice: an update takes one new content per passage", (long long)*twice);
    }
    if (n == 0) return CLB_OK;
    return replace_passages(s, n, pids, &add, codes, residuals, on_device, n_changed);
}
int clb_searcher_update(clb_searcher* s, int64_t n, const int64_t* pids, const int64_t* doclens, int64_t n_new_emb,
                        const uint32_t* codes, const uint8_t* residuals, int64_t* n_changed) {
    return searcher_update_impl(s, n, pids, doclens, n_new_emb, codes, residuals, false, n_changed);
}
int clb_searcher_update_device(clb_searcher* s, int64_t n, const int64_t* pids, const int64_t* doclens, int64_t n_new_emb,
                               const uint32_t* d_codes, const uint8_t* d_residuals, void* hip_stream, int64_t* n_changed) {
    (void)hip_stream;     // the call waits for the whole device on entry, the work of that stream included
    return searcher_update_impl(s, n, pids, doclens, n_new_emb, d_codes, d_residuals, true, n_changed);
}
// a count cannot carry an error code: a null handle gives -CLB_EARGUMENT and the message
int64_t clb_searcher_generation(const clb_searcher* s) { return s ? s->generation : -(int64_t)fail(CLB_EARGUMENT, "null searcher"); }
int64_t clb_searcher_num_docs(const clb_searcher* s) { return s ? s->n_docs : -(int64_t)fail(CLB_EARGUMENT, "null searcher"); }
int64_t clb_searcher_num_embeddings(const clb_searcher* s) { return s ? s->n_emb : -(int64_t)fail(CLB_EARGUMENT, "null searcher"); }

int64_t clb_searcher_device_bytes(const clb_searcher* s) {
    if (!s) return 0;
    int64_t tot = s->index_bytes;
    for (const auto& w : s->ws) {
        // not every buffer of Workspace is summed: bounds, wsel and the g_* buffers are left out (the reported figure is unchanged)
        const DevBuf* bufs[] = {&w.Qdev, &w.cells, &w.cells_q, &w.partial, &w.sel, &w.bitmap, &w.blocksum, &w.ncand, &w.cand,
                                &w.cand_hdr, &w.scores, &w.list, &w.nlist, &w.thresh, &w.outp, &w.outs, &w.flags, &w.stats, &w.redo, &w.rowmask, &w.eps_pair, &w.tokmax, &w.tau_glob, &w.tscale, &w.rangep, &w.cells8};
        for (auto* b : bufs) tot += (int64_t)b->bytes;
    }
    return tot;
}

int clb_searcher_set_mode(clb_searcher* s, int mode) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (mode != 0 && mode != 1) return fail(CLB_EARGUMENT, "mode must be 0 (exact) or 1 (two-pass)");
    if (mode == 1 && !s->approx_ok) return fail(CLB_EUNSUPPORTED, "two-pass mode needs dim=128, nbits=2");
    s->mode = mode;
    return CLB_OK;
}
int clb_searcher_get_mode(const clb_searcher* s) { return s ? s->mode : -1; }

int clb_searcher_set_wide_select(clb_searcher* s, int on) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (on < -1 || on > 1) return fail(CLB_EARGUMENT, "wide select must be -1 (by candidate capacity), 0 (never) or 1 (always)");
    s->wide_select = on;
    return CLB_OK;
}

int clb_searcher_sync_bound_consts(clb_searcher* s, clb_comm* c) {
    if (!s || !c) return fail(CLB_EARGUMENT, "null argument");
    CLB_TRY(use_device(s->device));
    float consts[6];
    CLB_TRY(clb_searcher_get_bound_consts(s, consts));
    DevBuf d;
    CLB_TRY(upload(d, consts, sizeof consts, s->stream));
    CLB_TRY(clb_comm_all_reduce_max_f32(c, d.as<float>(), 6, s->stream));
    CLB_HIP(hipMemcpyAsync(consts, d.p, sizeof consts, hipMemcpyDeviceToHost, s->stream));
    CLB_HIP(hipStreamSynchronize(s->stream));
    return clb_searcher_set_bound_consts(s, consts);
}

int clb_searcher_set_pass1_gather(clb_searcher* s, int form) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (form < -1 || form > 1) return fail(CLB_EARGUMENT, "pass-1 gather form must be -1 (by the code statistics), 0 (VGPR) or 1 (LDS-DMA)");
    s->gather_lds = form < 0 ? default_gather_lds(s) : form;
    return CLB_OK;
}
int clb_searcher_get_pass1_gather(const clb_searcher* s, double* adjacency) {
    if (!s) return -1;
    if (adjacency) *adjacency = s->code_adjacency;
    return s->gather_lds;
}

int clb_searcher_set_score_rows(clb_searcher* s, int form) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (form < -1 || form > 1) return fail(CLB_EARGUMENT, "score rows must be -1 (default: fp16), 0 (64-byte fp16 rows) or 1 (32-byte rows of 8-bit cells)");
    if (form == 1 && !s->approx_ok) return fail(CLB_EUNSUPPORTED, "8-bit score rows need the two-pass mode (dim=128, nbits=2)");
    s->cell8 = form;
    return CLB_OK;
}
int clb_searcher_get_score_rows(const clb_searcher* s) { return s ? (cell8_rows(s) ? 1 : 0) : -1; }

int clb_searcher_set_centroid_products(clb_searcher* s, int n) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (n != -1 && n != 1 && n != 3) return fail(CLB_EARGUMENT, "centroid products must be -1 (default), 1 (one fp16 product) or 3 (bf16 split)");
    s->s1_x1 = n == 1 ? 1 : n == 3 ? 0 : -1;
    return CLB_OK;
}
int clb_searcher_get_centroid_products(const clb_searcher* s, float* max_f16_error) {
    if (!s) return -1;
    if (max_f16_error) *max_f16_error = s->dc_f16;
    return single_product_table(s) ? 1 : 3;
}

int clb_searcher_get_bound_consts(const clb_searcher* s, float* consts) {
    if (!s || !consts) return fail(CLB_EARGUMENT, "null argument");
    bound_consts_to_abi(s->approx_consts, consts);
    return CLB_OK;
}
int clb_searcher_set_bound_consts(clb_searcher* s, const float* consts) {
    if (!s || !consts) return fail(CLB_EARGUMENT, "null argument");
    for (int i = 0; i < 6; ++i)
        if (!(consts[i] >= 0.f)) return fail(CLB_EARGUMENT, "bound constants must be non-negative numbers");
    raise_bound_consts(s->approx_consts, consts);
    s->bounds_synced = true;
    return CLB_OK;
}

// ---- the four routes of a search request ------------------------------------------------------------------------------
int clb_search_batch_request_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const clb_search_request* req, int64_t* d_out_pids, float* d_out_scores,
                                         int64_t* d_n_cand, void* hip_stream) {
    size_t filt_count = 0;
    CLB_TRY(check_request(s, req, T, B, nprobe, k, Route::device, &filt_count, [] { return CLB_OK; }));
    const clb_search_request& r = *req;
    const int64_t hits = request_hits(r);
    Workspace* w = nullptr;
    CLB_TRY(slot_workspace(s, slot, &w));
    hipStream_t st = (hipStream_t)hip_stream;   // NULL = the HIP null stream, as for any HIP API
    CLB_TRY(for_sub_batches(s, *w, T, B, nprobe, k, r, filt_count, [&](int64_t b0, Batch& q) -> int {
        q.dQ = d_Q + (size_t)b0 * T * s->dim;
        if (r.after_scores) { q.d_after_s = r.after_scores + b0; q.d_after_p = r.after_pids + b0; }
        if (r.list_pids) {         // the sub-batch's own rows of the caller's device arrays
            q.d_list_pids = r.list_pids + (size_t)b0 * r.list_stride; q.d_list_lens = r.list_lens + b0;
            q.d_list_scores = r.list_scores ? r.list_scores + (size_t)b0 * r.list_stride : nullptr;
            q.d_list_prior = r.list_prior ? r.list_prior + (size_t)b0 * r.list_stride : nullptr;
        }
        q.d_out_pids = hits ? w->hit_p.as<int64_t>() : d_out_pids + (size_t)b0 * k;
        q.d_out_scores = hits ? w->hit_s.as<float>() : d_out_scores + (size_t)b0 * k;
        q.d_hit_pids = d_out_pids + (size_t)b0 * k * hits;
        q.d_hit_scores = d_out_scores + (size_t)b0 * k * hits;
        q.d_n_cand = d_n_cand ? d_n_cand + b0 : nullptr;
        return run_search(s, *w, st, q);
    }));
    if (r.grouping && !hits && B <= kSubBatch) {
        auto& d = w->grouped_done;
        d.valid = true; d.B = B; d.k = k; d.generation = s->generation; d.grp = r.grouping; d.stream = hip_stream;
    }
    return CLB_OK;
}

int clb_search_batch_request(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                             const clb_search_request* req, int64_t* out_pids, float* out_scores, int64_t* n_cand) {
    size_t filt_count = 0;
    CLB_TRY(check_request(s, req, T, B, nprobe, k, Route::host, &filt_count, [] { return CLB_OK; }));
    const clb_search_request& r = *req;
    const int64_t hits = request_hits(r);
    const int64_t km = k * std::max<int64_t>(hits, 1);     // entries of one query's result
    Workspace* wp = nullptr;
    CLB_TRY(slot_workspace(s, 0, &wp));
    Workspace& w = *wp;
    hipStream_t st = s->stream;
    std::vector<int> nc((size_t)B), fl((size_t)B);
    const size_t L = r.list_pids ? (size_t)r.list_stride : 0;
    if (L) {        // room for one sub-batch's rows of the candidate lists
        const size_t rows = (size_t)std::min<int64_t>(kSubBatch, B);
        CLB_TRY(w.lst_pids.ensure(sizeof(int64_t) * rows * L));
        CLB_TRY(w.lst_lens.ensure(sizeof(int64_t) * rows));
        if (r.list_scores) CLB_TRY(w.lst_scores.ensure(sizeof(float) * rows * L));
        if (r.list_prior) CLB_TRY(w.lst_prior.ensure(sizeof(float) * rows * L));
    }
    // the queries go up into the slot's own buffer and the results come back from it, sub-batch by sub-batch
    CLB_TRY(for_sub_batches(s, w, T, B, nprobe, k, r, filt_count, [&](int64_t b0, Batch& q) -> int {
        CLB_HIP(hipMemcpyAsync(w.Qdev.p, Q + (size_t)b0 * T * s->dim, sizeof(float) * q.B * T * s->dim, hipMemcpyHostToDevice, st));
        if (L) {                   // the sub-batch's lists go up beside its queries
            CLB_HIP(hipMemcpyAsync(w.lst_pids.p, r.list_pids + (size_t)b0 * L, sizeof(int64_t) * q.B * L, hipMemcpyHostToDevice, st));
            CLB_HIP(hipMemcpyAsync(w.lst_lens.p, r.list_lens + b0, sizeof(int64_t) * q.B, hipMemcpyHostToDevice, st));
            q.d_list_pids = w.lst_pids.as<int64_t>(); q.d_list_lens = w.lst_lens.as<int64_t>();
            q.d_list_scores = r.list_scores ? w.lst_scores.as<float>() : nullptr;
            if (r.list_prior) {
                CLB_HIP(hipMemcpyAsync(w.lst_prior.p, r.list_prior + (size_t)b0 * L, sizeof(float) * q.B * L, hipMemcpyHostToDevice, st));
                q.d_list_prior = w.lst_prior.as<float>();
            }
        }
        if (r.after_scores) {      // the sub-batch's cursors go up beside its queries
            CLB_HIP(hipMemcpyAsync(w.after_cur_s.p, r.after_scores + b0, sizeof(float) * q.B, hipMemcpyHostToDevice, st));
            CLB_HIP(hipMemcpyAsync(w.after_cur_p.p, r.after_pids + b0, sizeof(int64_t) * q.B, hipMemcpyHostToDevice, st));
            q.d_after_s = w.after_cur_s.as<float>(); q.d_after_p = w.after_cur_p.as<int64_t>();
        }
        q.dQ = w.Qdev.as<float>();
        q.d_out_pids = hits ? w.hit_p.as<int64_t>() : w.outp.as<int64_t>();
        q.d_out_scores = hits ? w.hit_s.as<float>() : w.outs.as<float>();
        q.d_hit_pids = w.outp.as<int64_t>();
        q.d_hit_scores = w.outs.as<float>();
        CLB_TRY(run_search(s, w, st, q));
        CLB_HIP(hipMemcpyAsync(out_pids + (size_t)b0 * km, w.outp.p, sizeof(int64_t) * q.B * km, hipMemcpyDeviceToHost, st));
        CLB_HIP(hipMemcpyAsync(out_scores + (size_t)b0 * km, w.outs.p, sizeof(float) * q.B * km, hipMemcpyDeviceToHost, st));
        CLB_HIP(hipMemcpyAsync(nc.data() + b0, reported_count(w, q), sizeof(int) * q.B, hipMemcpyDeviceToHost, st));
        CLB_HIP(hipMemcpyAsync(fl.data() + b0, w.flags.p, sizeof(int) * q.B, hipMemcpyDeviceToHost, st));
        if (q.d_list_scores)
            CLB_HIP(hipMemcpyAsync(r.list_scores + (size_t)b0 * L, w.lst_scores.p, sizeof(float) * q.B * L, hipMemcpyDeviceToHost, st));
        return CLB_OK;
    }));
    CLB_HIP(hipStreamSynchronize(st));
    int64_t docs = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (n_cand) n_cand[b] = nc[b];
        docs += nc[b];
    }
    s->last_cand_docs = docs;
    if (!r.pad_short)
        for (int64_t b = 0; b < B; ++b)
            if (fl[b])  // searching.jl:127 `pids[1:k]` on a shorter vector
                return fail(CLB_EBOUNDS, "query %lld has %d candidate %s, fewer than k=%lld", (long long)b, nc[b],
                            r.grouping ? "groups" : "passages", (long long)k);
    return CLB_OK;
}

int clb_search_shard_phase1_request_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const clb_search_request* req, float* d_local_top, int64_t* d_local_gid,
                                         float* d_local_mabs, void* hip_stream) {
    size_t filt_count = 0;
    CLB_TRY(check_request(s, req, T, B, nprobe, k, Route::phase1, &filt_count, [&] {
        if (!d_local_top) return fail(CLB_EARGUMENT, "d_local_top is null");
        if (req->prior && !d_local_mabs) return fail(CLB_EARGUMENT, "d_local_mabs is null");
        if (req->grouping && !d_local_gid) return fail(CLB_EARGUMENT, "d_local_gid is null");
        return (int)CLB_OK;
    }));
    const clb_search_request& r = *req;
    Workspace* wp = nullptr;
    CLB_TRY(slot_workspace(s, slot, &wp));
    Workspace& w = *wp;
    CLB_TRY(ensure_workspace(s, w, B, T, nprobe, k, filt_count, r.grouping != nullptr));
    if (r.grouping || r.prior) CLB_TRY(w.tau_glob.ensure(sizeof(float) * B));      // phase 2 then allocates nothing
    w.pending.valid = false;
    w.grouped_done.valid = false;
    Batch q = make_batch(d_Q, B, T, nprobe, k, r, 0, filt_count);
    q.phase = 1; q.d_local_top = d_local_top; q.d_local_gid = d_local_gid;
    q.d_local_mabs = r.prior ? d_local_mabs : nullptr;
    CLB_TRY(run_search(s, w, (hipStream_t)hip_stream, q));
    w.pending.valid = true; w.pending.dQ = d_Q; w.pending.T = T; w.pending.B = B; w.pending.nprobe = nprobe;
    w.pending.k = k; w.pending.stream = hip_stream; w.pending.filt_now = q.filt_now;
    w.pending.grp = r.grouping; w.pending.group_base = r.group_base;
    w.pending.prior = r.prior; w.pending.weight = r.prior ? r.prior_weight : 0.f;
    return CLB_OK;
}

int clb_search_shard_phase2_request_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const clb_search_request* req, const float* d_all_top,
                                         const int64_t* d_all_gid, const float* d_all_mabs, int64_t n_shards, int64_t* d_out_pids,
                                         float* d_out_scores, int64_t* d_out_gids, int64_t* d_n_cand, int64_t* d_edge_gids,
                                         void* hip_stream) {
    size_t filt_count = 0;
    CLB_TRY(check_request(s, req, T, B, nprobe, k, Route::phase2, &filt_count, [&] {
        if (!d_all_top || n_shards < 1) return fail(CLB_EARGUMENT, "d_all_top is null or n_shards < 1");
        if (req->prior) {
            if (!d_all_mabs) return fail(CLB_EARGUMENT, "d_all_mabs is null");
            if (!d_out_pids || !d_out_scores || !d_n_cand)
                return fail(CLB_EARGUMENT, "an output of the prior phase 2 is null (d_out_pids, d_out_scores, d_n_cand)");
        }
        if (req->grouping) {
            if (!d_all_gid) return fail(CLB_EARGUMENT, "d_all_gid is null");
            if (!d_out_pids || !d_out_scores || !d_out_gids || !d_n_cand || !d_edge_gids)
                return fail(CLB_EARGUMENT, "an output of the grouped phase 2 is null (d_out_pids, d_out_scores, d_out_gids, d_n_cand, d_edge_gids)");
        }
        return (int)CLB_OK;
    }));
    const clb_search_request& r = *req;
    if (r.grouping && n_shards > kMaxGroupShards)
        return fail(CLB_EUNSUPPORTED, "the grouped phase 2 takes at most %d shards, got %lld", kMaxGroupShards, (long long)n_shards);
    Workspace* wp = nullptr;
    CLB_TRY(slot_workspace(s, slot, &wp));
    Workspace& w = *wp;
    const auto& pd = w.pending;
    if (!pd.valid || pd.dQ != d_Q || pd.T != T || pd.B != B || pd.nprobe != nprobe || pd.k != k || pd.stream != hip_stream ||
        pd.grp != r.grouping || (r.grouping && pd.group_base != r.group_base) || pd.prior != r.prior ||
        (r.prior && std::memcmp(&pd.weight, &r.prior_weight, sizeof(float)) != 0))
        return fail(CLB_EARGUMENT, "clb_search_shard_phase2 without a matching clb_search_shard_phase1 "
                                   "on this workspace slot (same queries, T, B, nprobe, k and stream -- with a grouping or a prior: the same "
                                   "grouping, group_base, prior and weight -- and no other search on the slot in between)");
    // every shard must cut at tau_global - 2 eps with ONE eps (the largest): a shard still on its own bound constants
    // could drop a member of the global top-k silently, so phase 2 with other shards' scores is refused until the host
    // has shared them (clb_searcher_get_bound_consts on every shard -> element-wise maximum -> clb_searcher_set_bound_consts)
    if (n_shards > 1 && !s->bounds_synced)
        return fail(CLB_EARGUMENT, "clb_search_shard_phase2 with %lld shards before clb_searcher_set_bound_consts: the shards "
                                   "must share one error bound (all-reduce MAX of clb_searcher_get_bound_consts)", (long long)n_shards);
    w.pending.valid = false;
    // phase 1's filters are in the candidate list it left on the slot (cand / cand_hdr / ncand): everything from here on
    // reads only that list, and the two-pass proof holds for whatever candidate set it is given -- no filter operand
    Batch q = make_batch(d_Q, B, T, nprobe, k, r, 0, filt_count);
    q.filt_now = pd.filt_now;       // ... but the selection kernels are chosen by the same candidate capacity
    q.d_out_pids = d_out_pids; q.d_out_scores = d_out_scores; q.d_n_cand = d_n_cand;
    q.phase = 2; q.d_all_top = d_all_top; q.n_shards = (int)n_shards;
    // the group and magnitude records are read, and the group outputs written, only with what they belong to
    q.d_all_gid = r.grouping ? d_all_gid : nullptr; q.d_out_gids = r.grouping ? d_out_gids : nullptr;
    q.d_edge_gids = r.grouping ? d_edge_gids : nullptr; q.d_all_mabs = r.prior ? d_all_mabs : nullptr;
    return run_search(s, w, (hipStream_t)hip_stream, q);
}

// ---- the named entry points: each its own refusal (if it has one), a request, one call -----------------------------------
// (request fields in order: struct_bytes, filters, scope, pad_short, grouping, per_group, group_base, prior, prior_weight,
// list_prior, after_scores, after_pids, list_pids, list_lens, list_stride, list_scores; what a named entry leaves out is zero)
constexpr int64_t kReq = sizeof(clb_search_request);

int clb_search_batch_device(clb_searcher* s, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                            int64_t k, int64_t* d_out_pids, float* d_out_scores, int64_t* d_n_cand,
                            void* hip_stream) {
    return clb_search_batch_device_slot(s, 0, d_Q, T, B, nprobe, k, d_out_pids, d_out_scores, d_n_cand, hip_stream);
}

int clb_search_batch_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                 int64_t k, int64_t* d_out_pids, float* d_out_scores, int64_t* d_n_cand,
                                 void* hip_stream) {
    const clb_search_request r = {kReq};
    return clb_search_batch_request_device_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_out_pids, d_out_scores, d_n_cand, hip_stream);
}

int clb_search_batch_filtered_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                          int64_t k, const clb_filter* const* filters, int scope, int64_t* d_out_pids,
                                          float* d_out_scores, int64_t* d_n_cand, void* hip_stream) {
    const clb_search_request r = {kReq, filters, scope};
    return clb_search_batch_request_device_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_out_pids, d_out_scores, d_n_cand, hip_stream);
}

int clb_search_batch_grouped_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const clb_filter* const* filters, int scope, const clb_grouping* grouping,
                                         int64_t* d_out_pids, float* d_out_scores, int64_t* d_n_cand, void* hip_stream) {
    const clb_search_request r = {kReq, filters, scope, 0, grouping};
    return clb_search_batch_request_device_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_out_pids, d_out_scores, d_n_cand, hip_stream);
}

// the hits entries' own refusal: they need a grouping, and the request's per_group == 0 ("none") is no number of hits
static int check_hits_entry(const clb_grouping* grouping, int64_t per_group) {
    if (!grouping) return hits_without_grouping();
    return per_group == 0 ? bad_per_group(per_group) : CLB_OK;
}

int clb_search_batch_grouped_hits_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                              int64_t k, const clb_filter* const* filters, int scope,
                                              const clb_grouping* grouping, int64_t per_group, int64_t* d_out_pids,
                                              float* d_out_scores, int64_t* d_n_cand, void* hip_stream) {
    CLB_TRY(check_hits_entry(grouping, per_group));
    const clb_search_request r = {kReq, filters, scope, 0, grouping, per_group};
    return clb_search_batch_request_device_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_out_pids, d_out_scores, d_n_cand, hip_stream);
}

int clb_search_batch_prior_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                       int64_t k, const clb_filter* const* filters, int scope, const clb_grouping* grouping,
                                       const clb_prior* prior, float weight, int64_t* d_out_pids, float* d_out_scores,
                                       int64_t* d_n_cand, void* hip_stream) {
    const clb_search_request r = {kReq, filters, scope, 0, grouping, 0, 0, prior, weight};
    return clb_search_batch_request_device_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_out_pids, d_out_scores, d_n_cand, hip_stream);
}

// the cursor entries' own refusal, ahead of everything else: the handle and the outputs
static int check_after_entry(const clb_searcher* s, const void* out_pids, const void* out_scores) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (!out_pids || !out_scores) return fail(CLB_EARGUMENT, "out_pids / out_scores is null");
    return CLB_OK;
}

int clb_search_batch_after_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                       int64_t k, const clb_filter* const* filters, int scope, const float* d_after_scores,
                                       const int64_t* d_after_pids, int64_t* d_out_pids, float* d_out_scores,
                                       int64_t* d_n_cand, void* hip_stream) {
    CLB_TRY(check_after_entry(s, d_out_pids, d_out_scores));
    const clb_search_request r = {kReq, filters, scope, 0, nullptr, 0, 0, nullptr, 0.f, nullptr, d_after_scores, d_after_pids};
    return clb_search_batch_request_device_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_out_pids, d_out_scores, d_n_cand, hip_stream);
}

int clb_search_batch(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                     int pad_short, int64_t* out_pids, float* out_scores, int64_t* n_cand) {
    const clb_search_request r = {kReq, nullptr, CLB_FILTER_CANDIDATES, pad_short};
    return clb_search_batch_request(s, Q, T, B, nprobe, k, &r, out_pids, out_scores, n_cand);
}

int clb_search_batch_filtered(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                              const clb_filter* const* filters, int scope, int64_t* out_pids, float* out_scores,
                              int64_t* n_cand) {
    const clb_search_request r = {kReq, filters, scope, /*pad_short=*/1};
    return clb_search_batch_request(s, Q, T, B, nprobe, k, &r, out_pids, out_scores, n_cand);
}

int clb_search_batch_grouped(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                             const clb_filter* const* filters, int scope, const clb_grouping* grouping, int pad_short,
                             int64_t* out_pids, float* out_scores, int64_t* n_cand) {
    const clb_search_request r = {kReq, filters, scope, pad_short, grouping};
    return clb_search_batch_request(s, Q, T, B, nprobe, k, &r, out_pids, out_scores, n_cand);
}

int clb_search_batch_grouped_hits(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                                  const clb_filter* const* filters, int scope, const clb_grouping* grouping, int64_t per_group,
                                  int pad_short, int64_t* out_pids, float* out_scores, int64_t* n_cand) {
    CLB_TRY(check_hits_entry(grouping, per_group));
    const clb_search_request r = {kReq, filters, scope, pad_short, grouping, per_group};
    return clb_search_batch_request(s, Q, T, B, nprobe, k, &r, out_pids, out_scores, n_cand);
}

int clb_search_batch_prior(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                           const clb_filter* const* filters, int scope, const clb_grouping* grouping, const clb_prior* prior,
                           float weight, int pad_short, int64_t* out_pids, float* out_scores, int64_t* n_cand) {
    const clb_search_request r = {kReq, filters, scope, pad_short, grouping, 0, 0, prior, weight};
    return clb_search_batch_request(s, Q, T, B, nprobe, k, &r, out_pids, out_scores, n_cand);
}

int clb_search_batch_after(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                           const clb_filter* const* filters, int scope, const float* after_scores, const int64_t* after_pids,
                           int64_t* out_pids, float* out_scores, int64_t* n_cand) {
    CLB_TRY(check_after_entry(s, out_pids, out_scores));
    const clb_search_request r = {kReq, filters, scope, /*pad_short=*/1, nullptr, 0, 0, nullptr, 0.f, nullptr, after_scores, after_pids};
    return clb_search_batch_request(s, Q, T, B, nprobe, k, &r, out_pids, out_scores, n_cand);
}

// the listed entries' own refusal: without lists they would be the unlisted search, which has entries of its own
static int check_listed_entry(const int64_t* list_pids, const int64_t* list_lens) {
    return list_pids || list_lens ? CLB_OK : fail(CLB_EARGUMENT, "list_pids and list_lens are null (without lists: clb_search_batch)");
}

int clb_search_batch_listed(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                            const int64_t* list_pids, const int64_t* list_lens, int64_t list_stride, float* list_scores,
                            int64_t* out_pids, float* out_scores, int64_t* n_cand) {
    CLB_TRY(check_listed_entry(list_pids, list_lens));
    const clb_search_request r = {kReq, nullptr, CLB_FILTER_CANDIDATES, /*pad_short=*/1, nullptr, 0, 0, nullptr, 0.f, nullptr, nullptr,
                                  nullptr, list_pids, list_lens, list_stride, list_scores};
    return clb_search_batch_request(s, Q, T, B, nprobe, k, &r, out_pids, out_scores, n_cand);
}

int clb_search_batch_listed_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                        int64_t k, const int64_t* d_list_pids, const int64_t* d_list_lens, int64_t list_stride,
                                        float* d_list_scores, int64_t* d_out_pids, float* d_out_scores, int64_t* d_n_cand,
                                        void* hip_stream) {
    CLB_TRY(check_listed_entry(d_list_pids, d_list_lens));
    const clb_search_request r = {kReq, nullptr, CLB_FILTER_CANDIDATES, 0, nullptr, 0, 0, nullptr, 0.f, nullptr, nullptr,
                                  nullptr, d_list_pids, d_list_lens, list_stride, d_list_scores};
    return clb_search_batch_request_device_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_out_pids, d_out_scores, d_n_cand, hip_stream);
}

// ... with list priors: the listed request with the value block and the weight (list_prior == NULL: exactly the listed call)
int clb_search_batch_listed_prior(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                                  const int64_t* list_pids, const int64_t* list_lens, int64_t list_stride, const float* list_prior,
                                  float weight, float* list_scores, int64_t* out_pids, float* out_scores, int64_t* n_cand) {
    CLB_TRY(check_listed_entry(list_pids, list_lens));
    const clb_search_request r = {kReq, nullptr, CLB_FILTER_CANDIDATES, /*pad_short=*/1, nullptr, 0, 0, nullptr, weight, list_prior,
                                  nullptr, nullptr, list_pids, list_lens, list_stride, list_scores};
    return clb_search_batch_request(s, Q, T, B, nprobe, k, &r, out_pids, out_scores, n_cand);
}

int clb_search_batch_listed_prior_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                              int64_t k, const int64_t* d_list_pids, const int64_t* d_list_lens,
                                              int64_t list_stride, const float* d_list_prior, float weight, float* d_list_scores,
                                              int64_t* d_out_pids, float* d_out_scores, int64_t* d_n_cand, void* hip_stream) {
    CLB_TRY(check_listed_entry(d_list_pids, d_list_lens));
    const clb_search_request r = {kReq, nullptr, CLB_FILTER_CANDIDATES, 0, nullptr, 0, 0, nullptr, weight, d_list_prior,
                                  nullptr, nullptr, d_list_pids, d_list_lens, list_stride, d_list_scores};
    return clb_search_batch_request_device_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_out_pids, d_out_scores, d_n_cand, hip_stream);
}

int clb_search_shard_phase1(clb_searcher* s, const float* d_Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                            float* d_local_top, void* hip_stream) {
    return clb_search_shard_phase1_slot(s, 0, d_Q, T, B, nprobe, k, d_local_top, hip_stream);
}

int clb_search_shard_phase1_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                 int64_t k, float* d_local_top, void* hip_stream) {
    return clb_search_shard_phase1_filtered_slot(s, slot, d_Q, T, B, nprobe, k, nullptr, CLB_FILTER_CANDIDATES, d_local_top,
                                                 hip_stream);
}

int clb_search_shard_phase1_filtered_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                          int64_t k, const clb_filter* const* filters, int scope, float* d_local_top,
                                          void* hip_stream) {
    const clb_search_request r = {kReq, filters, scope};
    return clb_search_shard_phase1_request_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_local_top, nullptr, nullptr, hip_stream);
}

int clb_search_shard_phase1_grouped_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const clb_filter* const* filters, int scope, const clb_grouping* grouping,
                                         int64_t group_base, float* d_local_top, int64_t* d_local_gid, void* hip_stream) {
    const clb_search_request r = {kReq, filters, scope, 0, grouping, 0, group_base};
    return clb_search_shard_phase1_request_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_local_top, d_local_gid, nullptr, hip_stream);
}

int clb_search_shard_phase1_prior_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                       int64_t k, const clb_filter* const* filters, int scope, const clb_grouping* grouping,
                                       int64_t group_base, const clb_prior* prior, float weight, float* d_local_top,
                                       int64_t* d_local_gid, float* d_local_mabs, void* hip_stream) {
    const clb_search_request r = {kReq, filters, scope, 0, grouping, 0, group_base, prior, weight};
    return clb_search_shard_phase1_request_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_local_top, d_local_gid, d_local_mabs, hip_stream);
}

int clb_search_shard_phase2(clb_searcher* s, const float* d_Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                            const float* d_all_top, int64_t n_shards, int64_t* d_out_pids, float* d_out_scores,
                            int64_t* d_n_cand, void* hip_stream) {
    return clb_search_shard_phase2_slot(s, 0, d_Q, T, B, nprobe, k, d_all_top, n_shards, d_out_pids, d_out_scores, d_n_cand,
                                        hip_stream);
}

int clb_search_shard_phase2_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                 int64_t k, const float* d_all_top, int64_t n_shards, int64_t* d_out_pids,
                                 float* d_out_scores, int64_t* d_n_cand, void* hip_stream) {
    const clb_search_request r = {kReq};
    return clb_search_shard_phase2_request_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_all_top, nullptr, nullptr, n_shards, d_out_pids,
                                                d_out_scores, nullptr, d_n_cand, nullptr, hip_stream);
}

int clb_search_shard_phase2_grouped_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const float* d_all_top, const int64_t* d_all_gid, int64_t n_shards,
                                         const clb_grouping* grouping, int64_t group_base, int64_t* d_out_pids,
                                         float* d_out_scores, int64_t* d_out_gids, int64_t* d_n_cand, int64_t* d_edge_gids,
                                         void* hip_stream) {
    if (!grouping) return fail(CLB_EARGUMENT, "grouping is null (without one: clb_search_shard_phase2_slot)");
    const clb_search_request r = {kReq, nullptr, CLB_FILTER_CANDIDATES, 0, grouping, 0, group_base};
    return clb_search_shard_phase2_request_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_all_top, d_all_gid, nullptr, n_shards,
                                                d_out_pids, d_out_scores, d_out_gids, d_n_cand, d_edge_gids, hip_stream);
}

int clb_search_shard_phase2_prior_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                       int64_t k, const float* d_all_top, const int64_t* d_all_gid, const float* d_all_mabs,
                                       int64_t n_shards, const clb_grouping* grouping, int64_t group_base, const clb_prior* prior,
                                       float weight, int64_t* d_out_pids, float* d_out_scores, int64_t* d_out_gids,
                                       int64_t* d_n_cand, int64_t* d_edge_gids, void* hip_stream) {
    if (!prior)
        return fail(CLB_EARGUMENT, "prior is null (without one: clb_search_shard_phase2_slot / clb_search_shard_phase2_grouped_slot)");
    const clb_search_request r = {kReq, nullptr, CLB_FILTER_CANDIDATES, 0, grouping, 0, group_base, prior, weight};
    return clb_search_shard_phase2_request_slot(s, slot, d_Q, T, B, nprobe, k, &r, d_all_top, d_all_gid, d_all_mabs, n_shards,
                                                d_out_pids, d_out_scores, d_out_gids, d_n_cand, d_edge_gids, hip_stream);
}

int clb_search_result_groups_slot(clb_searcher* s, int slot, const clb_grouping* grouping, int64_t group_base,
                                  const int64_t* d_pids, int64_t B, int64_t k, int64_t* d_out_gids, int64_t* d_edge_gids,
                                  void* hip_stream) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (!grouping) return fail(CLB_EARGUMENT, "grouping is null");
    if (!d_pids || !d_out_gids || !d_edge_gids) return fail(CLB_EARGUMENT, "d_pids, d_out_gids or d_edge_gids is null");
    if (B < 1 || k < 1 || group_base < 0) return fail(CLB_EARGUMENT, "B and k must be >= 1 and group_base >= 0");
    CLB_TRY(check_grouping(s, grouping));       // (not a search: it carries no request)
    Workspace* wp = nullptr;
    CLB_TRY(slot_workspace(s, slot, &wp));
    const auto& d = wp->grouped_done;
    if (!d.valid || d.B != B || d.k != k || d.grp != grouping || d.stream != hip_stream || d.generation != s->generation)
        return fail(CLB_EARGUMENT, "clb_search_result_groups_slot without a matching clb_search_batch_grouped_device_slot on this "
                                   "workspace slot (same grouping, B <= %lld, k and stream, and nothing else on the slot in between)",
                    (long long)kSubBatch);
    launch_result_groups(s, *wp, (hipStream_t)hip_stream, grouping, group_base, d_pids, (int)B, (int)k, d_out_gids, d_edge_gids);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

// ---- clb_prior ----------------------------------------------------------------------------------------------------
using PriorPtr = std::unique_ptr<clb_prior, decltype(&clb_prior_destroy)>;
// the arguments both creators share, checked before the device is touched
static int prior_args(clb_searcher* s, const float* values, int64_t n, clb_prior** out) {
    if (out) *out = nullptr;
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (!out) return fail(CLB_EARGUMENT, "out is null");
    if (n != s->n_docs)
        return fail(CLB_EARGUMENT, "a prior holds one value per passage: n=%lld, the searcher has %lld passages", (long long)n,
                    (long long)s->n_docs);
    if (n > 0 && !values) return fail(CLB_EARGUMENT, "values is null");
    return CLB_OK;
}
// a prior of s with its values allocated, on s's device
static int prior_alloc(clb_searcher* s, int64_t n, PriorPtr& p) {
    CLB_TRY(use_device(s->device));
    p.reset(new clb_prior());
    p->owner = s->serial; p->device = s->device; p->n_docs = n;
    return p->values.alloc(sizeof(float) * (size_t)n);
}
static int bad_prior_value(const clb_searcher* s, int64_t i) {
    return fail(CLB_EARGUMENT, "the prior of passage %lld is not a finite number", (long long)(s->pid_offset + i + 1));
}

int clb_prior_create(clb_searcher* s, const float* values, int64_t n, clb_prior** out) {
    PriorPtr p(nullptr, clb_prior_destroy);
    CLB_TRY(prior_args(s, values, n, out));
    float max_abs = 0.f;            // finiteness and the maximum on the host, before anything is allocated
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(values[i])) return bad_prior_value(s, i);
        max_abs = std::max(max_abs, std::fabs(values[i]));
    }
    CLB_TRY(prior_alloc(s, n, p));
    p->max_abs = max_abs;
    if (n > 0) {       // the library never retains a host pointer
        CLB_HIP(hipMemcpyAsync(p->values.p, values, sizeof(float) * n, hipMemcpyHostToDevice, s->stream));
        CLB_HIP(hipStreamSynchronize(s->stream));
    }
    *out = p.release();
    return CLB_OK;
}

int clb_prior_create_device(clb_searcher* s, const float* d_values, int64_t n, clb_prior** out) {
    PriorPtr p(nullptr, clb_prior_destroy);
    CLB_TRY(prior_args(s, d_values, n, out));
    CLB_TRY(prior_alloc(s, n, p));
    if (n > 0) {
        CLB_HIP(hipDeviceSynchronize());      // whatever wrote the caller's device array
        const hipStream_t st = s->stream;
        CLB_HIP(hipMemcpyAsync(p->values.p, d_values, sizeof(float) * n, hipMemcpyDeviceToDevice, st));
        // first non-finite value and max |value| on the device, one read-back
        DevBuf d_res;
        const unsigned long long init[2] = {(unsigned long long)n, 0ull};
        unsigned long long res[2] = {0ull, 0ull};
        CLB_TRY(upload(d_res, init, sizeof init, st));
        hipLaunchKernelGGL(prior_check_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (n + 255) / 256))), dim3(256),
                           0, st, (const float*)p->values.as<float>(), n, d_res.as<unsigned long long>());
        CLB_HIP(hipMemcpyAsync(res, d_res.p, sizeof res, hipMemcpyDeviceToHost, st));
        CLB_HIP(hipStreamSynchronize(st));
        CLB_HIP(hipGetLastError());
        if (res[0] < (unsigned long long)n) return bad_prior_value(s, (int64_t)res[0]);
        const uint32_t bits = (uint32_t)res[1];
        memcpy(&p->max_abs, &bits, sizeof bits);
    }
    *out = p.release();
    return CLB_OK;
}

float clb_prior_max_abs(const clb_prior* p) { return p ? p->max_abs : 0.f; }

int clb_prior_destroy(clb_prior* p) {
    if (!p) return CLB_OK;
    (void)hipSetDevice(p->device);
    delete p;
    return CLB_OK;
}

// ---- clb_grouping -------------------------------------------------------------------------------------------------
int clb_grouping_create(clb_searcher* s, const int64_t* group_ids, int64_t n, clb_grouping** out) {
    if (out) *out = nullptr;
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (!out) return fail(CLB_EARGUMENT, "out is null");
    if (n != s->n_docs)
        return fail(CLB_EARGUMENT, "a grouping holds one group id per passage: n=%lld, the searcher has %lld passages", (long long)n,
                    (long long)s->n_docs);
    if (n > 0 && !group_ids) return fail(CLB_EARGUMENT, "group_ids is null");
    // equal ids must be one contiguous pid range: checked on the host, before anything is allocated
    for (int64_t i = 1; i < n; ++i)
        if (group_ids[i] < group_ids[i - 1])
            return fail(CLB_EARGUMENT, "group ids must be non-decreasing in pid: they decrease at passage %lld (%lld after %lld)",
                        (long long)(s->pid_offset + i + 1), (long long)group_ids[i], (long long)group_ids[i - 1]);
    CLB_TRY(use_device(s->device));
    std::unique_ptr<clb_grouping, decltype(&clb_grouping_destroy)> g(new clb_grouping(), clb_grouping_destroy);
    g->owner = s->serial; g->device = s->device; g->n_docs = n;
    if (n > 0) {
        hipStream_t st = s->stream;
        DevBuf d_ids, flag, before;
        CLB_TRY(g->gid.alloc(sizeof(uint32_t) * (size_t)n));
        CLB_TRY(upload(d_ids, group_ids, sizeof(int64_t) * n, st));
        CLB_TRY(flag.alloc(sizeof(uint32_t) * (size_t)(n + 1)));
        CLB_TRY(before.alloc(sizeof(uint32_t) * (size_t)(n + 1)));
        const dim3 blocks((unsigned)((n + 1 + 255) / 256));
        hipLaunchKernelGGL(grouping_flags_kernel, blocks, dim3(256), 0, st, d_ids.as<int64_t>(), n, flag.as<uint32_t>());
        CLB_TRY(exclusive_scan_u32(flag.as<uint32_t>(), before.as<uint32_t>(), (size_t)n, st));
        hipLaunchKernelGGL(grouping_index_kernel, blocks, dim3(256), 0, st, flag.as<uint32_t>(), before.as<uint32_t>(), n,
                           g->gid.as<uint32_t>());
        uint32_t total = 0;     // the heads among passages 1 .. n - 1
        CLB_HIP(hipMemcpyAsync(&total, before.as<uint32_t>() + n, sizeof total, hipMemcpyDeviceToHost, st));
        CLB_HIP(hipStreamSynchronize(st));      // ... before the scratch and the host array go away
        CLB_HIP(hipGetLastError());
        g->count = (int64_t)total + 1;
    }
    *out = g.release();
    return CLB_OK;
}

int64_t clb_grouping_count(const clb_grouping* g) { return g ? g->count : 0; }

int clb_grouping_destroy(clb_grouping* g) {
    if (!g) return CLB_OK;
    (void)hipSetDevice(g->device);
    delete g;
    return CLB_OK;
}

// ---- clb_filter ---------------------------------------------------------------------------------------------------
// the words are on the device: clear the tail bits, count once (creation may synchronise, searching never reads the count back)
static int filter_finish(clb_searcher* s, FilterPtr f, clb_filter** out) {
    DevWord<unsigned long long> cnt;
    const int W = (int)((s->n_docs + 31) / 32);
    CLB_TRY(cnt.init(s->stream));
    if (W > 0)
        hipLaunchKernelGGL(filter_count_kernel, dim3((unsigned)std::max(1, std::min(1024, (W + 255) / 256))), dim3(256), 0, s->stream,
                           f->bits.as<uint32_t>(), W, (int)s->n_docs, cnt.ptr());
    CLB_TRY(cnt.read(s->stream));
    f->count = (int64_t)cnt.value;
    *out = f.release();
    return CLB_OK;
}
// a filter of s with its words allocated, on s's device; the callers have checked their arguments
static int filter_new(const clb_searcher* s, FilterPtr& f) {
    CLB_TRY(use_device(s->device));
    f.reset(new clb_filter());
    f->owner = s->serial; f->device = s->device; f->n_docs = s->n_docs;
    return f->bits.alloc(sizeof(uint32_t) * (size_t)((s->n_docs + 31) / 32));
}

int clb_filter_create_pids(clb_searcher* s, const int64_t* pids, int64_t n, clb_filter** out) {
    if (out) *out = nullptr;
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (!out) return fail(CLB_EARGUMENT, "out is null");
    if (n < 0 || (n > 0 && !pids)) return fail(CLB_EARGUMENT, "pids is null or n < 0");
    for (int64_t i = 0; i < n; ++i)
        if (pids[i] <= s->pid_offset || pids[i] > s->pid_offset + s->n_docs)
            return fail(CLB_EBOUNDS, "pid %lld (entry %lld) outside %lld..%lld", (long long)pids[i], (long long)i,
                        (long long)(s->pid_offset + 1), (long long)(s->pid_offset + s->n_docs));
    FilterPtr f(nullptr, clb_filter_destroy);
    CLB_TRY(filter_new(s, f));
    CLB_HIP(hipMemsetAsync(f->bits.p, 0, f->bits.bytes, s->stream));
    if (n > 0) {
        DevBuf d_pids;
        DevWord<int> err;
        CLB_TRY(upload(d_pids, pids, sizeof(int64_t) * n, s->stream));
        CLB_TRY(err.init(s->stream));
        hipLaunchKernelGGL(filter_mark_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, d_pids.as<int64_t>(),
                           n, s->pid_offset, (int)s->n_docs, f->bits.as<uint32_t>(), err.ptr());
        CLB_TRY(err.read(s->stream));        // ... before d_pids and the host array go away
        if (err.value) return fail(CLB_EBOUNDS, "a pid outside the searcher's passages");
    }
    return filter_finish(s, std::move(f), out);
}

int clb_filter_create_pids_global(clb_searcher* s, const int64_t* pids, int64_t n, clb_filter** out, int64_t* n_inside) {
    if (out) *out = nullptr;
    if (n_inside) *n_inside = 0;
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (!out || !n_inside) return fail(CLB_EARGUMENT, "out or n_inside is null");
    if (n < 0 || (n > 0 && !pids)) return fail(CLB_EARGUMENT, "pids is null or n < 0");
    FilterPtr f(nullptr, clb_filter_destroy);
    CLB_TRY(filter_new(s, f));
    CLB_HIP(hipMemsetAsync(f->bits.p, 0, f->bits.bytes, s->stream));
    if (n > 0) {       // range test, marking and count in one pass over the list, on the device
        DevBuf d_pids;
        DevWord<int> err;
        DevWord<unsigned long long> inside;
        CLB_TRY(upload(d_pids, pids, sizeof(int64_t) * n, s->stream));
        CLB_TRY(err.init(s->stream));
        CLB_TRY(inside.init(s->stream));
        hipLaunchKernelGGL(filter_mark_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream,
                           d_pids.as<int64_t>(), n, s->pid_offset, (int)s->n_docs, f->bits.as<uint32_t>(), err.ptr(), inside.ptr());
        CLB_TRY(err.read(s->stream));        // ... before d_pids and the host array go away
        CLB_TRY(inside.read(s->stream));
        if (err.value) return fail(CLB_EBOUNDS, "a pid < 1 in a global pid list");
        *n_inside = (int64_t)inside.value;
    }
    return filter_finish(s, std::move(f), out);
}

int clb_filter_create_bitmap(clb_searcher* s, const uint32_t* words, int64_t n_words, clb_filter** out) {
    if (out) *out = nullptr;
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (!out) return fail(CLB_EARGUMENT, "out is null");
    const int64_t W = (s->n_docs + 31) / 32;
    if (n_words != W) return fail(CLB_EARGUMENT, "n_words=%lld, the searcher's bitmap has ceil(n_docs / 32) = %lld words", (long long)n_words, (long long)W);
    if (W > 0 && !words) return fail(CLB_EARGUMENT, "words is null");
    FilterPtr f(nullptr, clb_filter_destroy);
    CLB_TRY(filter_new(s, f));
    if (W > 0) {       // the library never retains a host pointer
        CLB_HIP(hipMemcpyAsync(f->bits.p, words, sizeof(uint32_t) * W, hipMemcpyHostToDevice, s->stream));
        CLB_HIP(hipStreamSynchronize(s->stream));
    }
    return filter_finish(s, std::move(f), out);
}

// ---- composing filters on the device (filter_kernels.hpp): each writes the words of a fresh bitmap on the searcher's stream
// and ends in filter_finish, which clears the tail bits and counts with creation's one read-back
static unsigned word_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

int clb_filter_combine(clb_searcher* s, int op, const clb_filter* const* operands, int64_t n, clb_filter** out) {
    if (out) *out = nullptr;
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (!out) return fail(CLB_EARGUMENT, "out is null");
    if (op < CLB_FILTER_OP_AND || op > CLB_FILTER_OP_NOT)
        return fail(CLB_EARGUMENT, "op must be CLB_FILTER_OP_AND (0), _OR (1), _ANDNOT (2) or _NOT (3), got %d", op);
    if (n < 1 || n > CLB_MAX_FILTER_OPERANDS)
        return fail(CLB_EARGUMENT, "n must be 1..%d operands, got %lld", CLB_MAX_FILTER_OPERANDS, (long long)n);
    if (op == CLB_FILTER_OP_NOT && n != 1)
        return fail(CLB_EARGUMENT, "CLB_FILTER_OP_NOT takes n = 1 operand, got %lld", (long long)n);
    if (!operands) return fail(CLB_EARGUMENT, "operands is null");
    for (int64_t i = 0; i < n; ++i)
        if (!operands[i]) return fail(CLB_EARGUMENT, "operand %lld is null", (long long)i);
    for (int64_t i = 0; i < n; ++i) {         // check_filters' rules and wording, by operand
        if (operands[i]->owner != s->serial)
            return fail(CLB_EARGUMENT, "the filter of operand %lld was made for another searcher", (long long)i);
        if (operands[i]->n_docs != s->n_docs)
            return fail(CLB_EARGUMENT, "the filter of operand %lld: filter made before an append; make another", (long long)i);
    }
    FilterPtr f(nullptr, clb_filter_destroy);
    CLB_TRY(filter_new(s, f));
    const int W = (int)((s->n_docs + 31) / 32);
    if (W > 0) {
        FilterOperands ops = {};
        ops.n = (int)n;
        for (int64_t i = 0; i < n; ++i) ops.bits[i] = operands[i]->bits.as<uint32_t>();
        hipLaunchKernelGGL(filter_combine_kernel, dim3(word_blocks(W)), dim3(256), 0, s->stream, ops, op, W, f->bits.as<uint32_t>());
    }
    return filter_finish(s, std::move(f), out);
}

int clb_filter_create_range(clb_searcher* s, const clb_prior* values, float lo, float hi, int flags, clb_filter** out) {
    if (out) *out = nullptr;
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (!out) return fail(CLB_EARGUMENT, "out is null");
    if (!values) return fail(CLB_EARGUMENT, "values is null: a range is taken over a clb_prior");
    if (lo != lo) return fail(CLB_EARGUMENT, "lo is NaN");
    if (hi != hi) return fail(CLB_EARGUMENT, "hi is NaN");
    if (flags & ~(CLB_RANGE_LO_OPEN | CLB_RANGE_HI_OPEN))
        return fail(CLB_EARGUMENT, "flags must be a combination of CLB_RANGE_LO_OPEN (1) and CLB_RANGE_HI_OPEN (2), got %d", flags);
    CLB_TRY(check_prior(s, values, 0.f));     // this searcher's, made for the passages it holds now
    FilterPtr f(nullptr, clb_filter_destroy);
    CLB_TRY(filter_new(s, f));
    const int W = (int)((s->n_docs + 31) / 32);
    if (W > 0)
        hipLaunchKernelGGL(filter_range_kernel, dim3(word_blocks(s->n_docs)), dim3(256), 0, s->stream,
                           (const float*)values->values.as<float>(), (int)s->n_docs, lo, hi, flags & CLB_RANGE_LO_OPEN,
                           flags & CLB_RANGE_HI_OPEN, W, f->bits.as<uint32_t>());
    return filter_finish(s, std::move(f), out);
}

int clb_filter_extend(clb_searcher* s, const clb_filter* f_old, int fill, clb_filter** out) {
    if (out) *out = nullptr;
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    if (!out) return fail(CLB_EARGUMENT, "out is null");
    if (!f_old) return fail(CLB_EARGUMENT, "f is null");
    if (fill != 0 && fill != 1) return fail(CLB_EARGUMENT, "fill must be 0 (appended passages out) or 1 (in), got %d", fill);
    if (f_old->owner != s->serial) return fail(CLB_EARGUMENT, "the filter f was made for another searcher");
    if (f_old->n_docs > s->n_docs)       // (a handle never loses passages: not reachable through this library)
        return fail(CLB_EARGUMENT, "the filter f holds %lld passages, the searcher %lld", (long long)f_old->n_docs, (long long)s->n_docs);
    FilterPtr f(nullptr, clb_filter_destroy);
    CLB_TRY(filter_new(s, f));
    const int W = (int)((s->n_docs + 31) / 32);
    if (W > 0)
        hipLaunchKernelGGL(filter_extend_kernel, dim3(word_blocks(W)), dim3(256), 0, s->stream,
                           (const uint32_t*)f_old->bits.as<uint32_t>(), (int)f_old->n_docs, fill ? ~0u : 0u, W, f->bits.as<uint32_t>());
    return filter_finish(s, std::move(f), out);
}

int clb_filter_bitmap(const clb_filter* f, uint32_t* words, int64_t n_words) {
    if (!f) return fail(CLB_EARGUMENT, "f is null");
    const int64_t W = (f->n_docs + 31) / 32;
    if (n_words != W)
        return fail(CLB_EARGUMENT, "n_words=%lld, the filter's bitmap has ceil(n_docs / 32) = %lld words", (long long)n_words, (long long)W);
    if (W > 0 && !words) return fail(CLB_EARGUMENT, "words is null");
    if (W == 0) return CLB_OK;
    CLB_TRY(use_device(f->device));
    // creation ended with the read-back of the count on the stream that wrote the words: they are complete
    CLB_HIP(hipMemcpy(words, f->bits.p, sizeof(uint32_t) * W, hipMemcpyDeviceToHost));
    return CLB_OK;
}

int64_t clb_filter_count(const clb_filter* f) { return f ? f->count : 0; }

int clb_filter_destroy(clb_filter* f) {
    if (!f) return CLB_OK;
    (void)hipSetDevice(f->device);
    delete f;
    return CLB_OK;
}

int clb_search(clb_searcher* s, const float* Q, int64_t T, int64_t nprobe, int64_t k, int64_t* out_pids,
               float* out_scores, int64_t* n_cand) {
    return clb_search_batch(s, Q, T, 1, nprobe, k, 0, out_pids, out_scores, n_cand);
}

int clb_retrieve(clb_searcher* s, const float* Q, int64_t T, int64_t nprobe, int64_t* out_pids,
                 int64_t* n_out) {
    CLB_TRY(check_search_args(s, T, 1, nprobe, 1));
    CLB_TRY(use_device(s->device));
    Workspace& w = s->ws[0];
    w.pending.valid = false;
    CLB_TRY(ensure_workspace(s, w, 1, T, nprobe, 1));
    hipStream_t st = s->stream;
    CLB_HIP(hipMemcpyAsync(w.Qdev.p, Q, sizeof(float) * T * s->dim, hipMemcpyHostToDevice, st));
    const Batch q = make_batch(w.Qdev.as<float>(), 1, T, nprobe, 1);     // one query, no filter
    if (s->generic || T > 128) CLB_TRY(run_retrieve_general(s, w, st, q, 0));
    else CLB_TRY(run_retrieve(s, w, st, q));
    int nc = 0;
    CLB_HIP(hipMemcpyAsync(&nc, w.ncand.p, sizeof(int), hipMemcpyDeviceToHost, st));
    CLB_HIP(hipStreamSynchronize(st));
    std::vector<uint32_t> c((size_t)nc);
    if (nc) CLB_HIP(hipMemcpy(c.data(), w.cand.p, sizeof(uint32_t) * nc, hipMemcpyDeviceToHost));
    for (int i = 0; i < nc; ++i) out_pids[i] = s->pid_offset + (int64_t)c[i] + 1;
    *n_out = nc;
    return CLB_OK;
}

static int merge_topk_launch(int device, const int64_t* d_pids, const float* d_scores, int64_t k, int64_t n_lists,
                             int64_t B, size_t pid_stride, size_t score_stride, int64_t* d_out_pids,
                             float* d_out_scores, void* hip_stream) {
    if (k < 1 || n_lists < 1 || B < 1) return fail(CLB_EARGUMENT, "k, n_lists and B must be >= 1");
    CLB_TRY(use_device(device));
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(fill_pad_kernel, dim3((unsigned)((B * k + 255) / 256)), dim3(256), 0, st, d_out_pids,
                       d_out_scores, B * k);
    hipLaunchKernelGGL(merge_topk_kernel, dim3((unsigned)((n_lists * k + 255) / 256), (unsigned)B), dim3(256), 0, st,
                       d_pids, d_scores, (int)k, (int)n_lists, (int)B, pid_stride, score_stride, d_out_pids,
                       d_out_scores);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

int clb_merge_topk_device(int device, const int64_t* d_pids, const float* d_scores, int64_t k, int64_t n_lists,
                          int64_t B, int64_t* d_out_pids, float* d_out_scores, void* hip_stream) {
    return merge_topk_launch(device, d_pids, d_scores, k, n_lists, B, (size_t)(B * k), (size_t)(B * k), d_out_pids,
                             d_out_scores, hip_stream);
}

int64_t clb_packed_topk_bytes(int64_t k, int64_t B) { return (B * k * 12 + 7) / 8 * 8; }

static int merge_topk_grouped_launch(int device, const int64_t* d_pids, const float* d_scores, const int64_t* d_gids, int64_t k,
                                     int64_t n_lists, int64_t B, size_t pid_stride, size_t score_stride, size_t gid_stride,
                                     const int64_t* d_n_cand_lists, size_t n_cand_stride, const int64_t* d_edge_gids,
                                     size_t edge_stride, int64_t* d_out_pids, float* d_out_scores, int64_t* d_out_n_cand,
                                     void* hip_stream) {
    if (k < 1 || n_lists < 1 || B < 1) return fail(CLB_EARGUMENT, "k, n_lists and B must be >= 1");
    if (!d_pids || !d_scores || !d_gids || !d_n_cand_lists || !d_edge_gids)
        return fail(CLB_EARGUMENT, "an input of the grouped merge is null");
    if (!d_out_pids || !d_out_scores || !d_out_n_cand) return fail(CLB_EARGUMENT, "an output of the grouped merge is null");
    if (n_lists > kMaxGroupShards)
        return fail(CLB_EUNSUPPORTED, "the grouped merge takes at most %d lists, got %lld", kMaxGroupShards, (long long)n_lists);
    if (n_lists * k > INT32_MAX) return fail(CLB_EUNSUPPORTED, "n_lists * k exceeds 2^31 - 1");
    CLB_TRY(use_device(device));
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(fill_pad_kernel, dim3((unsigned)((B * k + 255) / 256)), dim3(256), 0, st, d_out_pids, d_out_scores, B * k);
    hipLaunchKernelGGL(merge_topk_grouped_kernel, dim3((unsigned)((n_lists * k + 255) / 256), (unsigned)B), dim3(256), 0, st,
                       d_pids, d_scores, d_gids, (int)k, (int)n_lists, (int)B, pid_stride, score_stride, gid_stride,
                       d_n_cand_lists, n_cand_stride, d_edge_gids, edge_stride, d_out_pids, d_out_scores, d_out_n_cand);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

int clb_merge_topk_grouped_device(int device, const int64_t* d_pids, const float* d_scores, const int64_t* d_gids, int64_t k,
                                  int64_t n_lists, int64_t B, const int64_t* d_n_cand_lists, const int64_t* d_edge_gids,
                                  int64_t* d_out_pids, float* d_out_scores, int64_t* d_out_n_cand, void* hip_stream) {
    return merge_topk_grouped_launch(device, d_pids, d_scores, d_gids, k, n_lists, B, (size_t)(B * k), (size_t)(B * k),
                                     (size_t)(B * k), d_n_cand_lists, (size_t)B, d_edge_gids, (size_t)(2 * B), d_out_pids,
                                     d_out_scores, d_out_n_cand, hip_stream);
}

int64_t clb_packed_grouped_bytes(int64_t k, int64_t B) { return clb_packed_topk_bytes(k, B) + 8 * B * k + 8 * B + 16 * B; }

int clb_merge_topk_grouped_packed_device(int device, const void* d_packed, int64_t k, int64_t n_lists, int64_t B,
                                         int64_t* d_out_pids, float* d_out_scores, int64_t* d_out_n_cand, void* hip_stream) {
    if (k < 1 || B < 1) return fail(CLB_EARGUMENT, "k, n_lists and B must be >= 1");
    if (!d_packed) return fail(CLB_EARGUMENT, "d_packed is null");
    const size_t block = (size_t)clb_packed_grouped_bytes(k, B);       // a multiple of 8
    const size_t at_gids = (size_t)clb_packed_topk_bytes(k, B), at_n = at_gids + (size_t)B * k * 8, at_edges = at_n + (size_t)B * 8;
    const char* base = static_cast<const char*>(d_packed);
    return merge_topk_grouped_launch(device, reinterpret_cast<const int64_t*>(base),
                                     reinterpret_cast<const float*>(base + (size_t)B * k * 8),
                                     reinterpret_cast<const int64_t*>(base + at_gids), k, n_lists, B, block / 8, block / 4, block / 8,
                                     reinterpret_cast<const int64_t*>(base + at_n), block / 8,
                                     reinterpret_cast<const int64_t*>(base + at_edges), block / 8, d_out_pids, d_out_scores,
                                     d_out_n_cand, hip_stream);
}

int clb_debug_group_tau_device(const float* d_all_top, const int64_t* d_all_gid, int64_t n_shards, int64_t B, int64_t k,
                               float* d_tau, void* hip_stream) {
    if (!d_all_top || !d_all_gid || !d_tau) return fail(CLB_EARGUMENT, "d_all_top, d_all_gid or d_tau is null");
    if (n_shards < 1 || B < 1 || k < 1) return fail(CLB_EARGUMENT, "n_shards, B and k must be >= 1");
    if (n_shards > kMaxGroupShards)
        return fail(CLB_EUNSUPPORTED, "at most %d shards, got %lld", kMaxGroupShards, (long long)n_shards);
    if (n_shards * k > INT32_MAX) return fail(CLB_EUNSUPPORTED, "n_shards * k exceeds 2^31 - 1");
    hipLaunchKernelGGL(group_global_tau_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)hip_stream, d_all_top, d_all_gid,
                       (int)n_shards, (int)B, (int)k, d_tau);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

int clb_debug_prior_tau_device(const float* d_all_top, const int64_t* d_all_gid, const float* d_all_mabs, const float* d_eps,
                               int64_t n_shards, int64_t B, int64_t k, float* d_tau_in, void* hip_stream) {
    if (!d_all_top || !d_all_mabs || !d_eps || !d_tau_in)
        return fail(CLB_EARGUMENT, "d_all_top, d_all_mabs, d_eps or d_tau_in is null");
    if (n_shards < 1 || B < 1 || k < 1) return fail(CLB_EARGUMENT, "n_shards, B and k must be >= 1");
    if (d_all_gid && n_shards > kMaxGroupShards)
        return fail(CLB_EUNSUPPORTED, "at most %d shards with group indices, got %lld", kMaxGroupShards, (long long)n_shards);
    if (n_shards * k > INT32_MAX) return fail(CLB_EUNSUPPORTED, "n_shards * k exceeds 2^31 - 1");
    hipLaunchKernelGGL(prior_global_tau_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)hip_stream, d_all_top, d_all_gid,
                       d_all_mabs, (int)n_shards, (int)B, (int)k, d_eps, (const float*)nullptr, 0, ApproxConsts{},
                       (const float4*)nullptr, 0, d_tau_in);
    CLB_HIP(hipGetLastError());
    return CLB_OK;
}

int clb_merge_topk_packed_device(int device, const void* d_packed, int64_t k, int64_t n_lists, int64_t B,
                                 int64_t* d_out_pids, float* d_out_scores, void* hip_stream) {
    if (k < 1 || B < 1) return fail(CLB_EARGUMENT, "k, n_lists and B must be >= 1");
    const size_t block = (size_t)clb_packed_topk_bytes(k, B);
    const char* base = static_cast<const char*>(d_packed);
    return merge_topk_launch(device, reinterpret_cast<const int64_t*>(base),
                             reinterpret_cast<const float*>(base + (size_t)B * k * 8), k, n_lists, B, block / 8, block / 4,
                             d_out_pids, d_out_scores, hip_stream);
}

int clb_debug_scores(clb_searcher* s, const float* Q, int64_t T, int64_t nprobe, int64_t k, int64_t cap,
                     int64_t* out_pids, float* out_approx, float* out_exact, int64_t* n_out, float* tau,
                     float* eps, int64_t* n_rescore) {
    CLB_TRY(check_search_args(s, T, 1, nprobe, k));
    if (!s->approx_ok || T > 32) return fail(CLB_EUNSUPPORTED, "two-pass mode not available for this index/query");
    CLB_TRY(use_device(s->device));
    Workspace& w = s->ws[0];
    w.pending.valid = false;
    // 8-bit score rows exist for batches of 16+ queries only: the query then runs as sixteen copies of itself (the report is
    // copy 0's), so that this hook sees the table format, the scaled query operand and the bound a real batch gets
    const int Bd = cell8_rows(s) ? kTeamQueries : 1;
    CLB_TRY(ensure_workspace(s, w, Bd, T, nprobe, k));
    hipStream_t st = s->stream;
    for (int c = 0; c < Bd; ++c)
        CLB_HIP(hipMemcpyAsync(w.Qdev.as<float>() + (size_t)c * T * kDim, Q, sizeof(float) * T * kDim, hipMemcpyHostToDevice, st));
    const float* dQ = w.Qdev.as<float>();
    {   // the fp16 score table pass 1 gathers from is only written in two-pass mode: on a handle set to the exact mode the
        // hook would otherwise score against whatever an earlier query left in the slot (or nothing at all)
        const int mode = s->mode;
        s->mode = 1;
        const int rc = run_retrieve(s, w, st, make_batch(dQ, Bd, T, nprobe, k));     // no filter
        s->mode = mode;
        CLB_TRY(rc);
    }
    launch_pass1(s, w, st, dQ, dim3(8 * 32), Bd, (int)T);
    const BoundOperands bo = bound_operands(s, w);      // the bound a search of this table reports (launch_select)
    hipLaunchKernelGGL(select_margin_kernel, dim3(1), dim3(1024), 0, st, w.scores.as<float>(), w.ncand.as<int>(), dQ,
                       (int)T, (int)k, w.cand_cap, bo.ac, w.list.as<int>(), w.nlist.as<int>(),
                       w.thresh.as<float>(), w.eps_pair.as<float>(), (const float*)nullptr, 0, bo.tscale, bo.cell8);
    int nc = 0, nl = 0;
    float th[2];
    CLB_HIP(hipMemcpyAsync(&nc, w.ncand.p, sizeof(int), hipMemcpyDeviceToHost, st));
    CLB_HIP(hipMemcpyAsync(&nl, w.nlist.p, sizeof(int), hipMemcpyDeviceToHost, st));
    CLB_HIP(hipMemcpyAsync(th, w.thresh.p, sizeof th, hipMemcpyDeviceToHost, st));
    CLB_HIP(hipStreamSynchronize(st));
    if (nc > cap) return fail(CLB_EARGUMENT, "output capacity %lld < %d candidates", (long long)cap, nc);
    std::vector<uint32_t> c((size_t)nc);
    if (nc) {
        CLB_HIP(hipMemcpy(c.data(), w.cand.p, sizeof(uint32_t) * nc, hipMemcpyDeviceToHost));
        CLB_HIP(hipMemcpy(out_approx, w.scores.p, sizeof(float) * nc, hipMemcpyDeviceToHost));
    }
    switch (s->nbits) {
        case 2: launch_score_exact<2>(s, w, st, dQ, 1, (int)T, nullptr, nullptr, 2048); break;
        default: return fail(CLB_EUNSUPPORTED, "nbits");
    }
    CLB_HIP(hipGetLastError());
    CLB_HIP(hipStreamSynchronize(st));
    if (nc) CLB_HIP(hipMemcpy(out_exact, w.scores.p, sizeof(float) * nc, hipMemcpyDeviceToHost));
    for (int i = 0; i < nc; ++i) out_pids[i] = s->pid_offset + (int64_t)c[i] + 1;
    *n_out = nc; *tau = th[0]; *eps = th[1]; *n_rescore = nl;
    return CLB_OK;
}

int clb_profile_enable(clb_searcher* s, int on) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    s->prof.on = on != 0;
    s->prof.counters = on >= 2;
    return CLB_OK;
}

int clb_profile_read(clb_searcher* s, const char** names, double* total_ms, int64_t* launches, int cap) {
    if (!s) return 0;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    int n = 0;
    std::vector<hipEvent_t> seen;       // chained kernels share events: every event goes back to the pool once
    s->prof.chain = nullptr;
    for (int id = 0; id < KID_COUNT && n < cap; ++id) {
        for (auto& pr : s->prof.pending[id]) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                s->prof.total_ms[id] += ms;
                s->prof.launches[id] += 1;
            }
            seen.push_back(pr.first);
            seen.push_back(pr.second);
        }
        s->prof.pending[id].clear();
        names[n] = kKernelNames[id];
        total_ms[n] = s->prof.total_ms[id];
        launches[n] = s->prof.launches[id];
        s->prof.total_ms[id] = 0;
        s->prof.launches[id] = 0;
        ++n;
    }
    std::sort(seen.begin(), seen.end());
    seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
    s->prof.pool.insert(s->prof.pool.end(), seen.begin(), seen.end());
    if (s->prof.failed) {               // some launches went untimed: the totals above are incomplete
        s->prof.failed = false;
        (void)fail(CLB_EHIP, "HIP event creation/record failed while profiling: timings are incomplete");
        return -1;
    }
    return n;
}

int clb_last_batch_stats(clb_searcher* s, int64_t* cand_docs, int64_t* cand_embs, int64_t* rescored_docs,
                         int64_t* rescored_embs) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    CLB_TRY(use_device(s->device));
    CLB_HIP(hipDeviceSynchronize());
    // computed on demand from the device-side counts of the last batch
    unsigned long long h[8] = {0};
    for (auto& w : s->ws) {
        unsigned long long t[8] = {0};
        if (w.stats.p) CLB_HIP(hipMemcpy(t, w.stats.p, sizeof t, hipMemcpyDeviceToHost));
        for (int i = 0; i < 8; ++i) h[i] += t[i];
    }
    if (cand_docs) *cand_docs = (int64_t)h[0];
    if (cand_embs) *cand_embs = (int64_t)h[1];
    if (rescored_docs) *rescored_docs = (int64_t)h[2];
    if (rescored_embs) *rescored_embs = (int64_t)h[3];
    return CLB_OK;
}

int clb_last_batch_half_rows(clb_searcher* s, int64_t* rows_lo, int64_t* rows_hi) {
    if (!s) return fail(CLB_EARGUMENT, "null searcher");
    CLB_TRY(use_device(s->device));
    CLB_HIP(hipDeviceSynchronize());
    unsigned long long h[2] = {0, 0};
    for (auto& w : s->ws) {
        unsigned long long t[8] = {0};
        if (w.stats.p) CLB_HIP(hipMemcpy(t, w.stats.p, sizeof t, hipMemcpyDeviceToHost));
        h[0] += t[4];
        h[1] += t[5];
    }
    if (rows_lo) *rows_lo = (int64_t)h[0];
    if (rows_hi) *rows_hi = (int64_t)h[1];
    return CLB_OK;
}

}  // extern "C"
