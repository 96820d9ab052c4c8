/*
 * colbert_hip.h -- C ABI of libcolbert_hip.so, the MI355X (gfx950) implementation of ColBERT.jl's
 * hot path: candidate generation + fused decompress/MaxSim + top-k (src/search, src/searching.jl),
 * the residual codec and index-build kernels (src/indexing, src/utils.jl) and the encoder epilogue
 * (src/modelling/embedding_utils.jl).
 *
 * The reference (pure Julia) has no FFI of its own; each entry point below replaces the Julia call
 * site cited next to it, and `julia/ColBERT/src/ColBERT.jl` + INTEGRATION.md show the `ccall`
 * binding a maintainer adds.  Conventions are the reference's:
 *   - matrices are column-major and densely packed (a Julia Array's memory, passed as Ptr{T});
 *   - centroid codes, pids and embedding ids are 1-based; Int is int64_t;
 *   - element types: float (Float32), uint32_t codes, uint8_t packed residuals, int64_t doclens/pids/ivf.
 * Ownership: the caller owns every host buffer; the library copies in/out before returning and never
 * retains a host pointer.  All device memory belongs to the library (handles are opaque).
 * Threading: every call is synchronous (results are in the output buffers on return) except the
 * *_device entry points, which enqueue on the given HIP stream.  One handle, one thread at a time.
 * clb_searcher_append / clb_searcher_append_device / clb_searcher_remove / clb_searcher_update / clb_searcher_update_device
 * replace the handle's device arrays: they wait for the whole device on entry and before the swap, and the caller must have no search of that handle in flight on another thread.
 * Errors: every function returns 0 or a CLB_E* code; codes 1..4 map 1:1 onto the Julia exception the
 * reference throws in the same situation.  clb_last_error() returns a message for the calling thread.
 * There is NO CPU fallback: without a GPU every compute entry point fails with CLB_EHIP.
 */
#ifndef COLBERT_HIP_H
#define COLBERT_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CLB_OK 0
#define CLB_EDIMENSION 1   /* DimensionMismatch */
#define CLB_EDOMAIN 2      /* DomainError */
#define CLB_EBOUNDS 3      /* BoundsError */
#define CLB_EARGUMENT 4    /* ArgumentError */
#define CLB_EHIP 10        /* HIP runtime failure / no device */
#define CLB_EUNSUPPORTED 11/* valid for the reference, not implemented by the HIP path */
#define CLB_ENOMEM 12

typedef struct clb_searcher clb_searcher;

const char* clb_version(void);
const char* clb_last_error(void);
/* number of visible HIP devices (0 without a GPU); never initialises a device */
int clb_device_count(void);
/* The copy rate of `device` right now: `reps` device-to-device copies of `bytes` between two HIP events, by three forms of a
 * 16-bytes-per-lane kernel and by hipMemcpyAsync; *gb_per_s = (bytes read + bytes written) / time of the fastest.  Measurement support for the roofline record of bench.py
 * ("HBM 8.0 TB/s spec, 6.29 TB/s measured copy; re-measure on the box"); no counterpart in the reference. */
int clb_measure_copy_rate(int device, int64_t bytes, int reps, double* gb_per_s);
/* ... and of a kernel that only READS `bytes` (16 bytes per lane, four pieces in flight): *gb_per_s = bytes / time.  Pass 1 of
 * the search is all reads; bench.py quotes its measured HBM traffic per second against this number. */
int clb_measure_read_rate(int device, int64_t bytes, int reps, double* gb_per_s);

/* ------------------------------------------------------------------------------------------------
 * Searcher: the resident index  (struct Searcher, src/searching.jl:1-16; Searcher(index_path) :18-80,
 * _build_emb2pid :82-91).  The arrays are the fields the reference keeps on the host; here they are
 * uploaded once into HBM.  `pid_offset` is added to every returned pid (0 for an unsharded index;
 * for a passage shard, the number of passages in the shards before it).
 * ---------------------------------------------------------------------------------------------- */
int clb_searcher_create(int device, int64_t dim, int nbits, int64_t K,
                        const float* centroids /* (dim,K) */, const float* bucket_weights /* 2^nbits */,
                        int64_t n_docs, const int64_t* doclens, int64_t n_emb,
                        const uint32_t* codes /* n_emb, 1-based */,
                        const uint8_t* residuals /* (dim/8*nbits, n_emb) */,
                        const int64_t* ivf /* n_emb, 1-based embedding ids */,
                        const int64_t* ivf_lengths /* K */, int64_t pid_offset,
                        clb_searcher** out);
/* The same Searcher from an index that is already in HBM (built there by clb_codec_compress_device /
 * clb_build_ivf_device: Searcher(index_path) loads exactly these arrays, src/searching.jl:41-59): d_centroids, d_codes,
 * d_residuals and d_ivf are device pointers on `device`, copied into the handle (the caller may free them on return);
 * bucket_weights, doclens and ivf_lengths are host arrays as above. */
int clb_searcher_create_device(int device, int64_t dim, int nbits, int64_t K, const float* d_centroids,
                               const float* bucket_weights, int64_t n_docs, const int64_t* doclens, int64_t n_emb,
                               const uint32_t* d_codes, const uint8_t* d_residuals, const int64_t* d_ivf,
                               const int64_t* ivf_lengths, int64_t pid_offset, clb_searcher** out);
int clb_searcher_destroy(clb_searcher* s);
/* Append passages to the resident index (no counterpart in the reference, whose index is built once; upstream ColBERT's
 * IndexUpdater.add with a fixed codec).  The n_new passages come after the handle's last passage: they become local passages
 * n_docs+1 .. n_docs+n_new (returned pids: pid_offset + those).  codes: UInt32[n_new_emb], 1-based; residuals:
 * (dim/8*nbits, n_new_emb); doclens: Int64[n_new] -- what compress() with the index's own centroids and cutoffs gives.
 * Afterwards every entry point behaves bit for bit as on a handle made by clb_searcher_create from the concatenated arrays
 * with ivf = stable sortperm(all codes) (_build_ivf, collection_indexer.jl:349-353): every new embedding id exceeds every old
 * one, so a centroid's merged list is its old list followed by its new entries in embedding order.  Bound constants that
 * were set or synced (clb_searcher_set_bound_consts) are never lowered: the handle keeps the element-wise maximum of the old
 * values and the grown index's own; sync a shard group again after an append.  What create derives from the index is derived
 * again -- pass 1's gather form returns to the choice by the grown index's code statistics (clb_searcher_set_pass1_gather
 * to force one again); the mode and the other settings of the handle are kept.
 * Failure leaves the handle unchanged and searchable: CLB_EDIMENSION sum(doclens) != n_new_emb; CLB_EARGUMENT a negative
 * doclen or a null pointer; CLB_EDOMAIN a code outside 1..K (checked on the device, as create does); CLB_EUNSUPPORTED the
 * totals exceed create's 2^32-1 embeddings / 2^31-1 passages; CLB_ENOMEM.  n_new = 0 is CLB_OK and changes nothing.
 * Memory: the grown arrays are built beside the old ones and swapped in at the end, so the call transiently holds about
 * the old index plus the new index (and the sort scratch of the new rows).
 * Threading: the call waits for the whole device on entry and again before the swap; the caller must have no search of
 * this handle in flight on another thread.  All four workspace slots are sized again by the next search, a pending
 * clb_search_shard_phase1 is dropped, a HIP graph captured over this handle holds freed addresses and must be captured again
 * (compare clb_searcher_generation), and a clb_filter made before the append is refused (CLB_EARGUMENT): make another. */
int clb_searcher_append(clb_searcher* s, int64_t n_new, const int64_t* doclens, int64_t n_new_emb, const uint32_t* codes,
                        const uint8_t* residuals);
/* The same with d_codes / d_residuals on the searcher's device (what clb_codec_compress_device wrote; neither is written);
 * doclens on the host.  hip_stream names the stream that produced them: its work, like all work of the device, is waited
 * for on entry, and the call returns with the append complete. */
int clb_searcher_append_device(clb_searcher* s, int64_t n_new, const int64_t* doclens, int64_t n_new_emb,
                               const uint32_t* d_codes, const uint8_t* d_residuals, void* hip_stream);
/* Remove passages from the resident index (no counterpart in the reference; upstream ColBERT's IndexUpdater.remove).  pids
 * are as search returns them: 1-based with pid_offset added, n entries in any order, duplicates allowed.  Pids are stable: a
 * removed passage stays in the numbering as an EMPTY passage (doclen 0, as create accepts one); n_docs, pid_offset and every
 * other passage's pid are unchanged, and a later append numbers its passages from n_docs + 1 as before.  Naming a passage
 * that is empty already is no error and does nothing for that pid.  *n_removed (may be null) receives the number of passages
 * that lost at least one embedding in this call.
 * Afterwards every entry point behaves bit for bit as on a handle made by clb_searcher_create from the reduced index: the same
 * centroids and weights, doclens with the removed entries set to 0, codes / residuals with those passages' columns deleted,
 * ivf = stable sortperm(reduced codes) (_build_ivf, collection_indexer.jl:349-353) -- a centroid's list is its old list
 * without the removed passages' entries, in the old order.  Bound constants that were set or synced
 * (clb_searcher_set_bound_consts) are never lowered; otherwise they are the reduced index's own.  What create derives from
 * the index is derived again (pass 1's gather form returns to the choice by the code statistics); the mode and the other
 * settings of the handle are kept.
 * n = 0, or *n_removed = 0, is CLB_OK, changes nothing and does not bump the generation.
 * Failure leaves the handle unchanged and searchable: CLB_EBOUNDS a pid outside pid_offset+1 .. pid_offset+n_docs (checked on
 * the host before any device work); CLB_EARGUMENT a null handle, null pids with n > 0, or n < 0; CLB_ENOMEM.
 * Memory, threading and invalidation are append's: the reduced arrays are built beside the old ones (the call transiently
 * holds the old plus the reduced index and two words of scan scratch per old embedding); the call waits for the whole device
 * on entry and again before the swap; all four workspace slots are sized again by the next search, a pending
 * clb_search_shard_phase1 is dropped, and a HIP graph captured over this handle must be captured again (compare
 * clb_searcher_generation).  A clb_filter made before the removal STAYS valid: n_docs, and so its bitmap, did not change. */
int clb_searcher_remove(clb_searcher* s, const int64_t* pids, int64_t n, int64_t* n_removed);
/* Replace the content of passages of the resident index in place, keeping their pids (no counterpart in the reference, nor in
 * upstream ColBERT's IndexUpdater, which has remove and add only).  pids are as search returns them (1-based with pid_offset
 * added), n entries in any order, each pid at most once.  Passage pids[i] loses all its rows and receives doclens[i] new ones:
 * the columns sum(doclens[:i]) .. sum(doclens[:i+1]) - 1 of codes (UInt32[n_new_emb], 1-based) / residuals ((dim/8*nbits,
 * n_new_emb)), in append's layouts -- what compress() with the index's own centroids and cutoffs gives.  doclens[i] == 0
 * empties the passage exactly as clb_searcher_remove does; a passage that is empty now (doclen 0 at create, or removed
 * earlier) may be named and is filled again.  n_docs, pid_offset and every other passage's pid are unchanged.  *n_changed
 * (may be null) receives the number of named passages whose old or new length is not zero.
 * Afterwards every entry point behaves bit for bit as on a handle made by clb_searcher_create from the index with those
 * passages' columns replaced, their doclens set, and ivf = stable sortperm(codes) (_build_ivf, collection_indexer.jl:349-353):
 * a passage is wholly kept or wholly replaced, so a centroid's list is the merge by passage of its kept entries and the new
 * entries with that code.  On a handle created with lists in an order of the caller's own (not ascending embedding ids) the
 * new entries go behind the kept ones of their list; results do not depend on the order inside a list.  Bound constants, the
 * gather form, the mode and the other settings follow append's and remove's rules.
 * n = 0, or *n_changed = 0, is CLB_OK, changes nothing and does not bump the generation.
 * Failure leaves the handle unchanged and searchable; all of these are decided before the changed index is allocated:
 * CLB_EARGUMENT a null handle, a null array with a non-zero count, n < 0, a negative doclen, or a pid named twice (two
 * contents for one passage: the message names the pid); CLB_EBOUNDS a pid outside pid_offset+1 .. pid_offset+n_docs;
 * CLB_EDIMENSION sum(doclens) != n_new_emb; CLB_EDOMAIN a code outside 1..K (checked on the device); CLB_EUNSUPPORTED the new
 * totals exceed create's limits; CLB_ENOMEM.
 * Memory, threading and invalidation are append's and remove's: the changed arrays are built beside the old ones (the call
 * transiently holds the old plus the new index, two words of scan scratch per old embedding and the staged new rows with
 * their sort scratch); the call waits for the whole device on entry and again before the swap; all four workspace slots are
 * sized again by the next search, a pending clb_search_shard_phase1 is dropped, and a HIP graph captured over this handle must
 * be captured again (compare clb_searcher_generation).  A clb_filter made before the update STAYS valid: n_docs did not
 * change. */
int clb_searcher_update(clb_searcher* s, int64_t n, const int64_t* pids, const int64_t* doclens, int64_t n_new_emb,
                        const uint32_t* codes, const uint8_t* residuals, int64_t* n_changed);
/* The same with d_codes / d_residuals on the searcher's device (neither is written); pids and doclens on the host.
 * hip_stream as in clb_searcher_append_device. */
int clb_searcher_update_device(clb_searcher* s, int64_t n, const int64_t* pids, const int64_t* doclens, int64_t n_new_emb,
                               const uint32_t* d_codes, const uint8_t* d_residuals, void* hip_stream, int64_t* n_changed);
/* Number of appends, removals and updates that changed the handle (0 after create), its passages and its embeddings.  These return
 * counts, not CLB_* codes: a null handle gives -CLB_EARGUMENT (and the message in clb_last_error). */
int64_t clb_searcher_generation(const clb_searcher* s);
int64_t clb_searcher_num_docs(const clb_searcher* s);
int64_t clb_searcher_num_embeddings(const clb_searcher* s);
/* bytes of HBM held by the handle (index + workspace) */
int64_t clb_searcher_device_bytes(const clb_searcher* s);

/* search(searcher, query, k) after the encoder  (src/searching.jl:102-127):
 * retrieve -> gather -> decompress -> maxsim -> stable sortperm(rev=true) -> first k.
 * Q is (dim, T) for one query.  out_pids/out_scores have k entries.  Fewer than k candidates is the
 * reference's BoundsError (searching.jl:127) -> CLB_EBOUNDS.  *n_cand receives the candidate count. */
int clb_search(clb_searcher* s, const float* Q, int64_t T, int64_t nprobe, int64_t k,
               int64_t* out_pids, float* out_scores, int64_t* n_cand);
/* B queries at once: Q is (dim, T, B); out_pids/out_scores are (k, B); n_cand has B entries.
 * pad_short != 0: a query with fewer than k candidates is not an error; its tail is filled with
 * pid 0 and score -Inf (what a passage shard needs before the cross-shard merge). */
int clb_search_batch(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                     int pad_short, int64_t* out_pids, float* out_scores, int64_t* n_cand);
/* Same, device-resident: every pointer is a device pointer on the searcher's device; the work is
 * enqueued in stream order on `hip_stream` (a hipStream_t; NULL = the HIP null stream) and not waited for:
 * work queued later on that stream sees the results.
 * Always pads short results (pid 0, -Inf).  Used by the multi-GPU driver and bench.py. */
int clb_search_batch_device(clb_searcher* s, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                            int64_t k, int64_t* d_out_pids, float* d_out_scores, int64_t* d_n_cand,
                            void* hip_stream);
/* The same with an explicit workspace slot (0..3): several batches can be in flight on streams of the caller, each
 * on its own per-batch scratch -- the latency-bound selection kernels of one batch then overlap the scoring kernels of
 * the other (bench.py).  Calls that use the same slot must be stream-ordered by the caller.  Every other entry point
 * uses slot 0. */
int clb_search_batch_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                 int64_t k, int64_t* d_out_pids, float* d_out_scores, int64_t* d_n_cand,
                                 void* hip_stream);
/* Sharded (multi-GPU) search in two calls, so that every shard cuts at the GLOBAL k-th approximate score instead
 * of its own (a shard must otherwise re-score ~k passages exactly however small it is).  Two-pass mode only
 * (CLB_EUNSUPPORTED otherwise: use clb_search_batch_device).
 *   phase 1: S1..pass 1 on this shard; d_local_top (B, k) = its k largest approximate scores per query (-Inf padded);
 *   the caller all-gathers these blocks over the shards: d_all_top = [n_shards][B][k];
 *   phase 2: selection at the k-th largest gathered score, exact pass, top-k -- outputs as clb_search_batch_device.
 * Phase 2 must follow phase 1 of the same batch on the same handle and stream.  With filters:
 * clb_search_shard_phase1_filtered_slot (below, "Filtered search"). */
int clb_search_shard_phase1(clb_searcher* s, const float* d_Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                            float* d_local_top, void* hip_stream);
int clb_search_shard_phase2(clb_searcher* s, const float* d_Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                            const float* d_all_top, int64_t n_shards, int64_t* d_out_pids, float* d_out_scores,
                            int64_t* d_n_cand, void* hip_stream);
/* The two phases on an explicit workspace slot (0..3), like clb_search_batch_device_slot: batches that are in flight on
 * different streams of the caller MUST use different slots -- phase 2 continues on the scratch phase 1 left in its slot. */
int clb_search_shard_phase1_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                 int64_t k, float* d_local_top, void* hip_stream);
int clb_search_shard_phase2_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                 int64_t k, const float* d_all_top, int64_t n_shards, int64_t* d_out_pids,
                                 float* d_out_scores, int64_t* d_n_cand, void* hip_stream);
/* 0: exact single pass (every candidate scored with the canonical fp32 arithmetic);
 * 1: two-pass (bf16-MFMA approximate pass with a proven error bound selects a superset of the top-k,
 *    which is then re-scored exactly) -- results are identical by construction.  Default 1 when the
 *    index shape supports it (dim 128, nbits 2), else 0. */
int clb_searcher_set_mode(clb_searcher* s, int mode);
int clb_searcher_get_mode(const clb_searcher* s);
/* Selection step of the two-pass mode (the k-th approximate score and the list it cuts; part of search(), no call site of
 * its own in the reference): one work-group per query, or -- "wide" -- 16 work-groups per query with one launch per radix
 * pass, for shards whose queries have far more candidates than one work-group holds in registers (10 M passages on one
 * GPU: ~96 k per query).  on = -1: chosen by the handle's candidate capacity (default), 0: never, 1: always.  The
 * results are identical either way. */
int clb_searcher_set_wide_select(clb_searcher* s, int on);
/* Gather form of pass 1 of the two-pass mode (how the fp16 centroid-score rows of ranking.jl:27 reach the scorer; no call
 * site of its own in the reference): 0 = per-lane VGPR loads, 1 = LDS-DMA with four adjacent lanes per row, -1 = chosen at
 * load from the index's own code statistics (default).  Results are identical either way.  The getter returns the form
 * in use and, through *adjacency (may be null), the statistic: the fraction of consecutive embeddings whose score rows
 * share a 128-byte line. */
int clb_searcher_set_pass1_gather(clb_searcher* s, int form);
int clb_searcher_get_pass1_gather(const clb_searcher* s, double* adjacency);
/* Row format of the centroid-score table pass 1 gathers from, for batches of 16 or more queries in the two-pass mode (the
 * (32, K) cells matrix of ranking.jl:27-30; no call site of its own in the reference): form = 0, 64-byte rows of fp16 scores;
 * form = 1, 32-byte rows of 8-bit cells, linear per (query, token) over the range that token's K scores span (measured by the
 * centroid kernel; the fp16 table is requantised), with half a step in the error bound -- half the gathered bytes, pass 1
 * 12-20 % faster where the codes are not id-adjacent, but about twice the rows re-scored exactly: measured end to end it
 * loses on every workload of bench.py, so form = -1, the default, is 0.  Returned pids and scores are identical either
 * way; on the shards of a group set the form alike on all shards.  The getter returns the form batches of 16+ queries take. */
int clb_searcher_set_score_rows(clb_searcher* s, int form);
int clb_searcher_get_score_rows(const clb_searcher* s);
/* Products of the batched centroid stage (the Q x centroids GEMM of ranking.jl:9-13 for batches of 16 or more queries in
 * the two-pass mode; no call site of its own in the reference): n = 1, the fp16 score table of pass 1 is made from ONE fp16
 * product per fp32 product, with the measured conversion errors of both operands in the error bound; n = 3, from the
 * three-product bf16 split (every smaller batch always is); n = -1, the default: 1 on a shard of a group (a handle that
 * clb_searcher_set_bound_consts / clb_searcher_sync_bound_consts has been called on), 3 on a single GPU -- measured on the
 * 1 M-passage workload the single product takes 0.020 ms off the centroid kernel (0.104 -> 0.084) and its wider bound
 * (+12 % re-scored rows) puts 0.01-0.02 ms back on pass 2; on N shards the centroid stage is replicated and the extra rows
 * are divided by N.  n = 1 on an index with a centroid component outside the fp16 range stays at 3.  Results are
 * identical either way (the nprobe best centroids are re-scored in canonical fp32, the table only feeds the approximate pass,
 * whose bound carries the difference).  The getter returns the count in use for such batches and, through *max_f16_error
 * (may be null), max over the centroids of ||c - fp16(c)|| (0: out of range). */
int clb_searcher_set_centroid_products(clb_searcher* s, int n);
int clb_searcher_get_centroid_products(const clb_searcher* s, float* max_f16_error);
/* Constants of the two-pass error bound of this handle: consts[0] = max ||centroid||, [1] = sqrt(dim) * max |bucket
 * weight|, [2] = max over the shard's embeddings of 1/(||c + r|| + eps), [3] = max ||fp16-rounded residual vector||,
 * [4] = sqrt(dim) * max |w - fp16(w)|, [5] = the quantisation error of the packed inv_norm.  Sharded search with a global threshold (clb_search_shard_phase1/2) needs ONE
 * bound on every shard: take the element-wise maximum over the shards (an all-reduce MAX of six floats at load time)
 * and set it on each handle.  `set` never lowers a value. */
int clb_searcher_get_bound_consts(const clb_searcher* s, float* consts /* 6 */);
int clb_searcher_set_bound_consts(clb_searcher* s, const float* consts /* 6 */);

/* ------------------------------------------------------------------------------------------------
 * Filtered search: "search, but only among these passages" (no counterpart in the reference; upstream ColBERT's
 * search(..., filter_fn=...) and search(..., pids=...)).  A clb_filter is a passage set resident in HBM as one bitmap of
 * ceil(n_docs / 32) words -- bit i of word j = local passage 32 j + i, the layout of the candidate bitmap of retrieve()
 * (ranking.jl:32-43) -- which the marking / compaction kernels take as one more operand: tau, eps, the re-score list and the
 * top-k are then computed over the filtered candidates by the unchanged scoring kernels.  A filter is bound to the searcher
 * it was made for, is created once and reused over any number of calls (one per tenant, say), and is never written by a
 * search.  It MUST outlive every call that uses it, including calls still enqueued on a stream or captured in a graph;
 * it may be destroyed before or after its searcher.  Creation synchronises (the population count is read back once);
 * searching with it does not.  An append (n_docs changes) invalidates it; a removal does not: after clb_searcher_remove the
 * handle answers with it as a fresh handle on the reduced index answers with the same bitmap, in both scopes (a
 * passage without embeddings -- an empty passage of create, or one emptied by clb_searcher_remove -- holds nothing to score
 * and is never a candidate: CLB_FILTER_ALL ranks the set's passages that hold embeddings, n_cand counts those, while
 * clb_filter_count stays the population of the set).
 * ---------------------------------------------------------------------------------------------- */
typedef struct clb_filter clb_filter;
/* pids as search returns them: 1-based with the searcher's pid_offset added, n entries in any order, duplicates allowed;
 * a pid outside pid_offset+1 .. pid_offset+n_docs is CLB_EBOUNDS.  n = 0 is the empty filter.  The bitmap is built on the
 * device. */
int clb_filter_create_pids(clb_searcher* s, const int64_t* pids, int64_t n, clb_filter** out);
/* clb_filter_create_pids for a shard GROUP: `pids` is a GLOBAL list, handed unchanged to every shard of the group.  The pids
 * inside this shard's range pid_offset+1 .. pid_offset+n_docs set their bit; pids of other shards are skipped, not errors;
 * a pid < 1 is CLB_EBOUNDS (that the list stays inside the GROUP's passages is the caller's check: a shard does not know
 * its group).  *n_inside = the number of list entries that fell inside this shard, duplicates counted (clb_filter_count
 * stays the population).  Range test, marking and count are one pass over the list on the device.  n = 0, or a list wholly
 * outside the shard, gives a valid empty filter: under CLB_FILTER_ALL the shard then has no candidate. */
int clb_filter_create_pids_global(clb_searcher* s, const int64_t* pids, int64_t n, clb_filter** out, int64_t* n_inside);
/* the bitmap itself (host words): n_words must be ceil(n_docs / 32), else CLB_EARGUMENT; bits past n_docs are cleared. */
int clb_filter_create_bitmap(clb_searcher* s, const uint32_t* words, int64_t n_words, clb_filter** out);
/* number of passages in the set (a host value, fixed at creation); 0 for a null handle */
int64_t clb_filter_count(const clb_filter* f);
/* a null handle is CLB_OK, like clb_searcher_destroy */
int clb_filter_destroy(clb_filter* f);
/* scope of a filtered search:
 *   CLB_FILTER_CANDIDATES  candidates = retrieve(Q) INTERSECT filter (upstream's filter_fn): S1-S3 run as ever and the filter
 *                          word is AND-ed in where the candidate bitmap is counted and written out;
 *   CLB_FILTER_ALL         candidates = the filter's passages, whatever retrieve(Q) would give: a re-rank of a caller-chosen
 *                          list (upstream's pids=).  nprobe is validated and otherwise unused; the workspace grows to hold
 *                          the largest clb_filter_count of the batch per query (CLB_EUNSUPPORTED, naming the count, if it
 *                          cannot).  A query whose entry is NULL is an ordinary unfiltered query in either scope. */
enum { CLB_FILTER_CANDIDATES = 0, CLB_FILTER_ALL = 1 };
/* clb_search_batch with a filter per query: `filters` is a HOST array of B handles (a NULL entry: that query is not
 * filtered; a NULL array: none is), each made for `s` (CLB_EARGUMENT otherwise).  Short results are always padded with
 * pid 0 / -Inf -- a filter routinely leaves fewer than k passages, which is no error -- and n_cand[b] is the number of
 * candidates AFTER the filter.  A call in which no query is filtered launches exactly what clb_search_batch launches. */
int clb_search_batch_filtered(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                              const clb_filter* const* filters, int scope, int64_t* out_pids, float* out_scores,
                              int64_t* n_cand);
/* clb_search_batch_device_slot with a filter per query: `filters` is still a HOST array, read before the call returns (the
 * handles reach the kernels in their arguments: stream-ordered, no copy, capturable in a HIP graph -- the captured graph
 * holds the filters' device addresses, so they must live as long as it is replayed). */
int clb_search_batch_filtered_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                          int64_t k, const clb_filter* const* filters, int scope, int64_t* d_out_pids,
                                          float* d_out_scores, int64_t* d_n_cand, void* hip_stream);
/* clb_search_shard_phase1_slot with the `filters` / `scope` operands of clb_search_batch_filtered_device_slot: the filtered
 * search across the shards of a group.  Each shard's filters are its OWN (clb_filter_create_pids_global cuts one global pid
 * list per shard); they act where phase 1 makes the shard's candidate list, so d_local_top holds approximate scores of
 * filtered candidates only, and clb_search_shard_phase2(_slot) -- its signature unchanged, and with no filter operand: it
 * continues on the candidate list phase 1 left on the slot, and the two-pass proof holds for whatever candidate set it is
 * given -- returns the filtered result, d_n_cand the counts AFTER the filter.  The same argument checks as both calls it
 * extends (a bad scope, a filter of another searcher or from before an append: CLB_EARGUMENT).  filters == NULL, or no
 * non-NULL entry, launches exactly what clb_search_shard_phase1_slot launches (which IS this call with filters == NULL).
 * The phase calls keep the whole batch on one slot, and a launch carries at most 64 filter handles: a call in which some
 * query is filtered takes B <= 64 queries, CLB_EUNSUPPORTED (naming the limit) beyond -- split the batch, one phase-1 /
 * phase-2 pair per piece (ShardedSearcher does). */
int clb_search_shard_phase1_filtered_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                          int64_t k, const clb_filter* const* filters, int scope, float* d_local_top,
                                          void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Composing filters on the device: a request carries several predicates at once ("this tenant's passages, published after
 * day D, not in the hidden set"), and the operands -- other filters, a per-passage attribute held as a clb_prior -- are
 * resident already.  Each call below makes a NEW immutable clb_filter bound to `s`, with the lifetime rules of every other
 * filter; every search call, scope, route, captured graph and shard protocol takes it as it takes any other.  Operands are
 * only read: they may be in use by searches in flight, may be destroyed as soon as the call returns, and the same operand may
 * be named more than once.  Creation synchronises once, for the count (so it is not capturable); *out is NULL on every
 * failure; all argument checks run before any device work, and those that need nothing of the searcher's state (a null s /
 * out / operands / entry, an op outside the enum, the rules for n, a NaN bound, unknown flag bits, a fill outside 0 / 1) are
 * answered on a machine without a GPU.
 * ---------------------------------------------------------------------------------------------- */
/* the set operations: AND the intersection of all operands, OR their union, ANDNOT operand 0 minus the union of the rest,
 * NOT the complement of the single operand within the searcher's passages */
enum { CLB_FILTER_OP_AND = 0, CLB_FILTER_OP_OR = 1, CLB_FILTER_OP_ANDNOT = 2, CLB_FILTER_OP_NOT = 3 };
/* the most operands of one clb_filter_combine call: their word pointers travel in the kernel's arguments */
enum { CLB_MAX_FILTER_OPERANDS = 16 };
/* `operands`: a HOST array of n handles, 1 <= n <= CLB_MAX_FILTER_OPERANDS, and n == 1 exactly for CLB_FILTER_OP_NOT
 * (anything else: CLB_EARGUMENT).  AND, OR and ANDNOT with n = 1 give a copy.  An operand made for another searcher, or made
 * before an append, is CLB_EARGUMENT naming its index ("the filter of operand 2: filter made before an append; make
 * another").  A searcher without passages gives a valid empty filter without a launch. */
int clb_filter_combine(clb_searcher* s, int op, const clb_filter* const* operands, int64_t n, clb_filter** out);
/* flags of clb_filter_create_range: the bound itself is outside the range */
enum { CLB_RANGE_LO_OPEN = 1, CLB_RANGE_HI_OPEN = 2 };
/* The passages whose value in `values` lies between lo and hi: passage p is in when
 *     (flags & CLB_RANGE_LO_OPEN ? v > lo : v >= lo) && (flags & CLB_RANGE_HI_OPEN ? v < hi : v <= hi)
 * for the stored fp32 value v, by IEEE comparison (-0 equals +0).  The attribute is a clb_prior: recency, quality, a tenant
 * id.  Values are fp32, so integers are exact up to 2^24: an id or a day number beyond that does not survive
 * clb_prior_create.  The prior must be this searcher's and made for the passages it holds now (CLB_EARGUMENT otherwise: "the
 * prior was made for another searcher", "prior made before an append; make another").  A NaN bound and flag bits outside the
 * two are CLB_EARGUMENT.  -Inf / +Inf as a bound is an open end (a prior's values are always finite).  lo > hi, or lo == hi
 * with an open end, is a valid empty filter; lo == hi with both ends closed is equality, and membership in a few values is
 * the CLB_FILTER_OP_OR of such filters.  (struct clb_prior: the clb_prior of "Score priors" below.) */
int clb_filter_create_range(clb_searcher* s, const struct clb_prior* values, float lo, float hi, int flags, clb_filter** out);
/* A filter made before an append, carried over it: `f` must be a filter of `s` with no more passages than `s` holds now
 * (CLB_EARGUMENT otherwise).  The result has the searcher's current n_docs: the passages `f` knew keep their bit, the passages
 * appended since are all out (fill = 0) or all in (fill = 1; anything else: CLB_EARGUMENT).  With equal n_docs it is a copy.
 * `f` itself is unchanged and, if stale, stays refused by every search. */
int clb_filter_extend(clb_searcher* s, const clb_filter* f, int fill, clb_filter** out);
/* The words of a filter, copied to the host after waiting for the device work that made them: n_words must be the filter's
 * ceil(n_docs / 32), else CLB_EARGUMENT; bits past n_docs are zero.  It works on any filter, stale ones and those whose
 * searcher is gone included. */
int clb_filter_bitmap(const clb_filter* f, uint32_t* words, int64_t n_words);

/* ------------------------------------------------------------------------------------------------
 * Grouped search: rank DOCUMENTS by their best passage (no counterpart in the reference; the "collapse" of Elasticsearch and
 * Vespa, the docs2passages evaluation of upstream ColBERT).  A clb_grouping maps every local passage to a group.  The
 * caller's group_ids -- exactly n_docs entries, entry i = local passage i -- must be NON-DECREASING in pid, so that equal
 * ids are one contiguous pid range (anything else is CLB_EARGUMENT, naming the first passage at which the ids decrease;
 * the check runs on the host before anything is allocated; groups that are not contiguous are not supported).  Resident
 * form: one u32 per passage, the dense 0-based index of its group (4 MB per million passages), computed on the device.
 *
 * A grouped search of a query returns k GROUPS, each by its representative passage and that passage's fp32 score: the
 * candidate passage of the group with the largest exact MaxSim score, the lowest pid among equal scores; groups ordered by
 * score descending, the lower representative pid first among equal scores.  That is the reference's full stable ranking of
 * the query's candidates with the first occurrence of every group kept and then the first k taken -- pids and score bits are
 * identical to that.  n_cand is the number of distinct groups among the query's candidates (after any filter); fewer than
 * k of them is a short result.  Filters compose in both scopes: the filter defines the candidates, the grouping acts on what
 * is left.  A passage without embeddings is never a candidate, so a group of only such passages never appears.
 *
 * Like a filter, a grouping is immutable, bound to the searcher it was made for and to its n_docs: it stays valid over
 * clb_searcher_remove and clb_searcher_update, one made before an append is refused ("grouping made before an append; make
 * another"), one made for another searcher is refused (both CLB_EARGUMENT).  It MUST outlive every call that uses it,
 * including calls still enqueued on a stream or captured in a graph; it may be destroyed before or after its searcher.
 * Creation synchronises; searching with it does not.  A call takes ONE grouping for the whole batch.  Across the shards of
 * a group: "Grouped search across a shard group" below.
 * ---------------------------------------------------------------------------------------------- */
typedef struct clb_grouping clb_grouping;
int clb_grouping_create(clb_searcher* s, const int64_t* group_ids, int64_t n, clb_grouping** out);
/* number of groups (a host value, fixed at creation); 0 for a null handle */
int64_t clb_grouping_count(const clb_grouping* g);
/* a null handle is CLB_OK, like clb_filter_destroy */
int clb_grouping_destroy(clb_grouping* g);
/* clb_search_batch_filtered with a grouping: `filters` / `scope` as there (filters == NULL: nothing is filtered), pad_short
 * as in clb_search_batch (0: a query with fewer than k candidate groups is CLB_EBOUNDS; 1: pid 0 / -Inf padding).
 * grouping == NULL launches exactly what clb_search_batch_filtered launches. */
int clb_search_batch_grouped(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                             const clb_filter* const* filters, int scope, const clb_grouping* grouping, int pad_short,
                             int64_t* out_pids, float* out_scores, int64_t* n_cand);
/* clb_search_batch_filtered_device_slot with a grouping: stream-ordered, no host synchronisation; after the slot's first
 * grouped call it allocates nothing (the first one grows the slot by two slot lists of its candidate capacity per query).
 * Capturable in a HIP graph under the rule of the filtered search: the graph holds the grouping's device address, and a
 * call that grows the workspace makes a captured graph stale.  grouping == NULL launches exactly what
 * clb_search_batch_filtered_device_slot launches. */
int clb_search_batch_grouped_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const clb_filter* const* filters, int scope, const clb_grouping* grouping,
                                         int64_t* d_out_pids, float* d_out_scores, int64_t* d_n_cand, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Hits of a grouped search: each of the k groups by its best `per_group` candidate passages (the inner_hits of an
 * Elasticsearch collapse), 1 <= per_group <= CLB_MAX_PER_GROUP.  The groups, their order, n_cand and the short-result
 * behaviour are those of the grouped search; the outputs hold B * k * per_group entries, [b][j][0 .. per_group) being the
 * passages of query b's j-th group: score descending, the lower pid first among equal scores, padded with pid 0 / -Inf when
 * the group has fewer candidate passages (never an error); a padded group (short result) is all padding.  That is the
 * reference's full stable ranking of the query's candidates (after any filter) with the first k distinct groups kept in
 * order of first occurrence and of each its first per_group occurrences -- pids and score bits are identical to that.
 * Entry 0 of a group is the representative the grouped search returns, bit for bit.  A passage of the group that is not a
 * candidate of the query does not appear (CLB_FILTER_ALL ranks all passages of a filter).
 * per_group == 1 launches exactly what the grouped call launches.  per_group outside 1..CLB_MAX_PER_GROUP or a null
 * grouping is CLB_EARGUMENT.  filters / scope / pad_short, the sub-batches of a large batch and the slot entry's rules
 * (stream-ordered, no host synchronisation, capturable; B <= 64 when a query is filtered) are those of the calls they
 * extend.  A slot's first call with hits grows it (in the two-pass mode by 16 bytes per query and candidate of its
 * capacity), as does a call with a larger per_group than the slot has seen; later calls allocate nothing.  The phase calls
 * of a shard group take no per_group.
 * ---------------------------------------------------------------------------------------------- */
enum { CLB_MAX_PER_GROUP = 16 };
int clb_search_batch_grouped_hits(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                                  const clb_filter* const* filters, int scope, const clb_grouping* grouping, int64_t per_group,
                                  int pad_short, int64_t* out_pids, float* out_scores, int64_t* n_cand);
int clb_search_batch_grouped_hits_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                              int64_t k, const clb_filter* const* filters, int scope,
                                              const clb_grouping* grouping, int64_t per_group, int64_t* d_out_pids,
                                              float* d_out_scores, int64_t* d_n_cand, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Score priors: rank by MaxSim plus a resident per-passage term (no counterpart in the reference; the rank_feature /
 * function_score of Elasticsearch, a first-phase expression over an attribute in Vespa): recency, popularity, a quality
 * score, a tenant's boost.  A clb_prior holds one FINITE fp32 value per local passage -- exactly n_docs entries, entry i =
 * local passage i (4 MB per million passages).  A non-finite value is CLB_EARGUMENT, naming the first offending passage;
 * creation records max |value| (clb_prior_max_abs).  clb_prior_create checks on the host before anything is allocated;
 * clb_prior_create_device takes the values from device memory (of the searcher's device) and checks them there, with one
 * read-back.
 *
 * A search call takes at most ONE prior and one finite fp32 `weight` for the whole batch.  For every candidate passage p of
 * a query (after any filter, in either scope), with e(p) the fp32 MaxSim score the call returns without a prior:
 *     pi(p) = fl32(weight * value[p])          one rounded multiply
 *     E(p)  = fl32(e(p) + pi(p))               one rounded add, never contracted into an fma
 * The result is the first k candidates ordered by E descending, the lower pid first among equal E, and the returned scores
 * are E, bit for bit.  n_cand, the padding of short results (pid 0 / -Inf) and pad_short behave as without a prior, and the
 * candidate set is unchanged: a prior never makes a passage a candidate.  With a grouping the representative of a group is
 * its candidate passage with the largest E (lower pid first) and the groups are ordered by that value.  In the two-pass
 * mode the cut moves with the prior: a passage that only the prior lifts into the top k is re-scored.
 * A weight that is not finite, or with |weight| * max|value| not below FLT_MAX, is CLB_EARGUMENT (pi is always finite).
 *
 * Like a grouping, a prior is immutable, bound to the searcher it was made for and to its n_docs: it stays valid over
 * clb_searcher_remove and clb_searcher_update, one made before an append is refused ("prior made before an append; make
 * another"), one made for another searcher is refused (both CLB_EARGUMENT).  It MUST outlive every call that uses it,
 * including calls still enqueued on a stream or captured in a graph; it may be destroyed before or after its searcher.
 * Creation synchronises; searching with it does not.  The hits of a grouped search (clb_search_batch_grouped_hits*) take no
 * prior -- their extended list is built from approximate MaxSim scores; the Python driver answers `per_group` together with a
 * prior with Unsupported, naming both.
 * Entry points that take a prior: clb_search_batch_prior, clb_search_batch_prior_device_slot and, for a shard group, the two
 * phase calls clb_search_shard_phase1_prior_slot / clb_search_shard_phase2_prior_slot ("Score priors across a shard group"
 * below); the other phase calls take none.
 * ---------------------------------------------------------------------------------------------- */
typedef struct clb_prior clb_prior;
int clb_prior_create(clb_searcher* s, const float* values, int64_t n, clb_prior** out);
int clb_prior_create_device(clb_searcher* s, const float* d_values, int64_t n, clb_prior** out);
/* max |value| (a host value, fixed at creation); 0 for a null handle */
float clb_prior_max_abs(const clb_prior* p);
/* a null handle is CLB_OK, like clb_filter_destroy */
int clb_prior_destroy(clb_prior* p);
/* clb_search_batch_grouped with a prior: `filters` / `scope` / `grouping` / `pad_short` as there (NULL: none).
 * prior == NULL launches exactly what clb_search_batch_grouped launches (weight is then ignored). */
int clb_search_batch_prior(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                           const clb_filter* const* filters, int scope, const clb_grouping* grouping, const clb_prior* prior,
                           float weight, int pad_short, int64_t* out_pids, float* out_scores, int64_t* n_cand);
/* clb_search_batch_grouped_device_slot with a prior: stream-ordered, no host synchronisation; after the slot's first call
 * with a prior it allocates nothing (the first one grows the slot by two floats per query: the boosted threshold and the
 * largest boosted score).  Capturable in a HIP graph under the rule of the filtered search: the graph holds the prior's
 * device address and the weight, and a call that grows the workspace makes a captured graph stale.  prior == NULL launches
 * exactly what clb_search_batch_grouped_device_slot launches. */
int clb_search_batch_prior_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                       int64_t k, const clb_filter* const* filters, int scope, const clb_grouping* grouping,
                                       const clb_prior* prior, float weight, int64_t* d_out_pids, float* d_out_scores,
                                       int64_t* d_n_cand, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Search after a cursor: the next k results past a (score, pid), exactly (no counterpart in the reference; the search_after
 * of Elasticsearch, a continuation token in Vespa).  A cursor is one pair (s*, p*) per query: s* an fp32 score, p* a GLOBAL
 * 1-based pid (int64).  It need not be a result that was ever returned.  For a query whose candidates (after any filter, in
 * either scope) have the exact fp32 MaxSim scores e(p),
 *     after(p)  <=>  e(p) < s*   or   (e(p) == s* and pid(p) > p*)
 * and the call returns the first k members of {p : after(p)} by (e descending, pid ascending), with their pids and fp32
 * score bits: what the ranking of the call without a cursor continues with.
 *   - Paging with the cursor (scores[k-1], pids[k-1]) of the previous page yields the ranking of all candidates cut into
 *     pieces of k, bit for bit, runs of exactly equal scores that cross a page boundary included.
 *   - s* = +Inf is "no cursor" for that query (p* is ignored): its result is that of the call without cursors, bit for bit.
 *     A batch may mix queries with and without a cursor.
 *   - s* = -Inf gives an empty page.  A NaN s* is CLB_EARGUMENT on the host entry point; on the device entry point, where
 *     nothing can be raised, it gives an empty page.
 *   - A page is always padded: entries past the last member are pid 0 / -Inf, and a short page is never CLB_EBOUNDS (the
 *     last page is short by nature; a page of padding alone is the end marker).
 *   - n_cand is what the call without cursors reports, the candidates after the filter, the same on every page.  The number
 *     of candidates after the cursor is not reported: the two-pass mode does not know it.
 *   - A cursor never changes the candidate set.
 * In the two-pass mode the cut moves with the cursor: what is re-scored is the page and the
 * candidates whose approximate score lies within three error bounds of its ends, whatever came before it -- a candidate that is
 * certainly before the cursor is not re-scored.  Every k is served, above 16 384 by the full sort.
 * Cursors compose with `filters` in both scopes.  They are not offered with a grouping, with hits or with a prior -- these
 * entry points have no such parameters; the Python driver answers the combinations with Unsupported, naming both keywords --
 * nor by the phase calls of a shard group.
 *
 * after_scores / after_pids: [B] each.  Both NULL: exactly clb_search_batch_filtered (its launches, its results); one NULL
 * and one not is CLB_EARGUMENT.  The arguments -- a NULL handle or output, the pair, NaN -- are checked before any device
 * work; the limits of the filtered calls apply (sub-batches of 64 queries).
 * ---------------------------------------------------------------------------------------------- */
int clb_search_batch_after(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                           const clb_filter* const* filters, int scope, const float* after_scores /* [B], host */,
                           const int64_t* after_pids /* [B], host */, int64_t* out_pids, float* out_scores, int64_t* n_cand);
/* clb_search_batch_filtered_device_slot with cursors in DEVICE memory (of the searcher's device): stream-ordered, no host
 * synchronisation; after the slot's first call with cursors it allocates nothing (the first one grows the slot by 4 bytes
 * per query and candidate of its capacity: the list of the slots after the cursor).  Capturable in a HIP graph under the
 * rule of the filtered search; the graph holds the ADDRESSES of the cursor arrays, not their values -- paging under a graph
 * is: copy the last row of the outputs into the cursor arrays, replay.  Both arrays NULL launches exactly what
 * clb_search_batch_filtered_device_slot launches. */
int clb_search_batch_after_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                       int64_t k, const clb_filter* const* filters, int scope, const float* d_after_scores,
                                       const int64_t* d_after_pids, int64_t* d_out_pids, float* d_out_scores,
                                       int64_t* d_n_cand, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Grouped search across a shard group. Every shard holds a clb_grouping made from ITS slice of the group ids (a dense
 * local index per local passage, as ever) and the caller passes `group_base`: the GLOBAL dense index of the group of the
 * shard's first passage, so that the global index of local passage p is group_base + index[p].  (The host has the whole id
 * array: the global dense index of passage i is the number of id changes before it.)  A group that straddles a cut is the
 * last group of one shard and the first of the next, and its index is the same on both: that is how the three steps below
 * recognise it.  Global group indices travel as int64, -1 is "none".
 *
 *   phase 1: clb_search_shard_phase1_filtered_slot, then the best approximate score of every candidate group; d_local_top /
 *            d_local_gid (B, k) = up to k groups per query with the largest such scores and their global indices, in no
 *            order, padded with -Inf / -1.  The caller all-gathers both: d_all_top / d_all_gid = [n_shards][B][k];
 *   phase 2: tau = the k-th largest score over the DISTINCT indices of the gathered records (a repeated index counts once,
 *            with its largest score; -Inf when fewer than k exist), the selection at tau, the row sweep, the exact pass,
 *            the best passage of every group among the re-scored, their top-k.  d_out_pids / d_out_scores (B, k) as
 *            clb_search_batch_grouped_device_slot, d_out_gids (B, k) the global group index of every result (-1 for
 *            padding), d_n_cand[b] the shard's distinct candidate groups, d_edge_gids (B, 2) the global group index of the
 *            query's lowest-pid and highest-pid candidate (-1, -1 without candidates);
 *   merge:   clb_merge_topk_grouped_device over the gathered results (below).
 * Checks as the calls they extend: a grouping of another searcher or from before an append is CLB_EARGUMENT, a handle
 * outside the two-pass mode CLB_EUNSUPPORTED, a null output CLB_EARGUMENT, more than 64 queries with a filter
 * CLB_EUNSUPPORTED; phase 2 must follow the grouped phase 1 of the same batch, grouping and group_base; at most 256 shards.
 * grouping == NULL in phase 1 launches exactly what clb_search_shard_phase1_filtered_slot launches and leaves d_local_gid
 * untouched (phase 2 is then clb_search_shard_phase2_slot).  Stream-ordered, no host synchronisation; after a slot's first
 * grouped phase 1 nothing is allocated.
 * ---------------------------------------------------------------------------------------------- */
int clb_search_shard_phase1_grouped_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const clb_filter* const* filters, int scope, const clb_grouping* grouping,
                                         int64_t group_base, float* d_local_top, int64_t* d_local_gid, void* hip_stream);
int clb_search_shard_phase2_grouped_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const float* d_all_top, const int64_t* d_all_gid, int64_t n_shards,
                                         const clb_grouping* grouping, int64_t group_base, int64_t* d_out_pids,
                                         float* d_out_scores, int64_t* d_out_gids, int64_t* d_n_cand, int64_t* d_edge_gids,
                                         void* hip_stream);
/* The single exchange (every shard runs its whole grouped search, clb_search_batch_grouped_device_slot, in any mode): this
 * call, stream-ordered behind that search on the same slot and stream, gives the merge what the search does not return --
 * d_out_gids (B, k) from the result pids d_pids, and d_edge_gids (B, 2) from the candidate lists the search left on the
 * slot.  B <= 64 (one sub-batch: the slot holds the lists of the last one); anything else on the slot in between, another
 * grouping, B, k or stream is CLB_EARGUMENT. */
int clb_search_result_groups_slot(clb_searcher* s, int slot, const clb_grouping* grouping, int64_t group_base,
                                  const int64_t* d_pids, int64_t B, int64_t k, int64_t* d_out_gids, int64_t* d_edge_gids,
                                  void* hip_stream);
/* Test hook: the de-duplicated threshold of the grouped phase 2 alone, d_tau[b] from d_all_top / d_all_gid
 * [n_shards][B][k].  Input as phase 1 makes it: the indices of one list are distinct, and an index two lists share is the
 * lowest or the highest of each. */
int clb_debug_group_tau_device(const float* d_all_top, const int64_t* d_all_gid, int64_t n_shards, int64_t B, int64_t k,
                               float* d_tau, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Score priors across a shard group.  Every shard holds a clb_prior made from ITS slice of the values, and every shard gets
 * the same weight; the caller checks |weight| * max|value| against the largest clb_prior_max_abs of the group.  The result of
 * the two phases and the merge equals the unsharded clb_search_batch_prior: pids, fp32 score bits, counts.  Two-pass mode only.
 *
 *   phase 1: clb_search_shard_phase1_grouped_slot up to pass 1, then A = fl(a + fl(weight * value)) written over the slot's
 *            approximate scores for ALL candidates; with a grouping the groups collapse on A.  d_local_top (B, k) = the
 *            shard's k largest A per query (with a grouping: the best A of its k best groups, and d_local_gid their global
 *            indices), in no order, padded with -Inf / -1; d_local_mabs [B] = M_i, the largest |A| over the shard's
 *            candidates of the query (0 without candidates).  The caller all-gathers all three: d_all_top / d_all_gid =
 *            [n_shards][B][k], d_all_mabs = [n_shards][B];
 *   phase 2: tau = the k-th largest gathered A (with a grouping over the DISTINCT indices, as the grouped phase 2; -Inf with
 *            fewer than k), M = max_i M_i, delta = 4 * 2^-24 * (M + eps) with eps the query's error bound under the shared
 *            constants, and the selection cuts at tau - 2 delta - 2 eps (-Inf for an unsafe query or a non-finite M); then the
 *            row sweep, the exact pass, E = fl(e + pi) over the re-scored, with a grouping the collapse on E, the top-k.
 *            Outputs as the grouped phase 2; d_all_gid, d_out_gids and d_edge_gids are ignored (may be NULL) without a
 *            grouping.
 *   merge:   clb_merge_topk_packed_device, or with a grouping clb_merge_topk_grouped_packed_device: both order by (score
 *            descending, pid ascending), which is the order of E.
 * M must be the maximum over ALL shards: a shard that cut with its own M_i could lose a member of the top k that another
 * shard's large prior values pushed tau towards.
 * Everything else follows the grouped phase calls: slot rules, stream order, no host synchronisation, nothing allocated
 * after a slot's first such phase 1, capturable, at most 64 queries when one is filtered, at most 256 shards with a grouping,
 * CLB_EUNSUPPORTED outside the two-pass mode, the refusal of phase 2 before the bound constants are shared.  The prior is
 * checked as in clb_search_batch_prior (another searcher's, made before an append, the weight: CLB_EARGUMENT); a null
 * d_local_mabs / d_all_mabs or output is CLB_EARGUMENT.  Phase 2 must follow the prior phase 1 of the same batch, prior,
 * weight (bit for bit), grouping and group_base on that slot: anything else, the other phase-2 calls included, is
 * CLB_EARGUMENT.  prior == NULL in phase 1 launches exactly what clb_search_shard_phase1_grouped_slot launches and leaves
 * d_local_mabs untouched (phase 2 is then one of the calls without a prior); prior == NULL in phase 2 is CLB_EARGUMENT.
 * The single exchange needs nothing new: clb_search_batch_prior_device_slot on every shard, then with a grouping
 * clb_search_result_groups_slot, then the merge.
 * ---------------------------------------------------------------------------------------------- */
int clb_search_shard_phase1_prior_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                       int64_t k, const clb_filter* const* filters, int scope, const clb_grouping* grouping,
                                       int64_t group_base, const clb_prior* prior, float weight, float* d_local_top,
                                       int64_t* d_local_gid, float* d_local_mabs, void* hip_stream);
int clb_search_shard_phase2_prior_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                       int64_t k, const float* d_all_top, const int64_t* d_all_gid,
                                       const float* d_all_mabs /* [n_shards][B] */, int64_t n_shards,
                                       const clb_grouping* grouping, int64_t group_base, const clb_prior* prior, float weight,
                                       int64_t* d_out_pids, float* d_out_scores, int64_t* d_out_gids, int64_t* d_n_cand,
                                       int64_t* d_edge_gids, void* hip_stream);
/* Test hook: the threshold kernel of the prior phase 2 alone, d_tau_in[b] = tau - 2 delta from d_all_top / d_all_gid (may be
 * NULL: no grouping) / d_all_mabs and d_eps [B] in place of the queries' own error bounds. */
int clb_debug_prior_tau_device(const float* d_all_top, const int64_t* d_all_gid, const float* d_all_mabs, const float* d_eps,
                               int64_t n_shards, int64_t B, int64_t k, float* d_tau_in, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * The search request: everything a search call may carry besides its queries, sizes and outputs, as ONE struct.  Every named
 * search entry point above fills a request and makes one of the four calls below; a caller may do the same.  The rules of
 * the fields are those documented at the named entries; which fields combine, and which named entry fills which, is the
 * table of DESIGN section 5 ("The search request") and INTEGRATION.md.  All of them are checked in one place, and the checks
 * that need no searcher (struct_bytes, the per_group range, a finite weight, the cursor pair, the combinations) run before
 * the searcher is looked at.  Zero-initialise the struct, set struct_bytes, then the fields of the features in use:
 * everything left zero / NULL means "none".
 * Refused combinations, all CLB_EUNSUPPORTED: a prior with per_group > 1 (the hits are built from approximate MaxSim scores),
 * cursors with a grouping, cursors with a prior, candidate lists with filters, list priors with a prior, with per_group > 1 or
 * with cursors; on the phase routes also per_group > 1, cursors and candidate lists, and phase 2 takes no filters (it
 * continues on the candidates phase 1 left on the slot).
 * ---------------------------------------------------------------------------------------------- */
typedef struct clb_search_request {
    int64_t struct_bytes;                 /* sizeof this struct: anything else is CLB_EARGUMENT */
    const clb_filter* const* filters;     /* HOST array of B handles (a NULL entry: that query is unfiltered), or NULL */
    int scope;                            /* CLB_FILTER_CANDIDATES / CLB_FILTER_ALL */
    int pad_short;                        /* host route only (the device routes always pad): see clb_search_batch */
    const clb_grouping* grouping;         /* or NULL */
    int64_t per_group;                    /* 0: none; 1: the grouped search itself; 2..CLB_MAX_PER_GROUP: hits (needs grouping) */
    int64_t group_base;                   /* phase routes with a grouping: the global index of the shard's first group */
    const clb_prior* prior;               /* or NULL: without prior and list_prior, prior_weight is ignored */
    float prior_weight;                   /* the weight of prior or of list_prior: finite, or CLB_EARGUMENT */
    const float* list_prior;              /* or NULL.  List priors ("Re-rank given passages" below): [B][list_stride] values beside */
                                          /* list_pids, where the lists live; needs the lists, never together with prior */
    const float* after_scores;            /* cursors, [B] each, both or neither: HOST arrays on the host route (a NaN score */
    const int64_t* after_pids;            /* is CLB_EARGUMENT), DEVICE arrays on the device route */
    const int64_t* list_pids;             /* candidate lists ("Re-rank given passages" below), both or neither: [B][list_stride] */
    const int64_t* list_lens;             /* pids and [B] lengths; HOST arrays on the host route, DEVICE arrays on the device route */
    int64_t list_stride;                  /* L >= 1: entries per row of list_pids / list_prior / list_scores */
    float* list_scores;                   /* or NULL.  The one OUTPUT a request carries: [B][list_stride], where the lists live */
} clb_search_request;
/* The host route: clb_search_batch and every clb_search_batch_* entry without _device.  With per_group > 1 the outputs
 * hold B * k * per_group entries. */
int clb_search_batch_request(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                             const clb_search_request* req, int64_t* out_pids, float* out_scores, int64_t* n_cand);
/* The device route: every clb_search_batch_*_device_slot entry. */
int clb_search_batch_request_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const clb_search_request* req, int64_t* d_out_pids, float* d_out_scores,
                                         int64_t* d_n_cand, void* hip_stream);
/* The phase routes: every clb_search_shard_phase1_* / phase2_* entry.  The exchange buffers belong to the phase, not to the
 * request: d_local_gid / d_all_gid / d_out_gids / d_edge_gids are read or written only with a grouping, d_local_mabs /
 * d_all_mabs only with a prior (NULL otherwise).  Phase 2 must be given the grouping, group_base, prior and weight (bit for
 * bit) of the phase 1 it follows. */
int clb_search_shard_phase1_request_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const clb_search_request* req, float* d_local_top, int64_t* d_local_gid,
                                         float* d_local_mabs, void* hip_stream);
int clb_search_shard_phase2_request_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                         int64_t k, const clb_search_request* req, const float* d_all_top,
                                         const int64_t* d_all_gid, const float* d_all_mabs, int64_t n_shards, int64_t* d_out_pids,
                                         float* d_out_scores, int64_t* d_out_gids, int64_t* d_n_cand, int64_t* d_edge_gids,
                                         void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Re-rank given passages: the candidate set of every query is a pid list of the caller's -- first-stage results of another
 * retriever, labelled pairs, teacher scores -- with no handle to create or destroy.  A call carries lists for the whole
 * batch or for none.  Query b's list is the first list_lens[b] entries (0 <= list_lens[b] <= L = list_stride) of row b of
 * list_pids; entries are pids as search returns them (1-based, pid_offset added), in any order, duplicates allowed.
 *   candidates: the DISTINCT listed passages that lie in the handle's range and hold at least one embedding (a passage
 *            without embeddings -- empty at create, emptied by remove / update -- never is one, as under CLB_FILTER_ALL).
 *            nprobe is validated and otherwise unused; a query of length 0 has no candidates.
 *   result:  bit for bit that of clb_search_batch_filtered with a CLB_FILTER_ALL filter made from the same pids -- pids, fp32
 *            scores, n_cand, pid 0 / -Inf padding.  Always padded: a short list is no error.
 *   list_scores (optional, [B][L] fp32): the exact fp32 score of the passage at every INPUT position -- MaxSim, or with a prior
 *            E = fl32(e + fl32(weight * value)) -- the bits the ranked output reports for that pid; every occurrence of a
 *            duplicate receives it.  -Inf where the position holds no candidate: positions >= list_lens[b], pids outside the
 *            handle's range, passages without embeddings.  They are PASSAGE scores: a grouping or cursors do not change them,
 *            nor do the handle's mode, gather form or score-row form.  A call that asks for them needs the exact score of every
 *            candidate and runs as the single exact pass whatever clb_searcher_set_mode says (the two-pass mode is identical
 *            to it by construction; the handle's mode is left as it was).
 * Lists compose with everything that acts after candidate making -- grouping, per_group, prior, cursors (through
 * clb_search_batch_request*; what those refuse among themselves stays refused) -- and are refused with filters (any non-NULL
 * entry: CLB_EUNSUPPORTED, a list IS the candidate set) and on the phase routes of a shard group (CLB_EUNSUPPORTED).
 * Host route: every check runs before any device work.  One of list_pids / list_lens NULL with the other set, list_stride < 1
 * or a length outside 0..L is CLB_EARGUMENT; a pid outside pid_offset+1 .. pid_offset+n_docs is CLB_EBOUNDS naming the query and
 * the position.
 * Device route: stream-ordered, no host synchronisation, capturable, and nothing can be raised about the arrays' CONTENTS: a
 * length is clamped to 0..L and a pid outside the range is skipped (another shard's pid, as clb_filter_create_pids_global skips
 * it).  A captured graph holds the ADDRESSES of the three arrays: to re-rank under a graph, write the next batch's pids and
 * lengths into the same buffers and replay.  The slot's candidate capacity is sized from min(list_stride, n_docs), a host
 * value: a slot's first listed call, or one with a larger stride, may grow it (outside a capture); later calls allocate
 * nothing.  Batches above 64 queries run as sub-batches, each reading its own rows.
 * list_pids == NULL and list_lens == NULL here is CLB_EARGUMENT (without lists: clb_search_batch / ..._device_slot).
 *
 * List priors: re-rank with first-stage scores.  A listed call may carry one fp32 value per list position, list_prior[b][i]
 * beside list_pids[b][i], and one finite weight for the batch (prior_weight): hybrid fusion E = MaxSim + w * first-stage score,
 * teacher scores, a per-request boost -- an additive term per (query, passage), where a clb_prior holds one per passage.
 *   value:   v_b(p) of candidate p of query b is the value at the LOWEST position i < list_lens[b] with list_pids[b][i] == p: of
 *            a duplicate's values the first counts, on every route.  Values at positions >= list_lens[b], beside pids outside
 *            the handle's range and beside passages without embeddings are never read as values.
 *   result:  clb_prior's formulas -- pi = fl32(weight * v_b(p)), E = fl32(e(p) + pi), one rounded multiply and one rounded add,
 *            never an fma -- the first k candidates by (E descending, pid ascending), the scores E.  Row b is bit for bit the
 *            same handle's call for query b alone with the list and a clb_prior that holds v_b(p) for listed p and 0 elsewhere.
 *            Candidates, n_cand and padding are those of the call without list priors; all-zero values or weight 0 give its bits.
 *            list_scores then holds E at every input position.  In the two-pass mode the cut is that of a prior
 *            (tau - 2 delta - 2 eps).
 *   with:    a grouping (per_group 0 or 1: a group is represented by its candidate with the largest E).  CLB_EUNSUPPORTED
 *            together with a prior (a call has ONE additive term), with per_group > 1 and with cursors; CLB_EARGUMENT without
 *            lists and with a weight that is not finite.  All answered before the searcher is looked at.
 * Host route, before any device work: a value at a position i < list_lens[b] that is not finite is CLB_EARGUMENT naming the
 * query and the position, and so is |weight| * max |value| over those positions not below FLT_MAX.
 * Device route: nothing can be raised about the values either -- one that is not finite, or whose product with the weight is
 * not finite, counts as 0.  Stream-ordered and capturable like the lists: a graph holds the ADDRESS of the value block.  A
 * slot's first call with list priors may grow it by 4 bytes per query and candidate of its capacity; later calls allocate
 * nothing.  With list_prior == NULL the two entries below launch exactly what clb_search_batch_listed* launch.
 * ---------------------------------------------------------------------------------------------- */
int clb_search_batch_listed(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                            const int64_t* list_pids, const int64_t* list_lens, int64_t list_stride,
                            float* list_scores /* may be NULL */, int64_t* out_pids, float* out_scores, int64_t* n_cand);
int clb_search_batch_listed_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                        int64_t k, const int64_t* d_list_pids, const int64_t* d_list_lens, int64_t list_stride,
                                        float* d_list_scores /* may be NULL */, int64_t* d_out_pids, float* d_out_scores,
                                        int64_t* d_n_cand, void* hip_stream);
int clb_search_batch_listed_prior(clb_searcher* s, const float* Q, int64_t T, int64_t B, int64_t nprobe, int64_t k,
                                  const int64_t* list_pids, const int64_t* list_lens, int64_t list_stride,
                                  const float* list_prior /* may be NULL */, float weight, float* list_scores /* may be NULL */,
                                  int64_t* out_pids, float* out_scores, int64_t* n_cand);
int clb_search_batch_listed_prior_device_slot(clb_searcher* s, int slot, const float* d_Q, int64_t T, int64_t B, int64_t nprobe,
                                              int64_t k, const int64_t* d_list_pids, const int64_t* d_list_lens,
                                              int64_t list_stride, const float* d_list_prior /* may be NULL */, float weight,
                                              float* d_list_scores /* may be NULL */, int64_t* d_out_pids, float* d_out_scores,
                                              int64_t* d_n_cand, void* hip_stream);

/* retrieve()  (src/search/ranking.jl:23-44) on its own -- test hook.  out_pids needs n_docs entries. */
int clb_retrieve(clb_searcher* s, const float* Q, int64_t T, int64_t nprobe, int64_t* out_pids,
                 int64_t* n_out);

/* Test hook for the two-pass mode: for one query returns every candidate pid with its approximate (pass 1) and
 * exact score, the selection threshold tau (k-th largest approximate score), the proven error bound eps and the
 * number of candidates with approx >= tau - 2 eps (those the exact pass re-scores).  The report is that of the two-pass
 * pipeline whatever clb_searcher_set_mode says (the handle's mode is left as it was). */
int clb_debug_scores(clb_searcher* s, const float* Q, int64_t T, int64_t nprobe, int64_t k, int64_t cap,
                     int64_t* out_pids, float* out_approx, float* out_exact, int64_t* n_out, float* tau,
                     float* eps, int64_t* n_rescore);

/* Merge per-shard top-k lists (device pointers): `n_lists` lists of k (pid, score) records per query,
 * each sorted by (score desc, pid asc) and padded with (0, -Inf).  Input layout [n_lists][B][k] (k
 * fastest) -- what an all-gather of every rank's (k, B) result produces; output (k, B).  Replaces the
 * final sortperm of search() across passage shards (searching.jl:125-127). */
int clb_merge_topk_device(int device, const int64_t* d_pids, const float* d_scores, int64_t k,
                          int64_t n_lists, int64_t B, int64_t* d_out_pids, float* d_out_scores,
                          void* hip_stream);
/* The same merge over PACKED per-rank blocks, so that one all-gather moves a rank's whole result: block r of
 * `d_packed` is clb_packed_topk_bytes(k, B) bytes = [B*k int64 pids][B*k fp32 scores][pad to 8 bytes].  A rank
 * produces its block by pointing clb_search_batch_device's d_out_pids / d_out_scores into one such buffer. */
int64_t clb_packed_topk_bytes(int64_t k, int64_t B);
int clb_merge_topk_packed_device(int device, const void* d_packed, int64_t k, int64_t n_lists, int64_t B,
                                 int64_t* d_out_pids, float* d_out_scores, void* hip_stream);

/* clb_merge_topk_device for grouped results: every record carries its global group index (d_gids, [n_lists][B][k], -1
 * for padding; the indices of one list are distinct, and an index two lists share is the lowest or the highest of each --
 * what contiguous shards give).  Records are ordered by (score desc, pid asc); of the records of one group only the first
 * survives; the first k survivors are written, padded with (0, -Inf).  d_n_cand_lists [n_lists][B] and d_edge_gids
 * [n_lists][B][2] are the shards' d_n_cand and d_edge_gids: d_out_n_cand[b] = the sum of the lists' counts minus the number
 * of lists whose first edge group equals the last edge group of the nearest list before it that has candidates -- a group
 * over two or more shards is counted once.  At most 256 lists. */
int clb_merge_topk_grouped_device(int device, const int64_t* d_pids, const float* d_scores, const int64_t* d_gids, int64_t k,
                                  int64_t n_lists, int64_t B, const int64_t* d_n_cand_lists, const int64_t* d_edge_gids,
                                  int64_t* d_out_pids, float* d_out_scores, int64_t* d_out_n_cand, void* hip_stream);
/* The same over PACKED per-shard blocks, so that one all-gather moves a shard's whole grouped result: block r of `d_packed`
 * is clb_packed_grouped_bytes(k, B) bytes = [the clb_packed_topk_bytes(k, B) block of pids and scores][B*k int64 group
 * indices][B int64 n_cand][B*2 int64 edge groups].  A shard produces its block by pointing the outputs of
 * clb_search_shard_phase2_grouped_slot (or of the grouped search and clb_search_result_groups_slot) into one such buffer. */
int64_t clb_packed_grouped_bytes(int64_t k, int64_t B);
int clb_merge_topk_grouped_packed_device(int device, const void* d_packed, int64_t k, int64_t n_lists, int64_t B,
                                         int64_t* d_out_pids, float* d_out_scores, int64_t* d_out_n_cand, void* hip_stream);

/* Per-kernel timing with HIP events on the stream the kernels are launched on (bench.py's roofline).
 * enable, run searches, then read: names[i] (static strings), total milliseconds and launch counts.
 * Returns the number of entries written (<= cap). */
/* on = 0: off; 1: event timing only; 2: timing + the work counters read by clb_last_batch_stats (one extra
 * kernel per batch, so keep it out of timed regions). */
int clb_profile_enable(clb_searcher* s, int on);
int clb_profile_read(clb_searcher* s, const char** names, double* total_ms, int64_t* launches, int cap);
/* per-kernel work counters of the last batch: candidate passages / candidate embeddings summed over
 * the WHOLE batch of the last call (a batch above 64 queries runs as 64-query sub-batches inside the call: the counters
 * add up over them; the per-query flag / candidate-count scratch of a workspace slot holds the last sub-batch only), and
 * embeddings re-scored by the exact pass */
int clb_last_batch_stats(clb_searcher* s, int64_t* cand_docs, int64_t* cand_embs, int64_t* rescored_docs,
                         int64_t* rescored_embs);
/* two-pass mode, same batch and same counters run: the rows the exact pass multiplied against query tokens 0..15
 * (rows_lo) and against tokens 16..31 (rows_hi; 0 when the query has at most 16 tokens).  A row selected by tokens of
 * both halves counts in both, so max(rows_lo, rows_hi) <= rescored_embs <= rows_lo + rows_hi.  Both are 0 outside the
 * two-pass mode. */
int clb_last_batch_half_rows(clb_searcher* s, int64_t* rows_lo, int64_t* rows_hi);

/* ------------------------------------------------------------------------------------------------
 * Codec and ranking pieces as stand-alone calls (host buffers, run on `device`).
 * ---------------------------------------------------------------------------------------------- */
/* decompress  (src/indexing/codecs/residual.jl:759-784) ; out is (dim, n) */
int clb_decompress(int device, int64_t dim, int nbits, const float* centroids, int64_t K,
                   const float* bucket_weights, int64_t n_weights, const uint32_t* codes, int64_t n_codes,
                   const uint8_t* residuals, int64_t res_rows, int64_t res_cols, float* out);
/* maxsim  (src/search/ranking.jl:69-86) ; D is (dim, n_D) */
int clb_maxsim(int device, const float* Q, int64_t dim, int64_t T, const float* D, int64_t n_D,
               const int64_t* pids, int64_t n_pids, const int64_t* doclens, int64_t n_docs, float* scores);
/* compress_into_codes!  (residual.jl:67-81) */
int clb_compress_into_codes(int device, uint32_t* codes, int64_t n_codes, const float* centroids,
                            int64_t dim, int64_t K, const float* embs, int64_t n);
/* compress  (residual.jl:586-604) : codes + packed residuals */
int clb_compress(int device, const float* centroids, int64_t K, const float* bucket_cutoffs,
                 int64_t n_cutoffs, int64_t dim, int nbits, const float* embs, int64_t n,
                 uint32_t* codes, uint8_t* residuals);
/* _normalize_array!(X, dims=1)  (src/utils.jl:320-325) */
int clb_normalize_columns(int device, float* X, int64_t dim, int64_t n);

/* ------------------------------------------------------------------------------------------------
 * Index build  (src/utils.jl:253-318, src/indexing/collection_indexer.jl)
 * ---------------------------------------------------------------------------------------------- */
/* kmeans_gpu_onehot!  (utils.jl:253-318) with the random initial centroids (utils.jl:261) supplied by
 * the caller in `centroids` (in/out, (dim,K)).  assignments: Int32[n], 1-based. */
int clb_kmeans(int device, const float* data, int64_t dim, int64_t n, float* centroids, int64_t K,
               int64_t max_iters, float tol, int64_t point_bsize, int32_t* assignments,
               int64_t* iters_done);
/* The same iteration split for a point set sharded over several GPUs (BASELINE config 5).  Each rank
 * holds its points on its device (`clb_kmeans_shard`); per iteration it computes the un-normalised per-cluster sums
 * (dim,K) and counts of ITS points with the current centroids (clb_kmeans_shard_pass: the batch loop of utils.jl:271-300
 * over the shard, batches counted from the shard's first point), the ranks all-gather these blocks (RCCL), and
 * clb_kmeans_reduce_update adds them in RANK ORDER -- total = ((p_0 + p_1) + p_2) + ..., deterministic and identical
 * on every rank -- and applies utils.jl:302-314: new = total ./ max.(counts,1), delta = max|old - new|; `delta < tol`
 * leaves `centroids` untouched and sets *converged.  With one shard the result equals clb_kmeans bit for bit. */
typedef struct clb_kmeans_shard clb_kmeans_shard;
int clb_kmeans_shard_create(int device, const float* data /* (dim, n) */, int64_t dim, int64_t n, int64_t K,
                            int64_t point_bsize, clb_kmeans_shard** out);
int clb_kmeans_shard_destroy(clb_kmeans_shard* h);
int clb_kmeans_shard_pass(clb_kmeans_shard* h, const float* centroids /* (dim,K) */, float* sums /* (dim,K) */,
                          int64_t* counts /* K */, int32_t* assignments /* n, 1-based; may be NULL */);
/* The same iteration with the exchange kept on the device (the blocks are 64 MB per rank at K = 131 072: no host round
 * trip).  The centroids live in the shard handle: set_centroids uploads the initial ones (utils.jl:261), pass_device
 * writes this rank's block -- (dim,K) fp32 sums, padded to 8 bytes, then K int64 counts: clb_kmeans_shard_block_bytes --
 * into d_block on `hip_stream`, the ranks all-gather the blocks (clb_comm_all_gather / RCCL) and update_device reduces
 * the n_ranks gathered blocks in rank order and applies utils.jl:302-314 to the handle's centroids (one 4-byte
 * read-back per iteration: delta).  Bit-identical to clb_kmeans_shard_pass + clb_kmeans_reduce_update. */
int64_t clb_kmeans_shard_block_bytes(const clb_kmeans_shard* h);
/* `centroids` may be a host or a device pointer in both calls (the runtime tells them apart) */
int clb_kmeans_shard_set_centroids(clb_kmeans_shard* h, const float* centroids /* (dim,K) */);
int clb_kmeans_shard_get_centroids(clb_kmeans_shard* h, float* centroids /* (dim,K) */);
/* A shard whose points are ALREADY in HBM (the clustering sample of a collection too large to stage through host
 * memory: 14 M x 128 fp32 at 1 M passages): d_data (dim, n) is borrowed, not copied -- the caller keeps it alive and
 * unchanged until clb_kmeans_shard_destroy. */
int clb_kmeans_shard_create_device(int device, const float* d_data /* (dim, n) device */, int64_t dim, int64_t n,
                                   int64_t K, int64_t point_bsize, clb_kmeans_shard** out);
/* the assignments of the last pass (Int32, 1-based: `assignments` of kmeans_gpu_onehot!, utils.jl:253); host or
 * device pointer, n entries */
int clb_kmeans_shard_get_assignments(clb_kmeans_shard* h, int32_t* assignments);
int clb_kmeans_shard_pass_device(clb_kmeans_shard* h, void* d_block, void* hip_stream);
int clb_kmeans_shard_update_device(clb_kmeans_shard* h, const void* d_gathered /* n_ranks blocks */, int64_t n_ranks,
                                   float tol, float* delta_out, int* converged, void* hip_stream);
int clb_kmeans_reduce_update(int device, float* centroids /* (dim,K) in/out */,
                             const float* gathered_sums /* [world][dim*K] */,
                             const int64_t* gathered_counts /* [world][K] */, int64_t world, int64_t dim, int64_t K,
                             float tol, float* delta_out, int* converged);
/* _compute_avg_residuals!  (collection_indexer.jl:177-195) incl. _bucket_cutoffs_and_weights :141-152 */
int clb_compute_avg_residuals(int device, int nbits, const float* centroids, int64_t dim, int64_t K,
                              const float* heldout, int64_t n, uint32_t* codes, int64_t n_codes,
                              float* bucket_cutoffs, float* bucket_weights, float* avg_residual);
/* _build_ivf  (collection_indexer.jl:349-353) */
int clb_build_ivf(int device, const uint32_t* codes, int64_t n, int64_t K, int64_t* ivf,
                  int64_t* ivf_lengths);
/* Test hooks of the library's own stable radix sort and exclusive scan (csrc/sort.hip: the `sortperm(codes)` of
 * collection_indexer.jl:350, the quantile sort of :147-150, the load-time re-ordering of the Searcher, the general top-k):
 * host arrays in and out.  key_bits 32 = uint32 keys sorted stably on their low end_bit bits WITH uint32 values; 64 = uint64
 * keys, with or without values; -32 = float keys, ascending.  clb_debug_exclusive_scan: out[0..n] = prefix sums of in[0..n),
 * out[n] = the total (modulo 2^32). */
int clb_debug_sort(int device, int key_bits, const void* keys, const uint32_t* vals, int64_t n, int end_bit, void* keys_out,
                   uint32_t* vals_out);
int clb_debug_exclusive_scan(int device, const uint32_t* in, int64_t n, uint32_t* out);
/* Test hook of the nearest-centroid search every index build goes through (k-means, compress, the residual statistics), at
 * dim 128: the build's own launch sequence on host arrays, read-only, plus what its tiers saw.  mode 0 = argmax of the dot
 * product (compress_into_codes!), 1 = the k-means distance.  products -1 = as shipped (COLBERT_NEAREST_PRODUCTS is honoured),
 * 1 = one fp16 product if the centroids allow it, 3 = the three-product bf16 split.  chunk_max = points per launch (the build
 * uses 1 << 22).  scratch: null, or a handle that keeps the device scratch across calls the way k-means does.
 * Out: codes UInt32[n] (1-based); lists [n][2 halves][L] of {float value, int32 group id} (the first tier's group lists,
 * L = stats[7]; id 0x7fffffff = empty slot); margins Float32[n] (what the first exact pass allowed below the best listed
 * value); tiers UInt8[n]: 0 = decided from those lists, 1 = by the second tier's lists, 2 = by the exhaustive scan.
 * stats Int64[8]: [0] single-product lists in use, [1] bits of max ||c|| (x 1.001), [2] bits of max ||c - fp16(c)|| (0 with three
 * products), [3] chunks, [4] points the first tier left undecided, [5] points sent through the second tier, [6] points that
 * tier left undecided, [7] L.  K < 32 has no lists: codes only, every other byte of lists, margins and tiers 0xff. */
typedef struct clb_nearest_scratch clb_nearest_scratch;
int clb_debug_nearest_scratch_create(int device, clb_nearest_scratch** out);
int clb_debug_nearest_scratch_destroy(clb_nearest_scratch* s);
int clb_debug_nearest(int device, int mode, int products, int64_t chunk_max, const float* centroids, int64_t K, const float* embs,
                      int64_t n, clb_nearest_scratch* scratch, uint32_t* codes, void* lists, float* margins, uint8_t* tiers,
                      int64_t* stats);
/* The same over device arrays (80 M codes at 1 M passages never visit the host): d_codes UInt32[n] 1-based,
 * d_ivf Int64[n], d_ivf_lengths Int64[K], all on `device`; runs on `hip_stream` and waits for it (the range check of
 * counts(values, K) has to be read back: CLB_EBOUNDS). */
int clb_build_ivf_device(int device, const uint32_t* d_codes, int64_t n, int64_t K, int64_t* d_ivf,
                         int64_t* d_ivf_lengths, void* hip_stream);

/* The chunk loop of index()  (src/indexing.jl:102-118, collection_indexer.jl:271-297: encode a chunk of passages ->
 * compress -> save) with the codec resident: the centroids (64 MB at K = 131 072), their bf16 split and the
 * nearest-centroid scratch are uploaded / allocated once instead of once per chunk, and a chunk's embeddings, codes and
 * residuals are device arrays -- the encoder's output (clb_encode_docs on the device) or a generator's.
 * clb_codec_create: `centroids` (dim,K) and `bucket_cutoffs` (2^nbits - 1) may be host or device pointers.
 * clb_codec_compress_device = compress (residual.jl:586-604) for n embeddings d_embs (dim, n): d_codes UInt32[n] 1-based,
 * d_residuals UInt8 (dim/8*nbits, n); enqueued on hip_stream, not waited for.  Bit-identical to clb_compress. */
typedef struct clb_codec clb_codec;
int clb_codec_create(int device, int64_t dim, int nbits, int64_t K, const float* centroids,
                     const float* bucket_cutoffs, int64_t n_cutoffs, clb_codec** out);
int clb_codec_destroy(clb_codec* c);
int clb_codec_compress_device(clb_codec* c, const float* d_embs, int64_t n, uint32_t* d_codes, uint8_t* d_residuals,
                              void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Device arrays for a host that has none of its own (the Julia shim; Python uses torch tensors for the same purpose).
 * The device-resident route of index() (src/indexing.jl:63-147 with the sample, the codes and the residuals kept in HBM:
 * clb_encode_docs_packed_device -> clb_gather_rows_device -> clb_kmeans_shard_create_device -> clb_codec_compress_device ->
 * clb_build_ivf_device -> clb_searcher_create_device) needs to allocate, fill and read back plain device buffers and to
 * cut the sampled / shuffled rows out of a device matrix -- the reference's `sample[:, randperm(...)]` and
 * `embs[:, sampled columns]` (collection_indexer.jl:56-91) -- without the embeddings crossing PCIe.
 * ---------------------------------------------------------------------------------------------- */
int clb_device_malloc(int device, int64_t bytes, void** d_out);
int clb_device_free(int device, void* d_ptr);
/* blocking copies between host memory and a buffer of clb_device_malloc (any device pointer on `device` will do) */
int clb_device_upload(int device, void* d_dst, const void* src, int64_t bytes);
int clb_device_download(int device, void* dst, const void* d_src, int64_t bytes);
int clb_device_synchronize(int device);
/* free / total bytes of HBM on `device` (index() picks the device-resident route only if its footprint fits) */
int clb_device_memory(int device, int64_t* free_bytes, int64_t* total_bytes);
/* d_dst[i, :] = d_src[d_rows[i], :] for i < n: rows of `row_bytes` bytes (a multiple of 4; column j of Julia's (dim, n_src)
 * Float32 matrix is row j here), d_rows Int64[n] on the device, 0-BASED, each in [0, n_src).  Runs on `hip_stream` and
 * waits for it: an index outside the range is CLB_EBOUNDS (nothing is read outside d_src; the destination row is zeroed).
 * d_dst must not overlap d_src. */
int clb_gather_rows_device(int device, const void* d_src, int64_t n_src, int64_t row_bytes, const int64_t* d_rows,
                           int64_t n, void* d_dst, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Exchange step of the sharded search / index build on RCCL  (the reference is single-GPU)
 * One communicator per process and GPU.  Rank 0 calls clb_comm_unique_id and hands the bytes to the other ranks by
 * whatever the host has (a file, MPI, a socket); every rank then calls clb_comm_create -- it blocks until all ranks
 * have joined.  librccl is opened at run time; without it these calls return CLB_EHIP and nothing else is affected.
 * The Python driver may use torch.distributed instead (the same RCCL underneath); hosts without torch -- the Julia
 * shim -- use these.
 * ---------------------------------------------------------------------------------------------- */
typedef struct clb_comm clb_comm;
int64_t clb_comm_unique_id_bytes(void);
int clb_comm_unique_id(void* id, int64_t bytes);
int clb_comm_create(int device, int rank, int n_ranks, const void* id, int64_t bytes, clb_comm** out);
int clb_comm_destroy(clb_comm* c);
int clb_comm_rank(const clb_comm* c);
int clb_comm_size(const clb_comm* c);
/* all-gather of `bytes_per_rank` bytes from every rank, in rank order, into d_recv (n_ranks * bytes_per_rank), enqueued
 * on hip_stream: the packed per-shard top-k blocks (clb_packed_topk_bytes -> clb_merge_topk_packed_device), the (B, k)
 * score blocks between clb_search_shard_phase1 and phase2, the cluster sums of clb_kmeans_shard_pass. */
int clb_comm_all_gather(clb_comm* c, const void* d_send, void* d_recv, int64_t bytes_per_rank, void* hip_stream);
/* element-wise maximum over the ranks, in place (the six bound constants of clb_searcher_get/set_bound_consts) */
int clb_comm_all_reduce_max_f32(clb_comm* c, float* d_buf, int64_t n, void* hip_stream);
/* The whole round trip the two-phase sharded search needs once per shard group, inside the library (a host without its
 * own device arrays -- the Julia shim -- cannot hand clb_comm_all_reduce_max_f32 a device pointer):
 * clb_searcher_get_bound_consts -> all-reduce MAX over the communicator -> clb_searcher_set_bound_consts.  Collective:
 * every rank of `c` calls it with its shard's handle.  Blocks until done. */
int clb_searcher_sync_bound_consts(clb_searcher* s, clb_comm* c);

/* ------------------------------------------------------------------------------------------------
 * Encoder  (src/modelling/checkpoint.jl)
 * ---------------------------------------------------------------------------------------------- */
typedef struct clb_encoder clb_encoder;
/* The BERT + Dense weights of a ColBERT checkpoint (what load_hgf_pretrained_local returns,
 * src/local_loading.jl:139-209) as ONE flat fp32 blob, torch Linear layout [out][in]:
 *   word_emb [vocab][H], pos_emb [max_pos][H], type_emb [type_vocab][H], emb_ln_gamma [H], emb_ln_beta [H],
 *   per layer: Wq,Wk,Wv [3H][H], bq,bk,bv [3H], Wo [H][H], bo [H], ln1_gamma, ln1_beta [H],
 *              W1 [I][H], b1 [I], W2 [H][I], b2 [H], ln2_gamma, ln2_beta [H],
 *   linear_W [dim][H], linear_b [dim].
 * tools/export_checkpoint.py writes it from a HuggingFace directory. */
int clb_encoder_create(int device, int64_t vocab, int64_t hidden, int64_t layers, int64_t heads,
                       int64_t intermediate, int64_t max_pos, int64_t type_vocab, int64_t dim, float ln_eps,
                       const float* weights, int64_t n_weights, clb_encoder** out);
int clb_encoder_destroy(clb_encoder* e);
/* Arithmetic of the Linear layers (the reference multiplies in Float32, checkpoint.jl:21-25 through Transformers.jl).
 * Every fp32 operand is split into 16-bit planes and the product is a sum of exact MFMA plane products in an fp32
 * accumulator.  mode 3 (default) = "f16x3": two fp16 planes of the operand scaled by a power of two (round-to-nearest makes
 * two fp16 planes hold all 24 significant bits), three products, error per product < 2^-23 |a||b|; fp16's exponent range
 * limits the activations to |x| < 4 094 (an encode that leaves it reports CLB_EDOMAIN: non-finite output).
 * mode 2 = "bf16x6": three bf16 planes, six products, < 2^-22 per product over the whole fp32 range; mode 1 = "bf16x3": two
 * bf16 planes, three products, < 2^-15; mode 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32, 1/16 of the 16-bit rate). */
int clb_encoder_set_gemm_mode(clb_encoder* e, int mode);
/* Self-attention for head size 64 and up to 512 positions: mode 0 (default) = fused in registers -- behind the f16x3 Linear
 * layers on the 16-bit matrix pipe, on fp16 planes the Q/K/V projection writes for it (three exact products per fp32
 * product; batches of more than 64 tokens), else fp32 MFMA (all score tiles resident up to 64 keys, online softmax beyond);
 * 1 = fp32 MFMA, register-resident for every length; 2 = the three-kernel path (scores in memory; always taken for other head
 * sizes); 3 = mode 0 on the fp32 MFMA whatever the GEMM mode -- 1 to 3 exist for comparison.  5 (the K / V tiles of a
 * (sequence, head) staged once in LDS: bit-identical to 0 and slower) was retired and returns CLB_EUNSUPPORTED. */
int clb_encoder_set_attention_mode(clb_encoder* e, int mode);
/* LayerNorm folded around the Linear layers (f16x3 only): the Linear that produces a LayerNorm's input stores the raw rows and
 * their partial (mean, M2); the Linear that consumes it multiplies the raw rows with gamma (.) W and applies
 * rstd (a . (gamma (.) W)^T - mean u) + c in its epilogue -- no stand-alone LayerNorm pass (48.7 us x 24 per 64 x 300 passage
 * batch).  Same function of the inputs as `doc` (src/modelling/checkpoint.jl:21-25), different rounding.
 * mode: -1 = batches too long to split over K (the default: a 64 x 300 passage batch 14.34 -> 13.93 ms,
 * profiles/r05_experiments.md), 0 = never, 1 = always (tests). */
int clb_encoder_set_ln_fold(clb_encoder* e, int mode);
/* doc(bert, linear, integer_ids, bitmask)  (checkpoint.jl:21-25): integer_ids Int32 (L, N), 1-based token ids;
 * bitmask (L, N) 0/1 bytes = attention (key) mask; out Float32 (dim, L, N).  No epilogue follows this forward, so one
 * small pass of its own looks for non-finite rows: CLB_EDOMAIN, like the other entry points. */
int clb_encode(clb_encoder* e, const int32_t* integer_ids, const uint8_t* bitmask, int64_t L, int64_t N, float* out);
/* _doc_embeddings_and_doclens  (checkpoint.jl:27-52): forward, clear skiplist tokens, normalise, doclens,
 * compaction.  out_embs (dim, <= L*N); doclens Int64[N]; *n_out = kept columns.
 * When every unattended token (bitmask 0) is one the skiplist drops -- the [PAD] padding of tensorize_docs is -- and the
 * encoder runs the fp16-plane attention, the rows the output never sees are not computed (the batch is packed on the way to
 * the device, attended tokens keep their positions): same outputs up to the rounding of a different tile plan, about twice
 * the throughput on batches padded to their longest passage.  Otherwise the whole (L, N) batch is computed. */
int clb_encode_docs(clb_encoder* e, const int32_t* integer_ids, const uint8_t* bitmask, int64_t L, int64_t N,
                    const int64_t* skiplist, int64_t n_skip, float* out_embs, int64_t* doclens, int64_t* n_out);
/* _query_embeddings  (checkpoint.jl:54-71): forward, clear skiplist tokens, normalise.  out (dim, L, N). */
int clb_encode_queries(clb_encoder* e, const int32_t* integer_ids, const uint8_t* bitmask, int64_t L, int64_t N,
                       const int64_t* skiplist, int64_t n_skip, float* out);

/* _query_embeddings with every pointer on the encoder's device, enqueued on `hip_stream` and not waited for: the
 * (dim, L, N) output is what clb_search_batch_device takes as d_Q, so encode_queries + search (src/searching.jl:93-127)
 * run back to back without leaving HBM.  d_skiplist: n_skip Int64 ids on the device.  An id outside the vocabulary
 * cannot be reported from an asynchronous call: it is clamped (use clb_encode_queries to validate inputs). */
int clb_encode_queries_device(clb_encoder* e, const int32_t* d_integer_ids, const uint8_t* d_bitmask, int64_t L, int64_t N,
                              const int64_t* d_skiplist, int64_t n_skip, float* d_out, void* hip_stream);
/* _doc_embeddings_and_doclens  (checkpoint.jl:27-52) with every pointer on the encoder's device, enqueued on `hip_stream`
 * and not waited for: forward, skiplist mask, normalisation, doclens and compaction without a host round trip -- the chunk
 * loop of index() (src/indexing.jl:102-118) then hands the embeddings of a batch straight to clb_codec_compress_device.
 * d_out_embs: capacity (dim, L*N); the first *d_n_out columns are valid (read d_n_out / d_doclens back when needed).
 * Ids outside the vocabulary are clamped and reported by clb_encoder_check_last_ids, like clb_encode_queries_device. */
int clb_encode_docs_device(clb_encoder* e, const int32_t* d_integer_ids, const uint8_t* d_bitmask, int64_t L, int64_t N,
                           const int64_t* d_skiplist, int64_t n_skip, float* d_out_embs, int64_t* d_doclens,
                           int64_t* d_n_out, void* hip_stream);
/* The same for a PACKED batch -- N passages back to back without padding rows: d_ids[rows] token ids (1-based), d_pos[rows]
 * the position of every token in its passage (0-based), d_seq[rows] its passage (0..N-1), d_cu[N + 1] the row offsets
 * (d_cu[N] = rows), Lmax the longest passage.  tensorize_docs (doc_tokenization.jl:143-156) pads a batch to its longest
 * passage with [PAD], which the attention mask hides and the skiplist drops (checkpoint.jl:37-43): the padding rows never
 * reach the output, and with passages of ~80 tokens in batches padded to ~160 they are half of the encoder's work.  Here
 * they are not computed.  Every row counts as attended.  Needs the fp16-plane attention (head size 64, GEMM mode 3,
 * attention mode 0): CLB_EARGUMENT otherwise -- the caller then pads.  Outputs as clb_encode_docs_device. */
int clb_encode_docs_packed_device(clb_encoder* e, const int32_t* d_ids, const int32_t* d_pos, const int32_t* d_seq,
                                  const int32_t* d_cu, int64_t N, int64_t Lmax, int64_t rows, const int64_t* d_skiplist,
                                  int64_t n_skip, float* d_out_embs, int64_t* d_doclens, int64_t* d_n_out, void* hip_stream);
/* The asynchronous device path cannot report an id outside the vocabulary when it is enqueued (it clamps): this call
 * waits for the device and returns the BoundsError of ANY device-path encode since the previous check (the flag is
 * sticky: set by the kernels, cleared by this call), or CLB_EDOMAIN when an encode produced non-finite embeddings (the
 * f16x3 split's range).  The host-buffer entry points (clb_encode, clb_encode_docs, clb_encode_queries) enqueue the same
 * forward and epilogue as their device counterparts on the encoder's own stream and read the flag themselves, once per
 * call, before they copy any result out: they report both from the call itself and leave the flag clear. */
int clb_encoder_check_last_ids(clb_encoder* e);
/* The sticky flag itself: *d_flag receives the device address of the int32 the encode kernels OR their findings into
 * (bit 0: id outside the vocabulary, bit 1: non-finite output).  A serving loop copies its 4 bytes back together with the
 * results of a query (search(searcher, query::String, k), src/searching.jl:93-127) and calls clb_encoder_check_last_ids only
 * when it is non-zero -- an asynchronous encode whose activations leave the f16 split's range would otherwise hand NaN
 * scores to the caller without an error.  The address is stable for the life of the handle; valid after the first encode
 * or this call (which allocates and clears the flag if no encode has run yet). */
int clb_encoder_error_flag_device(clb_encoder* e, void** d_flag);
/* Per-stage HIP-event timing of the encoder forward (bench.py's encoder roofline; the stages are the Linear layers of
 * `doc`, src/modelling/checkpoint.jl:21-25, by role).  enable, run encodes, then read: names[i] (static strings), total
 * milliseconds and stage executions since the last read.  Returns the number of entries written (<= cap), -1 on error. */
int clb_encoder_profile_enable(clb_encoder* e, int on);
int clb_encoder_profile_read(clb_encoder* e, const char** names, double* total_ms, int64_t* launches, int cap);
/* Test hooks of the encoder's tile plans.  Every Linear of `doc` (src/modelling/checkpoint.jl:21-25) picks its work-group tile,
 * the depth of its LDS ring and the number of K slices from (M, N, K), its epilogue and what surrounds it; the rule is one pure
 * function.  clb_debug_encoder_plan evaluates it without a device: gemm_mode 1 to 3 (the modes whose Linear layers run on
 * planes), epi = the epilogue bits (1 bias, 2 GELU, 4 residual), flags = CLB_PLAN_* -> out[0..4] = tile rows, tile columns, ring
 * stages, K slices, and the pass that sums the slices (0 none, 1 fused with the LayerNorm four columns per lane, 2 / 3 fused
 * with the LayerNorm for widths that are not multiples of four (<= 768 / <= 1 024), 4 plain, 5 plain writing the attention
 * planes).  clb_encoder_last_plans: what the LAST forward of this handle launched, in launch order -- names[i] is the stage
 * (the names of clb_encoder_profile_read), records[i * CLB_ENCODER_PLAN_FIELDS ...] = layer (the projection: the number of
 * layers), M, N, K, tile rows, tile columns, stages, K slices, reduce pass, flags, epilogue bits.  The attention kernel of a
 * layer has a record of its own under "attention": M = rows, N = sequence length, K = head size, tile rows = query blocks of
 * 32 per wave (0: an fp32 kernel), tile columns = key tiles of 32, epilogue field = 0 fp16 planes, 1 fp32 online softmax,
 * 2 fp32 register-resident, 3 three kernels.  Filled on the host while the launches are enqueued (a replayed graph does not
 * touch it); the fp32 GEMM path (mode 0, or a model whose shape keeps it off the planes) records its attention only.
 * Returns the number of records written (<= cap), -1 on error. */
enum {
    CLB_ENCODER_PLAN_FIELDS = 11,
    CLB_PLAN_PART = 1,         /* split-K scratch is available to this Linear */
    CLB_PLAN_LN = 2,           /* a LayerNorm of the output follows (its own pass, or fused into the reduce pass) */
    CLB_PLAN_ATT = 4,          /* the output feeds the fp16-plane attention (Q | K planes, key-blocked V) */
    CLB_PLAN_FOLD = 8,         /* a LayerNorm is folded around the product (clb_encoder_set_ln_fold) ... */
    CLB_PLAN_FOLD_STATS = 16,  /* ... whose row statistics it produces */
    CLB_PLAN_FOLD_U = 32,      /* ... whose row statistics it consumes (gamma (.) W planes, vectors u and c) */
    CLB_PLAN_PACKED = 64       /* records only: the batch was packed (clb_encode_docs_packed_device) */
};
int clb_debug_encoder_plan(int gemm_mode, int64_t M, int64_t N, int64_t K, int epi, int flags, int* out);
int clb_encoder_last_plans(clb_encoder* e, const char** names, int64_t* records, int cap);


/* Encoder epilogue as stand-alone calls  (src/modelling/checkpoint.jl:27-71, embedding_utils.jl:172-205) */
/* _doc_embeddings_and_doclens after doc(): clear skiplist tokens, normalise, doclens, compaction.
 * D (dim, L, N) is read only; out (dim, <= L*N); doclens Int64[N]; *n_out = kept columns. */
int clb_doc_epilogue(int device, const float* D, int64_t dim, int64_t L, int64_t N,
                     const int32_t* integer_ids, const int64_t* skiplist, int64_t n_skip, float* out,
                     int64_t* doclens, int64_t* n_out);
/* _query_embeddings after doc(): clear skiplist tokens, normalise (in place). */
int clb_query_epilogue(int device, float* Q, int64_t dim, int64_t L, int64_t N,
                       const int32_t* integer_ids, const int64_t* skiplist, int64_t n_skip);

#ifdef __cplusplus
}
#endif
#endif
