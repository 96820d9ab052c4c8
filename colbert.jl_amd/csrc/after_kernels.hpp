// after_kernels.hpp -- search after a cursor: the next k results past a (score, pid) (no counterpart in the reference; the
// search_after of Elasticsearch, a continuation token in Vespa).  A cursor is one pair (s*, p*) per query, s* an fp32 score
// and p* a global 1-based pid; with e(p) the exact fp32 MaxSim score of candidate p,
//     after(p)  <=>  e(p) < s*   or   (e(p) == s* and pid(p) > p*)
// and the call returns the first k members of {p : after(p)} by (e descending, pid ascending): what the ranking of the
// call without a cursor continues with.  s* = +Inf: no cursor for that query (p* ignored), every candidate is after it.
// s* = -Inf or NaN: nothing is after it.  The candidate set and the count a call reports are those of the call without one.
// Two kernels, both one work-group per query with the cursors read from device memory (a captured graph holds the ADDRESSES
// of the cursor arrays): after_cut_kernel moves the cut of the two-pass mode behind the cursor and
// after_filter_kernel, in every mode, hands the top-k forms the exact-scored slots that lie after it.
// Between pass 1 and pass 2 nothing reads the slot's score buffer as a MaxSim value (prior_kernels.hpp): the cut writes
// -Inf over the approximate score of a candidate that is certainly before the cursor, and the selection leaves it out.
#pragma once
#include "approx_kernels.hpp"
#include "search_kernels.hpp"

namespace clb {

constexpr float kAfterFltMax = 3.4028234663852886e+38f;
constexpr float kAfterFltMin = 1.1754943508222875e-38f;      // the smallest normal number

// One fp32 step down / up.  From (-FLT_MIN, FLT_MIN] the step down goes to -FLT_MIN (no subnormal is ever formed: a longer
// step keeps the inequality it is taken for); an infinity of the step's own sign stays, the other one becomes -+FLT_MAX.
__device__ __forceinline__ float f32_step_down(float x) {
    if (x == kNegInf) return x;
    if (x == __builtin_inff()) return kAfterFltMax;
    if (x <= kAfterFltMin && x > -kAfterFltMin) return -kAfterFltMin;
    const uint32_t u = __float_as_uint(x);
    return __uint_as_float(x > 0.f ? u - 1u : u + 1u);
}
__device__ __forceinline__ float f32_step_up(float x) { return -f32_step_down(-x); }

// a cursor score as the kernels read it: NaN counts as -Inf (an empty page; the host entry point refuses it)
__device__ __forceinline__ float after_cursor_score(float s) { return s != s ? kNegInf : s; }

// A1 (two-pass mode, between pass 1 and the selection).  With |a - e| <= eps (the query's eps_sum) and
//     lo = one step below fl(s* - eps)  <=  s* - eps,      hi = one step above fl(s* + eps)  >=  s* + eps
// a candidate with a < lo is SURE (e < s*: after the cursor) and one with a > hi has PASSED (e > s*: before it).
// tau_out[b] = tau - delta, tau a lower bound (to 2^-16 of the key range) of the k-th largest a over the sure candidates and
//     delta = 2^-22 (|tau| + 2 eps)
// the slack that keeps the two roundings of fl(fl(tau - delta) - 2 eps), the threshold the selection forms, below tau - 2 eps:
// they add at most 2^-24 (2 |tau| + 2 delta + 2 eps) < delta.  The k sure candidates with a >= tau have e >= tau - eps and are
// after the cursor, so the k-th member of the answer has e >= tau - eps and every member a >= tau - 2 eps; every member has
// e <= s*, hence a <= hi: {a >= tau - 2 eps and a <= hi} holds the whole answer, ties at rank k included.
// Fewer than k sure candidates: no cut -- tau_out = -FLT_MAX, whose threshold lies below every score and above the -Inf
// written over the passed candidates (the selection lists !(a < thr), so a -Inf threshold would list them again).
// An unsafe query (eps = inf): tau_out = -Inf and nothing is masked; the selection lists everything.  s* = +Inf: every
// candidate is sure and none has passed (never +Inf - eps); with fewer than k candidates tau_out = -Inf as without a cursor.
// The selection kernels (select_margin_kernel / wide_*) then run unchanged with tau_in = tau_out.  grid = B, block = 1024.
static __global__ __launch_bounds__(1024) void after_cut_kernel(float* __restrict__ scores, const int* __restrict__ ncand,
                                                               int k, size_t cand_cap,
                                                               const float* __restrict__ after_s,
                                                               const float* __restrict__ Q, int T, ApproxConsts ac,
                                                               const float4* __restrict__ tscale, int cell8,
                                                               float* __restrict__ tau_out) {
    __shared__ __attribute__((aligned(16))) int hist[256];
    __shared__ uint32_t s_prefix, s_kmin, s_kmax;
    __shared__ int s_remaining, s_sure;
    __shared__ float s_aux[4];
    __shared__ float s_qn, s_dq;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = ncand[b];
    const QueryBound qb = query_bound(Q, b, T, ac, &s_qn, &s_dq, tscale, s_aux, cell8 != 0);
    if (qb.unsafe) {                                   // uniform over the block
        if (tid == 0) tau_out[b] = kNegInf;
        return;
    }
    const float cur = after_cursor_score(after_s[b]);
    const bool open = cur == __builtin_inff();         // no cursor
    const float eps = qb.eps_sum;
    const float lo = open ? cur : f32_step_down(__fsub_rn(cur, eps));
    const float hi = open ? cur : f32_step_up(__fadd_rn(cur, eps));
    float* sc = scores + (size_t)b * cand_cap;
    const int chunk = (n + 1023) >> 10;
    if (tid == 0) { s_prefix = 0u; s_remaining = k; s_sure = 0; }
    __syncthreads();
    int sure = 0;
    for (int c = 0; c < chunk; ++c) {
        const int i = c * 1024 + tid;
        sure += i < n && (open || sc[i] < lo);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sure += __shfl_xor(sure, o, 64);
    if ((tid & 63) == 0 && sure) atomicAdd(&s_sure, sure);
    __syncthreads();
    const bool cut = s_sure >= k;                      // uniform
    if (cut) {
#define CLB_SEL_FOR_EACH(...)                                                                   \
    for (int c = 0; c < chunk; ++c) {                                                           \
        const int i_ = c * 1024 + tid;                                                          \
        const float a_ = i_ < n ? sc[i_] : 0.f;                                                 \
        const bool valid = i_ < n && (open || a_ < lo);                                         \
        const uint32_t key = valid ? f32_order_key(a_) : 0u;                                    \
        __VA_ARGS__                                                                             \
    }
        CLB_RADIX_SELECT_N(2)
#undef CLB_SEL_FOR_EACH
    }
    // (every read of the approximate scores above is behind a barrier: a masked score would otherwise count as sure)
    if (tid == 0) {
        float t = open ? kNegInf : -kAfterFltMax;
        if (cut) {
            const float tau = f32_from_order_key(s_prefix);
            const float delta = 2.3841858e-07f /* 2^-22 */ * (fabsf(tau) + 2.f * eps);
            t = __fsub_rn(tau, delta);
            if (!(t > -kAfterFltMax)) t = open ? kNegInf : -kAfterFltMax;      // NaN-safe
        }
        tau_out[b] = t;
    }
    if (open) return;
    for (int c = 0; c < chunk; ++c) {
        const int i = c * 1024 + tid;
        if (i < n && sc[i] > hi) sc[i] = kNegInf;
    }
}

// A2 (every mode and route, between the exact scores and the ranking).  out_list[b] = the slots with after(e, pid), pid =
// pid_offset + cand[slot] + 1, among the query's listed slots (list / nlist: the re-scored list of the two-pass mode) or,
// with list == nullptr, among its ncand[b] candidate slots 0, 1, ...; out_n[b] = their number.  The order of the input is
// kept (ascending slots = ascending pids: the top-k forms take the first of a run of equal scores by position).
// Thread t owns the contiguous positions [t * chunk, (t + 1) * chunk); one block-wide scan places the chunks.
// grid = B, block = 1024.
static __global__ __launch_bounds__(1024) void after_filter_kernel(const float* __restrict__ scores,
                                                                  const uint32_t* __restrict__ cand,
                                                                  const int* __restrict__ ncand,
                                                                  const int* __restrict__ list /*optional*/,
                                                                  const int* __restrict__ nlist,
                                                                  const float* __restrict__ after_s,
                                                                  const int64_t* __restrict__ after_p, size_t cand_cap,
                                                                  int64_t pid_offset, int* __restrict__ out_list,
                                                                  int* __restrict__ out_n) {
    __shared__ int sh_scan[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = list ? nlist[b] : ncand[b];
    const float* sc = scores + (size_t)b * cand_cap;
    const uint32_t* cnd = cand + (size_t)b * cand_cap;
    const int* lst = list ? list + (size_t)b * cand_cap : nullptr;
    int* out = out_list + (size_t)b * cand_cap;
    const float cur = after_cursor_score(after_s[b]);
    const int64_t curp = after_p[b];
    const bool open = cur == __builtin_inff(), closed = cur == kNegInf;
    const int chunk = (n + 1023) >> 10;
    const int i0 = tid * chunk, i1 = min(i0 + chunk, n);
#define CLB_AFTER_KEEP(slot_)                                                                   \
    (open || (!closed && (sc[slot_] < cur ||                                                    \
                          (sc[slot_] == cur && pid_offset + (int64_t)cnd[slot_] + 1 > curp))))
    int cnt = 0;
    for (int i = i0; i < i1; ++i) {
        const int slot = lst ? lst[i] : i;
        cnt += CLB_AFTER_KEEP(slot);
    }
    const int lane = tid & 63, wave = tid >> 6;
    int x = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh_scan[wave] = x;
    __syncthreads();
    int wbase = 0, tot = 0;
    for (int w2 = 0; w2 < 16; ++w2) {
        const int sv = sh_scan[w2];
        if (w2 < wave) wbase += sv;
        tot += sv;
    }
    int pos = wbase + x - cnt;                         // < tot <= n <= cand_cap
    for (int i = i0; i < i1; ++i) {
        const int slot = lst ? lst[i] : i;
        if (CLB_AFTER_KEEP(slot)) out[pos++] = slot;
    }
#undef CLB_AFTER_KEEP
    if (tid == 0) out_n[b] = tot;
}

}  // namespace clb
