// prior_kernels.hpp -- score priors: rank by MaxSim plus a resident per-passage term (no counterpart in the reference; the
// rank_feature / function_score of Elasticsearch, a first-phase expression over an attribute in Vespa).  A prior is one
// finite fp32 value per local passage; a call adds weight * value[p] to the score of every candidate p:
//     pi(p) = fl32(weight * value[p])      one rounded multiply
//     E(p)  = fl32(e(p) + pi(p))           one rounded add, never contracted into an fma
// and ranks by E.  The candidates of a query are slots of an ascending pid list (bitmap_emit_kernel): the prior is read
// through cand[slot], a 4-byte gather in a table of 4 MB per million passages.
// In the two-pass mode the boost runs twice: on the approximate scores right after pass 1 (the selection then cuts on
// A = fl(a + pi), at the threshold prior_tau_kernel leaves) and on the exact scores of the re-scored list after pass 2.
// Nothing between the two reads the slot's score buffer as a MaxSim value: the row sweep works from tokmax / eps_pair and the
// exact kernel only writes it.
// Across a shard group (the two phase calls with a prior) the first boost runs in phase 1, which publishes the shard's k largest
// A and its largest |A|, and prior_global_tau_kernel forms phase 2's threshold from what all shards published.
#pragma once
#include "approx_kernels.hpp"
#include "group_kernels.hpp"
#include "search_kernels.hpp"

namespace clb {

// Where P1 reads the value of a candidate slot.  A resident prior: values[cand[slot]], one value per local passage.  List
// priors (kListed; list_kernels.hpp): the values travel beside the caller's candidate lists, row b of stride L for query b,
// and slot_pos[b][slot] (stride pos_stride) is the lowest list position that names the slot's passage (list_slot_kernel).
// Such values come straight from the caller on the device route, where nothing can be raised: a value that is not finite,
// or whose product with the weight is not finite, counts as 0 -- what the host route would have refused.
struct PriorTerm {
    const float* values;
    const int* slot_pos;
    int L;
    size_t pos_stride;
};
template <bool kListed>
__device__ __forceinline__ float prior_value(const PriorTerm& t, int b, uint32_t passage, int slot, float weight) {
    if (!kListed) return t.values[passage];
    if ((size_t)slot >= t.pos_stride) return 0.f;      // (a listed query has no more candidates than that: never taken)
    const int pos = t.slot_pos[(size_t)b * t.pos_stride + slot];
    if (pos < 0 || pos >= t.L) return 0.f;             // (every candidate came from the list: never taken)
    const float v = t.values[(size_t)b * t.L + pos];
    const bool fin = fabsf(v) < __builtin_inff() && fabsf(__fmul_rn(weight, v)) < __builtin_inff();
    return fin ? v : 0.f;
}

// P1.  scores[b][slot] = fl(scores[b][slot] + fl(weight * value(slot))) for the query's nlist[b] listed slots or, with
// list == nullptr, its ncand[b] candidate slots 0, 1, ...; value(slot) by PriorTerm.  mabs (optional, [B]): max |new score|
// over those slots (NaN ignored), the M of prior_tau_kernel.  grid = B, block = 1024.
template <bool kListed>
static __global__ __launch_bounds__(1024) void prior_boost_kernel(float* __restrict__ scores,
                                                                 const uint32_t* __restrict__ cand,
                                                                 const int* __restrict__ ncand,
                                                                 const int* __restrict__ list /*optional*/,
                                                                 const int* __restrict__ nlist,
                                                                 PriorTerm term, float weight,
                                                                 size_t cand_cap, float* __restrict__ mabs /*optional*/) {
    __shared__ unsigned int s_max;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = list ? nlist[b] : ncand[b];
    float* sc = scores + (size_t)b * cand_cap;
    const uint32_t* cnd = cand + (size_t)b * cand_cap;
    const int* lst = list ? list + (size_t)b * cand_cap : nullptr;
    if (tid == 0) s_max = 0u;
    float m = 0.f;
    for (int i = tid; i < n; i += 1024) {
        const int slot = lst ? lst[i] : i;
        const float pi = __fmul_rn(weight, prior_value<kListed>(term, b, cnd[slot], slot, weight));
        const float v = __fadd_rn(sc[slot], pi);
        sc[slot] = v;
        m = fmaxf(m, fabsf(v));
    }
    if (!mabs) return;                                 // uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __syncthreads();
    if ((tid & 63) == 0) atomicMax(&s_max, __float_as_uint(m));      // non-negative floats order as their bits
    __syncthreads();
    if (tid == 0) mabs[b] = __uint_as_float(s_max);
}

// P2 (two-pass mode).  tau_out[b] = tau - 2 delta: tau a lower bound, to 2^-16 of the key range, of the k-th largest boosted
// approximate score A among the query's candidates -- or, with glist, among scores[glist[b][i]], i < nglist[b]: the best
// A of every group (group_collapse_kernel), i.e. group_tau_kernel's value -- and
//     delta = 4 * 2^-24 * (M + eps),   M = mabs[b] = max |A| over ALL the query's candidates, eps = the query's eps_sum,
// the rounding slack of DESIGN section 5: with |a - e| <= eps, A = fl(a + pi) and E = fl(e + pi),
//     |E - A| <= eps + 2^-24 (|e + pi| + |a + pi|) <= eps + 2^-24 (2 M / (1 - 2^-24) + eps) =: eps + delta0,
// so every member of the true top k by E has A >= tau - 2 eps - 2 delta0; the selection forms fl(fl(tau - 2 delta) - 2 eps),
// whose two roundings add at most 2^-24 (2 M + 4 delta + 2 eps): delta >= delta0 + 2^-24 (M + eps + 2 delta) holds for
// delta = 4 * 2^-24 (M + eps), which exceeds 2^-24 (3 M + 2 eps) by more than every second-order term left out.
// -inf (fewer than k entries, an unsafe query, a non-finite M): the selection lists everything (margin_threshold).
// The selection kernels (select_margin_kernel / wide_*) then run unchanged with tau_in = tau_out.  grid = B, block = 1024.
static __global__ __launch_bounds__(1024) void prior_tau_kernel(const float* __restrict__ scores,
                                                               const int* __restrict__ ncand,
                                                               const int* __restrict__ glist /*optional*/,
                                                               const int* __restrict__ nglist, int k, size_t cand_cap,
                                                               const float* __restrict__ mabs,
                                                               const float* __restrict__ Q, int T, ApproxConsts ac,
                                                               const float4* __restrict__ tscale, int cell8,
                                                               float* __restrict__ tau_out) {
    __shared__ __attribute__((aligned(16))) int hist[256];
    __shared__ uint32_t s_prefix, s_kmin, s_kmax;
    __shared__ int s_remaining;
    __shared__ float s_aux[4];
    __shared__ float s_qn, s_dq;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = glist ? nglist[b] : ncand[b];
    if (n < k) {                                       // uniform over the block
        if (tid == 0) tau_out[b] = kNegInf;
        return;
    }
    const QueryBound qb = query_bound(Q, b, T, ac, &s_qn, &s_dq, tscale, s_aux, cell8 != 0);
    const float* sc = scores + (size_t)b * cand_cap;
    const int* lst = glist ? glist + (size_t)b * cand_cap : nullptr;
    const int chunk = (n + 1023) >> 10;
#define CLB_SEL_FOR_EACH(...)                                                                   \
    for (int c = 0; c < chunk; ++c) {                                                           \
        const int i_ = c * 1024 + tid;                                                          \
        const bool valid = i_ < n;                                                              \
        const uint32_t key = valid ? f32_order_key(sc[lst ? lst[i_] : i_]) : 0u;                \
        __VA_ARGS__                                                                             \
    }
    if (tid == 0) { s_prefix = 0u; s_remaining = k; }
    __syncthreads();
    CLB_RADIX_SELECT_N(2)
#undef CLB_SEL_FOR_EACH
    if (tid == 0) {
        const float tau = f32_from_order_key(s_prefix);
        const float u = 5.9604645e-08f;  // 2^-24
        const float delta = 4.f * u * (mabs[b] + qb.eps_sum);
        const float t = tau - 2.f * delta;
        tau_out[b] = (qb.unsafe || !(t > kNegInf)) ? kNegInf : t;      // NaN-safe: a non-finite slack lists everything
    }
}

// P3 (two-phase search of a shard group with a prior, phase 2).  tau_out[b] = tau - 2 delta from what the shards published in
// phase 1, all_top [n_shards][B][k] (each shard's k largest boosted approximate scores A, -inf padding) and all_mabs
// [n_shards][B] (each shard's M_i = max |A| over ITS candidates of the query):
//     tau   = the k-th largest gathered A -- with all_gid ([n_shards][B][k], the global group index of every record, -1 padding)
//             over the DISTINCT indices, a repeated index counting once with its largest value (group_global_tau_kernel's
//             rule) -- -inf with fewer than k: the k-th largest A over the union C of the shards' candidates, or a lower bound;
//     M     = max_i M_i: |A(p)| <= M for every p in C and |tau| <= M, what P2's argument needs over C.  A shard's own M_i is
//             NOT enough: another shard's large prior values can lift tau to a magnitude whose rounding its M_i does not cover;
//     delta = 4 * 2^-24 * (M + eps), eps the query's eps_sum under the group's shared bound constants (eps_in[b] when given
//             -- the test hook -- else query_bound).
// -inf for an unsafe query and for a non-finite M or eps.  n_shards <= kMaxGroupShards with all_gid.  grid = B, block = 1024.
static __global__ __launch_bounds__(1024) void prior_global_tau_kernel(const float* __restrict__ all_top,
                                                                      const int64_t* __restrict__ all_gid /*optional*/,
                                                                      const float* __restrict__ all_mabs, int n_shards, int B,
                                                                      int k, const float* __restrict__ eps_in /*optional*/,
                                                                      const float* __restrict__ Q, int T, ApproxConsts ac,
                                                                      const float4* __restrict__ tscale, int cell8,
                                                                      float* __restrict__ tau_out) {
    __shared__ __attribute__((aligned(16))) int hist[256];
    __shared__ uint32_t s_prefix, s_kmin, s_kmax, s_mbits;
    __shared__ int s_remaining;
    __shared__ float s_aux[4];
    __shared__ float s_qn, s_dq;
    __shared__ long long e_gid[2 * kMaxGroupShards];
    __shared__ uint32_t e_key[2 * kMaxGroupShards];
    __shared__ int e_at[2 * kMaxGroupShards];
    __shared__ int e_dead[2 * kMaxGroupShards];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = n_shards * k;
    if (tid == 0) { s_prefix = 0u; s_remaining = k; s_mbits = 0u; }
    if (all_gid) group_boundary_records(all_top, all_gid, n_shards, B, b, k, e_gid, e_key, e_at, e_dead);
    __syncthreads();
    {   // M: |x| of a NaN orders above +inf as bits, +inf above every finite value -- a non-finite M_i survives the maximum
        uint32_t m = 0u;
        for (int l = tid; l < n_shards; l += 1024) {
            const uint32_t v = __float_as_uint(fabsf(all_mabs[(size_t)l * B + b]));
            m = v > m ? v : m;
        }
        if (m) atomicMax(&s_mbits, m);
    }
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
            const bool gone_ = all_gid && (all_gid[at_] < 0 || (e_at[2 * l_] == i_ && e_dead[2 * l_]) || \
                                           (e_at[2 * l_ + 1] == i_ && e_dead[2 * l_ + 1]));     \
            key = gone_ ? neg_key : f32_order_key(all_top[at_]);                                \
        }                                                                                       \
        __VA_ARGS__                                                                             \
    }
    CLB_RADIX_SELECT()
#undef CLB_SEL_FOR_EACH
    float eps = 0.f;
    bool unsafe = false;
    if (eps_in) {                                      // uniform over the block
        eps = eps_in[b];
    } else {
        const QueryBound qb = query_bound(Q, b, T, ac, &s_qn, &s_dq, tscale, s_aux, cell8 != 0);
        eps = qb.eps_sum;
        unsafe = qb.unsafe;
    }
    if (tid == 0) {
        const float tau = f32_from_order_key(s_prefix);
        const float u = 5.9604645e-08f;  // 2^-24
        const float delta = 4.f * u * (__uint_as_float(s_mbits) + eps);
        const float t = tau - 2.f * delta;
        tau_out[b] = (unsafe || !(t > kNegInf)) ? kNegInf : t;        // NaN-safe: a non-finite slack lists everything
    }
}

// clb_prior_create_device: the values of a prior checked where they are.  out[0] = the index of the first non-finite value
// (n: none), out[1] = the bits of max |value| over the finite ones; both start as {n, 0}.
static __global__ __launch_bounds__(256) void prior_check_kernel(const float* __restrict__ v, int64_t n,
                                                                unsigned long long* __restrict__ out) {
    unsigned long long bad = (unsigned long long)n;
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float x = v[i];
        const bool fin = fabsf(x) < __builtin_inff();  // false for NaN and +-Inf
        if (!fin && (unsigned long long)i < bad) bad = (unsigned long long)i;
        m = fin ? fmaxf(m, fabsf(x)) : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ob = __shfl_xor(bad, o, 64);
        bad = ob < bad ? ob : bad;
        m = fmaxf(m, __shfl_xor(m, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad < (unsigned long long)n) atomicMin(&out[0], bad);
        atomicMax(&out[1], (unsigned long long)__float_as_uint(m));
    }
}

}  // namespace clb
