// Grouped retrieval (include/hrag.h, hrag_group_rows / hrag_retrieve_grouped): passage score rows [B][ld] -> one score
// and one representative passage per GROUP of passages (source documents), ready for the row ranking of topk.hip.
//
// group_reduce_kernel<AGG, MASKED>: a group CSR (group_ptr int64 [G + 1], members int32, ascending inside a group) and
// optionally the doc filter's bitset.  Per (query, group):
//   representative  the allowed member with the largest ranking key (common.h rank_key: score descending, ties -> larger
//                   passage position, every NaN above +inf) -- a max of 64-bit keys, order-free;
//   MAX             the representative's score as stored;
//   SUM             the allowed members' scores added in fp64 in ASCENDING MEMBER ORDER, rounded once to fp32: what
//                   np.bincount(weights=float64) does.  No atomics, no tree: one dependent chain of fp64 adds per
//                   (query, group) -- a member that is not allowed adds +0.0, which leaves a chain that started at +0.0
//                   unchanged bit for bit (x + 0 = x; -0 cannot arise from +0 + anything).
// A group without an allowed member gets score 0, representative -1 and a clear bit in the group bitset the kernel emits;
// the ranking runs masked by that bitset, so no score value has to stand for "absent" (NaN and -inf are real scores).
//
// Work split: a workgroup takes 256 consecutive groups of ONE query (blockIdx.y).  Groups of up to kGroupLaneMax members:
// one lane walks one group -- chunks of a source are usually consecutive positions, so the 64 lanes of a wavefront read
// one nearly contiguous span of the row and re-use its cache lines over the iterations.  Longer groups: the wavefront that
// met the group walks it together, 64 members per step -- coalesced where the members are consecutive, the key maximum per
// lane then across lanes; for SUM every lane adds the 64 scores of the step in member order (v_readlane broadcasts), so
// the chain is the sequential one: the loads are parallel, the adds are not, by definition.
//
// group_hits_kernel<MASKED> (hrag_group_hits_rows / hrag_last_group_hits): the m best allowed members of each RANKED group.
// One wavefront owns one (query, ranked slot): it walks the group's members 64 per step like the long-group path above,
// every lane forming the ranking key of its member (0: not allowed), and keeps the best keys seen so far SORTED ACROSS ITS
// LANES -- lane i holds the i-th best.  A step whose keys all lie below the held m-th key is skipped after one ballot;
// otherwise the step's keys are bitonic-sorted across the lanes, the elementwise maximum of the held list against the
// reversed new list is a bitonic sequence holding the best 64 of both, and the 6-stage bitonic merge sorts it again.  Keys
// are unique (the position is their low half), so the result does not depend on any order of execution; no atomics, no
// scratch, no LDS.  Lanes < m write the position and the score decoded from the key -- the canonical quiet NaN, -0 as +0,
// as every ranking returns scores.
#include <algorithm>

#include "common.h"

namespace hrag {

namespace {

constexpr int kGroupThreads = 256;
constexpr int kGroupLaneMax = 64;   // members one lane walks alone

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int lane) {
    const uint32_t lo = __shfl((uint32_t)v, lane, 64), hi = __shfl((uint32_t)(v >> 32), lane, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

template <int AGG, bool MASKED>
__global__ __launch_bounds__(kGroupThreads) void group_reduce_kernel(
    const float *__restrict__ scores, int64_t n, int64_t ld, const int64_t *__restrict__ group_ptr,
    const int32_t *__restrict__ members, int64_t n_groups, const uint32_t *__restrict__ mask, int64_t mask_ld,
    int64_t mask_bit0, float *__restrict__ gscore, int32_t *__restrict__ gbest, int64_t out_ld,
    uint32_t *__restrict__ gmask, int64_t gmask_ld) {
    const int q = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kGroupThreads + threadIdx.x;
    const float *row = scores + (size_t)q * ld;
    const uint32_t *mrow = MASKED ? mask + (size_t)q * mask_ld : nullptr;
    auto allowed = [&](int32_t m) -> bool {
        if ((uint64_t)(uint32_t)m >= (uint64_t)n) return false;   // a member outside the row is never read
        if constexpr (MASKED) {
            const int64_t b = mask_bit0 + m;
            return (mrow[b >> 5] >> (b & 31)) & 1u;
        }
        return true;
    };
    int64_t beg = 0, end = 0;
    if (g < n_groups) {
        beg = group_ptr[g];
        end = group_ptr[g + 1];
        beg = beg < 0 ? 0 : beg > n ? n : beg;          // the member array has n entries
        end = end < beg ? beg : end > n ? n : end;
    }
    const int64_t len = end - beg;
    uint64_t best = 0;
    double acc = 0.0;
    if (len <= kGroupLaneMax) {
        for (int64_t j = beg; j < end; ++j) {
            const int32_t m = members[j];
            if (!allowed(m)) continue;
            const float v = row[m];
            const uint64_t key = rank_key(v, (uint32_t)m);
            best = key > best ? key : best;
            if constexpr (AGG == HRAG_GROUP_SUM) acc += (double)v;
        }
    }
    // long groups of this wavefront, one after the other, all 64 lanes on each
    uint64_t todo = __ballot(len > kGroupLaneMax);
    while (todo) {
        const int owner = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const int64_t b0 = (int64_t)shfl_u64((uint64_t)beg, owner), e0 = (int64_t)shfl_u64((uint64_t)end, owner);
        uint64_t wbest = 0;
        double wacc = 0.0;
        for (int64_t j0 = b0; j0 < e0; j0 += 64) {
            const int64_t j = j0 + lane;
            float v = 0.f;
            if (j < e0) {
                const int32_t m = members[j];
                if (allowed(m)) {
                    v = row[m];
                    const uint64_t key = rank_key(v, (uint32_t)m);
                    wbest = key > wbest ? key : wbest;
                }
            }
            if constexpr (AGG == HRAG_GROUP_SUM) {
                // the 64 scores of this step in member order; lanes past the end and members not allowed hold +0.0
#pragma unroll
                for (int i = 0; i < 64; ++i) wacc += (double)__shfl(v, i, 64);
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t other = shfl_xor_u64(wbest, o);
            wbest = other > wbest ? other : wbest;
        }
        if (lane == owner) { best = wbest; acc = wacc; }
    }
    const bool present = best != 0;
    if (g < n_groups) {
        const int32_t rep = present ? (int32_t)(uint32_t)best : -1;
        float out = 0.f;
        if (present) out = AGG == HRAG_GROUP_SUM ? (float)acc : row[rep];
        gscore[(size_t)q * out_ld + g] = out;
        gbest[(size_t)q * out_ld + g] = rep;
    }
    if (gmask) {
        const uint64_t bits = __ballot(present);
        const int64_t word = (g - lane) >> 5;   // the wavefront's 64 groups are words word, word + 1
        const int64_t words = (n_groups + 31) >> 5;
        if (lane == 0 && word < words) gmask[(size_t)q * gmask_ld + word] = (uint32_t)bits;
        if (lane == 32 && word + 1 < words) gmask[(size_t)q * gmask_ld + word + 1] = (uint32_t)(bits >> 32);
    }
}

// compare-exchange with the lane `o` away: the lane that `keep_max` names keeps the larger key, its partner the smaller
__device__ __forceinline__ uint64_t cmp_xchg(uint64_t v, int o, bool keep_max) {
    const uint64_t other = shfl_xor_u64(v, o);
    return (other > v) == keep_max ? other : v;
}

constexpr int kHitsThreads = 256;   // four wavefronts, one (query, ranked slot) each

template <bool MASKED>
__global__ __launch_bounds__(kHitsThreads) void group_hits_kernel(
    const float *__restrict__ scores, int64_t n, int64_t ld, const int64_t *__restrict__ group_ptr,
    const int32_t *__restrict__ members, int64_t n_groups, const uint32_t *__restrict__ mask, int64_t mask_ld,
    int64_t mask_bit0, const int32_t *__restrict__ group_idx, int32_t k, int32_t hits, int32_t *__restrict__ hit_idx,
    float *__restrict__ hit_score) {
    const int q = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * (kHitsThreads / 64) + (threadIdx.x >> 6);
    if (slot >= k) return;                                   // wavefront-uniform
    const float *row = scores + (size_t)q * ld;
    const uint32_t *mrow = MASKED ? mask + (size_t)q * mask_ld : nullptr;
    auto allowed = [&](int32_t m) -> bool {
        if ((uint64_t)(uint32_t)m >= (uint64_t)n) return false;   // a member outside the row is never read
        if constexpr (MASKED) {
            const int64_t b = mask_bit0 + m;
            return (mrow[b >> 5] >> (b & 31)) & 1u;
        }
        return true;
    };
    const int64_t g = group_idx[(size_t)q * k + slot];
    int64_t beg = 0, end = 0;
    if (g >= 0 && g < n_groups) {                            // a padded slot (-1) or an id outside the table: an empty row
        beg = group_ptr[g];
        end = group_ptr[g + 1];
        beg = beg < 0 ? 0 : beg > n ? n : beg;               // the member array has n entries
        end = end < beg ? beg : end > n ? n : end;
    }
    uint64_t held = 0;                                       // lane i: the i-th best key so far (0: none)
    for (int64_t j0 = beg; j0 < end; j0 += 64) {
        const int64_t j = j0 + lane;
        uint64_t key = 0;
        if (j < end) {
            const int32_t m = members[j];
            if (allowed(m)) key = rank_key(row[m], (uint32_t)m);
        }
        if (!__ballot(key > shfl_u64(held, hits - 1))) continue;   // nothing here enters the best `hits`
        // bitonic sort, descending over the lanes: blocks of kk lanes alternate descending / ascending until kk = 64
#pragma unroll
        for (int kk = 2; kk <= 64; kk <<= 1)
#pragma unroll
            for (int o = kk >> 1; o > 0; o >>= 1) key = cmp_xchg(key, o, ((lane & o) == 0) == ((lane & kk) == 0));
        if (j0 != beg) {
            // held (descending) against the new keys reversed (ascending): the maxima are the best 64 of both, bitonic
            const uint64_t rev = shfl_u64(key, 63 - lane);
            key = rev > held ? rev : held;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) key = cmp_xchg(key, o, (lane & o) == 0);
        }
        held = key;
    }
    if (lane < hits) {
        const size_t at = ((size_t)q * k + slot) * hits + lane;
        hit_idx[at] = held ? (int32_t)(uint32_t)held : -1;
        hit_score[at] = held ? ordered_to_f32((uint32_t)(held >> 32)) : 0.f;
    }
}

// out[q][i] = (s - mn[q]) / (mx[q] - mn[q]), a zero range giving 1: the normalisation the dense ranking applies to the
// scores it returns (topk.hip minmax_norm), as a row so that groups can be formed over it
__global__ void minmax_rows_kernel(const float *__restrict__ src, int64_t n, int64_t ld, const float *__restrict__ mn,
                                   const float *__restrict__ mx, float *__restrict__ dst, int64_t dst_ld) {
    const int q = blockIdx.y;
    const float lo = mn[q], range = mx[q] - lo;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[(size_t)q * dst_ld + i] = range == 0.f ? 1.f : __fdiv_rn(src[(size_t)q * ld + i] - lo, range);
}

// best_doc[q][j] = gbest[q][group_idx[q][j]] (-1 where the ranking padded)
__global__ void group_best_kernel(const int32_t *__restrict__ group_idx, const int32_t *__restrict__ gbest, int64_t gld,
                                  int64_t n_groups, int32_t k, int32_t batch, int32_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)batch * k) return;
    const int64_t q = t / k;
    const int32_t gi = group_idx[t];
    out[t] = (gi >= 0 && gi < n_groups) ? gbest[(size_t)q * gld + gi] : -1;
}

}  // namespace

hrag_status launch_group_reduce(const float *scores, int32_t batch, int64_t n, int64_t ld, const int64_t *group_ptr,
                                const int32_t *members, int64_t n_groups, int32_t agg, const TopkMask *mask,
                                float *gscore, int32_t *gbest, int64_t out_ld, uint32_t *gmask, int64_t gmask_ld,
                                hipStream_t s) {
    HRAG_REQUIRE(scores && group_ptr && members && gscore && gbest, "NULL argument");
    HRAG_REQUIRE(batch >= 1 && batch <= 65535, "batch=%d outside [1, 65535]", batch);
    HRAG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && ld >= n, "n=%lld / ld=%lld: 1 <= n < 2^31, ld >= n", (long long)n,
                 (long long)ld);
    HRAG_REQUIRE(n_groups >= 1 && n_groups <= n, "n_groups=%lld outside [1, n=%lld]", (long long)n_groups, (long long)n);
    HRAG_REQUIRE(out_ld >= n_groups, "out_ld=%lld < n_groups=%lld", (long long)out_ld, (long long)n_groups);
    HRAG_REQUIRE(agg == HRAG_GROUP_MAX || agg == HRAG_GROUP_SUM, "agg=%d: HRAG_GROUP_MAX (0) or HRAG_GROUP_SUM (1)", agg);
    HRAG_REQUIRE(!gmask || gmask_ld >= (n_groups + 31) / 32, "group bitset rows of %lld words, %lld needed",
                 (long long)gmask_ld, (long long)((n_groups + 31) / 32));
    if (mask) {
        HRAG_REQUIRE(mask->words != nullptr && mask->bit_offset >= 0, "bad filter");
        HRAG_REQUIRE(mask->ld_words == 0 || mask->ld_words >= (mask->bit_offset + n + 31) / 32,
                     "filter_ld_words=%lld: 0 (one row for the batch) or >= ceil((bit offset + n) / 32) = %lld",
                     (long long)mask->ld_words, (long long)((mask->bit_offset + n + 31) / 32));
    }
    const dim3 grid((unsigned)ceil_div(n_groups, kGroupThreads), (unsigned)batch);
    const uint32_t *mw = mask ? mask->words : nullptr;
    const int64_t mld = mask ? mask->ld_words : 0, mb0 = mask ? mask->bit_offset : 0;
#define HRAG_GROUP_LAUNCH(A, M)                                                                                        \
    hipLaunchKernelGGL((group_reduce_kernel<A, M>), grid, dim3(kGroupThreads), 0, s, scores, n, ld, group_ptr, members, \
                       n_groups, mw, mld, mb0, gscore, gbest, out_ld, gmask, gmask_ld)
    if (agg == HRAG_GROUP_SUM) {
        if (mask) HRAG_GROUP_LAUNCH(HRAG_GROUP_SUM, true); else HRAG_GROUP_LAUNCH(HRAG_GROUP_SUM, false);
    } else {
        if (mask) HRAG_GROUP_LAUNCH(HRAG_GROUP_MAX, true); else HRAG_GROUP_LAUNCH(HRAG_GROUP_MAX, false);
    }
#undef HRAG_GROUP_LAUNCH
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status launch_group_hits(const float *scores, int32_t batch, int64_t n, int64_t ld, const int64_t *group_ptr,
                              const int32_t *members, int64_t n_groups, const int32_t *group_idx, int32_t k, int32_t hits,
                              const TopkMask *mask, int32_t *hit_idx, float *hit_score, hipStream_t s) {
    HRAG_REQUIRE(scores && group_ptr && members && group_idx && hit_idx && hit_score, "NULL argument");
    HRAG_REQUIRE(batch >= 1 && batch <= 65535, "batch=%d outside [1, 65535]", batch);
    HRAG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && ld >= n, "n=%lld / ld=%lld: 1 <= n < 2^31, ld >= n", (long long)n,
                 (long long)ld);
    HRAG_REQUIRE(n_groups >= 1 && n_groups <= n, "n_groups=%lld outside [1, n=%lld]", (long long)n_groups, (long long)n);
    HRAG_REQUIRE(k >= 1, "k=%d: at least 1", k);
    HRAG_REQUIRE(hits >= 1 && hits <= HRAG_GROUP_HITS_MAX, "hits=%d outside [1, HRAG_GROUP_HITS_MAX=%d]", hits,
                 HRAG_GROUP_HITS_MAX);
    if (mask) {
        HRAG_REQUIRE(mask->words != nullptr && mask->bit_offset >= 0, "bad filter");
        HRAG_REQUIRE(mask->ld_words == 0 || mask->ld_words >= (mask->bit_offset + n + 31) / 32,
                     "filter_ld_words=%lld: 0 (one row for the batch) or >= ceil((bit offset + n) / 32) = %lld",
                     (long long)mask->ld_words, (long long)((mask->bit_offset + n + 31) / 32));
    }
    const dim3 grid((unsigned)ceil_div(k, kHitsThreads / 64), (unsigned)batch);
    if (mask)
        hipLaunchKernelGGL((group_hits_kernel<true>), grid, dim3(kHitsThreads), 0, s, scores, n, ld, group_ptr, members,
                           n_groups, mask->words, mask->ld_words, mask->bit_offset, group_idx, k, hits, hit_idx, hit_score);
    else
        hipLaunchKernelGGL((group_hits_kernel<false>), grid, dim3(kHitsThreads), 0, s, scores, n, ld, group_ptr, members,
                           n_groups, (const uint32_t *)nullptr, (int64_t)0, (int64_t)0, group_idx, k, hits, hit_idx,
                           hit_score);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status launch_minmax_rows(const float *src, int32_t batch, int64_t n, int64_t ld, const float *mn, const float *mx,
                               float *dst, int64_t dst_ld, hipStream_t s) {
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n, 256), 1024), (unsigned)batch);
    hipLaunchKernelGGL(minmax_rows_kernel, grid, dim3(256), 0, s, src, n, ld, mn, mx, dst, dst_ld);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status launch_group_best(const int32_t *group_idx, const int32_t *gbest, int64_t gld, int64_t n_groups, int32_t k,
                              int32_t batch, int32_t *out, hipStream_t s) {
    const int64_t total = (int64_t)batch * k;
    hipLaunchKernelGGL(group_best_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, group_idx, gbest, gld,
                       n_groups, k, batch, out);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

}  // namespace hrag
