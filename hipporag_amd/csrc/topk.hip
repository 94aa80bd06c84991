// K4 -- row-wise top-k selection with the library ranking rule (score desc, index desc), fused
// with the row min / max that min_max_normalize needs.
//
// Replaces the full np.argsort(...)[::-1] of the reference wherever only a prefix is consumed:
//   rerank_facts      np.argsort(query_fact_scores)[-link_top_k:][::-1]   HippoRAG.py:1683-1688
//   run_ppr           np.argsort(doc_scores)[::-1] (top retrieval_top_k)   HippoRAG.py:1746, :503
//   dense_passage_retrieval  np.argsort(query_doc_scores)[::-1]            HippoRAG.py:1500
// and min_max_normalize (utils/misc_utils.py:130-139) for the selected entries.
//
// One 1024-thread workgroup per row, two streaming passes, everything else in LDS:
//   pass 1: every thread keeps its 2 largest 64-bit keys (ordered(score) << 32 | index; keys are
//           unique, so ties need no special casing) and the running min / max.  The k-th largest
//           of the 2048 thread-local maxima is a lower bound L of the true k-th key (at least k
//           elements are >= L).
//   pass 2: keys >= L are appended to an LDS candidate buffer (expected k..~1.3k entries),
//           bitonic-sorted descending, and the first k are written out.
// If the candidates overflow the buffer (an adversarial distribution, or simply a large k on a long row) the bound is
// refined by radix histograms over the key space (10 bits per streaming pass, round 6; bisection before) until they fit,
// and pass 2 is repeated; correctness never depends on luck.
#include <algorithm>

#include "common.h"

namespace hrag {
namespace {

constexpr int TK_THREADS = 1024;
constexpr int TK_CAP = 4096;  // LDS candidate capacity (32 KiB of keys)

__device__ __forceinline__ void bitonic_sort_desc(uint64_t *buf, int n_pow2, int tid) {
    for (int size = 2; size <= n_pow2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (n_pow2 >> 1); t += TK_THREADS) {
                const int i = ((t / stride) * (stride << 1)) + (t % stride);
                const int j = i + stride;
                const bool first_half = (i & size) == 0;
                const uint64_t a = buf[i], b = buf[j];
                if ((a < b) == first_half) {
                    buf[i] = b;
                    buf[j] = a;
                }
            }
            __syncthreads();
        }
    }
}

template <typename F>
__device__ __forceinline__ void for_each_in_row(const float *s, int64_t n, int tid, F f) {
    const bool vec = (reinterpret_cast<uintptr_t>(s) & 15) == 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        const float4 *s4 = reinterpret_cast<const float4 *>(s);
        int64_t i = tid;
        // four independent 16-byte loads in flight per lane (one per iteration left a 1024-thread workgroup with 16 KB
        // outstanding: latency-bound at ~1/3 of the stream rate on 125k-long rows); the SET of elements a thread sees is
        // unchanged, and nothing downstream depends on their order
        for (; i + 3 * TK_THREADS < n4; i += 4 * TK_THREADS) {
            const float4 v0 = s4[i], v1 = s4[i + TK_THREADS], v2 = s4[i + 2 * TK_THREADS], v3 = s4[i + 3 * TK_THREADS];
            const float4 vv[4] = {v0, v1, v2, v3};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t b = (uint32_t)(4 * (i + u * TK_THREADS));
                f(vv[u].x, b);
                f(vv[u].y, b + 1);
                f(vv[u].z, b + 2);
                f(vv[u].w, b + 3);
            }
        }
        for (; i < n4; i += TK_THREADS) {
            const float4 v = s4[i];
            f(v.x, (uint32_t)(4 * i));
            f(v.y, (uint32_t)(4 * i + 1));
            f(v.z, (uint32_t)(4 * i + 2));
            f(v.w, (uint32_t)(4 * i + 3));
        }
        for (int64_t i = (n4 << 2) + tid; i < n; i += TK_THREADS) f(s[i], (uint32_t)i);
    } else {
        for (int64_t i = tid; i < n; i += TK_THREADS) f(s[i], (uint32_t)i);
    }
}

// ---- doc filter (TopkMask): one row of the bitset, seen from element 0 of the scores the kernel streams.  bit0 need
// not be a multiple of 32 (row shards start at p_offset, split parts at part * plen, plen a multiple of 4)
struct MaskRow {
    const uint32_t *w;
    int64_t bit0;
    // bits of elements i .. i + 3 (every one < n: the words they name exist), bit u for element i + u
    __device__ __forceinline__ uint32_t nibble(int64_t i) const {
        const int64_t b = bit0 + i;
        const int sh = (int)(b & 31);
        uint32_t v = w[b >> 5] >> sh;
        if (sh > 28) v |= w[(b >> 5) + 1] << (32 - sh);
        return v;
    }
    __device__ __forceinline__ bool test(int64_t i) const {
        const int64_t b = bit0 + i;
        return (w[b >> 5] >> (b & 31)) & 1u;
    }
};

// set bits among elements [0, n) of the row (a popcount over n / 32 words: 1/32 of the score bytes); every thread
// gets the count.  acc: an LDS word, free again when this returns
__device__ __forceinline__ int64_t mask_count(const MaskRow &m, int64_t n, int tid, unsigned int *acc) {
    if (tid == 0) *acc = 0;
    __syncthreads();
    const int sh = (int)(m.bit0 & 31);
    const uint32_t *w = m.w + (m.bit0 >> 5);
    unsigned int c = 0;
    for (int64_t t = tid; t * 32 < n; t += TK_THREADS) {
        const int valid = n - t * 32 < 32 ? (int)(n - t * 32) : 32;   // bits at or above n are ignored
        uint32_t v = w[t] >> sh;
        if (sh + valid > 32) v |= w[t + 1] << (32 - sh);               // (sh > 0 here: the word exists)
        if (valid < 32) v &= (1u << valid) - 1u;
        c += (unsigned int)__popc(v);
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((tid & 63) == 0 && c) atomicAdd(acc, c);
    __syncthreads();
    const unsigned int r = *acc;
    __syncthreads();
    return (int64_t)r;
}

// for_each_in_row with the ranking key of every element: f(v, key).  Masked: a masked-out element has key 0 (no real
// key is 0, common.h), so it never passes a threshold >= 1.  The unmasked form is for_each_in_row + rank_key as before
template <bool kMasked, typename F>
__device__ __forceinline__ void for_each_key(const float *s, int64_t n, int tid, const MaskRow &m, F f) {
    if constexpr (!kMasked) {
        for_each_in_row(s, n, tid, [&](float v, uint32_t i) { f(v, rank_key(v, i)); });
    } else {
        const bool vec = (reinterpret_cast<uintptr_t>(s) & 15) == 0;
        auto four = [&](const float4 &v, uint32_t b, uint32_t bits) {   // one mask read per four scores
            f(v.x, (bits & 1u) ? rank_key(v.x, b) : 0ull);
            f(v.y, (bits & 2u) ? rank_key(v.y, b + 1) : 0ull);
            f(v.z, (bits & 4u) ? rank_key(v.z, b + 2) : 0ull);
            f(v.w, (bits & 8u) ? rank_key(v.w, b + 3) : 0ull);
        };
        if (vec) {
            const int64_t n4 = n >> 2;
            const float4 *s4 = reinterpret_cast<const float4 *>(s);
            int64_t i = tid;
            for (; i + 3 * TK_THREADS < n4; i += 4 * TK_THREADS) {   // the loads of for_each_in_row, bits alongside
                const float4 v0 = s4[i], v1 = s4[i + TK_THREADS], v2 = s4[i + 2 * TK_THREADS], v3 = s4[i + 3 * TK_THREADS];
                const uint32_t m0 = m.nibble(4 * i), m1 = m.nibble(4 * (i + TK_THREADS)),
                               m2 = m.nibble(4 * (i + 2 * TK_THREADS)), m3 = m.nibble(4 * (i + 3 * TK_THREADS));
                four(v0, (uint32_t)(4 * i), m0);
                four(v1, (uint32_t)(4 * (i + TK_THREADS)), m1);
                four(v2, (uint32_t)(4 * (i + 2 * TK_THREADS)), m2);
                four(v3, (uint32_t)(4 * (i + 3 * TK_THREADS)), m3);
            }
            for (; i < n4; i += TK_THREADS) four(s4[i], (uint32_t)(4 * i), m.nibble(4 * i));
            for (int64_t i = (n4 << 2) + tid; i < n; i += TK_THREADS) {
                const float v = s[i];
                f(v, m.test(i) ? rank_key(v, (uint32_t)i) : 0ull);
            }
        } else {
            for (int64_t i = tid; i < n; i += TK_THREADS) {
                const float v = s[i];
                f(v, m.test(i) ? rank_key(v, (uint32_t)i) : 0ull);
            }
        }
    }
}

__device__ __forceinline__ float wave_min(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// the row min / max: fminf / fmaxf, which skip NaN -- a signalling NaN is quieted first, because v_min_f32 / v_max_f32
// return NaN for one (IEEE mode) and the running extreme would restart after it
__device__ __forceinline__ void minmax_add(float &mn, float &mx, float v) {
    v = __builtin_canonicalizef(v);
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
}

__device__ __forceinline__ float minmax_norm(float s, float mn, float mx) {
    const float range = mx - mn;
    return range == 0.f ? 1.f : __fdiv_rn(s - mn, range);  // misc_utils.py:130-139
}

// parts > 1: workgroup (row_in * parts + part) selects from the slice [part * plen, +plen) of input
// row row_in and writes its k candidates (global positions, raw values) as output row blockIdx.x;
// topk_merge_kernel then picks the final k.
// kMasked: only the elements the mask allows are ranked (a part's target is min(k, its allowed count)); the row min /
// max still cover every element, or (mask.minmax_allowed: the scoped fact ranking) the allowed ones only -- a part
// without any then reports +inf / -inf, which the merge's fminf / fmaxf pass over
template <bool kMasked>
__global__ __launch_bounds__(TK_THREADS) void row_topk_kernel(
    const float *__restrict__ scores, int64_t n_total, int64_t ld, int32_t k, int32_t idx_offset_in,
    int32_t norm, int32_t *__restrict__ idx_out, float *__restrict__ val_out,
    float *__restrict__ mn_out, float *__restrict__ mx_out, int32_t parts, int64_t plen, TopkMask mask) {
    __shared__ uint64_t buf[TK_CAP];
    __shared__ float red_mn[TK_THREADS / 64], red_mx[TK_THREADS / 64];
    __shared__ unsigned int s_count;

    const int tid = threadIdx.x;
    const int row = blockIdx.x;          // output row
    const int row_in = row / parts, part = row % parts;
    const float *s = scores + (size_t)row_in * ld + (size_t)part * plen;
    int64_t n = parts > 1 ? n_total - (int64_t)part * plen : n_total;
    n = n < 0 ? 0 : (parts > 1 && n > plen ? plen : n);
    const int32_t idx_offset = parts > 1 ? (int32_t)(part * plen) : idx_offset_in;
    MaskRow mrow{nullptr, 0};
    int64_t n_sel = n;   // elements that may be selected
    if constexpr (kMasked) {
        mrow.w = mask.words + (size_t)row_in * (size_t)mask.ld_words;
        mrow.bit0 = mask.bit_offset + (parts > 1 ? (int64_t)part * plen : 0);
        n_sel = mask_count(mrow, n, tid, &s_count);
    }
    const int kk = (int)((int64_t)k < n_sel ? (int64_t)k : n_sel);

    // ---- pass 1: thread-local top-2 + min / max
    uint64_t t0 = 0, t1 = 0;
    float mn = INFINITY, mx = -INFINITY;
    for_each_key<kMasked>(s, n, tid, mrow, [&](float v, uint64_t key) {
        if (!kMasked || !mask.minmax_allowed || key != 0) minmax_add(mn, mx, v);
        if (key > t1) {
            if (key > t0) {
                t1 = t0;
                t0 = key;
            } else {
                t1 = key;
            }
        }
    });
    mn = wave_min(mn);
    mx = wave_max(mx);
    if ((tid & 63) == 0) {
        red_mn[tid >> 6] = mn;
        red_mx[tid >> 6] = mx;
    }
    buf[tid] = t0;
    buf[TK_THREADS + tid] = t1;
    __syncthreads();
    mn = red_mn[0];
    mx = red_mx[0];
    for (int w = 1; w < TK_THREADS / 64; ++w) {
        mn = fminf(mn, red_mn[w]);
        mx = fmaxf(mx, red_mx[w]);
    }
    if (tid == 0) {
        if (mn_out) mn_out[row] = mn;
        if (mx_out) mx_out[row] = mx;
    }
    if (kk == 0) {
        for (int j = tid; j < k; j += TK_THREADS) {
            idx_out[(size_t)row * k + j] = -1;
            val_out[(size_t)row * k + j] = 0.f;
        }
        return;
    }
    // A lower bound of the kk-th largest key without sorting the 2048 thread-local maxima (66 barrier stages, ~25 us --
    // most of the kernel on short rows): every wavefront finds the r-th largest of ITS 128 keys, r = ceil(kk / 16), by
    // rank counting over shuffles (keys are unique); the minimum over the 16 wavefronts has at least 16 r >= kk keys
    // above or at it.  (A wavefront with fewer than r real keys answers 0: everything is collected, and the refinement
    // below takes over if that does not fit.)
    __shared__ uint64_t wave_rth[TK_THREADS / 64];
    {
        const int r_target = (kk + TK_THREADS / 64 - 1) / (TK_THREADS / 64) - 1;     // 0-based rank inside the wavefront
        int ra = 0, rb = 0;
        for (int j = 0; j < 64; ++j) {
            const uint64_t oa = __shfl(t0, j, 64), ob = __shfl(t1, j, 64);
            ra += (oa > t0 ? 1 : 0) + (ob > t0 ? 1 : 0);
            rb += (oa > t1 ? 1 : 0) + (ob > t1 ? 1 : 0);
        }
        uint64_t mine = (ra == r_target && t0) ? t0 : ((rb == r_target && t1) ? t1 : 0);
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t other = __shfl_xor(mine, o, 64);
            mine = other > mine ? other : mine;
        }
        if ((tid & 63) == 0) wave_rth[tid >> 6] = mine;
    }
    __syncthreads();
    uint64_t thresh = wave_rth[0];
    for (int w = 1; w < TK_THREADS / 64; ++w) thresh = wave_rth[w] < thresh ? wave_rth[w] : thresh;
    if constexpr (kMasked) thresh = thresh ? thresh : 1;   // "everything" means every allowed key, never key 0
    __syncthreads();

    // ---- pass 2: collect candidates >= thresh (refine the bound first if they would not fit)
    // collect straight away (the usual case: k .. ~1.3 k candidates); only when they do NOT fit is the
    // bound refined (below) and the collection repeated -- one streaming pass less than counting first
    auto collect = [&](uint64_t t) -> unsigned int {
        if (tid == 0) s_count = 0;
        __syncthreads();
        for_each_key<kMasked>(s, n, tid, mrow, [&](float, uint64_t key) {
            if (key >= t) {
                const unsigned int slot = atomicAdd(&s_count, 1u);
                if (slot < TK_CAP) buf[slot] = key;
            }
        });
        __syncthreads();
        const unsigned int r = s_count;
        __syncthreads();
        return r;
    };
    unsigned int cnt = collect(thresh);
    if (cnt > TK_CAP) {
        // More than TK_CAP keys at or above the bound (large k on a long row: k = 2047 of 875 k in the index-time KNN puts
        // the bound at the weakest of all thread-local maxima, ~1 - 2 % of the row).  Until round 6 the exact kk-th key was
        // then found by bisection on the 64-bit key space -- up to 64 counting passes over the row, 35 of the 44 ms of a
        // 1000-query KNN block.  Radix refinement instead: a 1024-bin histogram of the keys inside [lo, hi] (LDS atomics; the
        // candidate buffer lends its memory), the bin that holds the kk-th largest is the next [lo, hi]; stop as soon as
        // count(key >= lo) fits the buffer -- 10 bits per pass and no need for the exact key: 2 - 3 passes.
        // Invariant: count(key > hi) = above < kk <= above + count(lo <= key <= hi).  It holds at the start because hi = ~0
        // lies above every key and thresh has >= kk keys at or above it.  (hi must not be derived from the row max: mx comes
        // from fmaxf, which skips NaN, and the keys of NaN scores lie above rank_key(mx, ~0) -- they would never be counted.)
        unsigned int *hist = reinterpret_cast<unsigned int *>(buf);
        static_assert(TK_THREADS == 1024, "one thread per histogram bin");
        uint64_t lo = thresh, hi = ~0ull;
        unsigned int above = 0;
        for (;;) {
            const uint64_t width = hi - lo;
            int shift = 0;
            while ((width >> shift) >= 1024) ++shift;              // bins 0 .. width >> shift <= 1023
            hist[tid] = 0;
            if (tid == 0) s_count = 0;                             // the bin search below never reads a stale count
            __syncthreads();
            for_each_key<kMasked>(s, n, tid, mrow, [&](float, uint64_t key) {
                if (key >= lo && key <= hi) atomicAdd(&hist[(unsigned int)((key - lo) >> shift)], 1u);
            });
            __syncthreads();
            for (int o = 1; o < TK_THREADS; o <<= 1) {              // hist[b] := keys in the bins >= b
                const unsigned int add = tid + o < TK_THREADS ? hist[tid + o] : 0u;
                __syncthreads();
                hist[tid] += add;
                __syncthreads();
            }
            // the counts fall with b, above + hist[0] >= kk and above < kk: exactly one bin b has
            // above + hist[b] >= kk > above + hist[b + 1] (bin 0 always qualifies for `here`)
            const bool here = above + hist[tid] >= (unsigned int)kk;
            const bool next = tid + 1 < TK_THREADS && above + hist[tid + 1] >= (unsigned int)kk;
            if (here && !next) s_count = (unsigned int)tid;
            __syncthreads();
            const int b = (int)s_count;
            const unsigned int c_ge = above + hist[b];
            const unsigned int c_gt = b + 1 < TK_THREADS ? above + hist[b + 1] : above;
            __syncthreads();
            const uint64_t blo = lo + ((uint64_t)b << shift);
            if (c_ge <= (unsigned int)TK_CAP || shift == 0) {       // (shift 0: bins are single keys, c_ge = c_gt + 1 <= kk)
                thresh = blo;
                break;
            }
            const uint64_t span = ((uint64_t)1 << shift) - 1;
            above = c_gt;
            hi = hi - blo > span ? blo + span : hi;
            lo = blo;
        }
        cnt = collect(thresh);
    }
    cnt = cnt < (unsigned int)TK_CAP ? cnt : (unsigned int)TK_CAP;
    int p2 = 2;
    while (p2 < (int)cnt) p2 <<= 1;
    for (int j = (int)cnt + tid; j < p2; j += TK_THREADS) buf[j] = 0;
    __syncthreads();
    bitonic_sort_desc(buf, p2, tid);

    for (int j = tid; j < k; j += TK_THREADS) {
        int32_t idx = -1;
        float val = 0.f;
        if (j < kk) {
            const uint64_t key = buf[j];
            idx = (int32_t)(uint32_t)key + idx_offset;
            val = ordered_to_f32((uint32_t)(key >> 32));
            if (norm == kNormMinMax) val = minmax_norm(val, mn, mx);
        }
        idx_out[(size_t)row * k + j] = idx;
        val_out[(size_t)row * k + j] = val;
    }
}

__global__ __launch_bounds__(TK_THREADS) void row_minmax_kernel(const float *__restrict__ scores,
                                                                int64_t n, int64_t ld,
                                                                float *__restrict__ mn_out,
                                                                float *__restrict__ mx_out) {
    __shared__ float red_mn[TK_THREADS / 64], red_mx[TK_THREADS / 64];
    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    const float *s = scores + (size_t)row * ld;
    float mn = INFINITY, mx = -INFINITY;
    for_each_in_row(s, n, tid, [&](float v, uint32_t) {
        minmax_add(mn, mx, v);
    });
    mn = wave_min(mn);
    mx = wave_max(mx);
    if ((tid & 63) == 0) {
        red_mn[tid >> 6] = mn;
        red_mx[tid >> 6] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < TK_THREADS / 64; ++w) {
            mn = fminf(mn, red_mn[w]);
            mx = fmaxf(mx, red_mx[w]);
        }
        mn_out[row] = mn;
        mx_out[row] = mx;
    }
}

// the scoped passage prior (launch_masked_prior): min / max over the allowed elements of the row, then the row is
// rewritten -- allowed: minmax_norm over them (the formula every prior kernel uses), others: 0
__global__ __launch_bounds__(TK_THREADS) void masked_prior_kernel(float *__restrict__ scores, int64_t n, int64_t ld,
                                                                  TopkMask mask) {
    __shared__ float red_mn[TK_THREADS / 64], red_mx[TK_THREADS / 64];
    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    float *s = scores + (size_t)row * ld;
    const MaskRow mrow{mask.words + (size_t)row * (size_t)mask.ld_words, mask.bit_offset};
    float mn = INFINITY, mx = -INFINITY;
    for_each_key<true>(s, n, tid, mrow, [&](float v, uint64_t key) {
        if (key != 0) minmax_add(mn, mx, v);
    });
    mn = wave_min(mn);
    mx = wave_max(mx);
    if ((tid & 63) == 0) {
        red_mn[tid >> 6] = mn;
        red_mx[tid >> 6] = mx;
    }
    __syncthreads();
    mn = red_mn[0];
    mx = red_mx[0];
    for (int w = 1; w < TK_THREADS / 64; ++w) {
        mn = fminf(mn, red_mn[w]);
        mx = fmaxf(mx, red_mx[w]);
    }
    // (no allowed element: mn / mx stay +-inf and every element is written 0 without reading them)
    for (int64_t i = tid; i < n; i += TK_THREADS) s[i] = mrow.test(i) ? minmax_norm(s[i], mn, mx) : 0.f;
}

// the scoped passage prior of a row shard (launch_masked_stats, launch_masked_prior_ext): the two halves of
// masked_prior_kernel with the statistics crossing the shards in between.
//   kRewrite false: mn_out / mx_out = min / max over the allowed elements of the row (+inf / -inf: none), row untouched;
//   kRewrite true:  the row rewritten with the GLOBAL allowed min / max mn_in / mx_in (allowed: minmax_norm, others: 0),
//                   mn_out / mx_out = min / max of the rewritten row.  mn_in / mx_in may alias mn_out / mx_out: every
//                   thread reads them before the barrier that precedes the write
template <bool kRewrite>
__global__ __launch_bounds__(TK_THREADS) void masked_rows_kernel(float *__restrict__ scores, int64_t n, int64_t ld,
                                                                 TopkMask mask, const float *mn_in, const float *mx_in,
                                                                 float *mn_out, float *mx_out) {
    __shared__ float red_mn[TK_THREADS / 64], red_mx[TK_THREADS / 64];
    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    float *s = scores + (size_t)row * ld;
    const MaskRow mrow{mask.words + (size_t)row * (size_t)mask.ld_words, mask.bit_offset};
    float mn = INFINITY, mx = -INFINITY;
    if constexpr (kRewrite) {
        const float lo = mn_in[row], hi = mx_in[row];
        for (int64_t i = tid; i < n; i += TK_THREADS) {
            const float v = mrow.test(i) ? minmax_norm(s[i], lo, hi) : 0.f;
            s[i] = v;
            minmax_add(mn, mx, v);
        }
    } else {
        for_each_key<true>(s, n, tid, mrow, [&](float v, uint64_t key) {
            if (key != 0) minmax_add(mn, mx, v);
        });
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    if ((tid & 63) == 0) {
        red_mn[tid >> 6] = mn;
        red_mx[tid >> 6] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < TK_THREADS / 64; ++w) {
            mn = fminf(mn, red_mn[w]);
            mx = fmaxf(mx, red_mx[w]);
        }
        mn_out[row] = mn;
        mx_out[row] = mx;
    }
}

// second level of the split selection: parts * k candidates per row (keys are unique), parts * k <= TK_CAP.
// kMasked: a part with fewer than k allowed elements left -1 slots (key 0 here), which sort last: a slot whose key is 0
// writes -1 / 0 (the row's target min(k, allowed) is then met without counting)
template <bool kMasked>
__global__ __launch_bounds__(TK_THREADS) void topk_merge_kernel(
    const int32_t *__restrict__ cand_idx, const float *__restrict__ cand_val,
    const float *__restrict__ part_mn, const float *__restrict__ part_mx, int32_t parts, int32_t k,
    int64_t n_total, int32_t idx_offset, int32_t norm, int32_t *__restrict__ idx_out,
    float *__restrict__ val_out, float *__restrict__ mn_out, float *__restrict__ mx_out) {
    __shared__ uint64_t buf[TK_CAP];
    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    const int n_cand = parts * k;
    int p2 = 2;
    while (p2 < n_cand) p2 <<= 1;
    for (int j = tid; j < p2; j += TK_THREADS) {
        uint64_t key = 0;
        if (j < n_cand) {
            const int32_t ci = cand_idx[(size_t)row * n_cand + j];
            if (ci >= 0) key = rank_key(cand_val[(size_t)row * n_cand + j], (uint32_t)ci);
        }
        buf[j] = key;
    }
    float mn = INFINITY, mx = -INFINITY;
    for (int p = 0; p < parts; ++p) {
        mn = fminf(mn, part_mn[(size_t)row * parts + p]);
        mx = fmaxf(mx, part_mx[(size_t)row * parts + p]);
    }
    __syncthreads();
    bitonic_sort_desc(buf, p2, tid);
    if (tid == 0) {
        if (mn_out) mn_out[row] = mn;
        if (mx_out) mx_out[row] = mx;
    }
    const int kk = (int)((int64_t)k < n_total ? (int64_t)k : n_total);
    for (int j = tid; j < k; j += TK_THREADS) {
        int32_t idx = -1;
        float val = 0.f;
        if (j < kk && (!kMasked || buf[j] != 0)) {
            const uint64_t key = buf[j];
            idx = (int32_t)(uint32_t)key + idx_offset;
            val = ordered_to_f32((uint32_t)(key >> 32));
            if (norm == kNormMinMax) val = minmax_norm(val, mn, mx);
        }
        idx_out[(size_t)row * k + j] = idx;
        val_out[(size_t)row * k + j] = val;
    }
}

// ---- K4': exact top-k for k > kTopkMax (any k; the full ranking of a row included)
//
// The same ranking rule and output format as row_topk_kernel, in three steps:
//   select   one workgroup per row finds the exact kk-th largest key, kk = min(k, n), by 1024-bin radix histograms over
//            the whole 64-bit key range (lo = 0, hi = ~0: keys of NaN scores are counted like any other; no pass when
//            kk == n), then streams the row once more for the row min / max and the kk keys >= that threshold (keys are
//            unique: exactly kk of them);
//   sort     kk <= kLargeTile: the keys never leave LDS (select + sort + write in one kernel); larger kk: the keys go to
//            the workspace, every kLargeTile tile is bitonic-sorted in LDS, then log2(L / kLargeTile) merge-path passes
//            (co-rank by binary search, a fixed span of kMergeSpan outputs per thread) ping-pong between two buffers --
//            the last pass writes the indices and scores.
// The atomics only decide slot order, which the sort erases: the output is deterministic.
constexpr int kMergeSpan = 8;   // outputs per thread of a merge pass

template <typename F>
__device__ __forceinline__ void wave_append(bool take, unsigned int *counter, F store) {
    // one LDS atomic per wavefront instead of one per taken element (rows where every key is taken: kk == n)
    const uint64_t m = __ballot(take);
    if (!m) return;
    const int lane = __lane_id();
    const int leader = __ffsll((unsigned long long)m) - 1;
    unsigned int base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned int)__popcll(m));
    base = __shfl(base, leader, 64);
    if (take) store(base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull)));
}

// kMasked: kk = min(k, allowed elements of the row), the search and the compaction see allowed keys only (lo starts
// at 1, above key 0); the row min / max still cover every element
template <bool kMasked>
__global__ __launch_bounds__(TK_THREADS) void large_select_kernel(
    const float *__restrict__ scores, int64_t n, int64_t ld, int32_t k, int32_t idx_offset, int32_t norm,
    int32_t *__restrict__ idx_out, float *__restrict__ val_out, float *__restrict__ mn_out, float *__restrict__ mx_out,
    uint64_t *__restrict__ keys, int64_t L, float *__restrict__ row_mnmx, TopkMask mask) {
    extern __shared__ uint64_t lbuf[];   // kLargeTile keys (keys == nullptr), or the histogram only
    __shared__ float red_mn[TK_THREADS / 64], red_mx[TK_THREADS / 64];
    __shared__ unsigned int s_count, s_bin;
    unsigned int *hist = reinterpret_cast<unsigned int *>(lbuf);
    static_assert(TK_THREADS == 1024, "one thread per histogram bin");

    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    const float *s = scores + (size_t)row * ld;
    MaskRow mrow{nullptr, 0};
    int64_t n_sel = n;   // elements that may be selected
    if constexpr (kMasked) {
        mrow.w = mask.words + (size_t)row * (size_t)mask.ld_words;
        mrow.bit0 = mask.bit_offset;
        n_sel = mask_count(mrow, n, tid, &s_count);
    }
    const int64_t kk = (int64_t)k < n_sel ? (int64_t)k : n_sel;

    // ---- select: the exact kk-th largest key.  Invariant: count(key > hi) = above < kk <= above + count(lo <= key <= hi)
    uint64_t thresh = kMasked ? 1 : 0;
    if (kk < n_sel) {
        uint64_t lo = kMasked ? 1 : 0, hi = ~0ull;
        unsigned int above = 0;
        for (;;) {
            const uint64_t width = hi - lo;
            int shift = 0;
            while ((width >> shift) >= 1024) ++shift;   // bins 0 .. width >> shift <= 1023
            hist[tid] = 0;
            if (tid == 0) s_bin = 0;
            __syncthreads();
            for_each_key<kMasked>(s, n, tid, mrow, [&](float, uint64_t key) {
                if (key >= lo && key <= hi) atomicAdd(&hist[(unsigned int)((key - lo) >> shift)], 1u);
            });
            __syncthreads();
            for (int o = 1; o < TK_THREADS; o <<= 1) {   // hist[b] := keys in the bins >= b
                const unsigned int add = tid + o < TK_THREADS ? hist[tid + o] : 0u;
                __syncthreads();
                hist[tid] += add;
                __syncthreads();
            }
            // the counts fall with b, above + hist[0] >= kk and above < kk: exactly one bin b has
            // above + hist[b] >= kk > above + hist[b + 1]
            const bool here = above + hist[tid] >= (unsigned int)kk;
            const bool next = tid + 1 < TK_THREADS && above + hist[tid + 1] >= (unsigned int)kk;
            if (here && !next) s_bin = (unsigned int)tid;
            __syncthreads();
            const int b = (int)s_bin;
            const unsigned int c_ge = above + hist[b];
            const unsigned int c_gt = b + 1 < TK_THREADS ? above + hist[b + 1] : above;
            __syncthreads();
            const uint64_t blo = lo + ((uint64_t)b << shift);
            if (c_ge == (unsigned int)kk || shift == 0) {   // (shift 0: bins are single keys, so c_ge = c_gt + 1 = kk)
                thresh = blo;
                break;
            }
            const uint64_t span = ((uint64_t)1 << shift) - 1;
            above = c_gt;
            hi = hi - blo > span ? blo + span : hi;
            lo = blo;
        }
    }

    // ---- compact the kk keys >= thresh (LDS or the workspace row) + the row min / max
    if (tid == 0) s_count = 0;
    __syncthreads();
    uint64_t *grow = keys ? keys + (size_t)row * L : nullptr;
    float mn = INFINITY, mx = -INFINITY;
    for_each_key<kMasked>(s, n, tid, mrow, [&](float v, uint64_t key) {
        minmax_add(mn, mx, v);
        wave_append(key >= thresh, &s_count, [&](unsigned int slot) {
            if (slot < (unsigned int)kk) {
                if (grow) grow[slot] = key; else lbuf[slot] = key;
            }
        });
    });
    mn = wave_min(mn);
    mx = wave_max(mx);
    if ((tid & 63) == 0) {
        red_mn[tid >> 6] = mn;
        red_mx[tid >> 6] = mx;
    }
    __syncthreads();
    mn = red_mn[0];
    mx = red_mx[0];
    for (int w = 1; w < TK_THREADS / 64; ++w) {
        mn = fminf(mn, red_mn[w]);
        mx = fmaxf(mx, red_mx[w]);
    }
    if (tid == 0) {
        if (mn_out) mn_out[row] = mn;
        if (mx_out) mx_out[row] = mx;
    }
    if (grow) {   // sorted by large_tile_sort_kernel + large_merge_kernel; pad the row to L with the smallest key
        for (int64_t j = kk + tid; j < L; j += TK_THREADS) grow[j] = 0;
        if (tid == 0) {
            row_mnmx[2 * row] = mn;
            row_mnmx[2 * row + 1] = mx;
        }
        return;
    }
    int p2 = 2;
    while (p2 < (int)kk) p2 <<= 1;
    for (int j = (int)kk + tid; j < p2; j += TK_THREADS) lbuf[j] = 0;
    __syncthreads();
    bitonic_sort_desc(lbuf, p2, tid);
    for (int64_t j = tid; j < k; j += TK_THREADS) {
        int32_t idx = -1;
        float val = 0.f;
        if (j < kk) {
            const uint64_t key = lbuf[j];
            idx = (int32_t)(uint32_t)key + idx_offset;
            val = ordered_to_f32((uint32_t)(key >> 32));
            if (norm == kNormMinMax) val = minmax_norm(val, mn, mx);
        }
        idx_out[(size_t)row * k + j] = idx;
        val_out[(size_t)row * k + j] = val;
    }
}

// every kLargeTile run of a workspace row sorted descending in LDS; grid (L / kLargeTile, batch)
__global__ __launch_bounds__(TK_THREADS) void large_tile_sort_kernel(uint64_t *__restrict__ keys, int64_t L) {
    extern __shared__ uint64_t lbuf[];
    uint64_t *t = keys + (size_t)blockIdx.y * L + (size_t)blockIdx.x * kLargeTile;
    for (int j = threadIdx.x; j < kLargeTile; j += TK_THREADS) lbuf[j] = t[j];
    __syncthreads();
    bitonic_sort_desc(lbuf, kLargeTile, threadIdx.x);
    for (int j = threadIdx.x; j < kLargeTile; j += TK_THREADS) t[j] = lbuf[j];
}

// one merge-path pass: the sorted runs [2 p w, +w) and [2 p w + w, +w) of every row (clipped to L) become one run.
// Thread t emits the kMergeSpan outputs starting at o0 = t * kMergeSpan; its co-rank (how many come from the first run)
// is found by binary search, ties taken from the first run (only the zero padding repeats a key).
// last: write the indices / scores of the outputs o < k (and -1 / 0 for kk <= o < k) instead of keys.
// kMasked: kk is the host's min(k, n); a row with fewer allowed elements is padded with key 0, which writes -1 / 0
template <bool kMasked>
__global__ __launch_bounds__(TK_THREADS) void large_merge_kernel(
    const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, int64_t L, int64_t w, int32_t last, int32_t k,
    int64_t kk, int32_t idx_offset, int32_t norm, const float *__restrict__ row_mnmx, int32_t *__restrict__ idx_out,
    float *__restrict__ val_out) {
    const int row = blockIdx.y;
    const int64_t o0 = ((int64_t)blockIdx.x * TK_THREADS + threadIdx.x) * kMergeSpan;
    uint64_t out[kMergeSpan];
    if (o0 < L) {   // L is a multiple of kMergeSpan and of 2 w / kLargeTile: a span never straddles a run pair
        const uint64_t *r = src + (size_t)row * L;
        const int64_t base = o0 / (2 * w) * (2 * w);
        const uint64_t *A = r + base, *B = r + base + w;
        const int64_t la = L - base < w ? L - base : w;
        const int64_t lb = L - base - w <= 0 ? 0 : (L - base - w < w ? L - base - w : w);
        const int64_t d = o0 - base;
        int64_t lo = d - lb > 0 ? d - lb : 0, hi = d < la ? d : la;
        while (lo < hi) {   // smallest i with NOT (A[i] goes before B[d - i - 1])
            const int64_t i = (lo + hi) >> 1;
            if (A[i] >= B[d - i - 1]) lo = i + 1; else hi = i;
        }
        int64_t i = lo, j = d - lo;
#pragma unroll
        for (int u = 0; u < kMergeSpan; ++u) {
            if (i < la && (j >= lb || A[i] >= B[j])) out[u] = A[i++];
            else out[u] = B[j++];
        }
    }
    if (!last) {
        if (o0 < L) {
#pragma unroll
            for (int u = 0; u < kMergeSpan; ++u) dst[(size_t)row * L + o0 + u] = out[u];
        }
        return;
    }
    const float mn = row_mnmx[2 * row], mx = row_mnmx[2 * row + 1];
#pragma unroll
    for (int u = 0; u < kMergeSpan; ++u) {
        const int64_t o = o0 + u;
        if (o >= k) break;
        int32_t idx = -1;
        float val = 0.f;
        if (o < kk && (!kMasked || out[u] != 0)) {
            idx = (int32_t)(uint32_t)out[u] + idx_offset;
            val = ordered_to_f32((uint32_t)(out[u] >> 32));
            if (norm == kNormMinMax) val = minmax_norm(val, mn, mx);
        }
        idx_out[(size_t)row * k + o] = idx;
        val_out[(size_t)row * k + o] = val;
    }
}

}  // namespace

// a filter row must hold the bits [bit_offset, bit_offset + n); rows closer than that would overlap
static hrag_status check_mask(const TopkMask *m, int64_t n) {
    if (!m) return HRAG_OK;
    HRAG_REQUIRE(m->words != nullptr, "top-k filter: NULL mask");
    HRAG_REQUIRE(m->bit_offset >= 0, "top-k filter: bit offset %lld < 0", (long long)m->bit_offset);
    HRAG_REQUIRE(m->ld_words == 0 || m->ld_words >= ceil_div(m->bit_offset + n, 32),
                 "top-k filter: %lld words per row < %lld (0: one row for the batch)", (long long)m->ld_words,
                 (long long)ceil_div(m->bit_offset + n, 32));
    return HRAG_OK;
}

hrag_status launch_row_topk(const float *scores, int32_t batch, int64_t n, int64_t ld, int32_t k,
                            int32_t idx_offset, TopkNorm norm, int32_t *idx_out, float *val_out,
                            float *mn_out, float *mx_out, hipStream_t s, void *ws, size_t ws_bytes,
                            const TopkMask *mask) {
    HRAG_REQUIRE(k >= 1 && k <= kTopkMax, "top-k k=%d outside [1, %d]", k, kTopkMax);
    HRAG_REQUIRE(n >= 0 && n < (int64_t)0xffffffffll, "row length %lld not supported", (long long)n);
    HRAG_TRY(check_mask(mask, n));
    if (batch == 0) return HRAG_OK;
    // one workgroup per row leaves the chip idle for a handful of rows: split long rows
    int parts = 1;
    if (ws && batch < 64 && n >= 32768) {
        // the merge kernel bitonic-sorts parts * k keys (barrier stages ~ log^2): keep that at <= 1024 keys when k allows
        const int64_t merge_cap = k <= 512 ? 1024 : TK_CAP;
        parts = (int)std::min<int64_t>(std::min<int64_t>(merge_cap / k, ceil_div(n, 8192)), std::max(1, 256 / batch));
        parts = std::min(parts, 64);
        while (parts > 1 && (size_t)batch * parts * ((size_t)k * 8 + 8) > ws_bytes) --parts;
    }
    const TopkMask m = mask ? *mask : TopkMask{nullptr, 0, 0};
    if (parts <= 1) {
        if (mask)
            hipLaunchKernelGGL(row_topk_kernel<true>, dim3((unsigned)batch), dim3(TK_THREADS), 0, s, scores, n, ld, k,
                               idx_offset, (int32_t)norm, idx_out, val_out, mn_out, mx_out, 1, (int64_t)0, m);
        else
            hipLaunchKernelGGL(row_topk_kernel<false>, dim3((unsigned)batch), dim3(TK_THREADS), 0, s, scores, n, ld, k,
                               idx_offset, (int32_t)norm, idx_out, val_out, mn_out, mx_out, 1, (int64_t)0, m);
        HRAG_LAUNCH_CHECK();
        return HRAG_OK;
    }
    const int64_t plen = round_up(ceil_div(n, parts), 4);
    const size_t n_cand = (size_t)batch * parts * k;
    int32_t *c_idx = static_cast<int32_t *>(ws);
    float *c_val = reinterpret_cast<float *>(c_idx + n_cand);
    float *p_mn = c_val + n_cand;
    float *p_mx = p_mn + (size_t)batch * parts;
    if (mask) {
        hipLaunchKernelGGL(row_topk_kernel<true>, dim3((unsigned)(batch * parts)), dim3(TK_THREADS), 0, s, scores, n, ld,
                           k, 0, (int32_t)kNormNone, c_idx, c_val, p_mn, p_mx, parts, plen, m);
        HRAG_LAUNCH_CHECK();
        hipLaunchKernelGGL(topk_merge_kernel<true>, dim3((unsigned)batch), dim3(TK_THREADS), 0, s, c_idx, c_val, p_mn,
                           p_mx, parts, k, n, idx_offset, (int32_t)norm, idx_out, val_out, mn_out, mx_out);
    } else {
        hipLaunchKernelGGL(row_topk_kernel<false>, dim3((unsigned)(batch * parts)), dim3(TK_THREADS), 0, s, scores, n, ld,
                           k, 0, (int32_t)kNormNone, c_idx, c_val, p_mn, p_mx, parts, plen, m);
        HRAG_LAUNCH_CHECK();
        hipLaunchKernelGGL(topk_merge_kernel<false>, dim3((unsigned)batch), dim3(TK_THREADS), 0, s, c_idx, c_val, p_mn,
                           p_mx, parts, k, n, idx_offset, (int32_t)norm, idx_out, val_out, mn_out, mx_out);
    }
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

int64_t topk_large_ws_bytes(int32_t batch, int64_t n, int32_t k) {
    if (batch < 1 || n < 0 || k <= kTopkMax) return 0;
    const int64_t kk = std::min<int64_t>(k, n);
    if (kk <= kLargeTile) return 0;   // select + sort + write in one kernel, nothing leaves LDS
    const int64_t L = round_up(kk, kLargeTile);
    return 2 * (int64_t)batch * L * (int64_t)sizeof(uint64_t) + round_up((int64_t)batch * 2 * (int64_t)sizeof(float), 256);
}

hrag_status launch_row_topk_large(const float *scores, int32_t batch, int64_t n, int64_t ld, int32_t k,
                                  int32_t idx_offset, TopkNorm norm, int32_t *idx_out, float *val_out, float *mn_out,
                                  float *mx_out, hipStream_t s, void *ws, size_t ws_bytes, const TopkMask *mask) {
    HRAG_REQUIRE(k > kTopkMax, "large top-k path for k > %d only (k=%d)", kTopkMax, k);
    HRAG_REQUIRE(n >= 0 && n < (int64_t)0xffffffffll, "row length %lld not supported", (long long)n);
    HRAG_TRY(check_mask(mask, n));
    if (batch == 0) return HRAG_OK;
    const int64_t need = topk_large_ws_bytes(batch, n, k);
    HRAG_REQUIRE((int64_t)ws_bytes >= need && (need == 0 || ws != nullptr),
                 "top-k workspace too small: %lld < %lld bytes (hrag_topk_rows_workspace_bytes)", (long long)ws_bytes,
                 (long long)need);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "top-k workspace must be 8-byte aligned");
    HRAG_REQUIRE(need == 0 || batch <= 65535, "large top-k: batch %d above 65535 rows per call", batch);
    constexpr int lds_tile = kLargeTile * (int)sizeof(uint64_t);   // 128 KiB: > 64 KiB of dynamic LDS needs the opt-in
    static bool configured = false;
    if (!configured) {
        HRAG_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(large_select_kernel<false>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, lds_tile));
        HRAG_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(large_select_kernel<true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, lds_tile));
        HRAG_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(large_tile_sort_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, lds_tile));
        configured = true;
    }
    const TopkMask m = mask ? *mask : TopkMask{nullptr, 0, 0};
    auto select = mask ? large_select_kernel<true> : large_select_kernel<false>;
    if (need == 0) {
        hipLaunchKernelGGL(select, dim3((unsigned)batch), dim3(TK_THREADS), lds_tile, s, scores, n, ld, k,
                           idx_offset, (int32_t)norm, idx_out, val_out, mn_out, mx_out, nullptr, (int64_t)0, nullptr, m);
        HRAG_LAUNCH_CHECK();
        return HRAG_OK;
    }
    const int64_t kk = std::min<int64_t>(k, n);
    const int64_t L = round_up(kk, kLargeTile);
    uint64_t *ka = static_cast<uint64_t *>(ws);
    uint64_t *kb = ka + (size_t)batch * L;
    float *row_mnmx = reinterpret_cast<float *>(kb + (size_t)batch * L);
    hipLaunchKernelGGL(select, dim3((unsigned)batch), dim3(TK_THREADS), 4 * TK_THREADS, s, scores, n, ld, k,
                       idx_offset, (int32_t)norm, idx_out, val_out, mn_out, mx_out, ka, L, row_mnmx, m);
    HRAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(large_tile_sort_kernel, dim3((unsigned)(L / kLargeTile), (unsigned)batch), dim3(TK_THREADS),
                       lds_tile, s, ka, L);
    HRAG_LAUNCH_CHECK();
    const int64_t per_wg = (int64_t)TK_THREADS * kMergeSpan;
    auto merge = mask ? large_merge_kernel<true> : large_merge_kernel<false>;
    for (int64_t w = kLargeTile; w < L; w *= 2) {
        const bool last = 2 * w >= L;
        const int64_t outs = last ? std::max<int64_t>(L, k) : L;
        hipLaunchKernelGGL(merge, dim3((unsigned)ceil_div(outs, per_wg), (unsigned)batch), dim3(TK_THREADS),
                           0, s, ka, kb, L, w, (int32_t)last, k, kk, idx_offset, (int32_t)norm, row_mnmx, idx_out,
                           val_out);
        HRAG_LAUNCH_CHECK();
        std::swap(ka, kb);
    }
    return HRAG_OK;
}

hrag_status launch_masked_prior(float *scores, int32_t batch, int64_t n, int64_t ld, const TopkMask &mask, hipStream_t s) {
    HRAG_REQUIRE(n >= 0 && n < (int64_t)0xffffffffll, "row length %lld not supported", (long long)n);
    HRAG_TRY(check_mask(&mask, n));
    if (batch == 0 || n == 0) return HRAG_OK;
    hipLaunchKernelGGL(masked_prior_kernel, dim3((unsigned)batch), dim3(TK_THREADS), 0, s, scores, n, ld, mask);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status launch_masked_stats(const float *scores, int32_t batch, int64_t n, int64_t ld, const TopkMask &mask,
                                float *mn_out, float *mx_out, hipStream_t s) {
    HRAG_REQUIRE(n >= 1 && n < (int64_t)0xffffffffll, "row length %lld not supported", (long long)n);
    HRAG_TRY(check_mask(&mask, n));
    if (batch == 0) return HRAG_OK;
    hipLaunchKernelGGL(masked_rows_kernel<false>, dim3((unsigned)batch), dim3(TK_THREADS), 0, s,
                       const_cast<float *>(scores), n, ld, mask, (const float *)nullptr, (const float *)nullptr, mn_out,
                       mx_out);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status launch_masked_prior_ext(float *scores, int32_t batch, int64_t n, int64_t ld, const TopkMask &mask,
                                    const float *mn_in, const float *mx_in, float *mn_out, float *mx_out, hipStream_t s) {
    HRAG_REQUIRE(n >= 1 && n < (int64_t)0xffffffffll, "row length %lld not supported", (long long)n);
    HRAG_TRY(check_mask(&mask, n));
    if (batch == 0) return HRAG_OK;
    hipLaunchKernelGGL(masked_rows_kernel<true>, dim3((unsigned)batch), dim3(TK_THREADS), 0, s, scores, n, ld, mask,
                       mn_in, mx_in, mn_out, mx_out);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status launch_row_minmax(const float *scores, int32_t batch, int64_t n, int64_t ld,
                              float *mn_out, float *mx_out, hipStream_t s) {
    if (batch == 0) return HRAG_OK;
    hipLaunchKernelGGL(row_minmax_kernel, dim3((unsigned)batch), dim3(TK_THREADS), 0, s, scores, n, ld,
                       mn_out, mx_out);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

}  // namespace hrag
