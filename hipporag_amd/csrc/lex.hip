// Lexical retrieval (include/hrag.h, "lexical retrieval": hrag_lex_create / hrag_lex_scores / hrag_lex_blend_rows): the
// score rows [B][n_passages] of sparse queries against a sparse passage index held in inverted form (per term: the
// passages that hold it, ascending, with their weights), and the blend of such rows into dense rows.
//
// lex_scores_kernel: one 256-thread workgroup per (query, tile of HRAG_LEX_TILE consecutive passages).  The tile's fp64
// accumulators live in LDS (16 KB; with the term records 20 KB per workgroup, seven workgroups per CU).  The query's term
// list is read once: thread j takes term j (HRAG_LEX_MAX_QUERY_TERMS == the workgroup size) and cuts its posting list to
// the segment inside the tile by two binary searches (the second over at most a tile's length behind the first).  Then
// the workgroup walks the terms IN LIST ORDER: the lanes add the products of a segment into LDS -- the passages of one
// list are unique, so no two lanes meet -- and a barrier separates two non-empty segments (an empty segment costs
// nothing: its length is read from LDS by every thread alike).  The tile is rounded once and stored, one float4 per lane
// where the rows are 16-byte aligned.  No atomics, no global read-modify-write, every column written exactly once; the
// columns n .. ld are not touched.  The row min / max, where asked for, are a launch of the library's row_minmax kernel
// over the rows just written.
//
// lex_blend_kernel<W>: element-wise, one thread per W columns of one row (W = 4: float4 loads and stores).  A row whose
// lexical side has no range is copied bit for bit; out may be the dense rows themselves (an element is read and written
// by one thread).
#include "engine_impl.h"

struct hrag_lex {
    int64_t n_passages = 0, n_terms = 0, nnz = 0;
    int64_t *d_term_ptr = nullptr;   // [n_terms + 1]
    int32_t *d_doc = nullptr;        // [nnz] passage positions, ascending within a list
    float *d_w = nullptr;            // [nnz]
};

namespace hrag {
namespace {

constexpr int kLexThreads = 256;
constexpr int kLexPer = HRAG_LEX_TILE / kLexThreads;    // accumulators per thread
static_assert(kLexPer * kLexThreads == HRAG_LEX_TILE && kLexPer % 4 == 0, "a thread stores whole float4 groups");
static_assert(HRAG_LEX_MAX_QUERY_TERMS == kLexThreads, "thread j cuts the posting list of term j");
static_assert(HRAG_LEX_MAX_QUERY_TERMS >= 64, "the cap of include/hrag.h");

__device__ __forceinline__ float round_once(double a) {
    const float f = (float)a;
    return f != f ? __uint_as_float(0x7fc00000u) : f;
}

// first position in [lo, hi) whose passage is >= bound (the list is ascending)
__device__ __forceinline__ int64_t lower_bound_doc(const int32_t *__restrict__ doc, int64_t lo, int64_t hi, int64_t bound) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)doc[mid] < bound) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kLexThreads) void lex_scores_kernel(const int64_t *__restrict__ term_ptr,
                                                                 const int32_t *__restrict__ post_doc,
                                                                 const float *__restrict__ post_w, int64_t n_terms,
                                                                 int64_t n, const int32_t *__restrict__ q_ptr,
                                                                 const int32_t *__restrict__ q_term,
                                                                 const float *__restrict__ q_weight, int64_t q_nnz,
                                                                 float *__restrict__ out, int64_t ld, int32_t n_tiles,
                                                                 int32_t vec) {
    __shared__ __attribute__((aligned(16))) double acc[HRAG_LEX_TILE];
    __shared__ int64_t s_lo[HRAG_LEX_MAX_QUERY_TERMS];
    __shared__ int32_t s_len[HRAG_LEX_MAX_QUERY_TERMS];
    __shared__ float s_w[HRAG_LEX_MAX_QUERY_TERMS];

    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x / n_tiles;
    const int64_t tile0 = ((int64_t)blockIdx.x % n_tiles) * HRAG_LEX_TILE;
    const int32_t tile_n = (int32_t)(n - tile0 < HRAG_LEX_TILE ? n - tile0 : HRAG_LEX_TILE);

#pragma unroll
    for (int u = 0; u < kLexPer; ++u) acc[tid + kLexThreads * u] = 0.0;

    // the term list: whatever q_ptr holds, only q_term / q_weight [0, q_nnz) are read, and at most the cap
    int64_t beg = q_ptr[b], end = q_ptr[b + 1];
    beg = beg < 0 ? 0 : beg > q_nnz ? q_nnz : beg;
    end = end < beg ? beg : end > q_nnz ? q_nnz : end;
    const int32_t nq = (int32_t)(end - beg < HRAG_LEX_MAX_QUERY_TERMS ? end - beg : HRAG_LEX_MAX_QUERY_TERMS);
    if (tid < nq) {
        const int32_t t = q_term[beg + tid];
        int64_t lo = 0;
        int32_t len = 0;
        if (t >= 0 && (int64_t)t < n_terms) {
            const int64_t a = term_ptr[t], e = term_ptr[t + 1];
            lo = lower_bound_doc(post_doc, a, e, tile0);
            const int64_t cap = lo + tile_n < e ? lo + tile_n : e;      // a tile holds at most tile_n entries of a list
            len = (int32_t)(lower_bound_doc(post_doc, lo, cap, tile0 + tile_n) - lo);
        }
        s_lo[tid] = lo;
        s_len[tid] = len;
        s_w[tid] = q_weight[beg + tid];
    }
    __syncthreads();

    bool written = false;
    for (int32_t j = 0; j < nq; ++j) {
        const int32_t len = s_len[j];       // the same value in every thread: the barrier below is uniform
        if (len == 0) continue;
        if (written) __syncthreads();       // the adds of the previous non-empty segment
        written = true;
        const int64_t lo = s_lo[j];
        const double w = (double)s_w[j];
        for (int32_t i = tid; i < len; i += kLexThreads) {
            const int64_t p = (int64_t)post_doc[lo + i] - tile0;
            if (p >= 0 && p < tile_n) acc[p] += w * (double)post_w[lo + i];     // exact product, one fp64 add
        }
    }
    __syncthreads();

    float *row = out + (size_t)b * ld + tile0;
#pragma unroll
    for (int u = 0; u < kLexPer / 4; ++u) {
        const int c = (tid + kLexThreads * u) * 4;
        if (c >= tile_n) continue;
        const float v0 = round_once(acc[c]), v1 = round_once(acc[c + 1]), v2 = round_once(acc[c + 2]),
                    v3 = round_once(acc[c + 3]);
        if (vec && c + 3 < tile_n) {
            *reinterpret_cast<float4 *>(row + c) = make_float4(v0, v1, v2, v3);
        } else {
            row[c] = v0;
            if (c + 1 < tile_n) row[c + 1] = v1;
            if (c + 2 < tile_n) row[c + 2] = v2;
            if (c + 3 < tile_n) row[c + 3] = v3;
        }
    }
}

// min-max of one element as every kernel of the library forms it (common.h prior_entry): a zero range gives 1
__device__ __forceinline__ float minmax_norm(float s, float mn, float range) {
    return range == 0.f ? 1.f : __fdiv_rn(s - mn, range);
}

template <int W>
__global__ __launch_bounds__(256) void lex_blend_kernel(const float *dense, int64_t ld_d, const float *__restrict__ lex,
                                                        int64_t ld_l, int64_t n, const float *__restrict__ mn_d,
                                                        const float *__restrict__ mx_d, const float *__restrict__ mn_l,
                                                        const float *__restrict__ mx_l, float alpha, float *out,
                                                        int64_t ld_o) {
    const int64_t b = blockIdx.y;
    const int64_t col = ((int64_t)blockIdx.x * 256 + threadIdx.x) * W;
    if (col >= n) return;
    const float lmn = mn_l[b], lmx = mx_l[b];
    const bool blend = alpha != 0.f && lmx > lmn;       // false: no range, or no number in the lexical row (+inf / -inf)
    const float *drow = dense + (size_t)b * ld_d + col;
    float *orow = out + (size_t)b * ld_o + col;
    if (!blend) {
        if (orow == drow) return;
        if (W == 4 && col + 4 <= n) {
            *reinterpret_cast<float4 *>(orow) = *reinterpret_cast<const float4 *>(drow);
        } else {
            for (int i = 0; i < W && col + i < n; ++i) orow[i] = drow[i];
        }
        return;
    }
    const float dmn = mn_d[b], rd = mx_d[b] - dmn, rl = lmx - lmn;
    const double a1 = (double)(1.0f - alpha), a2 = (double)alpha;
    const float *lrow = lex + (size_t)b * ld_l + col;
    float d[W], l[W], o[W];
    const bool whole = W == 1 || col + W <= n;
    if (W == 4 && whole) {
        const float4 x = *reinterpret_cast<const float4 *>(drow), y = *reinterpret_cast<const float4 *>(lrow);
        __builtin_memcpy(d, &x, sizeof(x));
        __builtin_memcpy(l, &y, sizeof(y));
    } else {
        for (int i = 0; i < W; ++i) {
            d[i] = col + i < n ? drow[i] : 0.f;
            l[i] = col + i < n ? lrow[i] : 0.f;
        }
    }
#pragma unroll
    for (int i = 0; i < W; ++i) {
        // both products are exact in fp64: one fp64 add, one rounding
        const float f = (float)(a1 * (double)minmax_norm(d[i], dmn, rd) + a2 * (double)minmax_norm(l[i], lmn, rl));
        o[i] = f != f ? __uint_as_float(0x7fc00000u) : f;
    }
    if (W == 4 && whole) {
        float4 v;
        __builtin_memcpy(&v, o, sizeof(v));
        *reinterpret_cast<float4 *>(orow) = v;
    } else {
        for (int i = 0; i < W && col + i < n; ++i) orow[i] = o[i];
    }
}

void lex_free(hrag_lex *x) {
    if (!x) return;
    if (x->d_term_ptr) (void)hipFree(x->d_term_ptr);
    if (x->d_doc) (void)hipFree(x->d_doc);
    if (x->d_w) (void)hipFree(x->d_w);
    delete x;
}

// the host rules of hrag_lex_create; nothing is allocated before they all hold
hrag_status lex_validate(int64_t n_passages, int64_t n_terms, const int64_t *term_ptr, const int32_t *post_doc,
                         const float *post_w) {
    HRAG_REQUIRE(n_passages >= 1 && n_passages < ((int64_t)1 << 31), "n_passages=%lld outside [1, 2^31)", (long long)n_passages);
    HRAG_REQUIRE(n_terms >= 0 && n_terms < ((int64_t)1 << 31), "n_terms=%lld outside [0, 2^31)", (long long)n_terms);
    HRAG_REQUIRE(term_ptr != nullptr, "term_ptr is NULL");
    HRAG_REQUIRE(term_ptr[0] == 0, "term_ptr[0] = %lld, 0 expected", (long long)term_ptr[0]);
    for (int64_t t = 0; t < n_terms; ++t)
        HRAG_REQUIRE(term_ptr[t + 1] >= term_ptr[t], "term_ptr decreases at term %lld (%lld -> %lld)", (long long)t,
                     (long long)term_ptr[t], (long long)term_ptr[t + 1]);
    const int64_t nnz = term_ptr[n_terms];
    HRAG_REQUIRE(nnz == 0 || (post_doc && post_w), "post_doc / post_w are NULL with %lld postings", (long long)nnz);
    for (int64_t t = 0; t < n_terms; ++t) {
        for (int64_t i = term_ptr[t]; i < term_ptr[t + 1]; ++i) {
            HRAG_REQUIRE(post_doc[i] >= 0 && (int64_t)post_doc[i] < n_passages,
                         "posting %lld of term %lld names passage %d outside [0, %lld)", (long long)i, (long long)t,
                         post_doc[i], (long long)n_passages);
            HRAG_REQUIRE(i == term_ptr[t] || post_doc[i] > post_doc[i - 1],
                         "the postings of term %lld are not strictly ascending at posting %lld (%d after %d)", (long long)t,
                         (long long)i, post_doc[i], post_doc[i - 1]);
            HRAG_REQUIRE(std::isfinite(post_w[i]), "posting %lld of term %lld has a weight that is not finite", (long long)i,
                         (long long)t);
        }
    }
    return HRAG_OK;
}

}  // namespace
}  // namespace hrag

using namespace hrag;

// ---- exports (include/hrag.h, lexical retrieval)
hrag_status hrag_lex_create(int64_t n_passages, int64_t n_terms, const int64_t *term_ptr, const int32_t *post_doc,
                            const float *post_w, hrag_lex **out) {
    HRAG_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    HRAG_TRY(lex_validate(n_passages, n_terms, term_ptr, post_doc, post_w));
    hrag_lex *x = new (std::nothrow) hrag_lex();
    if (!x) { set_error("out of host memory"); return HRAG_ENOMEM; }
    x->n_passages = n_passages;
    x->n_terms = n_terms;
    x->nnz = term_ptr[n_terms];
    hrag_status st = dev_upload(&x->d_term_ptr, term_ptr, n_terms + 1);
    if (st == HRAG_OK) st = dev_upload(&x->d_doc, post_doc, x->nnz);
    if (st == HRAG_OK) st = dev_upload(&x->d_w, post_w, x->nnz);
    if (st != HRAG_OK) {
        lex_free(x);
        return st;
    }
    *out = x;
    return HRAG_OK;
}

hrag_status hrag_lex_destroy(hrag_lex *lex) {
    lex_free(lex);
    return HRAG_OK;
}

hrag_status hrag_lex_scores(const hrag_lex *lex, const int32_t *q_ptr_dev, const int32_t *q_term_dev,
                            const float *q_weight_dev, int64_t q_nnz, int32_t batch, float *out_dev, int64_t ld,
                            float *min_out_dev, float *max_out_dev, hrag_stream stream) {
    HRAG_REQUIRE(lex != nullptr, "the lexical index is NULL");
    HRAG_REQUIRE(q_ptr_dev && out_dev, "NULL argument");
    HRAG_REQUIRE(q_nnz >= 0 && q_nnz < ((int64_t)1 << 31), "q_nnz=%lld outside [0, 2^31)", (long long)q_nnz);
    HRAG_REQUIRE(q_nnz == 0 || (q_term_dev && q_weight_dev), "q_term / q_weight are NULL with q_nnz=%lld", (long long)q_nnz);
    HRAG_REQUIRE(batch >= 1, "batch=%d: at least 1", batch);
    HRAG_REQUIRE(ld >= lex->n_passages, "ld=%lld below n_passages=%lld", (long long)ld, (long long)lex->n_passages);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(out_dev) & 3) == 0, "the output must be 4-byte aligned");
    HRAG_REQUIRE((min_out_dev == nullptr) == (max_out_dev == nullptr), "min_out_dev and max_out_dev: both or neither");
    const int64_t n_tiles = ceil_div(lex->n_passages, HRAG_LEX_TILE);
    const int64_t grid = (int64_t)batch * n_tiles;
    HRAG_REQUIRE(grid < ((int64_t)1 << 31), "batch=%d x %lld tiles exceeds one launch", batch, (long long)n_tiles);
    hipStream_t s = (hipStream_t)stream;
    const int32_t vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0;
    hipLaunchKernelGGL(lex_scores_kernel, dim3((unsigned)grid), dim3(kLexThreads), 0, s, lex->d_term_ptr, lex->d_doc, lex->d_w,
                       lex->n_terms, lex->n_passages, q_ptr_dev, q_term_dev, q_weight_dev, q_nnz, out_dev, ld,
                       (int32_t)n_tiles, vec);
    HRAG_LAUNCH_CHECK();
    if (min_out_dev) return launch_row_minmax(out_dev, batch, lex->n_passages, ld, min_out_dev, max_out_dev, s);
    return HRAG_OK;
}

hrag_status hrag_lex_blend_rows(const float *dense_dev, int64_t ld_d, const float *lex_dev, int64_t ld_l, int32_t batch,
                                int64_t n, const float *mn_d_dev, const float *mx_d_dev, const float *mn_l_dev,
                                const float *mx_l_dev, float alpha, float *out_dev, int64_t ld_o, hrag_stream stream) {
    HRAG_REQUIRE(dense_dev && lex_dev && out_dev && mn_d_dev && mx_d_dev && mn_l_dev && mx_l_dev, "NULL argument");
    HRAG_REQUIRE(alpha >= 0.f && alpha <= 1.f, "alpha=%g outside [0, 1]", (double)alpha);     // (false for NaN)
    HRAG_REQUIRE(batch >= 1 && batch <= 65535, "batch=%d outside [1, 65535]", batch);
    HRAG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "n=%lld outside [1, 2^31)", (long long)n);
    HRAG_REQUIRE(ld_d >= n && ld_l >= n && ld_o >= n, "ld_d=%lld / ld_l=%lld / ld_o=%lld below n=%lld", (long long)ld_d,
                 (long long)ld_l, (long long)ld_o, (long long)n);
    HRAG_REQUIRE(out_dev != dense_dev || ld_o == ld_d, "out aliases dense with another row stride (%lld vs %lld)",
                 (long long)ld_o, (long long)ld_d);
    HRAG_REQUIRE(((reinterpret_cast<uintptr_t>(dense_dev) | reinterpret_cast<uintptr_t>(lex_dev) |
                   reinterpret_cast<uintptr_t>(out_dev)) & 3) == 0, "score rows must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = ((ld_d | ld_l | ld_o) & 3) == 0 &&
                     ((reinterpret_cast<uintptr_t>(dense_dev) | reinterpret_cast<uintptr_t>(lex_dev) |
                       reinterpret_cast<uintptr_t>(out_dev)) & 15) == 0;
    const dim3 grid((unsigned)ceil_div(vec ? ceil_div(n, 4) : n, 256), (unsigned)batch);
    if (vec)
        hipLaunchKernelGGL(lex_blend_kernel<4>, grid, dim3(256), 0, s, dense_dev, ld_d, lex_dev, ld_l, n, mn_d_dev, mx_d_dev,
                           mn_l_dev, mx_l_dev, alpha, out_dev, ld_o);
    else
        hipLaunchKernelGGL(lex_blend_kernel<1>, grid, dim3(256), 0, s, dense_dev, ld_d, lex_dev, ld_l, n, mn_d_dev, mx_d_dev,
                           mn_l_dev, mx_l_dev, alpha, out_dev, ld_o);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}
