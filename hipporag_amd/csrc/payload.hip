// Payload filters (include/hrag.h, "payload filters": hrag_payload_create / hrag_payload_filter / hrag_bitset_count_rows):
// typed per-passage columns on the device and the evaluation of a small per-query clause program over them straight into
// the packed words of a doc filter.
//
// payload_filter_kernel: one 256-thread workgroup per (query, tile of HRAG_PAY_TILE consecutive passages).  The query's
// clause records -- at most HRAG_PAY_MAX_CLAUSES, with the column pointers they name already resolved from the handle's
// device table -- are staged once in LDS (3.5 KB).  A clause that is ill-formed is staged as DEAD (it hits nothing).  The
// staging and the evaluation of a clause are payload_clause.h's: boost.hip evaluates the same clauses with the same code.
// The clause loop is uniform over the workgroup; thread t evaluates the passages tile0 + 256 u + t, u = 0 .. 7: coalesced
// 8-byte column reads, a presence word shared by 32 lanes.  The verdicts of a wavefront are packed by the 64-bit wave ballot --
// lanes past n_passages stay in it with a false predicate, which is what zeroes the tail bits -- into 64 words in LDS, and
// the first 64 threads store the tile's words, the words below W only.  No atomics, no global read-modify-write, every
// output word written exactly once; the words W .. ld_o of a row are not touched.
//
// bitset_count_kernel: one workgroup per row, the popcounts of its words (the last one cut to n bits) summed per thread,
// per wavefront, then over the four wavefronts in LDS.  No atomics.
#include "payload_clause.h"

namespace hrag {
namespace {

constexpr int kPayThreads = 256;
constexpr int kPayPer = HRAG_PAY_TILE / kPayThreads;       // passages per thread
constexpr int kPayTileWords = HRAG_PAY_TILE / 32;
static_assert(kPayPer * kPayThreads == HRAG_PAY_TILE && kPayPer == 8, "a thread keeps its verdicts in 8-bit masks");
static_assert(kPayTileWords == 64 && kPayTileWords <= kPayThreads, "the first 64 threads store the tile's words");
static_assert(HRAG_PAY_MAX_CLAUSES <= kPayThreads, "thread j stages clause j");

__global__ __launch_bounds__(kPayThreads) void payload_filter_kernel(
    const PayCol *__restrict__ cols, int32_t n_cols, int64_t n, const int32_t *__restrict__ f_ptr,
    const int32_t *__restrict__ c_col, const int32_t *__restrict__ c_op, const int64_t *__restrict__ c_lo,
    const int64_t *__restrict__ c_hi, const int32_t *__restrict__ c_set_ptr, const int64_t *__restrict__ set_vals,
    int64_t n_clauses, int64_t set_nnz, const uint32_t *__restrict__ and_words, int64_t ld_a, uint32_t *__restrict__ out,
    int64_t ld_o, int64_t W, int32_t n_tiles) {
    __shared__ PayClause s_cl[HRAG_PAY_MAX_CLAUSES];
    __shared__ uint32_t s_words[kPayTileWords];

    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x / n_tiles;
    const int64_t tile0 = ((int64_t)blockIdx.x % n_tiles) * HRAG_PAY_TILE;

    // the clause list: whatever f_ptr holds, only clauses [0, n_clauses) are read, and at most the cap
    int32_t nc = 0;
    if (n_clauses > 0) {
        int64_t beg = f_ptr[b], end = f_ptr[b + 1];
        beg = beg < 0 ? 0 : beg > n_clauses ? n_clauses : beg;
        end = end < beg ? beg : end > n_clauses ? n_clauses : end;
        nc = (int32_t)(end - beg < HRAG_PAY_MAX_CLAUSES ? end - beg : HRAG_PAY_MAX_CLAUSES);
        if (tid < nc) s_cl[tid] = stage_clause(cols, n_cols, c_col, c_op, c_lo, c_hi, c_set_ptr, set_nnz, beg + tid);
    }
    __syncthreads();

    // bit u of a mask: the passage tile0 + 256 u + tid
    uint32_t inb = 0;
#pragma unroll
    for (int u = 0; u < kPayPer; ++u) inb |= (uint32_t)(tile0 + kPayThreads * u + tid < n) << u;
    uint32_t pass = clauses_pass(s_cl, nc, set_vals, tile0, tid, inb);

    if (and_words) {
        const uint32_t *row = and_words + (size_t)b * ld_a;      // ld_a 0: one row for the batch
#pragma unroll
        for (int u = 0; u < kPayPer; ++u) {
            if (!((pass >> u) & 1u)) continue;                   // (in bounds: pass is a subset of inb)
            const int64_t p = tile0 + kPayThreads * u + tid;
            if (!((row[p >> 5] >> (p & 31)) & 1u)) pass &= ~(1u << u);
        }
    }

    // every lane votes, the ones past n_passages with false: the tail bits of the last word are 0
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int u = 0; u < kPayPer; ++u) {
        const unsigned long long m = __ballot((pass >> u) & 1u);
        if (lane == 0) {
            s_words[u * 8 + wave * 2] = (uint32_t)m;
            s_words[u * 8 + wave * 2 + 1] = (uint32_t)(m >> 32);
        }
    }
    __syncthreads();
    if (tid < kPayTileWords) {
        const int64_t w = tile0 / 32 + tid;
        if (w < W) out[(size_t)b * ld_o + w] = s_words[tid];
    }
}

__global__ __launch_bounds__(256) void bitset_count_kernel(const uint32_t *__restrict__ words, int64_t ld, int64_t n,
                                                           int64_t W, int32_t *__restrict__ count_out) {
    __shared__ int32_t s_part[4];
    const int tid = threadIdx.x;
    const uint32_t *row = words + (size_t)blockIdx.x * ld;
    const uint32_t last = (n & 31) ? (0xffffffffu >> (32 - (n & 31))) : 0xffffffffu;
    int32_t c = 0;
    for (int64_t w = tid; w < W; w += 256) c += __popc(w == W - 1 ? row[w] & last : row[w]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((tid & 63) == 0) s_part[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) count_out[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

void payload_free(hrag_payload *x) {
    if (!x) return;
    for (void *p : x->owned)
        if (p) (void)hipFree(p);
    delete x;
}

// the host rules of hrag_payload_create; nothing is allocated before they all hold
hrag_status payload_validate(int64_t n_passages, int32_t n_cols, const int32_t *col_type, const void *const *col_values) {
    HRAG_REQUIRE(n_passages >= 1 && n_passages < ((int64_t)1 << 31), "n_passages=%lld outside [1, 2^31)", (long long)n_passages);
    HRAG_REQUIRE(n_cols >= 0 && n_cols <= HRAG_PAY_MAX_COLS, "n_cols=%d outside [0, %d]", n_cols, HRAG_PAY_MAX_COLS);
    HRAG_REQUIRE(n_cols == 0 || (col_type && col_values), "col_type / col_values are NULL with %d columns", n_cols);
    for (int32_t c = 0; c < n_cols; ++c) {
        HRAG_REQUIRE(col_type[c] == HRAG_PAY_I64 || col_type[c] == HRAG_PAY_F64, "column %d has the unknown type %d", c, col_type[c]);
        HRAG_REQUIRE(col_values[c] != nullptr, "the values of column %d are NULL", c);
    }
    return HRAG_OK;
}

}  // namespace
}  // namespace hrag

using namespace hrag;

// ---- exports (include/hrag.h, payload filters)
hrag_status hrag_payload_create(int64_t n_passages, int32_t n_cols, const int32_t *col_type, const void *const *col_values,
                                const uint32_t *const *col_present, hrag_payload **out) {
    HRAG_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    HRAG_TRY(payload_validate(n_passages, n_cols, col_type, col_values));
    hrag_payload *x = new (std::nothrow) hrag_payload();
    if (!x) { set_error("out of host memory"); return HRAG_ENOMEM; }
    x->n_passages = n_passages;
    x->n_cols = n_cols;
    x->col_type.assign(col_type, col_type + n_cols);
    const int64_t words = ceil_div(n_passages, 32);
    std::vector<PayCol> table((size_t)n_cols);
    hrag_status st = HRAG_OK;
    for (int32_t c = 0; c < n_cols && st == HRAG_OK; ++c) {
        int64_t *d_v = nullptr;
        uint32_t *d_p = nullptr;
        st = dev_upload(&d_v, static_cast<const int64_t *>(col_values[c]), n_passages);
        x->owned.push_back(d_v);
        if (st == HRAG_OK && col_present && col_present[c]) {
            st = dev_upload(&d_p, col_present[c], words);
            x->owned.push_back(d_p);
        }
        table[(size_t)c] = PayCol{d_v, d_p, col_type[c], 0};
    }
    if (st == HRAG_OK && n_cols > 0) {
        st = dev_upload(&x->d_cols, table.data(), (int64_t)n_cols);
        x->owned.push_back(x->d_cols);
    }
    if (st != HRAG_OK) {
        payload_free(x);
        return st;
    }
    *out = x;
    return HRAG_OK;
}

hrag_status hrag_payload_destroy(hrag_payload *pay) {
    payload_free(pay);
    return HRAG_OK;
}

hrag_status hrag_payload_filter(const hrag_payload *pay, const int32_t *f_ptr_dev, const int32_t *c_col_dev,
                                const int32_t *c_op_dev, const int64_t *c_lo_dev, const int64_t *c_hi_dev,
                                const int32_t *c_set_ptr_dev, const int64_t *set_vals_dev, int64_t n_clauses, int64_t set_nnz,
                                int32_t batch, const uint32_t *and_words_dev, int64_t ld_a, uint32_t *out_words_dev,
                                int64_t ld_o, hrag_stream stream) {
    HRAG_REQUIRE(pay != nullptr, "the payload index is NULL");
    HRAG_REQUIRE(out_words_dev != nullptr, "out_words_dev is NULL");
    HRAG_REQUIRE(batch >= 1 && batch <= 65535, "batch=%d outside [1, 65535]", batch);
    HRAG_REQUIRE(n_clauses >= 0 && n_clauses < ((int64_t)1 << 31), "n_clauses=%lld outside [0, 2^31)", (long long)n_clauses);
    HRAG_REQUIRE(set_nnz >= 0 && set_nnz < ((int64_t)1 << 31), "set_nnz=%lld outside [0, 2^31)", (long long)set_nnz);
    HRAG_REQUIRE(n_clauses == 0 || (f_ptr_dev && c_col_dev && c_op_dev && c_lo_dev && c_hi_dev && c_set_ptr_dev),
                 "a clause array is NULL with n_clauses=%lld", (long long)n_clauses);
    HRAG_REQUIRE(set_nnz == 0 || set_vals_dev, "set_vals_dev is NULL with set_nnz=%lld", (long long)set_nnz);
    const int64_t W = ceil_div(pay->n_passages, 32);
    HRAG_REQUIRE(ld_o >= W, "ld_o=%lld below ceil(n_passages / 32) = %lld", (long long)ld_o, (long long)W);
    HRAG_REQUIRE(and_words_dev == nullptr || ld_a == 0 || ld_a >= W,
                 "ld_a=%lld: 0 (one row for the batch) or >= ceil(n_passages / 32) = %lld", (long long)ld_a, (long long)W);
    HRAG_REQUIRE(((reinterpret_cast<uintptr_t>(out_words_dev) | reinterpret_cast<uintptr_t>(and_words_dev)) & 3) == 0,
                 "the word rows must be 4-byte aligned");
    const int64_t n_tiles = ceil_div(pay->n_passages, HRAG_PAY_TILE);
    const int64_t grid = (int64_t)batch * n_tiles;
    HRAG_REQUIRE(grid < ((int64_t)1 << 31), "batch=%d x %lld tiles exceeds one launch", batch, (long long)n_tiles);
    hipLaunchKernelGGL(payload_filter_kernel, dim3((unsigned)grid), dim3(kPayThreads), 0, (hipStream_t)stream, pay->d_cols,
                       pay->n_cols, pay->n_passages, f_ptr_dev, c_col_dev, c_op_dev, c_lo_dev, c_hi_dev, c_set_ptr_dev,
                       set_vals_dev, n_clauses, set_nnz, and_words_dev, and_words_dev ? ld_a : 0, out_words_dev, ld_o, W,
                       (int32_t)n_tiles);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status hrag_bitset_count_rows(const uint32_t *words_dev, int64_t ld, int64_t n, int32_t batch, int32_t *count_out_dev,
                                   hrag_stream stream) {
    HRAG_REQUIRE(words_dev && count_out_dev, "NULL argument");
    HRAG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "n=%lld outside [1, 2^31)", (long long)n);
    HRAG_REQUIRE(batch >= 1, "batch=%d: at least 1", batch);
    const int64_t W = ceil_div(n, 32);
    HRAG_REQUIRE(ld == 0 || ld >= W, "ld=%lld: 0 (one row for the batch) or >= ceil(n / 32) = %lld", (long long)ld, (long long)W);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(words_dev) & 3) == 0, "the word rows must be 4-byte aligned");
    hipLaunchKernelGGL(bitset_count_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, words_dev, ld, n, W,
                       count_out_dev);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}
