// Late-interaction reranking (include/hrag.h, "late-interaction reranking": hrag_late_create / hrag_late_scores /
// hrag_late_rank_rows / hrag_late_rerank): ColBERT-style MaxSim of a query's token vectors over the token vectors of the
// c <= 1024 candidates a ranking returned, per query, without leaving the device.
//
// late_maxsim_kernel<F16>: one 256-thread workgroup per (query, candidate slot).  The query's tokens are staged once in
// LDS as the B operand (column = query token; rows padded by 16 bytes as sim_gemm.hip pads them, k zero-filled to a
// multiple of 32, tokens zero-filled to a multiple of 16).  The passage's token rows are the A operand: 16 rows per
// wavefront, 64 per workgroup step, read by 16-byte loads straight from tok_emb in the fragment layout of
// v_mfma_f32_16x16x32 (lane l holds row l & 15, k = 8 (l >> 4) + j of each 32-wide k step) -- no gathered copy in memory;
// all loads of a lane's row are issued before the step's first MFMA.  One accumulator per 16 query tokens; C/D
// layout col = lane & 15 (query token), row = 4 (lane >> 4) + reg (passage token).  A row at or beyond the passage's last
// token is never loaded and enters the maximum as -inf (NOT as a zero row: a zero row wins whenever every real product
// is negative); a column at or beyond the query's last token is never summed.  The step epilogue takes fmaxf over the
// lane's four rows into a running maximum in registers; after the last step the maxima meet across the four lane groups
// by shuffles and across the four wavefronts once in LDS, and wavefront 0 forms the fp64 sum in ascending token order.
// No atomics, every output written exactly once, nothing read back: the bits of a (query, passage) pair do not depend on
// the batch, the slot or the neighbours.
//
// late_rank_kernel: one 256-thread workgroup per query; keys ordered(score) << 32 | ~slot of the live slots (common.h
// rank_key: NaN above +inf, -0 ties +0, a tie to the SMALLER slot as in mmr_select_kernel), 0 for an empty slot; an LDS
// bitonic sort over the next power of two >= c <= 1024 keys, descending; the first k written with plain vector stores.
#include "engine_impl.h"

struct hrag_late {
    int64_t n_passages = 0, n_tokens = 0;
    int32_t dim = 0, dtype = HRAG_BF16;
    int64_t *d_tok_ptr = nullptr;        // [n_passages + 1], owned
    const uint16_t *tok_emb = nullptr;   // [n_tokens, dim] on the device, the caller's
};

namespace hrag {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

template <bool F16>
__device__ __forceinline__ f32x4 mfma32(const uint4 &ua, const uint4 &ub, f32x4 acc) {
    if constexpr (F16) {
        f16x8 a, b;
        __builtin_memcpy(&a, &ua, 16);
        __builtin_memcpy(&b, &ub, 16);
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
    } else {
        bf16x8 a, b;
        __builtin_memcpy(&a, &ua, 16);
        __builtin_memcpy(&b, &ub, 16);
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
}

constexpr int kLateThreads = 256;
constexpr int kQTiles = HRAG_LATE_MAX_QUERY_TOKENS / 16;   // accumulators: one per 16 query tokens
constexpr int kKSteps = HRAG_LATE_MAX_DIM / 32;            // 32-wide k steps of the longest row
constexpr int kRowsPerStep = 64;                           // passage tokens per workgroup step (16 per wavefront)
constexpr int kQPad = 8;                                   // 16-bit elements of padding per LDS row (sim_gemm.hip)
static_assert(kQTiles * 16 == HRAG_LATE_MAX_QUERY_TOKENS && kKSteps * 32 == HRAG_LATE_MAX_DIM, "tile counts");

__device__ __forceinline__ float canonical(float v) { return v != v ? __uint_as_float(0x7fc00000u) : v + 0.0f; }

// (four waves per SIMD, at most 128 VGPRs: the loads of a step are not overlapped with its own MFMAs but with the steps of
// the three other workgroups resident on the CU)
template <bool F16>
__global__ __launch_bounds__(kLateThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void late_maxsim_kernel(const uint16_t *__restrict__ tok_emb,
                                                                   const int64_t *__restrict__ tok_ptr, int64_t n,
                                                                   int32_t dim, const int32_t *__restrict__ q_ptr,
                                                                   const uint16_t *__restrict__ q_tok, int64_t q_total,
                                                                   int32_t nq_cap, const int32_t *__restrict__ cand, int32_t c,
                                                                   float *__restrict__ out, int64_t ld) {
    extern __shared__ __attribute__((aligned(16))) uint16_t qs[];   // [16 * nt][dimp + kQPad]
    __shared__ float red[4][HRAG_LATE_MAX_QUERY_TOKENS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = (int64_t)blockIdx.x / c;
    const int slot = (int)((int64_t)blockIdx.x % c);
    float *dst = out + (size_t)b * ld + slot;

    // everything below up to the staging loop is uniform over the workgroup: an early return leaves no barrier behind
    const int32_t p = cand[(size_t)b * c + slot];
    if (p < 0 || (int64_t)p >= n) {          // an empty slot has no score
        if (tid == 0) *dst = 0.0f;
        return;
    }
    // (the host checked q_ptr; the clamps keep a device-side q_ptr that disagrees with it inside q_tok)
    int64_t q0 = q_ptr[b], q1 = q_ptr[b + 1];
    q0 = q0 < 0 ? 0 : q0 > q_total ? q_total : q0;
    q1 = q1 < q0 ? q0 : q1 > q_total ? q_total : q1;
    const int nq = (int)(q1 - q0 > nq_cap ? nq_cap : q1 - q0);       // nq_cap: the longest query the host saw, what LDS holds
    if (nq == 0) {                           // a query without tokens: the empty sum
        if (tid == 0) *dst = 0.0f;
        return;
    }
    const int64_t t0 = tok_ptr[p];
    const int64_t len = tok_ptr[p + 1] - t0;
    if (len <= 0) {                          // a passage without tokens: every m_i stays -inf
        if (tid == 0) *dst = -INFINITY;
        return;
    }

    const int nt = (nq + 15) >> 4;           // 16-token tiles of the query
    const int dimp = (dim + 31) & ~31;       // k, zero-filled to whole MFMA steps
    const int nks = dimp >> 5;
    const int ldq = dimp + kQPad;
    {
        const int chunks = dimp >> 3, total = nt * 16 * chunks;
        for (int i = tid; i < total; i += kLateThreads) {
            const int r = i / chunks, ch = i - r * chunks;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r < nq && ch * 8 < dim) v = *reinterpret_cast<const uint4 *>(q_tok + (size_t)(q0 + r) * dim + ch * 8);
            *reinterpret_cast<uint4 *>(&qs[r * ldq + ch * 8]) = v;
        }
    }
    __syncthreads();

    const int frow = lane & 15, koff = 8 * (lane >> 4);
    const int64_t wrow = wave * 16;          // this wavefront's 16 rows of a step
    const uint16_t *base = tok_emb + (size_t)t0 * dim + koff;

    // the lane's 8 k-chunks of passage token `row` (zeros beyond the passage's last token and beyond dim: neither is read)
    auto load_row = [&](int64_t row, uint4 (&a)[kKSteps]) {
        const bool valid = row < len;
        const uint16_t *src = base + (size_t)(valid ? row : 0) * dim;
#pragma unroll
        for (int ks = 0; ks < kKSteps; ++ks) {
            a[ks] = make_uint4(0, 0, 0, 0);
            if (valid && ks * 32 + koff < dim) a[ks] = *reinterpret_cast<const uint4 *>(src + ks * 32);
        }
    };

    float m[kQTiles];
#pragma unroll
    for (int t = 0; t < kQTiles; ++t) m[t] = -INFINITY;

    for (int64_t r0 = 0; r0 < len; r0 += kRowsPerStep) {
        if (r0 + wrow < len) {               // (uniform over the wavefront) it holds at least one real row
            uint4 a_cur[kKSteps];
            load_row(r0 + wrow + frow, a_cur);   // the lane's whole row: all of its loads in flight at once
            f32x4 acc[kQTiles];
#pragma unroll
            for (int t = 0; t < kQTiles; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < kKSteps; ++ks) {
                if (ks < nks) {
#pragma unroll
                    for (int t = 0; t < kQTiles; ++t) {
                        if (t < nt) {
                            const uint4 bq = *reinterpret_cast<const uint4 *>(&qs[(t * 16 + frow) * ldq + ks * 32 + koff]);
                            acc[t] = mfma32<F16>(a_cur[ks], bq, acc[t]);
                        }
                    }
                }
            }
            // the lane owns passage rows rb .. rb + 3 of query token 16 t + frow: the row mask, then the running maximum
            const int64_t rb = r0 + wrow + 4 * (lane >> 4);
#pragma unroll
            for (int t = 0; t < kQTiles; ++t) {
                if (t < nt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) m[t] = fmaxf(m[t], rb + r < len ? acc[t][r] : -INFINITY);
                }
            }
        }
    }

    // across the four lane groups (the rows 4 g + r of a tile), then across the four wavefronts in LDS
#pragma unroll
    for (int t = 0; t < kQTiles; ++t) {
        m[t] = fmaxf(m[t], __shfl_xor(m[t], 16, 64));
        m[t] = fmaxf(m[t], __shfl_xor(m[t], 32, 64));
        if (lane < 16) red[wave][t * 16 + lane] = m[t];
    }
    __syncthreads();
    if (wave == 0) {
        const float mi = fmaxf(fmaxf(red[0][lane], red[1][lane]), fmaxf(red[2][lane], red[3][lane]));   // token `lane`
        double sum = 0.0;
        for (int i = 0; i < nq; ++i) sum += (double)__shfl(mi, i, 64);    // the column mask: tokens 0 .. nq - 1 only
        if (lane == 0) *dst = canonical((float)sum);
    }
}

constexpr int kRankThreads = 256;

// n_ids > 0: an id >= n_ids is an empty slot too; n_ids <= 0: negative ids only
__global__ __launch_bounds__(kRankThreads) void late_rank_kernel(const float *__restrict__ score, int64_t ld,
                                                                 const int32_t *__restrict__ cand, int64_t n_ids, int32_t c,
                                                                 int32_t k, int32_t np2, int32_t *__restrict__ sel_out,
                                                                 int32_t *__restrict__ idx_out, float *__restrict__ score_out) {
    __shared__ uint64_t keys[HRAG_LATE_MAX_CANDIDATES];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const float *srow = score + (size_t)b * ld;
    const int32_t *irow = cand + (size_t)b * c;
    for (int i = tid; i < np2; i += kRankThreads) {
        uint64_t key = 0;       // keys of live slots are > 0 (common.h rank_key)
        if (i < c) {
            const int32_t id = irow[i];
            if (id >= 0 && (n_ids <= 0 || (int64_t)id < n_ids)) key = rank_key(srow[i], ~(uint32_t)i);
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int size = 2; size <= np2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < np2; i += kRankThreads) {
                const int j = i ^ stride;
                if (j > i) {
                    const uint64_t x = keys[i], y = keys[j];
                    const bool desc = (i & size) == 0;      // the final merge (size == np2) is descending throughout
                    if (desc ? x < y : x > y) {
                        keys[i] = y;
                        keys[j] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int j = tid; j < k; j += kRankThreads) {
        const uint64_t key = keys[j];
        const int32_t s = key ? (int32_t)~(uint32_t)key : -1;
        if (sel_out) sel_out[(size_t)b * k + j] = s;
        idx_out[(size_t)b * k + j] = key ? irow[s] : -1;
        score_out[(size_t)b * k + j] = key ? ordered_to_f32((uint32_t)(key >> 32)) : 0.f;
    }
}

void late_free(hrag_late *x) {
    if (!x) return;
    if (x->d_tok_ptr) (void)hipFree(x->d_tok_ptr);
    delete x;
}

// the host rules of a batch of late queries
hrag_status late_check_queries(const hrag_late *ix, const int32_t *q_ptr, const int32_t *q_ptr_dev, const uint16_t *q_tok_dev,
                               int32_t batch, int32_t *max_nq) {
    HRAG_REQUIRE(ix != nullptr, "the token index is NULL");
    HRAG_REQUIRE(batch >= 1, "batch=%d: at least 1", batch);
    HRAG_REQUIRE(q_ptr && q_ptr_dev, "q_ptr / q_ptr_dev is NULL");
    HRAG_REQUIRE(q_ptr[0] == 0, "q_ptr[0] = %d, 0 expected", q_ptr[0]);
    *max_nq = 0;
    for (int32_t b = 0; b < batch; ++b) {
        *max_nq = std::max(*max_nq, q_ptr[b + 1] - q_ptr[b]);
        HRAG_REQUIRE(q_ptr[b + 1] >= q_ptr[b], "q_ptr decreases at query %d (%d -> %d)", b, q_ptr[b], q_ptr[b + 1]);
        HRAG_REQUIRE(q_ptr[b + 1] - q_ptr[b] <= HRAG_LATE_MAX_QUERY_TOKENS,
                     "query %d holds %d tokens, at most HRAG_LATE_MAX_QUERY_TOKENS=%d", b, q_ptr[b + 1] - q_ptr[b],
                     HRAG_LATE_MAX_QUERY_TOKENS);
    }
    HRAG_REQUIRE(q_ptr[batch] == 0 || q_tok_dev, "q_tok is NULL with %d query tokens", q_ptr[batch]);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(q_tok_dev) & 15) == 0, "q_tok must be 16-byte aligned");
    return HRAG_OK;
}

hrag_status late_check_cand(int32_t c, int64_t ld, const void *cand, const void *scores) {
    HRAG_REQUIRE(cand && scores, "NULL argument");
    HRAG_REQUIRE(c >= 1 && c <= HRAG_LATE_MAX_CANDIDATES, "c=%d outside [1, HRAG_LATE_MAX_CANDIDATES=%d]", c,
                 HRAG_LATE_MAX_CANDIDATES);
    HRAG_REQUIRE(ld >= c, "ld=%lld below c=%d", (long long)ld, c);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(scores) & 3) == 0, "the scores must be 4-byte aligned");
    return HRAG_OK;
}

hrag_status launch_late_scores(const hrag_late *ix, const int32_t *q_ptr_dev, const uint16_t *q_tok_dev, int64_t q_total,
                               int32_t max_nq, int32_t batch, const int32_t *cand, int32_t c, float *out, int64_t ld,
                               hipStream_t s) {
    const int64_t grid = (int64_t)batch * c;
    HRAG_REQUIRE(grid < ((int64_t)1 << 31), "batch=%d x c=%d exceeds one launch", batch, c);
    // the staged query tokens of the longest query of the batch, in whole 16-token tiles
    const int32_t nq_cap = std::min(max_nq, HRAG_LATE_MAX_QUERY_TOKENS);
    const size_t lds = (size_t)round_up(nq_cap, 16) * (size_t)(round_up(ix->dim, 32) + kQPad) * sizeof(uint16_t);
    if (ix->dtype == HRAG_FP16)
        hipLaunchKernelGGL(late_maxsim_kernel<true>, dim3((unsigned)grid), dim3(kLateThreads), lds, s, ix->tok_emb,
                           ix->d_tok_ptr, ix->n_passages, ix->dim, q_ptr_dev, q_tok_dev, q_total, nq_cap, cand, c, out, ld);
    else
        hipLaunchKernelGGL(late_maxsim_kernel<false>, dim3((unsigned)grid), dim3(kLateThreads), lds, s, ix->tok_emb,
                           ix->d_tok_ptr, ix->n_passages, ix->dim, q_ptr_dev, q_tok_dev, q_total, nq_cap, cand, c, out, ld);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status launch_late_rank(const float *scores, int64_t ld, const int32_t *cand, int64_t n_ids, int32_t batch, int32_t c,
                             int32_t k, int32_t *sel, int32_t *idx, float *score, hipStream_t s) {
    HRAG_REQUIRE(idx && score, "NULL argument");
    HRAG_REQUIRE(batch >= 1, "batch=%d: at least 1", batch);
    HRAG_REQUIRE(k >= 1 && k <= c, "k=%d outside [1, c=%d]", k, c);
    int32_t np2 = 2;
    while (np2 < c) np2 <<= 1;
    hipLaunchKernelGGL(late_rank_kernel, dim3((unsigned)batch), dim3(kRankThreads), 0, s, scores, ld, cand, n_ids, c, k, np2,
                       sel, idx, score);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

}  // namespace
}  // namespace hrag

using namespace hrag;

// ---- exports (include/hrag.h, late-interaction reranking)
hrag_status hrag_late_create(int64_t n_passages, const int64_t *tok_ptr, const uint16_t *tok_emb_dev, int32_t dim, int32_t dtype,
                             hrag_late **out) {
    HRAG_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    HRAG_REQUIRE(n_passages >= 1 && n_passages < ((int64_t)1 << 31), "n_passages=%lld outside [1, 2^31)", (long long)n_passages);
    HRAG_REQUIRE(dtype == HRAG_BF16 || dtype == HRAG_FP16, "dtype=%d: HRAG_BF16 (0) or HRAG_FP16 (1), the element type of tok_emb",
                 dtype);
    HRAG_REQUIRE(dim >= 8 && dim % 8 == 0, "dim=%d must be a positive multiple of 8", dim);
    HRAG_REQUIRE(dim <= HRAG_LATE_MAX_DIM, "dim=%d above HRAG_LATE_MAX_DIM=%d", dim, HRAG_LATE_MAX_DIM);
    HRAG_REQUIRE(tok_ptr != nullptr, "tok_ptr is NULL");
    HRAG_REQUIRE(tok_ptr[0] == 0, "tok_ptr[0] = %lld, 0 expected", (long long)tok_ptr[0]);
    for (int64_t p = 0; p < n_passages; ++p)
        HRAG_REQUIRE(tok_ptr[p + 1] >= tok_ptr[p], "tok_ptr decreases at passage %lld (%lld -> %lld)", (long long)p,
                     (long long)tok_ptr[p], (long long)tok_ptr[p + 1]);
    const int64_t n_tokens = tok_ptr[n_passages];
    HRAG_REQUIRE(n_tokens == 0 || tok_emb_dev, "tok_emb is NULL with %lld tokens", (long long)n_tokens);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(tok_emb_dev) & 15) == 0, "tok_emb must be 16-byte aligned");
    hrag_late *x = new (std::nothrow) hrag_late();
    if (!x) { set_error("out of host memory"); return HRAG_ENOMEM; }
    x->n_passages = n_passages;
    x->n_tokens = n_tokens;
    x->dim = dim;
    x->dtype = dtype;
    x->tok_emb = tok_emb_dev;
    const hrag_status st = dev_upload(&x->d_tok_ptr, tok_ptr, n_passages + 1);
    if (st != HRAG_OK) {
        late_free(x);
        return st;
    }
    *out = x;
    return HRAG_OK;
}

hrag_status hrag_late_destroy(hrag_late *ix) {
    late_free(ix);
    return HRAG_OK;
}

hrag_status hrag_late_scores(const hrag_late *ix, const int32_t *q_ptr, const int32_t *q_ptr_dev, const uint16_t *q_tok_dev,
                             int32_t batch, const int32_t *cand_idx_dev, int32_t c, float *out_dev, int64_t ld,
                             hrag_stream stream) {
    int32_t max_nq = 0;
    HRAG_TRY(late_check_queries(ix, q_ptr, q_ptr_dev, q_tok_dev, batch, &max_nq));
    HRAG_TRY(late_check_cand(c, ld, cand_idx_dev, out_dev));
    return launch_late_scores(ix, q_ptr_dev, q_tok_dev, q_ptr[batch], max_nq, batch, cand_idx_dev, c, out_dev, ld, (hipStream_t)stream);
}

hrag_status hrag_late_rank_rows(const float *scores_dev, int64_t ld, const int32_t *cand_idx_dev, int64_t n_ids, int32_t batch,
                                int32_t c, int32_t k, int32_t *sel_out_dev, int32_t *idx_out_dev, float *score_out_dev,
                                hrag_stream stream) {
    HRAG_TRY(late_check_cand(c, ld, cand_idx_dev, scores_dev));
    return launch_late_rank(scores_dev, ld, cand_idx_dev, n_ids, batch, c, k, sel_out_dev, idx_out_dev, score_out_dev,
                            (hipStream_t)stream);
}

int64_t hrag_late_workspace_bytes(int32_t batch, int32_t c) {
    if (batch < 1 || c < 1 || c > HRAG_LATE_MAX_CANDIDATES) return -1;
    return (int64_t)batch * round_up(c, 4) * (int64_t)sizeof(float);
}

hrag_status hrag_late_rerank(const hrag_late *ix, const int32_t *q_ptr, const int32_t *q_ptr_dev, const uint16_t *q_tok_dev,
                             int32_t batch, const int32_t *cand_idx_dev, int32_t c, int32_t k, int32_t *sel_out_dev,
                             int32_t *idx_out_dev, float *score_out_dev, void *workspace_dev, size_t workspace_bytes,
                             hrag_stream stream) {
    int32_t max_nq = 0;
    HRAG_TRY(late_check_queries(ix, q_ptr, q_ptr_dev, q_tok_dev, batch, &max_nq));
    HRAG_REQUIRE(cand_idx_dev && idx_out_dev && score_out_dev, "NULL argument");
    HRAG_REQUIRE(c >= 1 && c <= HRAG_LATE_MAX_CANDIDATES, "c=%d outside [1, HRAG_LATE_MAX_CANDIDATES=%d]", c,
                 HRAG_LATE_MAX_CANDIDATES);
    HRAG_REQUIRE(k >= 1 && k <= c, "k=%d outside [1, c=%d]", k, c);
    const int64_t need = hrag_late_workspace_bytes(batch, c);
    HRAG_REQUIRE(workspace_dev && (int64_t)workspace_bytes >= need,
                 "workspace of %lld bytes, %lld needed (hrag_late_workspace_bytes)", (long long)workspace_bytes, (long long)need);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(workspace_dev) & 15) == 0, "the workspace must be 16-byte aligned");
    float *scores = static_cast<float *>(workspace_dev);
    const int64_t ld = round_up(c, 4);
    hipStream_t s = (hipStream_t)stream;
    HRAG_TRY(launch_late_scores(ix, q_ptr_dev, q_tok_dev, q_ptr[batch], max_nq, batch, cand_idx_dev, c, scores, ld, s));
    return launch_late_rank(scores, ld, cand_idx_dev, ix->n_passages, batch, c, k, sel_out_dev, idx_out_dev, score_out_dev, s);
}
