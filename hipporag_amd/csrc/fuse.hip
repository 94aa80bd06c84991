// Fused retrieval (include/hrag.h, hrag_fuse_rows / hrag_rrf_rows / hrag_last_fused): the score rows of B member queries
// [B][ld] -> one row per QUESTION, the questions being consecutive runs of member rows (member_ptr int32 [Q + 1]).
//
// fuse_cols_kernel<MODE, WEIGHTED, W> (sum, max): one thread owns W columns (one float4, or one float where the rows are not
// 16-byte aligned) across ALL questions and walks the member rows 0 .. B - 1 in order, kFuseChunk rows per step: the loads
// of a step are independent of each other and of everything before them, so kFuseChunk loads per lane are in flight
// whatever the partition is (256 singletons, one question of 256 rows); only the fp64 adds of a question form a chain, by
// definition.  Row r closes question q when r + 1 == member_ptr[q + 1]: the fused value is stored to row q and the chain
// starts again.  IN PLACE: row q is written after row member_ptr[q + 1] - 1 >= q was consumed, by the thread that reads the
// column, and every row is loaded before a step that could overwrite it runs (a step's loads come before its stores) -- no
// second buffer, no synchronisation.  Loads of one row are contiguous over the wavefront.  member_ptr / weight are
// wavefront-uniform (scalar loads).  The columns n .. ld of a row are never read or written.
//   SUM  acc = +0.0; acc += (double)w * (double)s in member order, rounded once; the product of two fp32 values is exact in
//        fp64, so contracting it into an fma changes nothing.  NaN is stored as the quiet NaN.
//   MAX  the largest ranking key (common.h f32_to_ordered; every NaN above +inf), decoded as the ranking decodes it.
//
// rrf_scatter_kernel: one workgroup per question over caller-supplied ranked lists int32 [B][depth] (-1: an empty slot).
// Member by member, in order, the workgroup adds t = (float)((double)w / (double)(c + rank)) to the fused row at every listed
// passage -- an fp32 chain in member order -- with a barrier between members: the ids of ONE member are unique, so no two
// lanes touch one element between two barriers; no atomics, and the result does not depend on any order of execution.  The
// rows are zeroed by a launch of their own before (a passage no member lists keeps +0.0).
#include <algorithm>

#include "common.h"

namespace hrag {

namespace {

constexpr int kFuseThreads = 256;
constexpr int kFuseChunk = 8;       // member rows loaded per step
constexpr int kRrfThreads = 1024;

template <int W> struct FuseVec;
template <> struct FuseVec<1> { using type = float; };
template <> struct FuseVec<4> { using type = float4; };

template <int MODE, bool WEIGHTED, int W>
__device__ __forceinline__ void fuse_cols(float *rows, int64_t col, int64_t ld, const int32_t *__restrict__ member_ptr,
                                          int32_t batch, int32_t n_fused, const float *__restrict__ weight) {
    using V = typename FuseVec<W>::type;
    double acc[W];
    uint32_t best[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { acc[i] = 0.0; best[i] = 0u; }
    int32_t q = 0;
    int32_t end = member_ptr[1];
    for (int32_t r0 = 0; r0 < batch; r0 += kFuseChunk) {
        float v[kFuseChunk][W];
#pragma unroll
        for (int u = 0; u < kFuseChunk; ++u) {
            if (r0 + u < batch) {
                const V x = *reinterpret_cast<const V *>(rows + (size_t)(r0 + u) * ld + col);
                if constexpr (W == 4) { v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w; }
                else v[u][0] = x;
            }
        }
#pragma unroll
        for (int u = 0; u < kFuseChunk; ++u) {
            const int32_t r = r0 + u;
            if (r >= batch) break;
            if constexpr (MODE == HRAG_FUSE_SUM) {
                const double w = WEIGHTED ? (double)weight[r] : 1.0;
#pragma unroll
                for (int i = 0; i < W; ++i) acc[i] += w * (double)v[u][i];
            } else {
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const uint32_t o = v[u][i] != v[u][i] ? kOrderedNaN : f32_to_ordered(v[u][i]);
                    best[i] = o > best[i] ? o : best[i];
                }
            }
            if (r + 1 == end && q < n_fused) {
                float out[W];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    if constexpr (MODE == HRAG_FUSE_SUM) {
                        const float f = (float)acc[i];
                        out[i] = f != f ? __uint_as_float(0x7fc00000u) : f;
                    } else {
                        out[i] = ordered_to_f32(best[i]);
                    }
                    acc[i] = 0.0;
                    best[i] = 0u;
                }
                float *dst = rows + (size_t)q * ld + col;
                if constexpr (W == 4) *reinterpret_cast<float4 *>(dst) = make_float4(out[0], out[1], out[2], out[3]);
                else *dst = out[0];
                ++q;
                end = q < n_fused ? member_ptr[q + 1] : 0x7fffffff;
            }
        }
    }
}

template <int MODE, bool WEIGHTED, int W>
__global__ __launch_bounds__(kFuseThreads) void fuse_cols_kernel(float *rows, int64_t n, int64_t ld,
                                                                 const int32_t *__restrict__ member_ptr, int32_t batch,
                                                                 int32_t n_fused, const float *__restrict__ weight) {
    const int64_t col = ((int64_t)blockIdx.x * kFuseThreads + threadIdx.x) * W;
    if (col >= n) return;
    if (W == 1 || col + W <= n) {
        fuse_cols<MODE, WEIGHTED, W>(rows, col, ld, member_ptr, batch, n_fused, weight);
    } else {
        // the last, partial group of four: column by column (n .. ld is not touched)
        for (int64_t c = col; c < n; ++c) fuse_cols<MODE, WEIGHTED, 1>(rows, c, ld, member_ptr, batch, n_fused, weight);
    }
}

__global__ void zero_rows_kernel(float *__restrict__ rows, int64_t n, int64_t ld) {
    float *row = rows + (size_t)blockIdx.y * ld;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) row[i] = 0.f;
}

__global__ __launch_bounds__(kRrfThreads) void rrf_scatter_kernel(const int32_t *__restrict__ list_idx, int32_t depth,
                                                                  const int32_t *__restrict__ member_ptr,
                                                                  const float *__restrict__ weight, int32_t c, float *out,
                                                                  int64_t n, int64_t ld, int32_t batch) {
    const int32_t q = blockIdx.x;
    int32_t beg = member_ptr[q], end = member_ptr[q + 1];
    beg = beg < 0 ? 0 : beg > batch ? batch : beg;          // the lists have `batch` rows
    end = end < beg ? beg : end > batch ? batch : end;
    float *row = out + (size_t)q * ld;
    for (int32_t m = beg; m < end; ++m) {
        const double w = weight ? (double)weight[m] : 1.0;
        const int32_t *list = list_idx + (size_t)m * depth;
        for (int32_t j = threadIdx.x; j < depth; j += kRrfThreads) {
            const int32_t id = list[j];
            if (id < 0 || (int64_t)id >= n) continue;       // an empty slot; an id outside the row is never written
            const float t = (float)(w / ((double)c + (double)(j + 1)));
            row[id] = row[id] + t;
        }
        __syncthreads();    // the next member's adds see this member's (one workgroup, global memory)
    }
}

// per-member filter rows of a per-question filter: dst[m][w] = src[q][w] for every member m of question q
__global__ void expand_filter_kernel(const uint32_t *__restrict__ src, int64_t src_ld, int64_t words,
                                     const int32_t *__restrict__ member_ptr, int32_t batch, uint32_t *__restrict__ dst) {
    const int32_t q = blockIdx.y;
    int32_t beg = member_ptr[q], end = member_ptr[q + 1];
    beg = beg < 0 ? 0 : beg > batch ? batch : beg;
    end = end < beg ? beg : end > batch ? batch : end;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t v = src[(size_t)q * src_ld + i];
        for (int32_t m = beg; m < end; ++m) dst[(size_t)m * words + i] = v;
    }
}

hrag_status check_rows(const void *rows, int32_t batch, int64_t n, int64_t ld, const int32_t *member_ptr, int32_t n_fused) {
    HRAG_REQUIRE(rows && member_ptr, "NULL argument");
    HRAG_REQUIRE(batch >= 1, "batch=%d: at least 1", batch);
    HRAG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && ld >= n, "n=%lld / ld=%lld: 1 <= n < 2^31, ld >= n", (long long)n,
                 (long long)ld);
    HRAG_REQUIRE(n_fused >= 1 && n_fused <= batch, "n_fused=%d outside [1, batch=%d]", n_fused, batch);
    return HRAG_OK;
}

}  // namespace

hrag_status launch_fuse_rows(float *rows, int32_t batch, int64_t n, int64_t ld, const int32_t *member_ptr, int32_t n_fused,
                             const float *weight, int32_t mode, hipStream_t s) {
    HRAG_TRY(check_rows(rows, batch, n, ld, member_ptr, n_fused));
    HRAG_REQUIRE(mode == HRAG_FUSE_SUM || mode == HRAG_FUSE_MAX, "mode=%d: HRAG_FUSE_SUM (0) or HRAG_FUSE_MAX (1)", mode);
    HRAG_REQUIRE(mode != HRAG_FUSE_MAX || weight == nullptr, "HRAG_FUSE_MAX takes no weights");
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 3) == 0, "score rows must be 4-byte aligned");
    const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
    const dim3 grid((unsigned)ceil_div(vec ? ceil_div(n, 4) : n, kFuseThreads));
#define HRAG_FUSE_LAUNCH(M, WT, W)                                                                                   \
    hipLaunchKernelGGL((fuse_cols_kernel<M, WT, W>), grid, dim3(kFuseThreads), 0, s, rows, n, ld, member_ptr, batch, \
                       n_fused, weight)
    if (mode == HRAG_FUSE_MAX) {
        if (vec) HRAG_FUSE_LAUNCH(HRAG_FUSE_MAX, false, 4); else HRAG_FUSE_LAUNCH(HRAG_FUSE_MAX, false, 1);
    } else if (weight) {
        if (vec) HRAG_FUSE_LAUNCH(HRAG_FUSE_SUM, true, 4); else HRAG_FUSE_LAUNCH(HRAG_FUSE_SUM, true, 1);
    } else {
        if (vec) HRAG_FUSE_LAUNCH(HRAG_FUSE_SUM, false, 4); else HRAG_FUSE_LAUNCH(HRAG_FUSE_SUM, false, 1);
    }
#undef HRAG_FUSE_LAUNCH
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status launch_rrf_rows(const int32_t *list_idx, int32_t batch, int32_t depth, const int32_t *member_ptr,
                            int32_t n_fused, const float *weight, int32_t c, float *out, int64_t n, int64_t ld,
                            hipStream_t s) {
    HRAG_TRY(check_rows(out, batch, n, ld, member_ptr, n_fused));
    HRAG_REQUIRE(list_idx != nullptr, "NULL argument");
    HRAG_REQUIRE(depth >= 1, "depth=%d: at least 1", depth);
    HRAG_REQUIRE(c >= 0, "c=%d: at least 0", c);
    HRAG_REQUIRE(n_fused <= 65535, "n_fused=%d above 65535 questions per call", n_fused);
    const dim3 zgrid((unsigned)std::min<int64_t>(ceil_div(n, 256), 1024), (unsigned)n_fused);
    hipLaunchKernelGGL(zero_rows_kernel, zgrid, dim3(256), 0, s, out, n, ld);
    HRAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(rrf_scatter_kernel, dim3((unsigned)n_fused), dim3(kRrfThreads), 0, s, list_idx, depth, member_ptr,
                       weight, c, out, n, ld, batch);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status launch_expand_filter(const uint32_t *src, int64_t src_ld, int64_t words, const int32_t *member_ptr,
                                 int32_t batch, int32_t n_fused, uint32_t *dst, hipStream_t s) {
    HRAG_REQUIRE(src && member_ptr && dst && words >= 1 && src_ld >= words, "bad argument");
    HRAG_REQUIRE(n_fused >= 1 && n_fused <= 65535, "n_fused=%d outside [1, 65535]", n_fused);
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(words, 256), 64), (unsigned)n_fused);
    hipLaunchKernelGGL(expand_filter_kernel, grid, dim3(256), 0, s, src, src_ld, words, member_ptr, batch, dst);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

}  // namespace hrag
