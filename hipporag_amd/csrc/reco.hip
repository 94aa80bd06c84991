// Recommend by example (include/hrag.h, "recommend by example": hrag_reco_rows / hrag_reco_scores_rows / hrag_reco_scores /
// hrag_reco_query / hrag_reco_exclude): score rows [B, n] from B ragged lists of liked (+1) and disliked (-1) passage ids,
// without the [E, n] matrix of example-against-passage scores ever reaching memory.
//
// reco_cols_kernel: the COLUMN TABLE.  Query b owns the 32 columns 32 b .. 32 b + 31 -- two 16-column MFMA blocks, the
// second one live only when the query holds more than 16 examples -- and column 32 b + e is example e of its list:
// (id, sign) with id = -1 / sign = 0 for an empty example (id outside [0, rows), sign 0) and for padding; cnt[b] = the
// examples read (at most HRAG_RECO_MAX_EXAMPLES).  One MFMA column block never mixes queries.
//
// reco_scores_kernel<F16>: a GEMM whose A side streams HRAG_RECO_TILE = 128 passage rows exactly as sim_gemm_kernel does
// (global -> registers -> LDS in 64-element k slices, rows padded to 144 bytes, the next slice's loads in flight during
// the MFMAs) and whose B side is the example rows of FOUR queries (128 columns), read by id straight from the embedding
// matrix with 16-byte loads (gram_gather_kernel's B side; on a split engine the thirds of the stored [hi | lo | hi] row in
// the order (0, 2, 1)).  2 x 2 wavefronts of 64 rows x 64 columns (two queries each); a column block without examples is
// skipped whole (wavefront-uniform).  The chain per element IS sim_gemm_kernel's: BK = 64 steps of two
// v_mfma_f32_16x16x32 in ascending k into one fp32 accumulator, the k tail zero-filled in 8-element chunks.
// Epilogue: the accumulators (col = lane & 15, row = 4 (lane >> 4) + reg) go to LDS TRANSPOSED, [column][row], in two
// rounds of 64 rows (the k loop's tiles lend their memory); then thread (row, query) -- a wavefront per query, so the
// example count is uniform -- walks its query's columns in list order through reco_reduce below, the same function that
// reco_rows_kernel runs over rows in memory, and makes one coalesced fp32 store per (query, passage).  Padding and empty
// columns carry sign 0 and never enter the maximum or the sum.  No atomics; every output word is written once.
//
// reco_rows_kernel: the reduce alone over caller-supplied example score rows [E, ld], one thread per (query, passage).
// reco_query_kernel: HRAG_RECO_AVERAGE_VECTOR, one workgroup per query, a thread per component, ordered fp64 sums.
// reco_exclude_kernel: one thread per query clears the bits of its examples in its own filter row (one writer per row).
#include "engine_impl.h"

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

constexpr int kMaxEx = HRAG_RECO_MAX_EXAMPLES;   // columns of one query
constexpr int BM = HRAG_RECO_TILE;               // passages per workgroup
constexpr int kQPerWg = 4;                       // queries per workgroup
constexpr int BN = kQPerWg * kMaxEx;             // columns per workgroup
constexpr int BK = 64;
constexpr int LDS_LD = BK + 8;                   // 16-bit elements per LDS row (144 bytes, sim_gemm.hip)
constexpr int kHalf = BM / 2;                    // rows of one epilogue round
constexpr int S_LD = kHalf + 4;                  // floats per transposed column (272 bytes: float4 stores stay aligned)
static_assert(kMaxEx == 32 && BM == 128 && BN == 128, "2 x 2 wavefronts of 64 x 64, two 16-column blocks per query");
constexpr size_t kTileBytes = (size_t)(BM + BN) * LDS_LD * sizeof(uint16_t);
static_assert((size_t)BN * S_LD * sizeof(float) <= kTileBytes, "the transposed accumulators fit the k loop's tiles");

// The strategies of include/hrag.h over one (query, passage): sign(e) in {+1, -1, 0} and score(e) for e < cnt, list order.
template <typename Sign, typename Score>
__device__ __forceinline__ float reco_reduce(int mode, int cnt, Sign sign, Score score) {
    if (mode == HRAG_RECO_BEST_SCORE) {
        float bp = -INFINITY, bn = -INFINITY;
        for (int e = 0; e < cnt; ++e) {
            const int sg = sign(e);
            if (sg == 0) continue;
            const float v = score(e);
            if (sg > 0) {
                if (v > bp) bp = v;
            } else if (v > bn) {
                bn = v;
            }
        }
        return bp > bn ? bp : -__fmul_rn(bn, bn);
    }
    double acc = 0.0;
    for (int e = 0; e < cnt; ++e)
        if (sign(e) > 0) acc += (double)score(e);
    for (int e = 0; e < cnt; ++e)
        if (sign(e) < 0) acc -= (double)score(e);
    const float o = (float)acc;
    return o != o ? __uint_as_float(0x7fc00000u) : o;
}

// a query's example range as the device-side ex_ptr gives it, held inside [0, total] and to the cap
__device__ __forceinline__ void ex_range(const int32_t *__restrict__ ex_ptr, int64_t b, int32_t total, int32_t &p0, int32_t &cnt) {
    int32_t lo = ex_ptr[b], hi = ex_ptr[b + 1];
    lo = lo < 0 ? 0 : lo > total ? total : lo;
    hi = hi < lo ? lo : hi > total ? total : hi;
    p0 = lo;
    cnt = hi - lo > kMaxEx ? kMaxEx : hi - lo;
}

__global__ __launch_bounds__(256) void reco_cols_kernel(const int32_t *__restrict__ ex_ptr, const int32_t *__restrict__ ex_idx,
                                                        const int32_t *__restrict__ ex_sign, int32_t total, int32_t batch,
                                                        int64_t rows, int2 *__restrict__ cols, int32_t *__restrict__ cnt_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t b = i / kMaxEx;
    const int e = (int)(i % kMaxEx);
    if (b >= batch) return;
    int32_t p0, cnt;
    ex_range(ex_ptr, b, total, p0, cnt);
    int32_t id = -1, sg = 0;
    if (e < cnt) {
        id = ex_idx[p0 + e];
        sg = ex_sign[p0 + e];
        sg = sg > 0 ? 1 : sg < 0 ? -1 : 0;
        if (id < 0 || (int64_t)id >= rows || sg == 0) {
            id = -1;
            sg = 0;
        }
    }
    cols[i] = make_int2(id, sg);
    if (e == 0) cnt_out[b] = cnt;
}

// third: kdim / 3 on the split layout (the B side reads the thirds as (0, 2, 1)), 0 otherwise
template <bool F16>
__global__ __launch_bounds__(256) void reco_scores_kernel(const uint16_t *__restrict__ emb, int64_t rows, int32_t kdim,
                                                          int32_t third, const int2 *__restrict__ cols,
                                                          const int32_t *__restrict__ cnt, int32_t batch, int32_t mode,
                                                          float *__restrict__ out, int64_t ld, int32_t n_tiles_n) {
    constexpr int MI = 4, NJ = 4;   // 2 x 2 wavefronts of 64 x 64
    __shared__ __attribute__((aligned(16))) unsigned char smem[kTileBytes];
    __shared__ int32_t s_sign[BN];
    __shared__ int32_t s_cnt[kQPerWg];
    uint16_t(*As)[LDS_LD] = reinterpret_cast<uint16_t(*)[LDS_LD]>(smem);
    uint16_t(*Bs)[LDS_LD] = reinterpret_cast<uint16_t(*)[LDS_LD]>(smem + (size_t)BM * LDS_LD * sizeof(uint16_t));
    float *S = reinterpret_cast<float *>(smem);     // [BN][S_LD], after the k loop

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // the tile order of sim_gemm_kernel: the query tiles of one passage tile run back to back on one XCD
    const int64_t tile = blockIdx.x;
    const int64_t jj = tile >> 3;
    const int nt = (int)(jj % n_tiles_n);
    const int64_t mt = (jj / n_tiles_n) * 8 + (tile & 7);
    if (mt * BM >= rows) return;     // the grid is padded to a multiple of 8 passage tiles
    const int64_t m0 = mt * BM;
    const int q0 = nt * kQPerWg;

    if (tid < BN) {
        const int gq = q0 + tid / kMaxEx;
        s_sign[tid] = gq < batch ? cols[(size_t)gq * kMaxEx + (tid & (kMaxEx - 1))].y : 0;
    }
    if (tid < kQPerWg) s_cnt[tid] = q0 + tid < batch ? cnt[q0 + tid] : 0;

    const int ld_row = tid >> 3;        // 0..31: pass p holds passage row ld_row + 32 p and example ld_row of query q0 + p
    const int ld_chunk = (tid & 7) * 8; // element offset inside the BK slice
    const uint16_t *brow[kQPerWg];      // the embedding row of this thread's columns (nullptr: an empty or padding column)
#pragma unroll
    for (int p = 0; p < kQPerWg; ++p) {
        const int gq = q0 + p;
        const int32_t id = gq < batch ? cols[(size_t)gq * kMaxEx + ld_row].x : -1;
        brow[p] = (id >= 0 && (int64_t)id < rows) ? emb + (size_t)id * kdim : nullptr;
    }
    __syncthreads();
    // bit j: column block j of this wavefront holds an example (query 2 wn + (j >> 1), its examples 16 (j & 1) ...)
    int live = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) live |= (s_cnt[wn * 2 + (j >> 1)] > 16 * (j & 1) ? 1 : 0) << j;
    live = __builtin_amdgcn_readfirstlane(live);

    uint4 ra[BM / 32], rb[kQPerWg];
    auto load_tile = [&](int k0) {
        const int kk = k0 + ld_chunk;
        int kb = kk;                    // where the B ("query") side finds logical position kk in a stored row
        if (third > 0) kb = kk < third ? kk : kk < 2 * third ? kk + third : kk - third;
#pragma unroll
        for (int p = 0; p < BM / 32; ++p) {
            const int64_t gm = m0 + ld_row + 32 * p;
            ra[p] = make_uint4(0, 0, 0, 0);
            if (gm < rows && kk < kdim) ra[p] = *reinterpret_cast<const uint4 *>(emb + (size_t)gm * kdim + kk);
        }
#pragma unroll
        for (int p = 0; p < kQPerWg; ++p) {
            rb[p] = make_uint4(0, 0, 0, 0);
            if (brow[p] && kk < kdim) rb[p] = *reinterpret_cast<const uint4 *>(brow[p] + kb);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int p = 0; p < BM / 32; ++p) *reinterpret_cast<uint4 *>(&As[ld_row + 32 * p][ld_chunk]) = ra[p];
#pragma unroll
        for (int p = 0; p < kQPerWg; ++p) *reinterpret_cast<uint4 *>(&Bs[ld_row + 32 * p][ld_chunk]) = rb[p];
    };

    f32x4 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_tile(0);
    for (int k0 = 0; k0 < kdim; k0 += BK) {
        store_tile();
        __syncthreads();
        if (k0 + BK < kdim) load_tile(k0 + BK);  // in flight while the MFMAs below run
#pragma unroll
        for (int s = 0; s < BK / 32; ++s) {
            uint4 a[MI];
            const int kcol = s * 32 + 8 * (lane >> 4);
#pragma unroll
            for (int i = 0; i < MI; ++i)
                a[i] = *reinterpret_cast<const uint4 *>(&As[(wm * MI + i) * 16 + (lane & 15)][kcol]);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (!((live >> j) & 1)) continue;       // (uniform over the wavefront)
                const uint4 bq = *reinterpret_cast<const uint4 *>(&Bs[(wn * NJ + j) * 16 + (lane & 15)][kcol]);
#pragma unroll
                for (int i = 0; i < MI; ++i) acc[i][j] = mfma32<F16>(a[i], bq, acc[i][j]);
            }
        }
        __syncthreads();        // (the last one frees the tiles for S)
    }

    // epilogue, rows 64 h .. 64 h + 63 per round: the two wavefronts that own them write S[column][row]; then thread
    // (row = tid & 63, query = tid >> 6) reduces its query's columns in list order
    const int er = tid & 63, eq = tid >> 6;
    const int ecnt = s_cnt[eq];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (wm == h) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int col = (wn * NJ + j) * 16 + (lane & 15);
                    const int row = i * 16 + 4 * (lane >> 4);
                    const f32x4 v = acc[i][j];
                    *reinterpret_cast<float4 *>(&S[col * S_LD + row]) = make_float4(v[0], v[1], v[2], v[3]);
                }
        }
        __syncthreads();
        const int64_t m = m0 + h * kHalf + er;
        const int gq = q0 + eq;
        if (gq < batch && m < rows) {
            const float *scol = S + (size_t)eq * kMaxEx * S_LD + er;
            const int32_t *sg = s_sign + eq * kMaxEx;
            out[(size_t)gq * ld + m] = reco_reduce(
                mode, ecnt, [&](int e) { return sg[e]; }, [&](int e) { return scol[e * S_LD]; });
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void reco_rows_kernel(const float *__restrict__ ex_scores, int64_t ld,
                                                        const int32_t *__restrict__ ex_ptr, const int32_t *__restrict__ ex_sign,
                                                        int64_t n, int32_t mode, float *__restrict__ out, int64_t ld_out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t b = blockIdx.y;
    if (p >= n) return;
    int32_t p0 = ex_ptr[b], cnt = ex_ptr[b + 1] - p0;      // (no total here: the caller's ex_ptr is taken as it is, to the cap)
    p0 = p0 < 0 ? 0 : p0;
    cnt = cnt < 0 ? 0 : cnt > kMaxEx ? kMaxEx : cnt;
    const float *src = ex_scores + (size_t)p0 * ld + p;
    const int32_t *sg = ex_sign + p0;
    out[(size_t)b * ld_out + p] = reco_reduce(
        mode, cnt, [&](int e) { return sg[e]; }, [&](int e) { return src[(size_t)e * ld]; });
}

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {       // (knn.hip)
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// kind: 0 bf16 rows, 1 fp16 rows, 2 split rows [hi | lo | hi] (fp16 halves; the query is written [qhi | qhi | qlo])
__global__ __launch_bounds__(256) void reco_query_kernel(const uint16_t *__restrict__ emb, int64_t rows, int32_t dim,
                                                         int32_t kind, const int32_t *__restrict__ ex_ptr,
                                                         const int32_t *__restrict__ ex_idx, const int32_t *__restrict__ ex_sign,
                                                         int32_t total, uint16_t *__restrict__ q_out, float *__restrict__ v_out,
                                                         int32_t *__restrict__ flags_out) {
    __shared__ int32_t s_id[kMaxEx], s_sg[kMaxEx];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    int32_t p0, cnt;
    ex_range(ex_ptr, b, total, p0, cnt);
    if (tid < kMaxEx) {
        int32_t id = -1, sg = 0;
        if (tid < cnt) {
            id = ex_idx[p0 + tid];
            sg = ex_sign[p0 + tid];
            if (id < 0 || (int64_t)id >= rows) sg = 0;
        }
        s_id[tid] = id;
        s_sg[tid] = sg;
    }
    __syncthreads();
    int n_pos = 0, n_neg = 0;
    for (int e = 0; e < cnt; ++e) {
        n_pos += s_sg[e] > 0 ? 1 : 0;
        n_neg += s_sg[e] < 0 ? 1 : 0;
    }
    const int kdim = kind == 2 ? 3 * dim : dim;
    for (int k = tid; k < dim; k += 256) {
        double sp = 0.0, sn = 0.0;
        for (int e = 0; e < cnt; ++e) {
            const int sg = s_sg[e];
            if (sg == 0) continue;
            const uint16_t *row = emb + (size_t)s_id[e] * kdim;
            double val;
            if (kind == 0) {
                val = (double)__uint_as_float((uint32_t)row[k] << 16);
            } else {
                const _Float16 *hrow = reinterpret_cast<const _Float16 *>(row);
                val = (double)hrow[k];
                if (kind == 2) val = val + (double)hrow[dim + k];
            }
            if (sg > 0) sp += val;
            else sn += val;
        }
        double v = 0.0;
        if (n_pos > 0) {
            const double a = sp / (double)n_pos;
            v = a;
            if (n_neg > 0) {
                const double g = sn / (double)n_neg;
                v = a + (a - g);
            }
        }
        const float vf = (float)v;
        if (v_out) v_out[(size_t)b * dim + k] = vf;
        if (kind == 0) {
            q_out[(size_t)b * dim + k] = f32_to_bf16_rne(vf);
        } else {
            _Float16 *o = reinterpret_cast<_Float16 *>(q_out) + (size_t)b * kdim;
            const _Float16 h = (_Float16)vf;                 // round to nearest even (split3_kernel)
            o[k] = h;
            if (kind == 2) {
                o[dim + k] = h;
                o[2 * dim + k] = (_Float16)(vf - (float)h);
            }
        }
    }
    if (tid == 0 && flags_out) flags_out[b] = n_pos == 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void reco_exclude_kernel(uint32_t *__restrict__ words, int64_t ld_words, int64_t n,
                                                           const int32_t *__restrict__ ex_ptr, const int32_t *__restrict__ ex_idx,
                                                           const int32_t *__restrict__ ex_sign, int32_t batch) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    int32_t p0 = ex_ptr[b], cnt = ex_ptr[b + 1] - p0;
    p0 = p0 < 0 ? 0 : p0;
    cnt = cnt < 0 ? 0 : cnt > kMaxEx ? kMaxEx : cnt;
    uint32_t *row = words + (size_t)b * ld_words;
    for (int e = 0; e < cnt; ++e) {
        const int32_t id = ex_idx[p0 + e];
        if (id < 0 || (int64_t)id >= n || (ex_sign && ex_sign[p0 + e] == 0)) continue;
        row[id >> 5] &= ~(1u << (id & 31));      // (plain load and store: the row has one writer)
    }
}

// the host rules of a batch of examples
hrag_status reco_check_examples(const int32_t *ex_ptr, const void *ex_ptr_dev, const void *ex_idx_dev, const void *ex_sign_dev,
                                int32_t batch) {
    HRAG_REQUIRE(batch >= 1, "batch=%d: at least 1", batch);
    HRAG_REQUIRE(ex_ptr && ex_ptr_dev, "ex_ptr / ex_ptr_dev is NULL");
    HRAG_REQUIRE(ex_ptr[0] == 0, "ex_ptr[0] = %d, 0 expected", ex_ptr[0]);
    for (int32_t b = 0; b < batch; ++b)
        HRAG_REQUIRE(ex_ptr[b + 1] >= ex_ptr[b], "ex_ptr decreases at query %d (%d -> %d)", b, ex_ptr[b], ex_ptr[b + 1]);
    HRAG_REQUIRE(ex_ptr[batch] == 0 || (ex_idx_dev && ex_sign_dev), "ex_idx / ex_sign is NULL with %d examples", ex_ptr[batch]);
    return HRAG_OK;
}

hrag_status reco_check_emb(const uint16_t *emb, int64_t rows, int32_t kdim, int32_t dtype, int32_t split) {
    HRAG_REQUIRE(emb != nullptr, "the embedding rows are NULL");
    HRAG_REQUIRE(dtype == HRAG_BF16 || dtype == HRAG_FP16, "dtype=%d: HRAG_BF16 (0) or HRAG_FP16 (1), the element type of the rows",
                 dtype);
    HRAG_REQUIRE(rows >= 1 && rows < ((int64_t)1 << 31), "rows=%lld outside [1, 2^31)", (long long)rows);
    HRAG_REQUIRE(kdim > 0 && kdim % 8 == 0, "kdim %d must be a positive multiple of 8", kdim);
    HRAG_REQUIRE(!split || (kdim % 24 == 0 && dtype == HRAG_FP16),
                 "a split layout is fp16 halves with kdim = 3 * dim, dim a multiple of 8 (kdim %d, dtype %d)", kdim, dtype);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(emb) & 15) == 0, "the embedding rows must be 16-byte aligned");
    return HRAG_OK;
}

bool reco_mode_ok(int32_t mode) { return mode == HRAG_RECO_BEST_SCORE || mode == HRAG_RECO_SUM_SCORES; }

hrag_status launch_reco_scores(const uint16_t *emb, int64_t rows, int32_t kdim, int32_t dtype, int32_t split,
                               const int32_t *ex_ptr, const int32_t *ex_ptr_dev, const int32_t *ex_idx_dev,
                               const int32_t *ex_sign_dev, int32_t batch, int32_t mode, float *out, int64_t ld, void *ws,
                               size_t ws_bytes, hipStream_t s) {
    HRAG_TRY(reco_check_emb(emb, rows, kdim, dtype, split));
    HRAG_TRY(reco_check_examples(ex_ptr, ex_ptr_dev, ex_idx_dev, ex_sign_dev, batch));
    HRAG_REQUIRE(reco_mode_ok(mode), "mode=%d: HRAG_RECO_BEST_SCORE (0) or HRAG_RECO_SUM_SCORES (1)", mode);
    HRAG_REQUIRE(out != nullptr && (reinterpret_cast<uintptr_t>(out) & 3) == 0, "the output is NULL or not 4-byte aligned");
    HRAG_REQUIRE(ld >= rows, "ld=%lld below rows=%lld", (long long)ld, (long long)rows);
    const int64_t need = hrag_reco_workspace_bytes(batch);
    HRAG_REQUIRE(ws && (int64_t)ws_bytes >= need, "workspace of %lld bytes, %lld needed (hrag_reco_workspace_bytes)",
                 (long long)ws_bytes, (long long)need);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "the workspace must be 16-byte aligned");
    const int64_t tiles_m = ceil_div(rows, BM);
    const int32_t tn = (int32_t)ceil_div(batch, kQPerWg);
    const int64_t grid = round_up(tiles_m, 8) * tn;
    HRAG_REQUIRE(grid < ((int64_t)1 << 31), "batch=%d x %lld passage tiles exceeds one launch", batch, (long long)tiles_m);
    int2 *cols = static_cast<int2 *>(ws);
    int32_t *cnt = reinterpret_cast<int32_t *>(cols + (size_t)batch * kMaxEx);
    hipLaunchKernelGGL(reco_cols_kernel, dim3((unsigned)ceil_div((int64_t)batch * kMaxEx, 256)), dim3(256), 0, s, ex_ptr_dev,
                       ex_idx_dev, ex_sign_dev, ex_ptr[batch], batch, rows, cols, cnt);
    HRAG_LAUNCH_CHECK();
    const int32_t third = split ? kdim / 3 : 0;
    if (dtype == HRAG_FP16)
        hipLaunchKernelGGL(reco_scores_kernel<true>, dim3((unsigned)grid), dim3(256), 0, s, emb, rows, kdim, third, cols, cnt,
                           batch, mode, out, ld, tn);
    else
        hipLaunchKernelGGL(reco_scores_kernel<false>, dim3((unsigned)grid), dim3(256), 0, s, emb, rows, kdim, third, cols, cnt,
                           batch, mode, out, ld, tn);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

// what every engine form refuses (include/hrag.h): a row shard, an engine without passage embeddings, the batch
hrag_status reco_check_engine(const hrag_engine *e, int32_t batch, const char *what) {
    HRAG_REQUIRE(e != nullptr, "engine is NULL");
    HRAG_REQUIRE(e->p_rows == e->n_passages && e->n_rows == e->V,
                 "%s on a row-shard engine: it holds a slice of the passage embeddings (recommend is served by the unsharded "
                 "engine only)", what);
    HRAG_REQUIRE(e->d_pemb != nullptr, "%s: the engine was created without passage embeddings (hrag_reco_scores_rows on the "
                                       "caller's rows)", what);
    HRAG_REQUIRE(batch >= 1 && batch <= e->max_batch, "batch %d outside [1, max_batch=%d]", batch, e->max_batch);
    return HRAG_OK;
}

}  // namespace
}  // namespace hrag

// ---- exports (include/hrag.h, recommend by example)
int64_t hrag_reco_workspace_bytes(int32_t batch) {
    if (batch < 1) return -1;
    return round_up((int64_t)batch * kMaxEx * (int64_t)sizeof(int2) + (int64_t)batch * (int64_t)sizeof(int32_t), 16);
}

hrag_status hrag_reco_rows(const float *ex_scores, int64_t ld, const int32_t *ex_ptr_dev, const int32_t *ex_sign_dev,
                           int32_t batch, int64_t n, int32_t mode, float *out, int64_t ld_out, hrag_stream stream) {
    HRAG_REQUIRE(ex_scores && ex_ptr_dev && ex_sign_dev && out, "NULL argument");
    HRAG_REQUIRE(batch >= 1 && batch <= 65535, "batch=%d outside [1, 65535]", batch);
    HRAG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "n=%lld outside [1, 2^31)", (long long)n);
    HRAG_REQUIRE(ld >= n && ld_out >= n, "ld=%lld / ld_out=%lld below n=%lld", (long long)ld, (long long)ld_out, (long long)n);
    HRAG_REQUIRE(reco_mode_ok(mode), "mode=%d: HRAG_RECO_BEST_SCORE (0) or HRAG_RECO_SUM_SCORES (1)", mode);
    hipLaunchKernelGGL(reco_rows_kernel, dim3((unsigned)ceil_div(n, 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                       ex_scores, ld, ex_ptr_dev, ex_sign_dev, n, mode, out, ld_out);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status hrag_reco_scores_rows(const uint16_t *emb, int64_t rows, int32_t kdim, int32_t dtype, int32_t split,
                                  const int32_t *ex_ptr, const int32_t *ex_ptr_dev, const int32_t *ex_idx_dev,
                                  const int32_t *ex_sign_dev, int32_t batch, int32_t mode, float *out, int64_t ld, void *ws,
                                  size_t ws_bytes, hrag_stream stream) {
    return launch_reco_scores(emb, rows, kdim, dtype, split, ex_ptr, ex_ptr_dev, ex_idx_dev, ex_sign_dev, batch, mode, out, ld, ws,
                              ws_bytes, (hipStream_t)stream);
}

hrag_status hrag_reco_scores(hrag_engine *e, const int32_t *ex_ptr, const int32_t *ex_ptr_dev, const int32_t *ex_idx_dev,
                             const int32_t *ex_sign_dev, int32_t batch, int32_t mode, float *out, int64_t ld, void *ws,
                             size_t ws_bytes, hrag_stream stream) {
    HRAG_TRY(reco_check_engine(e, batch, "hrag_reco_scores"));
    HRAG_ENGINE_CALL(e, stream);
    return launch_reco_scores(e->d_pemb, e->p_rows, e->kdim, e->emb_dtype, e->split ? 1 : 0, ex_ptr, ex_ptr_dev, ex_idx_dev,
                              ex_sign_dev, batch, mode, out, ld, ws, ws_bytes, (hipStream_t)stream);
}

hrag_status hrag_reco_query(hrag_engine *e, const int32_t *ex_ptr, const int32_t *ex_ptr_dev, const int32_t *ex_idx_dev,
                            const int32_t *ex_sign_dev, int32_t batch, uint16_t *q_out, float *q_f32_out, int32_t *flags_out,
                            hrag_stream stream) {
    HRAG_TRY(reco_check_engine(e, batch, "hrag_reco_query"));
    HRAG_TRY(reco_check_examples(ex_ptr, ex_ptr_dev, ex_idx_dev, ex_sign_dev, batch));
    HRAG_REQUIRE(q_out && flags_out, "NULL argument");
    HRAG_ENGINE_CALL(e, stream);
    const int32_t kind = e->split ? 2 : e->emb_dtype == HRAG_FP16 ? 1 : 0;
    hipLaunchKernelGGL(reco_query_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, e->d_pemb, e->p_rows, e->dim,
                       kind, ex_ptr_dev, ex_idx_dev, ex_sign_dev, ex_ptr[batch], q_out, q_f32_out, flags_out);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status hrag_reco_exclude(uint32_t *words, int64_t ld_words, int64_t n, const int32_t *ex_ptr_dev, const int32_t *ex_idx_dev,
                              const int32_t *ex_sign_dev, int32_t batch, hrag_stream stream) {
    HRAG_REQUIRE(words && ex_ptr_dev && ex_idx_dev, "NULL argument");
    HRAG_REQUIRE(batch >= 1, "batch=%d: at least 1", batch);
    HRAG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "n=%lld outside [1, 2^31)", (long long)n);
    HRAG_REQUIRE(ld_words >= (n + 31) / 32, "ld_words=%lld: one row per query of >= ceil(n / 32) = %lld words (expand a shared "
                 "row first)", (long long)ld_words, (long long)((n + 31) / 32));
    hipLaunchKernelGGL(reco_exclude_kernel, dim3((unsigned)ceil_div(batch, 256)), dim3(256), 0, (hipStream_t)stream, words,
                       ld_words, n, ex_ptr_dev, ex_idx_dev, ex_sign_dev, batch);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}
