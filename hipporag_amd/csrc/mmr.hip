// Diversified retrieval (include/hrag.h, "diversified retrieval": hrag_gram_rows / hrag_mmr_rows / hrag_mmr): Maximal
// Marginal Relevance over the c <= 1024 candidates a ranking returned, per query, without leaving the device.
//
// gram_gather_kernel<F16>: G[b][i][j] = the score hrag_sim_gemm gives for embedding row cand[b][i] against row cand[b][j]
// used as the query, for i <= j, and its mirror.  One 256-thread workgroup per (query, 64 x 64 tile of the upper triangle:
// tile_i <= tile_j).  The rows come straight from the embedding matrix by candidate id (16-byte loads; no gathered copy in
// memory) into LDS in 64-element k slices, rows padded to 144 bytes as sim_gemm.hip pads them; the MFMA chain IS
// sim_gemm_kernel's: v_mfma_f32_16x16x32, a lane feeds 8 consecutive k of one row for A and B alike, BK = 64 steps of two
// MFMAs in ascending k into one fp32 accumulator, the k tail zero-filled in 8-element chunks (a slice's second MFMA runs
// on zeros exactly where sim_gemm_kernel's does).  A = the tile_i slots (the "embedding" side), B = the tile_j slots (the
// "query" side); C/D layout col = lane & 15 (B slot), row = 4 * (lane >> 4) + reg (A slot).  On a split engine the stored
// row is [hi | lo | hi] and a query is [hi | hi | lo]: the B side reads the thirds of the stored row in the order
// (0, 2, 1).  An empty slot (id outside [0, rows)) is a zero row: +0.0 in its row and column.  The epilogue stores every
// element with slot_i <= slot_j at [i][j] and, off the diagonal, at [j][i]; the lower half of a diagonal tile is computed
// and dropped.  Columns c .. ld are not touched.  No atomics.
//
// mmr_select_kernel: one 256-thread workgroup per query, slot = tid + 256 * u for u < 4 (c <= 1024); relevance, penalty and
// the live flags stay in registers.  Step t: every live slot forms its value, the workgroup takes the arg-max of the
// 64-bit key (ordered value << 32 | ~slot: the ranking key of common.h with the tie going to the SMALLER slot) by
// wavefront shuffles and one LDS exchange across the four wavefronts (double-buffered: one barrier per step), the thread
// that owns the winner writes the outputs, and the next step begins with one coalesced read of row sim[winner] to fold
// into the penalties.  Plain vector stores only.
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

constexpr int kGramTile = 64;
constexpr int BK = 64;
constexpr int LDS_LD = BK + 8;  // 16-bit elements per LDS row (144 bytes, sim_gemm.hip)

// third: kdim / 3 on the split layout (the B side reads the thirds as (0, 2, 1)), 0 otherwise
template <bool F16>
__global__ __launch_bounds__(256) void gram_gather_kernel(const uint16_t *__restrict__ emb, int64_t rows, int32_t kdim,
                                                          int32_t third, const int32_t *__restrict__ cand, int32_t c,
                                                          float *__restrict__ out, int64_t ld, int32_t nt,
                                                          int32_t n_upper) {
    constexpr int MI = 2, NJ = 2;   // 2 x 2 wavefronts of 32 x 32
    __shared__ __attribute__((aligned(16))) uint16_t As[kGramTile][LDS_LD];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[kGramTile][LDS_LD];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t b = (int64_t)blockIdx.x / n_upper;
    int t = (int)((int64_t)blockIdx.x % n_upper), ti = 0;
    while (t >= nt - ti) {      // tile number -> (tile_i, tile_j >= tile_i), row by row of the upper triangle
        t -= nt - ti;
        ++ti;
    }
    const int tj = ti + t;
    const int32_t *ids = cand + (size_t)b * c;

    const int ld_row = tid >> 3;        // 0..31
    const int ld_chunk = (tid & 7) * 8; // element offset inside the BK slice
    const uint16_t *arow[2], *brow[2];  // the embedding row of this thread's slots (nullptr: an empty slot)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int sa = ti * kGramTile + ld_row + 32 * p, sb = tj * kGramTile + ld_row + 32 * p;
        const int32_t ia = sa < c ? ids[sa] : -1, ib = sb < c ? ids[sb] : -1;
        arow[p] = (ia >= 0 && (int64_t)ia < rows) ? emb + (size_t)ia * kdim : nullptr;
        brow[p] = (ib >= 0 && (int64_t)ib < rows) ? emb + (size_t)ib * kdim : nullptr;
    }

    uint4 ra[2], rb[2];
    auto load_tile = [&](int k0) {
        const int kk = k0 + ld_chunk;
        int kb = kk;                    // where the B ("query") side finds logical position kk in a stored row
        if (third > 0) kb = kk < third ? kk : kk < 2 * third ? kk + third : kk - third;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            ra[p] = rb[p] = make_uint4(0, 0, 0, 0);
            if (kk < kdim) {
                if (arow[p]) ra[p] = *reinterpret_cast<const uint4 *>(arow[p] + kk);
                if (brow[p]) rb[p] = *reinterpret_cast<const uint4 *>(brow[p] + kb);
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            *reinterpret_cast<uint4 *>(&As[ld_row + 32 * p][ld_chunk]) = ra[p];
            *reinterpret_cast<uint4 *>(&Bs[ld_row + 32 * p][ld_chunk]) = rb[p];
        }
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
            uint4 a[MI], bq[NJ];
            const int kcol = s * 32 + 8 * (lane >> 4);
#pragma unroll
            for (int i = 0; i < MI; ++i)
                a[i] = *reinterpret_cast<const uint4 *>(&As[(wm * MI + i) * 16 + (lane & 15)][kcol]);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                bq[j] = *reinterpret_cast<const uint4 *>(&Bs[(wn * NJ + j) * 16 + (lane & 15)][kcol]);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = mfma32<F16>(a[i], bq[j], acc[i][j]);
        }
        __syncthreads();
    }

    // epilogue: a lane owns A slots si .. si + 3 of B slot sj for every (i, j) fragment
    float *g = out + (size_t)b * c * ld;
    const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int si = ti * kGramTile + (wm * MI + i) * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int sj = tj * kGramTile + (wn * NJ + j) * 16 + (lane & 15);
            if (sj >= c) continue;
            const f32x4 v = acc[i][j];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (si + r <= sj) g[(size_t)(si + r) * ld + sj] = v[r];     // (si + r <= sj < c)
            float *mir = g + (size_t)sj * ld + si;                           // the mirror: row sj, columns si .. si + 3
            if (vec && si + 3 < sj) {
                *reinterpret_cast<float4 *>(mir) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (si + r < sj) mir[r] = v[r];
            }
        }
    }
}

constexpr int kMmrThreads = 256;
constexpr int kMmrSlots = HRAG_MMR_MAX_CANDIDATES / kMmrThreads;   // slots per thread
static_assert(kMmrSlots * kMmrThreads == HRAG_MMR_MAX_CANDIDATES, "slots per thread");

__device__ __forceinline__ float canonical(float v) { return v != v ? __uint_as_float(0x7fc00000u) : v + 0.0f; }

// n_ids > 0: an id >= n_ids is an empty slot too (the engine call); n_ids <= 0: negative ids only
__global__ __launch_bounds__(kMmrThreads) void mmr_select_kernel(const float *__restrict__ score,
                                                                 const int32_t *__restrict__ cand,
                                                                 const float *__restrict__ sim, int64_t ld, int32_t c,
                                                                 int32_t k, float lambda, int32_t normalize, int64_t n_ids,
                                                                 int32_t *__restrict__ sel_out, int32_t *__restrict__ idx_out,
                                                                 float *__restrict__ score_out,
                                                                 float *__restrict__ value_out) {
    __shared__ uint64_t red[2][4];
    __shared__ float redf[8];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *srow = score + (size_t)b * c;
    const int32_t *irow = cand + (size_t)b * c;
    const float *g = sim + (size_t)b * c * ld;

    float s[kMmrSlots], rel[kMmrSlots], pen[kMmrSlots];
    int32_t id[kMmrSlots];
    bool live[kMmrSlots];
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < kMmrSlots; ++u) {
        const int slot = tid + kMmrThreads * u;
        s[u] = 0.f; pen[u] = 0.f; id[u] = -1; live[u] = false;
        if (slot < c) {
            id[u] = irow[slot];
            s[u] = srow[slot];
            live[u] = id[u] >= 0 && (n_ids <= 0 || (int64_t)id[u] < n_ids);
            if (live[u]) {
                mn = fminf(mn, s[u]);
                mx = fmaxf(mx, s[u]);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) {
        redf[wave] = mn;
        redf[4 + wave] = mx;
    }
    __syncthreads();
    mn = fminf(fminf(redf[0], redf[1]), fminf(redf[2], redf[3]));
    mx = fmaxf(fmaxf(redf[4], redf[5]), fmaxf(redf[6], redf[7]));
    const float range = mx - mn;
#pragma unroll
    for (int u = 0; u < kMmrSlots; ++u)
        rel[u] = !normalize ? s[u] : mx == mn ? 1.0f : __fdiv_rn(s[u] - mn, range);   // misc_utils.py:130-139

    const double dl = (double)lambda, dm = (double)(1.0f - lambda);
    int last = -1;
    for (int t = 0; t < k; ++t) {
        uint64_t best = 0;      // keys are > 0 (common.h rank_key): 0 = no live slot
#pragma unroll
        for (int u = 0; u < kMmrSlots; ++u) {
            if (!live[u]) continue;
            const int slot = tid + kMmrThreads * u;
            float v;
            if (t == 0) {
                v = (float)(dl * (double)rel[u]);
            } else {
                const float gv = g[(size_t)last * ld + slot];
                pen[u] = t == 1 ? gv : fmaxf(pen[u], gv);
                v = (float)(dl * (double)rel[u] - dm * (double)pen[u]);   // both products exact in fp64
            }
            const uint64_t key = rank_key(v, ~(uint32_t)slot);
            best = key > best ? key : best;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t other = __shfl_xor((unsigned long long)best, o, 64);
            best = other > best ? other : best;
        }
        if (lane == 0) red[t & 1][wave] = best;
        __syncthreads();        // red[t & 1] is written again at step t + 2, behind the barrier of step t + 1
        best = red[t & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) best = red[t & 1][w] > best ? red[t & 1][w] : best;
        if (best == 0) {        // the non-empty slots ran out: -1 / -1 / 0 / 0 from here on
            for (int j = t + tid; j < k; j += kMmrThreads) {
                if (sel_out) sel_out[(size_t)b * k + j] = -1;
                idx_out[(size_t)b * k + j] = -1;
                score_out[(size_t)b * k + j] = 0.f;
                value_out[(size_t)b * k + j] = 0.f;
            }
            break;
        }
        last = (int)~(uint32_t)best;
        if ((last & (kMmrThreads - 1)) == tid) {
#pragma unroll
            for (int u = 0; u < kMmrSlots; ++u)
                if (u == (last >> 8)) {
                    live[u] = false;
                    if (sel_out) sel_out[(size_t)b * k + t] = last;
                    idx_out[(size_t)b * k + t] = id[u];
                    score_out[(size_t)b * k + t] = canonical(s[u]);
                    value_out[(size_t)b * k + t] = ordered_to_f32((uint32_t)(best >> 32));
                }
        }
    }
}
static_assert(kMmrThreads == 256, "the owner of a slot is slot & 255, its register slot >> 8");

bool lambda_ok(float lambda) { return lambda >= 0.f && lambda <= 1.f; }   // false for NaN

}  // namespace

hrag_status launch_gram_rows(const uint16_t *emb, int64_t rows, int32_t kdim, int32_t dtype, int32_t split,
                             const int32_t *cand, int32_t batch, int32_t c, float *out, int64_t ld, hipStream_t s) {
    HRAG_REQUIRE(emb && cand && out, "NULL argument");
    HRAG_REQUIRE(dtype == HRAG_BF16 || dtype == HRAG_FP16, "dtype=%d: HRAG_BF16 (0) or HRAG_FP16 (1), the element type of the rows",
                 dtype);
    HRAG_REQUIRE(rows >= 1 && rows < ((int64_t)1 << 31), "rows=%lld outside [1, 2^31)", (long long)rows);
    HRAG_REQUIRE(kdim > 0 && kdim % 8 == 0, "kdim %d must be a positive multiple of 8", kdim);
    HRAG_REQUIRE(!split || kdim % 24 == 0, "kdim %d of a split layout must be 3 * dim with dim a multiple of 8", kdim);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(emb) & 15) == 0, "the embedding rows must be 16-byte aligned");
    HRAG_REQUIRE(batch >= 1, "batch=%d: at least 1", batch);
    HRAG_REQUIRE(c >= 1 && c <= HRAG_MMR_MAX_CANDIDATES, "c=%d outside [1, HRAG_MMR_MAX_CANDIDATES=%d]", c,
                 HRAG_MMR_MAX_CANDIDATES);
    HRAG_REQUIRE(ld >= c, "ld=%lld below c=%d", (long long)ld, c);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "the output must be 4-byte aligned");
    const int32_t nt = (int32_t)ceil_div(c, kGramTile), n_upper = nt * (nt + 1) / 2;
    const int64_t grid = (int64_t)batch * n_upper;
    HRAG_REQUIRE(grid < ((int64_t)1 << 31), "batch=%d x %d tiles exceeds one launch", batch, n_upper);
    const int32_t third = split ? kdim / 3 : 0;
    if (dtype == HRAG_FP16)
        hipLaunchKernelGGL(gram_gather_kernel<true>, dim3((unsigned)grid), dim3(256), 0, s, emb, rows, kdim, third, cand, c,
                           out, ld, nt, n_upper);
    else
        hipLaunchKernelGGL(gram_gather_kernel<false>, dim3((unsigned)grid), dim3(256), 0, s, emb, rows, kdim, third, cand, c,
                           out, ld, nt, n_upper);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status launch_mmr_rows(const float *score, const int32_t *cand, const float *sim, int64_t ld, int32_t batch, int32_t c,
                            int32_t k, float lambda, int32_t normalize, int64_t n_ids, int32_t *sel_out, int32_t *idx_out,
                            float *score_out, float *value_out, hipStream_t s) {
    HRAG_REQUIRE(score && cand && sim && idx_out && score_out && value_out, "NULL argument");
    HRAG_REQUIRE(batch >= 1, "batch=%d: at least 1", batch);
    HRAG_REQUIRE(c >= 1 && c <= HRAG_MMR_MAX_CANDIDATES, "c=%d outside [1, HRAG_MMR_MAX_CANDIDATES=%d]", c,
                 HRAG_MMR_MAX_CANDIDATES);
    HRAG_REQUIRE(k >= 1 && k <= c, "k=%d outside [1, c=%d]", k, c);
    HRAG_REQUIRE(ld >= c, "ld=%lld below c=%d", (long long)ld, c);
    HRAG_REQUIRE(lambda_ok(lambda), "lambda=%g outside [0, 1]", (double)lambda);
    hipLaunchKernelGGL(mmr_select_kernel, dim3((unsigned)batch), dim3(kMmrThreads), 0, s, score, cand, sim, ld, c, k, lambda,
                       normalize, n_ids, sel_out, idx_out, score_out, value_out);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

}  // namespace hrag

// ---- exports (include/hrag.h, diversified retrieval)
hrag_status hrag_gram_rows(const uint16_t *emb, int64_t rows, int32_t kdim, int32_t dtype, int32_t split, const int32_t *cand_idx,
                           int32_t batch, int32_t c, float *out, int64_t ld, hrag_stream stream) {
    return launch_gram_rows(emb, rows, kdim, dtype, split, cand_idx, batch, c, out, ld, (hipStream_t)stream);
}

hrag_status hrag_mmr_rows(const float *score, const int32_t *cand_idx, const float *sim, int64_t ld, int32_t batch, int32_t c,
                          int32_t k, float lambda, int32_t normalize, int32_t *sel_out, int32_t *idx_out, float *score_out,
                          float *value_out, hrag_stream stream) {
    HRAG_REQUIRE(sel_out != nullptr, "NULL argument");
    return launch_mmr_rows(score, cand_idx, sim, ld, batch, c, k, lambda, normalize, 0, sel_out, idx_out, score_out, value_out,
                           (hipStream_t)stream);
}

int64_t hrag_mmr_workspace_bytes(int32_t batch, int32_t c) {
    if (batch < 1 || c < 1 || c > HRAG_MMR_MAX_CANDIDATES) return -1;
    return (int64_t)batch * c * round_up(c, 4) * (int64_t)sizeof(float);
}

hrag_status hrag_mmr(hrag_engine *e, const int32_t *cand_idx, const float *cand_score, int32_t batch, int32_t c, int32_t k,
                     float lambda, int32_t normalize, int32_t *idx_out, float *score_out, float *value_out, void *workspace,
                     size_t workspace_bytes, hrag_stream stream) {
    return hrag_mmr_sel(e, cand_idx, cand_score, batch, c, k, lambda, normalize, nullptr, idx_out, score_out, value_out,
                        workspace, workspace_bytes, stream);
}

hrag_status hrag_mmr_sel(hrag_engine *e, const int32_t *cand_idx, const float *cand_score, int32_t batch, int32_t c, int32_t k,
                         float lambda, int32_t normalize, int32_t *sel_out, int32_t *idx_out, float *score_out,
                         float *value_out, void *workspace, size_t workspace_bytes, hrag_stream stream) {
    HRAG_REQUIRE(e != nullptr, "engine is NULL");
    HRAG_REQUIRE(e->p_rows == e->n_passages && e->n_rows == e->V,
                 "hrag_mmr on a row-shard engine: it holds a slice of the passage embeddings (diversified retrieval is served "
                 "by the unsharded engine only)");
    HRAG_REQUIRE(e->d_pemb != nullptr, "the engine was created without passage embeddings: hrag_gram_rows + hrag_mmr_rows on "
                                       "the caller's rows");
    HRAG_REQUIRE(cand_idx && cand_score && idx_out && score_out && value_out, "NULL argument");
    HRAG_REQUIRE(batch >= 1 && batch <= e->max_batch, "batch %d outside [1, max_batch=%d]", batch, e->max_batch);
    HRAG_REQUIRE(c >= 1 && c <= HRAG_MMR_MAX_CANDIDATES, "c=%d outside [1, HRAG_MMR_MAX_CANDIDATES=%d]", c,
                 HRAG_MMR_MAX_CANDIDATES);
    HRAG_REQUIRE(k >= 1 && k <= c, "k=%d outside [1, c=%d]", k, c);
    HRAG_REQUIRE(lambda_ok(lambda), "lambda=%g outside [0, 1]", (double)lambda);
    const int64_t need = hrag_mmr_workspace_bytes(batch, c);
    HRAG_REQUIRE(workspace && (int64_t)workspace_bytes >= need, "workspace of %lld bytes, %lld needed (hrag_mmr_workspace_bytes)",
                 (long long)workspace_bytes, (long long)need);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "the workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    HRAG_ENGINE_CALL(e, stream);
    float *gram = static_cast<float *>(workspace);
    const int64_t ld = round_up(c, 4);
    HRAG_TRY(launch_gram_rows(e->d_pemb, e->p_rows, e->kdim, e->emb_dtype, e->split ? 1 : 0, cand_idx, batch, c, gram, ld, s));
    return launch_mmr_rows(cand_score, cand_idx, gram, ld, batch, c, k, lambda, normalize, e->n_passages, sel_out, idx_out,
                           score_out, value_out, s);
}
