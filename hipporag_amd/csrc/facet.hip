// Facets (include/hrag.h, "facets": hrag_payload_facet / hrag_payload_facet_ids / hrag_payload_facet_ws_bytes): per-value
// counts of one payload column over the passages a doc filter allows, or over a list of passage ids.
//
// facet_count_kernel: one 256-thread workgroup per (query, window of HRAG_FACET_WINDOW bins, split of the passage range).
// The workgroup keeps the int32 histogram of its window in LDS (16 KB; a list of at most 1024 edges is copied there too, 8 KB,
// so that the binary search of a short range facet never leaves the CU) and walks its split in tiles of HRAG_PAY_TILE
// passages with payload_filter_kernel's access pattern: thread t takes the passages tile0 + 256 u + t, u = 0 .. 7 --
// coalesced 8-byte column reads, a filter word and a presence word shared by 32 lanes.  The bin of a passage is
// facet_bin.h's (the ids kernel maps a passage with the same code); a bin inside the window adds 1 to its LDS word.
// Window 0 also keeps "other" and "missing".  With one split the workgroup stores its window straight into counts_out,
// else into its slice of the workspace [batch, n_splits, n_bins + 2], and facet_reduce_kernel sums the slices in split
// order.  No global atomics, no memset: every output word (and every workspace word that is read) is written exactly
// once.  The adds are integer, so their order does not matter: the counts are exact and the same on every run.
//
// The skewed column -- one value holds a third of the corpus, or every passage is missing -- would send dozens of the 64
// lanes of a wave instruction to ONE LDS word, and the LDS serialises same-address atomics of an instruction.  Of the two
// plans the ballot step was chosen over per-wavefront sub-histograms: sub-histograms cost 64 KB of LDS per workgroup (two
// workgroups per CU instead of eight) and remove the contention BETWEEN wavefronts only -- the 64 lanes that collide sit in
// one wavefront.  The ballot step (hist_add): a wavefront carries a guess g of its hot bin in a scalar register; the lanes
// whose bin is g are counted by one ballot and popcount into a scalar accumulator instead of adding to LDS; the other
// lanes add with ds_add.  When fewer than kHotKeep lanes matched, the guess moves to the bin of the first lane that did not
// match (the accumulator is flushed by one lane first): a bin that holds a third of the passages is picked after about
// three steps and then stays.  "other" and "missing" are always counted by ballots into scalar registers and reach LDS once
// per wavefront.  On a uniform column the step costs three ballots and a lane read per wave instruction.
//
// facet_ids_kernel: one workgroup per (query, window); the k ids read coalesced, 256 at a time, the column gathered at each
// id inside [0, n_passages); the same histogram, the same hist_add.
//
// facet_splits: how many splits hrag_payload_facet uses -- a pure function of (n_passages, n_bins, batch), which is what
// hrag_payload_facet_ws_bytes reports.
#include "facet_bin.h"

namespace hrag {
namespace {

constexpr int kFacetThreads = 256;
constexpr int kFacetPer = HRAG_PAY_TILE / kFacetThreads;       // passages per thread and tile
constexpr int kHotKeep = 8;                                    // matches of the guess below which it moves
constexpr int64_t kFacetFill = 1024;      // workgroups that fill the machine: four per CU (measured: DESIGN.md section 4, facets)
static_assert(kFacetPer * kFacetThreads == HRAG_PAY_TILE, "a tile is a whole number of passages per thread");
static_assert(HRAG_FACET_MAX_BINS + 2 < (1 << 30), "bins are int32");

// n_splits of (n_passages, n_bins, batch): 1 when the (query, window) pairs fill the machine; else about kFacetFill
// workgroups, at most one split per tile, the tiles dealt in equal runs
int32_t facet_splits(int64_t n, int64_t n_bins, int32_t batch) {
    const int64_t n_tiles = ceil_div(n, HRAG_PAY_TILE), base = (int64_t)batch * ceil_div(n_bins, HRAG_FACET_WINDOW);
    if (base >= kFacetFill) return 1;
    const int64_t want = std::min(ceil_div(kFacetFill, base), n_tiles);
    const int64_t per = ceil_div(n_tiles, want);
    return (int32_t)ceil_div(n_tiles, per);
}

// the wave-uniform state of hist_add
struct WaveAcc {
    int32_t g, acc, other, missing;
};

// One wave instruction's worth of bins into the window's histogram (file header).  Every lane of the wavefront calls it;
// live: the lane has a passage to count; bin: facet_bin's result (anything when !live).
__device__ __forceinline__ void hist_add(int32_t *s_hist, WaveAcc &a, bool live, int32_t bin, int32_t n_bins, int32_t win0,
                                         int32_t wlen, int lane) {
    a.other += __popcll(__ballot(live && bin == n_bins));
    a.missing += __popcll(__ballot(live && bin == n_bins + 1));
    const int32_t local = bin - win0;
    const bool in = live && bin < n_bins && local >= 0 && local < wlen;
    const int c = __popcll(__ballot(in && local == a.g));
    a.acc += c;
    const bool rest = in && local != a.g;
    if (rest) atomicAdd(&s_hist[local], 1);          // (0 <= local < wlen <= HRAG_FACET_WINDOW)
    if (c < kHotKeep) {                              // uniform over the wavefront
        const unsigned long long r = __ballot(rest);
        if (r) {
            if (a.acc > 0 && lane == 0) atomicAdd(&s_hist[a.g], a.acc);      // (acc > 0: g was some lane's local)
            a.g = __builtin_amdgcn_readlane(local, __builtin_amdgcn_readfirstlane(__ffsll(r) - 1));
            a.acc = 0;
        }
    }
}

// what a wavefront still holds in registers, into LDS: once per wavefront
__device__ __forceinline__ void hist_flush(int32_t *s_hist, int32_t *s_tail, const WaveAcc &a, bool tail, int lane) {
    if (lane != 0) return;
    if (a.acc > 0) atomicAdd(&s_hist[a.g], a.acc);
    if (tail) {
        if (a.other) atomicAdd(&s_tail[0], a.other);
        if (a.missing) atomicAdd(&s_tail[1], a.missing);
    }
}

// blockIdx.x = (b * n_win + win) * n_splits + split.  dst row of (b, split): out + b * ld_b + split * ld_s
__global__ __launch_bounds__(kFacetThreads) void facet_count_kernel(
    const PayCol *__restrict__ cols, int32_t col, int32_t kind, int64_t lo, const int64_t *__restrict__ edges, int32_t m,
    int32_t n_bins, int64_t n, const uint32_t *__restrict__ words, int64_t ld_w, int32_t *__restrict__ out, int64_t ld_b,
    int64_t ld_s, int32_t n_win, int32_t n_splits, int32_t tiles_per_split, int32_t n_tiles) {
    __shared__ int32_t s_hist[HRAG_FACET_WINDOW];
    __shared__ int32_t s_tail[2];
    __shared__ int64_t s_edges[kFacetLdsEdges];

    const int tid = threadIdx.x, lane = tid & 63;
    const int32_t split = (int32_t)(blockIdx.x % (uint32_t)n_splits);
    const int32_t win = (int32_t)((blockIdx.x / (uint32_t)n_splits) % (uint32_t)n_win);
    const int64_t b = (int64_t)(blockIdx.x / (uint32_t)n_splits) / n_win;
    const int32_t win0 = win * HRAG_FACET_WINDOW;
    const int32_t wlen = n_bins - win0 < HRAG_FACET_WINDOW ? n_bins - win0 : HRAG_FACET_WINDOW;

    for (int i = tid; i < wlen; i += kFacetThreads) s_hist[i] = 0;
    if (tid < 2) s_tail[tid] = 0;
    const FacetRec rec = stage_facet(cols, col, kind, lo, edges, m, n_bins);
    stage_edges(s_edges, rec, tid, kFacetThreads);
    __syncthreads();

    const uint32_t *row = words ? words + (size_t)b * ld_w : nullptr;      // ld_w 0: one row for the batch
    WaveAcc acc{-1, 0, 0, 0};
    const int32_t t_end = (split + 1) * tiles_per_split < n_tiles ? (split + 1) * tiles_per_split : n_tiles;
    for (int32_t t = split * tiles_per_split; t < t_end; ++t) {
        const int64_t tile0 = (int64_t)t * HRAG_PAY_TILE;
        int32_t bin[kFacetPer];
        uint32_t live = 0;
#pragma unroll
        for (int u = 0; u < kFacetPer; ++u) {
            const int64_t p = tile0 + kFacetThreads * u + tid;
            bool ok = p < n;                                     // bits at or above n_passages are never looked at
            if (ok && row) ok = ((row[p >> 5] >> (p & 31)) & 1u) != 0;
            bin[u] = ok ? facet_bin(rec, s_edges, p) : 0;
            live |= (uint32_t)ok << u;
        }
#pragma unroll
        for (int u = 0; u < kFacetPer; ++u) hist_add(s_hist, acc, (live >> u) & 1u, bin[u], n_bins, win0, wlen, lane);
    }
    hist_flush(s_hist, s_tail, acc, win == 0, lane);
    __syncthreads();

    int32_t *dst = out + (size_t)b * ld_b + (size_t)split * ld_s;
    for (int i = tid; i < wlen; i += kFacetThreads) dst[win0 + i] = s_hist[i];
    if (win == 0 && tid < 2) dst[n_bins + tid] = s_tail[tid];
}

// counts_out[b, v] = the sum over the splits, in split order, of ws[b, split, v]; v < n_bins + 2
__global__ __launch_bounds__(kFacetThreads) void facet_reduce_kernel(const int32_t *__restrict__ ws, int32_t n_splits,
                                                                     int32_t width, int32_t *__restrict__ out, int64_t ld_c) {
    const int64_t b = blockIdx.y;
    const int32_t v = (int32_t)(blockIdx.x * kFacetThreads + threadIdx.x);
    if (v >= width) return;
    const int32_t *src = ws + (size_t)b * n_splits * width + v;
    int32_t c = 0;
    for (int32_t s = 0; s < n_splits; ++s) c += src[(size_t)s * width];
    out[(size_t)b * ld_c + v] = c;
}

// blockIdx.x = b * n_win + win
__global__ __launch_bounds__(kFacetThreads) void facet_ids_kernel(
    const PayCol *__restrict__ cols, int32_t col, int32_t kind, int64_t lo, const int64_t *__restrict__ edges, int32_t m,
    int32_t n_bins, int64_t n, const int32_t *__restrict__ idx, int64_t ld_i, int32_t k, int32_t *__restrict__ out,
    int64_t ld_c, int32_t n_win) {
    __shared__ int32_t s_hist[HRAG_FACET_WINDOW];
    __shared__ int32_t s_tail[2];
    __shared__ int64_t s_edges[kFacetLdsEdges];

    const int tid = threadIdx.x, lane = tid & 63;
    const int32_t win = (int32_t)(blockIdx.x % (uint32_t)n_win);
    const int64_t b = blockIdx.x / (uint32_t)n_win;
    const int32_t win0 = win * HRAG_FACET_WINDOW;
    const int32_t wlen = n_bins - win0 < HRAG_FACET_WINDOW ? n_bins - win0 : HRAG_FACET_WINDOW;

    for (int i = tid; i < wlen; i += kFacetThreads) s_hist[i] = 0;
    if (tid < 2) s_tail[tid] = 0;
    const FacetRec rec = stage_facet(cols, col, kind, lo, edges, m, n_bins);
    stage_edges(s_edges, rec, tid, kFacetThreads);
    __syncthreads();

    const int32_t *ids = idx + (size_t)b * ld_i;
    WaveAcc acc{-1, 0, 0, 0};
    for (int32_t base = 0; base < k; base += kFacetThreads) {       // uniform: every lane reaches every hist_add
        const int32_t i = base + tid;
        const int64_t p = i < k ? (int64_t)ids[i] : -1;
        const bool ok = p >= 0 && p < n;                            // the -1 padding and any other id outside: skipped
        hist_add(s_hist, acc, ok, ok ? facet_bin(rec, s_edges, p) : 0, n_bins, win0, wlen, lane);
    }
    hist_flush(s_hist, s_tail, acc, win == 0, lane);
    __syncthreads();

    int32_t *dst = out + (size_t)b * ld_c;
    for (int i = tid; i < wlen; i += kFacetThreads) dst[win0 + i] = s_hist[i];
    if (win == 0 && tid < 2) dst[n_bins + tid] = s_tail[tid];
}

// the host rules both calls share
hrag_status facet_validate(const hrag_payload *pay, const hrag_facet_spec *spec, int32_t batch, const int32_t *counts_out,
                           int64_t ld_c) {
    HRAG_REQUIRE(pay != nullptr, "the payload index is NULL");
    HRAG_REQUIRE(spec != nullptr, "spec is NULL");
    HRAG_REQUIRE(counts_out != nullptr, "counts_out_dev is NULL");
    HRAG_REQUIRE(batch >= 1 && batch <= 65535, "batch=%d outside [1, 65535]", batch);
    HRAG_REQUIRE(spec->column >= 0 && spec->column < pay->n_cols, "spec.column=%d outside the index's [0, %d)", spec->column,
                 pay->n_cols);
    HRAG_REQUIRE(spec->kind == HRAG_FACET_CODES || spec->kind == HRAG_FACET_EDGES, "spec.kind=%d is unknown", spec->kind);
    HRAG_REQUIRE(spec->kind != HRAG_FACET_CODES || pay->col_type[(size_t)spec->column] == HRAG_PAY_I64,
                 "spec.kind HRAG_FACET_CODES on the F64 column %d (I64 columns only)", spec->column);
    HRAG_REQUIRE(spec->n_bins >= 1 && spec->n_bins <= HRAG_FACET_MAX_BINS, "spec.n_bins=%lld outside [1, %d]",
                 (long long)spec->n_bins, HRAG_FACET_MAX_BINS);
    if (spec->kind == HRAG_FACET_EDGES) {
        HRAG_REQUIRE(spec->n_edges >= 0 && spec->n_bins == spec->n_edges + 1, "spec.n_bins=%lld is not spec.n_edges + 1 = %lld",
                     (long long)spec->n_bins, (long long)spec->n_edges + 1);
        HRAG_REQUIRE(spec->n_edges == 0 || spec->edges_dev, "spec.edges_dev is NULL with n_edges=%lld", (long long)spec->n_edges);
        HRAG_REQUIRE((reinterpret_cast<uintptr_t>(spec->edges_dev) & 7) == 0, "spec.edges_dev must be 8-byte aligned");
    }
    HRAG_REQUIRE(ld_c >= spec->n_bins + 2, "ld_c=%lld below n_bins + 2 = %lld", (long long)ld_c, (long long)spec->n_bins + 2);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(counts_out) & 3) == 0, "counts_out_dev must be 4-byte aligned");
    return HRAG_OK;
}

}  // namespace
}  // namespace hrag

using namespace hrag;

// ---- exports (include/hrag.h, facets)
hrag_status hrag_payload_facet_ws_bytes(const hrag_payload *pay, int64_t n_bins, int32_t batch, int64_t *out) {
    HRAG_REQUIRE(out != nullptr, "out is NULL");
    *out = 0;
    HRAG_REQUIRE(pay != nullptr, "the payload index is NULL");
    HRAG_REQUIRE(n_bins >= 1 && n_bins <= HRAG_FACET_MAX_BINS, "n_bins=%lld outside [1, %d]", (long long)n_bins, HRAG_FACET_MAX_BINS);
    HRAG_REQUIRE(batch >= 1 && batch <= 65535, "batch=%d outside [1, 65535]", batch);
    const int32_t n_splits = facet_splits(pay->n_passages, n_bins, batch);
    *out = n_splits > 1 ? (int64_t)sizeof(int32_t) * batch * n_splits * (n_bins + 2) : 0;
    return HRAG_OK;
}

hrag_status hrag_payload_facet(const hrag_payload *pay, const hrag_facet_spec *spec, const uint32_t *words_dev, int64_t ld_w,
                               int32_t batch, int32_t *counts_out_dev, int64_t ld_c, void *ws_dev, int64_t ws_bytes,
                               hrag_stream stream) {
    HRAG_TRY(facet_validate(pay, spec, batch, counts_out_dev, ld_c));
    const int64_t W = ceil_div(pay->n_passages, 32);
    HRAG_REQUIRE(words_dev == nullptr || ld_w == 0 || ld_w >= W,
                 "ld_w=%lld: 0 (one row for the batch) or >= ceil(n_passages / 32) = %lld", (long long)ld_w, (long long)W);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(words_dev) & 3) == 0, "words_dev must be 4-byte aligned");
    const int32_t n_bins = (int32_t)spec->n_bins;
    const int32_t n_splits = facet_splits(pay->n_passages, n_bins, batch);
    const int64_t need = n_splits > 1 ? (int64_t)sizeof(int32_t) * batch * n_splits * (n_bins + 2) : 0;
    HRAG_REQUIRE(ws_bytes >= need, "ws_bytes=%lld below hrag_payload_facet_ws_bytes = %lld", (long long)ws_bytes, (long long)need);
    HRAG_REQUIRE(need == 0 || ws_dev, "ws_dev is NULL with %lld bytes of workspace needed", (long long)need);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(ws_dev) & 3) == 0, "ws_dev must be 4-byte aligned");
    const int64_t n_tiles = ceil_div(pay->n_passages, HRAG_PAY_TILE), n_win = ceil_div(n_bins, HRAG_FACET_WINDOW);
    const int64_t per = ceil_div(n_tiles, n_splits);
    const int64_t grid = (int64_t)batch * n_win * n_splits;
    HRAG_REQUIRE(grid < ((int64_t)1 << 31), "batch=%d x %lld windows x %d splits exceeds one launch", batch, (long long)n_win, n_splits);
    const bool edges = spec->kind == HRAG_FACET_EDGES;
    const int64_t width = (int64_t)n_bins + 2;
    hipLaunchKernelGGL(facet_count_kernel, dim3((unsigned)grid), dim3(kFacetThreads), 0, (hipStream_t)stream, pay->d_cols,
                       spec->column, spec->kind, spec->lo, edges ? static_cast<const int64_t *>(spec->edges_dev) : nullptr,
                       edges ? (int32_t)spec->n_edges : 0, n_bins, pay->n_passages, words_dev, words_dev ? ld_w : 0,
                       n_splits > 1 ? static_cast<int32_t *>(ws_dev) : counts_out_dev, n_splits > 1 ? n_splits * width : ld_c,
                       n_splits > 1 ? width : 0, (int32_t)n_win, n_splits, (int32_t)per, (int32_t)n_tiles);
    HRAG_LAUNCH_CHECK();
    if (n_splits > 1) {
        hipLaunchKernelGGL(facet_reduce_kernel, dim3((unsigned)ceil_div(width, kFacetThreads), (unsigned)batch),
                           dim3(kFacetThreads), 0, (hipStream_t)stream, static_cast<const int32_t *>(ws_dev), n_splits,
                           (int32_t)width, counts_out_dev, ld_c);
        HRAG_LAUNCH_CHECK();
    }
    return HRAG_OK;
}

hrag_status hrag_payload_facet_ids(const hrag_payload *pay, const hrag_facet_spec *spec, const int32_t *idx_dev, int64_t ld_i,
                                   int32_t k, int32_t batch, int32_t *counts_out_dev, int64_t ld_c, hrag_stream stream) {
    HRAG_TRY(facet_validate(pay, spec, batch, counts_out_dev, ld_c));
    HRAG_REQUIRE(idx_dev != nullptr, "idx_dev is NULL");
    HRAG_REQUIRE(k >= 1, "k=%d: at least 1", k);
    HRAG_REQUIRE(ld_i >= k, "ld_i=%lld below k=%d", (long long)ld_i, k);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(idx_dev) & 3) == 0, "idx_dev must be 4-byte aligned");
    const int32_t n_bins = (int32_t)spec->n_bins;
    const int64_t n_win = ceil_div(n_bins, HRAG_FACET_WINDOW);
    const int64_t grid = (int64_t)batch * n_win;
    const bool edges = spec->kind == HRAG_FACET_EDGES;
    hipLaunchKernelGGL(facet_ids_kernel, dim3((unsigned)grid), dim3(kFacetThreads), 0, (hipStream_t)stream, pay->d_cols,
                       spec->column, spec->kind, spec->lo, edges ? static_cast<const int64_t *>(spec->edges_dev) : nullptr,
                       edges ? (int32_t)spec->n_edges : 0, n_bins, pay->n_passages, idx_dev, ld_i, k, counts_out_dev, ld_c,
                       (int32_t)n_win);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}
