// K2 -- entity ("phrase") seeds of the reset vector: 32 lanes per query, one per (kept fact, side).
//
// Restates the array-level effect of graph_search_with_fact_entities
// (reference src/hipporag/HippoRAG.py:1574-1623) + get_top_k_weights (:1505-1542):
//   for every kept fact (filter order) and for subject, then object:
//       vertex absent (-1)                                  -> skip              (:1595-1597)
//       w = fact_score / num_chunks[vertex] if num_chunks>0 -> fp32 division     (:1598-1601)
//       phrase_weights[vertex] += w ; number_of_occurs[vertex] += 1  (fp64)      (:1603-1604)
//   phrase_weights /= number_of_occurs                                           (:1608)
//   keep the link_top_k heaviest phrases (stable: ties keep first-occurrence order; the reference
//   order is that of a Python set, i.e. undefined); a NaN mean ranks above every number, like the
//   top-k's NaN (include/hrag.h)                                                 (:1528)
//   flag bit2 when a kept phrase has weight exactly +-0 -- the reference's
//   assert np.count_nonzero(...) == len(linking_score_map) would fire            (:1541)
//   seed_w is stored sanitised: NaN / negative (and -0) -> +0, as the reference's reset vector is (:1735)
// At most 2 * kf <= 32 (fact, side) entries per query: lane i of a query's half-wavefront holds entry i (fact i / 2,
// subject before object); the reference's dict is a pass of 32 shuffles (sum and count of the entries with the same
// vertex, in entry order = the order the reference adds them up), the stable selection another one (rank = entries
// of other phrases that are heavier, or equally heavy and earlier).  Round 2 ran one THREAD per query with
// dynamically indexed private arrays (scratch memory): 32 us at any batch size; this takes ~6.
#include "common.h"

namespace hrag {
namespace {

static_assert(kMaxSeeds == 32 && 2 * kMaxKeptFacts == kMaxSeeds, "one lane per (fact, side) entry");

__global__ __launch_bounds__(64) void build_seeds_kernel(const int32_t *__restrict__ kept_idx,
                                                         const float *__restrict__ kept_score,
                                                         const int32_t *__restrict__ kept_count, int32_t kf,
                                                         int32_t link_top_k, int32_t batch,
                                                         const int32_t *__restrict__ subj,
                                                         const int32_t *__restrict__ obj, int64_t n_facts,
                                                         const int32_t *__restrict__ num_chunks, int64_t num_vertices,
                                                         int32_t *__restrict__ seed_vtx, float *__restrict__ seed_w,
                                                         int32_t *__restrict__ seed_cnt, int32_t *__restrict__ flags) {
    const int lane = threadIdx.x & 63, half = lane >> 5, i = lane & 31, base = half * 32;
    const int q = blockIdx.x * 2 + half;
    const bool qv = q < batch;
    int cnt = qv ? kept_count[q] : 0;
    cnt = cnt < 0 ? 0 : (cnt > kf ? kf : cnt);
    const int r = i >> 1;                               // fact of this entry, in filter order
    const bool on = qv && r < cnt;
    const int32_t fidx = on ? kept_idx[q * kf + r] : -1;
    const float score = on ? kept_score[q * kf + r] : 0.f;
    int32_t v = -1;
    if (fidx >= 0 && (int64_t)fidx < n_facts) v = (i & 1) ? obj[fidx] : subj[fidx];
    int32_t nch = 0;
    if (v >= 0 && (int64_t)v < num_vertices) nch = num_chunks[v]; else v = -1;
    const float w = nch > 0 ? __fdiv_rn(score, (float)nch) : score;
    // the "dict": sum / count of the entries with my vertex, in entry order; `first` = its first entry
    double wsum = 0.0;
    int occ = 0, first = i;
    for (int j = 0; j < 32; ++j) {
        const int32_t vj = __shfl(v, base + j, 64);
        const float wj = __shfl(w, base + j, 64);
        if (v >= 0 && vj == v) {
            wsum += (double)wj;
            occ += 1;
            first = j < first ? j : first;
        }
    }
    const bool rep = v >= 0 && first == i;               // this lane speaks for its phrase
    const double mean = rep ? wsum / (double)occ : 0.0;
    // stable selection: heavier first, every NaN above every number, ties (NaN with NaN included) in first-occurrence
    // order -- a strict total order on the representatives, so the ranks are a permutation of [0, m)
    const bool nan_me = mean != mean;
    int rank = 0;
    for (int j = 0; j < 32; ++j) {
        const double mj = __shfl(mean, base + j, 64);
        const int rj = __shfl((int)rep, base + j, 64);
        const bool nan_j = mj != mj;
        const bool before = nan_j ? (!nan_me || j < i) : (!nan_me && (mj > mean || (mj == mean && j < i)));
        if (rj && j != i && before) rank += 1;
    }
    const unsigned long long reps = __builtin_amdgcn_ballot_w64(rep);
    const int m = __builtin_popcountll((reps >> base) & 0xffffffffull);
    const int keep = (link_top_k > 0 && link_top_k < m) ? link_top_k : m;
    const bool kept = rep && rank < keep;
    if (kept) {
        seed_vtx[q * kMaxSeeds + rank] = v;
        seed_w[q * kMaxSeeds + rank] = sanitise_reset((float)mean);
    }
    const unsigned long long zero_kept = __builtin_amdgcn_ballot_w64(kept && mean == 0.0);
    if (qv && i == 0) {
        int32_t flag = flags[q] & ~(1 | 4);
        if (cnt == 0) flag |= 1;                          // DPR fallback (HippoRAG.py:467-469)
        if ((zero_kept >> base) & 0xffffffffull) flag |= 4;
        seed_cnt[q] = keep;
        flags[q] = flag;
    }
}

// the fact bitset of a scoped phase A (launch_fact_mask): one thread per output word, i.e. per 32 facts, so the word is
// assembled in a register and stored once -- no atomics.  A fact's sources are few (usually one passage): the inner loop
// stops at the first allowed one
__global__ __launch_bounds__(256) void fact_mask_kernel(const uint32_t *__restrict__ doc, int64_t doc_ld_words,
                                                        int64_t doc_bit0, int64_t n_docs,
                                                        const int64_t *__restrict__ row_ptr,
                                                        const int32_t *__restrict__ pos, int64_t n_facts,
                                                        int64_t fact_words, uint32_t *__restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (w >= fact_words) return;
    const uint32_t *d = doc + (size_t)row * (size_t)doc_ld_words;
    const int64_t f0 = w * 32;
    const int nf = n_facts - f0 < 32 ? (int)(n_facts - f0) : 32;
    uint32_t bits = 0;
    for (int j = 0; j < nf; ++j) {
        const int64_t end = row_ptr[f0 + j + 1];
        for (int64_t e = row_ptr[f0 + j]; e < end; ++e) {
            const int64_t p = pos[e];
            if (p < 0 || p >= n_docs) continue;
            const int64_t b = doc_bit0 + p;
            if ((d[b >> 5] >> (b & 31)) & 1u) {
                bits |= 1u << j;
                break;
            }
        }
    }
    out[(size_t)row * (size_t)fact_words + w] = bits;
}

}  // namespace

hrag_status launch_fact_mask(const uint32_t *doc, int64_t doc_ld_words, int64_t doc_bit0, int64_t n_docs, int32_t rows,
                             const int64_t *row_ptr, const int32_t *pos, int64_t n_facts, uint32_t *out, hipStream_t s) {
    HRAG_REQUIRE(doc && row_ptr && out && rows >= 1 && n_facts >= 1 && n_docs >= 0 && doc_bit0 >= 0, "bad argument");
    HRAG_REQUIRE(doc_ld_words == 0 || doc_ld_words >= ceil_div(doc_bit0 + n_docs, 32),
                 "doc filter: %lld words per row < %lld (0: one row for every query)", (long long)doc_ld_words,
                 (long long)ceil_div(doc_bit0 + n_docs, 32));
    const int64_t fact_words = ceil_div(n_facts, 32);
    HRAG_REQUIRE(fact_words <= (int64_t)256 * 0x7fffffff && rows <= 65535, "fact mask of %lld x %lld words not supported",
                 (long long)rows, (long long)fact_words);
    hipLaunchKernelGGL(fact_mask_kernel, dim3((unsigned)ceil_div(fact_words, 256), (unsigned)rows), dim3(256), 0, s, doc,
                       doc_ld_words, doc_bit0, n_docs, row_ptr, pos, n_facts, fact_words, out);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

hrag_status launch_build_seeds(const int32_t *kept_idx, const float *kept_score,
                               const int32_t *kept_count, int32_t kf, int32_t link_top_k,
                               int32_t batch, const int32_t *subj, const int32_t *obj,
                               int64_t n_facts, const int32_t *num_chunks, int64_t num_vertices,
                               int32_t *seed_vtx, float *seed_w, int32_t *seed_cnt,
                               int32_t *flags, hipStream_t s) {
    HRAG_REQUIRE(kf >= 1 && kf <= kMaxKeptFacts, "kf=%d outside [1, %d]", kf, kMaxKeptFacts);
    if (batch == 0) return HRAG_OK;
    hipLaunchKernelGGL(build_seeds_kernel, dim3((unsigned)ceil_div(batch, 2)), dim3(64), 0, s,
                       kept_idx, kept_score, kept_count, kf, link_top_k, batch, subj, obj, n_facts,
                       num_chunks, num_vertices, seed_vtx, seed_w, seed_cnt, flags);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

}  // namespace hrag
