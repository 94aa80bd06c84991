// Internal: the bin function of facets (include/hrag.h, facets) on the device -- the staged record of a facet spec, its
// staging from the handle's column table and the bin of one passage, presence test included.  Shared by facet_count_kernel
// and facet_ids_kernel (facet.hip): both map a passage to its bin with this code and no other.  tests/facet_helpers.py
// states the same function in numpy.
#pragma once

#include "payload_clause.h"

namespace hrag {
namespace {

constexpr int kFacetLdsEdges = 1024;       // EDGES with at most this many bounds: searched in LDS (8 KB), else in global memory

struct FacetRec {
    const int64_t *values;
    const uint32_t *present;
    const int64_t *edges;       // EDGES: m ascending bounds, 8-byte words of the column's type
    int64_t lo;                 // CODES: the value of bin 0
    int32_t kind, f64, n_bins, m;
};

// the workgroup's copy of a short edge list (the caller puts a barrier behind it)
__device__ __forceinline__ void stage_edges(int64_t *s_edges, const FacetRec &r, int tid, int threads) {
    if (r.kind == HRAG_FACET_EDGES && r.m <= kFacetLdsEdges)
        for (int i = tid; i < r.m; i += threads) s_edges[i] = r.edges[i];
}

// the number of the ascending e[0 .. m) that are <= x, comparisons in the column's type (-0.0 == 0.0): 0 <= result <= m
// whatever e holds
__device__ __forceinline__ int32_t edges_below(const int64_t *e, int32_t m, bool f64, int64_t x) {
    int32_t lo = 0, hi = m;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const int64_t v = e[mid];
        const bool le = f64 ? as_f64(v) <= as_f64(x) : v <= x;
        if (le) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the spec with its column resolved; the host has checked the column id, the kind and n_bins (n_bins == m + 1 for EDGES)
__device__ __forceinline__ FacetRec stage_facet(const PayCol *__restrict__ cols, int32_t col, int32_t kind, int64_t lo,
                                                const int64_t *__restrict__ edges, int32_t m, int32_t n_bins) {
    const PayCol pc = cols[col];
    FacetRec r;
    r.values = pc.values;
    r.present = pc.present;
    r.edges = edges;
    r.lo = lo;
    r.kind = kind;
    r.f64 = pc.type == HRAG_PAY_F64;
    r.n_bins = n_bins;
    r.m = m;
    return r;
}

// the bin of the passage p < n_passages: [0, n_bins) a bin, n_bins "other" (a value that maps to no bin), n_bins + 1
// "missing" (no value).  Whatever the edges hold, the result is in [0, n_bins + 2): the search keeps 0 <= bin <= m.
// s_edges: stage_edges' copy (read when m <= kFacetLdsEdges)
__device__ __forceinline__ int32_t facet_bin(const FacetRec &r, const int64_t *s_edges, int64_t p) {
    if (r.present && !((r.present[p >> 5] >> (p & 31)) & 1u)) return r.n_bins + 1;
    const int64_t x = r.values[p];
    if (r.kind == HRAG_FACET_CODES) {
        // both conditions: x = INT64_MIN with lo = INT64_MAX wraps to 1
        const uint64_t d = (uint64_t)x - (uint64_t)r.lo;
        return (x >= r.lo && d < (uint64_t)r.n_bins) ? (int32_t)d : r.n_bins;
    }
    if (r.f64 && as_f64(x) != as_f64(x)) return r.n_bins;       // a NaN value is in no bucket
    return r.m <= kFacetLdsEdges ? edges_below(s_edges, r.m, r.f64, x) : edges_below(r.edges, r.m, r.f64, x);
}

}  // namespace
}  // namespace hrag
