// Internal: one clause of the payload-filter encoding (include/hrag.h, payload filters) on the device -- its staged record,
// the staging of clause j from the caller's arrays and its evaluation at one passage.  Shared by payload_filter_kernel
// (payload.hip) and boost_rows_kernel (boost.hip): both evaluate a clause with this code and no other.
#pragma once

#include "engine_impl.h"

namespace hrag {
namespace {

enum : int32_t { kDead = -1 };      // staged kind of an ill-formed clause

struct PayClause {
    const int64_t *values;
    const uint32_t *present;
    int64_t lo, hi;
    int32_t kind, role, f64, set_beg, set_len, pad;
};

__device__ __forceinline__ double as_f64(int64_t v) { return __longlong_as_double(v); }

// x equals one of the ascending values set[0 .. len): binary search, equality in the column's type
template <bool F64>
__device__ __forceinline__ bool in_set(const int64_t *__restrict__ set, int32_t len, int64_t x) {
    int32_t lo = 0, hi = len;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const int64_t v = set[mid];
        const bool less = F64 ? as_f64(v) < as_f64(x) : v < x;
        if (less) lo = mid + 1; else hi = mid;
    }
    if (lo >= len) return false;
    return F64 ? as_f64(set[lo]) == as_f64(x) : set[lo] == x;
}

// clause j of the caller's arrays with its column resolved; an ill-formed one is staged as kDead (it hits nothing), one
// with an unknown role as a MUST
__device__ __forceinline__ PayClause stage_clause(const PayCol *__restrict__ cols, int32_t n_cols,
                                                  const int32_t *__restrict__ c_col, const int32_t *__restrict__ c_op,
                                                  const int64_t *__restrict__ c_lo, const int64_t *__restrict__ c_hi,
                                                  const int32_t *__restrict__ c_set_ptr, int64_t set_nnz, int64_t j) {
    const int32_t col = c_col[j], op = c_op[j];
    PayClause c;
    c.values = nullptr;
    c.present = nullptr;
    c.lo = c_lo[j];
    c.hi = c_hi[j];
    c.kind = (op >> 8) & 0xff;
    c.role = op & 0xff;
    c.f64 = 0;
    c.pad = 0;
    // the set slice: only set_vals [0, set_nnz) is read
    int64_t sb = c_set_ptr[j], se = c_set_ptr[j + 1];
    sb = sb < 0 ? 0 : sb > set_nnz ? set_nnz : sb;
    se = se < sb ? sb : se > set_nnz ? set_nnz : se;
    c.set_beg = (int32_t)sb;
    c.set_len = (int32_t)(se - sb);
    bool ok = (op >> 16) == 0 && col >= 0 && col < n_cols && c.kind <= HRAG_PAY_PRESENT && c.role <= HRAG_PAY_SHOULD;
    if (c.role > HRAG_PAY_SHOULD || (op >> 16) != 0) c.role = HRAG_PAY_MUST;     // an unknown role: a MUST that hits nothing
    if (ok) {
        const PayCol pc = cols[col];
        c.values = pc.values;
        c.present = pc.present;
        c.f64 = pc.type == HRAG_PAY_F64;
        if (c.kind == HRAG_PAY_RANGE) ok = c.f64 ? as_f64(c.lo) <= as_f64(c.hi) : c.lo <= c.hi;   // (false for a NaN bound)
    }
    if (!ok) c.kind = kDead;
    return c;
}

// hit(clause, p) of a live clause (kind != kDead) at the passage p < n_passages
__device__ __forceinline__ bool clause_hit(const PayClause &c, const int64_t *__restrict__ set_vals, int64_t p) {
    bool h = c.present ? ((c.present[p >> 5] >> (p & 31)) & 1u) != 0 : true;
    if (h && c.kind != HRAG_PAY_PRESENT) {
        const int64_t x = c.values[p];
        if (c.kind == HRAG_PAY_RANGE)
            h = c.f64 ? (as_f64(c.lo) <= as_f64(x) && as_f64(x) <= as_f64(c.hi)) : (c.lo <= x && x <= c.hi);
        else
            h = c.f64 ? in_set<true>(set_vals + c.set_beg, c.set_len, x)
                      : in_set<false>(set_vals + c.set_beg, c.set_len, x);
    }
    return h;
}

// the verdict of a clause list over the (up to) eight passages tile0 + 256 u + tid of a thread, bit u of a mask each:
// every MUST hits, no MUST_NOT hits, and some SHOULD hits when there is one.  inb: the passages below n_passages
__device__ __forceinline__ uint32_t clauses_pass(const PayClause *s_cl, int32_t nc, const int64_t *__restrict__ set_vals,
                                                 int64_t tile0, int tid, uint32_t inb) {
    uint32_t pass = inb, should = 0;
    bool has_should = false;
    for (int32_t j = 0; j < nc; ++j) {       // uniform over the workgroup: every value below comes from LDS
        const PayClause c = s_cl[j];
        uint32_t hit = 0;
        if (c.kind != kDead) {
#pragma unroll
            for (int u = 0; u < HRAG_PAY_TILE / 256; ++u) {
                if (!((inb >> u) & 1u)) continue;
                hit |= (uint32_t)clause_hit(c, set_vals, tile0 + 256 * u + tid) << u;
            }
        }
        if (c.role == HRAG_PAY_MUST) pass &= hit;
        else if (c.role == HRAG_PAY_MUST_NOT) pass &= ~hit;
        else { has_should = true; should |= hit; }
    }
    if (has_should) pass &= should;
    return pass;
}

}  // namespace
}  // namespace hrag
