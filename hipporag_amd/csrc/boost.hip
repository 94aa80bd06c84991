// Boosted retrieval (include/hrag.h, "boosted retrieval": hrag_boost_rows; hrag_last_boosted is engine.hip's): score rows
// [B][n_passages] rewritten in place as s * M + A, M and A the fp64 product and sum of a small per-query list of boost
// terms over the payload columns -- constants under a condition, column values, decay functions of a column.
//
// boost_rows_kernel: one 256-thread workgroup per (query, tile of HRAG_PAY_TILE consecutive passages), the launch shape of
// payload_filter_kernel.  A workgroup whose query has no terms returns at once: its row is not touched.  The query's terms
// (at most HRAG_BOOST_MAX_TERMS, their columns resolved) and the condition clauses of all of them (at most
// HRAG_PAY_MAX_CLAUSES, staged and evaluated by payload_clause.h -- the code of the payload filter) go to LDS once, 6.5 KB.
// The term loop is uniform over the workgroup; thread t owns the passages tile0 + 256 u + t, u = 0 .. 7, and keeps their M
// and A in registers: coalesced 8-byte column reads, a presence word shared by 32 lanes, one coalesced 4-byte read and write
// of the row entry.  No atomics; an element is read and written by one thread; the columns n .. ld are not touched.
//
// Every fp64 operation of the definition is rounded on its own: contraction is off for everything below the pragma -- which
// is why the arithmetic is written with plain operators: the __dmul_rn / __dadd_rn wrappers are defined in a header ABOVE
// the pragma, carry the default contraction and fuse with each other once inlined -- and exp_dec is the library's own
// exponential (a libm exp would differ from the numpy restatement in the last bit).
#include "payload_clause.h"

#pragma clang fp contract(off)

namespace hrag {
namespace {

constexpr int kBoostThreads = 256;
constexpr int kBoostPer = HRAG_PAY_TILE / kBoostThreads;       // passages per thread
static_assert(kBoostPer * kBoostThreads == HRAG_PAY_TILE && kBoostPer == 8, "clauses_pass keeps 8-bit masks");
static_assert(HRAG_BOOST_MAX_TERMS <= kBoostThreads && HRAG_PAY_MAX_CLAUSES <= kBoostThreads, "thread j stages term / clause j");

struct BoostTerm {
    const int64_t *values;
    const uint32_t *present;
    double w, p0, p1, p2, missing;
    int32_t kind, mode, sub, has_missing, f64, cl_beg, cl_n, pad;     // kind kDead: an ill-formed term, neutral
};

__device__ __forceinline__ double pos_part(double y) { return y > 0.0 ? y : 0.0; }      // fmax(0, y); +0 for NaN and -0

// exp(x) for x <= 0 by the scheme of include/hrag.h: every product and sum rounded once, no fma
__device__ __forceinline__ double exp_dec(double x) {
    if (x != x) return x;
    if (x > 0.0) x = 0.0;
    if (x < -708.0) return 0.0;
    const double k = rint(x * 0x1.71547652b82fep+0);
    const double r = (x - k * 0x1.62e42fee00000p-1) - k * 0x1.a39ef35793c76p-33;
    // c_i = fp64(1 / i!), i = 13 .. 0
    constexpr double c[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0,
                              1.0 / 362880.0, 1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
    double p = c[13];
#pragma unroll
    for (int i = 12; i >= 0; --i) p = p * r + c[i];
    return ldexp(p, (int)k);
}

__global__ __launch_bounds__(kBoostThreads) void boost_rows_kernel(
    const PayCol *__restrict__ cols, int32_t n_cols, int64_t n, float *rows, int64_t ld, const float *__restrict__ mn,
    const float *__restrict__ mx, const int32_t *__restrict__ t_ptr, const int32_t *__restrict__ t_op,
    const int32_t *__restrict__ t_col, const double *__restrict__ t_num, const int32_t *__restrict__ t_cl_ptr,
    const int32_t *__restrict__ c_col, const int32_t *__restrict__ c_op, const int64_t *__restrict__ c_lo,
    const int64_t *__restrict__ c_hi, const int32_t *__restrict__ c_set_ptr, const int64_t *__restrict__ set_vals,
    int64_t n_terms, int64_t n_clauses, int64_t set_nnz, int32_t broadcast, int32_t n_tiles) {
    __shared__ BoostTerm s_t[HRAG_BOOST_MAX_TERMS];
    __shared__ PayClause s_cl[HRAG_PAY_MAX_CLAUSES];
    __shared__ int32_t s_cbeg[HRAG_BOOST_MAX_TERMS], s_clen[HRAG_BOOST_MAX_TERMS];

    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x / n_tiles;
    const int64_t tile0 = ((int64_t)blockIdx.x % n_tiles) * HRAG_PAY_TILE;

    // the term list: whatever t_ptr holds, only terms [0, n_terms) are read, and at most the cap
    int64_t beg = t_ptr[broadcast ? 0 : b], end = t_ptr[broadcast ? 1 : b + 1];
    beg = beg < 0 ? 0 : beg > n_terms ? n_terms : beg;
    end = end < beg ? beg : end > n_terms ? n_terms : end;
    const int32_t nt = (int32_t)(end - beg < HRAG_BOOST_MAX_TERMS ? end - beg : HRAG_BOOST_MAX_TERMS);
    if (nt == 0) return;        // (uniform: before any barrier) the row stays bit for bit

    // the clause slice of term tid, clamped to the clauses there are
    if (tid < nt) {
        int64_t cb = t_cl_ptr[beg + tid], ce = t_cl_ptr[beg + tid + 1];
        cb = cb < 0 ? 0 : cb > n_clauses ? n_clauses : cb;
        ce = ce < cb ? cb : ce > n_clauses ? n_clauses : ce;
        s_cbeg[tid] = (int32_t)cb;
        s_clen[tid] = (int32_t)(ce - cb < HRAG_PAY_MAX_CLAUSES ? ce - cb : HRAG_PAY_MAX_CLAUSES);
    }
    __syncthreads();
    if (tid < nt) {
        // the clauses of a query fill the cap in term order: a term keeps the first ones of its slice that still fit
        int32_t used = 0;
        for (int i = 0; i < tid; ++i) used += s_clen[i];
        used = used < HRAG_PAY_MAX_CLAUSES ? used : HRAG_PAY_MAX_CLAUSES;
        const int32_t len = s_clen[tid], room = HRAG_PAY_MAX_CLAUSES - used;
        const int64_t j = beg + tid;
        const int32_t op = t_op[j], col = t_col[j];
        BoostTerm t;
        t.values = nullptr;
        t.present = nullptr;
        t.w = t_num[5 * j];
        t.p0 = t_num[5 * j + 1];
        t.p1 = t_num[5 * j + 2];
        t.p2 = t_num[5 * j + 3];
        t.missing = t_num[5 * j + 4];
        t.kind = op & 0xff;
        t.mode = (op >> 8) & 0xff;
        t.sub = (op >> 16) & 0xff;
        t.has_missing = (op >> 24) & 1;
        t.f64 = 0;
        t.cl_beg = used;
        t.cl_n = len < room ? len : room;
        t.pad = 0;
        bool ok = (op >> 25) == 0 && t.kind <= HRAG_BOOST_DECAY && t.mode <= HRAG_BOOST_ADD &&
                  t.sub <= (t.kind == HRAG_BOOST_DECAY ? HRAG_BOOST_GAUSS : t.kind == HRAG_BOOST_FIELD ? HRAG_BOOST_SQRT : 0);
        if (ok && t.kind != HRAG_BOOST_CONST) {
            ok = col >= 0 && col < n_cols;
            if (ok) {
                const PayCol pc = cols[col];
                t.values = pc.values;
                t.present = pc.present;
                t.f64 = pc.type == HRAG_PAY_F64;
            }
        }
        if (!ok) t.kind = kDead;
        s_t[tid] = t;
    }
    __syncthreads();
    if (tid < HRAG_PAY_MAX_CLAUSES) {
        for (int i = 0; i < nt; ++i) {
            const int32_t at = tid - s_t[i].cl_beg;
            if (at >= 0 && at < s_t[i].cl_n) {
                s_cl[tid] = stage_clause(cols, n_cols, c_col, c_op, c_lo, c_hi, c_set_ptr, set_nnz, (int64_t)s_cbeg[i] + at);
                break;
            }
        }
    }
    __syncthreads();

    // bit u of a mask: the passage tile0 + 256 u + tid
    uint32_t inb = 0;
#pragma unroll
    for (int u = 0; u < kBoostPer; ++u) inb |= (uint32_t)(tile0 + kBoostThreads * u + tid < n) << u;

    double M[kBoostPer], A[kBoostPer];
#pragma unroll
    for (int u = 0; u < kBoostPer; ++u) { M[u] = 1.0; A[u] = 0.0; }

    for (int32_t i = 0; i < nt; ++i) {       // uniform over the workgroup: every value below comes from LDS
        const BoostTerm t = s_t[i];
        if (t.kind == kDead) continue;
        const uint32_t hit = clauses_pass(s_cl + t.cl_beg, t.cl_n, set_vals, tile0, tid, inb);     // (a subset of inb)
#pragma unroll
        for (int u = 0; u < kBoostPer; ++u) {
            if (!((hit >> u) & 1u)) continue;
            double v = 1.0;
            if (t.kind != HRAG_BOOST_CONST) {
                const int64_t p = tile0 + kBoostThreads * u + tid;
                bool have = t.present ? ((t.present[p >> 5] >> (p & 31)) & 1u) != 0 : true;
                double x = 0.0;
                if (have) {
                    const int64_t raw = t.values[p];
                    x = t.f64 ? as_f64(raw) : (double)raw;      // (int64 -> double rounds to nearest even)
                    have = x == x;                              // a NaN value is missing
                }
                if (!have) {
                    if (!t.has_missing) continue;
                    v = t.missing;
                } else if (t.kind == HRAG_BOOST_FIELD) {
                    v = t.sub == HRAG_BOOST_SQRT ? __dsqrt_rn(x) : x;
                } else {
                    const double d = pos_part(fabs(x - t.p0) - t.p1);
                    if (t.sub == HRAG_BOOST_LINEAR) v = pos_part((t.p2 - d) / t.p2);
                    else v = exp_dec(t.p2 * (t.sub == HRAG_BOOST_EXP ? d : d * d));
                }
            }
            const double tv = t.w * v;
            if (t.mode == HRAG_BOOST_MUL) M[u] = M[u] * tv;
            else A[u] = A[u] + tv;
        }
    }

    float lo = 0.f, range = 0.f;
    if (mn) { lo = mn[b]; range = mx[b] - lo; }
    float *row = rows + (size_t)b * ld + tile0;
#pragma unroll
    for (int u = 0; u < kBoostPer; ++u) {
        if (!((inb >> u) & 1u)) continue;
        float s = row[kBoostThreads * u + tid];
        if (mn) s = range == 0.f ? 1.f : __fdiv_rn(s - lo, range);      // the library's min-max: a zero range gives 1
        const float f = (float)((double)s * M[u] + A[u]);
        row[kBoostThreads * u + tid] = f != f ? __uint_as_float(0x7fc00000u) : f;
    }
}

}  // namespace

hrag_status launch_boost_rows(const hrag_payload *pay, float *rows, int64_t ld, int32_t batch, const float *mn,
                              const float *mx, const hrag_boost_program *g, int32_t broadcast, hipStream_t s) {
    HRAG_REQUIRE(pay != nullptr, "the payload index is NULL");
    HRAG_REQUIRE(rows != nullptr, "the score rows are NULL");
    HRAG_REQUIRE(g != nullptr, "the boost program is NULL");
    HRAG_REQUIRE(batch >= 1 && batch <= 65535, "batch=%d outside [1, 65535]", batch);
    HRAG_REQUIRE(ld >= pay->n_passages, "ld=%lld below n_passages=%lld", (long long)ld, (long long)pay->n_passages);
    HRAG_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 3) == 0, "the score rows must be 4-byte aligned");
    HRAG_REQUIRE((mn == nullptr) == (mx == nullptr), "mn and mx: both or neither");
    HRAG_REQUIRE(g->n_terms >= 0 && g->n_terms < ((int64_t)1 << 31), "n_terms=%lld outside [0, 2^31)", (long long)g->n_terms);
    HRAG_REQUIRE(g->n_clauses >= 0 && g->n_clauses < ((int64_t)1 << 31), "n_clauses=%lld outside [0, 2^31)",
                 (long long)g->n_clauses);
    HRAG_REQUIRE(g->set_nnz >= 0 && g->set_nnz < ((int64_t)1 << 31), "set_nnz=%lld outside [0, 2^31)", (long long)g->set_nnz);
    HRAG_REQUIRE(g->n_terms == 0 || (g->t_ptr && g->t_op && g->t_col && g->t_num && g->t_cl_ptr),
                 "a term array is NULL with n_terms=%lld", (long long)g->n_terms);
    HRAG_REQUIRE(g->n_clauses == 0 || (g->c_col && g->c_op && g->c_lo && g->c_hi && g->c_set_ptr),
                 "a clause array is NULL with n_clauses=%lld", (long long)g->n_clauses);
    HRAG_REQUIRE(g->set_nnz == 0 || g->set_vals, "set_vals is NULL with set_nnz=%lld", (long long)g->set_nnz);
    if (g->n_terms == 0) return HRAG_OK;        // no query has a term: no row is touched
    const int64_t n_tiles = ceil_div(pay->n_passages, HRAG_PAY_TILE);
    const int64_t grid = (int64_t)batch * n_tiles;
    HRAG_REQUIRE(grid < ((int64_t)1 << 31), "batch=%d x %lld tiles exceeds one launch", batch, (long long)n_tiles);
    hipLaunchKernelGGL(boost_rows_kernel, dim3((unsigned)grid), dim3(kBoostThreads), 0, s, pay->d_cols, pay->n_cols,
                       pay->n_passages, rows, ld, mn, mx, g->t_ptr, g->t_op, g->t_col, g->t_num, g->t_cl_ptr, g->c_col, g->c_op,
                       g->c_lo, g->c_hi, g->c_set_ptr, g->set_vals, g->n_terms, g->n_clauses, g->set_nnz, broadcast ? 1 : 0,
                       (int32_t)n_tiles);
    HRAG_LAUNCH_CHECK();
    return HRAG_OK;
}

}  // namespace hrag

using namespace hrag;

// ---- exports (include/hrag.h, boosted retrieval)
hrag_status hrag_boost_rows(const hrag_payload *pay, float *rows_dev, int64_t ld, int32_t batch, const float *mn_dev,
                            const float *mx_dev, const hrag_boost_program *program, int32_t broadcast, hrag_stream stream) {
    return launch_boost_rows(pay, rows_dev, ld, batch, mn_dev, mx_dev, program, broadcast, (hipStream_t)stream);
}
