/*
 * hrag.h -- C ABI of libhrag.so, the MI355X (gfx950) retrieval hot path of HippoRAG.
 *
 * The reference (OSU-NLP-Group/HippoRAG) has no FFI for this path: the seam is a
 * set of Python methods on class HippoRAG (src/hipporag/HippoRAG.py).  Each entry
 * point below names the reference method(s) it replaces; INTEGRATION.md shows
 * the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain C types only: pointers + sizes; no torch / C++ types cross the ABI;
 *   - every function returns an hrag_status (0 = OK); hrag_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - pointers named *_dev are DEVICE pointers on the engine's device; pointers
 *     in the *_desc structs used by hrag_engine_create may be host OR device
 *     (copied with hipMemcpyDefault; the caller may free them right after);
 *   - every compute entry point takes the HIP stream to enqueue on (pass
 *     torch.cuda.current_stream().cuda_stream) and returns after enqueueing: no
 *     device synchronisation, no allocation in the call path (graph-capture safe);
 *   - ONE call in flight per engine HANDLE: the workspace (scores, PPR state, seeds) belongs to the handle.  Calls on one
 *     stream queue up as usual; a call on ANOTHER stream is ordered behind the previous call ON THE DEVICE (the
 *     library makes the new stream wait for the event that ends the previous call: no host synchronisation, no
 *     error -- a multi-stream pipeline just serialises on this engine's workspace); a call from a second THREAD
 *     while one is still inside the library is REJECTED with HRAG_EBUSY (never a silent race).  Real concurrency =
 *     one WORKSPACE per stream / thread: hrag_workspace_create gives a second handle on the same index (nothing of
 *     the index is copied) whose calls run concurrently with this one's -- SURVEY.md 8(b).  Replays of a captured HIP
 *     graph bypass the library and are NOT ordered against direct calls on other streams: keep them on one stream;
 *   - bf16 = the upper 16 bits of an IEEE-754 binary32, passed as uint16_t (fp16 engines:
 *     IEEE binary16 bit patterns in the same uint16_t slots);
 *   - all index outputs are int32, all score outputs fp32;
 *   - ranking rule everywhere: score descending, ties -> larger index first
 *     (== numpy.argsort(x, kind="stable")[::-1]; the reference's np.argsort default
 *     leaves ties undefined, HippoRAG.py:1500,1688,1746).  NaN: every NaN, whatever its
 *     sign or payload, ranks above +inf, NaNs tie by index (numpy sorts NaN last); the
 *     score returned for it is the canonical quiet NaN (0x7fc00000);
 *   - row min / max (the min-max normalisation, the mn / mx outputs) are fminf / fmaxf:
 *     NaN is skipped; a row with no number (empty, or NaN only) gives +inf / -inf.
 */
#ifndef HRAG_H_
#define HRAG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version history of the ABI (hrag_version() = major * 1000 + minor):
 *   0.6  error-bound constants, HRAG_PPR_TOL_MIN; stage plan 1+2+3+4+4+4+2 for a FIXED sweep count.  Note for callers
 *        that read residual_out of a fixed-count call (ppr_tol = 0): that plan REPORTS about 2.2x the residual of the
 *        0.5 plan at the same true error (the last right-hand side is quantised later) -- a host-side threshold on it
 *        must be re-derived; a call with ppr_tol > 0 takes the plan ending on 2 + 1, so a fixed-count call and a
 *        tolerance call at the same 20 sweeps are no longer bit-identical;
 *   0.7  hrag_workspace_create, hrag_engine_stats (hrag_stats), hrag_ppr_sweeps flag 256 (gather replay); hrag_comm +
 *        hrag_shard_score_facts_all / hrag_shard_retrieve / hrag_shard_workspace_bytes (one call per phase on a row shard);
 *        hrag_shard_ppr_sweep enforces the ascending (step, group) order of a session with measured stage scales;
 *        later in 0.7 (no signature change): the accelerated two-stage fp16 plan (HRAG_OPT_ACCEL, batch <= 64, ppr_tol = 0)
 *        carries a margin of 16 instead of 4: 16 sweeps stand for 20 at damping 0.5 (14 before);
 *   0.8  hrag_sim_topk_min_score (the thresholded fused top-k of the index-time KNN: prefix first pass + cut);
 *        later in 0.8 (no struct layout changes; detect by the symbol): hrag_topk_rows_ws +
 *        hrag_topk_rows_workspace_bytes (any k), hrag_opts.max_topk above 2048;
 *        later in 0.8 (detect by the symbol): the doc filter -- hrag_topk_rows_masked, hrag_retrieve_filtered,
 *        hrag_retrieve_scored_filtered, hrag_dense_retrieve_filtered, hrag_shard_finish_filtered,
 *        hrag_shard_retrieve_filtered;
 *        later in 0.8 (detect by the symbol): the scoped doc filter -- hrag_engine_set_fact_sources,
 *        hrag_fact_mask_from_docs, hrag_score_facts_scoped, hrag_retrieve_scoped, hrag_retrieve_scored_scoped,
 *        hrag_dense_retrieve_scoped;
 *        later in 0.8 (detect by the symbol): the scoped doc filter on row shards -- hrag_shard_score_facts_scoped,
 *        hrag_shard_passage_scores_scoped, hrag_shard_mask_prior, hrag_shard_score_facts_all_scoped,
 *        hrag_shard_retrieve_scoped (hrag_engine_set_fact_sources then accepts a row-shard engine);
 *        later in 0.8 (detect by the symbol): fused retrieval -- hrag_fuse_rows, hrag_rrf_rows,
 *        hrag_fuse_workspace_bytes, hrag_last_fused;
 *        later in 0.8 (detect by the symbol): diversified retrieval -- hrag_gram_rows, hrag_mmr_rows,
 *        hrag_mmr_workspace_bytes, hrag_mmr, hrag_mmr_sel;
 *        later in 0.8 (detect by the symbol): lexical retrieval -- hrag_lex_create, hrag_lex_destroy, hrag_lex_scores,
 *        hrag_lex_blend_rows;
 *        later in 0.8 (detect by the symbol): payload filters -- hrag_payload_create, hrag_payload_destroy,
 *        hrag_payload_filter, hrag_bitset_count_rows;
 *        later in 0.8 (detect by the symbol): boosted retrieval -- hrag_boost_rows, hrag_last_boosted;
 *        later in 0.8 (detect by the symbol): facets -- hrag_payload_facet, hrag_payload_facet_ids,
 *        hrag_payload_facet_ws_bytes;
 *        later in 0.8 (detect by the symbol): late-interaction reranking -- hrag_late_create, hrag_late_destroy,
 *        hrag_late_scores, hrag_late_rank_rows, hrag_late_workspace_bytes, hrag_late_rerank;
 *        later in 0.8 (detect by the symbol): recommend by example -- hrag_reco_rows, hrag_reco_workspace_bytes,
 *        hrag_reco_scores_rows, hrag_reco_scores, hrag_reco_query, hrag_reco_exclude. */
#define HRAG_VERSION_MAJOR 0
#define HRAG_VERSION_MINOR 8

typedef enum hrag_status {
    HRAG_OK = 0,
    HRAG_EINVAL = 1,      /* bad shape / null pointer / unsupported option                    */
    HRAG_ENOMEM = 2,      /* hipMalloc failed                                                  */
    HRAG_EHIP = 3,        /* a HIP runtime call failed; text in hrag_last_error()              */
    HRAG_EBUSY = 4,       /* another THREAD is inside a call on this HANDLE (its workspace is in use; a second handle  */
                          /* from hrag_workspace_create runs concurrently; calls on other streams queue on the device) */
    HRAG_ECAPACITY = 5    /* batch / k larger than the engine was created for                  */
} hrag_status;

typedef struct hrag_engine hrag_engine; /* opaque */
typedef void *hrag_stream;              /* hipStream_t */

/* Knowledge graph as the PPR consumes it (replaces the igraph object handed to
 * graph.personalized_pagerank at HippoRAG.py:1736-1743).
 * CSR over OUTPUT vertices: row i lists the in-neighbours j of i with
 *   val = A[i][j] / sum_i A[i][j]           (column-stochastic, already normalised)
 * where A is the symmetric weighted adjacency in which parallel igraph edges are
 * summed (HippoRAG.py:1189-1223, :906-910).  hipporag_amd.graph.build_csr builds it.
 * Row sharding (multi-GPU): the engine owns rows [row_offset, row_offset + n_rows)
 * of a graph with num_vertices columns; single GPU: row_offset = 0, n_rows = V. */
typedef struct hrag_graph_desc {
    int64_t num_vertices;          /* V: columns of P == length of the PPR vector            */
    int64_t row_offset;            /* first global row owned by this engine                  */
    int64_t n_rows;                /* rows owned                                             */
    int64_t nnz;                   /* entries in the owned rows                              */
    const int32_t *row_ptr;        /* [n_rows + 1], row_ptr[0] == 0                          */
    const int32_t *col_idx;        /* [nnz] global column (source vertex) ids                */
    const float *val;              /* [nnz]                                                  */
    int64_t n_passages;            /* Np (global number of passages)                         */
    const int32_t *passage_vertex; /* [Np] vertex id of passage p (passage_node_idxs, :1333) */
    const double *col_sum;         /* [V] optional (may be NULL): sum_i A[i][j], the weighted degree   */
                                   /* each column was normalised with (0 for a vertex without edges). */
                                   /* Enables the fp8-state PPR for batches > 64 (csrc/ppr8.hip), which */
                                   /* iterates in the degree-scaled variable x / col_sum.             */
} hrag_graph_desc;

typedef enum hrag_dtype {
    HRAG_BF16 = 0,
    HRAG_FP16 = 1,     /* IEEE binary16 = BASELINE configs[4] */
    HRAG_F32_SPLIT = 2,/* fp32 in, fp32-faithful scores: what the reference computes (np.dot of fp32 matrices,           */
                       /* HippoRAG.py:1342-1345,1459,1496; embedding_store.py:216-221).  `data` is fp32 [rows, dim]; the  */
                       /* engine stores every vector as hi + lo (two fp16: 22 significant bits) in the layout            */
                       /* [hi | lo | hi] and a query as [qhi | qhi | qlo], so that one fp16 MFMA dot product of          */
                       /* 3 * dim elements IS hi.qhi + lo.qhi + hi.qlo -- through every kernel unchanged, at 3x the      */
                       /* embedding stream.  Every q_*_dev pointer of such an engine is fp32 [B, dim].                    */
                       /* Accuracy against the exact product of the fp32 vectors (tests/helpers.py split_score_bound):    */
                       /*   layout: sum_i e(x_i)|q_i| + |x_i|e(q_i) + e(x_i)e(q_i) + l(x_i)l(q_i), e(v) = max(2^-22 |v|,  */
                       /*     2^-25) bounds |v - hi - lo|, l(v) = 2^-11 |v| + 2^-25 bounds |lo| (the dropped lo.qlo);    */
                       /*     the 2^-25 is ABSOLUTE: lo is an fp16 subnormal below |v| = 2^-3, hi below 2^-14.  So the    */
                       /*     layout costs ~3 * 2^-22 |x||q| only while |x||q| dominates 2^-25 (|x|_1 + |q|_1): unit     */
                       /*     vectors (what embedding models return) keep it, vectors of norm 1e-3 at dim 4096 lose it   */
                       /*     (~2e-5 |x||q| RMS: scale such inputs to unit length first);                                */
                       /*   accumulation: fp32, one rounding per 32-element MFMA step: gamma_n sum|products| with        */
                       /*     n = 3 * dim / 32 + 5 in the worst case (4.6e-5 at dim 4096); rounding to nearest makes it   */
                       /*     a random walk in practice: ~2^-24 sqrt(2 * 3 * dim / 32) |score| over the last two thirds. */
                       /*   Precondition: every |component| < 65504 (fp16 overflow: an infinite half, NaN scores).       */
                       /* Ranking with bf16-rounded embeddings instead flips near-tied facts / passages                   */
                       /* (tests/test_ref_golden.py counts them on the reference-run fixture ref_synth_f32.npz)             */
    HRAG_F32_SPLIT_ROWS = 3 /* the same engine from rows that are ALREADY in the split layout: `data` is fp16             */
                       /* [rows, 3 * dim] as hrag_split_f32 / hrag_engine_gather_embeddings produce it (`dim` stays the  */
                       /* logical dimension): the index-update path, where the held rows never leave the device          */
} hrag_dtype;

/* Row-major, L2-normalised embedding matrix (self.fact_embeddings /
 * self.passage_embeddings, HippoRAG.py:1343-1345), rounded to bf16 or fp16, or fp32 (HRAG_F32_SPLIT); facts and
 * passages use the same dtype; every q_*_dev query pointer then carries that dtype too (declared uint16_t for the
 * 16-bit types; fp32 [B, dim] behind the same pointer on an HRAG_F32_SPLIT engine).
 * Row sharding: this engine holds rows [row_offset, row_offset + rows). */
typedef struct hrag_embed_desc {
    int64_t rows;
    int64_t row_offset;
    int32_t dim; /* D, multiple of 8 */
    hrag_dtype dtype;
    const void *data;
} hrag_embed_desc;

/* What graph_search_with_fact_entities needs to turn kept facts into seeds
 * (HippoRAG.py:1583-1606): the vertex of each fact's subject / object phrase
 * (-1 when md5("entity-"+phrase) is not a graph node) and, per vertex, the number
 * of chunks the entity occurs in (len(ent_node_to_chunk_ids[key]); 0 = do not divide). */
typedef struct hrag_fact_desc {
    int64_t n_facts;            /* global F                                       */
    const int32_t *subj_vertex; /* [F]                                            */
    const int32_t *obj_vertex;  /* [F]                                            */
    const int32_t *num_chunks;  /* [V]                                            */
} hrag_fact_desc;

#define HRAG_OPT_NATURAL_ROW_ORDER 1 /* keep CSR row order instead of degree-descending          */
#define HRAG_OPT_NT_CSR 2            /* fp32-state kernel: non-temporal loads for the col_idx / val stream */
#define HRAG_OPT_NT_STORE 4          /* fp32-state kernel: non-temporal stores for the new PPR state       */
#define HRAG_OPT_F32_STATE 8         /* plain CSR + fp32 slab state only: none of the staged fp8 state  */
                                     /* (batch > 64), the two-stage fp16 state (batch > 8, ppr_iters    */
                                     /* >= 11) and the small-batch kernels (batch <= 8); same 1e-5 bar  */
#define HRAG_OPT_TEMPORAL16 16       /* fp16-state kernels: plain instead of non-temporal (col, val)   */
                                     /* loads and state stores (non-temporal is 3 % faster at cfg 3)   */

#define HRAG_OPT_NO_FP8 32           /* never take the fp8-state PPR (batch > 64, 16 <= ppr_iters <= 30,                 */
                                     /* damping^ppr_iters <= 2^-20, col_sum given); the fp16 / fp32 state serves instead */

#define HRAG_OPT_ROWS_BY_MINCOL 64    /* experiment: SELL-8 rows of equal length ordered by smallest column id  */
#define HRAG_OPT_ROWS_BFS 128         /* experiment: ... by breadth-first rank (no L2 gain on  */
                                      /* the benchmark graph; kept for graphs with community structure)           */

#define HRAG_OPT_SLABS_PER_WG_1 256   /* fp8 sweep: one slab per workgroup (4 chunks) instead of the wavefronts of a   */
                                      /* workgroup sharing a chunk's (col, val) stream across 2 / 4 slabs             */

/* 512: was HRAG_OPT_FP8_MARGIN (two extra sweeps on the fp8 state); superseded by the convergence contract of   */
/* hrag_retrieve (ppr_tol / ppr_max_iters), which adds sweeps only where the measured residual asks for them    */

#define HRAG_OPT_NO_F16 1024          /* never take the fp16-state PPR either (two-stage fp16 state of batches 9..64 and of  */
                                      /* batches <= 8): the fp32 state serves.  Its values carry a relative precision of     */
                                      /* 2^-24 whatever their size, which passage scores many orders of magnitude below the */
                                      /* largest one need (a query on a slowly mixing graph that is being repeated for      */
                                      /* HRAG_FLAG_NOT_CONVERGED); runtime-switchable like HRAG_OPT_NO_FP8                    */

#define HRAG_OPT_XCD_BLOCKED 2048     /* fp8 sweep: every XCD walks a CONTIGUOUS eighth of the row order (instead of every    */
                                      /* eighth chunk group): with hrag_opts.sell_sigma on a graph with locality the rows     */
                                      /* that share in-neighbours then meet in ONE L2                                          */

#define HRAG_OPT_ACCEL 4096           /* sweep-count acceleration of the fp8-state PPR on an UNDIRECTED graph (HippoRAG's:    */
                                      /* is_directed_graph = False, config_utils.py:176): the stages run three Chebyshev      */
                                      /* steps on the real spectrum [-damping, damping] of the sweep operator instead of      */
                                      /* three Richardson sweeps (csrc/shard.hip ppr8_plan_accel).  `ppr_iters` then names an */
                                      /* ACCURACY -- the truncation error of that many plain sweeps -- and fewer sweeps run   */
                                      /* (damping 0.5, ppr_iters 20: 16; with ppr_tol > 0: 17 -- 1, 2 plain, Chebyshev stages,  */
                                      /* 2 plain at the end, so that the convergence measure reads a plain sweep's update as   */
                                      /* it does without the flag; iters_out reports them).                                   */
                                      /* The reference's PRPACK solve is tolerance-driven (HippoRAG.py:1736-1743): any sweep  */
                                      /* count that meets the tolerance is the same answer.  Guarantees: the e4m3 scale of    */
                                      /* every stage is MEASURED on the device -- each boundary reports the batch's max |R|,  */
                                      /* ppr8_next_scale_kernel maps (that maximum) x (max-norm contraction of the next       */
                                      /* stage, 7 / T_3(1 / damping)) x (growth of the iterate) to half the e4m3 range: a     */
                                      /* rigorous bound re-anchored at every stage, not a static chain.  Failure mode: a      */
                                      /* value outside the range sets HRAG_FLAG_FP8_SATURATED for its query -- clear the      */
                                      /* flag and repeat on the plain plan (the Python wrapper does), then HRAG_OPT_NO_FP8;   */
                                      /* every boundary forms the TRUE residual, so refinement stays exact                    */
                                      /* and the extension stages of the contract (plain) apply unchanged.  With ppr_tol = 0  */
                                      /* the accuracy is that of ppr_iters plain sweeps on well-mixing graphs (cfg 3: 4.4e-7  */
                                      /* against 5.5e-7) and up to 3x their truncation error on small hub-heavy ones: use the */
                                      /* contract where a bound is needed.  Off by default: ppr_iters is then the literal     */
                                      /* sweep count (BASELINE.json's 20).  Runtime-switchable.  The two-stage fp16 states    */
                                      /* (batch <= 64) accelerate too (16 sweeps for 20; 14 up to the first 0.7 builds), ppr_tol = 0 and damping <= 0.62 only.  The library */
                                      /* cannot see whether the CSR it was given came from a symmetric adjacency: setting the */
                                      /* flag on a DIRECTED graph is a caller error (complex spectrum: the steps may converge */
                                      /* more slowly than the plan assumes; the contract would flag it, ppr_tol = 0 would     */
                                      /* not) -- the Python wrapper checks row sums == column sums of A in chunks AND that    */
                                      /* 4096 sampled entries have a mirror entry of the same weight                          */
                                      /* (hipporag_amd.graph.looks_undirected, evaluated when the flag is first asked for),   */
                                      /* and refuses otherwise                                                                 */

#define HRAG_OPT_STORE_R1 8192        /* fp8-state PPR: keep the stored fp32 residual R_1 between the first sweep and the     */
                                      /* boundary that closes stage 2 instead of forming it again in registers from c_0 at    */
                                      /* that boundary (csrc/ppr8.hip modes B0N / B1, the default: 2 GB less traffic per      */
                                      /* retrieve at BASELINE configs[2]).  Results are bit-identical either way: the flag is */
                                      /* the A/B lever for the R_1 round trip and the reference of                            */
                                      /* tests/test_gpu_first_residual.py.  It is NOT the path of the builds before the       */
                                      /* recompute: their first sweep also lacked the skip of all-zero matrix slots, which    */
                                      /* the stored form now shares.  Runtime-switchable.                                     */

typedef struct hrag_opts {
    int32_t max_batch;    /* largest B any call will pass (workspace is sized once)              */
    int32_t max_topk;     /* largest k_p (retrieval_top_k), >= 1.  Above 2048 the final rankings */
                          /* take K4' (hrag_topk_rows_ws) and the workspace adds its scratch,    */
                          /* about max_batch * max_topk * 16 bytes when min(max_topk, passages)  */
                          /* > 16384 (none at or below that, none for max_topk <= 2048);         */
                          /* HRAG_ENOMEM if it does not fit                                      */
    int32_t slab_width;   /* PPR state slab width BC in {4,8,16,32,64}; 0 = auto                 */
    int32_t long_row_nnz; /* rows with more entries leave the G-lanes-per-row kernel and are cut  */
                          /* into wavefront-sized segments; 0 = auto (8 gather rounds)            */
    int32_t device;       /* HIP device ordinal, -1 = current                                    */
    int32_t flags;        /* tuning bits, 0 = defaults: HRAG_OPT_*                                  */
    int32_t segment_nnz;  /* entries per long-row segment (multiple of 64); 0 = auto (512)          */
    int32_t sell_seg_len; /* SELL-8 matrices (fp8 / fp16 / small-batch sweeps): rows longer than this are cut into */
                          /* segments whose partial sums are added in a fixed order.  0 = auto, from the work of one */
                          /* sweep of THIS engine (64 .. 2048).  The cut decides the summation order of long rows, so */
                          /* engines whose results must agree bit for bit (the row shards of a graph and the unsharded */
                          /* engine on it) have to be created with the same explicit value                            */
    int32_t sell_sigma;   /* SELL-8 matrices: sort rows by length inside windows of this many consecutive rows         */
                          /* (SELL-C-sigma) instead of globally.  0 = global sort (least padding; right for graphs       */
                          /* without locality such as the BASELINE generator).  With a vertex numbering that has         */
                          /* locality -- rows near each other share in-neighbours -- a window keeps the processing order */
                          /* close to the vertex order, so the gathered state rows are re-used from the XCD's L2; pair   */
                          /* it with HRAG_OPT_XCD_BLOCKED                                                                 */
    int32_t reserved[7];
} hrag_opts;

/* Phase timings of the last hrag_retrieve / hrag_score_facts on an engine, measured
 * with HIP events on the caller's stream (mirrors the reference's ppr_time /
 * rerank_time accumulators, HippoRAG.py:184-186).  Milliseconds. */
typedef struct hrag_timings {
    float fact_sim_ms;  /* fact GEMM + min/max + top-k           */
    float pass_sim_ms;  /* passage GEMM + min/max                */
    float seed_ms;      /* seed + teleport construction          */
    float ppr_ms;       /* all PPR iterations                    */
    float rank_ms;      /* normalise + gather + top-k            */
    float total_ms;
    int32_t ppr_iters;
    int32_t n_slabs;
    int32_t slab_width;
    int32_t n_long_rows;
} hrag_timings;

const char *hrag_last_error(void);
int hrag_version(void); /* major * 1000 + minor */

/* engine_create == prepare_retrieval_objects (HippoRAG.py:1287-1389): stage the graph,
 * the embedding matrices and the lookup arrays on the device once. `facts` / `fact_desc`
 * may be NULL for a DPR-only engine (StandardRAG). */
hrag_status hrag_engine_create(const hrag_graph_desc *graph, const hrag_embed_desc *facts,
                               const hrag_embed_desc *passages, const hrag_fact_desc *fact_desc,
                               const hrag_opts *opts, hrag_engine **out);
hrag_status hrag_engine_destroy(hrag_engine *e);

/* ------------------------------------------------------------------------------------------
 * Workspaces ("engine immutable after create -> concurrent read-only calls allowed on
 * distinct streams with distinct workspaces").  The reference serves one query at a time from one
 * Python thread (HippoRAG.py:459); a server that wants several retrieves in flight on ONE index makes
 * one workspace per stream / thread:
 *
 *   hrag_workspace_create(e, &w)   w is an engine HANDLE like e -- every entry point of this header takes
 *                                  it -- that BORROWS e's index (graph, SELL-8 matrices, embeddings, static
 *                                  tables: nothing is copied, no second 1.5 GB of embeddings) and OWNS a
 *                                  full set of per-call buffers (scores, PPR states, seeds, flags, the
 *                                  long-row arrival counters), its own entry flag, option flags
 *                                  (hrag_engine_set_flags acts on the handle it is given), events and
 *                                  timings.  Sized for e's max_batch / max_topk.
 *
 * Calls on e and on its workspaces may run CONCURRENTLY from different threads on different streams: a
 * handle rejects a second thread (HRAG_EBUSY) only for ITSELF.  Results are bit-identical to the same
 * call on e.  Rules: destroy every workspace (hrag_engine_destroy(w)) before the engine it came from
 * (hrag_engine_destroy(e) returns HRAG_EINVAL while workspaces are alive); the one entry point that
 * WRITES the index -- hrag_engine_gather_embeddings -- must not run while any other handle is in a call.
 * A workspace of a workspace is a workspace of the same root engine.
 * ------------------------------------------------------------------------------------------ */
hrag_status hrag_workspace_create(hrag_engine *e, hrag_engine **out);

/* What an engine handle holds and has done (SURVEY.md 8(b) hrag_stats).  Host-side, no device work. */
#define HRAG_PPR_STATE_F32 1    /* fp32 slabs (csrc/ppr_spmm.hip): every engine                                 */
#define HRAG_PPR_STATE_F16 2    /* two-stage fp16 state, 8 < batch <= 64 (csrc/ppr16.hip)                        */
#define HRAG_PPR_STATE_SMALL 4  /* batch <= 8 kernels (csrc/ppr_sv.hip)                                          */
#define HRAG_PPR_STATE_FP8 8    /* staged e4m3 state, batch > 64 and every row shard (csrc/ppr8.hip)             */
/* why an engine has NO staged e4m3 state -- its batches > 64 then run on the two-stage fp16 state (2 bytes per gathered
 * element instead of 1: about twice the sweep time) or, once V * 128 >= 2^32 (V >= 33.5 M), on the fp32 slabs (4 bytes);
 * same results within the same bar; hrag_shard_ppr_begin refuses such an engine.  hrag_stats.last_ppr_state says which
 * state a call ran on */
#define HRAG_FP8_UNAVAILABLE_NO_COL_SUM 1          /* hrag_graph_desc.col_sum was NULL                            */
#define HRAG_FP8_UNAVAILABLE_TOO_MANY_VERTICES 2   /* V + 1 > 2^24: the gather offsets are formed by a 24-bit     */
                                                   /* multiply ((V + 1) * 256 bytes must also stay below 2^32)   */
#define HRAG_FP8_UNAVAILABLE_SHARD_NOT_ALIGNED 4   /* owned passages != passages whose vertex is an owned row     */
#define HRAG_FP8_UNAVAILABLE_DISABLED 8            /* HRAG_OPT_F32_STATE / HRAG_OPT_NO_FP8 at creation             */
#define HRAG_FP8_UNAVAILABLE_SMALL_MAX_BATCH 16    /* unsharded engine with max_batch <= 64: never needed          */
typedef struct hrag_stats {
    int32_t is_workspace;       /* 1: the handle came from hrag_workspace_create                                  */
    int32_t live_workspaces;    /* workspaces of this engine that have not been destroyed                          */
    int64_t index_bytes;        /* device bytes of the shared half (graph, matrices, embeddings)                  */
    int64_t workspace_bytes;    /* device bytes of this handle's per-call half                                     */
    int32_t ppr_states;         /* HRAG_PPR_STATE_* the handle can run                                             */
    int32_t fp8_unavailable;    /* HRAG_FP8_UNAVAILABLE_* (0: the e4m3 state exists)                               */
    int32_t last_ppr_state;     /* HRAG_PPR_STATE_* the last hrag_retrieve / _scored on this handle ran on (0: none) */
    int32_t ppr8_r1_long_rows;  /* last e4m3-state PPR session of this handle: -1 = the first residual R_1 was stored for  */
                                /* every row (HRAG_OPT_STORE_R1 or a plan the recompute does not cover); n >= 0 = it was    */
                                /* recomputed at its boundary and only the n long rows kept the stored one (0: no session) */
    int64_t calls_score_facts, calls_retrieve, calls_dense_retrieve, calls_ppr, calls_shard;
    int64_t queries;            /* queries served by hrag_retrieve / _scored / hrag_dense_retrieve                  */
} hrag_stats;
hrag_status hrag_engine_stats(hrag_engine *e, hrag_stats *out);

/* Phase A == get_fact_scores (HippoRAG.py:1427-1465) + the candidate selection of
 * rerank_facts (:1683-1688) for B queries at once.
 *   q_fact_dev  bf16 [B, D]  "query_to_fact" embeddings, unit norm
 *   idx_out_dev int32 [B, k] fact ids (global), best first; -1 beyond min(k, F)
 *   score_out_dev fp32 [B, k] min-max normalised scores of those facts
 * The LLM filter (rerank.py:108-131) runs on the host between phase A and B. */
hrag_status hrag_score_facts(hrag_engine *e, const uint16_t *q_fact_dev, int32_t batch, int32_t k,
                             int32_t *idx_out_dev, float *score_out_dev, hrag_stream stream);

/* Phase B == graph_search_with_fact_entities (:1544-1656) + run_ppr (:1709-1749) +
 * the DPR fallback of retrieve (:467-469), for B queries at once.
 *   q_pass_dev       bf16 [B, D]  "query_to_passage" embeddings
 *   kept_idx_dev     int32 [B, kf] fact ids that survived the filter, in filter order
 *   kept_score_dev   fp32 [B, kf] their normalised scores (from phase A)
 *   kept_count_dev   int32 [B]    number of valid entries per row; 0 => DPR ranking
 *   doc_idx_out_dev  int32 [B, k] passage positions (index into passage_node_keys)
 *   doc_score_out_dev fp32 [B, k] PPR probability (or normalised DPR score on fallback)
 *   flags_out_dev    int32 [B]    bit0: DPR fallback used; bit1: reset vector had no mass
 *                                 bit2: the :1541 assert would fire (kept phrase weight 0)
 *                                 bit3: HRAG_FLAG_FP8_SATURATED -- a value of the fp8-state PPR left the e4m3
 *                                       range (a scale bound was violated; the scales are static powers of two at
 *                                       damping >= 0.46 and measured per stage below that and under
 *                                       HRAG_OPT_ACCEL): treat this query's scores as not trustworthy; rerun the
 *                                       batch after hrag_engine_set_flags(e, HRAG_OPT_NO_FP8, 1)
 *                                 bit4: HRAG_FLAG_NOT_CONVERGED -- ppr_tol > 0 and this query's residual (below)
 *                                       is still above it after ppr_max_iters sweeps: rerun with more sweeps
 *
 * Convergence contract of the PPR solve.  The reference hands the solve to PRPACK, which iterates until its
 * residual is below 1e-10 (HippoRAG.py:1736-1743); a fixed sweep count is only as accurate as the graph mixes.
 *   ppr_iters       sweeps that always run (20 in BASELINE.json)
 *   ppr_tol         0: exactly ppr_iters sweeps.  > 0: the engine measures, per query, the relative size of the
 *                   update its last sweep applied to the passage scores,
 *                       residual = damping / (1 - damping) * max over passages p of |x_p(K) - x_p(K-1)| / x_p(K)
 *                   (the error a contraction with factor `damping` has left after an update of that size), and
 *                   keeps sweeping -- decided ON THE DEVICE, no host synchronisation -- while that MEASURED residual
 *                   is above ppr_tol for some query of the batch and fewer than ppr_max_iters sweeps ran.  The
 *                   fp8-state path (batch > 64) extends in stages of 1, 2, 3, 3 sweeps up to 30 (the final sweep of a
 *                   stage runs over the passage rows only and measures; the launches of the next stage are enqueued
 *                   and skip themselves when a control word says so); the two-stage fp16 states (batch <= 64) extend
 *                   the same way by up to 9 sweeps beyond ppr_iters (stages of 1, 2, 3, 3 plain correction sweeps, each
 *                   closed by a measuring passage-row sweep); the fp32 states (other sweep counts / damping, the repeat
 *                   path) run the fixed count and report.
 *   ppr_max_iters   upper bound on the sweeps (>= ppr_iters; ignored when ppr_tol == 0)
 *   residual_out_dev fp32 [B] (may be NULL): the residual above for the sweeps that ran (0 on the DPR fallback)
 *   iters_out_dev   int32 [B] (may be NULL): sweeps that ran for the query's batch
 * The measure sees the passage rows only and is a heuristic, not a bound: where the error of a passage score is
 * fed from residual that sits on NON-passage rows (a slowly mixing graph with the seeds far from the passages: the
 * ring of tests/test_gpu_fp8_adversarial.py) it under-reads, down to 0.29 of the true error measured -- the mirror's
 * default ppr_tol = 1.5e-6 is the 1e-5 bar divided by that and by a margin of 1.9; where convergence oscillates
 * (bipartite-like graphs, the BASELINE generator) it over-reads by up to (1 + damping) / (1 - damping).  It does NOT
 * go blind on a bipartite graph: the iteration starts at x_0 = v, whose trailing term (damping P)^k v moves the
 * passage rows on every sweep, odd or even (tests/test_gpu_fp8_adversarial.py pins 20 and 21 sweeps).
 *
 * What a met tolerance bounds -- MEASURED over the adversarial suite and the randomised soaks, not proven:
 *       true relative error of every passage score  <=  max(HRAG_PPR_ERR_K * residual, floor)
 *   HRAG_PPR_ERR_K = 3.5: the worst under-reading of the measure (1 / 0.29, the ring graph);
 *   floor: what fp32 arithmetic on the state type leaves however small the measure reads -- the last sweep's update of
 *   a converged iterate rounds towards zero while the rounding of the stages before it stays (measured: a reported
 *   residual of 1.3e-8 next to a true error of 2.2e-7, 16k-vertex power-law graph, 257 queries, accelerated stages).
 *   HRAG_PPR_ERR_FLOOR_FP8 (staged e4m3 state, batch > 64, plain and HRAG_OPT_ACCEL), _F16 (two-stage fp16 states,
 *   batch <= 64), _F32 (fp32 state: other sweep counts / damping, HRAG_OPT_NO_FP8 | HRAG_OPT_NO_F16).  The floor of the
 *   e4m3 state depends on the graph (CPU emulation of the device arithmetic at 30 sweeps, where the measure reads
 *   < 1e-7: benchmark generator 4.4e-7, power-law 8.6e-7, star forest 3.8e-6); the constants are the largest values
 *   seen, rounded up.
 *   tests/test_gpu_accel.py and tests/test_gpu_fp8_adversarial.py assert the inequality query by query.
 * A tolerance below HRAG_PPR_TOL_MIN (the order of the smallest floor / K) promises nothing the arithmetic can deliver: hrag_retrieve,
 * hrag_retrieve_scored and hrag_shard_ppr_begin reject 0 < ppr_tol < HRAG_PPR_TOL_MIN with HRAG_EINVAL instead of
 * letting a caller believe it. */
#define HRAG_FLAG_NOT_CONVERGED 16
#define HRAG_PPR_ERR_K 3.5f
#define HRAG_PPR_ERR_FLOOR_FP8 5e-6f
#define HRAG_PPR_ERR_FLOOR_F16 2e-6f
#define HRAG_PPR_ERR_FLOOR_F32 5e-7f
#define HRAG_PPR_TOL_MIN 1e-7f
/* The reset vector ("personalization", HippoRAG.py:1574-1638) that every state path of hrag_retrieve /
 * hrag_retrieve_scored, the row shards and the hybrid mode hand to the PPR solve:
 *   seed order   phrases by descending fp64 mean weight, ties in first-occurrence order (the reference's order is
 *                that of a Python set: undefined); a phrase whose mean is NaN ranks above every number, NaN ties in
 *                first-occurrence order -- the top-k's NaN rule.  The link_top_k first are kept.
 *   seed_w       fp32(mean), sanitised: NaN, negative and zero become +0 (HippoRAG.py:1735 zeroes NaN / negative
 *                entries of the whole reset vector).  Flag bit 2 keeps its meaning: a kept phrase whose mean is exactly
 *                +-0 BEFORE sanitising (NaN and negative means are non-zero to the reference's count_nonzero).
 *   prior        minmax(score) * passage_node_weight with the row min / max over the numbers of the row (NaN skipped,
 *                hrag_row_minmax), then sanitised the same way on every path: an entry that is NaN or negative is 0.
 *                +-inf scores agree with the reference exactly ((inf - mn) / inf is NaN, every finite entry 0: the
 *                whole prior is 0).  The one difference: the reference's np.min propagates a NaN, so there one NaN
 *                passage zeroes the whole prior; here only that passage's entry is 0.  Everything derived from the
 *                prior -- the fp8 path's mass and scale bound, the fp16 scale -- is derived from the sanitised entries.
 *                "seeds" scope: the masked row keeps the NaN (the scoped DPR fallback ranks it first, as unscoped);
 *                the prior kernels that read it sanitise it.  An allowed set whose scores hold +-inf has no defined
 *                scoped prior (every allowed entry normalises to NaN or 0) and is not covered by this rule.
 * tests/test_gpu_reset_vector.py holds each part to its numpy restatement (tests/helpers.py seeds_np / prior_np). */
hrag_status hrag_retrieve(hrag_engine *e, const uint16_t *q_pass_dev, int32_t batch,
                          const int32_t *kept_idx_dev, const float *kept_score_dev,
                          const int32_t *kept_count_dev, int32_t kf, int32_t link_top_k,
                          float damping, float passage_node_weight, int32_t ppr_iters,
                          int32_t ppr_max_iters, float ppr_tol, int32_t k,
                          int32_t *doc_idx_out_dev, float *doc_score_out_dev,
                          int32_t *flags_out_dev, float *residual_out_dev, int32_t *iters_out_dev,
                          hrag_stream stream);

/* hrag_retrieve with the RAW passage scores supplied by the caller instead of computed from this engine's passage
 * embeddings: pass_scores_dev fp32 [B, pass_ld], np.dot(passage_embeddings, q) in passage order (HippoRAG.py:1496).
 * Everything else -- min-max, prior, seeds, PPR, ranking, the DPR fallback -- is hrag_retrieve's.  The PPR side of
 * the hybrid multi-GPU mode (hipporag_amd/dist.py HybridRetriever: embeddings row-sharded, the scores of a GPU's
 * queries arrive by an all-to-all, the PPR runs query-parallel on a replicated graph without any exchange).  Such an
 * engine can be created WITHOUT passage embeddings: hrag_embed_desc.data == NULL with rows = n_passages (and a fact
 * descriptor with rows == 0 next to a full hrag_fact_desc). */
hrag_status hrag_retrieve_scored(hrag_engine *e, const float *pass_scores_dev, int64_t pass_ld, int32_t batch,
                                 const int32_t *kept_idx_dev, const float *kept_score_dev,
                                 const int32_t *kept_count_dev, int32_t kf, int32_t link_top_k, float damping,
                                 float passage_node_weight, int32_t ppr_iters, int32_t ppr_max_iters, float ppr_tol,
                                 int32_t k, int32_t *doc_idx_out_dev, float *doc_score_out_dev, int32_t *flags_out_dev,
                                 float *residual_out_dev, int32_t *iters_out_dev, hrag_stream stream);

/* The scores of ALL passages of the engine's last hrag_retrieve / hrag_retrieve_scored (the array its top-k was taken
 * from: PPR probability, or the normalised DPR score on the fallback), fp32 [B, ld] in passage order.  The ranking of
 * any prefix of them (HippoRAG.py:501-507) is the call itself with k up to max_topk (any size; create the engine with
 * max_topk = n_passages for the full ranking), or hrag_topk_rows_ws on these rows.  Same stream discipline as every
 * call. */
hrag_status hrag_last_doc_scores(hrag_engine *e, int32_t batch, float *out_dev, int64_t ld, hrag_stream stream);

/* == dense_passage_retrieval (HippoRAG.py:1467-1502, StandardRAG.py:393-429), top-k only. */
hrag_status hrag_dense_retrieve(hrag_engine *e, const uint16_t *q_pass_dev, int32_t batch,
                                int32_t k, int32_t *doc_idx_out_dev, float *doc_score_out_dev,
                                hrag_stream stream);

/* ---- doc filter: exact top-k over a caller-chosen set of passages ----
 * A POST-filter: it decides which passages may appear in the ranked list and changes nothing else (phase A, the seeds,
 * the passage prior, the PPR, the min-max of the dense scores over ALL passages).  Per query the result is the first
 * min(k, |allowed|) entries of the unfiltered full ranking that are allowed, ids and scores bit-identical to those
 * entries; the slots beyond hold -1 / 0.  Queries on the DPR fallback (flags bit 0) follow the same rule on their
 * dense ranking.  An empty allowed set gives an all -1 row.  filter_dev == NULL is the unfiltered call, bit for bit.
 *
 * Mask format: a bitset of uint32 words; bit (j & 31) of word (j >> 5) is set when passage position j (the index
 * doc_idx_out uses) is allowed -- np.packbits(mask, bitorder="little") with the row padded to 4 bytes, read as
 * little-endian uint32.  filter_ld_words = 0: one row for the whole batch; otherwise >= ceil(n_passages / 32) words
 * per query row (HRAG_EINVAL below that).  Bits at or above n_passages are ignored.  A row shard reads the same GLOBAL
 * mask at bit offset p_offset (need not be a multiple of 32).  The filter costs one bit read per ranked score. */
hrag_status hrag_retrieve_filtered(hrag_engine *e, const uint16_t *q_pass_dev, int32_t batch,
                                   const int32_t *kept_idx_dev, const float *kept_score_dev,
                                   const int32_t *kept_count_dev, int32_t kf, int32_t link_top_k,
                                   float damping, float passage_node_weight, int32_t ppr_iters,
                                   int32_t ppr_max_iters, float ppr_tol, int32_t k,
                                   int32_t *doc_idx_out_dev, float *doc_score_out_dev,
                                   int32_t *flags_out_dev, float *residual_out_dev, int32_t *iters_out_dev,
                                   hrag_stream stream, const uint32_t *filter_dev, int64_t filter_ld_words);
hrag_status hrag_retrieve_scored_filtered(hrag_engine *e, const float *pass_scores_dev, int64_t pass_ld, int32_t batch,
                                          const int32_t *kept_idx_dev, const float *kept_score_dev,
                                          const int32_t *kept_count_dev, int32_t kf, int32_t link_top_k, float damping,
                                          float passage_node_weight, int32_t ppr_iters, int32_t ppr_max_iters,
                                          float ppr_tol, int32_t k, int32_t *doc_idx_out_dev, float *doc_score_out_dev,
                                          int32_t *flags_out_dev, float *residual_out_dev, int32_t *iters_out_dev,
                                          hrag_stream stream, const uint32_t *filter_dev, int64_t filter_ld_words);
hrag_status hrag_dense_retrieve_filtered(hrag_engine *e, const uint16_t *q_pass_dev, int32_t batch, int32_t k,
                                         int32_t *doc_idx_out_dev, float *doc_score_out_dev, hrag_stream stream,
                                         const uint32_t *filter_dev, int64_t filter_ld_words);

/* ---- scoped doc filter: the seeds and the passage prior come from the allowed passages ----
 * The doc filter above hides passages from the ranked list; the "seeds" scope also takes the query's evidence from them
 * only -- one tenant's documents inside a shared index.  For a query whose allowed passage set is A (same mask format
 * and filter_ld_words rule as above):
 *   phase A   hrag_score_facts_scoped: a fact is allowed when at least one passage it was extracted from is in A (the
 *             fact -> source table of hrag_engine_set_fact_sources; a fact without a source is never allowed).  The top
 *             k facts are taken among the allowed ones, their scores min-max normalised over the allowed facts' raw
 *             scores (a zero range gives 1).  Fewer than k allowed facts: the row ends in -1 / 0; none: all -1 -- a
 *             kept_count of 0 then sends the query to the DPR fallback of phase B (HippoRAG.py:467-469).
 *   prior     hrag_retrieve_scoped & co.: the raw passage scores are min-max normalised over A only (zero range: 1);
 *             passages outside A get prior 0.  Everything derived from the prior (its mass, the fp16 / fp8 scales)
 *             is derived from that masked prior.
 *   seeds     built from the kept facts exactly as in hrag_retrieve.  The divisor num_chunks of a phrase stays its
 *             GLOBAL count of chunks (a choice: the index has one ent_node_to_chunk_ids, not one per tenant).
 *   PPR       the whole graph, unchanged.  On an index that is a disjoint union of corpora (no shared entity, no edge
 *             between them) a scoped query over one corpus therefore sees exactly what an index of that corpus alone
 *             gives: the reset vector lives in its component and dangling mass returns to the reset vector.
 *   ranking   post-filtered by A exactly as hrag_retrieve_filtered.  DPR fallback / hrag_dense_retrieve_scoped: the
 *             dense ranking of A, normalised over A.
 *   empty A   the row is all -1 / 0 (no fault, no assert).
 * hrag_last_doc_scores after a scoped call: the PPR scores of every passage -- those outside A included, which can
 * receive mass through the graph -- or, on the DPR fallback, the dense score normalised over A and 0 outside it; with
 * an empty A the row carries no meaning.
 * A NULL filter is HRAG_EINVAL on the scoped calls (the unscoped calls are the "every passage" form). */

/* The fact -> source-passage table (proc_triples_to_docs, HippoRAG.py:1353-1361) as a CSR over host arrays: the
 * sources of fact f are passage_pos[row_ptr[f] .. row_ptr[f + 1]), passage positions in [0, n_passages).  n_facts must
 * be the engine's fact count.  Part of the shared index: call it on a root engine before any workspace is created
 * (HRAG_EINVAL after); workspaces created later borrow the table and get their own fact-mask buffer.  Calling it again
 * (still without workspaces) replaces the table.  An engine that never calls it allocates nothing for it.  A row-shard
 * engine takes the same global table and keeps the rows of its owned facts (hrag_shard_score_facts_scoped). */
hrag_status hrag_engine_set_fact_sources(hrag_engine *e, const int64_t *row_ptr, const int32_t *passage_pos,
                                         int64_t n_facts, int64_t nnz);

/* Test seam of the scoped phase A's first kernel: out_dev uint32 [rows, ceil(n_facts / 32)] (the mask format above),
 * bit f of row r set when one of fact f's sources (device CSR row_ptr_dev int64 [n_facts + 1], passage_pos_dev int32)
 * has bit (doc_bit_offset + passage) set in doc row r (doc_ld_words 0: one doc row for every output row, else >=
 * ceil((doc_bit_offset + n_docs) / 32)).  Sources outside [0, n_docs) count as not allowed. */
hrag_status hrag_fact_mask_from_docs(const uint32_t *doc_words_dev, int64_t doc_ld_words, int64_t doc_bit_offset,
                                     int64_t n_docs, int32_t rows, const int64_t *row_ptr_dev,
                                     const int32_t *passage_pos_dev, int64_t n_facts, uint32_t *out_dev,
                                     hrag_stream stream);

/* hrag_score_facts over the facts of the allowed passages (phase A above).  Without fact sources: HRAG_EINVAL. */
hrag_status hrag_score_facts_scoped(hrag_engine *e, const uint16_t *q_fact_dev, int32_t batch, int32_t k,
                                    int32_t *fact_idx_out_dev, float *fact_score_out_dev, hrag_stream stream,
                                    const uint32_t *filter_dev, int64_t filter_ld_words);

/* hrag_retrieve_filtered / hrag_retrieve_scored_filtered / hrag_dense_retrieve_filtered in the "seeds" scope (prior,
 * fallback and ranking above; the kept facts are the caller's -- from hrag_score_facts_scoped with the same filter). */
hrag_status hrag_retrieve_scoped(hrag_engine *e, const uint16_t *q_pass_dev, int32_t batch,
                                 const int32_t *kept_idx_dev, const float *kept_score_dev,
                                 const int32_t *kept_count_dev, int32_t kf, int32_t link_top_k,
                                 float damping, float passage_node_weight, int32_t ppr_iters,
                                 int32_t ppr_max_iters, float ppr_tol, int32_t k,
                                 int32_t *doc_idx_out_dev, float *doc_score_out_dev,
                                 int32_t *flags_out_dev, float *residual_out_dev, int32_t *iters_out_dev,
                                 hrag_stream stream, const uint32_t *filter_dev, int64_t filter_ld_words);
hrag_status hrag_retrieve_scored_scoped(hrag_engine *e, const float *pass_scores_dev, int64_t pass_ld, int32_t batch,
                                        const int32_t *kept_idx_dev, const float *kept_score_dev,
                                        const int32_t *kept_count_dev, int32_t kf, int32_t link_top_k, float damping,
                                        float passage_node_weight, int32_t ppr_iters, int32_t ppr_max_iters,
                                        float ppr_tol, int32_t k, int32_t *doc_idx_out_dev, float *doc_score_out_dev,
                                        int32_t *flags_out_dev, float *residual_out_dev, int32_t *iters_out_dev,
                                        hrag_stream stream, const uint32_t *filter_dev, int64_t filter_ld_words);
hrag_status hrag_dense_retrieve_scoped(hrag_engine *e, const uint16_t *q_pass_dev, int32_t batch, int32_t k,
                                       int32_t *doc_idx_out_dev, float *doc_score_out_dev, hrag_stream stream,
                                       const uint32_t *filter_dev, int64_t filter_ld_words);

/* ---- grouped retrieval: rank source documents, one best passage per source ----
 * An index is an index of chunks (passages); a caller who indexed sources -- papers, files -- as several passages each
 * asks for sources.  Every passage position p (the index doc_idx_out uses) belongs to one group g[p] in [0, n_groups),
 * 1 <= n_groups <= n_passages.  For one query with final passage scores s[p] (exactly what hrag_last_doc_scores returns)
 * and an optional doc filter:
 *   - only ALLOWED passages take part (no filter: all of them); a group with no allowed member does not appear;
 *   - REPRESENTATIVE of a group: its best allowed member under the ranking rule at the top of this header (score
 *     descending, ties -> larger passage position, every NaN above +inf);
 *   - GROUP SCORE: HRAG_GROUP_MAX -- the representative's score; HRAG_GROUP_SUM -- the sum of the allowed members' scores,
 *     accumulated in fp64 in ascending passage position and rounded once to fp32: numpy's
 *     np.bincount(g[allowed], weights=s[allowed].astype(np.float64), minlength=n_groups).astype(np.float32) bit for bit
 *     (NaN propagates; for PPR scores this is the walker's mass in the source);
 *   - groups are ranked by the same rule on (group score, group id): score descending, ties -> larger GROUP ID, NaN first.
 *     The result is the first min(k, groups with an allowed member) groups; the slots beyond hold -1 / 0 / -1.
 *   - queries on the DPR fallback (flags bit 0) follow the same rule on their normalised dense scores;
 *     the dense call: on the min-max normalised scores it returns (over the allowed passages in the "seeds" scope).
 * Consequence for HRAG_GROUP_MAX: when no two groups have bit-equal best scores, the grouped ranking is the ungrouped FULL
 * ranking with every passage but the first of each group removed, ids and scores bit-identical to those entries.
 * Nothing else changes: phase A, seeds, prior, PPR, the "seeds" scope, flags, residual and iteration outputs are those of
 * the ungrouped call; with no groups set, or through the other entry points, every output is what it was.
 * Cost: one read of the [B, n_passages] score rows (csrc/group.hip: no atomics -- one fixed-order chain of fp64 adds per
 * (query, group), so results are bitwise reproducible), then the ranking over n_groups instead of n_passages entries. */
#define HRAG_GROUP_MAX 0
#define HRAG_GROUP_SUM 1

/* The passage -> group table, host array group_of [n_passages] with 0 <= group_of[p] < n_groups (HRAG_EINVAL otherwise;
 * a group id that no passage carries is legal and never appears).  Part of the shared INDEX: accepted on a root engine
 * that has no live workspaces and is not inside a call (HRAG_EINVAL / HRAG_EBUSY otherwise), on neither a workspace handle
 * nor a row-shard engine; workspaces created afterwards borrow the table and get their own group buffers.  Calling it
 * again replaces the table; group_of == NULL clears it (n_groups is then ignored).  The per-call group buffers are
 * allocated here for the root and at creation for every later workspace -- never inside a retrieve call. */
hrag_status hrag_engine_set_passage_groups(hrag_engine *e, const int32_t *group_of, int64_t n_groups);

/* hrag_retrieve_filtered / hrag_retrieve_scored_filtered / hrag_dense_retrieve_filtered, grouped.  filter_dev may be NULL
 * (every passage); scoped != 0: the "seeds" scope of the scoped calls above (needs a filter).  agg: HRAG_GROUP_MAX /
 * HRAG_GROUP_SUM.  Outputs [B, k], k <= max_topk: group ids, group scores, the representative passage position of each
 * ranked group.  doc_idx_out_dev / doc_score_out_dev may be NULL; when given they receive the ungrouped ranking of the
 * same call (k entries, as the _filtered form writes them).  Without a group table: HRAG_EINVAL. */
hrag_status hrag_retrieve_grouped(hrag_engine *e, const uint16_t *q_pass_dev, int32_t batch,
                                  const int32_t *kept_idx_dev, const float *kept_score_dev,
                                  const int32_t *kept_count_dev, int32_t kf, int32_t link_top_k,
                                  float damping, float passage_node_weight, int32_t ppr_iters,
                                  int32_t ppr_max_iters, float ppr_tol, int32_t k,
                                  int32_t *doc_idx_out_dev, float *doc_score_out_dev,
                                  int32_t *flags_out_dev, float *residual_out_dev, int32_t *iters_out_dev,
                                  hrag_stream stream, const uint32_t *filter_dev, int64_t filter_ld_words,
                                  int32_t scoped, int32_t agg, int32_t *group_idx_out_dev, float *group_score_out_dev,
                                  int32_t *best_doc_idx_out_dev);
hrag_status hrag_retrieve_scored_grouped(hrag_engine *e, const float *pass_scores_dev, int64_t pass_ld, int32_t batch,
                                         const int32_t *kept_idx_dev, const float *kept_score_dev,
                                         const int32_t *kept_count_dev, int32_t kf, int32_t link_top_k, float damping,
                                         float passage_node_weight, int32_t ppr_iters, int32_t ppr_max_iters,
                                         float ppr_tol, int32_t k, int32_t *doc_idx_out_dev, float *doc_score_out_dev,
                                         int32_t *flags_out_dev, float *residual_out_dev, int32_t *iters_out_dev,
                                         hrag_stream stream, const uint32_t *filter_dev, int64_t filter_ld_words,
                                         int32_t scoped, int32_t agg, int32_t *group_idx_out_dev,
                                         float *group_score_out_dev, int32_t *best_doc_idx_out_dev);
hrag_status hrag_dense_retrieve_grouped(hrag_engine *e, const uint16_t *q_pass_dev, int32_t batch, int32_t k,
                                        int32_t *doc_idx_out_dev, float *doc_score_out_dev, hrag_stream stream,
                                        const uint32_t *filter_dev, int64_t filter_ld_words, int32_t scoped, int32_t agg,
                                        int32_t *group_idx_out_dev, float *group_score_out_dev,
                                        int32_t *best_doc_idx_out_dev);

/* The group reduction alone, engine-free: scores_dev fp32 [batch, ld] (n valid entries per row), the groups as a device
 * CSR -- group_ptr_dev int64 [n_groups + 1] from 0 to n, members_dev int32 [n] passage positions, ascending inside a
 * group (the order HRAG_GROUP_SUM adds in) -- and optionally the doc filter (format and filter_ld_words /
 * filter_bit_offset rule of hrag_topk_rows_masked; NULL: every element).  Writes gscore_out_dev fp32 and gbest_out_dev
 * int32, both [batch, out_ld], out_ld >= n_groups: the group score and the representative (-1 and score 0 for a group
 * without an allowed member).  A member outside [0, n) counts as not allowed. */
hrag_status hrag_group_rows(const float *scores_dev, int32_t batch, int64_t n, int64_t ld, const int64_t *group_ptr_dev,
                            const int32_t *members_dev, int64_t n_groups, int32_t agg, const uint32_t *filter_dev,
                            int64_t filter_ld_words, int64_t filter_bit_offset, float *gscore_out_dev,
                            int32_t *gbest_out_dev, int64_t out_ld, hrag_stream stream);

/* ---- grouped retrieval, group hits: the m best passages of each ranked source ----
 * A grouped call returns ONE passage per ranked group, the representative; a reader is fed the best few chunks of each of
 * the best sources.  For one query take its final passage scores s[p] (what hrag_last_doc_scores returns; after
 * hrag_dense_retrieve_grouped the min-max normalised scores that call ranked), the optional doc filter, and a ranked group
 * slot j holding group id g.  Then hits[j][0 .. m) are the first min(m, allowed members of g) entries of the ranking rule
 * at the top of this header restricted to the allowed members of g: score descending, ties -> larger passage position,
 * every NaN above +inf, -0 ties +0.  The slots beyond hold -1 / 0; a padded group slot (g == -1) gives an all -1 / 0 row.
 * Scores come back as every ranking returns them: the canonical quiet NaN, -0 as +0.  Consequences:
 *   1. hits[j][0] == best_doc_idx[j] for both aggregators.  HRAG_GROUP_MAX: its score equals the group score bit for
 *      bit; HRAG_GROUP_SUM: the hits carry each member's own score, not the sum.
 *   2. The hits of group g are the ungrouped filtered ranking (hrag_retrieve_filtered, "ranking" scope) of the same
 *      query under the filter (allowed AND member of g), ids and scores bit-identical -- without a second PPR.
 *   3. m == 1 returns what the grouped call already did.
 * 1 <= m <= HRAG_GROUP_HITS_MAX (one wavefront holds the list); anything else is HRAG_EINVAL before anything is enqueued.
 * Cost: one wavefront per (query, ranked slot) reads that group's members and their scores once (csrc/group.hip); no
 * atomics, no allocation, no synchronisation, no read-back -- capture-safe like the calls it follows. */
#define HRAG_GROUP_HITS_MAX 64

/* The selection alone, engine-free, beside hrag_group_rows with the same argument rules and checks: scores_dev, the group
 * CSR and the filter as there; group_idx_dev int32 [batch, k], each entry a group id or -1 (an id outside [0, n_groups)
 * counts as -1; ids may repeat).  Writes hit_idx_out_dev int32 and hit_score_out_dev fp32, both [batch, k, hits]. */
hrag_status hrag_group_hits_rows(const float *scores_dev, int32_t batch, int64_t n, int64_t ld,
                                 const int64_t *group_ptr_dev, const int32_t *members_dev, int64_t n_groups,
                                 const int32_t *group_idx_dev, int32_t k, int32_t hits, const uint32_t *filter_dev,
                                 int64_t filter_ld_words, int64_t filter_bit_offset, int32_t *hit_idx_out_dev,
                                 float *hit_score_out_dev, hrag_stream stream);

/* The hits of ranked groups over the score rows the handle's LAST retrieve, scored or grouped dense call left -- the rows
 * hrag_last_doc_scores reads; after hrag_dense_retrieve_grouped the normalised rows -- with the engine's group table.  A
 * follow-up call: issue it right after the grouped call (same handle, the usual stream and one-call-per-handle rules;
 * a workspace handle has its own rows), with the group ids that call returned and the filter it was given (NULL: every
 * passage).  The ids need not come from a grouped call: any [batch, k] ids in [-1, n_groups) are legal, k >= 1 is not
 * bound by max_topk.  The handle records the batch of the call that last wrote its rows; an ungrouped hrag_dense_retrieve*
 * call does not write them (it ranks the raw similarity rows), so the record then still names the call before it.
 * HRAG_EINVAL: no group table, a row-shard engine, no rows written yet on this handle, batch above the recorded one,
 * hits outside [1, HRAG_GROUP_HITS_MAX], k < 1; the outputs are then untouched. */
hrag_status hrag_last_group_hits(hrag_engine *e, int32_t batch, const int32_t *group_idx_dev, int32_t k, int32_t hits,
                                 const uint32_t *filter_dev, int64_t filter_ld_words, int32_t *hit_idx_out_dev,
                                 float *hit_score_out_dev, hrag_stream stream);

/* ---- fused retrieval: one ranking per QUESTION from several member queries ----
 * A multi-hop caller sends a question as several strings -- sub-questions, paraphrases, the thoughts of an IRCoT chain
 * (retrieve_ircot merges their document scores by max, HippoRAG.py:526-543) -- and wants ONE ranked list.  A batch of B
 * member rows is cut into Q questions by member_ptr int32 [Q + 1]: member_ptr[0] = 0, member_ptr[Q] = B, strictly
 * increasing -- every question has at least one member and its members are consecutive rows.  weight fp32 [B], NULL = all
 * 1; every weight finite and >= 0.  With s_i(p) the final score of passage p for member i (hrag_last_doc_scores) the
 * fused row of question q over ALL n_passages columns is
 *   HRAG_FUSE_SUM  the fp64 chain acc = +0.0; acc += (double)w_i * (double)s_i(p) in member order, rounded once to fp32
 *                  (the product of two fp32 values is exact in fp64); a NaN result is the quiet NaN 0x7fc00000;
 *   HRAG_FUSE_MAX  the member score with the largest ranking key under the rule at the top of this header (any NaN wins),
 *                  as the ranking returns scores: the quiet NaN, -0 as +0.  Takes no weights (HRAG_EINVAL);
 *   HRAG_FUSE_RRF  reciprocal rank fusion with a constant c >= 0 (the usual 60) and a depth d, 1 <= d <= min(max_topk,
 *                  n_passages): every member row is ranked at depth d by the rule at the top of this header, under its
 *                  question's filter row; a passage at 1-based rank r of member i contributes
 *                  t = (float)((double)w_i / (double)(c + r)), and the fused value is the fp32 chain acc = 0.0f;
 *                  acc = acc + t in member order over the members that list the passage.  A passage no member lists has
 *                  fused score +0.0 (among the allowed passages it ranks behind every listed one, by the usual tie rule).
 * No atomics anywhere (csrc/fuse.hip): every value is one chain in a fixed order, bitwise reproducible.
 * After a fusion rows [0, Q) of the handle's score rows hold the fused rows, the recorded batch of the rows becomes Q, rows
 * >= Q are unspecified; the fused rows are then ranked exactly as a retrieve call ranks its rows -- hrag_last_doc_scores
 * and hrag_last_group_hits with batch <= Q work on them unchanged. */
#define HRAG_FUSE_SUM 0
#define HRAG_FUSE_MAX 1
#define HRAG_FUSE_RRF 2

/* Sum / max alone, engine-free and IN PLACE: scores_dev fp32 [batch, ld] (n valid entries per row; the columns n .. ld
 * are neither read nor written), member_ptr_dev int32 [n_fused + 1] and weight_dev fp32 [batch] (or NULL) DEVICE arrays
 * that follow the rules above (they cannot be checked here; whatever they hold, nothing outside the rows is touched).
 * mode: HRAG_FUSE_SUM / HRAG_FUSE_MAX.  Rows [0, n_fused) receive the fused rows.  Serves dense fusion over
 * hrag_sim_scores output as well. */
hrag_status hrag_fuse_rows(float *scores_dev, int32_t batch, int64_t n, int64_t ld, const int32_t *member_ptr_dev,
                           int32_t n_fused, const float *weight_dev, int32_t mode, hrag_stream stream);

/* The scatter of HRAG_FUSE_RRF alone, engine-free: list_idx_dev int32 [batch, depth] the ranked lists of the member rows
 * (slot j = rank j + 1; -1 or an id outside [0, n): skipped; the ids of one row must be unique), device member_ptr /
 * weight as above, c >= 0.  out_dev fp32 [n_fused, ld] is zeroed over its n columns and filled. */
hrag_status hrag_rrf_rows(const int32_t *list_idx_dev, int32_t batch, int32_t depth, const int32_t *member_ptr_dev,
                          int32_t n_fused, const float *weight_dev, int32_t c, float *out_dev, int64_t n, int64_t ld,
                          hrag_stream stream);

/* Bytes of workspace hrag_last_fused needs (16-byte aligned device memory, scratch only): the copies of member_ptr and
 * weight; HRAG_FUSE_RRF adds the member lists [batch, depth] and, with one filter row per question
 * (per_question_filter != 0), the per-member filter rows.  Negative on a bad argument. */
int64_t hrag_fuse_workspace_bytes(int32_t batch, int64_t n_passages, int32_t mode, int32_t depth,
                                  int32_t per_question_filter);

/* The fusion over the score rows the handle's last retrieve, scored or grouped dense call left, then their ranking: a
 * follow-up call like hrag_last_group_hits (same handle, stream and one-call-per-handle rules; a workspace handle has
 * its own rows).  batch <= the recorded batch of the rows; member_ptr [n_fused + 1] and weight [batch] (or NULL) are
 * HOST arrays, validated before anything is enqueued and copied into the workspace on `stream` (keep them valid until
 * the stream has passed the call).  rrf_c / rrf_depth: HRAG_FUSE_RRF only.  filter_dev: NULL, one row for every question
 * (filter_ld_words 0) or one row per QUESTION; it applies to the RRF member rankings and to the final ranking.
 * Outputs, each set optional: doc_idx_out_dev / doc_score_out_dev [n_fused, k] the ungrouped ranking of the fused rows
 * under the filter; group_agg >= 0 (HRAG_GROUP_MAX / HRAG_GROUP_SUM; negative: no grouping) the grouped ranking
 * group_idx_out_dev / group_score_out_dev / best_doc_idx_out_dev [n_fused, k] as hrag_retrieve_grouped writes it.
 * 1 <= k <= max_topk when an output is given.  Nothing is allocated, synchronised or read back.
 * HRAG_EINVAL (nothing enqueued, outputs and rows untouched): a row-shard engine (its rows are slices of the passages),
 * no rows written yet on this handle, batch above the recorded one, member_ptr / weight / mode / c / depth / k outside
 * the rules above, weights with HRAG_FUSE_MAX, a workspace that is too small or misaligned. */
hrag_status hrag_last_fused(hrag_engine *e, int32_t batch, const int32_t *member_ptr, int32_t n_fused,
                            const float *weight, int32_t mode, int32_t rrf_c, int32_t rrf_depth, int32_t k,
                            const uint32_t *filter_dev, int64_t filter_ld_words, int32_t group_agg,
                            int32_t *doc_idx_out_dev, float *doc_score_out_dev, int32_t *group_idx_out_dev,
                            float *group_score_out_dev, int32_t *best_doc_idx_out_dev, void *workspace_dev,
                            size_t workspace_bytes, hrag_stream stream);

/* ---- diversified retrieval: MMR re-ranking of the candidates a ranking returned ----
 * A ranking by score alone puts near-duplicate passages (overlapping chunk windows, the same paragraph in two sources)
 * next to each other.  Maximal Marginal Relevance picks k of c candidates greedily, trading each candidate's relevance
 * against its similarity to what is already picked.  One query has
 *   candidates  cand_idx[0 .. c): passage positions; -1 or an id outside [0, n_passages) is an EMPTY slot;
 *   scores      cand_score[0 .. c), in the order some ranking returned them;
 *   lambda      in [0, 1], fp32;   k with 1 <= k <= c <= HRAG_MMR_MAX_CANDIDATES.
 * Relevance: mn / mx = fminf / fmaxf over the scores of the non-empty slots, starting from +inf / -inf;
 *   rel[i] = (s[i] - mn) / (mx - mn), one fp32 subtraction each and one fp32 division (min_max_normalize,
 *   misc_utils.py:130-139); rel[i] = 1.0f for every slot when mx == mn; normalize == 0: rel[i] = s[i].
 * Similarity G[i][j] for slots i < j: the score hrag_sim_gemm gives for embedding row cand_idx[i] against row cand_idx[j]
 *   used as the QUERY -- the same v_mfma_f32_16x16x32 chain, k ascending, one fp32 accumulator.  On a split engine the
 *   query side takes its thirds as [hi | hi | lo], read from the stored [hi | lo | hi] row.  G[j][i] = G[i][j] by
 *   definition (bf16 / fp16 / split need no second product); G[i][i] is not used.
 * Selection, step t = 0 .. k - 1, over the non-empty, not yet selected slots:
 *   pen[i] = fmaxf over the selected j, in selection order, of G[i][j];   mu = 1.0f - lambda in fp32;
 *   value[i] = (float)((double)lambda * (double)rel[i]) at t = 0,
 *              (float)((double)lambda * (double)rel[i] - (double)mu * (double)pen[i]) afterwards (both products are exact
 *              in fp64: one fp64 subtraction, one rounding);
 *   the slot with the largest ranking key of `value` is selected (the rule at the top of this header: every NaN above
 *   +inf, -0 ties +0); ties go to the SMALLER slot, the earlier place in the caller's ranking -- lambda = 1 over a
 *   ranking's finite scores returns its first k candidates unchanged.
 * Outputs per query, each [k]: sel_out the slots, idx_out the passage positions, score_out the candidates' own scores and
 * value_out the value of each pick, both canonical as every ranking returns scores (the quiet NaN, -0 as +0); once the
 * non-empty slots run out the remaining entries are -1 / -1 / 0 / 0.  No atomics: every value is one chain in a fixed
 * order, bitwise reproducible (csrc/mmr.hip). */
#define HRAG_MMR_MAX_CANDIDATES 1024

/* The gathered Gram of each query's candidates, engine-free: emb_dev the 16-bit rows [rows, kdim] (dtype HRAG_BF16 /
 * HRAG_FP16; kdim a multiple of 8, 16-byte aligned; split != 0: rows in the [hi | lo | hi] layout of hrag_split_f32,
 * kdim = 3 * dim), cand_idx_dev int32 [batch, c], 1 <= c <= HRAG_MMR_MAX_CANDIDATES.  out_dev fp32 [batch, c, ld],
 * ld >= c: element [i][j] = G[min(i, j)][max(i, j)] as defined above; an empty slot (id outside [0, rows)) gives +0.0 in
 * its row and column; the diagonal holds the row's product with itself as the query; the columns c .. ld are not
 * touched. */
hrag_status hrag_gram_rows(const uint16_t *emb_dev, int64_t rows, int32_t kdim, int32_t dtype, int32_t split,
                           const int32_t *cand_idx_dev, int32_t batch, int32_t c, float *out_dev, int64_t ld,
                           hrag_stream stream);

/* The selection alone, engine-free, over any caller-supplied similarity sim_dev fp32 [batch, c, ld]: score_dev fp32 and
 * cand_idx_dev int32 [batch, c]; outputs [batch, k].  There is no passage count here: a NEGATIVE id is an empty slot.
 * After slot j was selected the call reads ROW j of the matrix, pen[i] = fmaxf(pen[i], sim[j][i]): on a symmetric matrix
 * (what hrag_gram_rows writes) that is the definition's G[i][j]. */
hrag_status hrag_mmr_rows(const float *score_dev, const int32_t *cand_idx_dev, const float *sim_dev, int64_t ld,
                          int32_t batch, int32_t c, int32_t k, float lambda, int32_t normalize, int32_t *sel_out_dev,
                          int32_t *idx_out_dev, float *score_out_dev, float *value_out_dev, hrag_stream stream);

/* Bytes of workspace hrag_mmr needs (16-byte aligned device memory, scratch only): the [batch, c, round_up(c, 4)] fp32
 * Gram matrix.  Negative on a bad argument. */
int64_t hrag_mmr_workspace_bytes(int32_t batch, int32_t c);

/* The two steps over the engine's passage embeddings.  It reads only the index half, so it works on a workspace handle
 * and after any call that produced ids and scores: hrag_retrieve*, the dense calls, the representatives and group scores
 * of a grouped call, a fused ranking.  Bit-identical to hrag_gram_rows (ld = round_up(c, 4)) followed by hrag_mmr_rows on
 * the same buffers whenever no id is >= n_passages (such an id is an empty slot here).  The usual one-call-per-handle and
 * stream rules; nothing is allocated, synchronised or read back (capture safe).
 * HRAG_EINVAL (nothing enqueued, outputs untouched): a row-shard engine (it holds a slice of the passages), an engine
 * without passage embeddings, c outside [1, HRAG_MMR_MAX_CANDIDATES], k outside [1, c], lambda outside [0, 1] or NaN,
 * batch outside [1, max_batch], a NULL pointer, a workspace that is too small or misaligned. */
hrag_status hrag_mmr(hrag_engine *e, const int32_t *cand_idx_dev, const float *cand_score_dev, int32_t batch, int32_t c,
                     int32_t k, float lambda, int32_t normalize, int32_t *idx_out_dev, float *score_out_dev,
                     float *value_out_dev, void *workspace_dev, size_t workspace_bytes, hrag_stream stream);

/* hrag_mmr that also writes the selected SLOTS: sel_out_dev int32 [batch, k] (NULL: hrag_mmr), the position of each pick in
 * the caller's candidate row (-1 once the candidates run out) -- what a caller needs to carry anything else that came with
 * the candidates (the group ids of a grouped ranking) along with the picks. */
hrag_status hrag_mmr_sel(hrag_engine *e, const int32_t *cand_idx_dev, const float *cand_score_dev, int32_t batch, int32_t c,
                         int32_t k, float lambda, int32_t normalize, int32_t *sel_out_dev, int32_t *idx_out_dev,
                         float *score_out_dev, float *value_out_dev, void *workspace_dev, size_t workspace_bytes,
                         hrag_stream stream);

/* ---- late-interaction reranking: MaxSim over per-token embeddings of the candidates a ranking returned ----
 * A passage embedding is one vector, the mean of what the passage says; the rankings above order the candidates by that
 * one vector whatever the individual query tokens match.  Late interaction (ColBERT's MaxSim; the multivector max_sim /
 * rank_vectors of search engines) scores a candidate by its best-matching token for every query token.  ("rerank" names
 * the reference's LLM fact filter in this project: the option is called LATE everywhere.)
 *
 * A TOKEN INDEX holds, for n passages,
 *   tok_ptr   int64 [n + 1], ascending, tok_ptr[0] = 0; passage p owns the token rows tok_ptr[p] .. tok_ptr[p + 1] - 1
 *             (an empty range is allowed);
 *   tok_emb   16-bit [T, dim] on the device, T = tok_ptr[n]: HRAG_BF16 or HRAG_FP16 by the dtype code, as in
 *             hrag_sim_gemm; dim a multiple of 8 with 8 <= dim <= HRAG_LATE_MAX_DIM; the base pointer 16-byte aligned.
 * It is an object of its own, like hrag_lex and hrag_payload: its vectors are NOT the engine's passage embeddings, and
 * there is no split-fp32 form.
 * A BATCH OF LATE QUERIES is q_ptr int32 [batch + 1] (ascending from 0) and q_tok 16-bit [q_ptr[batch], dim] on the
 * device in the index's dtype, 16-byte aligned; at most HRAG_LATE_MAX_QUERY_TOKENS tokens per query.
 *
 * For query b and candidate slot s holding passage p = cand_idx[b][s]:
 *   s_ij   = the fp32 dot product of query token i and passage token j: the products are exact, the fp32 accumulation
 *            runs on v_mfma_f32_16x16x32_{bf16,f16}, the k tail zero-filled in 8-element chunks;
 *   m_i    = fmaxf over j in [tok_ptr[p], tok_ptr[p + 1]) of s_ij, starting from -inf (np.fmax: a NaN s_ij is ignored);
 *   score  = (float)(sum over i, in ascending order, of (double)m_i) + 0.0f: one rounding, -0 becomes +0; a NaN is the
 *            quiet NaN 0x7fc00000.
 * A passage without tokens scores -inf when the query has tokens; a query without tokens scores +0.0 everywhere.  An
 * EMPTY slot (id < 0 or id >= n) has no score: it reads 0.0 in the scores output and never ranks.  Rows beyond a
 * passage's last token and columns beyond a query's last token are masked, not zero-filled, and no load reaches past
 * tok_ptr[p + 1].
 * RANKING: the live slots ordered by the ranking key of this header (every NaN above +inf, -0 ties +0), a tie to the
 * SMALLER slot -- the earlier first-stage rank, the tie rule of hrag_mmr; the first k as (sel, idx, score), score
 * canonical, and -1 / -1 / 0 once the live slots run out.  1 <= k <= c <= HRAG_LATE_MAX_CANDIDATES.
 * No atomics, every output written exactly once: the score of a (query, passage) pair has the same bits at any batch,
 * in any slot, next to any neighbours (csrc/late.hip). */
#define HRAG_LATE_MAX_DIM 256
#define HRAG_LATE_MAX_QUERY_TOKENS 64
#define HRAG_LATE_MAX_CANDIDATES 1024

typedef struct hrag_late hrag_late; /* opaque; independent of any engine: engines and workspaces over the same passages share one */

/* The index over tok_ptr (HOST, validated here, copied to the current device) and tok_emb_dev (DEVICE, kept by
 * reference: it must outlive the index; nothing of it is copied).  HRAG_EINVAL, and nothing is allocated: tok_ptr[0] != 0
 * or tok_ptr descending, dim not a multiple of 8 or outside [8, HRAG_LATE_MAX_DIM], a dtype other than HRAG_BF16 /
 * HRAG_FP16, a misaligned or missing tok_emb_dev, n_passages outside [1, 2^31). */
hrag_status hrag_late_create(int64_t n_passages, const int64_t *tok_ptr, const uint16_t *tok_emb_dev, int32_t dim,
                             int32_t dtype, hrag_late **out);
hrag_status hrag_late_destroy(hrag_late *ix);

/* The scores above: out_dev fp32 [batch, ld], ld >= c, the columns c .. ld not touched; cand_idx_dev int32 [batch, c].
 * q_ptr is read on the HOST (the rules are checked before anything is enqueued: HRAG_EINVAL for q_ptr[0] != 0, a
 * descending q_ptr, a query of more than HRAG_LATE_MAX_QUERY_TOKENS tokens, c outside [1, HRAG_LATE_MAX_CANDIDATES],
 * ld < c, a NULL or misaligned pointer) and q_ptr_dev is the same array on the device, which the kernel reads (were it to
 * differ, its ranges are clamped to q_tok's q_ptr[batch] rows and the cap).  Enqueues on `stream`; nothing is allocated,
 * synchronised or read back.  Any number of calls may read one index at the same time. */
hrag_status hrag_late_scores(const hrag_late *ix, const int32_t *q_ptr, const int32_t *q_ptr_dev, const uint16_t *q_tok_dev,
                             int32_t batch, const int32_t *cand_idx_dev, int32_t c, float *out_dev, int64_t ld,
                             hrag_stream stream);

/* The ranking above over any score rows scores_dev fp32 [batch, ld] of candidates cand_idx_dev int32 [batch, c],
 * engine-free: outputs [batch, k]; sel_out_dev may be NULL.  n_ids > 0: an id >= n_ids is an empty slot too; n_ids <= 0:
 * a negative id only.  HRAG_EINVAL: c or k out of range, ld < c, a NULL pointer. */
hrag_status hrag_late_rank_rows(const float *scores_dev, int64_t ld, const int32_t *cand_idx_dev, int64_t n_ids,
                                int32_t batch, int32_t c, int32_t k, int32_t *sel_out_dev, int32_t *idx_out_dev,
                                float *score_out_dev, hrag_stream stream);

/* Bytes of workspace hrag_late_rerank needs (16-byte aligned device memory, scratch only): the [batch, round_up(c, 4)]
 * fp32 scores.  Negative on a bad argument. */
int64_t hrag_late_workspace_bytes(int32_t batch, int32_t c);

/* The two steps: bit-identical to hrag_late_scores (ld = round_up(c, 4)) followed by hrag_late_rank_rows with
 * n_ids = n_passages on the same buffers; afterwards the workspace holds the scores of every slot. */
hrag_status hrag_late_rerank(const hrag_late *ix, const int32_t *q_ptr, const int32_t *q_ptr_dev, const uint16_t *q_tok_dev,
                             int32_t batch, const int32_t *cand_idx_dev, int32_t c, int32_t k, int32_t *sel_out_dev,
                             int32_t *idx_out_dev, float *score_out_dev, void *workspace_dev, size_t workspace_bytes,
                             hrag_stream stream);

/* ---- recommend by example: score rows from liked and disliked passage ids, no query vector ----
 * Every ranking above starts from a query vector.  "More like these passages, less like those" (the recommend call of
 * vector databases, more_like_this of search engines) starts from passage ids: a reader's relevance feedback, a user's
 * liked and dismissed results.  One query b has a list of EXAMPLES ex_idx[ex_ptr[b] .. ex_ptr[b + 1]) with ex_sign +1
 * (positive) or -1 (negative), all int32.  The ids are passage positions; an id outside [0, n_passages) or a sign 0 is an
 * EMPTY example: it contributes nothing (it is skipped, not scored as 0).  Repeats are legal.  At most
 * HRAG_RECO_MAX_EXAMPLES examples of a query are read, later ones are ignored on the device, as HRAG_LEX_MAX_QUERY_TERMS
 * is (the Python binding refuses longer lists).
 * s(p, e) is the score hrag_sim_gemm gives passage row p with embedding row ex_idx[e] used as the QUERY -- the same
 * v_mfma_f32_16x16x32 chain: BK = 64 steps of two MFMAs in ascending k into one fp32 accumulator, the k tail zero-filled
 * in 8-element chunks; on a split engine the query side reads the stored [hi | lo | hi] row's thirds in the order
 * (0, 2, 1): exactly what hrag_gram_rows promises.  (hrag_sim_gemm itself serves batches of one or two queries by a
 * dot-product kernel with another summation order; "the score hrag_sim_gemm gives" is that of a batch of three or more.)
 * The score rows are out[b][p] for every p in [0, n_passages); columns beyond n_passages are not touched.
 * HRAG_RECO_BEST_SCORE (Qdrant's best_score):
 *     bp = bn = -inf
 *     for each positive in list order: if (s > bp) bp = s
 *     for each negative in list order: if (s > bn) bn = s        plain >, so a NaN is never taken
 *     out = bp > bn ? bp : -(bn * bn)                             one fp32 product
 *   No examples at all gives -inf.
 * HRAG_RECO_SUM_SCORES:
 *     acc = +0.0 (fp64);  acc += (double)s for the positives in list order;  acc -= (double)s for the negatives in list
 *     order;  out = acc rounded once to fp32.  A NaN result is the quiet NaN 0x7fc00000, as in hrag_fuse_rows.
 * HRAG_RECO_AVERAGE_VECTOR produces no rows but a QUERY per b, which then goes through the ordinary calls.  Per
 *   component k, in fp64 with every operation rounded on its own and no contraction:
 *     a = (sum over the positives in list order of value(e, k)) / n_pos;   g = the same over the negatives;
 *     v = a + (a - g) when n_neg > 0, v = a when n_neg == 0
 *   value is the stored 16-bit value, or hi + lo on a split engine.  v is rounded to fp32 and then written as the
 *   engine's query type: bf16 / fp16 round-to-nearest-even, or [qhi | qhi | qlo] exactly as hrag_split_f32(as_query = 1)
 *   makes it from that fp32 vector.  It is not normalised: every ranking here is invariant to a positive scale of the
 *   query, so the returned scores are dot products with v, not cosines.  n_pos == 0 gives the all-zero query and sets
 *   bit 0 of flags_out[b].
 * EXCLUSION: the doc filter of query b with the bits of its non-empty example ids cleared (every strategy): a call
 *   without a filter starts from all n bits set, a filter given as one shared row (ld 0) is expanded to one row per query
 *   first -- both by the caller; hrag_reco_exclude clears the bits.
 * No atomics; every output word is written once, by plain vector stores; results are bitwise reproducible at any batch
 * and at any position in it (csrc/reco.hip). */
#define HRAG_RECO_MAX_EXAMPLES 32
#define HRAG_RECO_TILE 128          /* passages per workgroup of the fused kernel */
#define HRAG_RECO_BEST_SCORE 0
#define HRAG_RECO_SUM_SCORES 1
#define HRAG_RECO_AVERAGE_VECTOR 2  /* hrag_reco_query; not a mode of the row calls */

/* The reduce alone, engine-free, over caller-supplied example score rows ex_scores_dev fp32 [E, ld] (row ex_ptr[b] + e
 * holds s(., e) of query b's example e): out_dev fp32 [batch, ld_out], n columns each.  ex_ptr_dev int32 [batch + 1] and
 * ex_sign_dev int32 [E] on the device; there are no ids here: an empty example is a sign 0; there is no host ex_ptr
 * either: the device-side one is taken as it is, a range cut at HRAG_RECO_MAX_EXAMPLES.  mode: HRAG_RECO_BEST_SCORE
 * or HRAG_RECO_SUM_SCORES.  HRAG_EINVAL: a NULL pointer, a bad mode, batch outside [1, 65535], ld or ld_out below n. */
hrag_status hrag_reco_rows(const float *ex_scores_dev, int64_t ld, const int32_t *ex_ptr_dev, const int32_t *ex_sign_dev,
                           int32_t batch, int64_t n, int32_t mode, float *out_dev, int64_t ld_out, hrag_stream stream);

/* Bytes of workspace the fused calls need (16-byte aligned device memory, scratch only): the column table -- (id, sign)
 * of the 32 columns of every query -- and the example counts.  Negative on a bad argument. */
int64_t hrag_reco_workspace_bytes(int32_t batch);

/* The fused product-and-reduce, engine-free: emb_dev the 16-bit rows [rows, kdim] (dtype, kdim, split as in
 * hrag_gram_rows); ex_ptr is read on the HOST (ex_ptr[0] == 0, ascending: checked before anything is enqueued) and
 * ex_ptr_dev is the same array on the device, which the kernels read (were it to differ, its ranges are clamped to
 * ex_ptr[batch] examples and the cap); ex_idx_dev / ex_sign_dev int32 [ex_ptr[batch]].  out_dev fp32 [batch, ld],
 * ld >= rows.  Bit-identical to gathering the example rows (on split: as queries [hi | hi | lo]), hrag_sim_gemm of three
 * or more of them into [E, rows], and hrag_reco_rows with the empty examples' signs 0 -- the [E, rows] matrix stays in
 * MFMA accumulators.  Nothing is allocated, synchronised or read back. */
hrag_status hrag_reco_scores_rows(const uint16_t *emb_dev, int64_t rows, int32_t kdim, int32_t dtype, int32_t split,
                                  const int32_t *ex_ptr, const int32_t *ex_ptr_dev, const int32_t *ex_idx_dev,
                                  const int32_t *ex_sign_dev, int32_t batch, int32_t mode, float *out_dev, int64_t ld,
                                  void *workspace_dev, size_t workspace_bytes, hrag_stream stream);

/* The same over the engine's passage embeddings.  It reads only the index half, so it works on a workspace handle.  The
 * usual one-call-per-handle and stream rules.  HRAG_EINVAL (nothing enqueued, outputs untouched): a row-shard engine, an
 * engine without passage embeddings, batch outside [1, max_batch], a bad mode, a NULL pointer, a short or misaligned
 * workspace. */
hrag_status hrag_reco_scores(hrag_engine *e, const int32_t *ex_ptr, const int32_t *ex_ptr_dev, const int32_t *ex_idx_dev,
                             const int32_t *ex_sign_dev, int32_t batch, int32_t mode, float *out_dev, int64_t ld,
                             void *workspace_dev, size_t workspace_bytes, hrag_stream stream);

/* HRAG_RECO_AVERAGE_VECTOR: q_out_dev 16-bit [batch, kdim] (kdim = dim, or 3 * dim on a split engine) in the layout the
 * similarity kernels take a query in; q_f32_out_dev fp32 [batch, dim] (may be NULL) the same vector before the last
 * rounding -- what a split engine's calls take as their query; flags_out_dev int32 [batch].  Refusals as above. */
hrag_status hrag_reco_query(hrag_engine *e, const int32_t *ex_ptr, const int32_t *ex_ptr_dev, const int32_t *ex_idx_dev,
                            const int32_t *ex_sign_dev, int32_t batch, uint16_t *q_out_dev, float *q_f32_out_dev,
                            int32_t *flags_out_dev, hrag_stream stream);

/* Clears, in row b of words_dev uint32 [batch, ld_words] (one row per query, ld_words >= ceil(n / 32)), the bits of query
 * b's non-empty examples: ids in [0, n) whose sign is not 0 (ex_sign_dev NULL: every id in [0, n)).  One thread per query,
 * plain loads and stores: a row has one writer.  A repeated id is harmless, every other bit and word is left alone.  As in
 * hrag_reco_rows there is no host ex_ptr here, so the device-side ex_ptr is taken as it is (a negative start reads from 0,
 * a range is cut at HRAG_RECO_MAX_EXAMPLES): only the fused calls and hrag_reco_query clamp it to the host's total. */
hrag_status hrag_reco_exclude(uint32_t *words_dev, int64_t ld_words, int64_t n, const int32_t *ex_ptr_dev,
                              const int32_t *ex_idx_dev, const int32_t *ex_sign_dev, int32_t batch, hrag_stream stream);

/* ---- lexical retrieval: sparse-vector (BM25, learned term weights) scores blended into the dense scores ----
 * Every score above starts from the cosine of dense embeddings, which smears the rare surface forms a multi-hop question
 * turns on -- a name, a product code, a year.  An exact term match does not.  A LEXICAL INDEX holds, for each of n_terms
 * terms, the passages that contain it with a weight each (the posting list of the term); a sparse query is a list of
 * (term, weight) pairs.  The library knows nothing about BM25: it scores whatever weights it is given (negative ones
 * included: learned sparse models produce them).  For query b and passage p the score is the fp64 chain
 *
 *   acc = +0.0
 *   for j in q_ptr[b] .. q_ptr[b+1] - 1, in list order:
 *       if passage p is in the posting list of q_term[j]:
 *           acc += (double)q_weight[j] * (double)post_w[that entry]
 *
 * rounded once to fp32.  The product of two fp32 values is exact in fp64.  A passage that no query term lists scores
 * +0.0.  A term id outside [0, n_terms) contributes nothing.  A term repeated within a query contributes once per
 * occurrence, in list order.  At most HRAG_LEX_MAX_QUERY_TERMS terms of a query are read: a device-side q_ptr cannot be
 * checked on the host, so the terms of a longer list beyond the cap are IGNORED (a caller that must not lose terms checks
 * the lengths itself, as the Python binding does); whatever q_ptr holds, only q_term / q_weight [0, q_nnz) are read and
 * nothing outside the output rows is written.  A NaN or inf q_weight propagates by IEEE rules; a NaN result is the quiet
 * NaN 0x7fc00000, as in hrag_fuse_rows.  No atomics, no read-modify-write of global memory: every value is one chain in a
 * fixed order and every column is written exactly once, bitwise reproducible (csrc/lex.hip: one workgroup per query and
 * tile of HRAG_LEX_TILE consecutive passages, the tile's fp64 accumulators in LDS).
 *
 * THE BLEND of a dense row d and a lexical row l with a weight alpha in [0, 1], per row:
 *   alpha == 0, or the lexical row has no range (mx_l == mn_l, or it holds no number -- a query none of whose terms match
 *   is the common case): the output row is the dense row BIT FOR BIT;
 *   otherwise nd = (d - mn_d) / (mx_d - mn_d) and nl = (l - mn_l) / (mx_l - mn_l), one fp32 subtraction and one fp32
 *   division each, a zero range giving 1.0f (min_max_normalize, misc_utils.py:130-139: the min-max of every kernel here),
 *   and out = (float)((double)(1.0f - alpha) * (double)nd + (double)alpha * (double)nl): two exact products, one fp64
 *   add, one rounding; a NaN result is the quiet NaN.
 * The blended rows are raw passage scores for hrag_retrieve_scored* (or for a ranking), and hrag_retrieve_scored min-max
 * normalises its rows AGAIN when it forms the passage prior and the DPR fallback.  That composition -- minmax(blend of
 * the two min-maxes) -- IS the definition of the lexical prior; it is not an approximation of some other formula.
 * Everything hrag_retrieve_scored* serves (the doc filter in the "ranking" scope, grouping, group hits) and everything
 * behind it (hrag_last_fused, hrag_mmr) therefore composes with no further entry point.  Rank-level blending (RRF of the
 * dense and the lexical ranking) is not a separate mode: hrag_rrf_rows serves a caller who ranks both rows themself. */
#define HRAG_LEX_TILE 2048               /* passages per workgroup tile of hrag_lex_scores (tests pick their sizes by it) */
#define HRAG_LEX_MAX_QUERY_TERMS 256     /* terms of one query that hrag_lex_scores reads */

typedef struct hrag_lex hrag_lex; /* opaque; independent of any engine: engines and workspaces over the same passages share one */

/* The index from HOST arrays in inverted form: the posting list of term t is post_doc[term_ptr[t] : term_ptr[t + 1]]
 * (passage positions) with the weights post_w at the same places; term_ptr int64 [n_terms + 1].  Validated on the host,
 * then copied to the current device (the arrays may be freed right after).  HRAG_EINVAL, and nothing is allocated, unless
 * term_ptr[0] == 0 and term_ptr is non-decreasing, every passage position lies in [0, n_passages) and the positions of a
 * list are strictly ascending, and every weight is finite; 1 <= n_passages < 2^31, 0 <= n_terms < 2^31. */
hrag_status hrag_lex_create(int64_t n_passages, int64_t n_terms, const int64_t *term_ptr, const int32_t *post_doc,
                            const float *post_w, hrag_lex **out);
hrag_status hrag_lex_destroy(hrag_lex *lex);

/* The score rows of `batch` sparse queries in device CSR form -- q_ptr_dev int32 [batch + 1], q_term_dev int32 and
 * q_weight_dev fp32 [q_nnz] -- by the chain above: out_dev fp32 [batch, ld], ld >= n_passages, every one of the
 * n_passages columns written, the columns n_passages .. ld not touched.  min_out_dev / max_out_dev fp32 [batch] (both or
 * both NULL): the row min / max of the result exactly as hrag_row_minmax gives them (fminf / fmaxf, NaN skipped).
 * Enqueues on `stream`; nothing is allocated, synchronised or read back.  Any number of calls may read one index at the
 * same time. */
hrag_status hrag_lex_scores(const hrag_lex *lex, const int32_t *q_ptr_dev, const int32_t *q_term_dev,
                            const float *q_weight_dev, int64_t q_nnz, int32_t batch, float *out_dev, int64_t ld,
                            float *min_out_dev, float *max_out_dev, hrag_stream stream);

/* The blend above, engine-free: dense_dev fp32 [batch, ld_d] and lex_dev fp32 [batch, ld_l] with n valid columns, the
 * per-row mn_d / mx_d / mn_l / mx_l fp32 [batch] on the device (as hrag_row_minmax and hrag_lex_scores write them), out_dev
 * fp32 [batch, ld_o]; out_dev may BE dense_dev (then ld_o == ld_d).  The columns n .. ld_o are not touched.  Enqueues on
 * `stream`; nothing is allocated, synchronised or read back.  HRAG_EINVAL: alpha outside [0, 1] or not finite, a NULL
 * pointer, batch outside [1, 65535], a row stride below n. */
hrag_status hrag_lex_blend_rows(const float *dense_dev, int64_t ld_d, const float *lex_dev, int64_t ld_l, int32_t batch,
                                int64_t n, const float *mn_d_dev, const float *mx_d_dev, const float *mn_l_dev,
                                const float *mx_l_dev, float alpha, float *out_dev, int64_t ld_o, hrag_stream stream);

/* ---- payload filters: metadata conditions evaluated on the device into a doc filter ----
 * Every filtered entry point above takes the doc filter as a finished bitset.  A PAYLOAD INDEX holds typed per-passage
 * columns on the device, and hrag_payload_filter evaluates a small per-query clause program over them straight into the
 * packed words of that bitset (bit p & 31 of word p >> 5): its output is an ordinary doc filter, so everything that takes
 * one composes with no further entry point.
 *
 * A column is HRAG_PAY_I64 (int64: integers, bools, the dictionary codes of keyword strings) or HRAG_PAY_F64 (IEEE
 * doubles; NaN and +-inf are legal values), 8 bytes per passage, with an optional presence bitset in the doc filter's
 * format (NULL: every passage has a value).
 *
 * Query b owns the clauses f_ptr[b] .. f_ptr[b + 1] (int32).  Clause j names a column c_col[j], an operation
 * c_op[j] = role | kind << 8, two 8-byte bounds c_lo[j] / c_hi[j] and the slice c_set_ptr[j] .. c_set_ptr[j + 1] of
 * set_vals.  For passage p and the value x of the clause's column there:
 *   HRAG_PAY_RANGE    lo <= x && x <= hi in the column's type: signed int64 compares on an I64 column; double compares on
 *                     an F64 column, the bounds being the doubles' bit patterns.  A NaN value is in no range.
 *   HRAG_PAY_IN       x equals one of the slice's values.  The slice is sorted ascending in the column's order and matched
 *                     by binary search, with equality in the column's type: -0.0 matches 0.0, NaN matches nothing.
 *   HRAG_PAY_PRESENT  the passage has a value.
 *   hit(j, p) = present(column, p) && test.  A missing value hits nothing, so HRAG_PAY_MUST_NOT of it lets the passage
 *   through.
 *   allowed(b, p) = base(b, p) && every MUST clause hits && no MUST_NOT clause hits && (no SHOULD clause || some SHOULD
 *   clause hits).
 * base is and_words_dev: [batch, ld_a] words, or one row for the batch when ld_a == 0, or all ones when NULL.  A query
 * with no clauses gives its base row.  The bits at positions >= n_passages of the last word are 0; the words
 * ceil(n_passages / 32) .. ld_o of a row are not touched.  out_words_dev must not overlap and_words_dev.
 *
 * The clause arrays live on the device and cannot be checked on the host, so the definition covers bad input:
 *   - whatever f_ptr / c_set_ptr hold, only the clauses [0, n_clauses) and the values [0, set_nnz) are ever read: both
 *     ends of a range are clamped (a descending pair is empty), as hrag_lex_scores clamps q_ptr;
 *   - at most HRAG_PAY_MAX_CLAUSES clauses of a query are read, the rest are IGNORED (a caller that must not lose clauses
 *     checks the lengths itself, as the Python binding does);
 *   - a column id outside [0, n_cols), an unknown kind or role (or any bit above the two bytes of c_op), or lo > hi (a NaN
 *     bound included) makes a clause that hits nothing; a clause with an unknown role counts as a MUST, so its query allows
 *     nothing.
 * No atomics, no read-modify-write of global memory; every output word is written exactly once (csrc/payload.hip: one
 * workgroup per query and tile of HRAG_PAY_TILE consecutive passages, the verdicts packed by the 64-bit wave ballot).
 *
 * OUT OF SCOPE: term clauses over the lexical index ("the passage contains term t"; the kind byte leaves room for one),
 * multi-valued fields (tag lists), nested boolean groups, keyword ranges and prefix matches, evaluation inside the row-shard,
 * hybrid or captured forms (they take the finished words), and a doc filter that stays on the device through the mirror. */
#define HRAG_PAY_TILE 2048               /* passages per workgroup tile of hrag_payload_filter (tests pick their sizes by it) */
#define HRAG_PAY_MAX_CLAUSES 64          /* clauses of one query that hrag_payload_filter reads */
#define HRAG_PAY_MAX_COLS 256            /* columns of one payload index */
#define HRAG_PAY_I64 0                   /* column types */
#define HRAG_PAY_F64 1
#define HRAG_PAY_MUST 0                  /* clause roles: the low byte of c_op */
#define HRAG_PAY_MUST_NOT 1
#define HRAG_PAY_SHOULD 2
#define HRAG_PAY_RANGE 0                 /* clause kinds: the second byte of c_op */
#define HRAG_PAY_IN 1
#define HRAG_PAY_PRESENT 2

typedef struct hrag_payload hrag_payload; /* opaque; independent of any engine: engines and workspaces over the same passages share one */

/* The index from HOST arrays: col_type int32 [n_cols]; col_values[c] the 8-byte values [n_passages] of column c;
 * col_present[c] packed uint32 [ceil(n_passages / 32)], or NULL (as may be col_present itself) for "every passage has a
 * value".  Validated on the host, then copied to the current device (the arrays may be freed right after).  HRAG_EINVAL, and
 * nothing is allocated, unless 1 <= n_passages < 2^31, 0 <= n_cols <= HRAG_PAY_MAX_COLS, every type is known and every
 * value pointer is not NULL. */
hrag_status hrag_payload_create(int64_t n_passages, int32_t n_cols, const int32_t *col_type, const void *const *col_values,
                                const uint32_t *const *col_present, hrag_payload **out);
hrag_status hrag_payload_destroy(hrag_payload *pay);

/* The doc filter rows of `batch` clause programs by the definition above: f_ptr_dev int32 [batch + 1]; c_col_dev / c_op_dev
 * int32, c_lo_dev / c_hi_dev int64 [n_clauses]; c_set_ptr_dev int32 [n_clauses + 1]; set_vals_dev int64 [set_nnz] (the
 * clause arrays may be NULL when n_clauses == 0, set_vals_dev when set_nnz == 0); out_words_dev uint32 [batch, ld_o].
 * Enqueues on `stream`; nothing is allocated, synchronised or read back.  Any number of calls may read one index at the
 * same time.  HRAG_EINVAL: a NULL handle or output, batch outside [1, 65535], ld_o < ceil(n_passages / 32), ld_a neither 0
 * nor >= ceil(n_passages / 32), a negative count. */
hrag_status hrag_payload_filter(const hrag_payload *pay, const int32_t *f_ptr_dev, const int32_t *c_col_dev,
                                const int32_t *c_op_dev, const int64_t *c_lo_dev, const int64_t *c_hi_dev,
                                const int32_t *c_set_ptr_dev, const int64_t *set_vals_dev, int64_t n_clauses, int64_t set_nnz,
                                int32_t batch, const uint32_t *and_words_dev, int64_t ld_a, uint32_t *out_words_dev,
                                int64_t ld_o, hrag_stream stream);

/* How many passages a doc filter leaves: count_out_dev int32 [batch], the number of set bits among the first n of each row
 * of words_dev uint32 [batch, ld] (ld >= ceil(n / 32), or 0: one row, counted for every entry).  Engine-free and for ANY doc
 * filter -- the count call of the vector stores, what a caller needs to size k.  One workgroup per row, no atomics.
 * Enqueues on `stream`. */
hrag_status hrag_bitset_count_rows(const uint32_t *words_dev, int64_t ld, int64_t n, int32_t batch, int32_t *count_out_dev,
                                   hrag_stream stream);

/* ---- facets: per-value counts of a payload column, counted on the device ----
 * A payload condition restricts a retrieval and hrag_bitset_count_rows says how many passages it leaves.  A FACET says what
 * is in there: for one column of a payload index and a set of allowed passages -- the words of any doc filter, or a list
 * of passage ids as a retrieve call returns them -- how many of them fall into each bin of the column's values (Qdrant's
 * facet API, Elasticsearch's terms / range / histogram aggregations).
 *
 * A facet SPEC names the column and maps a present value x to a bin in [0, n_bins) or to "other":
 *   HRAG_FACET_CODES  (I64 columns only; a keyword column is this with lo = 0)
 *                     bin = x - lo when x >= lo && (uint64)(x - lo) < n_bins, else other.  Both conditions are needed:
 *                     x = INT64_MIN with lo = INT64_MAX wraps to 1 and is other.
 *   HRAG_FACET_EDGES  (I64 or F64 columns) edges_dev holds n_edges ascending bounds as 8-byte words of the column's type and
 *                     n_bins == n_edges + 1; bin = the number of edges <= x, found by binary search with comparisons in the
 *                     column's type, as HRAG_PAY_IN matches its set: bin 0 is x < edges[0], bin i is edges[i - 1] <= x <
 *                     edges[i], the last bin is x >= edges[n_edges - 1].  No arithmetic on values is involved, so nothing
 *                     rounds; -0.0 equals 0.0; a NaN value of an F64 column is other; equal neighbouring edges give an
 *                     empty bin; n_edges == 0 is legal and gives one bin.
 * For query b the output row counts_out_dev[b * ld_c ...] (int32, ld_c >= n_bins + 2) holds
 *   [v], v < n_bins   the allowed passages p < n_passages at which the column is present and whose value maps to bin v;
 *   [n_bins]          "other": allowed and present, the value maps to no bin;
 *   [n_bins + 1]      "missing": allowed, the column is not present;
 * so a row sums to the number of allowed passages -- exactly what hrag_bitset_count_rows gives for the same words.  The
 * entries [n_bins + 2, ld_c) of a row are never written.
 *
 * The edges live on the device and their order cannot be checked on the host: unsorted edges (or NaN edges) give
 * UNSPECIFIED bins but never an out-of-range write -- the search keeps 0 <= bin <= n_edges whatever the edges hold, and
 * every bin index is bounded by n_bins before it is used.
 *
 * Counts are integers and integer addition does not depend on its order, so the result is exact and the same on every
 * run although the kernels add with LDS atomics (csrc/facet.hip: one workgroup per query, window of HRAG_FACET_WINDOW bins
 * and split of the passage range; an int32 histogram of the window in LDS; the splits summed in split order by a second
 * kernel).  No global atomics, no memset; every output word is written exactly once.
 *
 * OUT OF SCOPE: score-weighted facets (the sum of scores per value is what group_agg = "sum" computes), facets of several
 * columns at once, multi-valued fields, facets inside the row-shard, hybrid or captured forms. */
#define HRAG_FACET_MAX_BINS (1 << 20)    /* n_bins of one spec */
#define HRAG_FACET_WINDOW 4096           /* bins one workgroup holds in LDS (tests pick their sizes by it) */
#define HRAG_FACET_CODES 0               /* spec kinds */
#define HRAG_FACET_EDGES 1

typedef struct hrag_facet_spec {
    int32_t column;             /* the column of the payload index */
    int32_t kind;               /* HRAG_FACET_CODES / HRAG_FACET_EDGES */
    int64_t n_bins;             /* 1 .. HRAG_FACET_MAX_BINS; EDGES: n_edges + 1 */
    int64_t lo;                 /* CODES: the value of bin 0 */
    const void *edges_dev;      /* EDGES: n_edges 8-byte words on the device (may be NULL when n_edges == 0) */
    int64_t n_edges;            /* EDGES: the number of bounds; CODES: ignored */
} hrag_facet_spec;

/* The bytes of workspace hrag_payload_facet needs for (the handle's n_passages, n_bins, batch): 0 when one workgroup per
 * (query, window) streams the whole passage range -- batch * ceil(n_bins / HRAG_FACET_WINDOW) >= 1024 workgroups fill the
 * machine on their own -- else 4 * batch * n_splits * (n_bins + 2) for the partial counts of n_splits equal runs of
 * HRAG_PAY_TILE-passage tiles, n_splits a pure function of the three numbers (about 1024 workgroups in all, at most one
 * split per tile).  A caller that wants n_splits reads it off this value. */
hrag_status hrag_payload_facet_ws_bytes(const hrag_payload *pay, int64_t n_bins, int32_t batch, int64_t *out);

/* The counts of `spec` under doc filter words: words_dev uint32 [batch, ld_w] (ld_w >= ceil(n_passages / 32)), one row for
 * the batch when ld_w == 0, every passage allowed when NULL.  Bits at or above n_passages in the last word are ignored and
 * words beyond ceil(n_passages / 32) are never read.  ws_dev: ws_bytes >= hrag_payload_facet_ws_bytes of workspace (may be
 * NULL when that is 0); its contents before and after the call mean nothing.  Enqueues on `stream`; nothing is allocated,
 * synchronised or read back.  HRAG_EINVAL: a NULL handle, spec or output; a column outside the index; an unknown kind;
 * CODES on an F64 column; n_bins outside [1, HRAG_FACET_MAX_BINS]; EDGES with n_bins != n_edges + 1 or NULL edges; ld_c <
 * n_bins + 2; ld_w neither 0 nor >= ceil(n_passages / 32); rows that are not 4-byte (edges: 8-byte) aligned; batch outside
 * [1, 65535]; ws_bytes below what the query call returns. */
hrag_status hrag_payload_facet(const hrag_payload *pay, const hrag_facet_spec *spec, const uint32_t *words_dev, int64_t ld_w,
                               int32_t batch, int32_t *counts_out_dev, int64_t ld_c, void *ws_dev, int64_t ws_bytes,
                               hrag_stream stream);

/* The same counts over lists of passage ids: idx_dev int32 [batch, ld_i], the first k of a row read (ld_i >= k >= 1), as
 * the retrieve calls return them.  An id outside [0, n_passages) -- the -1 padding included -- is skipped and counted
 * nowhere; a repeated id counts each time.  One workgroup per (query, window): the ids read coalesced, the column gathered
 * at each id.  No workspace. */
hrag_status hrag_payload_facet_ids(const hrag_payload *pay, const hrag_facet_spec *spec, const int32_t *idx_dev, int64_t ld_i,
                                   int32_t k, int32_t batch, int32_t *counts_out_dev, int64_t ld_c, hrag_stream stream);

/* ---- boosted retrieval: payload-driven score boosts and decay functions on the device ----
 * A payload condition above can only EXCLUDE a passage.  A boost PROGRAM prefers instead: it rewrites score rows in place
 * as s * M + A, M and A built per passage from a small per-query list of TERMS over the columns of a payload index -- a
 * constant under a condition (trust these sources 1.5x, halve the drafts), a column value (a little score per citation),
 * a decay function of a column (prefer the last 90 days without hiding older material).
 *
 * Query b owns the terms t_ptr[b] .. t_ptr[b + 1] (int32); with broadcast != 0 every query owns t_ptr[0] .. t_ptr[1], as
 * ld_a = 0 gives one row of filter words to a batch.  At most HRAG_BOOST_MAX_TERMS terms of a query are read.  Term j holds
 *   t_op[j]       kind | mode << 8 | sub << 16 | has_missing << 24: kind HRAG_BOOST_CONST / _FIELD / _DECAY, mode
 *                 HRAG_BOOST_MUL / _ADD, sub the modifier of a FIELD (HRAG_BOOST_NONE / _SQRT) or the shape of a DECAY
 *                 (HRAG_BOOST_LINEAR / _EXP / _GAUSS), 0 for a CONST;
 *   t_col[j]      the column of a FIELD or DECAY (a CONST ignores it);
 *   t_num[5 j ..] five doubles: the weight w; three parameters -- a DECAY's origin, offset and c, unused otherwise --; the
 *                 value `missing` (read when has_missing);
 *   t_cl_ptr[j] .. t_cl_ptr[j + 1]   its CONDITION: a slice of clauses in the payload-filter encoding above (column,
 *                 op = role | kind << 8, lo, hi, set slice; RANGE / IN / PRESENT x MUST / MUST_NOT / SHOULD, the same rule,
 *                 without base words), evaluated by the device code of hrag_payload_filter itself.  An empty slice is true.
 *                 All terms of one query together use at most HRAG_PAY_MAX_CLAUSES clauses: they fill that cap in term
 *                 order, a term keeping the first clauses of its slice that still fit (the slice of an ill-formed term
 *                 counts like any other).
 *
 * For passage p with the row entry s (fp32) start with M = 1.0, A = 0.0 (fp64).  For each term in list order:
 *   1. hit = the term's condition at p.
 *   2. the value v: CONST 1.0.  FIELD: x, the column value as a double (an I64 value converted round-to-nearest-even);
 *      v = x (NONE) or the IEEE sqrt(x) (SQRT; NaN below 0).  DECAY: d = pos(fabs(x - origin) - offset), then
 *      LINEAR v = pos((c - d) / c), EXP v = exp_dec(c * d), GAUSS v = exp_dec(c * (d * d)); pos(y) = y > 0 ? y : +0.0 is
 *      fmax(0, y).  The HOST computes c once in fp64 from the usual scale and decay: scale / (1 - decay) for LINEAR,
 *      ln(decay) / scale for EXP, ln(decay) / scale^2 for GAUSS.  A value that is absent, or NaN on an F64 column, is
 *      MISSING for FIELD and DECAY: v = missing when the term carries one (as it is: no modifier, no decay), else
 *      hit = false.
 *   3. if hit: t = w * v, then M = M * t (MUL) or A = A + t (ADD).
 * Every product, quotient, difference and sum is rounded on its own in fp64; no fused multiply-add anywhere.
 *   out = (float)(((double)s * M) + A): two fp64 roundings and one to fp32, a NaN stored as the quiet NaN 0x7fc00000 (as
 *   hrag_lex_scores stores one).
 * The row of a query with NO terms is not touched: it stays bit for bit, -0.0 and NaN payloads included (a query whose
 * terms hit nothing is rewritten with M = 1, A = 0).  The columns n_passages .. ld of a row are never touched.  No atomics;
 * every element is read and written by one thread, which is why the operation is in place.
 *
 * With mn_dev / mx_dev (fp32 [batch], hrag_row_minmax of the rows) the kernel reads the min-max of the entry instead of s:
 * mx - mn == 0 ? 1 : (s - mn) / (mx - mn) in fp32, the library's rule (hrag_lex_blend_rows) -- what a dense ranking needs.
 *
 * exp_dec(x), x <= 0, is the library's own exponential, so that the definition is a sequence of rounded fp64 operations
 * a host can restate bit for bit: NaN gives NaN; x > 0 is taken as 0; x < -708 gives 0.0; else k = rint(x * LOG2E),
 * r = (x - k * LN2_HI) - k * LN2_LO with LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42fee00000p-1,
 * LN2_LO = 0x1.a39ef35793c76p-33; p by Horner from c13 down to c0, c_i = fp64(1 / i!), each step p = p * r + c_i as two
 * rounded operations; the result is ldexp(p, k).  Within 2 ulp of exp on [-708, 0], values in [0, 1], exp_dec(0) == 1.
 *
 * The program arrays live on the device and cannot be checked on the host, so the definition covers bad input, as the
 * payload filter's does: both ends of t_ptr / t_cl_ptr / c_set_ptr ranges are clamped to the arrays (a descending pair is
 * empty); terms and clauses beyond the caps are IGNORED (the Python binding raises instead); an ill-formed clause hits
 * nothing; an ill-formed TERM -- a column outside [0, n_cols) on a FIELD or DECAY, an unknown kind, mode or sub, a bit
 * above bit 24 of t_op -- is NEUTRAL: the score goes unboosted by it, never dropped.
 *
 * OUT OF SCOPE: logarithmic modifiers (no libm-free log here yet), geo distance, boosts applied to the passage prior
 * BEFORE the PPR, evaluation inside the retrieve call itself (hrag_last_boosted re-ranks the rows a call left: that
 * call's own ranking is computed and discarded), the row-shard, hybrid and captured forms. */
#define HRAG_BOOST_MAX_TERMS 32          /* terms of one query that hrag_boost_rows reads */
#define HRAG_BOOST_CONST 0               /* term kinds: the low byte of t_op */
#define HRAG_BOOST_FIELD 1
#define HRAG_BOOST_DECAY 2
#define HRAG_BOOST_MUL 0                 /* term modes: the second byte */
#define HRAG_BOOST_ADD 1
#define HRAG_BOOST_NONE 0                /* FIELD modifiers: the third byte */
#define HRAG_BOOST_SQRT 1
#define HRAG_BOOST_LINEAR 0              /* DECAY shapes: the third byte */
#define HRAG_BOOST_EXP 1
#define HRAG_BOOST_GAUSS 2
#define HRAG_BOOST_HAS_MISSING (1 << 24) /* the term carries a `missing` value */

/* The program arrays, all on the device: t_ptr int32 [batch + 1] ([2] when broadcast); t_op / t_col int32 [n_terms];
 * t_num fp64 [n_terms][5]; t_cl_ptr int32 [n_terms + 1]; the clause arrays as hrag_payload_filter takes them (c_set_ptr
 * int32 [n_clauses + 1]).  The term arrays may be NULL when n_terms == 0, the clause arrays when n_clauses == 0, set_vals
 * when set_nnz == 0.  The struct itself is read on the host, at the call. */
typedef struct hrag_boost_program {
    const int32_t *t_ptr;
    const int32_t *t_op;
    const int32_t *t_col;
    const double *t_num;
    const int32_t *t_cl_ptr;
    const int32_t *c_col;
    const int32_t *c_op;
    const int64_t *c_lo;
    const int64_t *c_hi;
    const int32_t *c_set_ptr;
    const int64_t *set_vals;
    int64_t n_terms, n_clauses, set_nnz;
} hrag_boost_program;

/* rows_dev fp32 [batch, ld] boosted in place by the definition above, n = the passages of `pay`.  Engine-free; enqueues on
 * `stream`; nothing is allocated, synchronised or read back; a program with n_terms == 0 launches nothing.  HRAG_EINVAL: a
 * NULL handle, rows or program, batch outside [1, 65535], ld < n_passages, rows not 4-byte aligned, only one of mn_dev /
 * mx_dev, a negative count, a NULL array with a positive count. */
hrag_status hrag_boost_rows(const hrag_payload *pay, float *rows_dev, int64_t ld, int32_t batch, const float *mn_dev,
                            const float *mx_dev, const hrag_boost_program *program, int32_t broadcast, hrag_stream stream);

/* The boosted ranking over the score rows the last call left on this handle (as hrag_last_group_hits and hrag_last_fused
 * read them: a retrieve, a scored or a grouped dense call, or a fusion): the first `batch` rows, one per query, are boosted
 * IN PLACE by `program` (no mn / mx: the rows are final scores) and then ranked as that call would have ranked them -- the
 * k best under the doc filter into doc_idx_out / doc_score_out (both or neither), or with group_agg >= 0 the grouped
 * ranking into the three group outputs (hrag_retrieve_grouped's; group_agg -1: ungrouped).  Afterwards
 * hrag_last_group_hits, hrag_last_doc_scores and hrag_last_fused read the boosted rows (a fusion then fuses boosted member
 * rows; hrag_last_boosted after hrag_last_fused boosts the fused rows instead).  Calling it twice boosts twice.
 * HRAG_EINVAL: a row-shard engine, a payload index over another number of passages, no score rows on the handle, batch
 * above the queries of the call that wrote them, k outside [1, max_topk], and what hrag_boost_rows rejects. */
hrag_status hrag_last_boosted(hrag_engine *e, const hrag_payload *pay, int32_t batch, const hrag_boost_program *program,
                              int32_t broadcast, int32_t k, const uint32_t *filter_dev, int64_t filter_ld_words,
                              int32_t group_agg, int32_t *doc_idx_out, float *doc_score_out, int32_t *group_idx_out,
                              float *group_score_out, int32_t *best_doc_idx_out, hrag_stream stream);

/* ---- lower-level seams (used by the per-method adapters and by the parity tests) ---- */

/* np.dot(embeddings, q.T) (HippoRAG.py:1459 / :1496): raw cosine scores.
 * which: 0 = facts, 1 = passages.  out_dev fp32 [B, rows] (row stride = rows). */
hrag_status hrag_sim_scores(hrag_engine *e, int32_t which, const uint16_t *q_dev, int32_t batch,
                            float *out_dev, hrag_stream stream);

/* run_ppr's numerical core (HippoRAG.py:1735-1743) for B reset vectors:
 *   reset_dev fp32 [B, V] (NaN / negative entries are zeroed like :1735)
 *   x_out_dev fp32 [B, V] PPR probabilities (each row sums to 1)
 *   flags_out_dev int32 [B] bit1 set when a row had no positive mass (may be NULL). */
hrag_status hrag_ppr(hrag_engine *e, const float *reset_dev, int32_t batch, float damping,
                     int32_t iters, float *x_out_dev, int32_t *flags_out_dev, hrag_stream stream);

/* Generic row-wise top-k with the library's ranking rule (np.argsort(...)[::-1][:k]) fused with
 * the row min / max.  scores_dev fp32 [B, ld] (n valid entries per row), 1 <= k <= 2048 (any k: hrag_topk_rows_ws).
 *   idx_out_dev int32 [B, k] = position + idx_offset (-1 beyond min(k, n))
 *   val_out_dev fp32 [B, k]  raw score, or (s - min) / (max - min) when normalize != 0
 *   min_out_dev / max_out_dev fp32 [B] (may be NULL).  No engine needed. */
hrag_status hrag_topk_rows(const float *scores_dev, int32_t batch, int64_t n, int64_t ld, int32_t k,
                           int32_t idx_offset, int32_t normalize, int32_t *idx_out_dev,
                           float *val_out_dev, float *min_out_dev, float *max_out_dev,
                           hrag_stream stream);
/* The same for ANY k >= 1 (the full ranking of a row included), same output: np.argsort(x, kind="stable")[::-1][:k]
 * exactly, so its first 2048 entries are hrag_topk_rows' at k = 2048 bit for bit.  k <= 2048 IS hrag_topk_rows (the
 * workspace is not touched).  Beyond, K4': the exact min(k, n)-th key by radix histograms, the keys above it compacted,
 * sorted in LDS (<= 16384 per row) or tile-sorted and merged in the workspace.  workspace_dev: 8-byte aligned,
 * hrag_topk_rows_workspace_bytes(batch, n, k) bytes (0 -- workspace_dev may be NULL -- when k <= 2048 or
 * min(k, n) <= 16384; else 16 * batch * round_up(min(k, n), 16384) + 256), used as scratch only: no allocation, host
 * synchronisation or read-back inside the call (hipGraph capture safe).  batch <= 65535 when the workspace is used. */
int64_t hrag_topk_rows_workspace_bytes(int32_t batch, int64_t n, int32_t k);
hrag_status hrag_topk_rows_ws(const float *scores_dev, int32_t batch, int64_t n, int64_t ld, int32_t k,
                              int32_t idx_offset, int32_t normalize, int32_t *idx_out_dev, float *val_out_dev,
                              float *min_out_dev, float *max_out_dev, void *workspace_dev, size_t workspace_bytes,
                              hrag_stream stream);
/* hrag_topk_rows_ws over the elements a mask allows (the doc filter's format above; mask_dev must not be NULL): row r
 * may select element i when bit (mask_bit_offset + i) of the words at mask_dev + r * mask_ld_words is set
 * (mask_ld_words 0: one row for the batch, else >= ceil((mask_bit_offset + n) / 32)).  Per row: the first min(k,
 * allowed) entries of hrag_topk_rows_ws's full ranking that are allowed, bit for bit, then -1 / 0.  min_out / max_out
 * and normalize still use EVERY element of the row.  Any k, the workspace rule of hrag_topk_rows_ws; at k <= 2048 a
 * workspace of at least 2 MiB is optional and lets a batch below 64 split long rows over several workgroups (the
 * engine's ranking does; same result). */
hrag_status hrag_topk_rows_masked(const float *scores_dev, int32_t batch, int64_t n, int64_t ld, int32_t k,
                                  int32_t idx_offset, int32_t normalize, const uint32_t *mask_dev, int64_t mask_ld_words,
                                  int64_t mask_bit_offset, int32_t *idx_out_dev, float *val_out_dev, float *min_out_dev,
                                  float *max_out_dev, void *workspace_dev, size_t workspace_bytes, hrag_stream stream);

/* ---- index-time entity KNN (retrieve_knn, utils/embed_utils.py:6-94; engine-less) ----
 * hrag_normalize_split_bf16: F.normalize (embed_utils.py:25,28) when normalize != 0, then the split
 *   x = hi + lo into two bf16 matrices (lo_dev may be NULL: plain bf16 rounding).
 * hrag_sim_gemm: out[b][m] (+)= sum_k q[b][k] * emb[m][k]  (torch.mm, :53); bf16 / fp16 in (dtype), fp32 out,
 *   row stride ld; accumulate != 0 adds to out.  retrieve_knn (hipporag_amd/knn.py) runs it ONCE per query block on
 *   the split layout of hrag_split_f32 (normalize != 0: F.normalize first): [hi | lo | hi] x [qhi | qhi | qlo],
 *   fp16 halves, on the wide-batch 256-row kernel: the accuracy of HRAG_F32_SPLIT above (unit vectors after
 *   normalisation: layout ~3 * 2^-22 + the fp32 accumulation).
 * The top-k of each score row is hrag_topk_rows (k <= 2048 covers synonymy_edge_topk = 2047), hrag_topk_rows_ws
 * beyond (retrieve_knn accepts any k). */
hrag_status hrag_normalize_split_bf16(const float *x_dev, int64_t rows, int32_t dim, int32_t normalize,
                                      uint16_t *hi_dev, uint16_t *lo_dev, hrag_stream stream);
hrag_status hrag_sim_gemm(const uint16_t *emb_dev, int64_t rows, int32_t dim, const uint16_t *q_dev,
                          int32_t batch, float *out_dev, int64_t ld, int32_t accumulate, int32_t dtype,
                          hrag_stream stream);
/* The k <= 16 best rows per query WITHOUT the score matrix (the engine-less form of hrag_score_facts' fused path: the
 * GEMM epilogue keeps every 128-row tile's maximum, the k tiles with the largest maxima are rescored with the same MFMA
 * chain -- exact, bit-identical to hrag_sim_gemm + hrag_topk_rows): idx int32 [B, k], raw scores fp32 [B, k].
 * When a query's 16th best score is below the synonymy threshold, its neighbours above the threshold are all among these
 * 16 and no [B, rows] block is ever written (retrieve_knn(min_score=...) ran on this call until ABI 0.8 and runs on the
 * thresholded form below since) (embed_utils.py:53-73 materialises
 * it block by block).  workspace_dev: hrag_sim_topk_workspace_bytes(rows, batch) bytes, ZEROED ONCE by the caller
 * before the first call (the call leaves it reusable). */
int64_t hrag_sim_topk_workspace_bytes(int64_t rows, int32_t batch);
hrag_status hrag_sim_topk(const uint16_t *emb_dev, int64_t rows, int32_t dim, const uint16_t *q_dev, int32_t batch,
                          int32_t k, int32_t dtype, void *workspace_dev, int64_t workspace_bytes,
                          int32_t *idx_out_dev, float *val_out_dev, hrag_stream stream);
/* The THRESHOLDED form (ABI 0.8; add_synonymy_edges reads neighbours down to synonymy_edge_sim_threshold only,
 * HippoRAG.py:1004-1007): the caller trusts results at or above min_score and nothing below it.
 *   - tiles whose maximum is below min_score - margin are never rescored;
 *   - approx_dim > 0: pass 1 (the tile maxima) runs over the first approx_dim elements of every row and query only; the
 *     caller states in `margin` a bound on |full product - prefix product|.  For the split layout of hrag_split_f32 with
 *     approx_dim = dim / 3 the prefix is hi . qhi and the rest, lo . qhi + hi . qlo, is at most 2 * 2^-11 |x| |q| = 9.8e-4
 *     for unit vectors (+ the fp16 subnormal floor 2^-25 (|x|_1 + |q|_1), 3.8e-6 at dim 4096): margin 1.2e-3, a third of the MFMA work.  approx_dim = 0: pass 1 over all of dim (margin may be 0);
 *   - pass 3 rescores the tiles that reach the cut over all `dim` elements: every returned score is the exact chain of
 *     hrag_sim_gemm, and every row with score >= min_score is returned (in score order, ahead of anything below
 *     min_score) UNLESS overflow_out_dev[b] != 0 (more than k tiles reached the cut) or the k-th returned score is itself
 *     >= min_score: for those queries the caller takes hrag_sim_gemm + hrag_topk_rows.  Entries below min_score are
 *     NOT the global ranking (rows of unselected tiles are missing among them).
 * k <= 16; workspace as hrag_sim_topk; overflow_out_dev int32 [B]. */
hrag_status hrag_sim_topk_min_score(const uint16_t *emb_dev, int64_t rows, int32_t dim, const uint16_t *q_dev, int32_t batch,
                                    int32_t k, int32_t dtype, int32_t approx_dim, float min_score, float margin,
                                    void *workspace_dev, int64_t workspace_bytes, int32_t *idx_out_dev,
                                    float *val_out_dev, int32_t *overflow_out_dev, hrag_stream stream);
/* fp32 [rows, dim] -> the fp16 [rows, 3 * dim] layout of an HRAG_F32_SPLIT engine: [hi | lo | hi] for embedding rows,
 * [hi | hi | lo] with as_query != 0 (new rows for hrag_engine_gather_embeddings; the engine converts its own inputs);
 * normalize != 0: rows are L2-normalised first (x / max(||x||, 1e-12), the KNN's F.normalize). */
hrag_status hrag_split_f32(const float *x_dev, int64_t rows, int32_t dim, int32_t as_query, int32_t normalize,
                           uint16_t *out_dev, hrag_stream stream);

/* Measurement hook: run `n` PPR SpMM sweeps over the engine's current state buffers for
 * `batch` right-hand sides (state is whatever the last hrag_retrieve / hrag_ppr left).
 * flags bit0: fp32 CSR path: main kernel only (skip its long-row and seed kernels); no effect on the SELL-8 kernels
 *             (bits 1-3), which finish long rows inside the sweep kernel;
 * flags bit1: the fp16-state kernel of the two-stage scheme (mode H) instead of the fp32 one
 *             (HRAG_EINVAL when the engine has no fp16 state: sharded, max_batch <= 8, F32_STATE);
 * flags bit2: the small-batch kernel (batch <= 8, state fp32 [V][1|2|4|8]);
 * flags bit3: the fp8-state kernel over the buffers of the last hrag_retrieve (HRAG_EINVAL without col_sum /
 *             max_batch <= 64 / batch <= 64 / no preceding hrag_retrieve); bits 4-5 pick the instantiation
 *             (0 stage sweep C, 1 boundary B, 2 final F, 3 first boundary B0), bits 6-7 the residual form of
 *             B / F (0 fp32, 2 fp32 in / 3-byte out, 3 3-byte in / out; F: 1 = 3-byte in);
 *             with bit 3, bit 8 (256) = GATHER REPLAY: the state-row gathers of a stage sweep and nothing else
 *             (same matrix, same state, same launch geometry; nothing is written) -- the floor of any sweep that
 *             fetches one state row per matrix slot (bench.py roofline.gather_replay_ms). */
hrag_status hrag_ppr_sweeps(hrag_engine *e, int32_t batch, int32_t n, float damping, int32_t flags,
                            hrag_stream stream);

/* ------------------------------------------------------------------------------------------
 * Stage-level operators.  hrag_retrieve() on the fp32 state (HRAG_OPT_F32_STATE, or any sweep count /
 * damping the narrower states do not take) is exactly the composition of these on engine-owned
 * buffers -- bit for bit: tests/test_gpu_stage_ops.py composes them by hand and on row windows that
 * share one state, tests/test_gpu_csr_sweep.py holds each of them to fp64 at every slab width.  They are
 * the seams for per-method adapters and those tests: fp32 state, every buffer caller-owned device memory,
 * a host may interleave its own steps between any two of them.  (The multi-GPU row-shard mode of
 * hipporag_amd/dist.py exchanged x between hrag_stage_ppr_step calls once; it runs on the hrag_shard_*
 * calls below, on the staged e4m3 state, and shares only hrag_stage_seeds with this list.)
 *
 * PPR state layout ("slab layout"): x is [n_slabs][V][bc] fp32; query q lives in slab q / bc,
 * column q % bc; hrag_ppr_layout() returns (bc, n_slabs) for a batch on this engine.
 * seed arrays: seed_vtx int32 [B][HRAG_SEED_STRIDE], seed_w fp32 [B][HRAG_SEED_STRIDE], seed_cnt int32 [B].
 * ------------------------------------------------------------------------------------------ */
#define HRAG_SEED_STRIDE 32

hrag_status hrag_ppr_layout(hrag_engine *e, int32_t batch, int32_t *slab_width_out,
                            int32_t *n_slabs_out);

/* min / max of every row (what min_max_normalize reduces, misc_utils.py:131-132). */
hrag_status hrag_row_minmax(const float *scores_dev, int32_t batch, int64_t n, int64_t ld,
                            float *min_out_dev, float *max_out_dev, hrag_stream stream);

/* seeds == HippoRAG.py:1574-1623 + :1505-1542 on fact ids (needs the engine's fact_desc).
 * flags_dev int32 [B] is read-modify-written (bits 0 and 2).  The reset-vector rule of hrag_retrieve (above) applies:
 * seeds ranked with NaN means first, seed_w sanitised; slots [seed_cnt, HRAG_SEED_STRIDE) are not written. */
hrag_status hrag_stage_seeds(hrag_engine *e, const int32_t *kept_idx_dev, const float *kept_score_dev,
                             const int32_t *kept_count_dev, int32_t kf, int32_t link_top_k,
                             int32_t batch, int32_t *seed_vtx_dev, float *seed_w_dev,
                             int32_t *seed_cnt_dev, int32_t *flags_dev, hrag_stream stream);

/* passage prior == HippoRAG.py:1626-1635: tele[slab][p][c] = minmax(S[q][p]) * passage_node_weight, sanitised
 * (the reset-vector rule above hrag_retrieve), for ALL Np passages (scores_dev fp32 [B, ld] raw cosine scores in passage order, min/max per
 * row); rows of queries whose flags bit0 is set (DPR fallback) are zero.
 * tele_out_dev: [n_slabs][Np][bc]. */
hrag_status hrag_stage_teleport(hrag_engine *e, const float *scores_dev, int64_t ld,
                                const float *min_dev, const float *max_dev, float passage_node_weight,
                                const int32_t *flags_dev, int32_t batch, float *tele_out_dev,
                                hrag_stream stream);

/* x0 = v on the rows this engine owns (rows [row_offset, row_offset + n_rows) of every slab). */
hrag_status hrag_stage_ppr_init(hrag_engine *e, const float *tele_dev, const int32_t *seed_vtx_dev,
                                const float *seed_w_dev, const int32_t *seed_cnt_dev, int32_t batch,
                                float *x_dev, hrag_stream stream);

/* one sweep y = damping * P x + (1 - damping) * v on the owned rows (reads all of x). */
hrag_status hrag_stage_ppr_step(hrag_engine *e, const float *tele_dev, const int32_t *seed_vtx_dev,
                                const float *seed_w_dev, const int32_t *seed_cnt_dev, int32_t batch,
                                float damping, const float *x_dev, float *y_dev, hrag_stream stream);

/* per-query sum of x over the owned rows -> sums_out_dev double [B] (all-reduce it across shards).
 * workspace_dev: hrag_colsum_workspace_bytes(e, batch) bytes. */
hrag_status hrag_stage_colsum(hrag_engine *e, const float *x_dev, int32_t batch, void *workspace_dev,
                              double *sums_out_dev, hrag_stream stream);
int64_t hrag_colsum_workspace_bytes(hrag_engine *e, int32_t batch);

/* doc_scores == pagerank_scores[passage_node_idxs] / sum (HippoRAG.py:1745) for ALL Np passages
 * from a complete x; queries with flags bit0 get minmax(scores_dev) (DPR fallback, :467-469);
 * sets flags bit1 where sums <= 0 on a non-fallback query.  out_dev fp32 [B, out_ld]. */
hrag_status hrag_stage_doc_scores(hrag_engine *e, const float *x_dev, const double *sums_dev,
                                  int32_t batch, const float *scores_dev, int64_t ld,
                                  const float *min_dev, const float *max_dev, int32_t *flags_dev,
                                  float *out_dev, int64_t out_ld, hrag_stream stream);

/* ------------------------------------------------------------------------------------------
 * Row-sharded hot path (multi-GPU): one engine per GPU, each created with the row shard
 * [row_offset, row_offset + n_rows) of the graph, the passage embeddings of the passages whose
 * vertex lies in that range (hrag_embed_desc.row_offset / rows must describe exactly those: the
 * passage prior then never crosses GPUs) and any contiguous slice of the fact embeddings.
 * The reference has no analogue (HippoRAG.py:459 is a serial loop over queries); this is the layout
 * BASELINE.json's north star names.  The PPR iterate is the staged e4m3 state of csrc/ppr8.hip,
 * replicated; after every sweep the host exchanges the owners' row blocks (1 byte per vertex and
 * query on the wire) -- hipporag_amd/dist.py does it with one RCCL all-gather per exchange group.
 * Needs hrag_graph_desc.col_sum; damping^ppr_iters <= 2^-20, 16 <= ppr_iters <= 30.
 *
 * State buffers (caller-owned, three of them, zero-initialised once): e4m3
 *   [n_groups][num_vertices + 1][slabs_per_group][128]; query q lives in slab q / 128; slab s in
 *   group s / slabs_per_group.  Row num_vertices of every group stays zero.  The owned rows of one
 *   group are ONE contiguous block (own_offset, own_bytes inside the group): with equal-sized shards
 *   in rank order (own_offset == rank * own_bytes) an in-place all-gather over the first
 *   world * own_bytes bytes of the group completes the buffer.
 *
 * Per batch:  hrag_shard_score_facts -> gather + merge candidates, min / max all-reduce
 *             hrag_shard_passage_scores -> all-reduce MIN / MAX of mn / mx
 *             hrag_stage_seeds (replicated)
 *             hrag_shard_prior_stats -> all-reduce MAX of zmax, SUM of mass
 *             hrag_shard_ppr_begin -> exchange every group of state[0]
 *             n_steps x n_groups x hrag_shard_ppr_sweep -> exchange group g of state[*exchange_out]
 *                 (n_steps = ppr_iters without a tolerance; measuring steps: est all-reduce + hrag_shard_ppr_decide)
 *             hrag_shard_finish -> gather + merge the local top-k lists
 * Per batch, "seeds" scope (the scoped doc filter above; every shard passes the same GLOBAL filter):
 *             hrag_shard_score_facts_scoped -> gather + merge candidates, min / max all-reduce (as unscoped)
 *             hrag_shard_passage_scores_scoped -> all-reduce MIN / MAX of the allowed min / max
 *             hrag_shard_mask_prior(those) -> all-reduce MIN / MAX of its min / max; then everything from
 *                 hrag_stage_seeds on as above, with these min / max and hrag_shard_finish_filtered
 * ------------------------------------------------------------------------------------------ */
#define HRAG_FLAG_FP8_SATURATED 8

typedef struct hrag_shard_layout {
    int32_t n_slabs;         /* 128-query slabs of the batch                                   */
    int32_t n_groups;        /* exchange groups                                                */
    int32_t slabs_per_group;
    int32_t reserved;
    int64_t state_bytes;     /* size of ONE state buffer = n_groups * group_bytes               */
    int64_t group_bytes;     /* (num_vertices + 1) * slabs_per_group * 128                      */
    int64_t own_offset;      /* byte offset of the owned rows inside a group                    */
    int64_t own_bytes;       /* n_rows * slabs_per_group * 128                                  */
} hrag_shard_layout;

/* want_groups: 0 = the narrowest groups; otherwise the number of exchange groups asked for.  The engine may
 * return a different number: a group is limited to 4 GiB and 2^24 vertices, and its width is kept EVEN
 * (the sweep kernels gather the two adjacent slabs of a vertex together), so the narrowest group holds two slabs. */
hrag_status hrag_shard_layout_query(hrag_engine *e, int32_t batch, int32_t want_groups,
                                    hrag_shard_layout *out);

/* local phase A: the k best facts of the owned fact rows per query, RAW cosine scores (global fact
 * ids, -1 beyond the shard's size) + the local min / max of every score row. */
hrag_status hrag_shard_score_facts(hrag_engine *e, const uint16_t *q_fact_dev, int32_t batch, int32_t k,
                                   int32_t *idx_out_dev, float *score_out_dev, float *min_out_dev,
                                   float *max_out_dev, hrag_stream stream);

/* cosine scores of the owned passages (kept inside the engine) + their local min / max fp32 [B]. */
hrag_status hrag_shard_passage_scores(hrag_engine *e, const uint16_t *q_pass_dev, int32_t batch,
                                      float *min_out_dev, float *max_out_dev, hrag_stream stream);

/* given the GLOBAL min / max: zmax_out_dev fp32 [B] (max over the owned passages of the normalised
 * score / weighted degree) and mass_out_dev double [2 * B] (prior mass, prior mass on isolated
 * passages) -- all-reduce MAX / SUM them.  flags_dev: bit0 queries carry no prior. */
hrag_status hrag_shard_prior_stats(hrag_engine *e, const float *min_dev, const float *max_dev,
                                   float passage_node_weight, const int32_t *flags_dev, int32_t batch,
                                   float *zmax_out_dev, double *mass_out_dev, hrag_stream stream);

/* reset vector on the owned rows + c_0 into the owned rows of state[0] (all groups). */
hrag_status hrag_shard_ppr_begin(hrag_engine *e, const float *min_dev, const float *max_dev,
                                 const float *zmax_dev, const double *mass_dev, float passage_node_weight,
                                 const int32_t *seed_vtx_dev, const float *seed_w_dev,
                                 const int32_t *seed_cnt_dev, int32_t *flags_dev, int32_t batch,
                                 float damping, int32_t ppr_iters, int32_t ppr_max_iters, float ppr_tol,
                                 int32_t n_groups, void *state0_dev, void *state1_dev, void *state2_dev,
                                 int32_t *n_steps_out, hrag_stream stream);

/* sweep `sweep` (0 .. ppr_iters - 1, in order per group) on the owned rows of exchange group `group`;
 * *exchange_out = index of the state buffer whose owned block of that group was written and must be
 * exchanged before the group's next sweep (-1 after the last sweep: nothing to exchange).
 * Issue the groups of one sweep in ASCENDING order (0 .. n_groups - 1) before any group of the next sweep: on an
 * engine that owns every row and measures its stage scales (damping < 0.46, HRAG_OPT_ACCEL) the boundary sweeps fold
 * each group's maximum into one running value and the launch of the last group turns it into the next scale. */
hrag_status hrag_shard_ppr_sweep(hrag_engine *e, int32_t sweep, int32_t group, int32_t *exchange_out,
                                 int32_t *checkpoint_out, hrag_stream stream);

/* The convergence contract of hrag_retrieve on row shards (ppr_tol > 0 in hrag_shard_ppr_begin; *n_steps_out then
 * counts the conditional steps too: run ALL of them, the gate words decide on the device which ones do anything --
 * and every shard decides alike because the measure is all-reduced):
 *   after a step whose *checkpoint_out was set (a final sweep that measures; all groups swept):
 *        hrag_shard_ppr_est(e, est, 0) -> all-reduce MAX of est fp32 [B] over the shards ->
 *        hrag_shard_ppr_est(e, est, 1) -> hrag_shard_ppr_decide(e, step)
 *   before hrag_shard_finish: the same get / all-reduce MAX / set once more (a session without extension stages has no
 *   measuring step), so that residual_out, iters_out and flags bit 4 come out identical on every shard. */
hrag_status hrag_shard_ppr_est(hrag_engine *e, float *est_dev, int32_t set, hrag_stream stream);
hrag_status hrag_shard_ppr_decide(hrag_engine *e, int32_t sweep, hrag_stream stream);
/* *open_out = 1 when step `step` of the session will do something (no gate, or its gate word says go), 0 when a
 * decision has closed its gate (every later step is then closed too) or `step` is past the last one.  The ONLY shard
 * entry point that synchronises the stream: a host loop that pays a collective per step calls it once after each
 * hrag_shard_ppr_decide and stops issuing steps -- and their exchanges -- when it returns 0. */
hrag_status hrag_shard_ppr_gate(hrag_engine *e, int32_t step, int32_t *open_out, hrag_stream stream);

/* doc scores of the owned passages (PPR probability, or the normalised DPR score on the fallback)
 * and their local top-k: idx_out_dev int32 [B, k] GLOBAL passage positions, score_out_dev fp32 [B, k].
 * flags_dev is read-modify-written (bit 1). */
hrag_status hrag_shard_finish(hrag_engine *e, const float *min_dev, const float *max_dev, int32_t *flags_dev,
                              int32_t batch, int32_t k, int32_t *idx_out_dev, float *score_out_dev,
                              float *residual_out_dev, int32_t *iters_out_dev, hrag_stream stream);
/* hrag_shard_finish with the doc filter (the GLOBAL mask of hrag_retrieve_filtered; the shard reads it at p_offset).
 * A shard whose slice holds no allowed passage returns all -1 rows, which the merge puts after every real entry. */
hrag_status hrag_shard_finish_filtered(hrag_engine *e, const float *min_dev, const float *max_dev, int32_t *flags_dev,
                                       int32_t batch, int32_t k, int32_t *idx_out_dev, float *score_out_dev,
                                       float *residual_out_dev, int32_t *iters_out_dev, hrag_stream stream,
                                       const uint32_t *filter_dev, int64_t filter_ld_words);

/* The "seeds" scope on a row shard (the scoped doc filter above, split where its statistics cross the shards).  The
 * filter is the GLOBAL one (filter_ld_words as in hrag_retrieve_filtered; NULL: HRAG_EINVAL).  The result of the recipe
 * above equals hrag_score_facts_scoped / hrag_retrieve_scoped of the unsharded engine bit for bit.
 * hrag_engine_set_fact_sources on a row shard takes the same GLOBAL table; the shard keeps the rows of its owned facts
 * (passage positions stay global).  The single-engine scoped calls return HRAG_EINVAL on a row shard.
 *   hrag_shard_score_facts_scoped     hrag_shard_score_facts among the owned facts that have an allowed source passage:
 *                                     RAW scores (global fact ids), min / max over those facts only; a shard without
 *                                     any (or without fact rows) returns -1 / 0 and +inf / -inf, the all-reduce's
 *                                     neutral values.  Needs hrag_engine_set_fact_sources.
 *   hrag_shard_passage_scores_scoped  the owned passage scores (kept inside the engine) + their min / max over the
 *                                     ALLOWED owned passages (none: +inf / -inf).
 *   hrag_shard_mask_prior             min_dev / max_dev = the all-reduced values of the previous step: rewrites the
 *                                     owned scores as hrag_retrieve_scoped's prior (allowed: (s - min) / (max - min), a
 *                                     zero range gives 1; others: 0) and returns the min / max of the rewritten rows
 *                                     (no owned passage: +inf / -inf).  Their all-reduce is what hrag_shard_prior_stats,
 *                                     hrag_shard_ppr_begin and hrag_shard_finish_filtered take.  min_out / max_out may
 *                                     be min_dev / max_dev. */
hrag_status hrag_shard_score_facts_scoped(hrag_engine *e, const uint16_t *q_fact_dev, int32_t batch, int32_t k,
                                          int32_t *idx_out_dev, float *score_out_dev, float *min_out_dev,
                                          float *max_out_dev, hrag_stream stream, const uint32_t *filter_dev,
                                          int64_t filter_ld_words);
hrag_status hrag_shard_passage_scores_scoped(hrag_engine *e, const uint16_t *q_pass_dev, int32_t batch,
                                             float *min_out_dev, float *max_out_dev, hrag_stream stream,
                                             const uint32_t *filter_dev, int64_t filter_ld_words);
hrag_status hrag_shard_mask_prior(hrag_engine *e, const float *min_dev, const float *max_dev, int32_t batch,
                                  float *min_out_dev, float *max_out_dev, hrag_stream stream, const uint32_t *filter_dev,
                                  int64_t filter_ld_words);

/* ------------------------------------------------------------------------------------------
 * ONE CALL PER PHASE on a row shard (round 6).  The steps above leave the order of the local steps, the exchanges and the
 * all-reduces to the host (hipporag_amd/dist.py ShardedRetriever is that host loop, ~100 lines per phase).  The two
 * drivers below run exactly that loop INSIDE the library and call the host back only for the collectives, so that a
 * multi-GPU host -- one process per GPU, one engine per process -- needs four small functions (RCCL one-liners on the
 * given stream) and two calls.  Results are bit-identical to the host loop (tests/test_gpu_multi.py, two processes).
 *
 * hrag_comm: every function works IN PLACE on DEVICE memory, must be ordered after the work already enqueued on `stream`
 * and before work enqueued on it later (an RCCL call on that stream is; a host-staged implementation synchronises it),
 * and returns 0 on success (anything else aborts the driver with HRAG_EINVAL).  world == 1: the pointers may be NULL.
 *   all_reduce      buf_dev: `count` elements of dtype HRAG_COMM_F32 / _F64 / _I32, op HRAG_COMM_MIN / _MAX / _SUM
 *   all_gather      recv_dev = world blocks of bytes_per_rank in rank order; block `rank` = send_dev
 *   exchange_begin  the per-sweep state exchange of one exchange group: region_dev = world blocks of own_bytes, block
 *                   `rank` holds this shard's fresh rows; start the all-gather in place (it may run asynchronously on a
 *                   stream of the host's as long as it is ordered behind `stream` at the time of the call) ...
 *   exchange_wait   ... and make `stream` wait for the exchange of `group` (every block then holds its owner's rows).
 *                   At most one exchange per group is in flight; group g's exchange overlaps the sweeps of the others.
 *                   When a driver returns an error it first calls exchange_wait for every exchange it had begun (rc
 *                   ignored), so the host's collective handles are never left open behind a failed call.
 * ------------------------------------------------------------------------------------------ */
#define HRAG_COMM_F32 0
#define HRAG_COMM_F64 1
#define HRAG_COMM_I32 2
#define HRAG_COMM_MIN 0
#define HRAG_COMM_MAX 1
#define HRAG_COMM_SUM 2
typedef struct hrag_comm {
    void *user;             /* passed back to every function */
    int32_t rank, world;
    int32_t (*all_reduce)(void *user, void *buf_dev, int64_t count, int32_t dtype, int32_t op, hrag_stream stream);
    int32_t (*all_gather)(void *user, const void *send_dev, void *recv_dev, int64_t bytes_per_rank, hrag_stream stream);
    int32_t (*exchange_begin)(void *user, void *region_dev, int64_t own_bytes, int32_t group, hrag_stream stream);
    int32_t (*exchange_wait)(void *user, int32_t group, hrag_stream stream);
} hrag_comm;

/* bytes of caller-owned device scratch the two drivers need for `batch` queries and lists of k entries (k > 2048: plus
 * the K4' scratch of the world * k -> k merge, hrag_topk_rows_workspace_bytes(batch, world * k, k)) */
int64_t hrag_shard_workspace_bytes(hrag_engine *e, int32_t world, int32_t batch, int32_t k);

/* phase A over all shards: hrag_shard_score_facts + all-gather of the candidates + MIN / MAX all-reduce + the merge:
 * idx_out_dev int32 [B, k] global fact ids (-1 beyond), score_out_dev fp32 [B, k] min-max normalised with the GLOBAL
 * row minimum / maximum -- replicated on every shard, equal to hrag_score_facts of the unsharded engine. */
hrag_status hrag_shard_score_facts_all(hrag_engine *e, const hrag_comm *comm, const uint16_t *q_fact_dev, int32_t batch,
                                       int32_t k, void *workspace_dev, int64_t workspace_bytes, int32_t *idx_out_dev,
                                       float *score_out_dev, hrag_stream stream);

/* phase B over all shards = hrag_retrieve of the unsharded engine (same arguments, same outputs, replicated on every
 * shard): passage scores, statistics all-reduced, hrag_shard_ppr_begin, every sweep of every exchange group with its
 * exchange, the contract's all-reduced measure and decisions (ppr_tol > 0), hrag_shard_finish, the merged top-k.
 * state0..2_dev: three state buffers of hrag_shard_layout_query(e, batch, n_groups).state_bytes, zeroed ONCE by the
 * caller (row V of every group must stay zero) and reusable across calls; flags_out_dev int32 [B] also carries bit 3
 * (HRAG_FLAG_FP8_SATURATED) of EVERY shard; residual_out_dev / iters_out_dev may be NULL (written when ppr_tol > 0). */
hrag_status hrag_shard_retrieve(hrag_engine *e, const hrag_comm *comm, const uint16_t *q_pass_dev, int32_t batch,
                                const int32_t *kept_idx_dev, const float *kept_score_dev, const int32_t *kept_count_dev,
                                int32_t kf, int32_t link_top_k, float damping, float passage_node_weight,
                                int32_t ppr_iters, int32_t ppr_max_iters, float ppr_tol, int32_t k, int32_t n_groups,
                                void *state0_dev, void *state1_dev, void *state2_dev, void *workspace_dev,
                                int64_t workspace_bytes, int32_t *doc_idx_out_dev, float *doc_score_out_dev,
                                int32_t *flags_out_dev, float *residual_out_dev, int32_t *iters_out_dev,
                                hrag_stream stream);
/* hrag_shard_retrieve with the doc filter (every shard passes the same global mask) = hrag_retrieve_filtered of the
 * unsharded engine. */
hrag_status hrag_shard_retrieve_filtered(hrag_engine *e, const hrag_comm *comm, const uint16_t *q_pass_dev, int32_t batch,
                                         const int32_t *kept_idx_dev, const float *kept_score_dev,
                                         const int32_t *kept_count_dev, int32_t kf, int32_t link_top_k, float damping,
                                         float passage_node_weight, int32_t ppr_iters, int32_t ppr_max_iters,
                                         float ppr_tol, int32_t k, int32_t n_groups, void *state0_dev, void *state1_dev,
                                         void *state2_dev, void *workspace_dev, int64_t workspace_bytes,
                                         int32_t *doc_idx_out_dev, float *doc_score_out_dev, int32_t *flags_out_dev,
                                         float *residual_out_dev, int32_t *iters_out_dev, hrag_stream stream,
                                         const uint32_t *filter_dev, int64_t filter_ld_words);
/* The drivers in the "seeds" scope (the recipe above inside the library; same arguments as hrag_shard_score_facts_all /
 * hrag_shard_retrieve_filtered, the same workspace; NULL filter: HRAG_EINVAL) = hrag_score_facts_scoped /
 * hrag_retrieve_scoped of the unsharded engine. */
hrag_status hrag_shard_score_facts_all_scoped(hrag_engine *e, const hrag_comm *comm, const uint16_t *q_fact_dev,
                                              int32_t batch, int32_t k, void *workspace_dev, int64_t workspace_bytes,
                                              int32_t *idx_out_dev, float *score_out_dev, hrag_stream stream,
                                              const uint32_t *filter_dev, int64_t filter_ld_words);
hrag_status hrag_shard_retrieve_scoped(hrag_engine *e, const hrag_comm *comm, const uint16_t *q_pass_dev, int32_t batch,
                                       const int32_t *kept_idx_dev, const float *kept_score_dev,
                                       const int32_t *kept_count_dev, int32_t kf, int32_t link_top_k, float damping,
                                       float passage_node_weight, int32_t ppr_iters, int32_t ppr_max_iters,
                                       float ppr_tol, int32_t k, int32_t n_groups, void *state0_dev, void *state1_dev,
                                       void *state2_dev, void *workspace_dev, int64_t workspace_bytes,
                                       int32_t *doc_idx_out_dev, float *doc_score_out_dev, int32_t *flags_out_dev,
                                       float *residual_out_dev, int32_t *iters_out_dev, hrag_stream stream,
                                       const uint32_t *filter_dev, int64_t filter_ld_words);

/* Index update with the embeddings staying on the device (incremental index() / delete(), HippoRAG.py:262-411:
 * the reference re-reads everything from its stores in prepare_retrieval_objects): compose the embedding
 * matrix of the NEXT engine from the rows this engine already holds and the rows that are new,
 *   out[i] = src_rows_dev[i] >= 0 ? held row src_rows_dev[i] : new_rows_dev[-src_rows_dev[i] - 1],
 * which: 0 = facts, 1 = passages; rows are dim 16-bit elements (3 * dim on an HRAG_F32_SPLIT engine: new rows in the
 * layout of hrag_split_f32); out_dev [n, dim] is caller-owned and can be
 * handed to hrag_engine_create as hrag_embed_desc.data (device pointers are accepted there). */
hrag_status hrag_engine_gather_embeddings(hrag_engine *e, int32_t which, const int32_t *src_rows_dev, int64_t n,
                                          const void *new_rows_dev, void *out_dev, hrag_stream stream);

/* set / clear HRAG_OPT_* tuning bits after creation (e.g. HRAG_OPT_NO_FP8 to rerun a batch that
 * reported HRAG_FLAG_FP8_SATURATED on the fp16 / fp32 state). */
hrag_status hrag_engine_set_flags(hrag_engine *e, int32_t flags, int32_t on);

hrag_status hrag_get_timings(hrag_engine *e, hrag_timings *out); /* synchronises the events */
hrag_status hrag_set_profiling(hrag_engine *e, int32_t enabled);

#ifdef __cplusplus
}
#endif
#endif /* HRAG_H_ */
