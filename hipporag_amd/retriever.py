"""Host-side mirror of the reference's retrieval surface, backed by the MI355X engine.

``HippoRAG`` here keeps the names, argument meaning, return types and error behaviour of the
reference class for THIS path (reference src/hipporag/HippoRAG.py):

    retrieve(queries, num_to_retrieve=None, gold_docs=None)      :413-499
    retrieve_dpr(queries, num_to_retrieve=None, gold_docs=None)  :665-732
    rag_qa(queries, gold_docs=None, gold_answers=None)           :591-663   (QA LLM injected)
    get_fact_scores / dense_passage_retrieval / rerank_facts / run_ppr / get_query_embeddings /
    prepare_retrieval_objects / ready_to_retrieve                :1287-1749 (per-method seams)

What is NOT here (out of scope, stays with the reference): OpenIE by LLM, embedding models,
vector stores, prompts, evaluation.  The index is therefore built from what those produce:
documents + their extracted triples + an embedding callable (``index_from_openie``), or straight
from arrays (``from_arrays``).  The graph rules are the reference's (add_fact_edges :867-913,
add_passage_edges :915-957, add_new_nodes :1159-1187, add_new_edges :1189-1223); synonymy edges
(:959-1020, needs the index-time KNN) are accepted as an explicit edge list.

Differences to the reference, all deliberate:
  * all queries of a call are batched through the device instead of the per-query loop (:459);
  * rankings use the documented tie rule (score desc, index desc) where numpy leaves ties open;
  * facts are kept in first-occurrence order (the reference uses list(set(...)), i.e. hash order).
"""

from __future__ import annotations

import contextlib
import gc
import logging
import re
import time
from dataclasses import dataclass, field
from hashlib import md5
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .graph import CSRGraph, build_csr, float_to_bf16_bits

logger = logging.getLogger("hipporag_amd")


# ------------------------------------------------------------------ utils/misc_utils.py mirrors
@dataclass(frozen=True)
class Chunk:                                            # misc_utils.py:35-40
    content: str
    source_id: Optional[str] = None
    metadata: Dict[str, Any] = field(default_factory=dict)


@dataclass
class RetrievalResult:                                  # misc_utils.py:43-50
    query: str
    docs: List[str]
    scores: np.ndarray
    doc_metadata: List[Dict[str, Any]] = field(default_factory=list)
    graph_seeds: List[Tuple] = field(default_factory=list)


@dataclass
class QuerySolution:                                    # misc_utils.py:52-78
    question: str
    docs: List[str]
    doc_scores: np.ndarray = None
    answer: str = None
    gold_answers: List[str] = None
    gold_docs: Optional[List[str]] = None
    thoughts: Optional[List[str]] = None
    doc_metadata: Optional[List[Dict[str, Any]]] = None
    graph_seeds: Optional[List[Tuple]] = None

    def to_dict(self):
        return {
            "question": self.question, "answer": self.answer, "gold_answers": self.gold_answers,
            "docs": self.docs[:5],
            "doc_scores": [round(v, 4) for v in self.doc_scores.tolist()[:5]] if self.doc_scores is not None else None,
            "gold_docs": self.gold_docs,
            "doc_metadata": self.doc_metadata[:5] if self.doc_metadata is not None else None,
            "graph_seeds": self.graph_seeds,
            **({"thoughts": self.thoughts} if self.thoughts is not None else {}),
        }


def compute_mdhash_id(content: str, prefix: str = "") -> str:      # misc_utils.py:141-152
    return prefix + md5(content.encode()).hexdigest()


def text_processing(text):                                          # misc_utils.py:80-85
    if isinstance(text, (list, tuple)):
        return [text_processing(t) for t in text]
    if not isinstance(text, str):
        text = str(text)
    return re.sub("[^A-Za-z0-9 ]", " ", text.lower()).strip()


def filter_invalid_triples(triples):                                # llm_utils.py:222-252
    """What index() applies to every chunk's OpenIE triples before anything else (reformat_openie_results,
    misc_utils.py:87-108, called at HippoRAG.py:305): triples without exactly three elements are dropped, EXACT duplicates
    (raw strings, before text_processing) collapse, order is kept.  Two triples that differ in case only stay two -- and
    count twice in the graph once text_processing has lower-cased them, as in the reference."""
    seen, out = set(), []
    for t in triples:
        if len(t) != 3:
            continue
        v = tuple(str(x) for x in t)
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def min_max_normalize(x):                                           # misc_utils.py:130-139
    mn, mx = np.min(x), np.max(x)
    rng = mx - mn
    if rng == 0:
        return np.ones_like(x)
    return (x - mn) / rng


# prompts/linking.py:1-10 -- the instruction sentences the reference hands to its (instruction-tuned)
# embedding models for the two query encodings of this path; stores embedded by the reference can only be
# searched with queries encoded under the same sentences
_QUERY_INSTRUCTIONS = {
    "query_to_fact": "Given a question, retrieve relevant triplet facts that matches this question.",
    "query_to_passage": "Given a question, retrieve relevant documents that best answer the question.",
}


def get_query_instruction(linking_method: str) -> str:
    return _QUERY_INSTRUCTIONS.get(linking_method, _QUERY_INSTRUCTIONS["query_to_passage"])


def sweeps_for_damping(damping: float, tol: float = 1e-6, lo: int = 16, hi: int = 400) -> int:
    """Number of power-iteration sweeps whose truncation error bound damping^K is <= tol (PRPACK iterates
    to 1e-10; the parity bar of this path is 1e-5 relative): 20 at the reference's 0.5, 86 at 0.85."""
    if not (0.0 < damping < 1.0):
        return lo
    return int(min(hi, max(lo, np.ceil(np.log(tol) / np.log(damping)))))


@dataclass
class RetrievalConfig:
    """The BaseConfig fields this path reads (utils/config_utils.py), same names and defaults."""
    linking_top_k: int = 5               # :184
    retrieval_top_k: int = 200           # :188
    damping: float = 0.5                 # :192
    passage_node_weight: float = 0.05    # :91
    qa_top_k: int = 5                    # :203
    embedding_return_as_normalized: bool = True   # :144
    is_directed_graph: bool = False      # :176
    # engine-only knobs (no reference analogue)
    embedding_precision: str = "f32"     # "f32": scores like the reference's fp32 np.dot (HippoRAG.py:1459,1496) -- the
                                         # stores' fp32 vectors as hi + lo fp16, three MFMA products per element
                                         # (HRAG_F32_SPLIT, 3x the embedding stream; unit-length vectors: include/hrag.h
                                         # states the bound); "bf16": vectors rounded to bf16 (1x
                                         # stream; near-tied facts / passages may swap against the reference)
    ppr_iters: Optional[int] = None      # None: derived from damping (sweeps_for_damping: 20 at 0.5)
    locality: Optional[str] = "auto"     # the engine renumbers the vertices by the first passage that links them (the
                                         # reference's entity ids are in hash order) and, when that numbering has
                                         # locality, sweeps in SELL-C-sigma windows with an XCD-blocked launch
                                         # (DESIGN.md 4.1); None: the caller's numbering as it is
    # convergence contract (include/hrag.h, hrag_retrieve; the reference's PRPACK iterates to 1e-10,
    # HippoRAG.py:1736-1743): the engine measures the relative update of the passage scores and keeps sweeping
    # while that measure is above ppr_tol.  The measure can UNDER-read the true error: the worst ratio measured
    # (tools/probe_convergence.py, ring graph) is residual / error = 0.29, so a query that passes at ppr_tol may carry
    # ppr_tol / 0.29.  1.5e-6 puts that worst case at 5.2e-6 = the 1e-5 relative parity bar with a factor 1.9 to
    # spare (round 3 shipped 3e-6: 1.03e-5 in that worst case, no margin); 0 = exactly ppr_iters sweeps
    ppr_tol: float = 1.5e-6
    ppr_max_iters: int = 400             # bound on the sweeps a slowly mixing graph may cost (fp8 state: 30, then
                                         # the flagged queries are repeated on the wider state)
    ppr_base_iters_narrow: Optional[int] = 12     # batches of at most 64 queries (interactive calls, IRCoT steps) under the
                                         # contract (ppr_tol > 0): this many sweeps ALWAYS run (>= 11) instead of the
                                         # worst-case count above, and the measured residual adds stages of 1, 2, 3, 3
                                         # sweeps where the graph needs them -- PRPACK likewise stops when ITS residual
                                         # says so (HippoRAG.py:1736-1743).  Same error bound (include/hrag.h; asserted per
                                         # query on the adversarial graphs: tests/test_gpu_fp8_adversarial.py); 15 sweeps
                                         # instead of 20 on the benchmark graph: -20 ... -24 % per call
                                         # (profiles/r06d_sweep_smallb_cfg3.json).  None / 0: the count above always runs
    ppr_accel: bool = True               # HRAG_OPT_ACCEL (include/hrag.h): wide batches (> 64 queries) run Chebyshev steps
                                         # inside the fp8 stages -- 17 sweeps + what the measured residual asks for
                                         # instead of 20 + ...; the answer is tolerance-driven either way, like the
                                         # reference's PRPACK solve (HippoRAG.py:1736-1743).  HippoRAG graphs are
                                         # undirected (config_utils.py:176), which is what the polynomial needs
    max_batch: int = 256
    slab_width: int = 0
    doc_filter_scope: str = "ranking"    # what a doc filter limits (include/hrag.h): "ranking" -- only the ranked list (a
                                         # post-filter); "seeds" -- also the facts phase A may pick and the passage prior,
                                         # normalised over the allowed passages (one tenant's documents in a shared index)
    group_by: Optional[str] = None       # grouped retrieval (include/hrag.h): a chunk-metadata key ("source_id" included);
                                         # retrieve() / retrieve_dpr() then rank the GROUPS of passages that share its value,
                                         # one best passage per group; None: passages, as the reference
    group_agg: str = "max"               # a group's score: "max" (its best passage's) or "sum" (of its passages' scores)
    group_hits: Optional[int] = None     # with group_by: the best m passages of each ranked group (1 .. 64) in the entry's
                                         # metadata ("group_hits"); None: the representative only
    mmr_lambda: Optional[float] = None   # diversified retrieval (include/hrag.h): retrieve() / retrieve_dpr() / rag_qa()
                                         # re-rank their candidates by Maximal Marginal Relevance with this lambda in [0, 1]
                                         # (1: relevance only, 0: diversity only after the first pick); None: off
    mmr_candidates: Optional[int] = None # how many ranked entries MMR picks from: max(this, num_to_retrieve), at most the
                                         # passages (or groups) there are and at most 1024; None: min(retrieval_top_k, 1024)
    lexical_weight: float = 0.0          # lexical retrieval (include/hrag.h): the weight in [0, 1] of the BM25 scores of the
                                         # query strings in the passage scores of retrieve() / retrieve_dpr() / rag_qa() /
                                         # retrieve_ircot(); 0: nothing is built and nothing changes
    lexical_tokenize_fn: Optional[Callable] = None   # str -> list of tokens, for passages and queries alike; None:
                                         # lexical.default_tokenize (lower-case, \w+)
    payload_index: bool = False          # payload filters (include/hrag.h): the chunk metadata (source_id included) as typed
                                         # columns on the device; metadata dict filters are then evaluated there and may use
                                         # $gt / $gte / $lt / $lte / $exists / $not / $any (payload.compile_filters); False:
                                         # the host bitsets, equality only
    late_candidates: Optional[int] = None   # late-interaction reranking (include/hrag.h; needs HippoRAG(token_encoder=)):
                                         # retrieve() / retrieve_dpr() / rag_qa() rank max(this, num_to_retrieve) entries, rescore
                                         # them by MaxSim over the token vectors and return the best by late score; None: off
    late_dtype: str = "bf16"             # the 16-bit type of the token vectors on the device: "bf16" or "fp16"
    feedback_weight: float = 0.3         # recommend by example (include/hrag.h): the weight in [0, 1] of the recommend rows of
                                         # retrieve(like=, unlike=) in the passage scores (relevance feedback into the prior)
    recommend_strategy: str = "best_score"   # "best_score" / "sum_scores" ("average_vector": recommend() only, refused by
                                         # retrieve(like=)): how the
                                         # liked and disliked passages of recommend() and retrieve(like=, unlike=) are scored
    boost: Optional[list] = None         # boosted retrieval (include/hrag.h): the default boost of every retrieve call, one list
                                         # of items in the grammar of boost.compile_boosts over the chunk-metadata columns
                                         # (needs payload_index=True); None: no boost


def identity_rerank_filter(query, candidate_items, candidate_indices, len_after_rerank=None):
    """Stand-in for DSPyFilter.__call__ (rerank.py:108-131): keeps every candidate."""
    n = len_after_rerank or len(candidate_items)
    return list(candidate_indices)[:n], list(candidate_items)[:n], {"confidence": None}


@contextlib.contextmanager
def gc_paused():
    """Materialising a batch allocates ~50 k small containers (lists of document strings, one metadata dict per
    document, HippoRAG.py:501-507); none of them can be part of a cycle, but they trip the cyclic collector every 700
    allocations and, every so often, a full pass over everything the process holds (the fact and passage tables: tens of
    milliseconds at 1 M facts).  retrieve() pauses the collector while it builds a batch's results: 7 -> 4 ms per
    256 x 200 documents."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class BatchRows(list):
    """What iter_batched_retrieve yields for a batch: the list of (doc ids, doc scores, kept facts) per query, plus the
    batch's arrays themselves (doc_idx int32 [b, k], doc_score fp32 [b, k]) for consumers that work on whole batches."""
    doc_idx = None
    doc_score = None
    group_idx = None     # grouped retrieval: int32 [b, k] group ids (doc_idx: each group's best passage, doc_score: its score)
    hit_idx = None       # group_hits=m: int32 [b, k, m] the best m allowed passages of each ranked group (-1 beyond them)
    hit_score = None     # fp32 [b, k, m] their own scores
    all_scores = None    # keep_all_scores=True: the device tensor fp32 [b, Np] of every passage's score
    repeated = False     # the convergence contract ran rows of the batch again: the engine's score rows are not the batch's


def unpack_mask(words, n: int) -> np.ndarray:
    """The doc filter's uint32 words [..., W] (engine.pack_mask) -> bool [..., n]."""
    w = np.ascontiguousarray(words, dtype="<u4")
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")[..., :n].astype(bool)


def ranked_scores(sc):
    """fp32 scores as every device ranking returns them: the quiet NaN, -0 as +0."""
    sc = np.array(sc, np.float32)
    sc[np.isnan(sc)] = np.float32(np.nan)
    return sc + np.float32(0)


def rank_allowed(full, allowed, want: int):
    """The host form of the filtered ranking: per row, the first `want` entries of np.argsort(x, kind="stable")[::-1]
    that `allowed` (bool [n] or [B, n]) admits, -1 / 0 beyond them -> (ids int32 [B, want], scores fp32 [B, want]);
    scores as every ranking returns them (ranked_scores)."""
    full = np.asarray(full, np.float32)
    b = full.shape[0]
    allowed = np.broadcast_to(np.asarray(allowed, bool), full.shape)
    idx = np.full((b, want), -1, np.int32)
    sc = np.zeros((b, want), np.float32)
    for i in range(b):
        order = np.argsort(full[i], kind="stable")[::-1]
        order = order[allowed[i][order]][:want]
        idx[i, :len(order)] = order
        sc[i, :len(order)] = full[i][order]
    return idx, ranked_scores(sc)


def group_hits_rows(full, group_of, allowed, group_idx, hits: int):
    """The host form of the group hits (include/hrag.h, group hits): per row of `full` fp32 [B, n] and per entry of
    group_idx int [B, k] (-1 or an id outside the table: an empty row) the first `hits` allowed members of that group by
    the ranking rule -> (hit_idx int32, hit_score fp32) [B, k, hits], -1 / 0 beyond the group's allowed members; scores as
    every ranking returns them (the quiet NaN, -0 as +0).  allowed: None, bool [n] or [B, n]."""
    full = np.asarray(full, np.float32)
    b, n = full.shape
    g = np.asarray(group_of, np.int64)
    gi = np.asarray(group_idx, np.int64)
    n_groups = int(g.max()) + 1 if g.size else 0
    allowed = np.ones((b, n), bool) if allowed is None else np.broadcast_to(np.asarray(allowed, bool), full.shape)
    hi = np.full(gi.shape + (hits,), -1, np.int32)
    hs = np.zeros(gi.shape + (hits,), np.float32)
    for i in range(b):
        order = np.argsort(full[i], kind="stable")[::-1]            # the ranking rule: best first, ties -> larger index
        order = order[allowed[i][order]]
        by_group = np.argsort(g[order], kind="stable")              # stable: the ranking's order inside every group
        members = order[by_group]
        start = np.searchsorted(g[order][by_group], np.arange(n_groups + 1))
        for j, gg in enumerate(gi[i]):
            if 0 <= gg < n_groups:
                top = members[start[gg]: min(start[gg + 1], start[gg] + hits)]
                hi[i, j, :len(top)] = top
                hs[i, j, :len(top)] = full[i][top]
    return hi, ranked_scores(hs)


def group_rank_rows(full, group_of, allowed, want: int, agg: str = "max", hits: Optional[int] = None):
    """The host form of the grouped ranking (include/hrag.h, grouped retrieval): per row of `full` fp32 [B, n] the first
    `want` groups -> (group ids, group scores, representative passages), -1 / 0 / -1 beyond the groups that have an allowed
    member.  allowed: None, bool [n] or [B, n].  hits=m: two more entries, group_hits_rows of the ranked groups."""
    full = np.asarray(full, np.float32)
    b, n = full.shape
    g = np.asarray(group_of, np.int64)
    n_groups = int(g.max()) + 1 if g.size else 0
    allowed = np.ones((b, n), bool) if allowed is None else np.broadcast_to(np.asarray(allowed, bool), full.shape)
    gi = np.full((b, want), -1, np.int32)
    gs = np.zeros((b, want), np.float32)
    rep = np.full((b, want), -1, np.int32)
    for i in range(b):
        order = np.argsort(full[i], kind="stable")[::-1]            # the ranking rule: best first, ties -> larger index
        order = order[allowed[i][order]]
        best = np.full(n_groups, -1, np.int64)
        best[g[order[::-1]]] = order[::-1]                           # the last write per group is its best member
        score = np.zeros(n_groups, np.float32)
        has = best >= 0
        if agg == "sum":
            a = allowed[i]
            with np.errstate(invalid="ignore", over="ignore"):
                score = np.bincount(g[a], weights=full[i][a].astype(np.float64), minlength=n_groups).astype(np.float32)
        else:
            score[has] = full[i][best[has]]
        rank = np.argsort(score, kind="stable")[::-1]
        rank = rank[has[rank]][:want]
        gi[i, :len(rank)], gs[i, :len(rank)], rep[i, :len(rank)] = rank, score[rank], best[rank]
    gs = ranked_scores(gs)
    if hits is not None:
        return (gi, gs, rep) + group_hits_rows(full, group_of, allowed, gi, hits)
    return gi, gs, rep


def fuse_rows_host(full, member_ptr, fuse: str, weights=None, rrf_c: int = 60, rrf_depth: int = 1, allowed=None):
    """The host form of the fusion (include/hrag.h, fused retrieval): member rows `full` fp32 [B, n] cut into questions by
    member_ptr -> fused rows fp32 [Q, n].  "sum": fp64 in member order, rounded once; "max": the member score that ranks
    first (any NaN wins; -0 as +0); "rrf": every member ranked at rrf_depth under its question's row of `allowed` (None,
    bool [n] or [Q, n]), float32(w / (rrf_c + rank)) added in fp32 in member order."""
    full = np.asarray(full, np.float32)
    mp = np.asarray(member_ptr, np.int64)
    nq, n = len(mp) - 1, full.shape[1]
    w = np.ones(full.shape[0], np.float32) if weights is None else np.asarray(weights, np.float32)
    out = np.zeros((nq, n), np.float32)
    if fuse == "rrf":
        allowed = np.ones((nq, n), bool) if allowed is None else np.broadcast_to(np.asarray(allowed, bool), (nq, n))
        lists, _ = rank_allowed(full, np.repeat(allowed, np.diff(mp), axis=0), rrf_depth)
        rank = np.arange(1, rrf_depth + 1, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(nq):
            rows = range(mp[q], mp[q + 1])
            if fuse == "sum":
                acc = np.zeros(n, np.float64)
                for i in rows:
                    acc = acc + np.float64(w[i]) * full[i].astype(np.float64)
                out[q] = acc.astype(np.float32)
            elif fuse == "max":
                m = full[mp[q]: mp[q + 1]]
                best = np.where(np.isnan(m), -np.inf, m).max(axis=0)
                out[q] = np.where(np.isnan(m).any(axis=0), np.float32(np.nan), best) + np.float32(0)
            else:
                for i in rows:
                    keep = lists[i] >= 0
                    t = (np.float64(w[i]) / (np.float64(rrf_c) + rank)).astype(np.float32)
                    out[q, lists[i][keep]] = out[q, lists[i][keep]] + t[keep]
    out[np.isnan(out)] = np.float32(np.nan)
    return out


def mmr_pool(mmr_candidates, want: int, available: int):
    """How many ranked entries MMR picks `want` of: max(mmr_candidates, want), at most the `available` passages (groups);
    None: want.  A value that is no int is handed on for check_mmr / mmr_plan to refuse."""
    if mmr_candidates is None:
        return want
    if isinstance(mmr_candidates, bool) or not isinstance(mmr_candidates, (int, np.integer)):
        return mmr_candidates
    return max(want, min(int(mmr_candidates), int(available)))


def masked_minmax_rows(raw, allowed):
    """The dense scores of the "seeds" scope on the host: per row, min_max_normalize over the allowed entries (a zero
    range gives 1), 0 elsewhere."""
    raw = np.asarray(raw, np.float32)
    allowed = np.broadcast_to(np.asarray(allowed, bool), raw.shape)
    out = np.zeros_like(raw)
    for i in range(raw.shape[0]):
        a = allowed[i]
        if a.any():
            out[i, a] = min_max_normalize(raw[i, a])
    return out


def scope_rows(doc_filter, lo: int, b: int):
    """The packed doc filter rows of queries [lo, lo + b) as the engine takes them (int32 view)."""
    import torch
    rows_w = doc_filter if doc_filter.ndim == 1 else doc_filter[lo: lo + b]
    return torch.from_numpy(np.ascontiguousarray(rows_w).view(np.int32))


def batched_retrieve(eng, queries: List[str], q_tensor: Callable, facts: Sequence, rerank_filter: Callable, **kw):
    """The body of retrieve() (HippoRAG.py:459-480) for all queries at once: one (doc ids, doc scores, kept facts) per
    query.  See iter_batched_retrieve, which this flattens."""
    out_rows = []
    for _, rows in iter_batched_retrieve(eng, queries, q_tensor, facts, rerank_filter, **kw):
        out_rows.extend(rows)
    return out_rows


def iter_batched_retrieve(eng, queries: List[str], q_tensor: Callable, facts: Sequence, rerank_filter: Callable, *,
                          linking_top_k: int, damping: float, passage_node_weight: float, ppr_iters: int,
                          num_to_retrieve: int, n_passages: int, timers=None, ppr_tol: float = 0.0,
                          ppr_max_iters: int = 0, ppr_base_iters_narrow: Optional[int] = None, doc_filter=None,
                          filter_scope: str = "ranking", group_agg: Optional[str] = None, group_of=None,
                          group_hits: Optional[int] = None, keep_all_scores: bool = False,
                          mmr_lambda: Optional[float] = None, mmr_candidates: Optional[int] = None,
                          lexical_encode: Optional[Callable] = None, lexical_weight: float = 0.0, boost=None,
                          late_encode: Optional[Callable] = None, late_candidates: Optional[int] = None,
                          feedback=None, feedback_weight: float = 0.0, feedback_strategy: str = "best_score"):
    """The body of retrieve() (HippoRAG.py:459-480), shared by the mirror class below and by
    reference_adapter.attach(): phase A on the device, the recognition-memory filter on the host (rerank_facts
    :1659-1707), phase B on the device, in batches of eng.max_batch queries.  Yields (offset of the batch, [(doc ids,
    doc scores, kept facts) per query]) batch by batch, in order; raises where the reference's asserts would (:1541,
    :1644).  timers: object whose rerank_time / ppr_time attributes are advanced like the reference's accumulators
    (:184-186).

    The batches are PIPELINED against the host: phase A of batch i + 1 is enqueued before the filter loop of batch i
    runs, and batch i's results are waited for (events on the copies to pinned memory, not a drain of the stream) only
    after batch i + 1's phase B was enqueued -- so the filter loop and whatever the consumer does with a yielded batch
    (the mirror builds its lists of document strings) run while the device works on the next batch.  The device sees
    A(0) A(1) B(0) A(2) B(1) ...; phase B takes everything it needs from its arguments, so the order is free.

    ppr_tol / ppr_max_iters: the convergence contract (RetrievalConfig): queries the engine flags as not converged
    within its sweep budget are repeated -- those queries only -- on the wider state with the sweeps their
    residual asks for, so a slowly mixing graph costs time, never accuracy.
    ppr_base_iters_narrow (RetrievalConfig.ppr_base_iters_narrow): the sweeps that ALWAYS run for a batch of at most 64
    queries under a tolerance -- the measure adds stages where the graph needs them.
    doc_filter: packed uint32 words (engine.pack_mask) [W] for every query or [len(queries), W]: only those passages
    are ranked (a post-filter: the scores do not change); passed to the engine only when given.
    filter_scope="seeds": phase A takes its facts from the allowed passages and phase B normalises the passage prior over
    them (include/hrag.h, scoped doc filter); needs doc_filter and an engine with fact sources.
    group_agg ("max" / "sum") with group_of (int array over the passages, already set on the engine): the rows rank
    GROUPS -- doc ids are each group's best passage, doc scores the group scores, rows.group_idx the group ids.
    group_hits=m (with group_agg): rows.hit_idx / rows.hit_score [b, k, m], the best m allowed passages of every ranked
    group; the engine serves them right behind each batch's grouped call, the host form beyond max_topk.
    mmr_lambda / mmr_candidates (include/hrag.h, diversified retrieval): each batch ranks max(mmr_candidates, want) entries
    -- at most the passages (groups) there are; mmr_candidates None: `want`, the mirror passes its retrieval_top_k -- and MMR
    picks `want` of them on the device (HippoRAGEngine.retrieve(mmr_lambda=)); rows.mmr_value [b, want] is the value of
    each pick.  At most min(1024, max_topk) candidates.
    lexical_encode / lexical_weight (include/hrag.h, lexical retrieval): with a weight above 0 every batch's query strings
    are encoded (lexical_encode(strings) -> the CSR triple of engine.check_lexical) and phase B gets lexical= /
    lexical_weight=; with 0 its arguments are exactly the plain ones.
    boost (include/hrag.h, boosted retrieval): a BoostProgram over all the queries (or a broadcast one); every batch's
    phase B gets boost= with its own rows of it, so every ranking output -- and all_scores -- is that of the boosted rows.
    late_encode / late_candidates (include/hrag.h, late-interaction reranking): every batch's query strings are encoded
    (late_encode(strings) -> a LateQueries) and phase B gets late= / late_candidates=: each batch ranks
    max(late_candidates, want) entries, rescores them and returns the `want` best by late score -- doc scores are the late
    scores, rows.first_score [b, want] each entry's first-stage score.  Not with group_agg or beyond max_topk; with
    mmr_lambda MMR picks among the rescored entries (mmr_candidates is then not used).
    feedback / feedback_weight / feedback_strategy (include/hrag.h, recommend by example): an Examples over ALL the queries;
    with a weight above 0 every batch's phase B gets feedback= with its own rows of it (Examples.select); with 0, or without
    examples, its arguments are exactly the plain ones.
    keep_all_scores: rows.all_scores is the device tensor of every passage's score of the batch and rows.repeated tells
    whether the contract ran rows again (retrieve_fused: the engine's own score rows are then not the batch's)."""
    import torch
    from .engine import host_copy_async, host_wait
    k_f = int(linking_top_k)
    want = max(1, min(int(num_to_retrieve), n_passages))
    from .engine import check_group_hits
    group_hits = check_group_hits(group_hits, group_agg)
    if group_agg is not None:
        if group_of is None:
            raise ValueError("group_agg needs group_of (the passage -> group table)")
        want = max(1, min(want, int(np.max(group_of)) + 1))
    k_docs = min(want, eng.max_topk)
    mmr = None
    if mmr_lambda is not None or mmr_candidates is not None:
        from .engine import MMR_MAX_CANDIDATES, mmr_plan
        mmr = mmr_plan(mmr_lambda, mmr_pool(mmr_candidates, want, n_passages if group_agg is None else
                                            min(n_passages, int(np.max(group_of)) + 1)), want)
        if mmr[1] > eng.max_topk:
            raise ValueError(f"mmr_candidates={mmr[1]} (at least num_to_retrieve) exceeds the engine's max_topk={eng.max_topk}: "
                             f"MMR picks from one device ranking of at most min({MMR_MAX_CANDIDATES}, max_topk) entries")
    # more documents than the device top-k holds (HippoRAG.py:501-507 slices any prefix of the full ranking): the
    # scores of all passages come back and are ranked here with the library's rule (score desc, larger index first)
    beyond = k_docs < want and hasattr(eng, "last_doc_scores")
    late_c = None
    if late_encode is not None:
        from .late import LATE_MAX_CANDIDATES
        if group_agg is not None:
            raise ValueError("late_candidates does not serve group_agg: a group's score is not a passage's")
        late_c = max(int(want if late_candidates is None else late_candidates), want)
        late_c = min(late_c, n_passages)
        if want > eng.max_topk or late_c > min(eng.max_topk, LATE_MAX_CANDIDATES):
            raise ValueError(f"late_candidates={late_c} (at least num_to_retrieve={want}) exceeds what one device ranking "
                             f"holds, min({LATE_MAX_CANDIDATES}, max_topk={eng.max_topk})")
    if k_docs < want and not beyond:
        logger.warning("num_to_retrieve=%d exceeds the engine's max_topk=%d: %d documents per query are returned "
                       "(create the engine with a larger retrieval_top_k)", num_to_retrieve, eng.max_topk, k_docs)
    use_facts = len(facts) > 0 and k_f > 0
    from .engine import check_filter_scope
    scoped = doc_filter is not None and check_filter_scope(filter_scope, doc_filter)
    if scoped and lexical_encode is not None and lexical_weight > 0:
        raise NotImplementedError('filter_scope="seeds" is not served with lexical_weight > 0: the blend\'s min-maxes run over '
                                  'every passage -- use filter_scope="ranking"')
    if feedback is not None and feedback_weight > 0:
        if lexical_encode is not None and lexical_weight > 0:
            raise ValueError("like / unlike together with lexical_weight > 0: both own the blend of the passage scores")
        if scoped:
            raise NotImplementedError('filter_scope="seeds" is not served with like / unlike: the blend\'s min-maxes run over '
                                      'every passage -- use filter_scope="ranking"')
        if feedback.batch != len(queries):
            raise ValueError(f"like / unlike hold {feedback.batch} queries, the call {len(queries)}")
    if scoped and use_facts and not getattr(eng, "has_fact_sources", False):
        raise ValueError('filter_scope="seeds" needs the fact -> passage table on the engine (set_fact_sources)')
    two_halves = hasattr(eng, "retrieve_converged_start")
    starts = list(range(0, len(queries), eng.max_batch))

    def tick(name, t0):
        if timers is not None:
            setattr(timers, name, getattr(timers, name, 0.0) + time.time() - t0)

    class Batch:
        pass

    def start_a(lo):                                                                   # phase A, enqueued
        bt = Batch()
        bt.lo, bt.qs = lo, queries[lo: lo + eng.max_batch]
        bt.a = None
        if use_facts:
            t0 = time.time()
            if scoped:
                idx, sc = eng.score_facts(q_tensor(bt.qs, "triple"), k=k_f,
                                          scope_filter=scope_rows(doc_filter, lo, len(bt.qs)))
            else:
                idx, sc = eng.score_facts(q_tensor(bt.qs, "triple"), k=k_f)
            bt.a = (host_copy_async(idx), host_copy_async(sc))
            tick("rerank_time", t0)
        return bt

    def filter_and_start_b(bt):                                                        # host: LLM filter; phase B, enqueued
        qs = bt.qs
        b = len(qs)
        kept_idx = np.full((b, max(k_f, 1)), -1, np.int32)
        kept_sc = np.zeros((b, max(k_f, 1)), np.float32)
        kept_cnt = np.zeros(b, np.int32)
        bt.seeds = [[] for _ in range(b)]
        t0 = time.time()
        if bt.a is not None:
            idx_l, sc_l = host_wait(bt.a[0]).tolist(), host_wait(bt.a[1]).tolist()     # python ints / floats, once
            for i, q in enumerate(qs):
                row, srow = idx_l[i], sc_l[i]
                cand = [j for j in row if j >= 0]
                try:
                    kidx, kfacts, _ = rerank_filter(q, [facts[j] for j in cand], cand, len_after_rerank=k_f)
                except Exception as exc:                                               # :1705-1707
                    logger.error("Error in rerank_facts: %s", exc)
                    kidx, kfacts = [], []
                score_of = {j: srow[p] for p, j in enumerate(row) if j >= 0}
                kidx = [j for j in map(int, kidx) if j in score_of][:k_f]
                n = len(kidx)
                if n:
                    kept_idx[i, :n] = kidx
                    kept_sc[i, :n] = [score_of[j] for j in kidx]
                kept_cnt[i] = n
                bt.seeds[i] = list(kfacts)
        tick("rerank_time", t0)
        t0 = time.time()
        args = (q_tensor(qs, "passage"), torch.from_numpy(kept_idx), torch.from_numpy(kept_sc), torch.from_numpy(kept_cnt))
        base = ppr_iters
        if ppr_base_iters_narrow and ppr_tol > 0 and len(qs) <= 64 and damping <= 0.5:     # (the two-stage state's short
            # split is an argument about damping^9: csrc/engine.hip two_stage_ok; other damping factors keep the count above)
            base = max(11, min(int(ppr_base_iters_narrow), ppr_iters))     # narrow batch under the contract: latency mode
        kw = dict(link_top_k=k_f, damping=damping, passage_node_weight=passage_node_weight, ppr_iters=base,
                  k=k_docs, ppr_tol=ppr_tol, ppr_max_iters=ppr_max_iters,
                  **({"want_all_scores": True} if beyond or keep_all_scores else {}))
        if doc_filter is not None:
            kw["doc_filter"] = scope_rows(doc_filter, bt.lo, b)
            if scoped:
                kw["filter_scope"] = "seeds"
        if group_agg is not None:
            kw["group_agg"] = group_agg
        if group_hits is not None and not beyond:
            kw["group_hits"] = group_hits
        if mmr is not None:
            kw.update(mmr_lambda=mmr[0], **({} if late_c is not None else {"mmr_candidates": mmr[1]}))
        if lexical_encode is not None and lexical_weight > 0:
            kw.update(lexical=lexical_encode(qs), lexical_weight=lexical_weight)
        if late_c is not None:
            kw.update(late=late_encode(qs), late_candidates=late_c)
        if boost is not None:
            kw["boost"] = boost.select(range(bt.lo, bt.lo + b))
        if feedback is not None and feedback_weight > 0:
            kw.update(feedback=feedback.select(range(bt.lo, bt.lo + b)), feedback_weight=feedback_weight,
                      feedback_strategy=feedback_strategy)
        if two_halves:
            bt.pending = eng.retrieve_converged_start(*args, **kw)
            o = bt.pending.out
            bt.copies = (host_copy_async(o.doc_idx), host_copy_async(o.doc_score))
            if group_agg is not None:
                bt.copies += (host_copy_async(o.group_idx),)
            if "group_hits" in kw:
                bt.copies += (host_copy_async(o.hit_idx), host_copy_async(o.hit_score))
            if mmr is not None:
                bt.mmr_copy = host_copy_async(o.mmr_value)
            if late_c is not None:
                bt.first_copy = host_copy_async(o.first_score)
        else:                                       # an engine with the one-call form only (test doubles)
            bt.pending, bt.out = None, eng.retrieve_converged(*args, **kw)
        tick("ppr_time", t0)

    def finish(bt):
        t0 = time.time()
        if bt.pending is not None:
            out = bt.pending.finish()
            if bt.pending.repeated:                 # something was run again: take what the tensors hold now
                d_idx, d_sc = out.doc_idx.cpu().numpy(), out.doc_score.cpu().numpy()
            else:
                # out of the pinned staging buffers: the rows handed out must not keep page-locked memory alive
                d_idx, d_sc = host_wait(bt.copies[0]).copy(), host_wait(bt.copies[1]).copy()
            flags = bt.pending.flags                # host copy: reading out.flags would drain the stream
        else:
            out = bt.out
            d_idx, d_sc = out.doc_idx.cpu().numpy(), out.doc_score.cpu().numpy()
            flags = out.flags.cpu().numpy()
        g_idx = h_idx = h_sc = None
        if group_agg is not None and not beyond:
            copied = bt.pending is not None and not bt.pending.repeated
            g_idx = host_wait(bt.copies[2]).copy() if copied else out.group_idx.cpu().numpy()
            if group_hits is not None:
                h_idx, h_sc = ((host_wait(bt.copies[3]).copy(), host_wait(bt.copies[4]).copy()) if copied
                               else (out.hit_idx.cpu().numpy(), out.hit_score.cpu().numpy()))
        if beyond and group_agg is not None:
            full = out.all_scores.cpu().numpy()
            rows_w = None if doc_filter is None else (doc_filter if doc_filter.ndim == 1
                                                      else doc_filter[bt.lo: bt.lo + len(bt.qs)])
            g_idx, d_sc, d_idx, *h = group_rank_rows(full, group_of, None if rows_w is None else
                                                     unpack_mask(rows_w, full.shape[1]), want, group_agg, group_hits)
            if h:
                h_idx, h_sc = h
        elif beyond:
            full = out.all_scores.cpu().numpy()
            if doc_filter is not None:
                rows_w = doc_filter if doc_filter.ndim == 1 else doc_filter[bt.lo: bt.lo + len(bt.qs)]
                d_idx, d_sc = rank_allowed(full, unpack_mask(rows_w, full.shape[1]), want)
            else:
                d_idx = np.stack([np.argsort(r, kind="stable")[::-1][:want] for r in full]).astype(np.int32)
                d_sc = ranked_scores(np.take_along_axis(full, d_idx.astype(np.int64), axis=1))
        tick("ppr_time", t0)
        rows = BatchRows()
        rows.doc_idx, rows.doc_score, rows.group_idx = d_idx, d_sc, g_idx
        rows.hit_idx, rows.hit_score = h_idx, h_sc
        rows.mmr_value = None
        if mmr is not None:
            copied = bt.pending is not None and not bt.pending.repeated
            rows.mmr_value = host_wait(bt.mmr_copy).copy() if copied else out.mmr_value.cpu().numpy()
        rows.first_score = None
        if late_c is not None:
            copied = bt.pending is not None and not bt.pending.repeated
            rows.first_score = host_wait(bt.first_copy).copy() if copied else out.first_score.cpu().numpy()
        if keep_all_scores:
            rows.all_scores = getattr(out, "all_scores", None)
            rows.repeated = bt.pending is None or bt.pending.repeated
        for i in range(len(bt.qs)):
            if flags[i] & 4:      # :1541
                raise AssertionError("count_nonzero(all_phrase_weights) != len(linking_score_map)")
            if flags[i] & 2:      # :1644
                raise AssertionError(f"No phrases found in the graph for the given facts: {bt.seeds[i]}")
            if flags[i] & 1:
                logger.info("No facts found after reranking, return DPR results")      # :468
            rows.append((d_idx[i], d_sc[i], bt.seeds[i]))
        return bt.lo, rows

    if not starts:
        return
    nxt, prev = start_a(starts[0]), None
    for n, lo in enumerate(starts):
        cur = nxt
        if bt_wait := cur.a:                        # batch n's fact candidates are needed on the host now
            t0 = time.time()
            host_wait(bt_wait[0])
            tick("rerank_time", t0)
        nxt = start_a(starts[n + 1]) if n + 1 < len(starts) else None
        filter_and_start_b(cur)
        if prev is not None:
            yield finish(prev)
        prev = cur
    yield finish(prev)


_NO_GROUP = object()     # a passage without the group_by key: a group of its own


class HippoRAG:
    def __init__(self, global_config: Optional[RetrievalConfig] = None, embedding_model=None,
                 rerank_filter: Optional[Callable] = None, qa_fn: Optional[Callable] = None, token_encoder=None):
        """embedding_model: object with batch_encode(texts, instruction=..., norm=True) -> [n, D]
        (reference embedding_model/base.py); rerank_filter: callable like DSPyFilter (identity by
        default); qa_fn(query_solutions) -> (solutions, messages, metadata) like HippoRAG.qa (:808);
        token_encoder: object with encode_tokens(texts, is_query) -> one float array [t_i, dim] per text (a ColBERT-style
        encoder; late-interaction reranking, late_candidates=)."""
        self.global_config = global_config or RetrievalConfig()
        self.embedding_model = embedding_model
        self.rerank_filter = rerank_filter or identity_rerank_filter
        self.qa_fn = qa_fn
        self.ready_to_retrieve = False
        self.engine = None
        self.ppr_time = self.rerank_time = self.all_retrieval_time = 0.0      # :184-186
        self.query_to_embedding: Dict[str, Dict[str, np.ndarray]] = {"triple": {}, "passage": {}}
        # index state
        self.passage_node_keys: List[str] = []
        self.passage_texts: List[str] = []
        self.chunk_metadata: Dict[str, Dict[str, Any]] = {}
        self.entity_node_keys: List[str] = []
        self.entity_texts: List[str] = []
        self.fact_node_keys: List[str] = []
        self.facts: List[Tuple[str, str, str]] = []
        self.node_name_to_vertex_idx: Dict[str, int] = {}
        self.ent_node_to_chunk_ids: Dict[str, set] = {}
        self.node_to_node_stats: Dict[Tuple[str, str], float] = {}
        self.proc_triples_to_docs: Dict[Tuple[str, str, str], set] = {}
        self._chunk_triples: Dict[str, list] = {}          # chunk key -> processed triples (the OpenIE store)
        self._graph = None                                 # graph.IncrementalGraph (the igraph object)
        self._pass_emb = self._fact_emb = None             # fp32 rows in store order
        self._arrays = None
        self.lexical_model = self.lexical_index = None     # lexical retrieval (lexical_weight > 0): built with the engine
        self.payload_index = None                          # payload filters (payload_index=True): built with the engine
        self.token_encoder = token_encoder                 # late-interaction reranking (late_candidates=)
        self.token_index = None                            # ... its TokenIndex, built with the engine or on first use
        self._token_cache: Dict[str, np.ndarray] = {}      # passage key -> its token vectors [t, dim] (encoded once)

    # ------------------------------------------------------------------ index side
    def index_from_openie(self, docs: Sequence, chunk_triples: Sequence[Sequence[Sequence[str]]],
                          synonym_edges: Optional[Sequence[Tuple[str, str, float]]] = None,
                          passage_embeddings=None, entity_embeddings=None, fact_embeddings=None,
                          synonymy=None, synonymy_edge_topk: int = 2047, synonymy_edge_sim_threshold: float = 0.8):
        """index() after its LLM steps (HippoRAG.py:262-335): documents + their OpenIE triples in, graph /
        fact / passage arrays out.  Like the reference it is INCREMENTAL: a later call adds the chunks that
        are new (duplicates collapse on their hash), appends the entities / facts / vertices that did not
        exist (stores and igraph keep insertion order), and appends edges for the NEW chunks only
        (add_fact_edges counts a triple only while its chunk is not a graph vertex yet, :899-903;
        add_passage_edges likewise, :939-947) -- parallel to the existing ones, which is how an entity pair
        seen again gains weight (igraph multigraph; graph.build_csr sums).  Embeddings are taken as given
        (rows for the docs of THIS call / for the NEW entities and facts in the order this method appends
        them) or computed with embedding_model.batch_encode(texts) (embedding_store.py:131).

        Synonymy edges (add_synonymy_edges, :959-1020 -- in the reference part of every index() call that adds a chunk):
        `synonym_edges` = an explicit list [(phrase a, phrase b, score)], and / or `synonymy` = "knn": the KNN over ALL
        entities the store holds after this call on the GPU (hipporag_amd.knn.synonymy_candidates, the reference's
        selection rules, `synonymy_edge_topk` / `synonymy_edge_sim_threshold` like config_utils.py), or a callable
        (entity keys, entity texts, fp32 embeddings, topk=, sim_threshold=) -> [(key a, key b, score)] with the same contract.
        Needs entity embeddings (given, or an embedding_model)."""
        from .graph import IncrementalGraph
        chunks = [d if isinstance(d, Chunk) else Chunk(content=d) for d in docs]
        if len(chunks) != len(chunk_triples):
            raise ValueError("one triple list per document")
        if self._graph is None:
            self._graph = IncrementalGraph()
        g = self._graph
        new_chunk_keys, new_chunk_rows = [], []
        for pos, (ch, tr) in enumerate(zip(chunks, chunk_triples)):   # duplicate docs collapse on their hash
            key = compute_mdhash_id(ch.content, "chunk-")
            meta = dict(ch.metadata)
            if ch.source_id is not None:
                meta["source_id"] = ch.source_id
            self.chunk_metadata[key] = meta
            if key not in self._chunk_triples:
                self._chunk_triples[key] = [tuple(text_processing(list(t))) for t in filter_invalid_triples(tr)]
                self.passage_node_keys.append(key)
                self.passage_texts.append(ch.content)
                new_chunk_keys.append(key)
                new_chunk_rows.append(pos)
        proc_new = [self._chunk_triples[k] for k in new_chunk_keys]
        # entity / fact stores: insert_strings appends what is missing (:316-320); sorted unique entities
        # (extract_entity_nodes, misc_utils.py:110-121), facts in first-occurrence order (flatten_facts :123-128)
        known_e = set(self.entity_node_keys)
        new_ents = [e for e in sorted({e for tr in proc_new for t in tr for e in (t[0], t[2])})
                    if compute_mdhash_id(e, "entity-") not in known_e]
        self.entity_texts += new_ents
        self.entity_node_keys += [compute_mdhash_id(e, "entity-") for e in new_ents]

        def embed(given, strings, dim=None):
            if given is not None:
                given = np.asarray(given, dtype=np.float32)
                if given.shape[0] != len(strings):
                    raise ValueError(f"{given.shape[0]} embedding rows for {len(strings)} new strings")
                return given
            if not strings:
                return np.zeros((0, dim or 0), np.float32)
            if self.embedding_model is None:
                raise ValueError("no embeddings given and no embedding_model to compute them")
            return np.asarray(self.embedding_model.batch_encode(list(strings)), dtype=np.float32)

        # the entity store's rows first: the synonymy KNN below reads them
        if entity_embeddings is not None or (self.embedding_model is not None and new_ents):
            ee_new = embed(entity_embeddings, new_ents)
            self.entity_embeddings = ee_new if getattr(self, "entity_embeddings", None) is None else (
                np.concatenate([self.entity_embeddings, ee_new]) if ee_new.size else self.entity_embeddings)
        elif not hasattr(self, "entity_embeddings"):
            self.entity_embeddings = None
        known_f = set(self.facts)
        new_facts = []
        for tr in proc_new:
            for t in tr:
                if t not in known_f:
                    known_f.add(t)
                    new_facts.append(t)
        self.facts += new_facts
        self.fact_node_keys += [compute_mdhash_id(str(f), "fact-") for f in new_facts]
        # graph bookkeeping: add_fact_edges (:867-913) + add_passage_edges (:915-957), new chunks only
        self.node_to_node_stats = {}
        for chunk_key, tr in zip(new_chunk_keys, proc_new):
            in_chunk = set()
            for t in tr:
                a, b = compute_mdhash_id(t[0], "entity-"), compute_mdhash_id(t[2], "entity-")
                in_chunk.update((a, b))
                self.node_to_node_stats[(a, b)] = self.node_to_node_stats.get((a, b), 0.0) + 1
                self.node_to_node_stats[(b, a)] = self.node_to_node_stats.get((b, a), 0.0) + 1
                self.proc_triples_to_docs.setdefault(t, set()).add(chunk_key)          # :1353-1361
            for n in in_chunk:
                self.ent_node_to_chunk_ids.setdefault(n, set()).add(chunk_key)
            for e in sorted({e for t in tr for e in (t[0], t[2])}):
                self.node_to_node_stats[(chunk_key, compute_mdhash_id(e, "entity-"))] = 1.0
        for a, b, w in (synonym_edges or []):              # add_synonymy_edges result (:1007-1018)
            ka = compute_mdhash_id(text_processing(a), "entity-")
            kb = compute_mdhash_id(text_processing(b), "entity-")
            self.node_to_node_stats[(ka, kb)] = float(w)
        if synonymy is not None and new_chunk_keys and len(self.entity_node_keys) > 1:      # :329-335: only with new chunks
            if synonymy == "knn":
                from .knn import synonymy_candidates as synonymy
            elif not callable(synonymy):
                raise ValueError("synonymy must be None, 'knn' or a callable")
            if self.entity_embeddings is None or len(self.entity_embeddings) != len(self.entity_node_keys):
                raise ValueError("synonymy edges need the embeddings of every entity (entity_embeddings= or an embedding_model)")
            for ka, kb, w in synonymy(list(self.entity_node_keys), list(self.entity_texts), self.entity_embeddings,
                                      topk=synonymy_edge_topk, sim_threshold=synonymy_edge_sim_threshold):
                self.node_to_node_stats[(ka, kb)] = float(w)      # overwrites a fact-edge count of the same pair, like :1015
        if new_chunk_keys:                                 # augment_graph only when chunks were added (:329-335)
            # vertices: the entity store's rows, then the chunk store's, that are not vertices yet (:1171-1187)
            g.add_vertices(self.entity_node_keys)
            g.add_vertices(self.passage_node_keys)
            g.add_edges(list(self.node_to_node_stats.keys()), list(self.node_to_node_stats.values()))   # :1200-1223

        if passage_embeddings is not None:                 # rows of THIS call's docs: keep the new chunks' rows
            passage_embeddings = np.asarray(passage_embeddings, np.float32)[new_chunk_rows]
        pe_new = embed(passage_embeddings, [self.passage_texts[self.passage_node_keys.index(k)] for k in new_chunk_keys])
        dim = pe_new.shape[1] if pe_new.size else (self._pass_emb.shape[1] if self._pass_emb is not None else 0)
        fe_new = embed(fact_embeddings, [str(f) for f in new_facts], dim)
        self._pass_emb = pe_new if self._pass_emb is None else np.concatenate([self._pass_emb, pe_new])
        self._fact_emb = fe_new if self._fact_emb is None or not self._fact_emb.size else (
            np.concatenate([self._fact_emb, fe_new]) if fe_new.size else self._fact_emb)
        self._refresh_arrays()
        return self

    def _refresh_arrays(self):
        """The engine-facing arrays from the current graph / stores (what prepare_retrieval_objects reads,
        HippoRAG.py:1287-1389)."""
        self._filter_cache = {}          # the passage list changed: every cached doc filter bitset is stale
        self._group_cache = None         # ... and so is the passage -> group table of grouped retrieval
        g = self._graph
        self.node_name_to_vertex_idx = dict(g.index)
        csr = g.to_csr()
        num_chunks = np.zeros(g.num_vertices, np.int32)
        for k, srcs in self.ent_node_to_chunk_ids.items():
            if k in g.index:
                num_chunks[g.index[k]] = len(srcs)

        def vid(phrase):                                   # HippoRAG.py:1584-1597
            return g.index.get(compute_mdhash_id(phrase.lower(), "entity-"), -1)

        subj = np.array([vid(f[0]) for f in self.facts], np.int32)
        obj = np.array([vid(f[2]) for f in self.facts], np.int32)
        pv = np.array([g.index[k] for k in self.passage_node_keys], np.int32)
        has_facts = len(self.facts) > 0
        self._arrays = dict(csr=csr, passage_vertex=pv, passage_emb=self._emb_for_engine(self._pass_emb),
                            fact_emb=self._emb_for_engine(self._fact_emb) if has_facts else None, subj=subj, obj=obj,
                            num_chunks=num_chunks)
        self.ready_to_retrieve = False                      # explicit invalidate hook

    def _emb_for_engine(self, emb):
        """The stores' fp32 rows as the engine takes them: fp32 (HRAG_F32_SPLIT) or bf16 bit patterns."""
        prec = self.global_config.embedding_precision
        if prec not in ("f32", "bf16"):
            raise ValueError(f"embedding_precision must be 'f32' or 'bf16', not {prec!r}")
        e = np.ascontiguousarray(emb, dtype=np.float32)
        return e if prec == "f32" else float_to_bf16_bits(e)

    # ------------------------------------------------------------------ delete :337-411
    def delete(self, docs_to_delete: Sequence[str]):
        """Remove documents: their chunk vertices, the facts no remaining chunk states, and the entities no
        remaining chunk mentions (stores, embeddings and graph vertices -- igraph renumbers the rest, :408).
        Like the reference, edges between entities that survive are NOT decremented (delete only removes
        vertices), and the surviving entities lose the deleted chunks from ent_node_to_chunk_ids (the
        divisor of the seed weights, :1600-1601)."""
        if self._graph is None:
            return self
        key_of = {t: k for k, t in zip(self.passage_node_keys, self.passage_texts)}
        chunk_ids = {key_of[d] for d in docs_to_delete if d in key_of}                 # :351-356
        if not chunk_ids:
            return self
        affected = {t for k in chunk_ids for t in self._chunk_triples[k]}                # :359-374
        dead_facts = set()
        for t in affected:
            left = self.proc_triples_to_docs.get(t, set()) - chunk_ids
            if left:
                self.proc_triples_to_docs[t] = left
            else:
                self.proc_triples_to_docs.pop(t, None)
                dead_facts.add(t)
        dead_ents = set()
        for e in {x for t in affected for x in (t[0], t[2])}:                            # :377-390
            k = compute_mdhash_id(e, "entity-")
            left = self.ent_node_to_chunk_ids.get(k, set()) - chunk_ids
            if left:
                self.ent_node_to_chunk_ids[k] = left
            else:
                self.ent_node_to_chunk_ids.pop(k, None)
                dead_ents.add(k)
        logger.info("Deleting %d Chunks", len(chunk_ids))
        logger.info("Deleting %d Triples", len(dead_facts))
        logger.info("Deleting %d Entities", len(dead_ents))
        keep_p = [i for i, k in enumerate(self.passage_node_keys) if k not in chunk_ids]   # stores (:398-403)
        keep_f = [i for i, f in enumerate(self.facts) if f not in dead_facts]
        keep_e = [i for i, k in enumerate(self.entity_node_keys) if k not in dead_ents]
        self.passage_node_keys = [self.passage_node_keys[i] for i in keep_p]
        self.passage_texts = [self.passage_texts[i] for i in keep_p]
        self._pass_emb = self._pass_emb[keep_p]
        self.facts = [self.facts[i] for i in keep_f]
        self.fact_node_keys = [self.fact_node_keys[i] for i in keep_f]
        self._fact_emb = self._fact_emb[keep_f] if self._fact_emb is not None and self._fact_emb.size else self._fact_emb
        self.entity_texts = [self.entity_texts[i] for i in keep_e]
        self.entity_node_keys = [self.entity_node_keys[i] for i in keep_e]
        if getattr(self, "entity_embeddings", None) is not None:
            self.entity_embeddings = self.entity_embeddings[keep_e]
        for k in chunk_ids:
            self._chunk_triples.pop(k, None)
            self.chunk_metadata.pop(k, None)
        self._graph.delete_vertices(list(dead_ents) + list(chunk_ids))                  # :408
        self._refresh_arrays()                                                          # :411 ready_to_retrieve = False
        return self

    @classmethod
    def from_arrays(cls, csr: CSRGraph, passage_vertex, passage_emb_bits, fact_emb_bits, subj, obj, num_chunks,
                    passage_texts: Optional[List[str]] = None, facts: Optional[List[Tuple]] = None, **kw):
        self = cls(**kw)
        n_p = len(passage_vertex)
        self.passage_texts = passage_texts or [f"passage {i}" for i in range(n_p)]
        self.passage_node_keys = [compute_mdhash_id(t, "chunk-") for t in self.passage_texts]
        n_f = 0 if fact_emb_bits is None else fact_emb_bits.shape[0]
        self.facts = facts or [(f"s{i}", "rel", f"o{i}") for i in range(n_f)]
        self.fact_node_keys = [compute_mdhash_id(str(f), "fact-") for f in self.facts]
        self._arrays = dict(csr=csr, passage_vertex=np.asarray(passage_vertex, np.int32),
                            passage_emb=passage_emb_bits, fact_emb=fact_emb_bits,
                            subj=np.asarray(subj, np.int32), obj=np.asarray(obj, np.int32),
                            num_chunks=np.asarray(num_chunks, np.int32))
        return self

    # ------------------------------------------------------------------ HippoRAG.py:1287-1389
    def prepare_retrieval_objects(self):
        """Stage the index on the device.  After an incremental index() / delete() the embedding rows the old
        engine already holds are gathered device-side into the new matrices (hrag_engine_gather_embeddings):
        only the rows that are new cross PCIe, the graph (CSR -> SELL-8) is recompiled from the edge list."""
        from . import _lib
        from .engine import HippoRAGEngine
        if self._arrays is None:
            raise RuntimeError("nothing indexed yet")
        a = self._arrays
        self.query_to_embedding = {"triple": {}, "passage": {}}
        has_facts = a["fact_emb"] is not None and a["fact_emb"].shape[0] > 0
        pe, fe = a["passage_emb"], (a["fact_emb"] if has_facts else None)
        old, held = self.engine, getattr(self, "_engine_rows", None)
        same_kind = old is not None and old.f32_split == (a["passage_emb"].dtype == np.float32)
        if old is not None and held is not None and same_kind and old.dim == a["passage_emb"].shape[1]:
            def compose(which, keys, bits, held_keys):
                pos = {k: i for i, k in enumerate(held_keys)}
                src, fresh = [], []
                for i, k in enumerate(keys):
                    if k in pos:
                        src.append(pos[k])
                    else:
                        fresh.append(i)
                        src.append(-len(fresh))
                return old.gather_embeddings(which, np.asarray(src, np.int32), bits[fresh] if fresh else None)
            pe = compose("passages", self.passage_node_keys, a["passage_emb"], held["passages"])
            if has_facts and held["facts"]:
                fe = compose("facts", self.fact_node_keys, a["fact_emb"], held["facts"])
        self._drop_lexical()
        self._drop_payload()
        self._drop_late()
        if old is not None:
            # the gathered matrices no longer depend on the old engine: free its index before the new one is built
            # (peak device memory = one index + the embedding matrices, not two indexes)
            import torch
            torch.cuda.synchronize(old.device)
            old.close()
            self.engine = None
        def build(pe_, fe_):
            return HippoRAGEngine(a["csr"], a["passage_vertex"], pe_, fe_,
                                  a["subj"] if has_facts else None, a["obj"] if has_facts else None,
                                  a["num_chunks"] if has_facts else None,
                                  max_batch=self.global_config.max_batch,
                                  max_topk=max(1, min(self.global_config.retrieval_top_k, len(a["passage_vertex"]))),
                                  slab_width=self.global_config.slab_width,
                                  flags=_lib.OPT_ACCEL if self.global_config.ppr_accel else 0,
                                  locality=self.global_config.locality)
        try:
            engine = build(pe, fe)
        except Exception as exc:
            # the old engine is gone (closed above to keep the peak at ONE index): leave a consistent "not ready"
            # state -- the host arrays still hold the whole index, so the next prepare_retrieval_objects() rebuilds
            # from them -- and say what happened instead of serving from a half-built object
            self.engine, self._engine_rows, self.ready_to_retrieve = None, None, False
            raise RuntimeError("building the device index failed; the previous engine was already released (peak "
                               "memory = one index).  The retriever is NOT ready: free device memory (or lower "
                               "max_batch / use embedding_precision='bf16') and call prepare_retrieval_objects() "
                               f"again -- {type(exc).__name__}: {exc}") from exc
        if has_facts and self.proc_triples_to_docs and hasattr(engine, "set_fact_sources"):   # (test doubles lack it)
            engine.set_fact_sources(*self.fact_source_table())
        self.engine = engine
        self._engine_rows = {"passages": list(self.passage_node_keys), "facts": list(self.fact_node_keys) if has_facts else []}
        self.passage_node_idxs = a["passage_vertex"].tolist()
        if self.global_config.lexical_weight > 0:
            self._build_lexical()
        if self.global_config.payload_index:
            self._build_payload()
        if self.global_config.late_candidates is not None and self.token_encoder is not None:
            self._build_late()
        self.ready_to_retrieve = True

    # ------------------------------------------------------------------ payload filters
    def _drop_payload(self):
        ix = getattr(self, "payload_index", None)
        if ix is not None:
            if getattr(getattr(self, "engine", None), "_payload_index", None) is ix:
                self.engine.set_payload_index(None)
            ix.close()
        self.payload_index = None

    def payload_columns(self) -> dict:
        """The chunk metadata (source_id included) as columns over the passages, key -> one value (or None) per passage in
        passage_node_keys order: every key payload.encode_columns accepts.  A key whose values it rejects (str mixed with
        numbers, an unhashable value) is left out and stays with the host path."""
        from .payload import _encode_column
        meta = self.chunk_metadata
        rows = [meta.get(k, {}) for k in self.passage_node_keys]
        cols = {}
        for key in dict.fromkeys(k for m in rows for k in m):
            col = [m.get(key) for m in rows]
            try:
                _encode_column(key, col, len(rows))
            except ValueError:
                continue
            cols[key] = col
        return cols

    def _build_payload(self):
        """The payload index of the passages the mirror holds, on the engine's device.  prepare_retrieval_objects rebuilds
        it after index() / delete(), where the lexical model is rebuilt."""
        from .payload import PayloadIndex
        self._drop_payload()
        if self.passage_node_keys:
            self.payload_index = PayloadIndex.from_columns(self.payload_columns(), len(self.passage_node_keys),
                                                           device=self.engine.device.index)
            if hasattr(self.engine, "set_payload_index"):      # (boost= evaluates over it inside the engine's calls)
                self.engine.set_payload_index(self.payload_index)

    # ------------------------------------------------------------------ facets
    def facets(self, fields, doc_filter=None, limit: int = 10, **spec_kw) -> List[dict]:
        """What is in there (include/hrag.h, facets; needs RetrievalConfig.payload_index=True): for each metadata key of
        `fields` (a name or a list of names; "source_id" included) the number of passages per value, over the passages
        doc_filter allows -- what retrieve takes: one dict / bool array for every query, or a list with one per query; None:
        every passage.  spec_kw: compile_facet's edges= or lo= / n_values= for a number key.  One dict per query (one for a
        single filter): {field: {"values": [(label, count), ...] -- the `limit` largest, count descending --, "other",
        "missing", "total" (the allowed passages)}}."""
        if not self.global_config.payload_index:
            raise ValueError("facets needs RetrievalConfig.payload_index=True (the counts are taken over the chunk metadata as "
                             "typed columns on the device)")
        import torch
        from .facet import compile_facet, top_of
        self._ensure_ready()
        ix = self.payload_index
        if ix is None:
            raise ValueError("facets: the index holds no passages")
        names = [fields] if isinstance(fields, str) else list(fields)
        nq = len(doc_filter) if isinstance(doc_filter, list) else 1
        words = self._doc_filter_words(doc_filter, nq)
        if words is not None:
            words = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(ix.device)
        out = [{} for _ in range(nq)]
        for name in names:
            fc = ix.facet(compile_facet(ix, name, **spec_kw), words)
            raw = fc.raw.cpu().numpy()
            for q, top in enumerate(top_of(raw[:, :fc.spec.n_bins], fc.labels, limit)):
                out[q][name] = {"values": top, "other": int(raw[q, -2]), "missing": int(raw[q, -1]), "total": int(raw[q].sum())}
        return out

    # ------------------------------------------------------------------ late-interaction reranking
    def _drop_late(self):
        ix = getattr(self, "token_index", None)
        if ix is not None:
            if getattr(getattr(self, "engine", None), "_token_index", None) is ix:
                self.engine.set_token_index(None)
            ix.close()
        self.token_index = None

    def _build_late(self):
        """The token index of the passages the mirror holds: token_encoder.encode_tokens(texts, False) for the passages
        that are not in the per-passage cache yet (keyed like the passage texts, so index() encodes the new chunks only and
        delete() none), then a TokenIndex on the engine's device.  An engine without set_token_index (a test double) gets
        the cache only."""
        self._drop_late()
        keys, texts = self.passage_node_keys, self.passage_texts
        live = set(keys)
        for k in [k for k in self._token_cache if k not in live]:
            del self._token_cache[k]
        fresh = [i for i, k in enumerate(keys) if k not in self._token_cache]
        if fresh:
            toks = self.token_encoder.encode_tokens([texts[i] for i in fresh], False)
            if len(toks) != len(fresh):
                raise ValueError(f"token_encoder.encode_tokens returned {len(toks)} arrays for {len(fresh)} passages")
            for i, t in zip(fresh, toks):
                self._token_cache[keys[i]] = np.asarray(t, np.float32)
        if hasattr(self.engine, "set_token_index"):
            from .late import TokenIndex
            self.token_index = TokenIndex.from_ragged([self._token_cache[k] for k in keys], self.global_config.late_dtype,
                                                      self.engine.device.index)
            self.engine.set_token_index(self.token_index)

    def _late(self, late_candidates, who: str = "retrieve") -> dict:
        """The late arguments of a call as iter_batched_retrieve takes them: the argument, else
        RetrievalConfig.late_candidates; {} when off.  Builds the token index on first use."""
        c = self.global_config.late_candidates if late_candidates is None else late_candidates
        if c is None:
            return {}
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 1:
            raise ValueError(f"late_candidates={c!r}: an int >= 1 expected")
        if self.token_encoder is None:
            raise ValueError(f"{who}(late_candidates={c}) needs HippoRAG(token_encoder=...): an object with "
                             "encode_tokens(texts, is_query)")
        if getattr(self, "token_index", None) is None:     # (a test double's engine: the cache alone, nothing is re-encoded)
            self._build_late()
        dtype = self.global_config.late_dtype
        device = getattr(self.engine, "device", None)

        def encode(strings):
            from .late import LateQueries
            return LateQueries.from_ragged(self.token_encoder.encode_tokens(list(strings), True), dtype, device)
        return {"late_encode": encode, "late_candidates": int(c)}

    def _refuse_late(self, who: str, late_candidates=None) -> None:
        c = self.global_config.late_candidates if late_candidates is None else late_candidates
        if c is not None:
            raise ValueError(f"{who} does not serve late_candidates={c}: late reranking rescores one plain ranking per query "
                             "-- use retrieve(late_candidates=...)")

    @staticmethod
    def _late_metadata(solutions, first) -> None:
        """"late_score" and "first_score" into the metadata of every returned entry of a late call."""
        if first is None:
            return
        for s, f in zip(solutions, first):
            for d, x, y in zip(s.doc_metadata, s.doc_scores, f):
                d["late_score"], d["first_score"] = float(x), float(y)

    # ------------------------------------------------------------------ lexical retrieval
    def _drop_lexical(self):
        ix = getattr(self, "lexical_index", None)
        if ix is not None:
            ix.close()
        self.lexical_model = self.lexical_index = None

    def _build_lexical(self):
        """The BM25 model of the passages the mirror holds (lexical.LexicalModel: vocabulary, idf, weights) and its device
        index on the engine.  prepare_retrieval_objects rebuilds it after index() / delete(): idf and the average length
        move with the corpus.  An engine without set_lexical_index (a test double) gets the model only."""
        from .lexical import LexicalModel
        self._drop_lexical()
        self.lexical_model = LexicalModel(self.passage_texts, self.global_config.lexical_tokenize_fn)
        if hasattr(self.engine, "set_lexical_index"):
            from .engine import LexicalIndex
            self.lexical_index = LexicalIndex.from_postings(len(self.passage_texts), *self.lexical_model.postings(),
                                                            device=self.engine.device.index)
            self.engine.set_lexical_index(self.lexical_index)

    def _lexical(self, lexical_weight) -> dict:
        """The lexical arguments of a call as iter_batched_retrieve takes them: the argument, else
        RetrievalConfig.lexical_weight; {} at weight 0.  Builds the index on first use when the config did not ask for it."""
        from .engine import check_lexical_weight
        w = check_lexical_weight(self.global_config.lexical_weight if lexical_weight is None else lexical_weight)
        if w == 0:
            return {}
        if getattr(self, "lexical_model", None) is None:
            self._build_lexical()
        return {"lexical_encode": self.lexical_model.encode_queries, "lexical_weight": w}

    def _refuse_lexical(self, who: str, lexical_weight=None) -> None:
        w = self.global_config.lexical_weight if lexical_weight is None else lexical_weight
        if w not in (None, 0, 0.0):
            raise ValueError(f"{who} does not serve lexical_weight={w}: it fuses the score rows of plain member calls -- use "
                             "retrieve(lexical_weight=...)")

    # ------------------------------------------------------------------ recommend by example
    def _doc_positions(self, docs, who: str) -> List[int]:
        """The passage positions of document strings or chunk hash ids; an unknown document raises."""
        t = getattr(self, "_pos_table", None)
        if t is None or t[0] is not self.passage_node_keys or t[1] != len(self.passage_node_keys):
            table = {}
            for i, (key, text) in enumerate(zip(self.passage_node_keys, self.passage_texts)):
                table.setdefault(text, i)
                table[key] = i
            t = self._pos_table = (self.passage_node_keys, len(self.passage_node_keys), table)
        out = []
        for d in docs:
            if d not in t[2]:
                raise ValueError(f"{who}: unknown document {str(d)[:60]!r} (a passage string or a chunk hash id of the index "
                                 "expected)")
            out.append(t[2][d])
        return out

    def _examples(self, positive, negative, n_queries: Optional[int], who: str):
        """per-query lists of liked / disliked documents -> an engine Examples (None when both are None)"""
        from .reco import Examples
        if positive is None and negative is None:
            return None
        n = len(positive if positive is not None else negative) if n_queries is None else n_queries
        pos = [[] for _ in range(n)] if positive is None else list(positive)
        neg = [[] for _ in range(n)] if negative is None or len(negative) == 0 else list(negative)
        if len(pos) != n or len(neg) != n:
            raise ValueError(f"{who}: one list of documents per query expected ({len(pos)} liked and {len(neg)} disliked lists "
                             f"for {n} queries)")
        if any(isinstance(x, str) for x in pos + neg):
            raise ValueError(f"{who}: per-query LISTS of documents expected, not bare strings")
        device = getattr(self.engine, "device", None)
        return Examples.from_lists([self._doc_positions(x, who) for x in pos], [self._doc_positions(x, who) for x in neg],
                                   device=device)

    def _feedback(self, like, unlike, feedback_weight, n_queries: int) -> dict:
        """The keywords of relevance feedback for the batch pipeline ({} without examples or at weight 0)."""
        from .reco import check_feedback_weight, check_strategy
        ex = self._examples(like, unlike, n_queries, "retrieve(like=, unlike=)")
        if ex is None:
            return {}
        w = check_feedback_weight(self.global_config.feedback_weight if feedback_weight is None else feedback_weight)
        strategy = self.global_config.recommend_strategy
        if strategy == "average_vector":
            raise ValueError('retrieve(like=, unlike=) does not serve RetrievalConfig.recommend_strategy="average_vector": '
                             'relevance feedback blends score ROWS into the passage scores -- set "best_score" or '
                             '"sum_scores" (recommend() serves the query strategy)')
        check_strategy(strategy, True, "recommend_strategy")
        return {"feedback": ex, "feedback_weight": w, "feedback_strategy": strategy} if w > 0 else {}

    @staticmethod
    def _refuse_like(who: str, like, unlike) -> None:
        for name, v in (("like", like), ("unlike", unlike)):
            if v is not None:
                raise ValueError(f"{who} does not serve {name}: relevance feedback blends the recommend rows into the passage "
                                 "scores of one plain call -- use retrieve(like=..., unlike=...)")

    def recommend(self, positive, negative=(), num_to_retrieve: Optional[int] = None, strategy: Optional[str] = None,
                  doc_filter=None, exclude_examples: bool = True, mmr_lambda: Optional[float] = None):
        """Recommend by example (include/hrag.h): "more like these passages, less like those", no query string.  positive /
        negative: per-query lists of document strings or chunk hash ids (an unknown document raises); strategy (default
        RetrievalConfig.recommend_strategy): "best_score", "sum_scores" or "average_vector"; doc_filter as in retrieve();
        exclude_examples: the examples themselves are never returned; mmr_lambda as in retrieve().  Returns QuerySolutions
        whose question is None and whose entries carry "recommended": strategy in their metadata."""
        from .reco import check_strategy
        cfg = self.global_config
        self._ensure_ready()
        strategy = cfg.recommend_strategy if strategy is None else strategy
        check_strategy(strategy)
        ex = self._examples(positive, negative, None, "recommend")
        n_p = len(self.passage_node_keys)
        want = max(1, min(int(cfg.retrieval_top_k if num_to_retrieve is None else num_to_retrieve), n_p))
        if want > self.engine.max_topk:
            raise ValueError(f"recommend: num_to_retrieve={want} exceeds the engine's max_topk={self.engine.max_topk}")
        words = self._doc_filter_words(doc_filter, ex.batch)
        results: List[QuerySolution] = []
        for lo in range(0, ex.batch, self.engine.max_batch):
            b = min(self.engine.max_batch, ex.batch - lo)
            out = self.engine.recommend(ex.select(range(lo, lo + b)), k=want, strategy=strategy,
                                        doc_filter=None if words is None else scope_rows(words, lo, b),
                                        exclude_examples=exclude_examples, mmr_lambda=mmr_lambda)
            d_idx, d_sc = out[0].cpu().numpy(), out[1].cpu().numpy()
            rows = BatchRows((d_idx[i], d_sc[i], []) for i in range(b))
            rows.doc_idx = None                     # (entries of -1 are dropped one query at a time)
            sols = self._build_query_solutions([None] * b, rows, want)
            if mmr_lambda is not None:
                self._mmr_metadata(sols, out[2].cpu().numpy())
            for s_ in sols:
                for d in s_.doc_metadata:
                    d["recommended"] = strategy
            results.extend(sols)
        return results

    def _boost(self, boost, n_queries: int, who: str = "retrieve"):
        """None, or the BoostProgram of a call's boost= (default RetrievalConfig.boost): one list of items for every query
        or one list per query, compiled against the payload index (which _ensure_ready has built)."""
        b = self.global_config.boost if boost is None else boost
        if b is None:
            return None
        ix = getattr(self, "payload_index", None)
        if ix is None:
            raise ValueError(f"{who}: boost needs RetrievalConfig.payload_index=True (the boost terms read the chunk metadata "
                             "as typed columns on the device)")
        from .boost import check_program
        prog = check_program(ix, b, n_queries)
        return prog

    @staticmethod
    def _boost_metadata(solutions, prog) -> None:
        """"boosted": True into the metadata of every returned entry of a boosted call."""
        if prog is not None:
            for s in solutions:
                for d in s.doc_metadata or []:
                    d["boosted"] = True

    @staticmethod
    def _lexical_metadata(solutions, lex: dict) -> None:
        """"lexical_weight" into the metadata of every returned entry of a lexical call."""
        if lex:
            for s in solutions:
                for d in s.doc_metadata or []:
                    d["lexical_weight"] = lex["lexical_weight"]

    def fact_source_table(self):
        """The fact -> source-passage table of the scoped doc filter as a CSR in self.facts order: (row_ptr int64
        [n_facts + 1], passage positions int32) from proc_triples_to_docs (HippoRAG.py:1353-1361), positions in
        passage_node_keys order -- rebuilt from the dicts, so it follows delete()'s renumbering."""
        pos_of = {k: i for i, k in enumerate(self.passage_node_keys)}
        row_ptr = np.zeros(len(self.facts) + 1, np.int64)
        pos = []
        for f, fact in enumerate(self.facts):
            src = sorted(pos_of[k] for k in self.proc_triples_to_docs.get(fact, ()) if k in pos_of)
            pos.extend(src)
            row_ptr[f + 1] = len(pos)
        return row_ptr, np.asarray(pos, np.int32)

    # ------------------------------------------------------------------ HippoRAG.py:1391-1425
    def get_query_embeddings(self, queries: List):
        strings = []
        for q in queries:
            s = q.question if isinstance(q, QuerySolution) else q
            if s not in self.query_to_embedding["triple"] or s not in self.query_to_embedding["passage"]:
                strings.append(s)
        if strings:
            if self.embedding_model is None:
                raise ValueError("embedding_model is required to encode queries")
            for kind, method in (("triple", "query_to_fact"), ("passage", "query_to_passage")):   # :1414-1423
                embs = self.embedding_model.batch_encode(strings, instruction=get_query_instruction(method),
                                                         norm=True)
                for s, e in zip(strings, embs):
                    self.query_to_embedding[kind][s] = np.asarray(e, dtype=np.float32)

    def _q_tensor(self, queries: List[str], kind: str):
        import torch
        m = np.stack([np.asarray(self.query_to_embedding[kind][q], np.float32).reshape(-1) for q in queries])
        return torch.from_numpy(m).to(self.engine.device).to(self.engine.emb_dtype)

    # ------------------------------------------------------------------ per-method seams (B = 1)
    def get_fact_scores(self, query: str) -> np.ndarray:                  # :1427-1465
        self._ensure_ready()
        if len(self.fact_node_keys) == 0:
            return np.array([])
        self.get_query_embeddings([query])
        s = self.engine.sim_scores("facts", self._q_tensor([query], "triple"))[0].cpu().numpy()
        return min_max_normalize(s)

    def dense_passage_retrieval(self, query: str) -> Tuple[np.ndarray, np.ndarray]:   # :1467-1502
        self._ensure_ready()
        self.get_query_embeddings([query])
        s = self.engine.sim_scores("passages", self._q_tensor([query], "passage"))[0].cpu().numpy()
        s = min_max_normalize(s)
        ids = np.argsort(s, kind="stable")[::-1]
        return ids, s[ids]

    def run_ppr(self, reset_prob: np.ndarray, damping: float = 0.5) -> Tuple[np.ndarray, np.ndarray]:   # :1709-1749
        import torch
        self._ensure_ready()
        if damping is None:
            damping = 0.5
        r = torch.from_numpy(np.asarray(reset_prob, dtype=np.float32).reshape(1, -1))
        x, flags = self.engine.ppr(r, damping=damping, iters=self._ppr_iters(damping))
        if int(flags[0].item()) & 2:
            raise ValueError("reset vector has no positive entry")     # igraph raises here
        doc_scores = x[0].cpu().numpy()[self._arrays["passage_vertex"]]
        ids = np.argsort(doc_scores, kind="stable")[::-1]
        return ids, doc_scores[ids]

    def rerank_facts(self, query: str, query_fact_scores: np.ndarray):     # :1659-1707
        k = self.global_config.linking_top_k
        if len(query_fact_scores) == 0 or len(self.fact_node_keys) == 0:
            return [], [], {"facts_before_rerank": [], "facts_after_rerank": []}
        try:
            cand = np.argsort(query_fact_scores, kind="stable")[::-1][:k].tolist()
            cand_facts = [self.facts[i] for i in cand]
            idx, facts, _ = self.rerank_filter(query, cand_facts, cand, len_after_rerank=k)
            return list(idx), list(facts), {"facts_before_rerank": cand_facts, "facts_after_rerank": list(facts)}
        except Exception as exc:                                           # :1705-1707
            logger.error("Error in rerank_facts: %s", exc)
            return [], [], {"facts_before_rerank": [], "facts_after_rerank": [], "error": str(exc)}

    def _ensure_ready(self):
        if not self.ready_to_retrieve:
            self.prepare_retrieval_objects()

    def _ppr_iters(self, damping: Optional[float] = None) -> int:
        cfg = self.global_config
        return int(cfg.ppr_iters) if cfg.ppr_iters else sweeps_for_damping(cfg.damping if damping is None else damping)

    # ------------------------------------------------------------------ doc filter
    def _value_bits(self, key, value) -> np.ndarray:
        """Packed bitset of the passages whose metadata (source_id included) has `key` == `value`; built the first time
        it is asked for and cached until the passage list changes (_refresh_arrays)."""
        cache = self.__dict__.setdefault("_filter_cache", {})
        try:
            ck = (key, value)
            hit = cache.get(ck)
        except TypeError:                    # an unhashable value: matched, not cached
            ck, hit = None, None
        if hit is None:
            from .engine import pack_mask
            meta = self.chunk_metadata
            hit = pack_mask(np.fromiter((key in m and m[key] == value
                                         for m in (meta.get(k, {}) for k in self.passage_node_keys)),
                                        bool, len(self.passage_node_keys)))
            if ck is not None:
                cache[ck] = hit
        return hit

    def _filter_words(self, f) -> np.ndarray:
        """One query's filter (a metadata dict or a bool array in passage_node_keys order) -> packed uint32 [W]."""
        from .engine import pack_mask
        n = len(self.passage_node_keys)
        if isinstance(f, dict):
            words = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
            for key, values in f.items():               # keys: AND; the values of one key: OR
                self._refuse_operators(key, values)
                alts = values if isinstance(values, (list, tuple, set, frozenset)) else [values]
                any_of = np.zeros_like(words)
                for v in alts:
                    any_of |= self._value_bits(key, v)
                words &= any_of
            return words
        if isinstance(f, np.ndarray):
            if f.dtype != bool:
                raise TypeError(f"doc_filter array dtype {f.dtype}: a bool array over the passages is expected")
            if f.shape != (n,):
                raise ValueError(f"doc_filter array of shape {f.shape}: ({n},) expected (one entry per passage)")
            return pack_mask(f)
        raise TypeError(f"doc_filter of type {type(f).__name__}: a metadata dict, a bool numpy array, or a list of those")

    @staticmethod
    def _refuse_operators(key, values) -> None:
        """The host path matches equality only: a $ key or $ operator raises instead of silently matching nothing."""
        if (isinstance(key, str) and key.startswith("$")) or (
                isinstance(values, dict) and any(isinstance(k, str) and k.startswith("$") for k in values)):
            raise ValueError(f"doc_filter: {key!r}: the $ operators need RetrievalConfig.payload_index=True and a key its "
                             "columns hold (payload_columns); the host path matches equality only")

    def _payload_filter_words(self, filters: list, broadcast: bool) -> np.ndarray:
        """The words of dict / bool-array / None filters with the dicts evaluated on the device (one hrag_payload_filter
        call, one copy back): per query, the keys the payload index holds -- and $not / $any -- go into the clause program;
        the other keys (equality only) and a bool array go through the host path into the base row."""
        import torch
        ix = self.payload_index
        n = len(self.passage_node_keys)
        progs, base, any_base = [], np.full((len(filters), (n + 31) // 32), 0xFFFFFFFF, np.uint32), False
        for i, f in enumerate(filters):
            if not isinstance(f, dict):
                base[i] = self._filter_words(f)            # a bool array (or the TypeError of anything else)
                progs.append(None)
                any_base = True
                continue
            host = {k: v for k, v in f.items() if not (isinstance(k, str) and k.startswith("$")) and k not in ix.names}
            if host:
                base[i] = self._filter_words(host)          # (a $ operator on such a key raises there)
                any_base = True
            progs.append({k: v for k, v in f.items() if k not in host})
        from .payload import compile_filters
        pf = compile_filters(ix, progs[0] if broadcast else progs)
        and_with = None
        if any_base:
            and_with = torch.from_numpy((base[0] if broadcast else base).view(np.int32)).to(ix.device)
        words = ix.evaluate(pf, and_with=and_with)
        return np.ascontiguousarray(words.cpu().numpy()).view(np.uint32)

    def _doc_filter_words(self, doc_filter, n_queries: int) -> Optional[np.ndarray]:
        """doc_filter as the engine takes it: None, packed [W] (one filter for the batch, sent as one broadcast row) or
        [n_queries, W] (a list: one filter per query).  With RetrievalConfig.payload_index the metadata dicts are evaluated
        on the device (_payload_filter_words)."""
        if doc_filter is None:
            return None
        if isinstance(doc_filter, list) and len(doc_filter) != n_queries:
            raise ValueError(f"doc_filter list of {len(doc_filter)} entries for {n_queries} queries")
        if getattr(self, "payload_index", None) is not None:
            per = doc_filter if isinstance(doc_filter, list) else [doc_filter]
            if per and any(isinstance(f, dict) for f in per):
                return self._payload_filter_words(per, not isinstance(doc_filter, list))
        if isinstance(doc_filter, list):
            w = (len(self.passage_node_keys) + 31) // 32
            return (np.stack([self._filter_words(f) for f in doc_filter]) if doc_filter
                    else np.zeros((0, w), np.uint32))
        return self._filter_words(doc_filter)

    # ------------------------------------------------------------------ grouped retrieval
    def group_table(self, group_by):
        """The passage -> group table of grouped retrieval: (group_of int32 [n_passages], values, sizes).  group_by: a
        chunk-metadata key ("source_id" included, matched as the doc filter matches it) -- passages with equal values
        share a group, a passage without the key is a group of its own (value None) -- or an int array over
        passage_node_keys (equal entries share a group; the entry is the value).  Group ids are assigned in
        first-occurrence order of passage position.  Cached until the passage list changes."""
        n = len(self.passage_node_keys)
        if isinstance(group_by, str):
            cached = self.__dict__.get("_group_cache")
            if cached is not None and cached[0] == group_by:
                return cached[1]
            meta = self.chunk_metadata
            raw = [meta.get(k, {}).get(group_by, _NO_GROUP) if group_by in meta.get(k, {}) else _NO_GROUP
                   for k in self.passage_node_keys]
        elif isinstance(group_by, np.ndarray) or isinstance(group_by, (list, tuple)):
            arr = np.asarray(group_by)
            if arr.dtype.kind not in "iu":
                raise TypeError(f"group_by array dtype {arr.dtype}: an integer array over the passages is expected")
            if arr.shape != (n,):
                raise ValueError(f"group_by array of shape {arr.shape}: ({n},) expected (one entry per passage)")
            raw = arr.tolist()
        else:
            raise TypeError(f"group_by of type {type(group_by).__name__}: a metadata key or an int array over the passages")
        ids, values, group_of = {}, [], np.empty(n, np.int32)
        for p, v in enumerate(raw):
            try:
                key = ("v", v) if v is not _NO_GROUP else ("p", p)
                hash(key)
            except TypeError:                               # an unhashable metadata value: by its repr
                key = ("r", repr(v))
            if key not in ids:
                ids[key] = len(values)
                values.append(None if v is _NO_GROUP else v)
            group_of[p] = ids[key]
        table = (group_of, values, np.bincount(group_of, minlength=len(values)))
        if isinstance(group_by, str):
            self._group_cache = (group_by, table)
        return table

    def _grouping(self, group_by, group_agg):
        """(group_agg or None, table or None) of a call: the arguments, else RetrievalConfig.group_by / group_agg."""
        from .engine import check_group_agg
        cfg = self.global_config
        group_by = cfg.group_by if group_by is None else group_by
        if group_by is None:
            if group_agg is not None:
                raise ValueError("group_agg needs group_by (a metadata key or an int array over the passages)")
            return None, None
        agg = cfg.group_agg if group_agg is None else group_agg
        check_group_agg(agg)
        if agg is None:
            raise ValueError("group_agg must be 'max' or 'sum'")
        return agg, self.group_table(group_by)

    def _hits(self, group_hits, agg):
        """The group hits of a call: the argument, else RetrievalConfig.group_hits; only a grouped call has them."""
        from .engine import check_group_hits
        if agg is None:
            if group_hits is not None:
                raise ValueError("group_hits needs group_by (it asks for the best passages of each ranked group)")
            return None
        return check_group_hits(self.global_config.group_hits if group_hits is None else group_hits, agg)

    def _engine_groups(self, table):
        """The engine ranks by `table` from here on (set once per table: it is part of the device index)."""
        eng = self.engine
        if getattr(eng, "_group_table_id", None) is not table[0]:
            if not hasattr(eng, "set_passage_groups"):
                raise NotImplementedError(f"{type(eng).__name__} does not serve grouped retrieval")
            eng.set_passage_groups(table[0])
            eng._group_table_id = table[0]

    def _group_solutions(self, queries, rows, table, num_to_retrieve):
        """QuerySolutions of a grouped batch: per entry the representative passage, the group score and the passage's
        metadata plus {"group": value, "group_size": n}; with group hits also "group_hits": [{"doc", "score", "position"}],
        the group's best passages, best first (entry 0 is the representative)."""
        texts, keys = self._result_tables()
        _, values, sizes = table
        meta = self.chunk_metadata
        out = []
        for i, q in enumerate(queries):
            gi = np.asarray(rows.group_idx[i][:num_to_retrieve], np.int64)
            keep = gi >= 0
            gi, ids = gi[keep], np.asarray(rows.doc_idx[i][:num_to_retrieve], np.int64)[keep]
            md = [{**meta.get(k, {}), "group": values[g], "group_size": int(sizes[g])} for k, g in zip(keys[ids], gi)]
            if rows.hit_idx is not None:
                h_idx = np.asarray(rows.hit_idx[i][:num_to_retrieve], np.int64)[keep]
                h_sc = np.asarray(rows.hit_score[i][:num_to_retrieve])[keep]
                for d, pos, sc in zip(md, h_idx, h_sc):
                    d["group_hits"] = [{"doc": texts[p], "score": float(v), "position": int(p)}
                                       for p, v in zip(pos, sc) if p >= 0]
            out.append(QuerySolution(question=q, docs=texts[ids].tolist(),
                                     doc_scores=np.asarray(rows.doc_score[i][:len(ids)]), doc_metadata=md,
                                     graph_seeds=(rows[i][2] if len(rows) > i else None) or []))
        return out

    def _mmr(self, mmr_lambda, mmr_candidates) -> dict:
        """The MMR arguments of a call as iter_batched_retrieve / dense_retrieve take them: the arguments, else
        RetrievalConfig.mmr_lambda / mmr_candidates, else retrieval_top_k candidates; {} when off."""
        cfg = self.global_config
        lam = cfg.mmr_lambda if mmr_lambda is None else mmr_lambda
        cand = cfg.mmr_candidates if mmr_candidates is None else mmr_candidates
        if cand is None:
            from .engine import MMR_MAX_CANDIDATES
            cand = min(cfg.retrieval_top_k, MMR_MAX_CANDIDATES)
        if lam is None:
            if mmr_candidates is not None:
                raise ValueError("mmr_candidates needs mmr_lambda")
            return {}
        return {"mmr_lambda": lam, "mmr_candidates": cand}

    def _refuse_mmr(self, who: str, mmr_lambda, mmr_candidates) -> None:
        from .engine import refuse_mmr
        cfg = self.global_config
        refuse_mmr(who, {"mmr_lambda": cfg.mmr_lambda if mmr_lambda is None else mmr_lambda,
                         "mmr_candidates": mmr_candidates})

    @staticmethod
    def _mmr_metadata(solutions, values) -> None:
        """"mmr_value" into the metadata of every returned entry (the picks are a prefix: -1 only once they run out)."""
        if values is None:
            return
        for s, v in zip(solutions, values):
            for d, x in zip(s.doc_metadata, v):
                d["mmr_value"] = float(x)

    def _scope(self, filter_scope, doc_filter) -> str:
        """The doc filter's scope of a call: the argument, else RetrievalConfig.doc_filter_scope; "ranking" without a
        filter."""
        from .engine import FILTER_SCOPES
        scope = self.global_config.doc_filter_scope if filter_scope is None else filter_scope
        if scope not in FILTER_SCOPES:
            raise ValueError(f"filter_scope={scope!r}: one of {FILTER_SCOPES} expected")
        if scope == "seeds" and doc_filter is not None and self.fact_node_keys and not self.proc_triples_to_docs:
            raise ValueError('filter_scope="seeds" needs the facts\' source passages (proc_triples_to_docs): index with '
                             'index_from_openie')
        return "ranking" if doc_filter is None else scope

    @staticmethod
    def _filter_rows(doc_filter, rows):
        """The doc filter of a subset of the queries (retrieve_ircot's later steps)."""
        return [doc_filter[i] for i in rows] if isinstance(doc_filter, list) else doc_filter

    # ------------------------------------------------------------------ retrieve :413-499
    def retrieve(self, queries: List[str], num_to_retrieve: Optional[int] = None,
                 gold_docs: Optional[List[List[str]]] = None, doc_filter=None, filter_scope: Optional[str] = None,
                 group_by=None, group_agg: Optional[str] = None, group_hits: Optional[int] = None,
                 mmr_lambda: Optional[float] = None, mmr_candidates: Optional[int] = None,
                 lexical_weight: Optional[float] = None, boost=None, late_candidates: Optional[int] = None,
                 like=None, unlike=None, feedback_weight: Optional[float] = None):
        """like / unlike (include/hrag.h, recommend by example): per-query lists of documents (strings or chunk hash ids) the
        reader judged useful / off-topic; their recommend rows (RetrievalConfig.recommend_strategy) are blended into the
        passage scores that feed the passage prior at feedback_weight (default RetrievalConfig.feedback_weight), exactly as
        lexical_weight blends the BM25 rows -- not together with it, not with filter_scope="seeds".  The examples are not
        excluded: doc_filter decides.  Every entry's metadata then carries "feedback_weight".
        late_candidates (default RetrievalConfig.late_candidates; include/hrag.h, late-interaction reranking; needs
        token_encoder=): every query ranks max(late_candidates, num_to_retrieve) entries as below, the token vectors of the
        query string are scored against theirs by MaxSim on the device and the docs come in late order: doc_scores are the
        late scores and every entry's metadata carries "late_score" and "first_score".  Not with group_by or more documents
        than the engine's max_topk.
        boost (default RetrievalConfig.boost; include/hrag.h, boosted retrieval; needs payload_index=True): one list of
        boost items (boost.compile_boosts) for every query, or one list per query, or a BoostProgram: the scores become
        s * M + A over the chunk-metadata columns before they are ranked -- a recency decay, a trusted source, a penalty --
        and everything below ranks the boosted scores; every entry's metadata then carries "boosted": True.
        lexical_weight (default RetrievalConfig.lexical_weight; include/hrag.h, lexical retrieval): above 0, the passage
        scores that feed the passage prior and the DPR fallback are the dense ones blended at this weight with the BM25
        scores of the query strings against the passages (hipporag_amd.lexical); every entry's metadata then carries
        "lexical_weight".  Everything below composes with it except filter_scope="seeds".
        mmr_lambda / mmr_candidates (defaults RetrievalConfig.mmr_lambda / mmr_candidates; include/hrag.h, diversified
        retrieval): the docs come in MMR order over the first max(mmr_candidates, num_to_retrieve) ranked entries (mmr_candidates
        None: retrieval_top_k; never more than the passages or groups there are), doc_scores
        are their retrieval scores and every entry's metadata carries "mmr_value"; with group_by the candidates are the
        groups' best passages with the group scores.
        group_by / group_agg (defaults RetrievalConfig.group_by / group_agg): rank GROUPS of passages -- source
        documents -- instead of passages (group_table): num_to_retrieve counts groups, every entry is a group's best
        passage with the group's score and {"group", "group_size"} in its metadata.
        group_hits=m (default RetrievalConfig.group_hits; with group_by): every entry's metadata also carries "group_hits",
        the group's best m allowed passages as [{"doc", "score", "position"}], best first; docs / doc_scores are unchanged.
        doc_filter: limit the ranked documents to a subset of the corpus (a post-filter: scores do not change) --
        a metadata dict {key: value} or {key: [values]} (values of a key: any of them; keys: all of them; matched
        against the chunk metadata, source_id included), a bool numpy array over passage_node_keys, or a list with one
        of those per query.  Each query gets the first num_to_retrieve allowed documents of its unfiltered ranking.
        filter_scope (default RetrievalConfig.doc_filter_scope): "ranking" as above; "seeds" -- the facts that seed the
        graph search come from the allowed documents and the dense prior is normalised over them as well (one tenant's
        documents inside a shared index: the ranking no longer depends on the other tenants' documents)."""
        t_start = time.time()
        cfg = self.global_config
        if num_to_retrieve is None:
            num_to_retrieve = cfg.retrieval_top_k
        self._ensure_ready()
        scope = self._scope(filter_scope, doc_filter)
        words = self._doc_filter_words(doc_filter, len(queries))
        agg, table = self._grouping(group_by, group_agg)
        hits = self._hits(group_hits, agg)
        mmr = self._mmr(mmr_lambda, mmr_candidates)
        lex = self._lexical(lexical_weight)
        prog = self._boost(boost, len(queries))
        late = self._late(late_candidates)
        if late and agg is not None:
            raise ValueError("retrieve does not serve late_candidates with group_by: a group's score is not a passage's")
        fb = self._feedback(like, unlike, feedback_weight, len(queries))
        if fb and lex:
            raise ValueError("retrieve does not serve like / unlike together with lexical_weight > 0: both own the blend of "
                             "the passage scores")
        self.get_query_embeddings(queries)
        results: List[QuerySolution] = []
        self._retrieve_into(results, queries, num_to_retrieve, words, scope, agg, table, hits, mmr, lex, prog, late, fb)
        self.all_retrieval_time += time.time() - t_start
        logger.info("Total Retrieval Time %.2fs", self.all_retrieval_time)
        logger.info("Total Recognition Memory Time %.2fs", self.rerank_time)
        logger.info("Total PPR Time %.2fs", self.ppr_time)
        if gold_docs is not None:
            return results, self._recall(gold_docs, [r.docs for r in results])
        return results

    def _retrieve_into(self, results, queries, num_to_retrieve, doc_filter=None, filter_scope: str = "ranking",
                       group_agg=None, table=None, group_hits=None, mmr=None, lex=None, boost=None, late=None, fb=None):
        cfg = self.global_config
        extra = {} if doc_filter is None else {"doc_filter": doc_filter, "filter_scope": filter_scope}
        extra.update(mmr or {})
        extra.update(lex or {})
        extra.update(late or {})
        extra.update(fb or {})
        if boost is not None:
            extra["boost"] = boost
        if group_agg is not None:
            self._engine_groups(table)
            extra.update(group_agg=group_agg, group_of=table[0])
            if group_hits is not None:
                extra["group_hits"] = group_hits
        # batch by batch: the lists of document strings of one batch are built while the device works on the next
        for lo, rows in iter_batched_retrieve(self.engine, queries, self._q_tensor, self.facts if self.fact_node_keys else [],
                                              self.rerank_filter, linking_top_k=cfg.linking_top_k, damping=cfg.damping,
                                              passage_node_weight=cfg.passage_node_weight, ppr_iters=self._ppr_iters(),
                                              ppr_tol=cfg.ppr_tol, ppr_max_iters=cfg.ppr_max_iters,
                                              ppr_base_iters_narrow=cfg.ppr_base_iters_narrow,
                                              num_to_retrieve=num_to_retrieve, n_passages=len(self.passage_node_keys),
                                              timers=self, **extra):
            with gc_paused():       # around the materialisation only: the filter (an LLM call in production) runs outside
                if group_agg is not None:
                    sols = self._group_solutions(queries[lo: lo + len(rows)], rows, table, num_to_retrieve)
                else:
                    sols = self._build_query_solutions(queries[lo: lo + len(rows)], rows, num_to_retrieve)
                self._mmr_metadata(sols, getattr(rows, "mmr_value", None))
                self._lexical_metadata(sols, lex)
                self._boost_metadata(sols, boost)
                self._late_metadata(sols, getattr(rows, "first_score", None))
                if fb:
                    for s_ in sols:
                        for d in s_.doc_metadata:
                            d["feedback_weight"] = fb["feedback_weight"]
                results.extend(sols)

    # ------------------------------------------------------------------ fused retrieval
    def retrieve_fused(self, questions: List[List[str]], weights=None, fuse: str = "rrf", rrf_c: int = 60,
                       rrf_depth: Optional[int] = None, num_to_retrieve: Optional[int] = None, doc_filter=None,
                       filter_scope: Optional[str] = None, group_by=None, group_agg: Optional[str] = None,
                       group_hits: Optional[int] = None, mmr_lambda: Optional[float] = None,
                       mmr_candidates: Optional[int] = None, boost=None, late_candidates: Optional[int] = None,
                       like=None, unlike=None):
        """One ranked list per QUESTION, each question given as several sub-queries -- a decomposition, paraphrases, the
        thoughts of an IRCoT chain (include/hrag.h, fused retrieval).  Every sub-query runs phase A and phase B as in
        retrieve(); the score rows of a question's sub-queries are fused ON THE DEVICE over all passages -- fuse="sum"
        (weighted, fp64), "max" (what retrieve_ircot merges by, over every passage instead of the returned lists) or "rrf"
        (reciprocal rank fusion, constant rrf_c, lists of rrf_depth entries: default num_to_retrieve) -- and the fused rows
        are ranked like any other: doc_filter (one per QUESTION), filter_scope, group_by / group_agg / group_hits as in
        retrieve().  weights: one list per question (or a flat array over all sub-queries), finite and >= 0, not with
        "max".  Returns one QuerySolution per question; its `question` is the question's first sub-query.  A question's
        sub-queries share one device batch: at most max_batch of them."""
        from .engine import check_fuse
        self._refuse_mmr("retrieve_fused", mmr_lambda, mmr_candidates)
        self._refuse_late("retrieve_fused", late_candidates)
        self._refuse_like("retrieve_fused", like, unlike)
        self._refuse_lexical("retrieve_fused")
        if boost is not None or self.global_config.boost is not None:
            raise ValueError("retrieve_fused does not serve boost: it fuses the score rows of plain member calls -- use "
                             "retrieve(boost=...), or HippoRAGEngine.last_fused(boost=...)")
        t_start = time.time()
        cfg = self.global_config
        if num_to_retrieve is None:
            num_to_retrieve = cfg.retrieval_top_k
        if not isinstance(questions, (list, tuple)) or any(
                not isinstance(q, (list, tuple)) or not q or not all(isinstance(s, str) for s in q) for q in questions):
            raise ValueError("questions: a list of non-empty lists of strings (the sub-queries of each question) expected")
        sizes = np.asarray([len(q) for q in questions], np.int64)
        member_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        flat = [s for q in questions for s in q]
        w_flat = None
        if weights is not None:
            if len(weights) == len(questions) and all(np.ndim(w) == 1 for w in weights):
                if [len(w) for w in weights] != sizes.tolist():
                    raise ValueError("weights: one weight per sub-query of every question expected")
                w_flat = np.concatenate([np.asarray(w, np.float32) for w in weights]) if questions else np.zeros(0, np.float32)
            else:
                w_flat = np.asarray(weights, np.float32)
        if not questions:
            return []
        depth = num_to_retrieve if rrf_depth is None else rrf_depth
        check_fuse(fuse, member_ptr, len(flat), w_flat, rrf_c, max(1, depth) if rrf_depth is None else depth)
        self._ensure_ready()
        eng = self.engine
        if not hasattr(eng, "last_fused"):
            raise NotImplementedError(f"{type(eng).__name__} does not serve fuse: the fusion works on the score rows of one "
                                      "unsharded engine handle")
        if int(sizes.max()) > eng.max_batch:
            raise ValueError(f"a question of {int(sizes.max())} sub-queries exceeds max_batch={eng.max_batch}")
        n_p = len(self.passage_node_keys)
        dmax = min(eng.max_topk, n_p)
        if fuse == "rrf":
            if rrf_depth is not None and not 1 <= depth <= dmax:
                raise ValueError(f"rrf_depth={rrf_depth}: outside [1, min(max_topk, n_passages) = {dmax}]")
            depth = max(1, min(depth, dmax))
        scope = self._scope(filter_scope, doc_filter)
        words = self._doc_filter_words(doc_filter, len(questions))
        agg, table = self._grouping(group_by, group_agg)
        hits = self._hits(group_hits, agg)
        if agg is not None:
            self._engine_groups(table)
        want = max(1, min(int(num_to_retrieve), n_p if agg is None else int(np.max(table[0])) + 1))
        k_docs = min(want, eng.max_topk)
        self.get_query_embeddings(flat)
        # whole questions per device batch
        chunks, lo = [], 0
        while lo < len(questions):
            hi = lo + 1
            while hi < len(questions) and member_ptr[hi + 1] - member_ptr[lo] <= eng.max_batch:
                hi += 1
            chunks.append((lo, hi))
            lo = hi
        results: List[QuerySolution] = []
        import torch
        for lo, hi in chunks:
            m0, m1 = int(member_ptr[lo]), int(member_ptr[hi])
            mp = member_ptr[lo: hi + 1] - m0
            q_words = None if words is None else (words if words.ndim == 1 else words[lo:hi])
            extra = {}
            if words is not None:       # the member runs: every sub-query under its question's filter
                extra = {"doc_filter": words if words.ndim == 1 else np.repeat(words[lo:hi], sizes[lo:hi], axis=0),
                         "filter_scope": scope}
            (_, rows), = iter_batched_retrieve(eng, flat[m0:m1], self._q_tensor, self.facts if self.fact_node_keys else [],
                                               self.rerank_filter, linking_top_k=cfg.linking_top_k, damping=cfg.damping,
                                               passage_node_weight=cfg.passage_node_weight, ppr_iters=self._ppr_iters(),
                                               ppr_tol=cfg.ppr_tol, ppr_max_iters=cfg.ppr_max_iters,
                                               ppr_base_iters_narrow=cfg.ppr_base_iters_narrow, num_to_retrieve=1,
                                               n_passages=n_p, timers=self, keep_all_scores=True, **extra)
            w = None if w_flat is None else w_flat[m0:m1]
            fused_rows = BatchRows()
            if rows.repeated or k_docs < want:
                # the contract ran some sub-queries again (the engine's rows are no longer this batch's), or more documents
                # are wanted than the device ranks: the host form over the batch's score rows
                allowed = None if q_words is None else unpack_mask(q_words, n_p)
                fused = fuse_rows_host(rows.all_scores.cpu().numpy(), mp, fuse, w, rrf_c, depth, allowed)
                if agg is not None:
                    fused_rows.group_idx, fused_rows.doc_score, fused_rows.doc_idx, *h = group_rank_rows(
                        fused, table[0], allowed, want, agg, hits)
                    if h:
                        fused_rows.hit_idx, fused_rows.hit_score = h
                else:
                    fused_rows.doc_idx, fused_rows.doc_score = rank_allowed(
                        fused, np.ones(n_p, bool) if allowed is None else allowed, want)
                    fused_rows.doc_score = fused_rows.doc_score + np.float32(0)
            else:
                flt = None if q_words is None else torch.from_numpy(np.ascontiguousarray(q_words).view(np.int32))
                out = eng.last_fused(mp, weights=w, fuse=fuse, rrf_c=rrf_c, rrf_depth=depth if fuse == "rrf" else None,
                                     k=k_docs, doc_filter=flt, group_agg=agg, group_hits=hits)
                fused_rows.doc_idx, fused_rows.doc_score = out.doc_idx.cpu().numpy(), out.doc_score.cpu().numpy()
                if agg is not None:
                    fused_rows.group_idx = out.group_idx.cpu().numpy()
                if hits is not None:
                    fused_rows.hit_idx, fused_rows.hit_score = out.hit_idx.cpu().numpy(), out.hit_score.cpu().numpy()
            for j in range(hi - lo):
                seeds = [f for i in range(int(mp[j]), int(mp[j + 1])) for f in (rows[i][2] or [])]
                fused_rows.append((fused_rows.doc_idx[j], fused_rows.doc_score[j], seeds))
            firsts = [q[0] for q in questions[lo:hi]]
            with gc_paused():
                results.extend(self._group_solutions(firsts, fused_rows, table, num_to_retrieve) if agg is not None
                               else self._build_query_solutions(firsts, fused_rows, num_to_retrieve))
        self.all_retrieval_time += time.time() - t_start
        return results

    # ------------------------------------------------------------------ retrieve_ircot :509-558
    def retrieve_ircot(self, queries: List[str], max_qa_steps: int, num_to_retrieve: Optional[int] = None,
                       gold_docs: Optional[List[List[str]]] = None, reason_fn: Optional[Callable] = None,
                       doc_filter=None, filter_scope: Optional[str] = None, group_by=None,
                       group_agg: Optional[str] = None, mmr_lambda: Optional[float] = None,
                       mmr_candidates: Optional[int] = None, lexical_weight: Optional[float] = None, boost=None,
                       late_candidates: Optional[int] = None, like=None, unlike=None):
        """Iterative retrieval: alternate retrieval and one reasoning step per query, merging the document
        scores by max (:526-543).  reason_fn(query, ranked_docs, thoughts) -> str stands for
        utils/qa_utils.reason_step (the IRCoT prompt + reader LLM are outside this package).  The reference
        walks the queries one by one and retrieves with a batch of one per step; queries are independent, so
        here every step retrieves for ALL still-active queries in one batched device call -- same result per
        query, batch kernels instead of 2 * max_qa_steps single-query passes.  lexical_weight (default
        RetrievalConfig.lexical_weight): every step's retrieve() takes it, the thoughts being the query strings.  boost
        (default RetrievalConfig.boost): every step's retrieve() takes it, a per-query one cut to the step's queries."""
        self._refuse_mmr("retrieve_ircot", mmr_lambda, mmr_candidates)
        self._refuse_late("retrieve_ircot", late_candidates)
        self._refuse_like("retrieve_ircot", like, unlike)
        if max_qa_steps < 1:
            raise ValueError("max_qa_steps must be at least 1.")
        if max_qa_steps > 1 and reason_fn is None:
            raise ValueError("retrieve_ircot with max_qa_steps > 1 needs a reason_fn (the reader LLM is outside this package)")
        if num_to_retrieve is None:
            num_to_retrieve = self.global_config.retrieval_top_k
        self._ensure_ready()
        prog = self._boost(boost, len(queries), "retrieve_ircot")
        first = self.retrieve(list(queries), num_to_retrieve=num_to_retrieve, doc_filter=doc_filter,
                              filter_scope=filter_scope, group_by=group_by, group_agg=group_agg,
                              lexical_weight=lexical_weight, boost=prog)
        merged = [dict(zip(r.docs, r.doc_scores.tolist())) for r in first]
        meta = [dict(zip(r.docs, r.doc_metadata or [])) for r in first]
        thoughts: List[List[str]] = [[] for _ in queries]
        active = list(range(len(queries)))
        for _ in range(1, max_qa_steps):
            step_q, step_i = [], []
            for i in active:
                ranked = sorted(merged[i], key=merged[i].get, reverse=True)
                thought = reason_fn(queries[i], ranked[:num_to_retrieve], thoughts[i])
                if not isinstance(thought, str):
                    raise TypeError(f"IRCoT reasoning expected a string response, got {type(thought).__name__}.")
                thoughts[i].append(thought)
                if "So the answer is:" in thought:
                    continue
                step_q.append(thought)
                step_i.append(i)
            if not step_q:
                break
            for i, r in zip(step_i, self.retrieve(step_q, num_to_retrieve=num_to_retrieve,
                                                  doc_filter=self._filter_rows(doc_filter, step_i),
                                                  filter_scope=filter_scope, group_by=group_by, group_agg=group_agg,
                                                  lexical_weight=lexical_weight,
                                                  boost=None if prog is None else prog.select(step_i))):
                for doc, score in zip(r.docs, r.doc_scores.tolist()):
                    merged[i][doc] = max(merged[i].get(doc, float("-inf")), score)
                meta[i].update(dict(zip(r.docs, r.doc_metadata or [])))
            active = step_i
        results = []
        for i, q in enumerate(queries):
            items = sorted(merged[i].items(), key=lambda kv: kv[1], reverse=True)
            results.append(QuerySolution(question=q, docs=[d for d, _ in items],
                                         doc_scores=np.asarray([s for _, s in items]), thoughts=thoughts[i],
                                         doc_metadata=[meta[i].get(d, {}) for d, _ in items]))
        if gold_docs is not None:
            return results, self._recall(gold_docs, [r.docs for r in results])
        return results

    def _result_tables(self):
        """passage texts / keys as numpy object arrays: a batch materialises B x num_to_retrieve document strings
        (HippoRAG.py:501-507 returns them as lists), which one fancy index per query does ~5x faster than a list
        comprehension.  Rebuilt when index() appended or delete() replaced the lists."""
        t = getattr(self, "_tables", None)
        if t is None or t[0] is not self.passage_texts or t[1] != len(self.passage_texts):
            texts = np.empty(len(self.passage_texts), dtype=object)
            texts[:] = self.passage_texts
            keys = np.empty(len(self.passage_node_keys), dtype=object)
            keys[:] = self.passage_node_keys
            t = self._tables = (self.passage_texts, len(self.passage_texts), texts, keys)
        return t[2], t[3]

    def _build_query_solutions(self, queries, rows, num_to_retrieve) -> List[QuerySolution]:
        """_build_retrieval_result + the QuerySolution of retrieve() (:471-480) for one batch.  When every query of the
        batch has a full list of valid ids (the usual case) and there is no chunk metadata, the document strings of the
        whole batch come from ONE fancy index into the text table."""
        ids = None if rows.doc_idx is None else np.asarray(rows.doc_idx)[:, :num_to_retrieve]
        if ids is None or self.chunk_metadata or ids.size == 0 or int(ids.min()) < 0:
            out = []
            for q, (d_idx, d_sc, seeds) in zip(queries, rows):
                r = self._build_retrieval_result(q, d_idx, d_sc, num_to_retrieve, seeds)
                out.append(QuerySolution(question=r.query, docs=r.docs, doc_scores=r.scores,
                                         doc_metadata=r.doc_metadata, graph_seeds=r.graph_seeds))
            return out
        texts, _ = self._result_tables()
        docs = texts[ids].tolist()
        n = ids.shape[1]
        return [QuerySolution(question=q, docs=docs[i], doc_scores=np.asarray(rows[i][1][:n]),
                              doc_metadata=[{} for _ in range(n)], graph_seeds=rows[i][2] or [])
                for i, q in enumerate(queries)]

    def _build_retrieval_result(self, query, sorted_doc_ids, sorted_doc_scores, num_to_retrieve, graph_seeds=None):
        ids = np.asarray(sorted_doc_ids[:num_to_retrieve], dtype=np.int64)                  # :501-507
        ids = ids[ids >= 0]
        texts, keys = self._result_tables()
        meta = self.chunk_metadata
        return RetrievalResult(query=query, docs=texts[ids].tolist(),
                               scores=np.asarray(sorted_doc_scores[:len(ids)]),
                               doc_metadata=([dict(meta.get(k, {})) for k in keys[ids]] if meta
                                             else [{} for _ in range(len(ids))]),
                               graph_seeds=graph_seeds or [])

    # ------------------------------------------------------------------ retrieve_dpr :665-732
    def retrieve_dpr(self, queries: List[str], num_to_retrieve: Optional[int] = None,
                     gold_docs: Optional[List[List[str]]] = None, doc_filter=None, filter_scope: Optional[str] = None,
                     group_by=None, group_agg: Optional[str] = None, group_hits: Optional[int] = None,
                     mmr_lambda: Optional[float] = None, mmr_candidates: Optional[int] = None,
                     lexical_weight: Optional[float] = None, boost=None, late_candidates: Optional[int] = None,
                     like=None, unlike=None):
        """late_candidates: as in retrieve(), over the dense ranking; then not with group_by, lexical_weight, boost or more
        documents than the engine's max_topk (ValueError naming late_candidates).
        Dense retrieval; doc_filter / filter_scope as in retrieve() ("seeds": the scores are normalised over the
        allowed passages); group_by / group_agg / group_hits as in retrieve(), over the normalised dense scores;
        mmr_lambda / mmr_candidates as in retrieve(), over the dense ranking.
        lexical_weight (default RetrievalConfig.lexical_weight) above 0: the ranking of the dense scores blended with the
        BM25 scores of the query strings (HippoRAGEngine.dense_retrieve(lexical=)); then not with group_by, mmr_lambda,
        filter_scope="seeds" or more documents than the engine's max_topk (ValueError naming lexical_weight).
        boost (default RetrievalConfig.boost): the ranking of the boosted min-max scores
        (HippoRAGEngine.dense_retrieve(boost=)); then not with group_by, mmr_lambda, lexical_weight, filter_scope="seeds" or
        more documents than the engine's max_topk (ValueError naming boost).
        like / unlike are refused by name: use retrieve(), or recommend()."""
        self._refuse_like("retrieve_dpr", like, unlike)
        cfg = self.global_config
        if num_to_retrieve is None:
            num_to_retrieve = cfg.retrieval_top_k
        self._ensure_ready()
        scope = self._scope(filter_scope, doc_filter)
        words = self._doc_filter_words(doc_filter, len(queries))
        agg, table = self._grouping(group_by, group_agg)
        hits = self._hits(group_hits, agg)
        import torch
        self.get_query_embeddings(queries)
        eng = self.engine
        want = max(1, min(num_to_retrieve, len(self.passage_node_keys)))
        if agg is not None:
            self._engine_groups(table)
            want = min(want, len(table[1]))
        k_docs = min(want, eng.max_topk)
        # more documents than the device top-k holds (:704-714 slices any prefix of the full ranking): the raw scores of all
        # passages come back and are normalised and ranked here with the library's rule (score desc, larger index first)
        beyond = k_docs < want
        from .engine import host_copy_async, host_wait
        results = []
        mmr = self._mmr(mmr_lambda, mmr_candidates)
        if mmr:
            from .engine import MMR_MAX_CANDIDATES, mmr_plan
            lam, c = mmr_plan(mmr["mmr_lambda"], mmr_pool(mmr["mmr_candidates"], want, len(self.passage_node_keys)
                                                          if agg is None else len(table[1])), want)
            if c > eng.max_topk:
                raise ValueError(f"mmr_candidates={c} (at least num_to_retrieve) exceeds the engine's max_topk={eng.max_topk}: "
                                 f"MMR picks from one device ranking of at most min({MMR_MAX_CANDIDATES}, max_topk) entries")
            mmr = {"mmr_lambda": lam, "mmr_candidates": c}
        lex = self._lexical(lexical_weight)
        if lex:
            for name, on in (("group_by", agg is not None), ("mmr_lambda", bool(mmr)), ('filter_scope="seeds"', scope == "seeds"),
                             (f"num_to_retrieve above max_topk={eng.max_topk}", beyond)):
                if on:
                    raise ValueError(f"retrieve_dpr does not serve lexical_weight={lex['lexical_weight']} with {name}: the "
                                     "blended rows are ranked once on the device -- use retrieve(lexical_weight=...)")

        prog = self._boost(boost, len(queries), "retrieve_dpr")
        if prog is not None:
            for name, on in (("group_by", agg is not None), ("mmr_lambda", bool(mmr)), ("lexical_weight", bool(lex)),
                             ('filter_scope="seeds"', scope == "seeds"),
                             (f"num_to_retrieve above max_topk={eng.max_topk}", beyond)):
                if on:
                    raise ValueError(f"retrieve_dpr does not serve boost with {name}: the boosted rows are ranked once on the "
                                     "device -- use retrieve(boost=...)")

        late = self._late(late_candidates, "retrieve_dpr")
        if late:
            from .late import LATE_MAX_CANDIDATES
            late_c = min(max(late["late_candidates"], want), len(self.passage_node_keys))
            for name, on in (("group_by", agg is not None), ("lexical_weight", bool(lex)), ("boost", prog is not None),
                             (f"num_to_retrieve above max_topk={eng.max_topk}", beyond),
                             (f"more than min({LATE_MAX_CANDIDATES}, max_topk={eng.max_topk}) candidates",
                              late_c > min(eng.max_topk, LATE_MAX_CANDIDATES))):
                if on:
                    raise ValueError(f"retrieve_dpr does not serve late_candidates={late_c} with {name}: late reranking "
                                     "rescores one plain device ranking of passages")

        def rows_of(lo, b):                 # the packed filter rows of queries [lo, lo + b)
            return words if words.ndim == 1 else words[lo: lo + b]

        def enqueue(lo):
            qs = queries[lo: lo + eng.max_batch]
            if beyond:
                return qs, host_copy_async(eng.sim_scores("passages", self._q_tensor(qs, "passage"))), None
            extra = {} if words is None else {
                "doc_filter": torch.from_numpy(np.ascontiguousarray(rows_of(lo, len(qs))).view(np.int32)),
                "filter_scope": scope}
            if agg is not None:
                if hits is not None:
                    extra["group_hits"] = hits
                gi, sc, idx, *h = eng.dense_retrieve(self._q_tensor(qs, "passage"), k=k_docs, group_agg=agg, **extra, **mmr)
                return (qs, host_copy_async(idx), host_copy_async(sc), host_copy_async(gi)) + tuple(map(host_copy_async, h))
            if lex:
                extra.update(lexical=lex["lexical_encode"](qs), lexical_weight=lex["lexical_weight"])
            if prog is not None:
                extra["boost"] = prog.select(range(lo, lo + len(qs)))
            if late:                        # (MMR then picks among the rescored entries: no mmr_candidates)
                extra.update(late=late["late_encode"](qs), late_candidates=late_c)
                idx, sc, *h = eng.dense_retrieve(self._q_tensor(qs, "passage"), k=k_docs, **extra,
                                                 **({"mmr_lambda": mmr["mmr_lambda"]} if mmr else {}))
                return (qs, host_copy_async(idx), host_copy_async(sc), None) + tuple(map(host_copy_async, h))
            idx, sc, *h = eng.dense_retrieve(self._q_tensor(qs, "passage"), k=k_docs, **extra, **mmr)
            return (qs, host_copy_async(idx), host_copy_async(sc)) + ((None,) + tuple(map(host_copy_async, h)) if h else ())

        # one batch ahead of the host, like retrieve(): batch i's lists are built while the device scores batch i + 1
        starts = list(range(0, len(queries), eng.max_batch))
        pending = enqueue(starts[0]) if starts else None
        for n in range(len(starts)):
            qs, idx_h, sc_h, *gi_h = pending
            pending = enqueue(starts[n + 1]) if n + 1 < len(starts) else None
            gi = h_idx = h_sc = values = first_sc = None
            if beyond:
                raw = host_wait(idx_h)[:, :len(self.passage_node_keys)]
                if scope == "seeds":
                    full = masked_minmax_rows(raw, unpack_mask(rows_of(starts[n], len(qs)), raw.shape[1]))
                else:
                    full = np.stack([min_max_normalize(r) for r in raw]).astype(np.float32)
                if agg is not None:
                    gi, sc, idx, *h = group_rank_rows(full, table[0], None if words is None else
                                                      unpack_mask(rows_of(starts[n], len(qs)), full.shape[1]), want, agg,
                                                      hits)
                    if h:
                        h_idx, h_sc = h
                elif words is not None:
                    idx, sc = rank_allowed(full, unpack_mask(rows_of(starts[n], len(qs)), full.shape[1]), want)
                else:
                    idx = np.stack([np.argsort(r, kind="stable")[::-1][:want] for r in full]).astype(np.int32)
                    sc = np.take_along_axis(full, idx.astype(np.int64), axis=1)
            else:
                idx, sc = host_wait(idx_h).copy(), host_wait(sc_h).copy()
                if late:                    # dense_retrieve's tuple ends with first_score
                    first_sc = host_wait(gi_h[-1]).copy()
                    gi_h = gi_h[:-1]
                if mmr:                     # ... and, before it, with mmr_value
                    values = host_wait(gi_h[-1]).copy()
                    gi_h = gi_h[:-1]
                gi = host_wait(gi_h[0]).copy() if gi_h and gi_h[0] is not None else None
                if len(gi_h) == 3:
                    h_idx, h_sc = host_wait(gi_h[1]).copy(), host_wait(gi_h[2]).copy()
            first = len(results)
            if agg is not None:
                rows = BatchRows([(idx[i], sc[i], None) for i in range(len(qs))])
                rows.doc_idx, rows.doc_score, rows.group_idx = idx, sc, gi
                rows.hit_idx, rows.hit_score = h_idx, h_sc
                results.extend(self._group_solutions(qs, rows, table, num_to_retrieve))
                self._mmr_metadata(results[first:], values)
                continue
            with gc_paused():
                for i, q in enumerate(qs):
                    r = self._build_retrieval_result(q, idx[i], sc[i], num_to_retrieve)
                    results.append(QuerySolution(question=r.query, docs=r.docs, doc_scores=r.scores,
                                                 doc_metadata=r.doc_metadata))
            self._mmr_metadata(results[first:], values)
            self._lexical_metadata(results[first:], lex)
            self._boost_metadata(results[first:], prog)
            self._late_metadata(results[first:], first_sc)
        if gold_docs is not None:
            return results, self._recall(gold_docs, [r.docs for r in results])
        return results

    # ------------------------------------------------------------------ rag_qa :591-663
    def rag_qa(self, queries, gold_docs: Optional[List[List[str]]] = None,
               gold_answers: Optional[List[List[str]]] = None, doc_filter=None, filter_scope: Optional[str] = None,
               lexical_weight: Optional[float] = None, boost=None, late_candidates: Optional[int] = None):
        if self.qa_fn is None:
            raise NotImplementedError("rag_qa needs a qa_fn (the reader LLM is outside this package)")
        retrieval_metrics = None
        if not isinstance(queries[0], QuerySolution):
            out = self.retrieve(queries=queries, gold_docs=gold_docs, doc_filter=doc_filter, filter_scope=filter_scope,
                                lexical_weight=lexical_weight, boost=boost, late_candidates=late_candidates)
            queries, retrieval_metrics = out if gold_docs is not None else (out, None)
        solutions, messages, metadata = self.qa_fn(queries)
        if gold_answers is not None:
            for s, g in zip(solutions, gold_answers):
                s.gold_answers = list(g)
        if gold_docs is not None:
            for s, g in zip(solutions, gold_docs):
                s.gold_docs = g
            return solutions, messages, metadata, retrieval_metrics, None
        return solutions, messages, metadata

    @staticmethod
    def _recall(gold_docs, retrieved_docs, k_list=(1, 2, 5, 10, 20, 30, 50, 100, 150, 200)):
        """RetrievalRecall.calculate_metric_scores (evaluation/retrieval_eval.py:16-73), pooled only."""
        out = {}
        for k in k_list:
            vals = []
            for gold, got in zip(gold_docs, retrieved_docs):
                gold_set = set(gold)
                vals.append(len(gold_set & set(got[:k])) / len(gold_set) if gold_set else 0.0)
            out[f"Recall@{k}"] = round(float(np.mean(vals)) if vals else 0.0, 4)
        return out
