"""Index-time host code of lexical retrieval (include/hrag.h, lexical retrieval): tokenizer, vocabulary, BM25 weights and
the query encoder.  Pure numpy -- the device side (engine.LexicalIndex, hrag_lex_scores) scores whatever weights it is
given and knows nothing of BM25; this module is one way to make them."""

from __future__ import annotations

import math
import re
from typing import Callable, List, Optional, Sequence

import numpy as np

from ._lib import LEX_MAX_QUERY_TERMS

_WORD = re.compile(r"\w+")


def default_tokenize(text: str) -> List[str]:
    """Lower-case, then every run of word characters (\\w+).  No stemming, no stop words."""
    return _WORD.findall(str(text).lower())


class Vocabulary:
    """Token -> dense term id, in order of first appearance."""

    def __init__(self):
        self.id_of = {}
        self.tokens: List[str] = []

    def add(self, token) -> int:
        i = self.id_of.get(token)
        if i is None:
            i = self.id_of[token] = len(self.tokens)
            self.tokens.append(token)
        return i

    def get(self, token) -> Optional[int]:
        return self.id_of.get(token)

    def __len__(self) -> int:
        return len(self.tokens)

    def __contains__(self, token) -> bool:
        return token in self.id_of


class Bm25Weights:
    """What bm25_weights returns: the vocabulary, the passage-major CSR (row_ptr int64 [N + 1], term int32, weight fp32;
    the terms of a passage in order of first occurrence), and the statistics behind it (df int64 and idf fp64 per term,
    doc_len int64 per passage, avg_len)."""

    def __init__(self, vocab, row_ptr, term, weight, df, idf, doc_len, avg_len, k1, b):
        self.vocab, self.row_ptr, self.term, self.weight = vocab, row_ptr, term, weight
        self.df, self.idf, self.doc_len, self.avg_len, self.k1, self.b = df, idf, doc_len, avg_len, k1, b


def bm25_weights(docs_tokens: Sequence[Sequence], k1: float = 1.2, b: float = 0.75) -> Bm25Weights:
    """BM25 weights of N tokenised passages, per (passage, term) with tf occurrences of the term in a passage of len
    tokens:  idf = ln(1 + (N - df + 0.5) / (df + 0.5)),  w = idf * tf * (k1 + 1) / (tf + k1 * (1 - b + b * len / avg_len)),
    evaluated in fp64 in exactly that order and rounded once to fp32.  avg_len is the mean passage length (1 where every
    passage is empty)."""
    vocab = Vocabulary()
    row_ptr = np.zeros(len(docs_tokens) + 1, np.int64)
    terms, tfs = [], []
    doc_len = np.zeros(len(docs_tokens), np.int64)
    for p, toks in enumerate(docs_tokens):
        counts = {}
        for tok in toks:
            t = vocab.add(tok)
            counts[t] = counts.get(t, 0) + 1
        doc_len[p] = len(toks)
        terms.extend(counts.keys())          # dicts keep insertion order: first occurrence
        tfs.extend(counts.values())
        row_ptr[p + 1] = len(terms)
    n = len(docs_tokens)
    term = np.asarray(terms, np.int32)
    tf = np.asarray(tfs, np.float64)
    df = np.bincount(term, minlength=len(vocab)).astype(np.int64)
    idf = np.asarray([math.log(1.0 + (n - d + 0.5) / (d + 0.5)) for d in df.tolist()], np.float64)
    avg_len = float(doc_len.sum()) / n if n and doc_len.sum() else 1.0
    length = np.repeat(doc_len.astype(np.float64), np.diff(row_ptr))
    w = idf[term] * tf * (k1 + 1.0) / (tf + k1 * (1.0 - b + b * length / avg_len))
    return Bm25Weights(vocab, row_ptr, term, w.astype(np.float32), df, idf, doc_len, avg_len, k1, b)


def encode_queries(texts: Sequence[str], vocab: Vocabulary, tokenize_fn: Optional[Callable] = None,
                   max_terms: int = LEX_MAX_QUERY_TERMS):
    """The sparse queries of `texts` as the CSR triple engine.check_lexical takes: (q_ptr int32 [len(texts) + 1], q_term
    int32, q_weight fp32).  A query keeps the terms the vocabulary knows, each once, in order of first occurrence, with
    its count in the query as the weight; unknown tokens are dropped.  A query with more than max_terms DISTINCT known
    terms is TRUNCATED to its first max_terms (after the merge of repeats, so a long but repetitive query loses nothing):
    the device scores at most LEX_MAX_QUERY_TERMS terms per query and the engine refuses longer lists."""
    tok = tokenize_fn or default_tokenize
    q_ptr = np.zeros(len(texts) + 1, np.int32)
    terms, weights = [], []
    for i, text in enumerate(texts):
        counts = {}
        for t in tok(text):
            j = vocab.get(t)
            if j is not None:
                counts[j] = counts.get(j, 0) + 1
        keep = list(counts.items())[:max_terms]
        terms.extend(j for j, _ in keep)
        weights.extend(c for _, c in keep)
        q_ptr[i + 1] = len(terms)
    return q_ptr, np.asarray(terms, np.int32), np.asarray(weights, np.float32)


def invert_postings(n_passages: int, n_terms: int, row_ptr, term, weight):
    """Passage-major CSR (the terms of passage p are term[row_ptr[p] : row_ptr[p + 1]] with their weights) -> the
    inverted form hrag_lex_create takes: (term_ptr int64 [n_terms + 1], post_doc int32, post_w fp32), the passages of
    every list ascending.  A term repeated within a passage, or outside [0, n_terms), is an error."""
    rp = np.asarray(row_ptr, np.int64)
    t = np.asarray(term, np.int64)
    w = np.asarray(weight, np.float32)
    if t.shape != w.shape or t.ndim != 1:
        raise ValueError("term and weight must be one-dimensional and of one length")
    if rp.ndim != 1 or rp.shape[0] != n_passages + 1 or rp[0] != 0 or (np.diff(rp) < 0).any() or rp[-1] != t.shape[0]:
        raise ValueError(f"row_ptr: {n_passages + 1} non-decreasing entries from 0 to len(term) = {t.shape[0]} expected")
    if t.size and (int(t.min()) < 0 or int(t.max()) >= n_terms):
        raise ValueError(f"term ids must lie in [0, n_terms={n_terms})")
    doc = np.repeat(np.arange(n_passages, dtype=np.int64), np.diff(rp))
    order = np.lexsort((doc, t))                       # by term, the passages of a term ascending
    t_s, d_s = t[order], doc[order]
    if t.size > 1:
        dup = np.flatnonzero((t_s[1:] == t_s[:-1]) & (d_s[1:] == d_s[:-1]))
        if dup.size:
            raise ValueError(f"term {int(t_s[dup[0]])} is repeated within passage {int(d_s[dup[0]])}: merge its weights "
                             "before building the index")
    ptr = np.zeros(n_terms + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(t, minlength=n_terms))
    return ptr, d_s.astype(np.int32), np.ascontiguousarray(w[order])


class LexicalModel:
    """The lexical side of a corpus as the mirror holds it: the tokenizer, the BM25 weights of the passages (with their
    vocabulary, df and idf) and the query encoder over that vocabulary.  Rebuilt whenever the corpus changes: idf and the
    average length move with it."""

    def __init__(self, passages: Sequence[str], tokenize_fn: Optional[Callable] = None, k1: float = 1.2, b: float = 0.75):
        self.tokenize = tokenize_fn or default_tokenize
        self.bm25 = bm25_weights([self.tokenize(p) for p in passages], k1, b)
        self.vocab, self.idf, self.df = self.bm25.vocab, self.bm25.idf, self.bm25.df
        self.n_passages = len(passages)

    def postings(self):
        """(term_ptr, post_doc, post_w) for engine.LexicalIndex.from_postings."""
        return invert_postings(self.n_passages, len(self.vocab), self.bm25.row_ptr, self.bm25.term, self.bm25.weight)

    def encode_queries(self, texts: Sequence[str]):
        return encode_queries(texts, self.vocab, self.tokenize)
