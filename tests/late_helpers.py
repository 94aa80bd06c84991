"""numpy restatements of late-interaction reranking (include/hrag.h, "late-interaction reranking"; csrc/late.hip).

Token vectors are given as float arrays whose values ARE 16-bit values (bf16 / fp16) already: every product is then exact in
fp64, and s_ij below is the fp64 dot product the kernel's fp32 MFMA chain approximates (exactly, on dyadic inputs).

    s_ij   = q_i . t_j                                  (fp64)
    m_i    = np.fmax over the passage's tokens of s_ij, from -inf (a NaN s_ij is ignored)
    score  = float32(sum over i ascending of m_i) + 0   (one rounding; -0 -> +0)

an empty slot (id < 0 or id >= n) reads 0.0 and never ranks; a passage without tokens scores -inf when the query has
tokens; a query without tokens scores +0.0 everywhere."""

import numpy as np


def ragged(arrays, dim):
    """list of [t_i, dim] arrays -> (ptr int64 [n + 1], rows float64 [T, dim])"""
    ptr = np.zeros(len(arrays) + 1, np.int64)
    ptr[1:] = np.cumsum([len(a) for a in arrays])
    rows = np.zeros((int(ptr[-1]), dim), np.float64)
    for i, a in enumerate(arrays):
        if len(a):
            rows[ptr[i]:ptr[i + 1]] = np.asarray(a, np.float64).reshape(-1, dim)
    return ptr, rows


def late_scores_np(tok_ptr, tok, q_ptr, q_tok, cand):
    """float32 [B, c]: the MaxSim score of every candidate slot, vectorised over the candidates of a query."""
    tok_ptr, q_ptr = np.asarray(tok_ptr, np.int64), np.asarray(q_ptr, np.int64)
    tok, q_tok, cand = np.asarray(tok, np.float64), np.asarray(q_tok, np.float64), np.asarray(cand, np.int64)
    n, (b, c) = tok_ptr.shape[0] - 1, cand.shape
    t_all = tok.shape[0]
    out = np.zeros((b, c), np.float32)
    live = (cand >= 0) & (cand < n)
    for q in range(b):
        qt = q_tok[q_ptr[q]:q_ptr[q + 1]]
        if qt.shape[0] == 0 or not live[q].any():
            continue                                                            # +0.0 everywhere
        uniq, inv = np.unique(cand[q][live[q]], return_inverse=True)            # every passage of the row once
        start, length = tok_ptr[uniq], tok_ptr[uniq + 1] - tok_ptr[uniq]
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.concatenate([qt @ tok.T, np.full((qt.shape[0], 1), -np.inf)], axis=1)   # [nq, T + 1]: column T is the mask
        j = np.arange(max(int(length.max()), 1))[None, :]
        pos = np.where(j < length[:, None], start[:, None] + j, t_all)          # [u, lmax]
        m = np.fmax.reduce(s[:, pos], axis=2, initial=-np.inf)                  # [nq, u]
        acc = np.zeros(len(uniq), np.float64)
        with np.errstate(invalid="ignore"):
            for i in range(m.shape[0]):                                         # ascending token order
                acc = acc + m[i]
            sc = acc.astype(np.float32) + np.float32(0)
        out[q, live[q]] = sc[inv]
    return out


def late_scores_naive(tok_ptr, tok, q_ptr, q_tok, cand):
    """The same by plain loops over (query, slot, query token, passage token)."""
    cand = np.asarray(cand)
    n = len(tok_ptr) - 1
    b, c = cand.shape
    out = np.zeros((b, c), np.float32)
    for q in range(b):
        for s in range(c):
            p = int(cand[q, s])
            if p < 0 or p >= n:
                continue
            total = 0.0
            for i in range(int(q_ptr[q]), int(q_ptr[q + 1])):
                best = -np.inf
                for j in range(int(tok_ptr[p]), int(tok_ptr[p + 1])):
                    with np.errstate(invalid="ignore", over="ignore"):
                        v = float(np.dot(np.asarray(q_tok[i], np.float64), np.asarray(tok[j], np.float64)))
                    if v > best:            # False for a NaN v: it is ignored
                        best = v
                with np.errstate(invalid="ignore"):
                    total = total + best
            with np.errstate(invalid="ignore"):
                out[q, s] = np.float32(total) + np.float32(0)
    return out


def late_rank_np(score, cand, n, k):
    """(sel int32, idx int32, score float32) [B, k]: the live slots by the library's ranking key -- every NaN above +inf,
    -0 ties +0 -- a tie to the smaller slot; -1 / -1 / 0 once the live slots run out.  n <= 0: a negative id only is empty."""
    score, cand = np.asarray(score, np.float32), np.asarray(cand, np.int64)
    b, c = cand.shape
    sel = np.full((b, k), -1, np.int32)
    idx = np.full((b, k), -1, np.int32)
    out = np.zeros((b, k), np.float32)
    for q in range(b):
        live = np.flatnonzero((cand[q] >= 0) & ((cand[q] < n) if n > 0 else True))
        v = score[q, live] + np.float32(0)
        nan = np.isnan(v)
        order = np.lexsort((live, -np.where(nan, np.float32(0), v).astype(np.float64), ~nan))
        top = live[order][:k]
        sel[q, :len(top)] = top
        idx[q, :len(top)] = cand[q, top]
        out[q, :len(top)] = score[q, top] + np.float32(0)
    return sel, idx, out


def late_rank_naive(score, cand, n, k):
    """The same by repeated selection of the best remaining slot."""
    score, cand = np.asarray(score, np.float32), np.asarray(cand)
    b, c = cand.shape
    sel = np.full((b, k), -1, np.int32)
    idx = np.full((b, k), -1, np.int32)
    out = np.zeros((b, k), np.float32)

    def better(x, y):       # x strictly ahead of y by value
        if np.isnan(x) or np.isnan(y):
            return bool(np.isnan(x) and not np.isnan(y))
        return bool(x > y)  # (-0 > +0 is False either way: they tie)

    for q in range(b):
        left = [s for s in range(c) if cand[q, s] >= 0 and (n <= 0 or cand[q, s] < n)]
        for t in range(k):
            if not left:
                break
            best = left[0]
            for s in left[1:]:
                if better(score[q, s], score[q, best]):
                    best = s
            left.remove(best)
            sel[q, t], idx[q, t] = best, cand[q, best]
            out[q, t] = score[q, best] + np.float32(0)
    return sel, idx, out


def exact_tokens(rng, lengths, dim, sign=None):
    """list of [t_i, dim] arrays of integers in [-3, 3] x 2^-3: every s_ij is a multiple of 2^-6 below 36 (dim <= 256) and
    every score below 2304, exact in fp32 whatever the accumulation order.  sign=+1 / -1: components in (0, 3] x 2^-3
    of that sign only (every product of a +1 and a -1 set is negative)."""
    out = []
    for t in lengths:
        if sign is None:
            a = rng.integers(-3, 4, size=(t, dim))
        else:
            a = sign * rng.integers(1, 4, size=(t, dim))
        out.append(a.astype(np.float64) * 2.0 ** -3)
    return out


def planted_late_corpus(seed, n_queries=6, n_fill=10, dim=64, nq=4):
    """A corpus on which one vector per passage ranks the wrong passage first and MaxSim the right one.

    Query q has nq token vectors, each with four entries of +-1/2 on positions of its own (unit norm exactly, in bf16 and
    fp16 alike); its single vector is their mean.  Its RIGHT passage holds those token vectors verbatim among 3 * nq
    others on coordinates no query token touches -- so its MaxSim is nq exactly, while its single vector (the mean of its
    tokens) is pulled away from the query's (cosine about 1/2).  Its DISTRACTOR holds nq copies of
    the query's mean direction: one vector as similar to the query vector as can be (cosine 1), but no token equals any
    query token: every s_ij is 1/2 and its MaxSim nq / 2.  n_fill filler passages of random tokens follow.

    -> dict(dim, q_tokens [list of [nq, dim]], p_tokens [list of [t, dim]], q_vec [Q, dim] float32, p_vec [n, dim] float32
    (unit rows), right [Q], distractor [Q])."""
    rng = np.random.default_rng(seed)
    assert dim >= 8 * nq
    q_tokens, p_tokens, right, distractor = [], [], [], []
    for q in range(n_queries):
        perm = rng.permutation(dim)
        toks = np.zeros((nq, dim))
        for i in range(nq):
            toks[i, perm[4 * i:4 * i + 4]] = rng.choice([-0.5, 0.5], size=4)
        mean_dir = toks.sum(0) / np.sqrt(nq)                    # unit: the tokens are orthogonal (entries +-1/4 for nq = 4)
        others = np.zeros((3 * nq, dim))
        for i in range(3 * nq):                                 # off the query's coordinates altogether: s_ij = 0
            others[i, perm[4 * nq + (4 * i) % (dim - 4 * nq - 3):][:4]] = 0.5
        q_tokens.append(toks)
        right.append(len(p_tokens))
        p_tokens.append(np.concatenate([others[:nq], toks, others[nq:]]))
        distractor.append(len(p_tokens))
        p_tokens.append(np.tile(mean_dir, (nq, 1)))
    for _ in range(n_fill):
        t = int(rng.integers(3, 9))
        p_tokens.append(rng.integers(-2, 3, size=(t, dim)) * 0.125)

    def unit_mean(rows):
        v = np.asarray(rows, np.float64).mean(0)
        nrm = np.linalg.norm(v)
        return (v / nrm if nrm > 0 else v).astype(np.float32)

    return {"dim": dim, "q_tokens": q_tokens, "p_tokens": p_tokens,
            "q_vec": np.stack([unit_mean(t) for t in q_tokens]), "p_vec": np.stack([unit_mean(t) for t in p_tokens]),
            "right": np.asarray(right), "distractor": np.asarray(distractor)}


class PlantedEmbedder:
    """embedding_model of the planted corpus: a text names its passage ("passage 3 ...", its fact and entities
    "... thing3 ...") or its query ("query 2 ...") and gets that one's single vector."""

    def __init__(self, corpus):
        self.c = corpus

    def batch_encode(self, texts, instruction=None, norm=True):
        import re
        texts = [texts] if isinstance(texts, str) else list(texts)
        out = []
        for t in texts:
            i = int(re.search(r"\d+", t).group())
            out.append(self.c["q_vec"][i] if t.startswith("query") else self.c["p_vec"][i])
        return np.stack(out).astype(np.float32)


class PlantedTokenEncoder:
    """token_encoder of the planted corpus, deterministic; `calls` records (texts, is_query) of every call."""

    def __init__(self, corpus):
        self.c, self.calls = corpus, []

    def encode_tokens(self, texts, is_query):
        import re
        self.calls.append((list(texts), bool(is_query)))
        src = self.c["q_tokens"] if is_query else self.c["p_tokens"]
        return [np.asarray(src[int(re.search(r"\d+", t).group())], np.float32) for t in texts]


def planted_texts(corpus):
    """(passage texts, one triple list per passage, query strings) of the planted corpus"""
    n = len(corpus["p_tokens"])
    docs = [f"passage {i} of the planted corpus" for i in range(n)]
    triples = [[(f"ent{i}", "is", f"thing{i}")] for i in range(n)]
    return docs, triples, [f"query {q} ?" for q in range(len(corpus["q_tokens"]))]
