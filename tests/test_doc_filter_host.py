"""The doc filter's host side (no GPU): the bitset format against np.packbits, the mirror's metadata matching, its
validation, the bitset cache across index_from_openie / delete, and the masked host ranking used beyond max_topk."""

import numpy as np
import pytest

from hipporag_amd.engine import doc_filter_words, pack_mask
from hipporag_amd.retriever import Chunk, HippoRAG, RetrievalConfig, rank_allowed, unpack_mask


class _Embedder:
    def __init__(self, dim=16):
        self.dim = dim

    def batch_encode(self, texts, instruction=None, norm=True):
        texts = [texts] if isinstance(texts, str) else list(texts)
        out = np.stack([np.random.default_rng(abs(hash(t)) % 2 ** 32).standard_normal(self.dim) for t in texts])
        return (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32)


CHUNKS = [Chunk("Alice wrote the first report.", source_id="s1", metadata={"user": "alice", "year": 2020}),
          Chunk("Bob wrote the second report.", source_id="s2", metadata={"user": "bob", "year": 2021}),
          Chunk("Alice reviewed the budget.", source_id="s1", metadata={"user": "alice", "year": 2021}),
          Chunk("Carol filed a note.", metadata={"year": 2022}),
          Chunk("Bob and Carol met Alice.", source_id="s3", metadata={"user": "carol"})]
TRIPLES = [[("Alice", "wrote", "first report")], [("Bob", "wrote", "second report")], [("Alice", "reviewed", "budget")],
           [("Carol", "filed", "note")], [("Bob", "met", "Alice")]]


def _mirror(chunks=CHUNKS, triples=TRIPLES):
    rag = HippoRAG(RetrievalConfig(max_batch=4), embedding_model=_Embedder())
    rag.index_from_openie(list(chunks), list(triples))
    return rag


def _allowed(rag, f):
    return unpack_mask(rag._filter_words(f), len(rag.passage_node_keys))


def _pos(rag, chunk):
    return rag.passage_texts.index(chunk.content)


@pytest.mark.parametrize("n", [1, 5, 31, 32, 33, 64, 100, 1000])
def test_pack_mask_is_packbits_little_endian_padded_to_words(n):
    rng = np.random.default_rng(n)
    m = rng.random((3, n)) < 0.4
    w = pack_mask(m)
    assert w.dtype == np.uint32 and w.shape == (3, (n + 31) // 32)
    b = np.packbits(m, axis=-1, bitorder="little")
    padded = np.zeros((3, 4 * w.shape[1]), np.uint8)
    padded[:, :b.shape[1]] = b
    np.testing.assert_array_equal(w, padded.view("<u4"))
    for j in rng.integers(0, n, 20):           # bit (j & 31) of word j >> 5
        assert bool((w[1, j >> 5] >> (j & 31)) & 1) == m[1, j]
    np.testing.assert_array_equal(unpack_mask(w, n), m)
    np.testing.assert_array_equal(pack_mask(m[0]), w[0])


def test_torch_bool_filters_pack_like_the_host_and_packed_words_pass_through():
    import torch
    rng = np.random.default_rng(7)
    n = 77
    m = rng.random((4, n)) < 0.5
    w, ld = doc_filter_words(torch.from_numpy(m), n, 4, torch.device("cpu"))
    assert ld == 3 and w.dtype == torch.int32
    np.testing.assert_array_equal(w.numpy().view(np.uint32), pack_mask(m))
    w1, ld1 = doc_filter_words(torch.from_numpy(m[2]), n, 4, torch.device("cpu"))
    assert ld1 == 0
    np.testing.assert_array_equal(w1.numpy().view(np.uint32), pack_mask(m[2]))
    packed = torch.from_numpy(pack_mask(m).view(np.int32))
    w2, ld2 = doc_filter_words(packed, n, 4, torch.device("cpu"))
    assert ld2 == 3 and torch.equal(w2, packed)
    with pytest.raises(ValueError):
        doc_filter_words(torch.from_numpy(m[:, :50]), n, 4, torch.device("cpu"))      # wrong length
    with pytest.raises(ValueError):
        doc_filter_words(torch.from_numpy(m[:3]), n, 4, torch.device("cpu"))          # wrong batch
    with pytest.raises(ValueError):
        doc_filter_words(packed[:, :2], n, 4, torch.device("cpu"))                    # too few words
    with pytest.raises(TypeError):
        doc_filter_words(torch.zeros(n), n, 4, torch.device("cpu"))
    with pytest.raises(TypeError):
        doc_filter_words(m, n, 4, torch.device("cpu"))


def test_metadata_dicts_match_one_value_a_list_of_values_source_id_and_never_a_missing_key():
    rag = _mirror()
    n = len(rag.passage_node_keys)
    pos = [_pos(rag, c) for c in CHUNKS]

    def want(*idx):
        m = np.zeros(n, bool)
        m[[pos[i] for i in idx]] = True
        return m

    np.testing.assert_array_equal(_allowed(rag, {"user": "alice"}), want(0, 2))
    np.testing.assert_array_equal(_allowed(rag, {"user": ["alice", "carol"]}), want(0, 2, 4))
    np.testing.assert_array_equal(_allowed(rag, {"source_id": "s1"}), want(0, 2))
    np.testing.assert_array_equal(_allowed(rag, {"source_id": ["s2", "s3"]}), want(1, 4))
    np.testing.assert_array_equal(_allowed(rag, {"year": 2021}), want(1, 2))
    np.testing.assert_array_equal(_allowed(rag, {"user": "alice", "year": 2021}), want(2))     # keys: AND
    np.testing.assert_array_equal(_allowed(rag, {"user": "dave"}), want())
    np.testing.assert_array_equal(_allowed(rag, {"colour": "red"}), want())                    # nobody has the key
    np.testing.assert_array_equal(_allowed(rag, {"year": [2022]}), want(3))                    # chunk 3: no user key
    np.testing.assert_array_equal(_allowed(rag, {}), np.ones(n, bool))                        # no condition
    arr = np.zeros(n, bool)
    arr[pos[3]] = True
    np.testing.assert_array_equal(_allowed(rag, arr), arr)


def test_filter_validation():
    rag = _mirror()
    n = len(rag.passage_node_keys)
    with pytest.raises(TypeError):
        rag._doc_filter_words("user=alice", 1)
    with pytest.raises(TypeError):
        rag._doc_filter_words(np.zeros(n, np.int32), 1)
    with pytest.raises(TypeError):
        rag._doc_filter_words([{"user": "bob"}, 3], 2)
    with pytest.raises(ValueError):
        rag._doc_filter_words(np.zeros(n + 1, bool), 1)
    with pytest.raises(ValueError):
        rag._doc_filter_words([{"user": "bob"}], 2)
    assert rag._doc_filter_words(None, 3) is None
    one = rag._doc_filter_words({"user": "bob"}, 3)
    assert one.shape == ((n + 31) // 32,)                       # one row for the whole batch
    per = rag._doc_filter_words([{"user": "bob"}, {"user": "alice"}, np.ones(n, bool)], 3)
    assert per.shape == (3, (n + 31) // 32)
    np.testing.assert_array_equal(per[0], one)


def test_the_bitset_cache_follows_index_from_openie_and_delete():
    rag = _mirror()
    first = _allowed(rag, {"user": "bob"})
    assert first.sum() == 1 and ("user", "bob") in rag._filter_cache
    extra = Chunk("Bob drafted a plan.", source_id="s9", metadata={"user": "bob"})
    rag.index_from_openie([extra], [[("Bob", "drafted", "plan")]])
    assert rag._filter_cache == {}                               # invalidated by the new passages
    after = _allowed(rag, {"user": "bob"})
    assert after.sum() == 2 and after[_pos(rag, extra)] and after[_pos(rag, CHUNKS[1])]
    rag.delete([CHUNKS[1].content])
    gone = _allowed(rag, {"user": "bob"})
    assert len(gone) == len(rag.passage_node_keys) and gone.sum() == 1 and gone[_pos(rag, extra)]


def test_masked_host_ranking_is_the_allowed_prefix_of_the_full_ranking():
    rng = np.random.default_rng(11)
    x = rng.integers(0, 6, (5, 300)).astype(np.float32)           # many ties: broken by the larger index
    x[0, 7] = np.nan
    allowed = rng.random((5, 300)) < 0.3
    allowed[3] = False
    for want in (1, 10, 200, 300):
        idx, sc = rank_allowed(x, allowed, want)
        for i in range(5):
            full = np.argsort(x[i], kind="stable")[::-1]
            keep = [j for j in full if allowed[i, j]][:want]
            assert idx[i, :len(keep)].tolist() == keep
            assert (idx[i, len(keep):] == -1).all() and (sc[i, len(keep):] == 0).all()
            np.testing.assert_array_equal(sc[i, :len(keep)], x[i, keep])
    idx, _ = rank_allowed(x, allowed[1], 4)                        # one row for all queries
    for i in range(5):
        assert idx[i].tolist() == [j for j in np.argsort(x[i], kind="stable")[::-1] if allowed[1, j]][:4]
