"""Every subset of {doc filter, filter_scope="seeds", group_agg, group_hits, mmr, lexical, boost} on every entry (retrieve,
retrieve_scored, dense_retrieve, retrieve_converged, last_fused behind a retrieve) of one engine, at B = 9 (the fp16 PPR
state) and B = 65 (the e4m3 state): 128 subsets, 64 per test -- those without the boost and those with it.  Each combination does one of two things: it raises the exception tests/option_helpers.py's
servable names -- the refusal table of engine.py's docstrings -- with the argument's name in the message, and leaves a
following plain call bit-identical to one made before; or every output matches option_helpers.expected_outputs, the numpy
restatement of the whole composed call over the score rows the call leaves on the handle (tools/soak_options.py's check).
No combination may do a third thing."""

import importlib.util
import itertools
import os

import numpy as np
import pytest

from tests.option_helpers import BOOST_FORMS, BOOST_KINDS, BOOST_PROGRAMS, ENTRIES, CallSpec, servable

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOGGLES = ("filter", "seeds", "group_agg", "group_hits", "mmr", "lexical", "boost")
# the index of tests/test_gpu_payload.py::case (375 passages, max_topk 200), one engine for both batches
CASE = dict(v=3000, e=24000, dim=64, pfrac=0.125, b=65, max_topk=200, groups="shuffled", seed=4141)
MEMBER_PTR = {9: [0, 4, 9], 65: [0, 1, 30, 65]}
FILTERS = (("half", "bool"), ("payload", "payload"), ("few", "words"), ("sparse", "bool"), ("payload", "words"))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def harness(gpu_device):
    import torch
    tool = _tool("soak_options")
    case = tool.Case(CASE, torch.device("cuda", 0))
    yield case
    case.close()


def _spec(entry, on, i, b):
    """the call of one subset: the option values rotate with the subset's number"""
    s = CallSpec(entry=entry, k=10, workspace=bool(i % 5 == 3))
    if "filter" in on:
        s.filter_kind, s.filter_form = FILTERS[i % len(FILTERS)]
        s.filter_per_query, s.filter_seed = bool(i % 3), 100 + i
        s.payload_ids = [(i + r) % 7 for r in range(b)]
        if not s.filter_per_query and s.payload_ids[0] == 5:        # (None is a per-query entry)
            s.payload_ids[0] = 3
    if "seeds" in on:
        s.filter_scope = "seeds"
    if "group_agg" in on:
        s.group_agg = ("max", "sum")[i % 2]
    if "group_hits" in on:
        s.group_hits = (2, 1, 5)[i % 3]
    if "mmr" in on:
        s.mmr_lambda, s.mmr_candidates = (0.5, 0.0, 1.0, 0.3)[i % 4], (40, None, 10, 200)[(i // 2) % 4]
    if "lexical" in on:
        s.lexical_weight, s.lexical_empty = (0.3, 1.0, 0.5)[i % 3], i % 8 == 7
    if entry == "last_fused":
        s.fuse, s.member_ptr = ("sum", "max", "rrf")[i % 3], MEMBER_PTR[b]
        if s.fuse == "sum" and i % 2:
            s.weights = [float(v % 4) / 2 for v in range(b)]
        if s.fuse == "rrf":
            s.rrf_depth = (None, 1, 25)[(i // 3) % 3]
    if "boost" in on:       # one list or one per row, as the grammar or compiled; the programs rotate over the rows
        s.boost_kind, s.boost_form = BOOST_KINDS[i % 2], BOOST_FORMS[(i // 2) % 2]
        s.boost_ids = [(i + 3 * r) % len(BOOST_PROGRAMS) for r in range(b if s.boost_kind == "per_query" else 1)]
        if s.boost_kind == "one" and BOOST_PROGRAMS[s.boost_ids[0]] is None:       # (None is a per-query entry)
            s.boost_ids[0] = 7
    return s


def _walk(c, b, want_state, entry, boost):
    """the 64 subsets of TOGGLES with (boost) or without the boost on one entry -> (served, refused)"""
    if c.b != b:
        c.set_batch(b)
    c.eng.retrieve(c.qp, c.idx, c.sc, c.cnt, k=1)
    assert c.eng.stats()["last_ppr_state"] == want_state
    lim = dict(max_topk=c.max_topk, fact_sources=True)
    bad, served, refused = [], 0, 0
    subsets = [on for r in range(len(TOGGLES) + 1) for on in itertools.combinations(TOGGLES, r)]
    assert len(subsets) == 128
    subsets = [on for on in subsets if ("boost" in on) == boost]
    assert len(subsets) == 64
    for i, on in enumerate(subsets):
        spec = _spec(entry, on, i, b)
        assert ("boost" in spec.options()) == boost
        err = servable(spec, lim)
        if err is None:
            served += 1
            why = c.check_call(spec, np.random.default_rng([b, i]))
        else:
            refused += 1
            why = c.check_refusal(spec, err)
        bad += [(on, w, spec.to_json()) for w in why]
    assert not bad, bad[:5]
    return served, refused


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("b,want_state", [(9, 2), (65, 8)])
def test_every_subset_of_the_options_is_refused_by_name_or_is_the_restatement(harness, b, want_state, entry):
    served, refused = _walk(harness, b, want_state, entry, boost=False)
    # what the table refuses here: seeds without a filter (16), group_hits without group_agg among the others (12), seeds
    # with lexical among the rest (6): 34 of the 64; dense_retrieve(lexical=) serves nothing but the ranking filter (44)
    assert (served, refused) == ((20, 44) if entry == "dense_retrieve" else (30, 34))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("b,want_state", [(9, 2), (65, 8)])
@pytest.mark.parametrize("boost", [True], ids=["boost"])
def test_every_subset_of_the_options_with_a_boost_is_refused_by_name_or_is_the_restatement(harness, boost, b, want_state, entry):
    """The other 64 of the 128 subsets: the same walk with boost= on (one list / per query, grammar / BoostProgram, the
    programs of option_helpers.BOOST_PROGRAMS rotating).  A served call is the restatement over the boosted rows, which are
    also what last_doc_scores returns afterwards; a refused one leaves the following plain call bit-identical."""
    served, refused = _walk(harness, b, want_state, entry, boost)
    # the boost adds no refusal to retrieve / retrieve_scored / retrieve_converged / last_fused: the same 34 of 64 as
    # without it; dense_retrieve(boost=) serves the ranking filter and nothing else: {boost} and {boost, filter}, 2 of 64
    assert (served, refused) == ((2, 62) if entry == "dense_retrieve" else (30, 34))


def test_more_candidates_than_the_engine_ranks_are_refused_by_name(harness):
    """c = max(mmr_candidates, k) <= min(max_topk, 1024) (engine.py, retrieve): beyond max_topk a ValueError naming
    mmr_candidates, on every entry, before the refused call enqueues anything (last_fused: behind its retrieve)."""
    c = harness
    if c.b != 9:
        c.set_batch(9)
    for entry in ENTRIES:
        for kw in (dict(mmr_candidates=c.max_topk + 1), dict(mmr_candidates=1025), dict(k=c.max_topk + 1)):
            spec = _spec(entry, (), 0, 9)
            spec.mmr_lambda = 0.5
            for name, v in kw.items():
                setattr(spec, name, v)
            err = servable(spec, dict(max_topk=c.max_topk))
            assert err == (ValueError, "mmr_candidates")
            assert not c.check_refusal(spec, err), (entry, kw)
            spec.lexical_weight = 0.3                       # ... and before the lexical blend is formed
            if entry != "dense_retrieve":                   # (dense_retrieve(lexical=) refuses mmr_lambda itself)
                assert servable(spec, dict(max_topk=c.max_topk)) == err and not c.check_refusal(spec, err), (entry, kw)
