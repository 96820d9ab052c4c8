"""The keywords of the Python search calls, the part that needs no GPU: every public signature as it was before the keywords
travelled as one record (searcher.SearchKeywords), the refusals of conflicting keywords at the three levels of a Searcher, what
the module-level `search` hands a searcher, and the record's `plain`."""
import ctypes as C
import dataclasses
import inspect

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import distributed, searcher, sharded
from tests.test_group_cpu import _NoDevice
from tests.test_prior_cpu import fake_prior
from tests.util_group import ids_from_lens

REQ = "<required>"
POS, KW = "pos", "kw"          # positional-or-keyword / keyword-only
_ONE = [("filter", KW, None), ("scope", KW, "candidates"), ("grouping", KW, None), ("per_group", KW, None), ("prior", KW, None),
        ("prior_weight", KW, 1.0), ("after", KW, None), ("candidates", KW, None), ("return_candidate_scores", KW, False),
        ("candidate_priors", KW, None)]
_SHARDED = [("scope", KW, "candidates"), ("protocol", KW, "auto"), ("grouping", KW, None), ("per_group", KW, None),
            ("after", KW, None), ("prior", KW, None), ("prior_weight", KW, 1.0), ("candidates", KW, None),
            ("return_candidate_scores", KW, False), ("candidate_priors", KW, None)]
_DEVICE = [("filters", POS, None), ("scope", POS, "candidates"), ("grouping", POS, None), ("per_group", POS, None),
           ("prior", POS, None), ("prior_weight", POS, 1.0), ("after", POS, None), ("candidates", POS, None),
           ("candidate_scores", POS, None), ("candidate_priors", POS, None)]
_Q = [("self", POS, REQ), ("Q", POS, REQ), ("k", POS, REQ), ("nprobe", POS, None)]
# written down from the commit before the record: names, kinds and defaults, in order
SIGNATURES = {
    "search": [("searcher", POS, REQ), ("query", POS, REQ), ("k", POS, REQ)] + _ONE,
    "Searcher.search": [("self", POS, REQ), ("query", POS, REQ), ("k", POS, REQ)] + _ONE,
    "Searcher.search_embeddings": _Q + _ONE,
    "Searcher.search_batch": _Q + [("pad_short", POS, False), ("filters", KW, None)] + _ONE[1:],
    "ShardedSearcher.search": [("self", POS, REQ), ("query", POS, REQ), ("k", POS, REQ), ("filter", KW, None)] + _SHARDED,
    "ShardedSearcher.search_embeddings": _Q + [("filter", KW, None)] + _SHARDED,
    "ShardedSearcher.search_batch": _Q + [("pad_short", POS, False), ("filters", KW, None)] + _SHARDED,
    "DeviceSearch.__call__": [("self", POS, REQ), ("Qdev", POS, REQ)] + _DEVICE,
    "DeviceSearch.capture": [("self", POS, REQ), ("Qstatic", POS, REQ)] + _DEVICE,
    "DeviceSearch.replay": [("self", POS, REQ), ("graph", POS, REQ), ("Qstatic", POS, REQ)] + _DEVICE,
    "DeviceSearch.phase1": [("self", POS, REQ), ("Qdev", POS, REQ), ("filters", POS, None), ("scope", POS, "candidates"),
                            ("grouping", POS, None), ("group_base", POS, 0), ("prior", POS, None), ("prior_weight", POS, 1.0)],
    "DeviceSearch.phase2": [("self", POS, REQ), ("Qdev", POS, REQ), ("all_top", POS, REQ), ("all_gid", POS, None),
                            ("grouping", POS, None), ("group_base", POS, 0), ("prior", POS, None), ("prior_weight", POS, 1.0),
                            ("all_mabs", POS, None)],
    "DeviceSearch.search_grouped_shard": [("self", POS, REQ), ("Qdev", POS, REQ), ("filters", POS, REQ), ("scope", POS, REQ),
                                          ("grouping", POS, REQ), ("group_base", POS, REQ), ("prior", POS, None),
                                          ("prior_weight", POS, 1.0)],
    "search_request": [("searcher", POS, REQ), ("B", POS, REQ), ("filters", KW, None), ("scope", KW, "candidates"),
                       ("grouping", KW, None), ("per_group", KW, None), ("prior", KW, None), ("prior_weight", KW, 1.0),
                       ("after", KW, None), ("pad_short", KW, False), ("group_base", KW, 0), ("cursor_arrays", KW, "_after_arrays"),
                       ("candidates", KW, None), ("candidate_scores", KW, None), ("candidate_arrays", KW, "_candidate_arrays"),
                       ("candidate_priors", KW, None), ("candidate_prior_arrays", KW, "_candidate_prior_arrays")],
}


def signature_of(name):
    obj = {"search": searcher, "search_request": searcher, "Searcher": searcher.Searcher, "ShardedSearcher": sharded.ShardedSearcher,
           "DeviceSearch": distributed.DeviceSearch}[name.split(".")[0]]
    kinds = {inspect.Parameter.POSITIONAL_OR_KEYWORD: POS, inspect.Parameter.KEYWORD_ONLY: KW}
    rows = []
    for p in inspect.signature(getattr(obj, name.split(".")[-1])).parameters.values():
        default = REQ if p.default is inspect.Parameter.empty else getattr(p.default, "__name__", p.default)
        rows.append((p.name, kinds[p.kind], default))            # any other kind of parameter is a KeyError: none had one
    return rows


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_public_signatures_are_those_of_the_parent(name):
    got = signature_of(name)
    if name == "search_request":       # it may additionally take a ready-made record: keyword-only, behind everything it had
        assert all(kind == KW and default is None for _, kind, default in got[len(SIGNATURES[name]):])
        got = got[:len(SIGNATURES[name])]
    assert got == SIGNATURES[name]


# ---- refusals: the same class and message from search (no encoder attached), search_embeddings and search_batch ----------
AFTER = "after together with {} is not supported: a cursor continues the ranking of passages by MaxSim"
NO_ENCODER = ("ColBERTError", "no query encoder attached: pass encoder=... or use search_embeddings(Q, k)")
# one-query keywords (G / F / P: an open grouping, filter and prior) -> (class, message), as the parent answered at all three
# levels; a triple where its levels disagreed: (search, search_embeddings, search_batch)
REFUSALS = [
    (dict(after=(3.0, 5), grouping="G"), ("Unsupported", AFTER.format("grouping"))),
    (dict(after=(3.0, 5), per_group=2), ("Unsupported", AFTER.format("per_group"))),
    (dict(after=(3.0, 5), grouping="G", per_group=2), ("Unsupported", AFTER.format("grouping"))),
    (dict(after=(3.0, 5), prior="P"), ("Unsupported", AFTER.format("prior"))),
    (dict(candidates=[1001, 1002], filter="F"),
     ("Unsupported", "candidates= together with filter(s)= is not supported: a list is the candidate set")),
    (dict(return_candidate_scores=True),
     ("ArgumentError", "candidate scores need candidates=: they are the scores of the listed passages")),
    (dict(candidate_priors=[0.5, 1.0]), ("ArgumentError", "candidate_priors needs candidates=: it holds one value per listed passage")),
    (dict(candidates=[1001, 1002], candidate_priors=[0.5, 1.0], prior="P"),
     ("Unsupported", "candidate_priors together with prior is not supported: a call has one additive term")),
    (dict(candidates=[1001, 1002], candidate_priors=[0.5, 1.0], grouping="G", per_group=2),
     ("Unsupported", "per_group together with candidate_priors is not supported: the hits of a grouped search take no additive term "
                     "(per_group=1 is the grouped search itself)")),
    (dict(candidates=[1001, 1002], candidate_priors=[0.5, 1.0], after=(3.0, 5)),
     ("Unsupported", "after together with candidate_priors is not supported: a cursor continues the ranking of passages by MaxSim")),
    (dict(scope="some"), ("ColBERTError", "scope must be 'candidates' or 'all', got 'some'")),
    (dict(scope="all", filter="F", after=(3.0, 5), prior="P"), ("Unsupported", AFTER.format("prior"))),
    # per_group with a prior is none of the four keyword rules: the request builder refuses it, behind the encoder check of search
    (dict(grouping="G", per_group=2, prior="P"),
     (NO_ENCODER,) + (("Unsupported", "per_group together with a prior is not supported: the hits of a grouped search take no prior"),) * 2),
    (dict(grouping="G", per_group=2, prior="P", prior_weight=0.5),
     (NO_ENCODER,) + (("Unsupported", "per_group together with a prior is not supported: the hits of a grouped search take no prior"),) * 2),
]


def outcome(call):
    try:
        call()
    except clb.ColBERTError as e:
        return type(e).__name__, str(e)
    return None


def three_levels(s, kw):
    """the outcome of one-query keywords at search, search_embeddings and -- lifted to a batch of one -- search_batch"""
    lift = {"filter": lambda f: ("filters", [f]), "after": lambda a: ("after", ([a[0]], [a[1]])),
            "candidates": lambda c: ("candidates", [c]), "candidate_priors": lambda v: ("candidate_priors", [v])}
    batch = dict(lift[name](v) if name in lift else (name, v) for name, v in kw.items())
    Q = np.zeros((128, 32, 1), np.float32, order="F")
    return (outcome(lambda: s.search("a query", 5, **kw)), outcome(lambda: s.search_embeddings(Q[:, :, 0], 5, **kw)),
            outcome(lambda: s.search_batch(Q, 5, **batch)))


@pytest.mark.parametrize("row", range(len(REFUSALS)))
def test_refusals_agree_across_the_levels_of_a_searcher(row):
    s = _NoDevice()
    s.encoder = None
    handles = {"G": clb.PassageGrouping(s, C.c_void_p(0xbee0), 2, ids_from_lens([60, 40])),
               "F": clb.PassageFilter(s, C.c_void_p(0xfee0), 3), "P": fake_prior(s, 2.0)}
    kw, want = REFUSALS[row]
    kw = {name: handles.get(v, v) if isinstance(v, str) else v for name, v in kw.items()}
    try:
        got = three_levels(s, kw)
    finally:
        for h in handles.values():
            h._h = None                                        # never destroyed: they were never created
    assert got == (want if len(want) == 3 else (want,) * 3)


# ---- the module-level search: what it hands a duck-typed searcher ---------------------------------------------------------
class _Recorder:
    def search(self, query, k, **kw):
        return "search", kw

    def search_embeddings(self, Q, k, **kw):
        return "search_embeddings", kw


ALWAYS = dict(filter=None, scope="candidates", grouping=None, per_group=None)
HANDED = [          # the caller's keywords -> what the searcher receives besides ALWAYS, as the parent handed it
    (dict(), dict()),
    (dict(after=(3.0, 5)), dict(after=(3.0, 5))),
    (dict(prior="P"), dict(prior="P", prior_weight=1.0)),
    (dict(prior_weight=2.0), dict(prior=None, prior_weight=2.0)),
    (dict(candidates=[4, 2]), dict(candidates=[4, 2], return_candidate_scores=False)),
    (dict(return_candidate_scores=True), dict(candidates=None, return_candidate_scores=True)),
    (dict(candidate_priors=[0.5]), dict(candidate_priors=[0.5])),
    (dict(candidates=[4], candidate_priors=[0.5], prior_weight=-1.0, scope="all", per_group=1),
     dict(candidates=[4], return_candidate_scores=False, candidate_priors=[0.5], prior=None, prior_weight=-1.0, scope="all",
          per_group=1)),
]


@pytest.mark.parametrize("row", range(len(HANDED)))
def test_module_search_hands_over_the_keywords_the_parent_handed_over(row):
    given, more = HANDED[row]
    for query, entry in (("a query", "search"), (np.zeros((128, 4), np.float32), "search_embeddings")):
        assert clb.search(_Recorder(), query, 5, **given) == (entry, {**ALWAYS, **more})


# ---- the record -----------------------------------------------------------------------------------------------------------
def test_the_record_is_plain_exactly_when_every_field_is_at_its_default():
    fields = dataclasses.fields(searcher.SearchKeywords)
    assert [f.name for f in fields] == [name for name, _, _ in _DEVICE]           # DeviceSearch's positional order
    assert [f.default for f in fields] == [default for _, _, default in _DEVICE]
    assert searcher.SearchKeywords().plain
    for f in fields:
        other = "all" if f.name == "scope" else 2.0 if f.name == "prior_weight" else object()
        assert not dataclasses.replace(searcher.SearchKeywords(), **{f.name: other}).plain, f.name
    with pytest.raises(dataclasses.FrozenInstanceError):
        searcher.SearchKeywords().scope = "all"


def test_the_record_lifts_one_query_to_a_batch_of_one():
    one = searcher.SearchKeywords(filters="F", after=(3.0, 5), candidates=[4, 2], candidate_priors=[0.5, 1.0], grouping="G")
    lifted = one.for_one_query()
    assert (lifted.filters, lifted.after, lifted.candidates, lifted.candidate_priors) == (["F"], ([3.0], [5]), [[4, 2]], [[0.5, 1.0]])
    assert lifted.grouping == "G" and searcher.SearchKeywords().for_one_query() == searcher.SearchKeywords()
    with pytest.raises(clb.ArgumentError, match=r"after must be a pair \(score, pid\)"):
        searcher.SearchKeywords(after=3.0).for_one_query()
