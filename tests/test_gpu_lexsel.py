"""The four forms of the BM25 top-`limit` selection (lexical.hip: sort, sampled threshold over 4096 or 8192 keys, exact
radix passes) driven by the designed postings of lexsel_vectors.py -- every case bit for bit against the vectorised
reference (rows, order, f32 score bits; no tolerance), and the form each call took read back from
rlr_lexical_select_forms: a case aimed at one form cannot pass through another.

One engine over SEL (24 576 rows of 32 elements) serves the module: its lexical index takes the single and the batched
calls, its embedding index makes the row filters, and the text searches run over both.

Under RLR_LEX_SAMPLE_RANK=1 (the retry test of test_gpu_fuzz.py runs test_single_path_every_case in such a process) the
threshold is the largest sample key, admitting at most 1 + 8 sample keys (the slack of the LDS select): a sampled case
that wants more than that of a sample that is the whole touched list MUST come back through the exact path, and one
that wants 100 and more of a strided sample does (the touched list holds at most 3.5 keys per sample key).  A case that
wants one document cannot: the threshold is itself a touched key, so the list is never short of one."""
import os

import numpy as np
import pytest

import lexsel_vectors as V

pytestmark = pytest.mark.gpu

DIM = 32
EPS = np.float32(1.1920929e-07)
FORCED = os.environ.get("RLR_LEX_SAMPLE_RANK") == "1"
_shared = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sel_engine(rlr):
    """the module's engine (built on first use; the retry test's child process calls the test functions directly)"""
    if "eng" not in _shared:
        from oracle import oracle as O
        O.lib()
        eng = rlr.RagEngine(DIM)
        eng.index.append(O.synth_rows(V.N_ROWS, DIM, seed=611), normalize=True)
        eng._chunks = [rlr.DocumentChunk(str(i), "sel", "", i) for i in range(V.N_ROWS)]
        for r, toks in enumerate(V.sel_rows()):
            eng.lexical.add_tokens(r, toks)
        _shared["eng"] = eng
        _shared["stored"] = eng.index.fetch_rows(np.arange(V.N_ROWS))
        _shared["filters"] = {name: eng.index.filter_rows(rows) for name, rows in V.sel_filters().items()}
    return _shared["eng"]


@pytest.fixture(scope="module", autouse=True)
def _close_engine():
    yield
    for f in _shared.pop("filters", {}).values():
        f.close()
    if "eng" in _shared:
        _shared.pop("eng").close()
    _shared.clear()


def full_list(query, flt=None):
    """the reference's whole list of a query (a token tuple) under a named filter: one pass, shared by every limit"""
    return V.full_list(tuple(query), flt)


def counts(g):
    return g.select_forms(), g.segments()["select_retries"]


def moved(g, before):
    forms, retries = counts(g)
    return {f: forms[f] - before[0][f] for f in V.FORMS}, retries - before[1]


def expect_forms(form, retries):
    want = dict.fromkeys(V.FORMS, 0)
    want[form] += 1
    want[V.EXACT] += retries
    return want


def check_retries(case_form, n_touched, limit, retries, ctx):
    """the retries one call may, must or must not have caused"""
    assert retries in (0, 1), ctx
    if case_form not in (V.S4096, V.S8192):
        assert retries == 0, ctx
        return
    m = V.sample_model(n_touched, limit, 4096 if case_form == V.S4096 else 8192)
    want = min(V.served_limit(limit), n_touched)
    if m["all_wanted"]:
        assert retries == 0, ctx                             # thr = 0: the list is the touched list
    elif not FORCED:
        if m["whole"]:
            assert retries == 0, ctx                         # the sample is the list: a retry is a logic error, not bad luck
    elif want == 1:
        assert retries == 0, ctx
    elif (m["whole"] and want > 1 + V.SLACK) or want >= 100:
        assert retries == 1, ctx


# ---------------------------------------------------------------- single path
def test_single_path_every_case(rlr):
    eng = sel_engine(rlr)
    g = eng.lexical
    ran = dict.fromkeys(V.FORMS, 0)
    touched_seen = set()
    for case in V.cases():
        flt = _shared["filters"][case["filter"]] if case["filter"] else None
        before = counts(g)
        rows, sc = g.score_tokens(case["query"], case["limit"], filter=flt)
        d_forms, d_retries = moved(g, before)
        want_rows, want_sc = V.reference(case)
        ctx = (case["name"], case["form"], d_forms, d_retries)
        assert np.array_equal(rows.astype(np.int64), want_rows), ctx
        assert np.array_equal(bits(sc), bits(want_sc)), ctx
        check_retries(case["form"], case["n_touched"], case["limit"], d_retries, ctx)
        assert d_forms == expect_forms(case["form"], d_retries), ctx
        for f, c in d_forms.items():
            ran[f] += c
        touched_seen.add(case["n_touched"])
    assert all(ran[f] >= 3 for f in V.FORMS), ran
    assert touched_seen >= {0, 50, 3000, 8192, 8193, 9000}
    print("forms run by the single-path cases:", ran)


def test_null_arguments_of_the_form_counts(rlr):
    import ctypes as C
    L = rlr.lib()
    g = sel_engine(rlr).lexical
    assert L.rlr_lexical_select_forms(None, None, None, None, None) == -1           # RLR_E_INVALID
    assert L.rlr_lexical_select_forms(g._h, None, None, None, None) == 0
    one = C.c_uint64(1 << 40)
    assert L.rlr_lexical_select_forms(g._h, None, None, None, C.byref(one)) == 0
    assert one.value == g.select_forms()["exact"]


# ---------------------------------------------------------------- batch path
def max_lexical(scores):
    """fold(0.0, f32::max) over the scores, floored at f32::EPSILON"""
    m = max([np.float32(s) for s in scores], default=np.float32(0.0))
    return m if m >= EPS else EPS


def check_batch(g, queries, limit, flts, **kw):
    """score_batch against the reference: rows, score bits and max_lexical per query.  flts: a filter name per query"""
    got, info = g.score_batch([" ".join(q) for q in queries], limit, return_info=True, **kw)
    assert len(got) == len(queries) and info["n_single"] == 0
    for i, q in enumerate(queries):
        rows, sc = full_list(q, flts[i])
        rows, sc = rows[:limit], sc[:limit]
        ctx = (i, q, limit, flts[i])
        assert np.array_equal(got[i][0].astype(np.int64), rows), ctx
        assert np.array_equal(bits(got[i][1]), bits(sc)), ctx
        assert bits([info["max_lexical"][i]])[0] == bits([max_lexical(sc)])[0], ctx


def unfiltered_queries():
    return list(dict.fromkeys(c["query"] for c in V.cases() if not c["filter"]))


def test_batch_path_unfiltered(rlr):
    """every unfiltered query in one call: 0 keys (`major`), 50, 3000, 8192, 8193, 9000 and 14 195 keys side by side, so
    the batch's largest key count exceeds 8192 while single queries sit at and under the sort's capacity"""
    g = sel_engine(rlr).lexical
    qs = unfiltered_queries()
    n_keys = {len(full_list(q)[0]) for q in qs}
    assert {0, 50, 3000, 8192, 8193, 9000} <= n_keys and max(n_keys) > 8192
    for limit in (1, 4096, 8192):
        check_batch(g, qs, limit, [None] * len(qs))


def test_batch_path_filtered(rlr):
    g = sel_engine(rlr).lexical
    F = _shared["filters"]
    q = ("full8192", "plus1out")
    # one filter for the call: the filtered cases' query among every other query
    qs = unfiltered_queries()
    for name in V.FILTERS:
        for limit in sorted({c["limit"] for c in V.cases() if c["filter"] == name} | {8192}):
            check_batch(g, qs, limit, [name] * len(qs), filter=F[name])
    # a filter per query: the four filters of the filtered cases in one call, then mixed with other queries
    for limit in sorted({c["limit"] for c in V.cases() if c["filter"]}):
        check_batch(g, [q] * 4, limit, list(V.FILTERS), filters=[F[n] for n in V.FILTERS])
    mixed = [(qq, n) for n in V.FILTERS for qq in (q, ("major",), ("tie9000", "full8192"), ("rare50", "major"))]
    for limit in (100, 4096):
        check_batch(g, [m[0] for m in mixed], limit, [m[1] for m in mixed], filters=[F[m[1]] for m in mixed])


# ---------------------------------------------------------------- text search over the same rows
TEXTS = (("full8192", "plus1out"), ("major", "rare50"), ("major",))


def check_search(rlr, oracle, k, diversity):
    """RagEngine.search / search_with_diversity with the query text against the oracle's search given the reference's
    pairs, and the form the BM25 side took.  The engine asks BM25 for 5 * k_seen pairs (k_seen: k, or the MMR pool)"""
    eng = sel_engine(rlr)
    g = eng.lexical
    stored = _shared["stored"]
    k_seen = k if diversity == 0.0 else max(3 * k, k + 10)
    limit = 5 * k_seen
    forms = set()
    for ti, query in enumerate(TEXTS):
        q = oracle.synth_query(DIM, seed=620 + ti)
        rows, sc = full_list(query)
        pairs = [(int(r), float(s)) for r, s in zip(rows[:limit], sc[:limit])]
        before = counts(g)
        if diversity == 0.0:
            got = eng.search(q, k, query_text=" ".join(query))
            wr, wc, we, wl = oracle.search(stored, q, k, lex=pairs)
        else:
            got = eng.search_with_diversity(q, k, diversity, query_text=" ".join(query))
            wr, wc, we, wl = oracle.search_with_diversity(stored, q, k, diversity, lex=pairs)
        d_forms, d_retries = moved(g, before)
        form = V.form(V.sel_corpus().upper(query), limit)
        ctx = (query, k, diversity, form, d_forms, d_retries)
        assert [h.row for h in got] == list(wr), ctx
        assert np.array_equal(bits([h.score for h in got]), bits(wc)), ctx
        assert np.array_equal(bits([h.embedding_score for h in got]), bits(we)), ctx
        assert np.array_equal(bits([h.lexical_score for h in got]), bits(wl)), ctx
        check_retries(form, len(rows), limit, d_retries, ctx)
        assert d_forms == expect_forms(form, d_retries), ctx
        forms.add(form)
    return forms


# k -> the form behind `full8192 plus1out` .. `major` (upper 8193 .. 12 550).  The blend on the device takes at most 2048
# BM25 pairs and 4096 candidate slots (need + 2 * pairs + 8): k = 371 is the last search it serves (1855 pairs, the
# unsorted final of the sampled selection), from 372 on the pairs come through rlr_lexical_score (sorted finals).
@pytest.mark.parametrize("k,form", [(100, V.S4096), (371, V.S4096), (372, V.S4096), (819, V.S8192), (820, V.EXACT),
                                    (1024, V.EXACT), (1025, V.EXACT)])
def test_text_search(rlr, oracle, k, form):
    assert check_search(rlr, oracle, k, 0.0) == {form}


@pytest.mark.parametrize("k,form", [(123, V.S4096), (124, V.S4096), (273, V.S8192), (274, V.EXACT)])
def test_text_search_with_diversity(rlr, oracle, k, form):
    """pools 369 (the last the device blend serves), 372, 819 and 822"""
    assert check_search(rlr, oracle, k, 0.5) == {form}
