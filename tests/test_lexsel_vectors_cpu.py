"""The designed postings of lexsel_vectors.py checked without a GPU:
  1  the corpus holds what its table promises (document frequencies, upper and n_touched of every case, computed from the
     rows as built), every form of the selection is expected by three cases and more, both sides of the three switches
     (upper 8192 | 8193, limit 4096 | 4097, 4096 | 8192 sample keys) are present, and the five constants of the dispatch
     model are the ones lexical.hip holds
  2  bm25_reference is oracle/lexical.py bit for bit (a 600-row cut for every query, the full corpus for one query per term
     group) and reproduces tests/golden/bm25_vectors.json
  3  sensitivity proof: the selection chain restated in plain Python on 64-bit keys returns the reference on every case
     as written -- with the touched list in row order and shuffled, with the sample rank of the design and with the
     forced rank 1 of the retry test -- and with each of eight defects planted the answer or the retry decision of a
     named case changes
"""
import json
import os
import re

import numpy as np
import pytest

import lexsel_vectors as V
from oracle import lexical as OL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- 1: designed properties
def test_corpus_holds_what_its_table_promises():
    rows = V.sel_rows()
    c = V.sel_corpus()
    assert len(rows) == V.N_ROWS == c.n == c.total_docs
    assert {t: c.df(t) for t in ("full8192", "plus1out", "plus1in", "tri1", "tri2", "tri3", "major", "rare50", "tie9000")} == \
        dict(full8192=8192, plus1out=1, plus1in=1, tri1=3000, tri2=3000, tri3=3000, major=12500, rare50=50, tie9000=9000)
    full = c.post["full8192"][0]
    assert full[0] == 0 and full[-1] == (V.N_ROWS - 1) // 3 * 3 and len(np.unique(full // 2048)) == 12   # every 2048-row slice
    assert c.post["plus1out"][0][0] not in set(full) and c.post["plus1in"][0][0] in set(full)
    assert np.array_equal(c.post["tri1"][0], c.post["tri2"][0]) and np.array_equal(c.post["tri1"][0], c.post["tri3"][0])
    assert 2 * c.df("major") > c.total_docs                               # idf clamps to 0
    rare, major = c.post["rare50"][0], set(c.post["major"][0].tolist())
    assert 20 <= sum(int(r) in major for r in rare) <= 30 and rare[-1] == V.N_ROWS - 1
    tie_rows, tie_tf = c.post["tie9000"]
    assert set(c.doc_len[tie_rows]) == {V.TIE_LEN} and set(tie_tf) == {1}
    for t in ("full8192", "tri1", "tri2", "tri3", "major", "rare50"):
        assert set(c.post[t][1]) == {1, 2, 3}, t
    assert not np.array_equal(c.post["tri1"][1], c.post["tri2"][1])
    # document lengths: 40 values and more, not monotone in the row number, spread over the rows
    assert len(set(c.doc_len.tolist())) >= 40
    d = np.diff(c.doc_len)
    assert (d > 0).sum() > V.N_ROWS // 4 and (d < 0).sum() > V.N_ROWS // 4
    assert all(len(set(c.doc_len[i: i + 2048].tolist())) >= 40 for i in range(0, V.N_ROWS, 2048))
    assert all(len(t.encode()) >= 3 for toks in rows[:500] for t in toks)


def test_cases_hold_their_upper_and_touched():
    c = V.sel_corpus()
    flt = V.sel_filters()
    names = set()
    for case in V.cases():
        assert case["name"] not in names
        names.add(case["name"])
        assert c.upper(case["query"]) == case["upper"], case["name"]
        allowed = flt[case["filter"]] if case["filter"] else None
        touched = len(V.bm25_reference(c, case["query"], 0, allowed)[0])
        assert touched == case["n_touched"], (case["name"], touched)
        rows, sc = V.reference(case)
        assert len(rows) == min(V.served_limit(case["limit"]), touched) and (sc > 0).all()
        assert case["form"] == V.form(case["upper"], case["limit"])
    assert len(flt["hundred"]) == 100 and flt["none"].size and flt["every"].size == V.N_ROWS
    assert {c_["n_touched"] for c_ in V.cases()} >= {0, 50, 100, 3000, 8192, 8193, 9000}
    # one score class: the answer is the lowest rows
    tie = next(c_ for c_ in V.cases() if c_["name"] == "tie9000@4096")
    rows, sc = V.reference(tie)
    assert np.array_equal(rows, c.post["tie9000"][0][:4096]) and len(set(bits(sc))) == 1


def test_every_form_and_both_sides_of_every_switch():
    cs = V.cases()
    for f in V.FORMS:
        assert sum(c["form"] == f for c in cs) >= 3, f
    by = {(c["upper"], c["limit"]): c["form"] for c in cs if not c["filter"]}
    assert by[(8192, 8192)] == V.SORT and by[(8192, 1)] == V.SORT                         # upper 8192 | 8193
    assert by[(8193, 1)] == V.S4096 and by[(8193, 8192)] == V.EXACT
    assert by[(8193, 4096)] == V.S8192 and by[(8193, 4097)] == V.EXACT                    # limit 4096 | 4097
    assert by[(9000, 4096)] == V.S8192 and by[(9000, 4097)] == V.EXACT
    last12, first13 = V.switch_limits(8193)                                              # 4096 | 8192 sample keys
    assert first13 == last12 + 1 and by[(8193, last12)] == V.S4096 and by[(8193, first13)] == V.S8192
    assert 3400 < last12 < 4096
    # the shapes of the sample: whole and not a power of two, whole behind the 8192-key launch, strided with both sizes,
    # empty, everything wanted, r capped at s
    shapes = set()
    for c in cs:
        if c["form"] in (V.S4096, V.S8192):
            m = V.sample_model(c["n_touched"], c["limit"], 4096 if c["form"] == V.S4096 else 8192)
            pow2 = m["s"] & (m["s"] - 1) == 0
            shapes.add((c["form"], m["whole"], m["all_wanted"], pow2, m["s"] == 0, m["r"] == m["s"]))
    assert (V.S4096, True, False, False, False, False) in shapes         # s == n, no power of two, a real threshold
    assert (V.S4096, True, False, False, False, True) in shapes          # ... with r capped at s
    assert (V.S4096, True, True, False, False, False) in shapes          # thr = 0
    assert (V.S8192, True, True, False, False, False) in shapes
    assert (V.S8192, True, False, True, False, False) in shapes          # 8192 of 8192
    assert (V.S4096, False, False, True, False, False) in shapes and (V.S8192, False, False, True, False, False) in shapes
    assert (V.S4096, True, True, True, True, False) in shapes            # n_touched = 0
    assert any(c["form"] == V.EXACT and c["n_touched"] == 0 for c in cs)
    assert any(c["form"] == V.EXACT and c["n_touched"] == 8192 == V.served_limit(c["limit"]) for c in cs)


def test_model_constants_are_the_sources():
    src = open(os.path.join(ROOT, "rust-local-rag_amd", "csrc", "lexical.hip")).read()
    m = re.search(r"constexpr uint32_t kSampleMax = (\d+), kFastLimitMax = (\d+);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (V.SAMPLES[1], V.FAST_LIMIT_MAX)
    m = re.search(r"constexpr uint32_t kMaxLimit = (?:RLR_LEXICAL_MAX_LIMIT|(\d+))", src)
    assert m
    if m.group(1) is None:
        hdr = open(os.path.join(ROOT, "include", "rlr_lexical.h")).read()
        m = re.search(r"#define RLR_LEXICAL_MAX_LIMIT (\d+)", hdr)
    assert int(m.group(1)) == V.SORT_CAP
    assert re.search(r"if \(upper <= kMaxLimit\) \{", src)
    m = re.search(r"lim <= kFastLimitMax && sampled_candidates\(lim, upper, kSampleMax\) <= ([0-9.]+)\)", src)
    assert m and float(m.group(1)) == V.CAND_LARGE
    m = re.search(r"sample_log2 = sampled_candidates\(lim, upper, (\d+)\) <= ([0-9.]+) \? (\d+)u : (\d+)u;", src)
    assert m and int(m.group(1)) == V.SAMPLES[0] and float(m.group(2)) == V.CAND_SMALL
    assert (1 << int(m.group(3)), 1 << int(m.group(4))) == V.SAMPLES
    m = re.search(r"return static_cast<double>\(limit\) \+ ([0-9.]+) \* std::sqrt\(static_cast<double>\(limit\) \* n / s\) \+ "
                  r"([0-9.]+) \* static_cast<double>\(n\) / s;", src)
    assert m and (float(m.group(1)), float(m.group(2))) == (4.5, 8.0)
    m = re.search(r"lds_kth_key64\(s_k, s, r, s_hist, s_pick, 1024, /\*slack=\*/(\d+), row_bits\)", src)
    assert m and int(m.group(1)) == V.SLACK


# ---------------------------------------------------------------- 2: the reference
def oracle_of(rows_tokens):
    o = OL.LexicalIndex()
    for r, toks in enumerate(rows_tokens):
        o.add_chunk(r, " ".join(toks), rank=r)
    return o


def same(got, want, ctx):
    assert [int(r) for r in got[0]] == [c for c, _ in want], ctx
    assert np.array_equal(bits(got[1]), bits([s for _, s in want])), ctx


def test_reference_is_the_oracle_on_a_cut():
    """600 rows, every 41st of SEL (rows of every designed term among them), every query and limit of the case list"""
    cut = V.sel_rows()[::41]
    assert len(cut) == 600
    c, o = V.Corpus(cut), oracle_of(cut)
    assert (c.total_docs, c.total_length) == (o.total_docs, o.total_length)
    n_pairs = 0
    for query in sorted({case["query"] for case in V.cases()}) + [("major", "major", "tri2", "unknownword", "tri1", "of")]:
        full = o.score(" ".join(query), 0, keep_zero=False)
        for limit in sorted({case["limit"] for case in V.cases()}):
            same(V.bm25_reference(c, query, limit), full[:limit] if limit else full, (query, limit))
        allowed = set(range(0, 600, 7))
        same(V.bm25_reference(c, query, 20, allowed), [p for p in full if p[0] in allowed][:20], (query, "filtered"))
        n_pairs += len(full)
    assert n_pairs > 1000                                    # (the cut holds a twelfth of full8192's rows, a ninth of tie9000's)
    assert V.bm25_reference(V.Corpus([]), ("major",), 5)[0].size == 0
    assert V.bm25_reference(c, (), 5)[0].size == 0 and V.bm25_reference(c, ("ab", "zz"), 5)[0].size == 0


def test_reference_is_the_oracle_on_the_full_corpus():
    o = oracle_of(V.sel_rows())
    c = V.sel_corpus()
    for query in (("full8192", "plus1out"), ("tri1", "tri2", "tri3"), ("major", "rare50"), ("tie9000",)):
        full = o.score(" ".join(query), 0, keep_zero=False)
        assert len(full) >= 50
        same(V.bm25_reference(c, query, 0), full, query)


def test_reference_reproduces_the_golden_bm25_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "bm25_vectors.json")) as f:
        doc = json.load(f)
    n_pos = 0
    for case in doc["cases"]:
        c = V.Corpus(case["docs"])
        for q in case["queries"]:
            rows, sc = V.bm25_reference(c, q["terms"], q["limit"])
            assert rows.tolist() == q["rows"], (case["name"], q["terms"])
            assert bits(sc).tolist() == q["score_bits"], (case["name"], q["terms"])
            n_pos += len(rows)
    assert n_pos >= 50


# ---------------------------------------------------------------- 3: the chain in plain Python, with planted defects
DEFECTS = {
    "score_word": "threshold and k-th comparison on the score word alone",
    "gt": "> for >= at the k-th key",
    "want_limit": "want = limit instead of min(limit, n_touched)",
    "stride12": "sample index (i * n) >> 12 used with the 8192-key sample",
    "accept_short": "a short candidate list accepted as complete",
    "cap8191": "candidate capacity 8191",
    "first_term": "the first-touch flag taken from the first term instead of from the sum becoming positive",
    "stale_n_sel": "n_sel left from the previous call",
}
MASK32 = 0xFFFFFFFF


def touched_keys(case, order, defect):
    """the touched list of a case as 64-bit (score, row) keys: accumulate per term, flag a row when its sum becomes
    positive (old == 0 and now > 0); order: "rows" or a seed for a shuffle"""
    c = V.sel_corpus()
    allowed = None
    if case["filter"]:
        allowed = np.zeros(c.n, bool)
        allowed[V.sel_filters()[case["filter"]]] = True
    scores = np.zeros(c.n, np.float32)
    flagged = []
    for ti, (rows, s) in enumerate(V.term_scores(c, case["query"], allowed)):
        old = scores[rows]
        now = old + s
        scores[rows] = now
        flag = np.full(len(rows), ti == 0) if defect == "first_term" else (old == 0) & (now > 0)
        flagged.append(rows[flag])
    at = np.concatenate(flagged) if flagged else np.zeros(0, np.int64)
    at = np.sort(at) if order == "rows" else np.random.default_rng(order).permutation(np.sort(at))
    word = bits(scores[at]).astype(np.uint64) | np.uint64(0x80000000)     # score_key of a sum >= +0.0
    keys = (word << np.uint64(32)) | (np.uint64(MASK32) - at.astype(np.uint64))
    return [int(k) for k in keys]


def ge(a, b, defect):
    return (a >> 32) >= (b >> 32) if defect == "score_word" else a >= b


def run_chain(case, keys, state, defect, r_forced=0):
    """-> (result keys in order, retried, forms launched).  state: what one workspace keeps between calls (the candidate /
    selection buffer and, with the stale_n_sel defect, its count).  r_forced: RLR_LEX_SAMPLE_RANK, the sample rank the
    retry test forces (1: the largest sample key is the threshold and the candidate list comes out short)"""
    cap = 8191 if defect == "cap8191" else V.SORT_CAP
    lim = V.served_limit(case["limit"])
    n = len(keys)
    want = lim if defect == "want_limit" else min(lim, n)
    f = V.form(case["upper"], case["limit"])
    forms = [f]
    if f == V.SORT:
        return sorted(keys[:cap], reverse=True)[: min(n, lim)], False, forms
    retried = False
    if f in (V.S4096, V.S8192):
        log2 = 12 if f == V.S4096 else 13
        s = min(n, 1 << log2)
        if lim >= n or s == 0:
            thr = 0
        else:
            shift = 12 if defect == "stride12" else log2
            at = [i if s == n else (i * n) >> shift for i in range(s)]
            sample = [keys[i] if i < n else 0 for i in at]                # (a slot behind the list: nothing a key is above)
            r = min(s, r_forced) if r_forced else V.sample_model(n, case["limit"], 1 << log2)["r"]
            thr = sorted(sample, reverse=True)[r - 1]
        cand = [k for k in keys if ge(k, thr, defect)]
        m = len(cand)
        short = m < want and defect != "accept_short"
        if m > cap or short:
            retried = True
            forms.append(V.EXACT)
        else:
            kth = sorted(cand, reverse=True)[want - 1] if m > want else 0
            win = [k for k in cand if (k > kth if defect == "gt" else ge(k, kth, defect))]
            return sorted(win, reverse=True)[:want], False, forms
    # exact: the k-th key over all touched keys, collect into the selection buffer, sort
    k = min(want, n) if defect == "want_limit" else want                  # (a rank past the list ends on the lowest key)
    kth = sorted(keys, reverse=True)[k - 1] if k else 1 << 64
    taken = [key for key in keys if (key > kth if defect == "gt" else ge(key, kth, defect))]
    n_sel = state["n_sel"] if defect == "stale_n_sel" else 0
    sel = state["sel"]
    for key in taken:
        if n_sel < cap:
            sel[n_sel] = key
        n_sel += 1
    state["n_sel"] = n_sel
    return sorted(sel[: min(n_sel, cap)], reverse=True)[: min(n_sel, lim)], retried, forms


REGIMES = [(order, r_forced) for r_forced in (0, 1) for order in ("rows", 7)]


def run_all(defect, order, r_forced=0):
    state = dict(n_sel=0, sel=[0] * V.SORT_CAP)
    out = {}
    for case in V.cases():
        keys = touched_keys(case, order, defect)
        out[case["name"]] = run_chain(case, keys, state, defect, r_forced)
    return out


def expected_keys(case):
    rows, sc = V.reference(case)
    word = bits(sc).astype(np.uint64) | np.uint64(0x80000000)
    return [int(k) for k in (word << np.uint64(32)) | (np.uint64(MASK32) - rows.astype(np.uint64))]


@pytest.fixture(scope="module")
def as_written():
    return {regime: run_all(None, *regime) for regime in REGIMES}


def test_chain_as_written_returns_the_reference(as_written):
    for (order, r_forced), res in as_written.items():
        n_forms = dict.fromkeys(V.FORMS, 0)
        for case in V.cases():
            got, retried, forms = res[case["name"]]
            ctx = (order, r_forced, case["name"])
            assert got == expected_keys(case), ctx
            assert forms[0] == case["form"] and forms[1:] == [V.EXACT] * retried
            if not r_forced:
                assert not retried, ctx                     # the sample as designed misjudges none of these lists
            elif case["form"] in (V.S4096, V.S8192):
                m = V.sample_model(case["n_touched"], case["limit"], 4096 if case["form"] == V.S4096 else 8192)
                if m["whole"]:                              # one candidate, the best key: short for every limit but 1
                    assert retried == (not m["all_wanted"] and case["limit"] > 1), ctx
            for f in forms:
                n_forms[f] += 1
        assert all(n_forms[f] >= 3 for f in V.FORMS), n_forms


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_every_planted_defect_is_caught(as_written, defect):
    caught = {}
    for regime in REGIMES:
        res = run_all(defect, *regime)
        for case in V.cases():
            got, retried, _ = res[case["name"]]
            base = as_written[regime][case["name"]]
            how = ("answer" if got != base[0] else "") + ("+retry" if retried != base[1] else "")
            if how:
                caught.setdefault(case["name"], set()).add(how.lstrip("+") + (" (forced rank)" if regime[1] else ""))
    print(f"\n{defect} ({DEFECTS[defect]}): caught by {len(caught)} cases")
    for name in sorted(caught):
        print(f"    {name}: {', '.join(sorted(caught[name]))}")
    assert caught, f"no designed case notices: {DEFECTS[defect]}"
