"""Postings designed for the top-`limit` selection behind the BM25 side of the text search (lexical.hip), a model of the
host's dispatch rule and a vectorised reference (test_lexsel_vectors_cpu.py proves what they reach, test_gpu_lexsel.py
runs them).  No GPU is used here.

The selection has four forms, chosen per call from `upper` (the sum of the query terms' document frequencies, capped at
the number of rows) and the limit alone:
    sort           upper <= 8192                                        lex_sort_kernel<true>
    sampled, 4096  upper > 8192, lim <= 4096, candidates(4096) <= 4000  lex_sample_kernel (sample_log2 = 12), filter, final
    sampled, 8192  ... only candidates(8192) <= 6000 holds              the same with sample_log2 = 13
    exact          otherwise, or after a retry                          8 radix passes, collect, sort or the unsorted set
What the kernels then see is n_touched, the rows whose sum became positive: equal to `upper` for one term, far below it
when terms share rows, when a term's idf clamps to 0 (it is in more than half of the documents) or under a row filter.

Corpus SEL: 24 576 rows of 24 .. 71 tokens (the rows of `tie9000` all hold 40), designed terms with tf 1 .. 3 on chosen
rows, filler words elsewhere:
    full8192          every third row, 0 .. 24 573       upper exactly the sort's capacity
    plus1out          row 12 289 (outside full8192)      `full8192 plus1out`: upper 8193, touched 8193
    plus1in           row 12 288 (inside full8192)       `full8192 plus1in`:  upper 8193, touched 8192
    tri1 tri2 tri3    the same 3000 rows                 upper 9000, touched 3000 (no power of two)
    major             12 500 rows: idf 0                 touched 0 behind a large upper
    rare50            50 rows, 25 of them in major       `major rare50` / `rare50 major`: upper 12 550, touched 50
    tie9000           9000 rows, one length, tf 1        one score class: keys differ in the row word only
"""
import ctypes
import ctypes.util
import functools

import numpy as np

F32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.argtypes = [ctypes.c_float]
_libm.logf.restype = ctypes.c_float

# ---------------------------------------------------------------- the dispatch rule, restated
SORT_CAP = 8192                # kMaxLimit: postings one workgroup sorts; also the candidate capacity and the largest limit
FAST_LIMIT_MAX = 4096          # kFastLimitMax: the largest limit of the sampled selection
SAMPLES = (4096, 8192)         # sample_log2 = 12 | 13 (kSampleMax = 8192)
CAND_SMALL, CAND_LARGE = 4000.0, 6000.0     # expected candidates the 4096-key / the 8192-key sample may promise
SORT, S4096, S8192, EXACT = "sort", "sampled_4096", "sampled_8192", "exact"
FORMS = (SORT, S4096, S8192, EXACT)
SLACK = 8                      # lex_sample_kernel: the threshold may admit up to 8 sample keys more than r


def sampled_candidates(limit, n, s):
    """expected candidates of the sampled selection, in float64 and in the order the host computes it"""
    return float(limit) + 4.5 * np.sqrt(float(limit) * n / s) + 8.0 * float(n) / s


def served_limit(limit):
    return SORT_CAP if limit == 0 else min(limit, SORT_CAP)


def form(upper, limit):
    lim = served_limit(limit)
    if upper <= SORT_CAP:
        return SORT
    if lim <= FAST_LIMIT_MAX and sampled_candidates(lim, upper, SAMPLES[1]) <= CAND_LARGE:
        return S4096 if sampled_candidates(lim, upper, SAMPLES[0]) <= CAND_SMALL else S8192
    return EXACT


def sample_model(n_touched, limit, size):
    """what lex_sample_kernel works with: s sample keys, mu expected hits, the rank r of the threshold (f32, as the
    kernel), `whole`: the sample is the touched list itself (the selection is then deterministic), `all_wanted`: thr = 0"""
    lim = served_limit(limit)
    s = min(n_touched, size)
    if lim >= n_touched or s == 0:
        return dict(s=s, mu=None, r=None, whole=s == n_touched, all_wanted=True)
    mu = F32(lim) * F32(s) / F32(n_touched)
    r = min(s, int(F32(mu + F32(4.5) * np.sqrt(mu))) + 8)
    return dict(s=s, mu=float(mu), r=r, whole=s == n_touched, all_wanted=False)


# ---------------------------------------------------------------- a corpus and the reference
def normal(tokens):
    """the tokens a chunk or a query keeps: 3 bytes and more, lower case (the tokens here are alphanumeric already)"""
    return [t.lower() for t in tokens if len(t.encode("utf-8")) >= 3]


class Corpus:
    """rows given as token lists -> postings per term (rows ascending, tf), document lengths, totals"""

    def __init__(self, rows_tokens):
        self.n = len(rows_tokens)
        self.doc_len = np.zeros(self.n, np.int64)
        rows, tfs = {}, {}
        for r, toks in enumerate(rows_tokens):
            counts = {}
            for t in normal(toks):
                counts[t] = counts.get(t, 0) + 1
            self.doc_len[r] = sum(counts.values())
            for t, c in counts.items():
                rows.setdefault(t, []).append(r)
                tfs.setdefault(t, []).append(c)
        self.post = {t: (np.array(rows[t], np.int64), np.array(tfs[t], np.int64)) for t in rows}
        self.total_docs = int((self.doc_len > 0).sum())
        self.total_length = int(self.doc_len.sum())

    def df(self, term):
        return len(self.post[term][0]) if term in self.post else 0

    def known_terms(self, query_tokens):
        """the query's known terms, once each, in order of first occurrence"""
        return [t for t in dict.fromkeys(normal(query_tokens)) if t in self.post]

    def upper(self, query_tokens):
        return min(sum(self.df(t) for t in self.known_terms(query_tokens)), self.n)


def term_scores(corpus, query_tokens, allowed=None):
    """per known term of the query, in order: (rows, f32 contributions), the operations of oracle/lexical.py::score on f32
    arrays; `allowed` (a boolean array over the rows) drops the other rows' postings"""
    if corpus.total_docs == 0:
        return []
    avg = F32(corpus.total_length) / F32(corpus.total_docs)
    k1, b = F32(1.5), F32(0.75)
    out = []
    for term in corpus.known_terms(query_tokens):
        rows, tf_i = corpus.post[term]
        df = F32(len(rows))
        ratio = (F32(corpus.total_docs) - df + F32(0.5)) / (df + F32(0.5))
        idf = F32(_libm.logf(float(ratio)))
        idf = idf if idf > 0 else F32(0.0)
        if allowed is not None:
            keep = allowed[rows]
            rows, tf_i = rows[keep], tf_i[keep]
        dl = corpus.doc_len[rows].astype(np.float32)
        tf = tf_i.astype(np.float32)
        denom = tf + k1 * (F32(1.0) - b + b * (dl / avg))
        ok = (dl != 0) & (denom != 0)
        s = (idf * (tf[ok] * (k1 + F32(1.0))) / denom[ok]).astype(np.float32)
        out.append((rows[ok], s))
    return out


def bm25_reference(corpus, query_tokens, limit, allowed=None):
    """-> (rows int64, scores f32): the positive sums ordered (score desc, row asc), cut to `limit` (0: all of them)"""
    if allowed is not None:                                 # (a set or an array of allowed rows)
        mask = np.zeros(corpus.n, bool)
        mask[np.asarray(sorted(allowed), np.int64)] = True
        allowed = mask
    scores = np.zeros(corpus.n, np.float32)
    for rows, s in term_scores(corpus, query_tokens, allowed):
        scores[rows] = scores[rows] + s                     # (a term holds a row once: no repeated index)
    rows = np.flatnonzero(scores > 0)
    order = np.lexsort((rows, -scores[rows].astype(np.float64)))
    rows = rows[order]
    if limit > 0:
        rows = rows[:limit]
    return rows, scores[rows]


# ---------------------------------------------------------------- SEL
N_ROWS = 24576
TIE_LEN = 40
LENGTHS = np.arange(24, 72)
N_FILLER = 300
ROW_OUT, ROW_IN = 12289, 12288


@functools.lru_cache(maxsize=1)
def sel_design():
    """-> {term: (rows ascending, tf)} and the document lengths of SEL"""
    rng = np.random.default_rng(20240607)
    n = N_ROWS
    every = np.arange(n)
    d = {}

    def put(term, rows, tf=None):
        rows = np.sort(np.asarray(rows, np.int64))
        d[term] = (rows, rng.integers(1, 4, size=len(rows)) if tf is None else np.full(len(rows), tf, np.int64))

    put("full8192", every[::3])
    put("plus1out", [ROW_OUT])
    put("plus1in", [ROW_IN])
    tri = rng.choice(n, size=3000, replace=False)
    for t in ("tri1", "tri2", "tri3"):
        put(t, tri)
    major = rng.choice(n - 1, size=12500, replace=False)                  # (row n - 1 stays outside: rare50's last row)
    put("major", major)
    outside = np.setdiff1d(every[: n - 1], major)
    put("rare50", np.r_[rng.choice(major, size=25, replace=False), rng.choice(outside, size=24, replace=False), n - 1])
    put("tie9000", rng.choice(n, size=9000, replace=False), tf=1)
    doc_len = rng.choice(LENGTHS, size=n)
    doc_len[d["tie9000"][0]] = TIE_LEN
    return d, doc_len


@functools.lru_cache(maxsize=1)
def sel_rows():
    """SEL as token lists (a tuple of tuples: shared, not to be changed)"""
    d, doc_len = sel_design()
    rng = np.random.default_rng(20240608)
    filler = [f"fil{i:03d}w" for i in range(N_FILLER)]
    rows = [[] for _ in range(N_ROWS)]
    for term, (at, tf) in d.items():
        for r, c in zip(at.tolist(), tf.tolist()):
            rows[r] += [term] * c
    for r in range(N_ROWS):
        need = int(doc_len[r]) - len(rows[r])
        assert need >= 1, "a row's designed terms leave no room for filler"
        rows[r] += [filler[i] for i in rng.integers(0, N_FILLER, size=need)]
    return tuple(tuple(rng.permutation(toks).tolist()) for toks in rows)


@functools.lru_cache(maxsize=1)
def sel_corpus():
    return Corpus(sel_rows())


def sel_texts():
    return [" ".join(toks) for toks in sel_rows()]


# ---------------------------------------------------------------- the cases
def switch_limits(upper):
    """the last limit the 4096-key sample takes at `upper` and the first the 8192-key sample takes, by the model"""
    lims = [lim for lim in range(1, FAST_LIMIT_MAX + 1) if form(upper, lim) == S4096]
    last = max(lims)
    assert lims == list(range(1, last + 1)) and form(upper, last + 1) == S8192
    return last, last + 1


FILTERS = ("hundred", "every", "high", "none")


@functools.lru_cache(maxsize=1)
def sel_filters():
    """name -> allowed rows (ascending) of the filtered cases over `full8192 plus1out`"""
    d, _ = sel_design()
    rng = np.random.default_rng(20240609)
    posted = np.union1d(d["full8192"][0], d["plus1out"][0])
    return {"hundred": np.sort(np.r_[rng.choice(posted[1:-1], size=98, replace=False), posted[0], posted[-1]]),
            "every": np.arange(N_ROWS), "high": np.arange(24000, N_ROWS), "none": np.arange(N_ROWS)[2::3]}


@functools.lru_cache(maxsize=1)
def cases():
    """-> list of dicts: name, query (a token tuple), limit, upper, n_touched, form, filter (a name of sel_filters or None).
    upper and n_touched are what the design promises; the CPU test holds them to the corpus as built."""
    out = []

    def add(query, upper, n_touched, limits, flt=None):
        for lim in limits:
            name = query.replace(" ", "+") + (f"|{flt}" if flt else "") + f"@{lim}"
            out.append(dict(name=name, query=tuple(query.split()), limit=lim, upper=upper, n_touched=n_touched,
                            form=form(upper, lim), filter=flt))

    add("full8192", 8192, 8192, (1, 4096, 8191, 8192, 0))
    last12, first13 = switch_limits(8193)
    for q, touched in (("full8192 plus1out", 8193), ("full8192 plus1in", 8192)):
        add(q, 8193, touched, (1, 100, last12, first13, 4096, 4097, 8191, 8192, 0))
    add("tri1 tri2 tri3", 9000, 3000, (1, 2999, 3000, 3001, 4096, 4097, 0))
    add("major", 12500, 0, (10, 5000))
    for q in ("major rare50", "rare50 major"):
        add(q, 12550, 50, (10, 49, 50, 51, 4096, 4097))
    add("tie9000", 9000, 9000, (1, 100, 4096, 4097, 8192))
    d, _ = sel_design()
    both = len(np.union1d(d["tie9000"][0], d["full8192"][0]))
    add("tie9000 full8192", 17192, both, (300,))
    f = sel_filters()
    posted = np.union1d(d["full8192"][0], d["plus1out"][0])
    add("full8192 plus1out", 8193, 100, (99, 100, 101), "hundred")
    add("full8192 plus1out", 8193, 8193, (4096,), "every")
    add("full8192 plus1out", 8193, len(np.intersect1d(posted, f["high"])), (50,), "high")
    add("full8192 plus1out", 8193, 0, (10,), "none")
    return tuple(out)


def reference(case):
    """the expected (rows, scores) of a case: at most 8192 pairs, as the library serves limit 0"""
    allowed = sel_filters()[case["filter"]] if case["filter"] else None
    return _reference(case["query"], case["filter"], served_limit(case["limit"]), allowed)


@functools.lru_cache(maxsize=None)
def full_list(query, flt):
    allowed = sel_filters()[flt] if flt else None
    rows, sc = bm25_reference(sel_corpus(), list(query), 0, allowed)
    rows.setflags(write=False)
    sc.setflags(write=False)
    return rows, sc


def _reference(query, flt, lim, allowed):
    rows, sc = full_list(query, flt)                            # one scoring pass per (query, filter), shared by the limits
    return rows[:lim], sc[:lim]
