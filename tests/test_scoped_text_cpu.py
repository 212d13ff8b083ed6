"""Batched text search with a document scope per query, without a GPU: the two entry points are exported, prototyped and
documented with an array of filters; argument errors come back with stand-in handles; search_documents_batch routes the
scoped text requests of a key through ONE search_text_batch(scopes=...) only under share_text_scopes=True; and the oracle
alone clears every (scope, query, text, mode, top_k, weights) the GPU test may put into a batch, for its assertion that
the batch handed no query back."""
import ctypes as C
import importlib
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import scoped_text_vectors as SV
import text_batch_filtered_vectors as V
from oracle import lexical as OL
from test_text_batch_filtered_cpu import CpuCorpus, _combine

eng_mod = importlib.import_module("rust-local-rag_amd.engine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"rlr_lexical_score_batch_scoped": ("rlr_lexical.h", 11, r"\(lex: \*mut rlr_lexical, filters: \*const \*const rlr_filter,",
                                              r"\(rlr_lexical \*lex, const rlr_filter \*const \*filters,"),
           "rlr_engine_search_text_batch_scoped": ("rlr_engine.h", 16,
                                                   r"\(idx: \*mut rlr_index, lex: \*mut rlr_lexical, filters: \*const \*const rlr_filter,",
                                                   r"\(rlr_index \*idx, rlr_lexical \*lex, const rlr_filter \*const \*filters,")}
f32 = np.float32


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_the_entry_points_are_exported_and_documented(rlr, name):
    header, n_args, rust, c_decl = EXPORTS[name]
    N = importlib.import_module("rust-local-rag_amd._native")
    fn = getattr(rlr.lib(), name)                                 # resolves in the built library
    assert fn.restype is not None and len(fn.argtypes) == n_args  # ... and carries its ctypes prototype
    assert C.POINTER(C.c_void_p) in fn.argtypes[:3]               # the filters go in as an array of handles
    assert name in [p[0] for p in N.PROTOTYPES]
    so = os.path.join(ROOT, "rust-local-rag_amd", "librlr_gpu.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(rf"\bT {name}\b", syms)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
        assert re.search(rf"pub fn {name}{rust}", text)
        assert len(re.findall(rf"`{name}`", text)) >= 1           # ... and a paragraph that names it
    with open(os.path.join(ROOT, "include", header)) as f:
        assert re.search(rf"int32_t {name}{c_decl}", f.read())


def test_the_version_is_unchanged(rlr):
    with open(os.path.join(ROOT, "include", "rlr_gpu.h")) as f:
        assert re.search(r"#define\s+RLR_VERSION\s+121\b", f.read())


def test_argument_errors_come_back_without_a_device(rlr):
    L = rlr.lib()
    N = importlib.import_module("rust-local-rag_amd._native")
    h = C.cast(C.create_string_buffer(4096), C.c_void_p)           # a non-null stand-in: never read before the checks fail
    arr = (C.c_void_p * 2)(h.value, h.value)
    up = np.array([0, 5, 3], dtype=np.uint64)                      # decreasing
    ok = np.array([0, 2, 4], dtype=np.uint64)
    rows, sc, n = np.zeros(16, np.uint64), np.zeros(16, np.float32), np.zeros(2, np.uint32)
    p = lambda a, t: a.ctypes.data_as(t)
    lex_tail = (5, p(rows, N.u64p), p(sc, N.f32p), p(n, N.u32p), None, None)
    call = L.rlr_lexical_score_batch_scoped
    assert call(None, arr, 2, b"ab cd", p(ok, N.u64p), *lex_tail) == -1
    assert call(h, None, 2, b"ab cd", p(ok, N.u64p), *lex_tail) == -1                     # a null array
    assert b"array" in L.rlr_last_error()
    assert call(h, (C.c_void_p * 2)(None, None), 2, b"ab cd", p(ok, N.u64p), *lex_tail) == -1   # a null entry, read first
    assert call(h, arr, 2, b"ab cd", p(up, N.u64p), *lex_tail) == -1
    assert b"decrease" in L.rlr_last_error()
    assert call(h, arr, 2, b"ab cd", None, *lex_tail) == -1
    assert call(h, arr, 2, b"ab cd", p(ok, N.u64p), 0, *lex_tail[1:]) == -1               # limit 0
    assert call(h, arr, 2, b"ab cd", p(ok, N.u64p), 8193, *lex_tail[1:]) == -1
    assert call(h, arr, 2, None, p(ok, N.u64p), *lex_tail) == -1                          # null tokens
    q = np.zeros(16, np.float32)
    hits = (N.SearchHitC * 64)()
    eng_tail = (5, 0.3, 0, None, hits, 32, p(n, N.u32p), None)
    call = L.rlr_engine_search_text_batch_scoped
    assert call(None, h, arr, p(q, N.f32p), 8, 2, b"ab cd", p(ok, N.u64p), *eng_tail) == -1
    assert call(h, None, arr, p(q, N.f32p), 8, 2, b"ab cd", p(ok, N.u64p), *eng_tail) == -1
    assert call(h, h, None, p(q, N.f32p), 8, 2, b"ab cd", p(ok, N.u64p), *eng_tail) == -1  # a null array
    assert call(h, h, (C.c_void_p * 2)(None, None), p(q, N.f32p), 8, 2, b"ab cd", p(ok, N.u64p), *eng_tail) == -1
    assert call(h, h, arr, p(q, N.f32p), 8, 2, b"ab cd", p(up, N.u64p), *eng_tail) == -1
    assert call(h, h, arr, None, 8, 2, b"ab cd", p(ok, N.u64p), *eng_tail) == -1
    assert call(h, h, arr, p(q, N.f32p), 8, 2, None, p(ok, N.u64p), *eng_tail) == -1       # null tokens
    assert call(h, h, arr, p(q, N.f32p), 8, 2, b"ab cd", None, *eng_tail) == -1


# ---- routing ----------------------------------------------------------------------------------------------------------
class FakeEngine(eng_mod.RagEngine):
    """RagEngine.search_documents_batch over recorded stand-ins for the routes it may take"""

    def __init__(self):                                            # (no GPU index, no lexical index)
        self.calls = []

    def search_text_batch(self, emb, texts, top_k, div, weights=None, stage=0, return_info=False, documents=None, scopes=None):
        assert documents is None or scopes is None
        if scopes is not None:
            assert len(scopes) == len(emb) == len(texts)
            self.calls.append(("text_scopes", [float(e[0]) for e in emb], list(texts), top_k, div, weights,
                               [tuple(s) for s in scopes]))
            return [[("text_scopes", float(e[0]), tuple(s))] for e, s in zip(emb, scopes)]
        self.calls.append(("text_batch", [float(e[0]) for e in emb], list(texts), top_k, div, weights,
                           None if documents is None else tuple(documents)))
        return [[("text_batch", float(e[0]), None if documents is None else tuple(documents))] for e in emb]

    def search_with_diversity_batch(self, emb, top_k, div, weights=None, documents=None, scopes=None):
        assert documents is None or scopes is None
        if scopes is not None:
            self.calls.append(("scopes", [float(e[0]) for e in emb], top_k, div, weights, [tuple(s) for s in scopes]))
            return [[("scopes", float(e[0]), tuple(s))] for e, s in zip(emb, scopes)]
        self.calls.append(("diversity_batch", [float(e[0]) for e in emb], top_k, div, weights, tuple(documents)))
        return [[("diversity_batch", float(e[0]), tuple(documents))] for e in emb]

    def search_documents(self, request):
        self.calls.append(("single", request.query, tuple(request.documents)))
        return [("single", float(request.query_embedding[0]), tuple(request.documents))]


def requests():
    R = eng_mod.SearchRequest
    w = eng_mod.QueryWeights(embedding=1.0, lexical=0.0)
    return [
        R(query_embedding=[0.0, 1.0], query="alpha"),                                   # 0 unscoped, text
        R(query_embedding=[1.0, 1.0], documents=["a.pdf"]),                              # 1 scoped, no text
        R(query_embedding=[2.0, 1.0], query="beta", documents=["a.pdf"]),               # 2 scoped, text
        R(query_embedding=[3.0, 1.0], query="gamma", documents=["b.pdf", "a.pdf"]),     # 3 scoped, text, another scope
        R(query_embedding=[4.0, 1.0], query="", documents=["c.pdf"]),                   # 4 empty text = none
        R(query_embedding=[5.0, 1.0], query="delta", documents=[]),                     # 5 [] is a scope, not None
        R(query_embedding=[6.0, 1.0]),                                                   # 6 unscoped, no text
        R(query_embedding=[7.0, 1.0], query="eps", documents=["d.pdf"], top_k=3),       # 7 other top_k: alone under its key
        R(query_embedding=[8.0, 1.0], query="zeta", documents=["a.pdf"], weights=w),    # 8, 9 other weights
        R(query_embedding=[9.0, 1.0], query="eta", documents=["e.pdf"], weights=w),
        R(query_embedding=[10.0, 1.0], query="theta", documents=["a.pdf"]),             # 10 the scope of 2
    ]


def test_the_routing_without_the_flag_is_todays():
    for kwargs in ({}, {"share_scopes": True}, {"share_text_scopes": False}):
        e = FakeEngine()
        out = e.search_documents_batch(requests(), **kwargs)
        assert [o[0][1] for o in out] == [float(i) for i in range(11)]
        assert not [c for c in e.calls if c[0] == "text_scopes"]
        text = sorted(((c[6], tuple(c[1]), tuple(c[2])) for c in e.calls if c[0] == "text_batch"), key=repr)
        assert text == sorted([(None, (0.0, 6.0), ("alpha", "")), (("a.pdf",), (2.0, 10.0), ("beta", "theta"))], key=repr)
        assert sorted(c for c in e.calls if c[0] == "single") == sorted(
            [("single", "gamma", ("b.pdf", "a.pdf")), ("single", "delta", ()), ("single", "eps", ("d.pdf",)),
             ("single", "zeta", ("a.pdf",)), ("single", "eta", ("e.pdf",))])
        shared = [c for c in e.calls if c[0] == "scopes"]
        assert len(shared) == (1 if kwargs.get("share_scopes") else 0)


@pytest.mark.parametrize("share_scopes", [False, True])
def test_share_text_scopes_is_one_call_per_key(share_scopes):
    e = FakeEngine()
    out = e.search_documents_batch(requests(), share_scopes=share_scopes, share_text_scopes=True)
    assert [o[0][1] for o in out] == [float(i) for i in range(11)]                       # every request got ITS result
    shared = sorted(((c[3], c[5] is not None, tuple(c[1]), tuple(c[2]), tuple(c[6])) for c in e.calls if c[0] == "text_scopes"),
                    key=repr)
    assert shared == sorted([
        (5, False, (2.0, 3.0, 5.0, 10.0), ("beta", "gamma", "delta", "theta"), (("a.pdf",), ("a.pdf", "b.pdf"), (), ("a.pdf",))),
        (5, True, (8.0, 9.0), ("zeta", "eta"), (("a.pdf",), ("e.pdf",))),
    ], key=repr)
    for i, scope in ((2, ("a.pdf",)), (3, ("a.pdf", "b.pdf")), (5, ()), (10, ("a.pdf",)), (8, ("a.pdf",)), (9, ("e.pdf",))):
        assert out[i][0][0] == "text_scopes" and out[i][0][2] == scope, i                # ... inside ITS OWN scope
    assert [c for c in e.calls if c[0] == "single"] == [("single", "eps", ("d.pdf",))]   # alone under its key
    text = [(c[6], tuple(c[1]), tuple(c[2])) for c in e.calls if c[0] == "text_batch"]
    assert text == [(None, (0.0, 6.0), ("alpha", ""))]                                   # the unscoped group: untouched
    # the two flags are independent: the text-less scoped requests go where share_scopes sends them
    assert len([c for c in e.calls if c[0] == "scopes"]) == (1 if share_scopes else 0)
    assert len([c for c in e.calls if c[0] == "diversity_batch"]) == (0 if share_scopes else 2)


def test_scopes_and_documents_exclude_each_other():
    class Bare(eng_mod.RagEngine):
        def __init__(self):
            self.dim = 2
    with pytest.raises(ValueError):
        Bare().search_text_batch(np.zeros((2, 2), np.float32), ["a", "b"], 5, 0.3, documents=["a.pdf"], scopes=[["a.pdf"], []])
    with pytest.raises(ValueError):                                                      # one scope per query
        Bare().search_text_batch(np.zeros((2, 2), np.float32), ["a", "b"], 5, 0.3, scopes=[["a.pdf"]])
    lex_mod = importlib.import_module("rust-local-rag_amd.lexical")

    class BareLex(lex_mod.LexicalIndex):
        def __init__(self):
            pass

        def __del__(self):
            pass
    with pytest.raises(ValueError):
        BareLex().score_batch(["a"], 5, filter=object(), filters=[object()])


# ---- the oracle clears every engine vector ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(V.CORPORA))
def test_the_oracle_clears_every_engine_vector(oracle, name):
    """The method of test_text_batch_filtered_cpu.test_the_oracle_clears_every_engine_vector, over the FULL product the
    batches draw from: ten scopes x the query seeds a batch can reach x 8 texts x 4 modes x 3 top-ks x the weights with
    w_embedding != 0.  For each: at most 128 unique known terms, and no tie chain at the query's OWN fetch boundary
    min(|F_q|, need_q + lexical count + 8) -- the rows query q looks at, whatever the batch fetched.  Any rotation of
    scopes and texts against the slots is therefore served by the batch itself."""
    c = CpuCorpus(oracle, *V.CORPORA[name])
    for text in V.TEXTS:
        known = [t for t in dict.fromkeys(OL.tokenize(text)) if t in c.olex.term_postings]
        assert len(known) <= 128, (name, text)
    n_checked = 0
    for s, scope in enumerate(SV.SCOPES):
        allowed = c.allowed(scope)
        assert allowed.size == SV.SCOPE_ROWS[s]
        if allowed.size == 0:
            continue
        pos = {int(r): i for i, r in enumerate(allowed)}
        for i in range(SV.N_SEEDS[name]):
            q = oracle.normalize(oracle.synth_query(c.dim, V.QUERY_SEED0 + i))
            cos = oracle.scan(c.stored[allowed], q)
            cs = np.sort(cos)[::-1]
            for text in V.TEXTS:
                lexfull = [(pos[r], sc) for r, sc in c.lexical(text) if r in pos]
                for (lam, stage), k, wi in itertools.product(V.MODES, V.TOP_KS, (0, 2)):
                    _, w_e, w_l = V.WEIGHTS[wi]
                    _, limit, need = V.sizes(allowed.size, k, lam, stage)
                    lex = lexfull[:limit]
                    fetch = min(allowed.size, need + len(lex) + 8)
                    if fetch >= allowed.size:
                        continue
                    mx = max([float(sc) for _, sc in lex] + [0.0])
                    mx = f32(mx) if mx >= 1.1920929e-07 else f32(1.1920929e-07)
                    l = np.zeros(allowed.size, np.float32)
                    for r, sc in lex:
                        l[r] = f32(sc) / mx
                    comb = np.sort((f32(w_e) * cos).astype(f32) + (f32(w_l) * l).astype(f32))[::-1]
                    tail = _combine(w_e, w_l, cs[fetch - 1], 0.0)
                    assert comb[need - 1] > tail, (name, s, i, text, lam, stage, k, wi, float(comb[need - 1]), float(tail))
                    n_checked += 1
    assert n_checked > 50
