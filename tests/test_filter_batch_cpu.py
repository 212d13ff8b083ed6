"""Batched document-scoped search without a GPU: the new entry point is exported and documented, and
RagEngine.search_documents_batch routes every request by its scope -- `documents` is part of the group key, and an empty
list is a scope of its own ("no rows"), not "no filter"."""
import importlib
import os
import re
import subprocess

import numpy as np

eng_mod = importlib.import_module("rust-local-rag_amd.engine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORT = "rlr_engine_search_with_diversity_batch_filtered"


def test_the_entry_point_is_exported_and_documented(rlr):
    fn = getattr(rlr.lib(), EXPORT)                              # resolves in the built library
    assert fn.restype is not None and len(fn.argtypes) == 11     # ... and carries its ctypes prototype
    so = os.path.join(ROOT, "rust-local-rag_amd", "librlr_gpu.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(rf"\bT {EXPORT}\b", syms)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert re.search(rf"pub fn {EXPORT}\(idx: \*mut rlr_index, f: \*const rlr_filter,", doc)
    with open(os.path.join(ROOT, "include", "rlr_engine.h")) as f:
        assert re.search(rf"int32_t {EXPORT}\(rlr_index \*idx, const rlr_filter \*f,", f.read())


class FakeEngine(eng_mod.RagEngine):
    """RagEngine.search_documents_batch over recorded stand-ins for the three routes it may take"""

    def __init__(self):                                          # (no GPU index, no lexical index)
        self.calls = []

    def search_text_batch(self, emb, texts, top_k, div, weights=None, stage=0, return_info=False):
        self.calls.append(("text_batch", len(emb), list(texts), top_k, div, weights))
        return [[("text_batch", float(e[0]))] for e in emb]

    def search_with_diversity_batch(self, emb, top_k, div, weights=None, documents=None):
        self.calls.append(("diversity_batch", len(emb), top_k, div, weights, documents))
        return [[("diversity_batch", float(e[0]), tuple(documents))] for e in emb]

    def search_documents(self, request):
        self.calls.append(("single", request.query, tuple(request.documents)))
        return [("single", float(request.query_embedding[0]), tuple(request.documents))]


def test_documents_are_part_of_the_group_key():
    R = eng_mod.SearchRequest
    w = eng_mod.QueryWeights(embedding=1.0, lexical=0.0)
    reqs = [
        R(query_embedding=[0.0, 1.0], query="alpha"),                                   # 0 unscoped, text
        R(query_embedding=[1.0, 1.0], documents=["a.pdf"]),                              # 1 scoped, no text
        R(query_embedding=[2.0, 1.0], query="beta", documents=["a.pdf"]),               # 2 scoped, text: one by one
        R(query_embedding=[3.0, 1.0], documents=["b.pdf", "a.pdf"]),                     # 3 another scope
        R(query_embedding=[4.0, 1.0], query="", documents=["a.pdf"]),                   # 4 scoped, empty text = no text
        R(query_embedding=[5.0, 1.0], documents=[]),                                     # 5 [] is a scope, not None
        R(query_embedding=[6.0, 1.0]),                                                   # 6 unscoped, no text
        R(query_embedding=[7.0, 1.0], documents=["a.pdf", "b.pdf"]),                     # 7 the scope of 3, other order
        R(query_embedding=[8.0, 1.0], documents=["a.pdf"], top_k=3),                     # 8 same scope, other top_k
        R(query_embedding=[9.0, 1.0], documents=["a.pdf"], weights=w),                   # 9 same scope, other weights
    ]
    e = FakeEngine()
    out = e.search_documents_batch(reqs)
    assert [o[0][1] for o in out] == [float(i) for i in range(10)]                       # every request got ITS result
    assert [o[0][0] for o in out] == ["text_batch", "diversity_batch", "single", "diversity_batch", "diversity_batch",
                                      "diversity_batch", "text_batch", "diversity_batch", "diversity_batch", "diversity_batch"]
    # scoped results carry their own scope: none was searched over the whole corpus or over another request's documents
    assert out[1][0][2] == ("a.pdf",) and out[4][0][2] == ("a.pdf",) and out[2][0][2] == ("a.pdf",)
    assert out[3][0][2] == ("a.pdf", "b.pdf") and out[7][0][2] == ("a.pdf", "b.pdf")
    assert out[5][0][2] == ()
    text = [c for c in e.calls if c[0] == "text_batch"]
    assert len(text) == 1 and text[0][1] == 2 and text[0][2] == ["alpha", ""]          # 0 and 6 together, nothing scoped
    div = [c for c in e.calls if c[0] == "diversity_batch"]
    by_scope = {(tuple(c[5]), c[2], c[4] is not None): c[1] for c in div}
    assert by_scope == {(("a.pdf",), 5, False): 2, (("a.pdf", "b.pdf"), 5, False): 2, ((), 5, False): 1,
                        (("a.pdf",), 3, False): 1, (("a.pdf",), 5, True): 1}
    assert [c for c in e.calls if c[0] == "single"] == [("single", "beta", ("a.pdf",))]


def test_an_unscoped_batch_runs_as_before():
    R = eng_mod.SearchRequest
    e = FakeEngine()
    out = e.search_documents_batch([R(query_embedding=[float(i), 0.0], query=f"t{i}") for i in range(4)])
    assert e.calls == [("text_batch", 4, ["t0", "t1", "t2", "t3"], eng_mod.N.DEFAULT_TOP_K, eng_mod.N.DEFAULT_DIVERSITY, None)]
    assert [o[0][1] for o in out] == [0.0, 1.0, 2.0, 3.0]
