"""Queries with a scope EACH without a GPU: rlr_search_topk_scoped and rlr_engine_search_with_diversity_batch_scoped are
exported, prototyped and documented; their argument errors come back before any device is touched; and
RagEngine.search_documents_batch routes as it always did unless share_scopes=True, which sends the text-less scoped
requests of one (top_k, diversity, weights) key through ONE search_with_diversity_batch(scopes=...) call."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

eng_mod = importlib.import_module("rust-local-rag_amd.engine")
native = importlib.import_module("rust-local-rag_amd._native")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPK, ENGINE = "rlr_search_topk_scoped", "rlr_engine_search_with_diversity_batch_scoped"


@pytest.mark.parametrize("name,n_args,header", [(TOPK, 9, "rlr_gpu.h"), (ENGINE, 11, "rlr_engine.h")])
def test_the_entry_points_are_exported_prototyped_and_documented(rlr, name, n_args, header):
    proto = {n: (res, args) for n, res, args in native.PROTOTYPES}
    assert name in proto and len(proto[name][1]) == n_args
    assert proto[name][1][1] == C.POINTER(C.c_void_p)              # the second argument is an ARRAY of filter handles
    fn = getattr(rlr.lib(), name)
    assert fn.restype is C.c_int32 and len(fn.argtypes) == n_args
    so = os.path.join(ROOT, "rust-local-rag_amd", "librlr_gpu.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(rf"\bT {name}\b", syms)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert re.search(rf"pub fn {name}\(idx: \*mut rlr_index, filters: \*const \*const rlr_filter,", f.read())
    with open(os.path.join(ROOT, "include", header)) as f:
        assert re.search(rf"int32_t {name}\(rlr_index \*idx, const rlr_filter \*const \*filters,", f.read())


def test_the_version_did_not_move(rlr):
    assert rlr.lib().rlr_version() == 121


def test_argument_errors_come_back_without_a_device(rlr):
    """no index can exist without a device, and none is needed: a null filter array and a null index handle are refused
    before anything is dereferenced"""
    L = rlr.lib()
    q = np.zeros(8, np.float32)
    rows, cos, n = np.zeros(4, np.uint64), np.zeros(4, np.float32), np.full(2, 77, np.uint32)
    tail = (q.ctypes.data_as(native.f32p), 1, 4, -1.0, rows.ctypes.data_as(native.u64p), cos.ctypes.data_as(native.f32p),
            n.ctypes.data_as(native.u32p))
    assert L.rlr_search_topk_scoped(None, None, *tail) == native.RLR_E_INVALID
    one = (C.c_void_p * 1)(None)
    assert L.rlr_search_topk_scoped(None, one, *tail) == native.RLR_E_INVALID
    fake_index = C.c_void_p(0x1000)                                # never dereferenced: the array is looked at first
    assert L.rlr_search_topk_scoped(fake_index, None, *tail) == native.RLR_E_INVALID
    assert "filter array" in L.rlr_last_error().decode()
    hits = (native.SearchHitC * 16)()
    etail = (q.ctypes.data_as(native.f32p), 8, 1, 5, 0.3, None, hits, 16, n.ctypes.data_as(native.u32p))
    assert L.rlr_engine_search_with_diversity_batch_scoped(None, one, *etail) == native.RLR_E_INVALID
    assert L.rlr_engine_search_with_diversity_batch_scoped(fake_index, None, *etail) == native.RLR_E_INVALID
    assert n[0] == 77                                              # nothing was written


class FakeEngine(eng_mod.RagEngine):
    """RagEngine.search_documents_batch over recorded stand-ins for the routes it may take"""

    def __init__(self):                                            # (no GPU index, no lexical index)
        self.calls = []

    def search_text_batch(self, emb, texts, top_k, div, weights=None, stage=0, return_info=False, documents=None):
        self.calls.append(("text_batch", [float(e[0]) for e in emb], list(texts), top_k, div, weights,
                           None if documents is None else tuple(documents)))
        return [[("text_batch", float(e[0]), None if documents is None else tuple(documents))] for e in emb]

    def search_with_diversity_batch(self, emb, top_k, div, weights=None, documents=None, scopes=None):
        assert documents is None or scopes is None
        if scopes is not None:
            assert len(scopes) == len(emb)
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
        R(query_embedding=[2.0, 1.0], query="beta", documents=["a.pdf"]),               # 2 scoped, text, alone in its scope
        R(query_embedding=[3.0, 1.0], documents=["b.pdf", "a.pdf"]),                     # 3 another scope
        R(query_embedding=[4.0, 1.0], query="", documents=["c.pdf"]),                   # 4 a third scope; empty text = none
        R(query_embedding=[5.0, 1.0], documents=[]),                                     # 5 [] is a scope, not None
        R(query_embedding=[6.0, 1.0]),                                                   # 6 unscoped, no text
        R(query_embedding=[7.0, 1.0], documents=["a.pdf", "b.pdf"]),                     # 7 the scope of 3, other order
        R(query_embedding=[8.0, 1.0], documents=["d.pdf"], top_k=3),                     # 8 other top_k
        R(query_embedding=[9.0, 1.0], documents=["a.pdf"], weights=w),                   # 9 other weights
        R(query_embedding=[10.0, 1.0], query="gamma", documents=["e.pdf"]),             # 10, 11 scoped, text, same scope
        R(query_embedding=[11.0, 1.0], query="delta", documents=["e.pdf"]),
        R(query_embedding=[12.0, 1.0], documents=["f.pdf"], weights=w),                  # 12 the weights of 9, other scope
    ]


def test_the_default_routing_is_todays():
    """without share_scopes (and with share_scopes=False) every scope is a group of its own: no scopes= call is issued"""
    for kwargs in ({}, {"share_scopes": False}):
        e = FakeEngine()
        out = e.search_documents_batch(requests(), **kwargs)
        assert [o[0][1] for o in out] == [float(i) for i in range(13)]
        assert not [c for c in e.calls if c[0] == "scopes"]
        div = sorted((c[5], c[2], c[4] is not None, tuple(c[1])) for c in e.calls if c[0] == "diversity_batch")
        assert div == sorted([(("a.pdf",), 5, False, (1.0,)), (("a.pdf", "b.pdf"), 5, False, (3.0, 7.0)), (("c.pdf",), 5, False, (4.0,)),
                              ((), 5, False, (5.0,)), (("d.pdf",), 3, False, (8.0,)), (("a.pdf",), 5, True, (9.0,)),
                              (("f.pdf",), 5, True, (12.0,))])
        text = sorted(((c[6], tuple(c[1]), tuple(c[2])) for c in e.calls if c[0] == "text_batch"), key=repr)
        assert text == sorted([(None, (0.0, 6.0), ("alpha", "")), (("e.pdf",), (10.0, 11.0), ("gamma", "delta"))], key=repr)
        assert [c for c in e.calls if c[0] == "single"] == [("single", "beta", ("a.pdf",))]
        assert len(e.calls) == 7 + 2 + 1


def test_share_scopes_is_one_call_per_key_for_the_textless_scoped_requests():
    e = FakeEngine()
    out = e.search_documents_batch(requests(), share_scopes=True)
    assert [o[0][1] for o in out] == [float(i) for i in range(13)]                       # every request got ITS result
    shared = sorted(((c[2], c[4] is not None, tuple(c[1]), tuple(c[5])) for c in e.calls if c[0] == "scopes"), key=repr)
    assert shared == sorted([
        (5, False, (1.0, 3.0, 4.0, 5.0, 7.0), (("a.pdf",), ("a.pdf", "b.pdf"), ("c.pdf",), (), ("a.pdf", "b.pdf"))),
        (3, False, (8.0,), (("d.pdf",),)),
        (5, True, (9.0, 12.0), (("a.pdf",), ("f.pdf",))),
    ], key=repr)
    # each result was searched inside ITS OWN scope
    for i, scope in ((1, ("a.pdf",)), (3, ("a.pdf", "b.pdf")), (4, ("c.pdf",)), (5, ()), (7, ("a.pdf", "b.pdf")), (8, ("d.pdf",)),
                     (9, ("a.pdf",)), (12, ("f.pdf",))):
        assert out[i][0][0] == "scopes" and out[i][0][2] == scope, i
    # the rest is today's: no one-scope diversity batch is left, the text requests go where they went
    assert not [c for c in e.calls if c[0] == "diversity_batch"]
    text = sorted(((c[6], tuple(c[1]), tuple(c[2])) for c in e.calls if c[0] == "text_batch"), key=repr)
    assert text == sorted([(None, (0.0, 6.0), ("alpha", "")), (("e.pdf",), (10.0, 11.0), ("gamma", "delta"))], key=repr)
    assert [c for c in e.calls if c[0] == "single"] == [("single", "beta", ("a.pdf",))]
    assert len(e.calls) == 3 + 2 + 1


def test_scopes_and_documents_exclude_each_other():
    class Bare(eng_mod.RagEngine):
        def __init__(self):
            self.dim = 2
    with pytest.raises(ValueError):
        Bare().search_with_diversity_batch(np.zeros((2, 2), np.float32), 5, 0.3, documents=["a.pdf"], scopes=[["a.pdf"], []])
    with pytest.raises(ValueError):
        Bare().search_with_diversity_batch(np.zeros((2, 2), np.float32), 5, 0.3, scopes=[["a.pdf"]])
