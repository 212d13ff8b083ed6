"""The document-column vectors (tests/document_vectors.py) against an independent restatement -- a Python loop over
rows --, four planted defects that the checks must catch, and the new C ABI without a device: declared, exported, in the
ctypes table, and refusing to work with no GPU (the library has no CPU path)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import document_vectors as V
from conftest import ROOT

NEW_SYMBOLS = ["rlr_index_set_documents", "rlr_index_tag_rows", "rlr_index_get_documents", "rlr_filter_create_documents",
               "rlr_filter_read", "rlr_index_delete_documents"]


# ---- the restatement ---------------------------------------------------------------------------------------------
def loop_expect(ids, docs):
    """mask words, ascending list and surviving column, one row at a time"""
    want = {int(d) for d in docs if int(d) != V.DOC_NONE}
    n = len(ids)
    words = [0] * ((n + 63) // 64)
    rows, after = [], []
    for r in range(n):
        if int(ids[r]) != V.DOC_NONE and int(ids[r]) in want:
            words[r >> 6] |= 1 << (r & 63)
            rows.append(r)
        else:
            after.append(int(ids[r]))
    return words, rows, after


def check(ids, docs, e):
    """every property the device results are held to, stated without the generator's own arithmetic"""
    n = len(ids)
    mask, rows = e["mask"], e["rows"]
    assert mask.dtype == np.uint64 and mask.size == (n + 63) // 64
    assert rows.dtype == np.uint32
    assert sum(bin(int(w)).count("1") for w in mask) == rows.size, "popcount of the mask != length of the list"
    if n % 64:
        assert int(mask[-1]) >> (n % 64) == 0, "tail bits of the last word are not zero"
    assert np.all(np.diff(rows.astype(np.int64)) > 0), "the list is not strictly ascending"
    assert all((int(mask[int(r) >> 6]) >> (int(r) & 63)) & 1 for r in rows[:: max(1, rows.size // 997)])
    assert np.array_equal(e["column_after"], np.delete(np.asarray(ids, np.uint32), rows.astype(np.int64)))


@pytest.mark.parametrize("n", V.SMALL_ROW_COUNTS)
def test_patterns_match_the_loop_restatement(n):
    pats = V.id_patterns(n)
    assert len(pats) >= 20 or n < 64
    for name, ids, docs in pats:
        e = V.expect(ids, docs)
        words, rows, after = loop_expect(ids, docs)
        assert [int(w) for w in e["mask"]] == words, (n, name)
        assert e["rows"].tolist() == rows, (n, name)
        assert e["column_after"].tolist() == after, (n, name)
        check(ids, docs, e)


@pytest.mark.parametrize("n", V.LARGE_ROW_COUNTS)
def test_large_patterns_hold_the_properties(n):
    for name, ids, docs in V.id_patterns(n):
        if name.startswith(("run_", "single_row_")) and not name.endswith(("_at_64", f"_{n - 1}")):
            continue   # (the word-edge cases of the first rows are covered at the small sizes)
        check(ids, docs, V.expect(ids, docs))


def test_alternating_words_and_row_counts():
    pats = dict((nm, (ids, docs)) for nm, ids, docs in V.id_patterns(129))
    assert [hex(int(w)) for w in V.expect(*pats["alternating_even"])["mask"]] == ["0x5555555555555555"] * 2 + ["0x1"]
    assert [hex(int(w)) for w in V.expect(*pats["alternating_odd"])["mask"]] == ["0xaaaaaaaaaaaaaaaa"] * 2 + ["0x0"]
    # the row counts follow the constants the kernel file states (docs.hip:15-18)
    src = open(os.path.join(ROOT, "rust-local-rag_amd", "csrc", "docs.hip")).read().split("\n")
    assert "kDocsRowsPerGroup = 4096" in src[15] and "kDocsSumsPerGroup = 1024" in src[16], src[15:18]
    hdr = open(os.path.join(ROOT, "rust-local-rag_amd", "csrc", "kernels.h")).read()
    assert f"kDocsRowsPerGroup = {V.ROWS_PER_GROUP};" in hdr and f"kDocsSumsPerGroup = {V.SUMS_PER_GROUP};" in hdr
    assert f"kDocsLdsMax = {V.LDS_SET_MAX};" in hdr
    G, S = V.ROWS_PER_GROUP, V.SUMS_PER_GROUP
    for edge in (G, G * S):
        assert {edge - 1, edge, edge + 1} <= set(V.ROW_COUNTS)
    assert max(V.ROW_COUNTS) >= (1 << 20) + 65 and {1, 63, 64, 65, 127, 128, 129} <= set(V.ROW_COUNTS)


def test_query_sets_cover_both_membership_paths():
    ids = V.random_1000(5000)
    sizes = {}
    for name, docs in V.query_sets():
        sizes[name] = np.unique(docs).size
        e = V.expect(ids, docs)
        words, rows, after = loop_expect(ids, docs)
        assert [int(w) for w in e["mask"]] == words and e["rows"].tolist() == rows and e["column_after"].tolist() == after, name
    assert sizes["one"] == 1 and sizes["two_unsorted"] == 2 and sizes["five_thousand"] == 5000
    assert sizes["lds_max"] == V.LDS_SET_MAX and sizes["lds_max_plus_1"] == V.LDS_SET_MAX + 1
    assert sizes["repeats_past_the_switch"] > V.LDS_SET_MAX
    q = dict(V.query_sets())
    assert q["repeats"].size > np.unique(q["repeats"]).size and np.any(np.diff(q["lds_max"].astype(np.int64)) < 0)
    assert V.expect(ids, q["tags_nothing"])["rows"].size == 0
    assert V.expect(ids, q["all_real_documents"])["rows"].size == ids.size


@pytest.mark.parametrize("n", [1, 64, 65, 300, 4097])
def test_delete_patterns_match_the_loop_restatement(n):
    for name, ids, docs in V.delete_patterns(n):
        e = V.expect(ids, docs)
        _, rows, after = loop_expect(ids, docs)
        assert e["rows"].tolist() == rows and e["column_after"].tolist() == after, (n, name)
        check(ids, docs, e)
    sizes = {name: V.expect(ids, docs)["rows"].size for name, ids, docs in V.delete_patterns(n)}
    assert sizes["everything"] == n and sizes["nothing"] == 0 and sizes["every_other_row"] == (n + 1) // 2


# ---- planted defects: each one must make some check fail ------------------------------------------------------------
def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_planted_defects_are_caught():
    n = 2 * V.ROWS_PER_GROUP + 37
    ids = V.random_1000(n)
    docs = [V.BASE + V.STEP * d for d in range(0, 1000, 2)]
    good = V.expect(ids, docs)
    check(ids, docs, good)
    words, rows, _ = loop_expect(ids, docs)

    # 1. off by one at a word edge: row 64's membership lands on row 63
    ids1 = np.full(200, 3, np.uint32); ids1[64] = 4
    bad = V.expect(np.roll(ids1, -1), [4])
    assert [int(w) for w in bad["mask"]] != loop_expect(ids1, [4])[0]
    assert bad["rows"].tolist() != loop_expect(ids1, [4])[1]

    # 2. a non-zero tail bit in the last word
    bad = dict(good, mask=good["mask"].copy())
    bad["mask"][-1] |= np.uint64(1) << np.uint64(n % 64)
    assert _fails(lambda: check(ids, docs, bad))

    # 3. a list that is not ascending across a workgroup seam: the first row of workgroup 1 before the last of workgroup 0
    seam = int(np.searchsorted(good["rows"], V.ROWS_PER_GROUP))
    assert 0 < seam < good["rows"].size
    bad = dict(good, rows=good["rows"].copy())
    bad["rows"][[seam - 1, seam]] = bad["rows"][[seam, seam - 1]]
    assert _fails(lambda: check(ids, docs, bad)) and bad["rows"].tolist() != rows

    # 4. RLR_DOC_NONE treated as a member
    ids4 = dict((nm, i) for nm, i, _ in V.id_patterns(300))["none_interleaved"]
    naive = np.isin(ids4, np.array([1, V.DOC_NONE], np.uint32))          # (what a membership test without the rule gives)
    assert V.mask_words(naive).tolist() != V.expect(ids4, [1, V.DOC_NONE])["mask"].tolist()
    assert [int(w) for w in V.expect(ids4, [1, V.DOC_NONE])["mask"]] == loop_expect(ids4, [1, V.DOC_NONE])[0]


def test_engine_cuts_its_tables_by_the_returned_rows(rlr):
    """RagEngine._cut_rows (what remove_document does with the rows delete_documents returns) against the plain
    statement: drop the dead rows, number the rest from 0"""
    from types import SimpleNamespace

    for n in (1, 5, 300):
        for name, ids, docs in V.delete_patterns(n):
            dead = V.expect(ids, docs)["rows"].astype(np.int64)
            if dead.size == 0:
                continue
            for planted in (False, True):
                chunks = [rlr.DocumentChunk(f"id{r}", f"d{ids[r]}", "", r) for r in range(n)]
                e = SimpleNamespace(_chunks=list(chunks), _row_of={} if planted else {ch.id: r for r, ch in enumerate(chunks)})
                rlr.RagEngine._cut_rows(e, dead)
                want = [ch for r, ch in enumerate(chunks) if r not in set(dead.tolist())]
                assert e._chunks == want and all(a is b for a, b in zip(e._chunks, want)), (n, name, planted)
                assert e._row_of == {ch.id: r for r, ch in enumerate(want)}, (n, name, planted)


# ---- the C ABI without a device -------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(rlr):
    hdr = open(os.path.join(ROOT, "include", "rlr_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from importlib import import_module
    native = import_module("rust-local-rag_amd._native")
    bound = {n for n, _, _ in native.PROTOTYPES}
    L = C.CDLL(rlr.SO_PATH)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", code), f"{name} is not declared in rlr_gpu.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in bound, f"{name} is missing from the ctypes table"
        assert name in doc, f"INTEGRATION.md shows no binding for {name}"
    assert re.search(r"#define\s+RLR_DOC_NONE\s+0xFFFFFFFFu", hdr)
    assert rlr.DOC_NONE == V.DOC_NONE
    assert "do NOT make filters" in hdr          # the header says that tagging leaves filters valid


def test_document_calls_need_a_device(rlr, gpu_available):
    L = rlr.lib()
    u32 = np.arange(3, dtype=np.uint32)
    u32p = u32.ctypes.data_as(C.POINTER(C.c_uint32))
    rows = np.zeros(4, np.uint64)
    n = C.c_uint64(99)
    h = C.c_void_p()
    want = -1 if gpu_available else -2           # a null index is a bad argument on a real device; no device comes first
    assert L.rlr_index_set_documents(None, u32p, 3) == want
    assert L.rlr_index_tag_rows(None, 0, 1, 5) == want
    assert L.rlr_index_get_documents(None, 0, 3, u32p) == want
    assert L.rlr_index_delete_documents(None, u32p, 3, rows.ctypes.data_as(C.POINTER(C.c_uint64)), 4, C.byref(n)) == want
    assert n.value == 0
    assert L.rlr_filter_read(None, None, None) == want
    assert L.rlr_filter_create_documents(None, u32p, 3, None) == -1          # a creator's null out
    assert L.rlr_filter_create_documents(None, u32p, 3, C.byref(h)) == want and not h.value
    if not gpu_available:
        assert b"no CPU path" in L.rlr_last_error()
