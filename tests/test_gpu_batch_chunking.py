"""How the batched entry points cut a call into shared chunks, read off the profile counters: the forms counters count
queries and cannot tell 9 queries as 5 + 4 from 8 + 1; n_batches / n_batch_queries / n_batch_fallbacks can.

One index for every case, the smallest shape the shared scans serve with room for eight queries a chunk: 300 rows of 768
f32 elements (grouped_batch_vectors.chunk_width says 8 for it), a document every four rows.  Sharing is forced (mode 2)
or off (mode 1); the gate of mode 0 is a cost model and is not held here.  What must come out:
  grouped / capped batch   2 -> one chunk, 8 -> one chunk, 9 -> 5 + 4, 17 -> 6 + 6 + 5; no query handed back
  range batch              8 -> one chunk behind the shared scan; 9 -> no shared pass at all (the scan takes 8 queries
                           at most, the GEMM wants 4096 rows): every query by rule"""
import numpy as np
import pytest

import grouped_batch_vectors as W

pytestmark = pytest.mark.gpu

DIM, N = 768, 300
PER_DOC = 2
CHUNKS = {2: 1, 8: 1, 9: 2, 17: 3}                           # queries of a call -> shared chunks


@pytest.fixture(scope="module")
def corpus(rlr, oracle):
    rows = oracle.synth_rows(N, DIM, seed=0x7A11)
    qs = np.stack([oracle.normalize(oracle.synth_query(DIM, seed=0x7A12 + i)) for i in range(17)])
    ix = rlr.GpuIndex(DIM, "f32")
    ix.upload(rows)
    ix.set_documents((np.arange(N) // 4).astype(np.uint32))
    assert W.chunk_width(N, DIM * 4, N, PER_DOC) == 8
    assert [len(W.split(nq, 8)) for nq in CHUNKS] == list(CHUNKS.values())
    yield ix, qs
    ix.close()


def counters(ix):
    p = ix.profile_read()
    return p.n_batches, p.n_batch_queries, p.n_batch_fallbacks


def grouped(ix, qs):
    ix.grouped_batch_forms(reset=True)
    got = ix.search_topk_grouped_batch(qs, 5, PER_DOC)
    assert all(g[0].size == 5 for g in got)
    return ix.grouped_batch_forms()


def capped(ix, qs):
    ix.capped_batch_forms(reset=True)
    got = ix.search_capped_batch(qs, 5, PER_DOC)
    assert all(g[0].size == 5 for g in got)
    return ix.capped_batch_forms()


@pytest.mark.parametrize("nq", sorted(CHUNKS))
@pytest.mark.parametrize("search,share", [(grouped, "set_grouped_sharing"), (capped, "set_capped_sharing")])
def test_grouped_and_capped_calls_are_cut_evenly(corpus, search, share, nq):
    ix, qs = corpus
    try:
        getattr(ix, share)(2)
        ix.profile_read(reset=True)
        forms = search(ix, qs[:nq])
        got = counters(ix)
        print(search.__name__, nq, "forced:", forms, got)
        assert forms == [nq, 0, 0, 0]
        assert got == (CHUNKS[nq], nq, 0)
        getattr(ix, share)(1)
        ix.profile_read(reset=True)
        forms = search(ix, qs[:nq])
        got = counters(ix)
        print(search.__name__, nq, "never:", forms, got)
        assert forms == [0, 0, 0, nq]
        assert got[0] == 0
    finally:
        getattr(ix, share)(0)


def test_range_calls_share_a_scan_up_to_eight_queries(corpus):
    ix, qs = corpus
    ix.set_range_sharing(2)
    try:
        for nq, forms, batches, batch_queries in ((8, [8, 0, 0, 0], 1, 8), (9, [0, 0, 0, 9], 0, 0)):
            ix.profile_read(reset=True)
            ix.range_batch_forms(reset=True)
            got = ix.search_range_batch(qs[:nq], 0.05, 16)
            counted, prof = ix.range_batch_forms(), counters(ix)
            print("range", nq, counted, prof)
            assert len(got) == nq
            assert counted == forms
            assert prof[:2] == (batches, batch_queries)
    finally:
        ix.set_range_sharing(0)
