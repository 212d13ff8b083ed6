"""The batched BM25 chain with a row mask PER QUERY (rlr_lexical_score_batch_scoped): every query of a batch is held to the
oracle's unfiltered, untruncated list reduced to ITS allowed rows and then cut to the limit -- rows and score bits -- and,
bit for bit, to LexicalIndex.score(filter=filters[q]) for the same text.  Every scoped batch is followed by an unfiltered
batch and by a one-filter batch against the oracle: the scoped chain must leave nothing behind.  The cases are the
smallest at which a grid row can take the wrong mask, the wrong index size or the wrong exit."""
import contextlib
import ctypes as C
import importlib

import numpy as np
import pytest

import scoped_text_vectors as SV
import text_batch_filtered_vectors as V
from oracle import lexical as OL
from test_gpu_filter_lexical import build, make_texts

pytestmark = pytest.mark.gpu
EPS = np.float32(1.1920929e-07)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def reduced(full, t, inside, limit):
    return [(c, s) for c, s in full[t] if c in inside][:limit]


def same_pairs(rows, sc, want, ctx):
    assert [int(r) for r in rows] == [c for c, _ in want], ctx
    assert np.array_equal(bits(sc), bits([s for _, s in want])), ctx


def check_scoped(g, o, full, texts, limit, filters, alloweds, n_single=0, singles=True, done=None):
    """scoped batch against the reduced oracle lists and the single filtered calls, then an unfiltered batch and a
    one-filter batch (the filter of slot 0) against the oracle; returns the per-query numbers of pairs"""
    for t in set(texts):
        if t not in full:                                                   # one oracle pass per text, shared
            full[t] = o.score(t, 0, keep_zero=False)
    insides = {id(a): set(int(r) for r in a) for a in alloweds}
    got, info = g.score_batch(texts, limit, return_info=True, filters=filters)
    assert info["n_single"] == n_single and len(got) == len(texts)
    done = {} if done is None else done
    counts = []
    for i, (t, (rows, sc)) in enumerate(zip(texts, got)):
        ctx = (i, t[:40], limit, len(alloweds[i]))
        want = reduced(full, t, insides[id(alloweds[i])], limit)
        same_pairs(rows, sc, want, ctx)
        mx = max([np.float32(s) for _, s in want], default=np.float32(0.0))
        assert info["max_lexical"][i] == (mx if mx >= EPS else EPS), ctx
        if singles:
            key = (t, limit, id(filters[i]))
            if key not in done:                                             # the single call, once per (text, filter)
                done[key] = g.score(t, limit, filter=filters[i])
            assert np.array_equal(rows, done[key][0]) and np.array_equal(bits(sc), bits(done[key][1])), ctx
        counts.append(len(want))
    for t, (rows, sc) in zip(texts, g.score_batch(texts, limit)):            # nothing of any mask is left behind
        same_pairs(rows, sc, full[t][:limit], (t[:40], limit, "unfiltered after"))
    for t, (rows, sc) in zip(texts, g.score_batch(texts, limit, filter=filters[0])):
        same_pairs(rows, sc, reduced(full, t, insides[id(alloweds[0])], limit), (t[:40], limit, "one filter after"))
    return counts


@pytest.fixture(scope="module")
def small(rlr):
    texts = make_texts(V.LEX_ROWS, seed=7)
    g, o, ix = build(rlr, texts)
    masks = V.lex_masks(V.LEX_ROWS, texts)
    with contextlib.ExitStack() as st:
        filters = {name: st.enter_context(ix.filter_rows(rows)) for name, rows in masks.items()}
        yield g, o, ix, {}, masks, filters
    g.close()
    ix.close()


@pytest.mark.parametrize("rot", [0, 1])
def test_every_mask_in_one_batch(small, rot):
    """the slots of ONE batch cycle through all seven masks: the workgroups of one slice leave by different exits; the same
    texts with the scopes rotated by one slot catch a mask applied to the wrong grid row"""
    g, o, ix, full, masks, filters = small
    names = sorted(masks)
    assert len(names) == 7
    texts = V.lex_batch(9)
    slot = [names[(i + rot) % 7] for i in range(9)]
    done, per_mask = {}, {n: 0 for n in names}
    for limit in V.LIMITS:
        counts = check_scoped(g, o, full, texts, limit, [filters[n] for n in slot], [masks[n] for n in slot], done=done)
        for n, c in zip(slot, counts):
            per_mask[n] += c
    assert per_mask["none"] == 0 and per_mask["every_row"] > 0 and sum(per_mask.values()) > per_mask["every_row"], per_mask


def test_the_same_filter_in_every_slot(small):
    g, o, ix, full, masks, filters = small
    texts = V.lex_batch(9)
    for name in ("every_other", "slice_edge"):
        for limit in (5, 8192):
            assert sum(check_scoped(g, o, full, texts, limit, [filters[name]] * 9, [masks[name]] * 9)) > 0
            a = g.score_batch(texts, limit, filters=[filters[name]] * 9)
            b = g.score_batch(texts, limit, filter=filters[name])
            for (ra, sa), (rb, sb) in zip(a, b):
                assert np.array_equal(ra, rb) and np.array_equal(bits(sa), bits(sb)), (name, limit)


def test_scopes_confined_to_one_slice_each(small):
    """query q's scope lies inside slice q % 3: every other slice of its grid row leaves by the mask exit; the first allowed
    row is the first row of a slice, or its last"""
    g, o, ix, full, masks, _ = small
    scopes = SV.slice_scopes(V.LEX_ROWS)
    for j, rows in enumerate(scopes):
        assert rows.min() // 2048 == rows.max() // 2048 == SV.SLICE_OF[j] == j % 3
    assert {int(r.min()) % 2048 for r in scopes} >= {0, 2047}
    texts = [V.BROAD, "w005x w006x", "w007x w008x w009x", V.BROAD, V.BROAD, "w010x w011x w012x"] * 2
    with contextlib.ExitStack() as st:
        fs = [st.enter_context(ix.filter_rows(r)) for r in scopes]
        for limit in V.LIMITS:
            counts = check_scoped(g, o, full, texts, limit, [fs[i % 6] for i in range(12)], [scopes[i % 6] for i in range(12)])
            assert sum(counts) > 0 and counts[0] > 0 and counts[5] > 0


def test_a_batch_beyond_one_sub_batch_and_a_query_of_129_terms(small):
    """257 queries: query 256 runs in the second sub-batch, where the filter array must be offset with the queries (its scope
    differs from query 0's); the 129-term query of slot 200 is re-run alone under ITS filter, not slot 0's"""
    g, o, ix, full, masks, filters = small
    names = sorted(masks)
    texts = V.lex_batch(257)
    texts[200] = V.MANY_TERMS
    texts[256] = V.BROAD
    slot = [names[i % 7] for i in range(257)]
    slot[0], slot[256], slot[200] = "word_edge", "every_other", "slice_masked"
    counts = check_scoped(g, o, full, texts, 5, [filters[n] for n in slot], [masks[n] for n in slot], n_single=1, singles=False)
    assert sum(counts) > 300 and counts[200] == 5 and counts[256] == 5
    got = g.score_batch(texts, 5, filters=[filters[n] for n in slot])
    for i in (0, 200, 256):
        rows, sc = g.score(texts[i], 5, filter=filters[slot[i]])
        assert np.array_equal(got[i][0], rows) and np.array_equal(bits(got[i][1]), bits(sc)), i


def test_filters_of_two_index_sizes_in_one_call(rlr, small):
    """filters of a 4100-row index and of the 4200-row index in ONE call: mask_rows is per query -- rows 4100 .. 4199 (inside
    the third slice, behind a mask word that ends at 4100 = 64 * 64 + 4) hold postings and are masked for some queries only"""
    g, o, ix, full, masks, filters = small
    short = rlr.GpuIndex(8)
    try:
        short.upload(np.ones((V.SMALL_INDEX, 8), np.float32))
        tail_rows = np.arange(4090, V.LEX_ROWS)
        with short.filter_rows(np.arange(V.SMALL_INDEX)) as f_all, short.filter_rows(np.arange(4090, V.SMALL_INDEX)) as f_tail, \
                ix.filter_rows(tail_rows) as f_long:
            fs = [f_all, f_long, f_tail, filters["every_row"], f_long, f_all, f_tail, f_long]
            al = [np.arange(V.SMALL_INDEX), tail_rows, np.arange(4090, V.SMALL_INDEX), masks["every_row"], tail_rows,
                  np.arange(V.SMALL_INDEX), np.arange(4090, V.SMALL_INDEX), tail_rows]
            texts = [V.BROAD] * 4 + ["w005x w006x", "w007x", V.BROAD, "w008x w009x w010x"]
            for order in (range(8), range(7, -1, -1)):                      # the widest filter first, and last
                order = list(order)
                for limit in (8192, 5):
                    counts = check_scoped(g, o, full, [texts[i] for i in order], limit, [fs[i] for i in order],
                                          [al[i] for i in order])
                    by = dict(zip(order, counts))
                    if limit == 8192:                                       # the rows behind 4100 show for the long filter only
                        assert by[1] > by[2] > 0 and by[3] > by[0] > 0, by
    finally:
        short.close()


def test_select_regimes_in_one_batch(rlr):
    """the 40 000-row recipe of test_select_regimes_and_exact_ties: one query's scope leaves more than 8192 keyed rows (the
    radix passes), its neighbours' a handful and about 6700 (the LDS sort) -- in ONE batch"""
    texts = make_texts(40000, seed=2, lo=2, hi=6, common_every=3)
    texts += ["ubiquitous rare"] * 50 + ["rare"] * 3
    n = len(texts)
    g, o, ix = build(rlr, texts)
    try:
        full = {}
        masks = {"most": np.delete(np.arange(n), np.arange(0, n, 7)), "every_other": np.arange(n)[::2], "few": np.arange(n)[::611]}
        batch = ["ubiquitous", "ubiquitous", "ubiquitous rare w000x", "ubiquitous", "rare", "w000x w001x common"]
        slot = ["few", "most", "every_other", "every_other", "most", "few"]
        with contextlib.ExitStack() as st:
            fs = {k: st.enter_context(ix.filter_rows(v)) for k, v in masks.items()}
            for limit in V.LIMITS:
                counts = check_scoped(g, o, full, batch, limit, [fs[s] for s in slot], [masks[s] for s in slot])
                assert counts[1] == limit and counts[0] == min(limit, counts[0]) > 0
            assert sum(1 for c, _ in full["ubiquitous"] if c % 7) > 8192
            assert sum(1 for c, _ in full["ubiquitous"] if c % 611 == 0) < 64
    finally:
        g.close()
        ix.close()


def test_appended_and_compacted_postings(rlr):
    """the segment recipes of test_gpu_lexical_batch: an appended segment beside the main one, then a removal from both
    (device compaction).  One scope lies inside the appended rows, one outside, one across; filters made after each step"""
    lex = importlib.import_module("rust-local-rag_amd.lexical")
    g = lex.LexicalIndex(0)
    cur = make_texts(5000, seed=21, lo=10, hi=30)
    for r, t in enumerate(cur):
        g.add_chunk(r, t)
    g.score("w000x", 5)                                                      # the main segment is built
    extra = make_texts(300, seed=22, lo=5, hi=30) + ["brandnewterm w005x", "brandnewterm brandnewterm w006x"]
    for t in extra:
        g.add_chunk(len(cur), t)
        cur.append(t)
    texts = [V.BROAD, "brandnewterm w005x", "w017x w101x", V.BROAD, "brandnewterm", "w006x w007x"]
    try:
        for phase in ("appended", "compacted"):
            if phase == "compacted":
                dead = set(range(100, 2300, 3)) | set(range(5010, 5290, 4))
                g.remove_rows(sorted(dead))
                cur = [t for r, t in enumerate(cur) if r not in dead]
            n, n_main = len(cur), len(cur) - (302 if phase == "appended" else 302 - 70)
            o = OL.LexicalIndex()
            for r, t in enumerate(cur):
                o.add_chunk(r, t, rank=r)
            ix = rlr.GpuIndex(8)
            try:
                ix.upload(np.ones((n, 8), np.float32))
                scopes = [np.arange(n_main, n), np.arange(0, n_main)[::3], np.arange(n_main - 50, n_main + 50)]
                with contextlib.ExitStack() as st:
                    fs = [st.enter_context(ix.filter_rows(r)) for r in scopes]
                    for limit in (5, 8192):
                        counts = check_scoped(g, o, {}, texts, limit, [fs[i % 3] for i in range(6)], [scopes[i % 3] for i in range(6)])
                        assert counts[0] > 0 and counts[1] > 0 and counts[4] == 0, (phase, counts)   # brandnewterm: appended rows only
                seg = g.segments()
                assert seg["appended_postings"] > 0, (phase, seg)
            finally:
                ix.close()
    finally:
        g.close()


def test_refusals_and_empty_batches(rlr, small):
    g, o, _, full, masks, filters = small
    N = importlib.import_module("rust-local-rag_amd._native")
    ix = rlr.GpuIndex(8)
    other = None
    try:
        ix.upload(np.ones((V.LEX_ROWS, 8), np.float32))
        with ix.filter_rows([3, 4, 2050]) as f, ix.filter_rows([]) as empty:
            got, info = g.score_batch(V.lex_batch(3), 5, return_info=True, filters=[empty, empty, empty])    # an all-empty batch
            assert [len(r) for r, _ in got] == [0, 0, 0] and info["n_single"] == 0
            assert all(m == EPS for m in info["max_lexical"])
            got, info = g.score_batch([V.MANY_TERMS, V.BROAD], 5, return_info=True, filters=[empty, f])
            assert len(got[0][0]) == 0 and info["n_single"] == 0                # (an empty scope has no terms to count)
            check_scoped(g, o, full, V.lex_batch(2), 5, [f, filters["every_other"]], [np.array([3, 4, 2050]), masks["every_other"]])
            # a null entry: RLR_E_INVALID before any GPU work
            toks = b"w005x w006x"
            off = np.array([0, 5, 11], np.uint64)
            rows, sc, n = np.zeros(10, np.uint64), np.zeros(10, np.float32), np.zeros(2, np.uint32)
            arr = (C.c_void_p * 2)(f.handle, None)
            st = N.lib().rlr_lexical_score_batch_scoped(g._h, arr, 2, toks, off.ctypes.data_as(N.u64p), 5, rows.ctypes.data_as(N.u64p),
                                                        sc.ctypes.data_as(N.f32p), n.ctypes.data_as(N.u32p), None, None)
            assert st == -1
            ix.append(np.ones((1, 8), np.float32))                              # a stale entry behind a current one
            with pytest.raises(rlr.RlrError) as ei:
                g.score_batch(V.lex_batch(2), 5, filters=[filters["every_other"], f])
            assert ei.value.status == -1 and "stale" in str(ei.value)
        if rlr.device_count() > 1:                                              # an entry that lives on another device
            other = rlr.GpuIndex(8, device=1)
            other.upload(np.ones((V.LEX_ROWS, 8), np.float32))
            with other.filter_rows([3, 4]) as f:
                with pytest.raises(rlr.RlrError) as ei:
                    g.score_batch(V.lex_batch(2), 5, filters=[filters["every_other"], f])
                assert ei.value.status == -1 and "device" in str(ei.value)
        texts = V.lex_batch(2)                                                   # the index is as usable as before
        for t in texts:
            full.setdefault(t, o.score(t, 0, keep_zero=False))
        for t, (r, s) in zip(texts, g.score_batch(texts, 5)):
            same_pairs(r, s, full[t][:5], t)
    finally:
        ix.close()
        if other is not None:
            other.close()
