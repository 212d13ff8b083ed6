"""Range, grouped and capped search across the index's state machine, on the device: one index per configuration walks
the whole plan of mutation_vectors.py, tags its document column as state_vectors.py says (the appended tail by tag_rows
or the whole column by set_documents, in turn; the whole column after every upload), and after EVERY step
  - get_documents() equals the column model straight after the mutation (an append's tail DOC_NONE, an upload's column
    gone, a delete's compacted) and the mirror after the tagging;
  - search_range / search_range_batch / count_range / count_range_batch, search_topk_grouped / _batch or search_capped /
    _batch return the definition's rows, score bits, documents and n_total for the step's probes one at a time, in
    groups of up to 8 and as one call;
  - the form counters say which path answered: a single entry decides on the device (range: form 1 where n_total
    exceeds cap), a batched entry reports exactly what state_vectors.range_batch_forms / chunk_forms restate from the
    dispatch with sharing forced (mode 2) -- no probe is handed back on a capacity or as undecidable;
  - the profile counters say which copy was read: a range GEMM streams the image where one is on (batch_gemm_bytes),
    and a single range query with more hits than cap -- every self-probe asks its own rank-25 score at cap 10 -- takes
    its rows from the top-k path over the 8-bit copy or the image (scan_bytes): a stale copy entry costs that probe a
    row (test_state_vectors_cpu.py proves it for every fault of mutation_vectors.FAULTS).
The dispatch, as the library has it at 256 columns: 2..8 range queries over f32 rows share a scan at ANY row count, 9 or
more (and 2..8 over binary16 rows) share the GEMM from 4096 rows on and go one by one below; grouped and capped batches
over f32 rows share a scan in chunks of up to 8 at any row count, over binary16 rows they go one by one.  So the emptied
index answers nothing, without an error, and the index cut down to 300 rows answers its GEMM-sized calls by the single
path and its small ones behind the shared scan.

Then row filters across the plan (a filter made before an append or delete is refused by all six entries, a fresh one
over every third row plus the probe rows gives the definition inside it on both of its paths) and the three sharing
modes on three steps.  GPU time per item (MI355X): DESIGN.md, "Searches across mutations"."""
import numpy as np
import pytest

import mutation_vectors as M
import state_vectors as S
from conftest import bits
from test_gpu_mutations import Walker

pytestmark = pytest.mark.gpu

CONFIGS = [("f32", "plain", "no_copy"), ("f32", "image_single_query", "on_before_upload"), ("f32", "q8", "on_before_upload"),
           ("f16", "plain", "no_copy")]
FAMILIES = ("range", "grouped", "capped")
FILTER_GROUPED = ((25, 1), (3, 3))
FILTER_CAPPED = ((3, 1, False, 3), (10, 2, True, 5))


def same_f32(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and bool(np.all(bits(got) == bits(want)))


class StateWalker(Walker):
    """test_gpu_mutations' Walker with a document column and the six entries"""

    def __init__(self, rlr, O, dtype, copies, schedule):
        super().__init__(rlr, O, dtype, copies, schedule)
        self.set_sharing(2)

    def set_sharing(self, mode):
        self.ix.set_range_sharing(mode)
        self.ix.set_grouped_sharing(mode)
        self.ix.set_capped_sharing(mode)

    def mutate(self, st):
        """the step's mutation and the walker's tagging; the column is held to the model before and after it"""
        col = S.column(st)
        self.apply(st)
        assert len(self.ix) == st.n_after, st.name
        got = self.ix.get_documents()
        assert np.array_equal(got, col.raw), (st.name, "column after the mutation", np.flatnonzero(got != col.raw)[:8])
        return col

    def tag(self, st, col):
        if col.tag == "rows":
            for first, count, doc in S.runs(col.tagged[st.n_before:]):
                self.ix.tag_rows(st.n_before + first, count, doc)
        elif col.tag == "whole":
            self.ix.set_documents(col.tagged)
        got = self.ix.get_documents()
        assert np.array_equal(got, S.doc_of(st.ids_after)), (st.name, "column after tagging", np.flatnonzero(got != col.tagged)[:8])

    # -- range -----------------------------------------------------------------------------------------------------
    def check_range(self, sp, allowed=None, filt=None, list_path=False, hold_forms=True):
        ix, st = self.ix, sp.st
        n = sp.n if allowed is None or len(allowed) else 0
        Q, taus, out = sp.range_queries, sp.taus, []
        for cap in S.RANGE_CAPS + (0,):
            want = sp.range_expect(cap, allowed)
            ctx = (self.dtype, self.copies, st.name, "range", cap, allowed is not None, list_path)

            def same(got, i, how):
                r, c, total = got
                assert total == want[i][2], (ctx, how, i, sp.cases[i], total, want[i][2])
                assert np.array_equal(r, want[i][0]), (ctx, how, i, sp.cases[i], r[:6], want[i][0][:6])
                assert same_f32(c, want[i][1]), (ctx, how, i, sp.cases[i])

            for i in range(len(taus)):
                ix.range_forms(reset=True)
                ix.profile_read(reset=True)
                if cap:
                    same(ix.search_range(Q[i], taus[i], cap, filter=filt)[0], i, "single")
                else:
                    assert ix.count_range(Q[i], taus[i], filter=filt) == [want[i][2]], (ctx, "count_range", i, sp.cases[i])
                p = ix.profile_read()
                forms = [0, 0, 0, 0]
                if n:
                    forms[3 if list_path else 1 if cap and want[i][2] > cap else 0] = 1
                assert ix.range_forms() == forms, (ctx, "single", i, sp.cases[i], ix.range_forms(), forms)
                if forms[1] and filt is None:
                    # more hits than cap: the rows come from the top-k path at k = cap, which nominates over the copy
                    # that is on (1 byte an element over the 8-bit copy, 2 over the image once it serves single queries)
                    assert p.n_scan_launches == 1 and p.scan_bytes == n * M.DIM * self.bytes_per_element(), \
                        (ctx, "hand-off", i, sp.cases[i], p, self.bytes_per_element())
            for sel in S.chunks(len(taus)) + [np.arange(len(taus))]:
                ix.range_batch_forms(reset=True)
                ix.profile_read(reset=True)
                if cap:
                    got = ix.search_range_batch(Q[sel], taus[sel], cap, filter=filt)
                    for j, i in enumerate(sel):
                        same(got[j], i, f"batch of {len(sel)}")
                    out.append(got)
                else:
                    got = ix.count_range_batch(Q[sel], taus[sel], filter=filt)
                    assert got == [want[i][2] for i in sel], (ctx, f"count_range_batch of {len(sel)}")
                    out.append(got)
                forms = ix.range_batch_forms()
                assert sum(forms) == (len(sel) if n else 0), (ctx, forms)
                if hold_forms:
                    want_forms = S.range_batch_forms(self.dtype, n, len(sel), list_path)
                    assert forms == want_forms, (ctx, f"batch of {len(sel)}", forms, want_forms)
                    # the operand the GEMM streamed: 2 bytes an element over the image (and over binary16 rows), 4 over
                    # f32 rows; nothing behind the shared scan or by rule
                    image = self.on and self.copies.startswith("image")
                    streamed = n * M.DIM * (2 if image or self.dtype == "f16" else 4) if want_forms[1] else 0
                    p = ix.profile_read()
                    assert p.batch_gemm_bytes == streamed, (ctx, f"batch of {len(sel)}", p.batch_gemm_bytes, streamed)
        return out

    # -- grouped ---------------------------------------------------------------------------------------------------
    def check_grouped(self, sp, combos=S.GROUPED, docs=None, allowed=None, filt=None, list_path=False, hold_forms=True,
                      phase="tagged"):
        ix, st = self.ix, sp.st
        n = sp.n if allowed is None or len(allowed) else 0
        n_allowed = n if allowed is None else len(allowed)
        Q, out = sp.queries, []
        for k, m in combos:
            want = sp.grouped_expect(k, m, docs=docs, allowed=allowed)
            ctx = (self.dtype, self.copies, st.name, "grouped", phase, k, m, allowed is not None, list_path)

            def same(got, i, how):
                r, c, d = got
                assert np.array_equal(r, want[i][0]), (ctx, how, i, r[:6], want[i][0][:6])
                assert same_f32(c, want[i][1]) and np.array_equal(d, want[i][2]), (ctx, how, i)

            for i in range(len(Q)):
                ix.grouped_forms(reset=True)
                same(ix.search_topk_grouped(Q[i], k, m, filter=filt)[0], i, "single")
                forms = [0, 0, 0, 0]
                if n:
                    forms[3 if list_path else 0] = 1
                assert ix.grouped_forms() == forms, (ctx, "single", i, ix.grouped_forms())
            for sel in S.chunks(len(Q)) + [np.arange(len(Q))]:
                ix.grouped_batch_forms(reset=True)
                got = ix.search_topk_grouped_batch(Q[sel], k, m, filter=filt)
                for j, i in enumerate(sel):
                    same(got[j], i, f"batch of {len(sel)}")
                out.append(got)
                forms = ix.grouped_batch_forms()
                assert sum(forms) == (len(sel) if n else 0), (ctx, forms)
                if hold_forms:
                    want_forms = S.chunk_forms(self.dtype, n, n_allowed, m, len(sel), list_path)
                    assert forms == want_forms, (ctx, f"batch of {len(sel)}", forms, want_forms)
        return out

    # -- capped ----------------------------------------------------------------------------------------------------
    def check_capped(self, sp, combos=S.CAPPED, allowed=None, filt=None, list_path=False, hold_forms=True):
        ix, st = self.ix, sp.st
        n = sp.n if allowed is None or len(allowed) else 0
        n_allowed = n if allowed is None else len(allowed)
        Q, out = sp.queries, []
        for combo in combos:
            need, m, diversify, picks = combo
            want = sp.capped_expect(self.O, combo, allowed=allowed)
            ctx = (self.dtype, self.copies, st.name, "capped", combo, allowed is not None, list_path)
            kw = dict(k=picks, lam=S.LAM if diversify else 0.0, diversify=diversify, w_embedding=S.W_E, w_lexical=S.W_L, filter=filt)

            def same(got, i, how):
                r, cos, comb, lexn, d = got
                w = want[i]
                assert np.array_equal(r, w["rows"]), (ctx, how, i, r[:6], w["rows"][:6])
                assert same_f32(cos, w["cos"]) and same_f32(comb, w["comb"]) and same_f32(lexn, w["lexn"]), (ctx, how, i)
                assert np.array_equal(d, w["docs"]), (ctx, how, i)

            for i in range(len(Q)):
                lr, ls, ml = sp.lex[i]
                ix.capped_forms(reset=True)
                same(ix.search_capped(Q[i], need, m, lex_rows=lr, lex_scores=ls, max_lex=ml, **kw), i, "single")
                forms = [0, 0, 0, 0]
                if n:
                    forms[3 if list_path else 0] = 1
                assert ix.capped_forms() == forms, (ctx, "single", i, ix.capped_forms())
            for sel in S.chunks(len(Q)) + [np.arange(len(Q))]:
                ix.capped_batch_forms(reset=True)
                got = ix.search_capped_batch(Q[sel], need, m, lex_rows=[sp.lex[i][0] for i in sel], lex_scores=[sp.lex[i][1] for i in sel],
                                             max_lex=[sp.lex[i][2] for i in sel], **kw)
                for j, i in enumerate(sel):
                    same(got[j], i, f"batch of {len(sel)}")
                out.append(got)
                forms = ix.capped_batch_forms()
                assert sum(forms) == (len(sel) if n else 0), (ctx, forms)
                if hold_forms:
                    want_forms = S.chunk_forms(self.dtype, n, n_allowed, m, len(sel), list_path)
                    assert forms == want_forms, (ctx, f"batch of {len(sel)}", forms, want_forms)
        return out

    def check(self, family, sp, **kw):
        return getattr(self, "check_" + family)(sp, **kw)


# ---------------------------------------------------------------- the walk
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype,copies,schedule", CONFIGS, ids=["-".join(c[:2]) for c in CONFIGS])
def test_walk(rlr, oracle, monkeypatch, dtype, copies, schedule, family):
    """every step of the plan (mutation_vectors.STEP_NAMES): the column and one family of entries after each one"""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    w = StateWalker(rlr, oracle, dtype, copies, schedule)
    try:
        for st in M.plan()[0]:
            col = w.mutate(st)
            sp = S.state_probes(oracle, st, dtype)
            if col.has_raw_phase and family == "grouped":       # before the tagging: an untagged tail, a dropped column
                w.check_grouped(sp, combos=S.RAW_GROUPED, docs=col.raw, phase="raw")
            w.tag(st, col)
            w.check(family, sp)
    finally:
        w.close()


# ---------------------------------------------------------------- row filters across the plan
@pytest.mark.parametrize("family", FAMILIES)
def test_filters_follow_the_walk(rlr, oracle, monkeypatch, family):
    """the plain f32 index: after every append and delete a filter made before the step is refused by all six entries
    with status -1, and a fresh one over every third row plus the step's probe rows gives the definition on both paths"""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    w = StateWalker(rlr, oracle, "f32", "plain", "no_copy")
    ix = w.ix
    q = M.stored(oracle)[:2]
    try:
        for st in M.plan()[0]:
            old = ix.filter_rows([0, 1, 2]) if st.n_before >= 3 else None
            col = w.mutate(st)
            w.tag(st, col)
            if st.op not in ("append", "delete"):
                if old is not None:
                    old.close()
                continue
            if old is not None:
                assert old.info()["stale"], st.name
                calls = {"range": (lambda: ix.search_range(q[0], 0.5, 5, filter=old), lambda: ix.search_range_batch(q, 0.5, 5, filter=old),
                                   lambda: ix.count_range(q[0], 0.5, filter=old), lambda: ix.count_range_batch(q, 0.5, filter=old)),
                         "grouped": (lambda: ix.search_topk_grouped(q[0], 3, 1, filter=old),
                                     lambda: ix.search_topk_grouped_batch(q, 3, 1, filter=old)),
                         "capped": (lambda: ix.search_capped(q[0], 3, 1, filter=old), lambda: ix.search_capped_batch(q, 3, 1, filter=old))}
                for call in calls[family]:
                    with pytest.raises(rlr.RlrError) as ei:
                        call()
                    assert ei.value.status == -1, st.name
                old.close()
            if st.n_after == 0:
                continue
            sp = S.state_probes(oracle, st)
            allowed = np.unique(np.concatenate([np.arange(0, st.n_after, 3), sp.positions]))
            more = {"range": {}, "grouped": dict(combos=FILTER_GROUPED), "capped": dict(combos=FILTER_CAPPED)}[family]
            with ix.filter_rows(allowed[::-1]) as f:
                assert f.info()["n_allowed"] == len(allowed)
                for path in ("list", "scan"):
                    f.set_path(path)
                    w.check(family, sp, allowed=allowed, filt=f, list_path=path == "list", **more)
    finally:
        w.close()


# ---------------------------------------------------------------- the sharing modes
def flat(results):
    """every array and number of a nested result, in order"""
    if isinstance(results, (list, tuple)):
        return [x for r in results for x in flat(r)]
    return [np.asarray(results)]


def test_sharing_modes_return_identical_bits(rlr, oracle, monkeypatch):
    """after the in-place append, the whole-tile delete and the refill past 4096 rows: the gate (mode 0), never (1) and
    wherever the shape allows (2) return the definition, in identical bits"""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    w = StateWalker(rlr, oracle, "f32", "plain", "no_copy")
    seen = []
    try:
        for st in M.plan()[0]:
            col = w.mutate(st)
            w.tag(st, col)
            if st.name not in S.SHARING_STEPS:
                continue
            seen.append(st.name)
            sp = S.state_probes(oracle, st)
            got = {}
            for mode in (2, 0, 1):
                w.set_sharing(mode)
                got[mode] = flat([w.check_range(sp, hold_forms=mode == 2), w.check_grouped(sp, combos=FILTER_GROUPED, hold_forms=mode == 2),
                                  w.check_capped(sp, combos=FILTER_CAPPED, hold_forms=mode == 2)])
                if mode == 1:                                    # never: every query of a batched call goes by rule
                    for forms in (w.ix.range_batch_forms(), w.ix.grouped_batch_forms(), w.ix.capped_batch_forms()):
                        assert forms[:3] == [0, 0, 0] and forms[3] > 0, (st.name, forms)
            w.set_sharing(2)
            for mode in (0, 1):
                assert len(got[mode]) == len(got[2])
                for a, b in zip(got[mode], got[2]):
                    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (st.name, mode)
        assert seen == list(S.SHARING_STEPS)
    finally:
        w.close()
