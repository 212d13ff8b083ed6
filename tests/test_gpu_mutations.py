"""The index's state machine on the device: one index per configuration walks the whole plan of mutation_vectors.py
(uploads, appends into and beyond the allocation, deletes at every position of a tile, an empty and a refilled index,
the nomination copies switched on, dropped and widened on the way).  After EVERY step the row count and every stored row
equal the host mirror bit for bit, and the step's probes -- stored rows as queries, which a stale copy entry costs their
own position (test_mutation_vectors_cpu.py proves it) -- return the oracle's rows and score bits as single queries, in
groups of 8 and as one call, while the profile counters prove which copy served them.  The oracle's scan of every
(mirror, probe) pair is computed once (mutation_vectors.step_probes) and shared by all configurations.

Then the 8-bit band statistic across an append (rows with a larger error norm than any stored one, appended into
reserved capacity and beyond it, and small rows appended in place behind the rows that own the maximum), row filters across the plan, and the multi-chunk compaction of 4096-d rows.

Two limits.  The image_single_query configuration widens the image to single queries only at its own toggle, behind the
in-place appends: until then the image those appends extended is read by the batched passes alone, afterwards (the later
deletes, the smaller upload, the appends into the emptied and the shrunk index) by the single-query image scan too.  On a
binary16 index the counters cannot tell the image from the rows (see Walker.search).

GPU time (MI355X): DESIGN.md, "Mutations"."""
import numpy as np
import pytest

import mutation_vectors as M
from conftest import bits

pytestmark = pytest.mark.gpu

# (dtype, copies): the configurations of the plan run; every one with a copy in two schedules
CONFIGS = [("f32", "plain"), ("f32", "image"), ("f32", "image_single_query"), ("f32", "q8"),
           ("f16", "plain"), ("f16", "image"), ("f16", "q8")]
RUNS = [(d, c, s) for d, c in CONFIGS for s in (("on_before_upload", "on_after_step_5") if c != "plain" else ("no_copy",))]


class Walker:
    """an index of one configuration, the copy flags it has been given so far, and the checks after a step"""

    def __init__(self, rlr, O, dtype, copies, schedule):
        self.rlr, self.O, self.dtype, self.copies, self.schedule = rlr, O, dtype, copies, schedule
        self.ix = rlr.GpuIndex(M.DIM, dtype)     # (RLR_BATCH_MIN is read here)
        self.ix.profile_enable(True)
        self.on = False                          # a copy is switched on
        self.single = False                      # single queries nominate over the image

    def close(self):
        self.ix.close()

    # -- the copy flags ------------------------------------------------------
    def _enable(self):
        if self.copies == "q8":
            self.ix.enable_batch_image(False, q8=True)
        else:
            self.ix.enable_batch_image(True, single_query=self.single)
        self.on = True

    def toggle(self, what):
        if self.copies == "plain":
            return
        if what in ("on_before_upload", "on_after_step_5"):
            if what == self.schedule:
                self._enable()
        elif what == "drop":
            if self.on:
                self.ix.enable_batch_image(False)
                self.on = False
        elif what == "reenable":
            self._enable()
        elif what == "widen_to_single_query":
            if self.copies == "image_single_query":
                assert self.on and not self.single
                self.single = True
                self._enable()                   # on=True -> single_query=True: the image stays as it is

    # -- one step ------------------------------------------------------------
    def apply(self, st):
        pool = M.stored(self.O, "f32")           # (a binary16 index rounds on the way in)
        if st.op == "toggle":
            self.toggle(st.arg)
        elif st.op == "reserve":
            self.ix.reserve(st.arg)
        elif st.op == "upload":
            self.ix.upload(pool[st.ids_after])
        elif st.op == "append":
            first = self.ix.append(pool[st.ids_after[st.n_before:]])
            assert first == st.n_before, st.name
        elif st.op == "delete":
            self.ix.delete_rows(st.arg)

    def check_rows(self, st):
        assert len(self.ix) == st.n_after, (st.name, len(self.ix), st.n_after)
        if st.n_after:
            got = self.ix.fetch_rows(np.arange(st.n_after))
            want = M.stored(self.O, self.dtype)[st.ids_after]
            assert np.array_equal(bits(got), bits(want)), (st.name, np.flatnonzero((bits(got) != bits(want)).any(axis=1))[:8])

    def bytes_per_element(self):
        if self.on and self.copies == "q8":
            return 1
        return 2 if self.dtype == "f16" or (self.on and self.single) else 4

    def search(self, st, probes, idx, k, ctx):
        """one call of the queries `idx` at top-k: the oracle's rows and bits, and the counters of the path that must serve"""
        n, nq = st.n_after, len(idx)
        self.ix.profile_read(reset=True)
        r, c = self.ix.search_topk(probes.queries[idx], k)
        p = self.ix.profile_read()
        kk = min(k, n)
        assert r.shape == (nq, kk) and c.shape == (nq, kk), (ctx, r.shape)
        if n == 0:
            return
        for j, qi in enumerate(idx):
            wr, wc = probes.expected(qi, k)
            if qi < probes.n_self:
                assert wr[0] == probes.positions[qi], (ctx, qi)        # the probe's own position comes first
            assert np.array_equal(r[j], wr), f"{ctx} query {qi}: rows differ: got {r[j][:5]} want {wr[:5]}"
            assert np.array_equal(bits(c[j]), bits(wc)), f"{ctx} query {qi}: scores differ: got {c[j][:5]} want {wc[:5]}"
        assert p.n_f16_range_fallbacks == 0, (ctx, p)
        if nq == 1 or n < M.BATCH_ROWS:          # the single-query pipeline, once per query, over the copy that is on
            assert p.n_batches == 0 and p.n_scan_launches == nq, (ctx, p)
            assert p.scan_bytes == nq * n * M.DIM * self.bytes_per_element(), (ctx, p, self.bytes_per_element())
        else:                                    # one batched pass; >= 16 queries over f32 rows without an image count as such
            assert p.n_batches == 1 and p.n_batch_queries == nq, (ctx, p)
            image = self.on and self.copies.startswith("image")
            without = int(nq >= 16 and self.dtype == "f32" and not image)
            assert p.n_batches_without_image == without, (ctx, p)
            # the operand the pass streamed: 2 bytes per element over the image (and over binary16 rows), 4 over f32 rows.
            # On a binary16 index the image and the rows have one element width and the same values, so no counter
            # tells them apart there: those walks hold the results to the oracle whichever of the two served.
            assert p.batch_gemm_bytes == n * M.DIM * (2 if image or self.dtype == "f16" else 4), (ctx, p)

    def check_probes(self, st):
        probes = M.step_probes(self.O, st, self.dtype)
        for idx, k in probes.groups():
            ctx = (self.dtype, self.copies, self.schedule, st.name, k)
            for qi in idx:
                self.search(st, probes, np.array([qi]), k, ctx + ("single",))
            for g in range(0, len(idx), 8):
                self.search(st, probes, idx[g:g + 8], k, ctx + ("group of 8",))
            self.search(st, probes, idx, k, ctx + ("one call",))


@pytest.mark.parametrize("dtype,copies,schedule", RUNS, ids=["-".join(r) for r in RUNS])
def test_plan(rlr, oracle, monkeypatch, dtype, copies, schedule):
    """every step of the plan (mutation_vectors.STEP_NAMES), checked after each one"""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    w = Walker(rlr, oracle, dtype, copies, schedule)
    try:
        for st in M.plan()[0]:
            w.apply(st)
            w.check_rows(st)
            w.check_probes(st)
        assert [st.name for st in M.plan()[0]] == list(M.STEP_NAMES)
    finally:
        w.close()


# ---------------------------------------------------------------- row filters across the plan
def test_filters_follow_the_plan(rlr, oracle, monkeypatch):
    """the plain f32 index: after every append and delete a filter made before the step is refused, and a fresh one over
    every third row plus the step's seam rows gives the oracle's result over those rows on both of its paths"""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    w = Walker(rlr, oracle, "f32", "plain", "no_copy")
    try:
        for st in M.plan()[0]:
            old = w.ix.filter_rows([0, 1, 2]) if st.n_before >= 3 else None
            w.apply(st)
            if st.op not in ("append", "delete"):
                if old is not None:
                    old.close()
                continue
            if old is not None:
                assert old.info()["stale"], st.name
                with pytest.raises(rlr.RlrError) as ei:
                    w.ix.search_topk(M.stored(oracle)[0], 1, filter=old)
                assert ei.value.status == -1, st.name
                old.close()
            if st.n_after == 0:
                continue
            probes = M.step_probes(oracle, st)
            allowed = np.unique(np.concatenate([np.arange(0, st.n_after, 3), probes.positions]))
            with w.ix.filter_rows(allowed[::-1]) as f:
                assert f.info()["n_allowed"] == len(allowed)
                for path in ("list", "scan"):
                    f.set_path(path)
                    for idx, k in probes.groups():
                        kk = min(k, len(allowed))
                        r, c = w.ix.search_topk(probes.queries[idx], kk, filter=f)
                        assert r.shape == (len(idx), kk), (st.name, path, r.shape)
                        for j, qi in enumerate(idx):
                            wr, wc = probes.expected(qi, kk, allowed)
                            assert np.array_equal(r[j], wr), (st.name, path, k, qi, r[j][:5], wr[:5])
                            assert np.array_equal(bits(c[j]), bits(wc)), (st.name, path, k, qi)
                        for qi in idx[:: max(1, len(idx) // 8)]:          # and as single queries
                            r1, c1 = w.ix.search_topk(probes.queries[qi], kk, filter=f)
                            wr, wc = probes.expected(qi, kk, allowed)
                            assert np.array_equal(r1[0], wr) and np.array_equal(bits(c1[0]), bits(wc)), (st.name, path, k, qi)
    finally:
        w.close()


# ---------------------------------------------------------------- the 8-bit band statistic across an append
def oracle_topk(O, rows, q, k):
    e = O.scan(rows, q)
    order = np.lexsort((np.arange(len(e)), -e.astype(np.float64)))[:k]
    return order.astype(np.uint64), e[order]


@pytest.mark.parametrize("k", M.BAND_KS)
@pytest.mark.parametrize("form", M.BAND_FORMS)
def test_band_grows_with_appended_rows(rlr, oracle, monkeypatch, form, k):
    """X, its decoys and its champions are appended to an 8-bit index that holds only filler, whose error norms are a
    sixth of theirs: a band from the old maximum loses X (test_mutation_vectors_cpu.py).  Into reserved capacity the
    copy is extended in place, beyond it everything is rebuilt.  The third form is the other direction: filler appended
    in place behind X and its decoys, then the last row deleted -- partial builds that must keep the old maximum."""
    monkeypatch.setenv("RLR_BATCH_MIN", "100000")
    reverse = form == "small_rows_appended_behind"
    base, tail, q, f = M.band_case_reversed(oracle, k) if reverse else M.band_case(oracle, k)
    dim = f["dim"]
    ix = rlr.GpuIndex(dim)
    try:
        ix.enable_batch_image(False, q8=True)
        if form != "append_outgrows_capacity":
            ix.reserve(2 * len(base))            # before the upload: the copy is sized for it too
        ix.upload(base)
        ix.profile_enable(True)

        def check(rows, want_x_at):
            ix.profile_read(reset=True)
            r, c = ix.search_topk(q, k)
            p = ix.profile_read()
            wr, wc = oracle_topk(oracle, rows, q, k)
            if want_x_at is not None:
                assert wr[k - 1] == want_x_at
            assert np.array_equal(r[0], wr), (form, k, r[0], wr)
            assert np.array_equal(bits(c[0]), bits(wc)), (form, k)
            assert p.n_batches == 0 and p.n_scan_launches == 1 and p.scan_bytes == len(rows) * dim, (form, k, p)

        check(base, f["x"] if reverse else None)
        assert ix.append(tail) == len(base)
        rows = np.concatenate([base, tail])
        assert np.array_equal(bits(ix.fetch_rows(np.arange(len(rows)))), bits(rows))
        check(rows, f["x"])
        if reverse:                              # a partial build of no rows at all must keep the statistic too
            ix.delete_rows([len(rows) - 1])
            rows = rows[:-1]
            check(rows, f["x"])
        ix.delete_rows(f["decoys"])              # the statistic may stay large: still exact
        rows = np.delete(rows, f["decoys"], axis=0)
        check(rows, f["x"])
    finally:
        ix.close()


# ---------------------------------------------------------------- multi-chunk compaction of wide rows
def test_wide_rows_compact_across_chunks(rlr, oracle):
    """40 000 rows of 4096-d f32 (16 KiB each: a compaction chunk is 16 384 rows), one delete whose survivors behind the
    first deleted row fill more than two chunks: the rows around every chunk seam, around the first deleted row, at the
    end and on a 1000-row sample are the generator's"""
    dead, keep, positions, seams = M.wide_case()
    ix = rlr.GpuIndex(M.WIDE_DIM)
    try:
        ix.fill_synthetic(M.WIDE_ROWS, seed=M.WIDE_SEED)
        ix.delete_rows(dead)
        assert len(ix) == len(keep)
        got = ix.fetch_rows(positions)
        want = M.wide_expected(oracle, keep, positions)
        bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
        assert len(bad) == 0, (positions[bad][:8], keep[positions[bad]][:8])
        for s in seams[:2]:                       # a row that moved across a seam, as the query
            p = s + 1
            row = want[np.searchsorted(positions, p)]
            q = oracle.normalize(row)
            r, c = ix.search_topk(q, 1)
            assert r[0, 0] == p, (s, r)
            assert bits(c[0, :1])[0] == bits(oracle.scan(row[None], q))[0], (s, c)
    finally:
        ix.close()
