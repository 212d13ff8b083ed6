"""Every nomination band against rows built to err at its bound (band_vectors.py; test_band_vectors_cpu.py proves how far
into each band they reach and that half or a quarter of the band would lose the winner).  Each corpus goes through every
path that can serve it, at k = 1, 10 and 100 with the winner X exactly at rank k: the oracle's rows in the oracle's order,
score bits equal, no tolerance; `run_path` of test_gpu_numeric_edges.py asserts through the profile counters that the
intended path ran.  Over the summation-order corpus also: the engine's entry points (which build their own plan), a row
filter forced onto the masked scan, and the proof on the device that the corpus bites -- with a band of zero the plain
f32 scan loses X."""
import functools

import numpy as np
import pytest

import band_vectors as V
import test_gpu_numeric_edges as edges
from conftest import bits
from test_gpu_numeric_edges import PATHS, pad_batch, run_path

pytestmark = pytest.mark.gpu

KS = (1, 10, 100)
F32_PATHS = tuple(p for p in PATHS if not p.startswith("f16"))
F16_PATHS = ("f16_scan", "f16_gemm")
BUILDERS = {"absorption": V.absorption, "operand_rounding": V.operand_rounding, "q8_rounding": V.q8_rounding}


class MemoOracle:
    """the oracle, with the scan of a (corpus, query) pair and the binary16 image of a corpus computed once: `run_path`
    asks for them again for every path and k.  Keyed on the arrays' addresses; the corpora below are cached and read-only."""

    def __init__(self, O):
        self._O = O
        self._scans = {}
        self._images = {}

    def __getattr__(self, name):
        return getattr(self._O, name)

    def scan(self, rows, q, threads=1):
        key = (rows.ctypes.data, rows.shape, np.ascontiguousarray(q, np.float32).tobytes())
        if key not in self._scans:
            e = self._O.scan(rows, q, threads)
            e.setflags(write=False)
            self._scans[key] = (rows, e)                     # (the corpus is kept alive: its address is the key)
        return self._scans[key][1]

    def round_f16(self, a):
        if not isinstance(a, np.ndarray) or a.flags.writeable:
            return self._O.round_f16(a)
        key = (a.ctypes.data, a.shape)
        if key not in self._images:
            r = self._O.round_f16(a)
            r.setflags(write=False)
            self._images[key] = (a, r)
        return self._images[key][1]


@pytest.fixture(scope="module")
def memo(oracle):
    return MemoOracle(oracle)


@functools.lru_cache(maxsize=None)
def corpus(name, k, *args):
    """-> (rows, the winner query first in a batch of 16, facts); built once, never changed"""
    from oracle import oracle as O
    rows, qs, f = BUILDERS[name](O, k, *args)
    # (pad_batch pads at the width of test_gpu_numeric_edges.py; the other widths run the single query alone)
    batch = pad_batch(O, [qs[0]], 16) if rows.shape[1] == edges.DIM else qs[:1].copy()
    rows.setflags(write=False)
    batch.setflags(write=False)
    return rows, batch, f


def assert_winner(memo, rows, batch, f):
    """the case is the one the CPU test proved: X at rank k of the oracle's ranking"""
    wr, _ = edges.oracle_topk(memo, rows, batch[0], f["k"])
    assert wr[-1] == f["x"]


# ---------------------------------------------------------------- every path, every builder
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,f16", [("absorption", False), ("absorption", True), ("operand_rounding", False),
                                      ("operand_rounding", True), ("q8_rounding", False)])
def test_paths_keep_the_winner_at_the_edge_of_their_band(rlr, memo, monkeypatch, name, f16, k):
    args = () if name == "q8_rounding" else (768, 4096, True) if name == "absorption" and f16 else (True,) if f16 else ()
    rows, batch, f = corpus(name, k, *args)
    assert batch.shape == (16, edges.DIM)
    assert_winner(memo, rows, batch, f)
    for path in (F16_PATHS if f16 else F32_PATHS):
        run_path(rlr, memo, monkeypatch, path, rows, batch, k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("dim,span", [(128, 2), (1024, V.N_DECOYS), (1536, V.N_DECOYS)])
def test_scan_templates_of_other_widths(rlr, memo, monkeypatch, dim, span, f16, k):
    """the summation-order rows at the widths of the other scan kernels, single-query scan only"""
    rows, batch, f = corpus("absorption", k, dim, 1024, f16, span)
    monkeypatch.setattr(edges, "DIM", dim)                   # run_path builds its index at the module's width
    assert_winner(memo, rows, batch, f)
    run_path(rlr, memo, monkeypatch, "f16_scan" if f16 else "scan", rows, batch[:1], k)


# ---------------------------------------------------------------- the summation-order corpus through other entry points
def test_band_of_zero_loses_the_winner_on_the_f32_scan(rlr, memo):
    """the proof on the device that the corpus reaches the scan's summation order: without a band the best row returned
    is a decoy (whose exact score is below X's); with the default band it is X"""
    rows, batch, f = corpus("absorption", 1)
    ix = rlr.GpuIndex(768)
    try:
        ix.upload(rows)
        ix.profile_enable(True)
        r0, c0 = ix.search_topk(batch[0], 1, guard_eps=0.0)
        r1, c1 = ix.search_topk(batch[0], 1)
        p = ix.profile_read()
        assert p.n_scan_launches == 2 and p.n_batches == 0, p
        e = memo.scan(rows, batch[0])
        assert r1[0, 0] == f["x"] and bits(c1[0, :1])[0] == bits(e[f["x"]:f["x"] + 1])[0]
        assert r0[0, 0] != f["x"], "the scan kept X with no band: the rows do not reach its summation order"
        assert r0[0, 0] in f["decoys"] and c0[0, 0] < c1[0, 0]
    finally:
        ix.close()


def test_engine_entry_points_keep_the_winner(rlr, memo):
    """RagEngine.search / search_with_diversity make their own plan: X is the last of the 30 stage-1 candidates of
    top_k = 10 and the last row of the 30-row MMR pool (unordered on the device), from which the diversified result picks it"""
    rows, batch, f = corpus("absorption", 30)
    raw = f["raw_query"]
    eng = rlr.RagEngine(768)
    try:
        eng.index.upload(rows)                               # as built: add_document would re-normalise the rows
        eng._chunks = [rlr.DocumentChunk(str(i), "bands", "", i) for i in range(len(rows))]
        for stage, top_k in ((1, 10), (0, 10), (0, 30)):
            got = eng.search(raw, top_k, stage=stage)
            wr, wc, we, _ = memo.search(rows, raw, top_k, stage=stage)
            assert [g.row for g in got] == list(wr), (stage, top_k)
            assert np.array_equal(bits([g.score for g in got]), bits(wc)), (stage, top_k)
            assert np.array_equal(bits([g.embedding_score for g in got]), bits(we)), (stage, top_k)
            assert (got[-1].row == f["x"]) == ((stage, top_k) != (0, 10))
        for lam in (0.7, 0.3):
            got = eng.search_with_diversity(raw, 10, lam)
            wr, wc, we, _ = memo.search_with_diversity(rows, raw, 10, lam)
            assert [g.row for g in got] == list(wr), lam
            assert np.array_equal(bits([g.score for g in got]), bits(wc)), lam
            assert np.array_equal(bits([g.embedding_score for g in got]), bits(we)), lam
        assert f["x"] in [g.row for g in eng.search_with_diversity(raw, 10, 0.7)]
    finally:
        eng.close()


@pytest.mark.parametrize("k", KS)
def test_masked_scan_keeps_the_winner(rlr, memo, k):
    """a filter that allows X, the decoys, the champions and every other filler row, forced onto the masked scan:
    the oracle's ranking of the allowed rows"""
    from test_gpu_filter import expected
    rows, batch, f = corpus("absorption", k)
    special = np.r_[f["x"], f["decoys"], f["champions"]]
    allow = np.zeros(len(rows), bool)
    allow[::2] = True
    allow[V.X_ROW:V.C_ROW + 100] = False
    allow[special] = True
    allowed = np.flatnonzero(allow)
    e = memo.scan(rows, batch[0])
    wr, wc = expected(e, allowed, k)
    assert wr[-1] == f["x"]
    ix = rlr.GpuIndex(768)
    try:
        ix.upload(rows)
        with ix.filter_rows(allowed) as flt:
            flt.set_path("scan")
            assert flt.info()["path"] == "scan"
            r, c = ix.search_topk(batch[0], k, filter=flt)
            assert np.array_equal(r[0], wr), (k, r[0][:5], wr[:5])
            assert np.array_equal(bits(c[0]), bits(wc)), k
    finally:
        ix.close()
