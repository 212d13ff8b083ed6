"""Coalescing of concurrent single-query searches (rlr_index_set_coalescing): callers on different threads share one pass
over the rows.  Every coalesced result must equal, bit for bit, the same call with coalescing off (and the oracle's
left-to-right scan where it is checked); the statistics (rlr_index_coalesce_stats) show that groups really formed and
which kernel served them."""
import threading

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

N_BIG = 1_000_000


def oracle_topk(O, rows, q, k):
    e = O.scan(rows, q)
    key = np.where(np.isnan(e), -np.inf, e)
    order = np.lexsort((np.arange(len(e)), -key.astype(np.float64)))[:k]
    return order.astype(np.uint64), e[order]


def queries(O, dim, n, seed):
    return [O.normalize(O.synth_query(dim, seed=seed + i)).astype(np.float32) for i in range(n)]


def run_threads(n_threads, work):
    """work(t) -> list of results, run on n_threads threads released together; exceptions re-raised"""
    barrier = threading.Barrier(n_threads)
    out, errs = [None] * n_threads, []

    def body(t):
        try:
            barrier.wait()
            out[t] = work(t)
        except BaseException as e:  # noqa: BLE001 -- re-raised on the main thread
            errs.append(e)

    ts = [threading.Thread(target=body, args=(t,)) for t in range(n_threads)]
    for th in ts:
        th.start()
    for th in ts:
        th.join(timeout=600)
    assert not any(th.is_alive() for th in ts), "a coalesced caller did not return"
    if errs:
        raise errs[0]
    return out


def same(a, b):
    (ra, ca), (rb, cb) = a, b
    return np.array_equal(ra, rb) and np.array_equal(bits(ca), bits(cb))


def consistent(st, n_calls):
    gs = st["group_size"]
    assert sum(s * gs[s] for s in range(9)) == st["n_grouped_queries"]
    assert sum(gs) == st["n_groups"]
    assert st["n_calls"] == n_calls
    assert st["n_solo"] + st["n_grouped_queries"] == n_calls


@pytest.fixture(scope="module")
def big_f32(rlr, oracle):
    ix = rlr.GpuIndex(768, "f32")
    ix.fill_synthetic(N_BIG, seed=4242, n_clusters=16)
    yield ix
    ix.close()


def test_default_is_off(rlr, oracle, big_f32):
    ix = big_f32
    qs = queries(oracle, 768, 8, 100)
    want = [ix.search_topk(q, 100) for q in qs]
    ix.coalesce_stats(reset=True)
    got = run_threads(8, lambda t: ix.search_topk(qs[t], 100))
    for t in range(8):
        assert same(got[t], want[t])
    st = ix.coalesce_stats()
    assert all(v == 0 for f, v in st.items() if f not in ("n_calls", "group_size")), st
    assert st["n_calls"] == 0 and not any(st["group_size"])


def test_f32_groups_are_bit_identical(rlr, oracle, big_f32):
    ix = big_f32
    qs = queries(oracle, 768, 48, 200)
    want = [ix.search_topk(q, 100) for q in qs]
    ix.set_coalescing(8, 5000)
    try:
        ix.coalesce_stats(reset=True)
        got = run_threads(8, lambda t: [ix.search_topk(qs[t * 6 + i], 100) for i in range(6)])
        st = ix.coalesce_stats()
    finally:
        ix.set_coalescing(0)
    flat = [r for per in got for r in per]
    for i in range(48):
        assert same(flat[i], want[i]), f"query {i} differs from the uncoalesced call"
    consistent(st, 48)
    assert st["n_groups"] >= 1 and sum(st["group_size"][2:]) > 0, st
    rows = oracle.synth_rows(N_BIG, 768, seed=4242, n_clusters=16)
    for i in (0, 13, 29, 47):
        wr, wc = oracle_topk(oracle, rows, qs[i], 100)
        assert np.array_equal(flat[i][0][0], wr) and np.array_equal(bits(flat[i][1][0]), bits(wc)), f"query {i} vs oracle"


def test_mixed_k_and_bands(rlr, oracle, big_f32):
    ix = big_f32
    qs = queries(oracle, 768, 8, 300)
    ks = [10, 30, 100, 10, 30, 100, 100, 10]
    eps_default = rlr.default_guard_eps(768)
    eps = [-1.0 if t % 2 == 0 else 2.0 * eps_default for t in range(8)]  # two bands, four callers each
    want = [ix.search_topk(qs[t], ks[t], guard_eps=eps[t]) for t in range(8)]
    ix.set_coalescing(8, 20000)
    try:
        for rnd in range(2):
            ix.coalesce_stats(reset=True)
            got = run_threads(8, lambda t: ix.search_topk(qs[t], ks[t], guard_eps=eps[t]))
            st = ix.coalesce_stats()
            for t in range(8):
                assert got[t][0].shape == (1, ks[t])
                assert same(got[t], want[t]), f"round {rnd} caller {t} (k={ks[t]}, eps={eps[t]})"
            consistent(st, 8)
            assert not any(st["group_size"][5:]), f"two bands shared a group: {st}"
    finally:
        ix.set_coalescing(0)
    # the k prefix: the k = 10 answer is the head of the k = 100 answer of the same query
    assert same((want[6][0][:, :10], want[6][1][:, :10]), ix.search_topk(qs[6], 10, guard_eps=eps[6]))


@pytest.mark.parametrize("dim", [1024, 768])
def test_binary16_rows(rlr, oracle, dim):
    ix = rlr.GpuIndex(dim, "f16")
    try:
        ix.fill_synthetic(N_BIG, seed=77, n_clusters=12)
        qs = queries(oracle, dim, 48, 400)
        want = [ix.search_topk(q, 100) for q in qs]
        ix.set_coalescing(8, 5000)
        ix.coalesce_stats(reset=True)
        got = run_threads(8, lambda t: [ix.search_topk(qs[t * 6 + i], 100) for i in range(6)])
        st = ix.coalesce_stats()
        ix.set_coalescing(0)
        flat = [r for per in got for r in per]
        for i in range(48):
            assert same(flat[i], want[i]), f"{dim}-d binary16 query {i} differs from the uncoalesced call"
        consistent(st, 48)
        assert st["n_groups_f16"] > 0 and st["n_groups_f16"] == st["n_groups"], st
        rows = oracle.round_f16(oracle.synth_rows(N_BIG, dim, seed=77, n_clusters=12))
        for i in (0, 31):
            wr, wc = oracle_topk(oracle, rows, qs[i], 100)
            assert np.array_equal(flat[i][0][0], wr) and np.array_equal(bits(flat[i][1][0]), bits(wc)), f"query {i} vs oracle"
    finally:
        ix.close()


def test_band_overflow_hands_members_back(rlr, oracle, monkeypatch):
    """10 000 exact copies of one row: every query near it has more rows in its band than the shared pass's finish takes
    (8192), so each member is re-run on the single-query pipeline inside the group's pass -- and is still exact."""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")  # (read at creation: groups qualify on a corpus this small)
    n, dim = 60000, 768
    rows = oracle.synth_rows(n, dim, seed=91, n_clusters=6)
    rows[20000:30000] = rows[5]
    ix = rlr.GpuIndex(dim, "f32")
    try:
        ix.upload(rows)
        qs = [rows[5].copy()] + [(oracle.normalize(rows[5] + 1e-3 * q)).astype(np.float32) for q in queries(oracle, dim, 7, 500)]
        ix.set_coalescing(8, 20000)
        ix.coalesce_stats(reset=True)
        got = run_threads(8, lambda t: ix.search_topk(qs[t], 100))
        st = ix.coalesce_stats()
        ix.set_coalescing(0)
        consistent(st, 8)
        assert st["n_groups"] >= 1 and st["n_handed_back"] > 0, st
        for t in range(8):
            wr, wc = oracle_topk(oracle, rows, qs[t], 100)
            assert np.array_equal(got[t][0][0], wr) and np.array_equal(bits(got[t][1][0]), bits(wc)), f"caller {t}"
    finally:
        ix.close()


def test_engine_calls_take_the_two_call_path(rlr, oracle):
    n, dim = N_BIG, 768
    eng = rlr.RagEngine(dim, "f32", device=0)
    try:
        eng.index.fill_synthetic(n, seed=4243, n_clusters=16)
        eng._chunks = [rlr.DocumentChunk(str(i), "synthetic", "", i) for i in range(n)]
        vocab = [f"w{i:03d}x" for i in range(40)] + ["common", "frequent"]
        rng = np.random.default_rng(5)
        for r in range(0, n, 500):  # 2000 rows carry text
            eng.lexical.add_chunk(r, " ".join(rng.choice(vocab, size=12)))
        qs = queries(oracle, dim, 8, 600)
        texts = ["w001x common", "w017x frequent", "w003x w004x", "common"] * 2

        def call(t, text_too):
            a = eng.search_with_diversity(qs[t], 10, 0.3)
            b = eng.search_with_diversity(qs[t], 10, 0.3, query_text=texts[t]) if text_too else []
            return [(r.row, np.float32(r.score).view(np.uint32), np.float32(r.embedding_score or 0).view(np.uint32))
                    for r in a + b]

        want = [call(t, True) for t in range(8)]
        eng.index.set_coalescing(8, 5000)
        eng.index.coalesce_stats(reset=True)
        got = run_threads(8, lambda t: call(t, True))
        st = eng.index.coalesce_stats()
        eng.index.set_coalescing(0)
        for t in range(8):
            assert got[t] == want[t], f"caller {t}: engine results differ with coalescing on"
        assert st["n_engine_handbacks"] > 0 and st["n_calls"] > 0, st
        # and off again: the fused calls are back
        eng.index.coalesce_stats(reset=True)
        assert call(0, True) == want[0]
        assert eng.index.coalesce_stats()["n_engine_handbacks"] == 0
    finally:
        eng.close()


def test_mutations_between_rounds(rlr, oracle, monkeypatch):
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    dim = 768
    rows = oracle.synth_rows(40000, dim, seed=321, n_clusters=8)
    ix = rlr.GpuIndex(dim, "f32")
    try:
        ix.upload(rows)
        ix.set_coalescing(8, 3000)
        for rnd in range(3):
            stored = ix.fetch_rows(np.arange(len(ix)))
            qs = queries(oracle, dim, 16, 700 + 16 * rnd)
            ix.coalesce_stats(reset=True)
            got = run_threads(8, lambda t: [ix.search_topk(qs[2 * t + i], 50) for i in range(2)])
            st = ix.coalesce_stats()
            consistent(st, 16)
            for t in range(8):
                for i in range(2):
                    wr, wc = oracle_topk(oracle, stored, qs[2 * t + i], 50)
                    r, c = got[t][i]
                    assert np.array_equal(r[0], wr) and np.array_equal(bits(c[0]), bits(wc)), f"round {rnd} caller {t}.{i}"
            # the mutators, alone (the header's external exclusion)
            ix.append(oracle.synth_rows(3000, dim, seed=900 + rnd, n_clusters=8))
            ix.delete_rows(np.array([3, 17 + rnd, len(ix) - 1], dtype=np.uint64))
    finally:
        ix.close()


def test_set_coalescing_rejects_bad_arguments(rlr, big_f32):
    with pytest.raises(rlr.RlrError):
        big_f32.set_coalescing(9)
    big_f32.set_coalescing(1, 0)  # 0 / 1: off
    assert big_f32.coalesce_stats()["n_calls"] >= 0
