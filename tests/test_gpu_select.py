"""The rank searches of the top-k select driven with the designed score arrays of select_vectors.py (what they reach is
proved in test_select_vectors_cpu.py): rows uploaded as given, one-hot queries, so the nominated scores of a query are a
column written key by key -- digit-1 and digit-2 ranks at the wave and thread edges of find_rank_bin, the fused batch
select's find_bin and lds_find_rank_bin_1024, both halves of the key map, the zero crossing of band_floor_key, the
DIRECT / REFINE switch, every branch of sort_emit_rows with distinct keys, special values and the n % 4 tail.

Every search must return the oracle's rows in the oracle's order (NaN last, ties by row) with scores equal as bits.  The
single-query pipelines are also held to the model's candidate count (a floor that is too LOW still answers exactly: only
the count shows it), or to one large-candidate retry where the model's count passes 4096; the batched paths to one batch
without a hand-back (a floor that is too HIGH leaves fewer than k candidates)."""
import numpy as np
import pytest

import select_vectors as S
from conftest import bits
from test_gpu_parity import make_index
from test_gpu_tail import MODES, tail_mode

pytestmark = pytest.mark.gpu

assert set(MODES) == set(S.PIPELINES)
assert {m: (("fused" if e.get("RLR_TAIL", "1") != "0" else "split"), int(e.get("RLR_TAIL_DIRECT_MAX", S.DEFAULT_DIRECT_MAX)))
        for m, e in MODES.items() if m != "split"} == {m: v for m, v in S.PIPELINES.items() if m != "split"}
PIPELINES = dict(S.PIPELINES, max64=S.MODE64)

_scans = {}


def reference(oracle, key, rows, g):
    """the oracle's scores of one-hot query g over `rows`, computed once per (corpus, column)"""
    if (key, g) not in _scans:
        e = oracle.scan(rows, S.one_hot(rows.shape[1], g))
        e.setflags(write=False)
        _scans[(key, g)] = e
    return _scans[(key, g)]


def in_mode(mode):
    m = tail_mode("default" if mode == "max64" else mode)
    if mode == "max64":
        m.env = {"RLR_TAIL": "1", "RLR_TAIL_DIRECT_MAX": "64"}
    return m


def same_as_oracle(r, c, e, k, among=None, what=""):
    want = S.topk_rows(e, k, among)
    assert len(r) == len(want), (what, len(r), len(want))
    assert np.array_equal(np.asarray(r, np.int64), want), (what, list(r[:8]), list(want[:8]))
    assert np.array_equal(bits(c), bits(e[want])), what


def run_single(rlr, oracle, name, mode, dtype="f32"):
    rows, cases, two_eps = S.corpus(name)
    pl, dm = PIPELINES[mode]
    with in_mode(mode):
        ix = make_index(rlr, rows, dtype=dtype)
    try:
        for case in cases:
            g = case["col"]
            e = reference(oracle, name, rows, g)
            q = S.one_hot(rows.shape[1], g)
            for k in case["ks"]:
                what = (case["name"], k, mode)
                ix.profile_read(reset=True)
                r, c = ix.search_topk(q, k)
                same_as_oracle(r[0], c[0], e, k, what=what)
                if not case["counted"]:
                    continue
                p = ix.profile_read()
                mo = S.model(rows[:, g], k, two_eps, pl, dm)
                n_cand, n_retries = S.tail_report(mo, rows[:, g], k, pl, dm)
                print(f"{case['name']} k={k} {mode}: {p.n_candidates} candidates (model {n_cand}, floor {mo['bin1']}.{mo['bin2']}, "
                      f"{'DIRECT' if mo['mode'] == S.DIRECT else 'REFINE'}), {p.n_retries} retries (model {n_retries})")
                assert p.n_retries == n_retries, (what, p.n_retries, n_retries, mo)
                if mo["count"] <= S.CAP:
                    assert p.n_candidates == n_cand, (what, p.n_candidates, n_cand, mo)
    finally:
        ix.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", [n for n in S.SINGLE if not n.endswith("_f16")])
def test_single_query_select(rlr, oracle, name, mode):
    run_single(rlr, oracle, name, mode)


def test_mode_switch_at_direct_max_64(rlr, oracle):
    """class C under RLR_TAIL_DIRECT_MAX=64: 64 scores in or above the k-th's bin take DIRECT (64 candidates), 65 REFINE (50)"""
    run_single(rlr, oracle, "C", "max64")


@pytest.mark.parametrize("mode", ["default", "refine"])
@pytest.mark.parametrize("name", ["A_pos_f16", "A_neg_f16"])
def test_binary16_index_select(rlr, oracle, name, mode):
    """classes A and G over a binary16 index (tail_stage*_kernel<true>): the columns lie on the binary16 grid"""
    run_single(rlr, oracle, name, mode, dtype="f16")


@pytest.mark.parametrize("mode", ["default", "refine", "split"])
@pytest.mark.parametrize("name", ["A_pos", "A_neg", "A_big"])
def test_masked_scan_select(rlr, oracle, name, mode):
    """class A under a filter whose allowed rows are the designed ones: k = n_allowed puts the k-th on the last score the
    histogram holds at all (masked rows are not counted), k = n_allowed - 1 one above it; results and candidate count"""
    rows, cases, two_eps = S.corpus(name)
    pl, dm = PIPELINES[mode]
    with in_mode(mode):
        ix = make_index(rlr, rows)
    try:
        for case in cases:
            allowed = np.sort(case["rows"])
            e = reference(oracle, name, rows, case["col"])
            masked = np.full(len(rows), np.nan, np.float32)  # what the masked scan leaves: NaN on every row outside the filter
            masked[allowed] = rows[allowed, case["col"]]
            with ix.filter_rows(allowed) as f:
                f.set_path("scan")
                for k in (len(allowed), len(allowed) - 1):
                    ix.profile_read(reset=True)
                    r, c = ix.search_topk(S.one_hot(rows.shape[1], case["col"]), k, filter=f)
                    same_as_oracle(r[0], c[0], e, k, among=allowed, what=(case["name"], k, mode))
                    p = ix.profile_read()
                    mo = S.model(masked, k, two_eps, pl, dm)
                    print(f"{case['name']} k={k} {mode} masked: {p.n_candidates} candidates (model {mo['count']}), {p.n_retries} retries")
                    assert (p.n_candidates, p.n_retries) == (mo["count"], 0) and mo["count"] <= len(allowed), (case["name"], k, mode, mo)
    finally:
        ix.close()


BATCH_KS = (1, 3, 5, 6, 11, 12)


def run_batch(ix, oracle, key, rows, columns, k):
    ix.profile_read(reset=True)
    qs = np.stack([S.one_hot(rows.shape[1], g) for g in columns])
    r, c = ix.search_topk(qs, k)
    p = ix.profile_read()
    assert p.n_batches == 1 and p.n_batch_queries == len(columns) and p.n_batch_fallbacks == 0, (columns, k, p)
    for i, g in enumerate(columns):
        same_as_oracle(r[i], c[i], reference(oracle, key, rows, g), k, what=(key, g, k, len(columns)))


@pytest.mark.parametrize("n_queries", [2, 3, 4, 5, 6, 7, 8])
def test_shared_scan_select(rlr, oracle, monkeypatch, n_queries):
    """2..8 one-hot queries over columns of one corpus share one scan; the sample is the corpus, so the batched select finds
    rank k itself (the five-launch form: find_rank_bin per query)"""
    rows, cases, _ = S.corpus("batch")
    monkeypatch.setenv("RLR_BATCH_MIN", "2")                # read when the index is created
    ix = make_index(rlr, rows)
    try:
        first = sum(range(2, n_queries))                    # every group starts where the one before it ended
        columns = [(first + i) % len(cases) for i in range(n_queries)]
        for k in BATCH_KS:
            run_batch(ix, oracle, "batch", rows, columns, k)
    finally:
        ix.close()


@pytest.mark.parametrize("n_queries", [16, 64])
def test_matrix_core_batch_select(rlr, oracle, monkeypatch, n_queries):
    """16 queries: every column once through the matrix-core batch (binary16-representable columns: the nomination is
    exact); 64 queries: the one-workgroup-per-query select (batch_select_fused_kernel) and its own find_bin"""
    rows, cases, _ = S.corpus("batch")
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    ix = make_index(rlr, rows)
    try:
        columns = [i % len(cases) for i in range(n_queries)]
        for k in BATCH_KS:
            run_batch(ix, oracle, "batch", rows, columns, k)
    finally:
        ix.close()


def test_sampled_batch_select(rlr, oracle, monkeypatch):
    """above 131 072 rows the batch selects over a sample of the first 65 536 rows and filters the rest in the GEMM epilogue
    by the sample's floor tau: the designed top-k inside the sample and behind it, tau positive and negative"""
    rows, cases = S.sampled_corpus()
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    ix = make_index(rlr, rows)
    try:
        run_batch(ix, oracle, "sampled", rows, [c["col"] for c in cases], S.K_SAMPLED)
        run_batch(ix, oracle, "sampled", rows, [c["col"] for c in cases if c["sign"] == "neg"], S.K_SAMPLED)
    finally:
        ix.close()
