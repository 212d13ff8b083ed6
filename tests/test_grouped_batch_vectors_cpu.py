"""tests/grouped_batch_vectors.py held to itself: the restated shared-table device path equals the definition
(grouped_vectors.expect per query) on every designed case and on random chunks, reports the designed status per query,
every planted defect breaks the designed case named for it (a defect no case catches would say nothing about the device),
and the workspace rule and the chunk split give the widths the issue states."""
import numpy as np
import pytest

import grouped_batch_vectors as V
import grouped_vectors as G

F32 = np.float32


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g[0], w) and g[0].dtype == np.uint64 for g, w in zip(got, want))


def wanted(case):
    return V.definition(case["exact"], case["docs"], case["k"], case["per_doc"], case.get("allowed"))


@pytest.mark.parametrize("name", list(V.CASES))
def test_the_restatement_equals_the_definition_on_every_designed_case(name):
    case = V.CASES[name]()
    a, e = case["nominated"], case["exact"]
    assert np.all(np.abs(a - e)[~np.isnan(a)] <= F32(case["eps"]))
    got = V.run(case)
    assert same(got, wanted(case)), name
    assert [s for _, s in got] == V.STATUS[name], name


@pytest.mark.parametrize("defect", [d for d in V.DEFECTS if d in V.BROKEN_BY])
def test_every_planted_defect_breaks_its_designed_case(defect):
    name = V.BROKEN_BY[defect]
    case = V.CASES[name]()
    got = V.run(case, defect=defect)
    if defect == "overflow_takes_chunk":
        # the answers are still the definition's (a handed-back query is answered by the single path); what is lost is
        # that the neighbour stays decided
        assert same(got, wanted(case)) and [s for _, s in got] == [1, 1] != V.STATUS[name]
        return
    assert not same(got, wanted(case)), (defect, name, "the answer itself must be wrong, not only the status")


def test_an_overflow_hands_back_one_query_and_its_neighbour_stays_decided():
    case = V.CASES["more_candidates_than_the_finish_holds"]()
    got = V.run(case)
    assert [s for _, s in got] == [1, 0] and same(got, wanted(case))
    assert got[0][0].tolist() == [5, 4] and got[1][0].tolist() == [0, 6]


@pytest.mark.parametrize("defect", V.DEFECTS)
def test_a_defect_leaves_the_cases_designed_for_others_alone_or_wrong_but_never_raises(defect):
    for make in V.CASES.values():
        V.run(make(), defect=defect)


def test_the_defect_list_and_the_case_table_agree():
    assert set(V.BROKEN_BY) | {"width_ignores_per_doc"} == set(V.DEFECTS) and len(V.DEFECTS) == 8
    assert set(V.BROKEN_BY.values()) <= set(V.CASES)
    assert set(V.STATUS) == set(V.CASES)


# ---- the workspace rule and the split -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [4097, 100_000, 1_000_000])
@pytest.mark.parametrize("per_doc", range(1, 9))
def test_768_elements_allow_eight_queries_for_every_per_doc(n_rows, per_doc):
    assert V.chunk_width(n_rows, 768 * 4, n_rows, per_doc) == 8


def test_256_elements_with_eight_per_document_narrow_the_chunk():
    n, row_bytes = 4097, 256 * 4
    w = V.chunk_width(n, row_bytes, n, 8)
    assert w == 3
    assert V.workspace_bytes(w, n, n, 8) <= n * row_bytes < V.workspace_bytes(w + 1, n, n, 8)
    assert V.chunk_width(n, row_bytes, n, 1) == 8
    assert V.chunk_width(n, row_bytes, n, 8, defect="width_ignores_per_doc") == 8 != w
    assert V.split(8, w) == [3, 3, 2] and V.forms_by_rule(8, w) == (8, 0)


def test_the_state_of_a_search_is_never_larger_than_what_it_searches():
    for n in (1, 65, 511, 4097, 70_000):
        for row_bytes in (1024, 2048, 3072, 4096):
            for per_doc in (1, 3, 8):
                for n_allowed in (1, max(1, n // 3), n):
                    w = V.chunk_width(n, row_bytes, n_allowed, per_doc)
                    assert w == 0 or (2 <= w <= 8 and V.workspace_bytes(w, n, n_allowed, per_doc) <= n * row_bytes)
                    if w < 8:
                        assert V.workspace_bytes(max(w, 1) + 1, n, n_allowed, per_doc) > n * row_bytes
    assert V.chunk_width(65, 1024, 65, 8) == 0               # 1024 slots x 8 values per query outweigh 65 rows of 1 KiB
    assert V.table_bits(1) == 10 and V.table_bits(512) == 10 and V.table_bits(513) == 11 and V.table_bits(4097) == 14


def test_the_remainder_is_split_evenly():
    assert V.split(9, 8) == [5, 4]
    assert V.split(17, 8) == [6, 6, 5]
    assert V.split(8, 8) == [8] and V.split(3, 8) == [3] and V.split(2, 8) == [2]
    assert V.split(1, 8) == [1] and V.split(5, 0) == [1] * 5
    assert V.split(3, 2) == [2, 1] and V.forms_by_rule(3, 2) == (2, 1)      # the lone remainder goes by rule
    for nq in range(1, 70):
        for w in range(2, 9):
            s = V.split(nq, w)
            assert sum(s) == nq and max(s) <= w and max(s) - min(s) <= 1 and len(s) == -(-nq // min(w, nq))


# ---- random chunks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_doc", [1, 2, 3, 8])
def test_random_chunks_equal_the_definition(per_doc):
    rng = np.random.default_rng(23 + per_doc)
    for trial in range(25):
        nq, n = int(rng.integers(2, 9)), int(rng.integers(1, 200))
        e = rng.uniform(-1, 1, (nq, n)).astype(np.float32)
        e[:, rng.integers(0, n)] = e[:, rng.integers(0, n)]                     # a tie here and there
        a = (e + rng.uniform(-1, 1, e.shape).astype(np.float32) * F32(0.9e-4)).astype(np.float32)
        kind = trial % 4
        docs = None if kind == 0 else rng.integers(0, max(1, n // (1 + kind)), n).astype(np.uint32)
        if kind == 3:
            docs[rng.random(n) < 0.3] = G.DOC_NONE
        allowed = None if trial % 3 else np.flatnonzero(rng.random(n) < 0.5)
        if allowed is not None and allowed.size == 0:
            allowed = np.array([0])
        k = int(rng.choice([1, 3, 10, 250]))
        got = V.device_path(a, e, docs, k, per_doc, 1e-4, allowed=allowed)
        assert same(got, V.definition(e, docs, k, per_doc, allowed)), (per_doc, trial)
        assert all(s == 0 for _, s in got)
