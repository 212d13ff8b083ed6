"""tests/capped_batch_vectors.py held to itself and to the models it stands on: its one-query collect + finish equals
capped_vectors.device_path on every designed case of that file, the restated chunk equals the definition
(capped_vectors.define per query, then the greedy MMR) on every designed chunk and on random chunks and reports the designed
forms, every planted defect breaks the chunk named for it in the way named for it, and the unbroken model passes every chunk."""
import numpy as np
import pytest

import capped_batch_vectors as V
import capped_vectors as CV
import grouped_vectors as G


def answers_equal(got, want):
    return len(got) == len(want) and all(V.same(g["res"], w) for g, w in zip(got, want))


@pytest.mark.parametrize("name", list(CV.CASES))
def test_the_one_query_restatement_is_the_single_device_path(name):
    c = CV.CASES[name]()
    want_status, want = CV.run_device(c)
    status, res = V.single_device_path(c["a"], c["e"], c["docs"], c["lex_rows"], c["lex_scores"], c["w_e"], c["w_l"], c["need"],
                                       c["per_doc"], c["eps"], c["allowed"])
    assert status == want_status == c["status"], name
    if status == 0:
        assert V.same(res, want) and V.same(res, CV.run_define(c)), name


@pytest.mark.parametrize("name", list(V.CASES))
def test_the_chunk_equals_the_definition_on_every_designed_chunk(name):
    c = V.CASES[name]()
    assert c["lex_offsets"].size == len(c["e"]) + 1 and np.all(np.diff(c["lex_offsets"].astype(np.int64)) >= 0)
    got = V.chunk_path(c)
    assert answers_equal(got, V.define_chunk(c)), name
    assert [g["form"] for g in got] == V.FORMS[name], name
    # a query whose status is non-zero leaves pool size 0: the launches behind the finish do nothing for it
    # (a by-rule query rides the chunk with an empty lexical slice; what it leaves is not read)
    assert all(g["size"] == 0 for g in got if g["form"] in (1, 2)), name


@pytest.mark.parametrize("defect", V.DEFECTS)
def test_every_planted_defect_breaks_its_designed_chunk(defect):
    name, what = V.BROKEN_BY[defect]
    c = V.CASES[name]()
    got, want = V.chunk_path(c, defect=defect), V.define_chunk(c)
    if what == "answer":
        assert not answers_equal(got, want), (defect, name)
    elif what == "forms":
        # a handed-over query is answered by the single path, so the answers hold; what is lost is WHO was handed over
        assert answers_equal(got, want) and [g["form"] for g in got] != V.FORMS[name], (defect, name)
    else:
        assert what == "size" and answers_equal(got, want), (defect, name)
        assert any(g["size"] != 0 for g in got if g["form"] in (1, 2)), (defect, name)


@pytest.mark.parametrize("defect", V.DEFECTS)
def test_a_defect_never_raises_on_the_chunks_designed_for_others(defect):
    for make in V.CASES.values():
        V.chunk_path(make(), defect=defect)


def test_the_tables_agree():
    assert set(V.BROKEN_BY) == set(V.DEFECTS) and len(V.DEFECTS) == 10
    assert {name for name, _ in V.BROKEN_BY.values()} <= set(V.CASES) and set(V.FORMS) == set(V.CASES)
    assert {what for _, what in V.BROKEN_BY.values()} == {"answer", "forms", "size"}


def test_a_boundary_tie_hands_back_one_query_and_its_neighbour_stays_decided():
    c = V.CASES["boundary_tie_beside_a_decided_query"]()
    got = V.chunk_path(c)
    assert [g["form"] for g in got] == [2, 0] and [g["size"] for g in got] == [0, c["need"]]
    assert len(got[1]["res"]["rows"]) == c["k"]


def test_short_pools_run_the_greedy_selection_over_their_own_size():
    c = V.CASES["short_pools_under_mmr"]()
    got = V.chunk_path(c)
    assert [g["size"] for g in got] == [3, 3] and c["need"] == 5
    assert got[0]["res"]["rows"].tolist() == [0, 2, 1]          # row 1 duplicates row 0: picked last
    assert got[1]["res"]["rows"].tolist() == [1, 5, 3]


def test_the_lexical_limit_is_per_query():
    c = V.CASES["lexical_limit_per_query"]()
    assert int(c["lex_offsets"][-1]) == 9 > c["lex_cap"]
    assert [g["form"] for g in V.chunk_path(c)] == [0, 0, 3]
    assert [g["form"] for g in V.chunk_path(c, defect="lex_limit_on_total")] == [3, 3, 3]


def test_the_chunk_width_and_the_split_are_the_grouped_batch_rule():
    assert V.chunk_width(4097, 768 * 4, 4097, 8) == 8 and V.split(9, 8) == [5, 4]
    assert V.chunk_width(4097, 256 * 4, 4097, 8) == 3 and V.split(9, 3) == [3, 3, 3]
    assert V.chunk_width(65, 256 * 4, 65, 8) == 0 and V.split(9, 0) == [1] * 9
    assert V.split(3, 2) == [2, 1]                               # the lone remainder goes by rule


@pytest.mark.parametrize("per_doc", [1, 3, 8])
@pytest.mark.parametrize("diversify", [False, True])
def test_random_chunks_equal_the_definition(per_doc, diversify):
    rng = np.random.default_rng(100 * per_doc + diversify)
    for trial in range(12):
        nq, n = int(rng.integers(2, 9)), int(rng.integers(2, 90))
        e = rng.uniform(-1, 1, (nq, n)).astype(np.float32)
        a = (e + rng.uniform(-1, 1, e.shape).astype(np.float32) * np.float32(0.9e-4)).astype(np.float32)
        kind = trial % 3
        docs = None if kind == 0 else rng.integers(0, max(1, n // (1 + kind)), n).astype(np.uint32)
        if kind == 2:
            docs[rng.random(n) < 0.3] = G.DOC_NONE
        allowed = None if trial % 2 else np.flatnonzero(rng.random(n) < 0.6)
        if allowed is not None and allowed.size == 0:
            allowed = np.array([0])
        lex = []
        for q in range(nq):
            rows = np.flatnonzero(rng.random(n) < rng.choice([0.0, 0.1, 0.5]))
            lex.append([(int(r), float(rng.uniform(0.1, 5.0))) for r in rows])
        max_lex = [float(CV.max_lex_of([s for _, s in l])) for l in lex]
        need = int(rng.choice([1, 4, 25]))
        g = rng.standard_normal((n, 6)).astype(np.float32)
        sim = (g @ g.T / 6).astype(np.float32)
        c = V._chunk(e, docs, lex, max_lex, 0.7, 0.3, need, per_doc, eps=1e-4, a=a, allowed=allowed, diversify=diversify,
                     k=int(rng.integers(1, 8)), lam=float(rng.choice([0.3, 1.0])), sim=(sim + sim.T) / 2)
        got = V.chunk_path(c)
        assert answers_equal(got, V.define_chunk(c)), (per_doc, diversify, trial)
        assert all(g_["form"] in (0, 2) for g_ in got)
