"""state_vectors.py checked without a GPU: the document rule makes caps bind, the column model follows the library's
stated rules, every plantable fault changes the expected result of a probe the GPU test sends, every range threshold
case separates rows, and the restated device paths hand no probe back.  Every test prints what it measured (pytest -s).

Measured (256-d f32 mirror): grouped probes that differ from plain top-k per step 25 of 72 .. 38 of 96 (0.33..0.40;
the assertion is the quarter the issue sets); 42..48 range pairs per step; largest candidate list of a grouped / capped
collect 27 of 2048.  Results that differ per affected step: image faults through the one-call range GEMM F1 2..23, F2
2..44, F3 2..27, F4 20..42, F5 38..39, F7 2..30 of 42..48 pairs (F6a / F6b leave the image right); every fault of
mutation_vectors.FAULTS through the top-k hand-off of the 9..12 self-probes that ask their own rank-25 score at cap 10,
over the image and over the 8-bit copy alike: F1 1..6, F2 1..12, F3 1..8, F4 5..12, F5 11..12, F7 1..7 on every affected
step, F6b 1..12 on all 16, F6a 1..12 on 15 of 16 (a foreign scale moves a score by a factor of 0.6..1.7 only: the three
changed rows of delete_in_last_partial_tile stay in place at k = 10; the probe's own row is lost on the two refills);
column faults through the grouped probes C1 10..92, C2 36..58, C3 32, C4 72..118, C5 32; the stride fault 29..38 pairs."""
import numpy as np
import pytest

import capped_batch_vectors as CB
import capped_vectors as CV
import grouped_batch_vectors as GB
import mutation_vectors as M
import range_batch_vectors as RB
import state_vectors as S


def steps():
    return M.plan()[0]


def row_steps():
    return [s for s in steps() if s.op in ("upload", "append", "delete")]


# ---------------------------------------------------------------- documents and the column
def test_document_rule_has_large_small_and_no_documents():
    ids = np.arange(M.plan()[1])
    d = S.doc_of(ids)
    big, none = d < S.N_BIG, d == S.DOC_NONE
    print(f"large {big.mean():.3f} in {S.N_BIG} documents, none {none.mean():.3f}, small documents {len(np.unique(d[~big & ~none]))}")
    assert 0.6 < big.mean() < 0.7 and 0.09 < none.mean() < 0.11 and len(np.unique(d[~big & ~none])) > 900
    assert S.runs(np.array([3, 3, S.DOC_NONE, 4, 4, 4], np.uint32)) == [(0, 2, 3), (3, 3, 4)]


def test_column_model_follows_the_stated_rules():
    seen = set()
    for st in steps():
        c = S.column(st)
        assert np.array_equal(c.tagged, S.doc_of(st.ids_after)), st.name
        if st.op == "upload":
            assert (c.raw == S.DOC_NONE).all() and c.tag == "whole"
        elif st.op == "append":
            assert np.array_equal(c.raw[:st.n_before], S.doc_of(st.ids_before)) and (c.raw[st.n_before:] == S.DOC_NONE).all()
            seen.add(c.tag)
        else:
            assert c.tag is None and np.array_equal(c.raw, c.tagged), st.name
        for first, count, doc in S.runs(c.tagged[st.n_before:]) if c.tag == "rows" else ():
            assert (c.tagged[st.n_before + first:st.n_before + first + count] == doc).all()
    assert seen == {"rows", "whole"}


@pytest.mark.parametrize("fault", S.COLUMN_FAULTS)
def test_probes_see_column_fault(oracle, fault):
    reached = []
    for st in steps():
        if not S.column_fault_applies(st, fault):
            continue
        good, bad = S.column(st), S.column(st, fault)
        sp = S.state_probes(oracle, st)
        lost = 0
        for phase, combos in (("raw", S.RAW_GROUPED if good.has_raw_phase else ()), ("tagged", S.GROUPED)):
            g, b = getattr(good, phase), getattr(bad, phase)
            if np.array_equal(g, b):
                continue
            for k, m in combos:
                want = sp.grouped_expect(k, m, docs=g)
                got = sp.grouped_expect(k, m, docs=b)
                lost += sum(not (np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2])) for x, y in zip(got, want))
        stale = int((good.raw != bad.raw).sum())
        print(f"{fault} {st.name}: {stale} wrong column entries, {lost} grouped results differ")
        if stale:
            assert lost, (fault, st.name)
            reached.append(st.name)
    assert reached, fault


# ---------------------------------------------------------------- copy faults through the range GEMM
@pytest.fixture(scope="module")
def model(oracle):
    return M.CopyModel(oracle)


@pytest.mark.parametrize("fault", M.FAULTS)
def test_range_pairs_see_copy_fault(oracle, model, fault):
    affected = 0
    for st in row_steps():
        if not M.fault_applies(st, fault) or st.n_after < M.BATCH_ROWS:
            continue
        sp = S.state_probes(oracle, st)
        got, status, n_stale = S.range_under_copy(model, sp, fault)
        if fault not in S.IMAGE_FAULTS:
            assert n_stale == 0, (fault, st.name)                  # the 8-bit copy's faults leave the image right
            continue
        if n_stale == 0:
            continue
        lost = S.differs(got, sp.range_expect(S.RANGE_CAPS[1]))
        affected += 1
        print(f"{fault} {st.name}: {n_stale} stale positions, {len(lost)} of {len(got)} range pairs differ {[sp.cases[i] for i in lost[:3]]}")
        assert lost and status == [0] * len(got), (fault, st.name, n_stale)
    assert affected or fault not in S.IMAGE_FAULTS, fault


@pytest.mark.parametrize("fault", M.FAULTS)
def test_hand_off_probes_see_copy_fault(oracle, model, fault):
    """a self-probe asking its own rank-25 score at cap 10 has more hits than cap: the single entry takes its rows from
    the top-k path at k = 10 over the copy that is on.  mutation_vectors.CopyModel.lost nominates with what the copy
    holds under the fault and selects with the widest band: results that differ from the oracle's top 10"""
    affected = 0
    for st in row_steps():
        if not M.fault_applies(st, fault) or not st.n_after:
            continue
        sp = S.state_probes(oracle, st)
        assert all(sp.range_expect(S.RANGE_CAPS[0])[sp.n_self + i][2] > S.RANGE_CAPS[0] for i in range(sp.n_self)), st.name
        for kind in ("image", "q8"):
            lost, n_stale = model.lost(st, sp, kind, fault)
            if n_stale == 0:
                continue
            with np.errstate(all="ignore"):                       # (a copy of zeros nominates 0: no bin)
                own = sum(sp.positions[qi] not in M.B.select(model.nominate(kind, *M.copy_after(st, kind, fault), sp.queries[qi:qi + 1])[0],
                                                             sp.scores[qi], k, model.band) for qi, k in lost)
            print(f"{fault} {st.name} {kind}: {n_stale} stale positions, {len(lost)} of {sp.n_self} hand-off results differ, "
                  f"{own} lack the probe's own row")
            affected += bool(lost)
    assert affected, fault


def test_stride_fault_is_seen_behind_the_shared_scan(oracle):
    reached = 0
    for st in row_steps():
        if not S.stride_fault_applies(st):
            continue
        sp = S.state_probes(oracle, st)
        lost = 0
        for sel in S.chunks(len(sp.taus)):
            if len(sel) < 2:
                continue
            want = [sp.range_expect(S.RANGE_CAPS[1])[i] for i in sel]
            assert not S.differs(S.range_under_stride(sp, sel, S.RANGE_CAPS[1], RB.stride_of(st.n_after)), want), st.name
            lost += len(S.differs(S.range_under_stride(sp, sel, S.RANGE_CAPS[1], RB.stride_of(st.n_before)), want))
        print(f"{S.STRIDE_FAULT} {st.name}: stride {RB.stride_of(st.n_before)} for {RB.stride_of(st.n_after)}: {lost} range pairs differ")
        assert lost, st.name
        reached += 1
    assert reached


# ---------------------------------------------------------------- what the probes ask
def test_probe_sets_stay_within_sixteen_queries_and_name_the_seam(oracle):
    for st in steps():
        sp = S.state_probes(oracle, st)
        assert len(sp.queries) <= S.MAX_PROBES and len(sp.queries) == sp.n_self + M.N_ORDINARY, st.name
        f = st.first_changed
        if st.n_after and f is not None:
            assert {p for p in (f - 1, f, f + 1, st.n_after - 1) if 0 <= p < st.n_after} <= set(sp.positions.tolist()), st.name
        sizes = [len(l[0]) for l in sp.lex]
        assert sizes[0] == 0 and (not st.n_after or np.array_equal(sp.lex[1][0], np.unique(sp.positions))), st.name
        for rows, scores, ml in sp.lex:
            assert (np.diff(rows.astype(np.int64)) > 0).all() and (rows < max(st.n_after, 1)).all() and (scores > 0).all() and ml > 0
        if st.n_after >= M.BATCH_ROWS:
            assert max(sizes) >= 30, (st.name, sizes)
        assert len(sp.taus) == (2 * sp.n_self + 2 * len(S.RANKS) * M.N_ORDINARY if st.n_after else M.N_ORDINARY), st.name


def test_caps_bind_on_every_step(oracle):
    for st in steps():
        if st.n_after < 25:
            continue
        sp = S.state_probes(oracle, st)
        differ = total = 0
        for k, m in S.GROUPED:
            plain = sp.topk(k)
            for got, want in zip(sp.grouped_expect(k, m), plain):
                total += 1
                differ += not np.array_equal(got[0], want)
        print(f"{st.name}: {differ} of {total} grouped probes differ from plain top-k")
        assert 4 * differ >= total, (st.name, differ, total)


def test_capped_definitions_are_capped_and_lexical(oracle):
    """on every step with rows some capped probe holds a lexical row and some document is at its cap"""
    for st in steps():
        if st.n_after < 25:
            continue
        sp = S.state_probes(oracle, st)
        lexical = full = 0
        for combo in S.CAPPED:
            for res in sp.capped_expect(oracle, combo):
                lexical += bool((res["lexn"] > 0).any())
                tagged = res["docs"][res["docs"] != S.DOC_NONE]
                full += bool(tagged.size and np.bincount(tagged).max() == combo[1])
                assert not tagged.size or np.bincount(tagged).max() <= combo[1]
        assert lexical and full, (st.name, lexical, full)


def test_every_tau_case_separates_rows(oracle):
    """a self-probe's 0.75 takes exactly its own row; the score at a rank takes that row in and one ulp above leaves it
    out; every case leaves rows out, every case but `above rank 1` takes rows in; both caps lie on both sides of n_total"""
    for st in steps():
        if not st.n_after:
            continue
        sp = S.state_probes(oracle, st)
        full = sp.range_expect(st.n_after)
        totals = {}
        for i, (rows, _, total) in enumerate(full):
            case = sp.cases[i]
            assert total < st.n_after, (st.name, case)
            if case == "self":
                assert rows.tolist() == [sp.positions[sp.pair_query[i]]], (st.name, i)
            elif case.startswith("self rank"):                   # the probe's own row first, more hits than the small cap
                assert rows[0] == sp.positions[sp.pair_query[i]] and total == min(S.RANKS[1], max(st.n_after // 2, 1)) > S.RANGE_CAPS[0]
            elif case.startswith("rank"):
                assert total >= 1 and total < st.n_after
                totals[(sp.pair_query[i], case)] = total
            else:
                assert total < totals[(sp.pair_query[i], case[6:])], (st.name, case)
        if st.n_after >= M.BATCH_ROWS:
            t = sorted(set(totals.values()))
            assert t[0] < S.RANGE_CAPS[0] < t[-1] and any(S.RANGE_CAPS[0] < x < S.RANGE_CAPS[1] for x in t), (st.name, t)


# ---------------------------------------------------------------- no probe is handed back
def test_range_restatement_decides_every_pair(oracle):
    for st in row_steps():
        if not st.n_after:
            continue
        sp = S.state_probes(oracle, st)
        exact = sp.scores[sp.pair_query]
        for cap in S.RANGE_CAPS + (0,):
            want = sp.range_expect(cap)
            groups = [(sel, "scan", S.EPS_SCAN) for sel in S.chunks(len(sp.taus)) if len(sel) >= 2]
            if st.n_after >= M.BATCH_ROWS:
                groups.append((np.arange(len(sp.taus)), "gemm", S.EPS_IMAGE))
            for sel, path, eps in groups:
                out = RB.device_path(exact[sel], exact[sel], eps, sp.taus[sel], cap, path=path)
                assert [o[3] for o in out] == [0] * len(sel), (st.name, cap, path)
                assert not S.differs([o[:3] for o in out], [want[i] for i in sel]), (st.name, cap, path)


def test_collects_stay_far_below_their_capacity(oracle):
    worst = 0
    for st in row_steps():
        if not st.n_after:
            continue
        sp = S.state_probes(oracle, st)
        for docs in (S.column(st).raw, sp.docs):
            for k, m in set(S.GROUPED) | {(c[0], c[1]) for c in S.CAPPED}:
                for e in sp.scores:
                    worst = max(worst, S.collect_count(e, docs, min(k, st.n_after), m, S.EPS_SCAN))
    print(f"largest candidate list {worst} of {GB.CAND_CAP}")
    assert worst <= min(GB.CAND_CAP, CV.GROUP_CAP) // 4


@pytest.mark.parametrize("name", [s.name for s in row_steps() if s.n_after])
def test_grouped_and_capped_restatements_decide_every_probe(oracle, name):
    st = steps()[M.STEP_NAMES.index(name)]
    sp = S.state_probes(oracle, st)
    inside = np.ones(st.n_after, bool)
    for k, m, sel in [(25, m, sel) for m in (1, 3) for sel in S.chunks(len(sp.queries))]:   # k = 25: the lowest U of GROUPED
        out = GB.device_path(sp.scores[sel], sp.scores[sel], sp.docs, k, m, S.EPS_SCAN)
        want = sp.grouped_expect(k, m)
        assert [s for _, s in out] == [0] * len(sel), (name, k, m)
        assert all(np.array_equal(out[j][0], want[i][0]) for j, i in enumerate(sel)), (name, k, m)
        for i in sel[::3]:
            assert S.collect_count(sp.scores[i], sp.docs, k, m, S.EPS_SCAN) == \
                len(CB.collect(sp.scores[i], sp.docs, k, m, S.EPS_SCAN, inside)["cand"]), (name, k, m, i)
    for need, m, diversify, _ in S.CAPPED:
        if diversify or need != 10:                               # need = 10: the lowest U; the pool is the same diversified
            continue
        want = sp.capped_expect(oracle, (need, m, False, need))
        for sel in S.chunks(len(sp.queries)):                     # the batched restatement: its own by-rule and status branches
            lex = [sp.lex[i] for i in sel]
            chunk = dict(e=sp.scores[sel], a=sp.scores[sel], docs=sp.docs, lex_rows=np.concatenate([l[0] for l in lex]),
                         lex_scores=np.concatenate([l[1] for l in lex]), lex_offsets=np.cumsum([0] + [len(l[0]) for l in lex]),
                         max_lex=np.array([l[2] for l in lex], np.float32), w_e=S.W_E, w_l=S.W_L, need=need, per_doc=m,
                         eps=S.EPS_SCAN)
            out = CB.chunk_path(chunk)
            assert [o["form"] for o in out] == [0] * len(sel), (name, need, m)
            assert all(CV.same(out[j]["res"], want[i]) for j, i in enumerate(sel)), (name, need, m)


def test_forms_follow_the_dispatch_rules():
    assert S.range_batch_forms("f32", 300, 8) == [8, 0, 0, 0] and S.range_batch_forms("f32", 300, 9) == [0, 0, 0, 9]
    assert S.range_batch_forms("f32", 4352, 36) == [0, 36, 0, 0] and S.range_batch_forms("f16", 4352, 4) == [0, 4, 0, 0]
    assert S.range_batch_forms("f16", 300, 4) == [0, 0, 0, 4] and S.range_batch_forms("f32", 0, 4) == [0, 0, 0, 0]
    assert S.range_batch_forms("f32", 5000, 1) == [0, 0, 0, 1] and S.range_batch_forms("f32", 5000, 8, list_path=True) == [0, 0, 0, 8]
    for n in (300, 4352, 6265):
        for m in (1, 2, 3):
            assert GB.chunk_width(n, M.DIM * 4, n, m) == 8 and GB.chunk_width(n, M.DIM * 4, (n + 2) // 3, m) == 8
    assert S.chunk_forms("f32", 4352, 4352, 3, 16) == [16, 0, 0, 0] and S.chunk_forms("f32", 300, 300, 1, 9) == [9, 0, 0, 0]
    assert S.chunk_forms("f16", 4352, 4352, 1, 8) == [0, 0, 0, 8] and S.chunk_forms("f32", 4352, 4352, 1, 1) == [0, 0, 0, 1]
