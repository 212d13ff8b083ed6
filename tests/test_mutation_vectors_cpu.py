"""The mutation plan (mutation_vectors.py) checked without a GPU: the plan holds every step class it claims (computed from
the plan's own row counts, capacities and delete lists, not declared), the mirror's delete is the header's renumbering
rule, every modelled fault of the copy bookkeeping costs at least one probe of every step it affects its oracle result,
the margin that makes a stale position visible holds over every row the plan ever stores, and the 8-bit band case loses
its winner under the stale statistic and keeps it under the right one.  Every test prints what it measured (pytest -s).

Measured (256-d, 18 765 pool rows, at most 6 265 in the index):
  largest cosine between two pool rows 0.385; smallest nominated self-score 0.99983 (binary16 image), 0.99832
  (8-bit copy); widest band 0.0169; collect floor of a self-query at k = 1: 0.875 - 0.0169 = 0.858; a stale
  position nominates at <= 0.385 (x 1.69, the largest ratio of two row scales, under fault F6a: 0.65)
  probes lost per affected step: F1 2..13, F2 2..78, F3 2..17, F4 8..102, F5 22..25, F6a 1..78, F6b 2..102, F7 2..14
  band case (768-d): filler's largest error norm 0.0092, X's and the decoys' 0.0530; full band 0.1035 keeps X at rank k,
  the band from the filler's maximum alone 0.0180 loses it (k = 1 and k = 10); rounded to binary16 the rows leave X at
  rank 31 (k = 1) and 40 (k = 10), so there is no binary16-typed form of the case; the other direction (200 filler rows,
  error norm 0.0088, appended behind the whole corpus): the band from the appended rows alone 0.0173, from a cleared
  statistic 0.0001, both lose X"""
import numpy as np
import pytest

import band_vectors as B
import mutation_vectors as M

T = M.TILE


def row_steps():
    return [s for s in M.plan()[0] if s.op in ("upload", "append", "delete")]


# ---------------------------------------------------------------- the plan covers what it claims
def _next_row_step(s):
    later = [t for t in row_steps() if t.index > s.index]
    return later[0] if later else None


def _prev(s):
    return M.plan()[0][s.index - 1] if s.index else None


CLASSES = {
    "01_upload_of_whole_tiles": lambda s: s.op == "upload" and s.n_before == 0 and s.n_after == 17 * T,
    "02_append_outgrows_capacity_leaves_partial_tile":
        lambda s: s.op == "append" and s.cap_after > s.cap_before and s.n_after % T != 0,
    "03_append_after_reserve_inside_capacity_and_partial_tile":
        lambda s: s.op == "append" and _prev(s).op == "reserve" and s.cap_after == s.cap_before and s.n_before % T != 0,
    "03b_append_rebuilt_incrementally_inside_partial_tile":
        lambda s: s.op == "append" and not s.fresh and s.n_before % T != 0 and s.n_after <= s.copy_cap_before,
    "04_append_completes_tile_exactly": lambda s: s.op == "append" and s.n_before % T != 0 and s.n_after % T == 0,
    "04b_append_of_one_row_opens_tile": lambda s: s.op == "append" and s.n_before % T == 0 and s.n_after == s.n_before + 1,
    "05_delete_first_dead_in_tile_interior_plus_scattered":
        lambda s: s.op == "delete" and 0 < s.first_changed % T < T - 1 and len(np.unique(s.dead // T)) > 2,
    "06_delete_first_dead_on_tile_edge": lambda s: s.op == "delete" and s.first_changed > 0 and s.first_changed % T == 0,
    "07_delete_first_dead_on_last_row_of_tile": lambda s: s.op == "delete" and s.first_changed % T == T - 1 and s.n_after > 0,
    "08_delete_one_whole_tile":
        lambda s: s.op == "delete" and np.array_equal(s.dead, np.arange(s.dead[0], s.dead[0] + T)) and s.dead[0] % T == 0,
    "09_delete_only_the_last_row": lambda s: s.op == "delete" and np.array_equal(s.dead, [s.n_before - 1]),
    "10_delete_only_rows_of_the_last_partial_tile":
        lambda s: s.op == "delete" and s.n_before % T != 0 and len(s.dead) > 1 and s.dead.min() >= s.n_before // T * T,
    "11_delete_run_across_three_tile_edges":
        lambda s: s.op == "delete" and np.array_equal(s.dead, np.arange(s.dead[0], s.dead[-1] + 1))
        and s.dead[-1] // T - s.dead[0] // T >= 3 and s.n_after > s.dead[0],
    "12_delete_with_duplicates": lambda s: s.op == "delete" and len(s.arg) > len(s.dead),
    "13_upload_of_fewer_rows_over_more": lambda s: s.op == "upload" and 0 < s.n_after < s.n_before,
    "14_delete_every_row_then_append":
        lambda s: s.op == "delete" and s.n_before > 0 and s.n_after == 0 and _next_row_step(s).op == "append"
        and _next_row_step(s).n_after >= M.BATCH_ROWS,
    "15_shrink_below_the_batched_minimum_then_grow_back":
        lambda s: s.op == "delete" and 0 < s.n_after < M.BATCH_ROWS <= s.n_before and _next_row_step(s).op == "append"
        and _next_row_step(s).n_after >= M.BATCH_ROWS,
    "16_toggle_on_before_upload":
        lambda s: s.op == "toggle" and s.arg == "on_before_upload" and s.n_after == 0 and s.index < row_steps()[0].index,
    "16_toggle_on_after_step_5":
        lambda s: s.op == "toggle" and s.arg == "on_after_step_5" and _prev(s).op == "delete"
        and sum(t.op == "delete" for t in M.plan()[0][:s.index]) == 1,
    "16_toggle_drop_and_reenable_between_two_deletes":
        lambda s: s.op == "toggle" and s.arg == "drop" and _prev(s).op == "delete"
        and M.plan()[0][s.index + 1].arg == "reenable" and M.plan()[0][s.index + 2].op == "delete",
    "16_toggle_widen_to_single_query": lambda s: s.op == "toggle" and s.arg == "widen_to_single_query" and s.n_after >= M.BATCH_ROWS,
}


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_plan_holds_step_class(cls):
    hits = [s.name for s in M.plan()[0] if CLASSES[cls](s)]
    print(f"{cls}: {hits}")
    assert hits, cls


def test_plan_stays_in_the_batched_range_except_where_named():
    steps, n_pool = M.plan()
    for s in steps:
        assert s.n_after <= 6400, s.name
        if s.n_after < M.BATCH_ROWS:
            assert s.name in ("toggle_on_before_upload", "delete_every_row", "delete_down_to_300"), s.name
    assert len(np.unique(np.concatenate([s.ids_after for s in steps]))) <= n_pool
    for s in steps:                                               # no row is stored twice
        assert len(np.unique(s.ids_after)) == s.n_after, s.name


def test_probe_sets_follow_the_rule():
    for s in M.plan()[0]:
        pos, note = M.probe_positions(s)
        assert len(pos) + M.N_ORDINARY <= M.MAX_QUERIES and len(np.unique(pos)) == len(pos), s.name
        assert ((0 <= pos) & (pos < max(s.n_after, 1))).all(), s.name
        for t in s.tiles:                                         # the first and the last changed row of every touched tile
            c = s.changed[s.changed // T == t]
            assert c[0] in pos and c[-1] in pos, (s.name, t)
        if s.n_after and not note:
            f = s.first_changed
            want = [s.n_after - 1] + ([p for p in (f - 1, f, f + 1, s.n_before - 1) if 0 <= p < s.n_after] if f is not None else [])
            if f is not None and len(s.changed):
                for e in range((f // T + 1) * T, int(s.changed[-1]) + 1, T):
                    want += [e - 1, e]
            assert set(want) <= set(pos.tolist()), (s.name, sorted(set(want) - set(pos.tolist())))
            same = s.n_after if f is None else min(f, s.n_after)
            assert int((pos < same).sum()) >= min(M.N_PREFIX, same), s.name
        print(f"{s.name}: {len(pos)} self-probes {note}")


# ---------------------------------------------------------------- the mirror's delete
def test_mirror_delete_is_the_headers_rule():
    """new_row = old_row - |{deleted d : d < old_row}|, duplicates ignored"""
    for s in M.plan()[0]:
        if s.op != "delete":
            continue
        dead = sorted(set(int(d) for d in s.arg))
        got = {int(i): p for p, i in enumerate(s.ids_after)}
        for old in range(s.n_before):
            pid = int(s.ids_before[old])
            if old in dead:
                assert pid not in got, (s.name, old)
            else:
                assert got[pid] == old - sum(d < old for d in dead), (s.name, old)
        assert s.n_after == s.n_before - len(dead)


# ---------------------------------------------------------------- the probes see a stale entry
@pytest.fixture(scope="module")
def model(oracle):
    return M.CopyModel(oracle)


@pytest.mark.parametrize("fault", M.FAULTS)
def test_probes_see_fault(oracle, model, fault):
    affected = 0
    for s in row_steps():
        if not M.fault_applies(s, fault):
            continue
        probes = M.step_probes(oracle, s)
        for kind in ("image", "q8"):
            lost, n_stale = model.lost(s, probes, kind, fault)
            if n_stale == 0:                                       # the fault leaves this copy of this step right
                continue
            affected += 1
            print(f"{fault} {s.name} {kind}: {n_stale} stale positions, {len(lost)} probe results differ {lost[:4]}")
            assert lost, (fault, s.name, kind, n_stale)
    assert affected, fault


def test_no_fault_no_loss(oracle, model):
    for s in row_steps():
        probes = M.step_probes(oracle, s)
        for kind in ("image", "q8"):
            lost, n_stale = model.lost(s, probes, kind, None)
            assert n_stale == 0 and not lost, (s.name, kind)


# ---------------------------------------------------------------- the probe margin
def test_probe_margin(oracle, model):
    pool = M.stored(oracle, "f32")
    n = len(pool)
    worst = 0.0
    for i0 in range(0, n, 1024):                                  # (rows are unit norm: dot products are cosines)
        g = pool[i0:i0 + 1024] @ pool[i0:].T
        g[np.arange(g.shape[0]), np.arange(g.shape[0])] = 0.0
        worst = max(worst, float(g.max()))
    q = np.stack([oracle.normalize(r) for r in pool])
    own_h = np.einsum("ij,ij->i", model.h.astype(np.float64), oracle.round_f16(q).astype(np.float64))
    own_q8 = np.einsum("ij,ij->i", model.codes.astype(np.float64), q.astype(np.float64)) * model.scale
    ratio = float(model.scale.max() / model.scale.min())
    floor = B.bin_floor(min(own_h.min(), own_q8.min())) - model.band
    print(f"largest off-diagonal cosine {worst:.4f}; smallest nominated self-score {own_h.min():.5f} (image) "
          f"{own_q8.min():.5f} (8-bit); band {model.band:.4f}; collect floor at k = 1 {floor:.4f}; scale ratio {ratio:.3f}")
    assert floor == 0.875 - model.band                            # every self-score nominates inside the top bin [0.875, 1)
    assert worst * ratio + model.band < floor                     # a stale position (even under a foreign scale) stays out


# ---------------------------------------------------------------- the band case bites
@pytest.mark.parametrize("k", M.BAND_KS)
def test_band_case_bites(oracle, k):
    base, tail, q, f = M.band_case(oracle, k)
    rows = np.concatenate([base, tail])
    x, D = f["x"], f["decoys"]
    assert len(base) == M.BATCH_ROWS and x == len(base) and len(D) == B.N_DECOYS
    e = oracle.scan(rows, q)
    order = np.lexsort((np.arange(len(e)), -e.astype(np.float64)))
    assert order[k - 1] == x and set(order[:k - 1]) == set(f["champions"].tolist())
    deq, delta, scale = B.q8_model(rows)
    nominated = deq @ q.astype(np.float64)
    assert (nominated[D] > nominated[x]).all() and (e[D] < e[x]).all()
    full = M.q8_band(f["dim"], delta.max(), float(scale.max()), f["query_norm"])
    stale = M.q8_band(f["dim"], delta[:len(base)].max(), float(scale[:len(base)].max()), f["query_norm"])
    print(f"k={k}: filler's largest error norm {delta[:len(base)].max():.4f}, X's and the decoys' {delta[len(base):].max():.4f}; "
          f"full band {full:.4f}, band from the filler's maximum {stale:.4f}")
    assert delta[:len(base)].max() < 0.0095 and delta[x] > 0.05
    for bins in (True, False):
        assert B.select(nominated, e, k, full, bins)[k - 1] == x
        assert x not in B.select(nominated, e, k, stale, bins)
    # deleting the decoys afterwards leaves X at rank k: the statistic may stay large
    kept = np.delete(np.arange(len(rows)), D)
    assert np.array_equal(kept[np.lexsort((kept, -e[kept].astype(np.float64)))[:k]], order[:k])
    # binary16 rows: the 0.49-of-a-step construction does not survive the rounding, X leaves rank k
    e16 = oracle.scan(oracle.round_f16(rows), q)
    rank16 = int(np.flatnonzero(np.lexsort((np.arange(len(e16)), -e16.astype(np.float64))) == x)[0]) + 1
    print(f"k={k}: rank of X among binary16-rounded rows {rank16}: no binary16-typed form of the case")
    assert rank16 != k


@pytest.mark.parametrize("k", M.BAND_KS)
def test_band_case_reversed_bites(oracle, k):
    """small rows appended behind X and its decoys: the statistic of the appended rows alone (a partial build that
    starts from zero) loses X, the maximum over all rows keeps it"""
    rows, extra, q, f = M.band_case_reversed(oracle, k)
    both = np.concatenate([rows, extra])
    x = f["x"]
    e = oracle.scan(both, q)
    assert np.lexsort((np.arange(len(e)), -e.astype(np.float64)))[k - 1] == x
    deq, delta, scale = B.q8_model(both)
    nominated = deq @ q.astype(np.float64)
    full = M.q8_band(f["dim"], delta.max(), float(scale.max()), f["query_norm"])
    stale = M.q8_band(f["dim"], delta[len(rows):].max(), float(scale[len(rows):].max()), f["query_norm"])
    zero = M.q8_band(f["dim"], 0.0, 0.0, f["query_norm"])
    print(f"k={k}: appended rows' largest error norm {delta[len(rows):].max():.4f}, stored rows' {delta[:len(rows)].max():.4f}; "
          f"full band {full:.4f}, from the appended rows alone {stale:.4f}, from a zeroed statistic {zero:.6f}")
    assert delta[len(rows):].max() < 0.0095 and delta[x] > 0.05
    for bins in (True, False):
        assert B.select(nominated, e, k, full, bins)[k - 1] == x
        assert x not in B.select(nominated, e, k, stale, bins) and x not in B.select(nominated, e, k, zero, bins)
    # ... and so does the last row's delete afterwards (a partial build of no rows at all)
    assert np.lexsort((np.arange(len(e) - 1), -e[:-1].astype(np.float64)))[k - 1] == x


# ---------------------------------------------------------------- the wide-row case
def test_wide_case_moves_more_than_two_chunks():
    dead, keep, positions, seams = M.wide_case()
    assert M.WIDE_CHUNK == 16384 and dead[0] == 100 and set(range(100, 105)) <= set(dead.tolist())
    assert len(keep) - 100 > 2 * M.WIDE_CHUNK and len(seams) >= 2 and seams[0] == 100 + 16384
    assert {seams[0] - 1, seams[0]} <= set(dead.tolist())         # the deleted run lies across the first seam
    assert len(dead) >= M.WIDE_ROWS // 100 + 5 and len(positions) >= 1000
    for s in seams:
        assert set(range(s - 2, s + 3)) <= set(positions.tolist()) and keep[s] != s
    print(f"{len(dead)} rows deleted, {len(keep)} left, chunk seams at {seams}, {len(positions)} positions compared")
