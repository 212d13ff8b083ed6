"""The designed score arrays of select_vectors.py checked without a GPU, for every corpus test_gpu_select.py uses:
  1  every column comes back through oracle.scan under its one-hot query bit for bit (-0.0 as +0.0, the one exception)
  2  every case holds what its class promises: bin populations at the edge it names, the bin (and digit-2 bin) of each
     k it asks, the mode at 64 / 65 scores, the candidate count, the rows of the n % 4 tail
  3  no score of a count-asserted case lies within 32 ulps of the model's key_lo, in any pipeline or mode: the count
     cannot hinge on how the library rounds the corpus' norm (that moves the band by far less than one ulp)
  4  mutation proof: the select run in Python with its finders' structure (select_vectors.finder) agrees with the model
     on every case -- and with one defect built in, the candidate count or the top-k of named cases changes
  5  every case of classes A-E and G is count-asserted, F alone is results-only, and class E reaches each branch of
     sort_emit_rows: the GPU test takes its cases from the same list and cannot quietly skip one"""
import numpy as np
import pytest

import select_vectors as S

COUNTED = "ABCDEG"
MODES = dict(S.PIPELINES, max64=S.MODE64)


def col_of(name, case):
    return S.corpus(name)[0][:, case["col"]]


def every_case(classes=COUNTED, f16=True):
    """(corpus, case) of the single-query corpora; f16=False: without the binary16 twins of A and G (same case names)"""
    return [(name, c) for name, c in S.all_cases() if c["cls"] in classes and (f16 or not name.endswith("_f16"))]


@pytest.mark.parametrize("name", list(S.SINGLE) + ["batch"])
def test_columns_come_back_through_the_oracle(oracle, name):
    rows, cases, _ = S.corpus(name)
    for c in cases:
        col = rows[:, c["col"]]
        e = oracle.scan(rows, S.one_hot(rows.shape[1], c["col"]))
        want = np.where(col == 0.0, np.float32(0.0), col)    # -0.0 -> +0.0
        assert np.array_equal(e.view(np.uint32), want.view(np.uint32)), c["name"]
        if c["cls"] != "F":
            assert not (np.signbit(col) & (col == 0.0)).any()


def test_sampled_columns_come_back_through_the_oracle(oracle):
    rows, cases = S.sampled_corpus()
    assert len(rows) > 2 * S.SAMPLE and rows.shape[1] % 128 == 0
    assert np.array_equal(rows.astype(np.float16).astype(np.float32).view(np.uint32), rows.view(np.uint32))
    for c in cases:
        col = rows[:, c["col"]]
        assert np.array_equal(oracle.scan(rows, S.one_hot(rows.shape[1], c["col"])).view(np.uint32), col.view(np.uint32))
        top = S.topk_rows(col, S.K_SAMPLED)
        assert set(top) <= set(c["rows"])
        assert (top < S.SAMPLE).all() if c["where"] == "inside" else (top >= S.SAMPLE).all()
        assert (col[top] < 0).all() == (c["sign"] == "neg")
        if c["where"] == "behind":                           # the sample's floor comes from its decoys, bins below the top-k
            floor = np.sort(col[:S.SAMPLE])[::-1][S.K_SAMPLED - 1]
            assert floor < col[top].min() and (S.score_key(floor)[0] >> 21) < (S.score_key(col[top].min())[0] >> 21) - 1


def test_binary16_corpora_lie_on_the_grid():
    for name in ("A_pos_f16", "A_neg_f16", "batch"):
        rows = S.corpus(name)[0]
        assert np.array_equal(rows.astype(np.float16).astype(np.float32).view(np.uint32), rows.view(np.uint32)), name
        assert np.abs(rows).max() < 65504.0


# ---------------------------------------------------------------- 2: the promises
def test_class_A_edges_sit_where_the_finders_change_hands():
    """b | b+1 against the finders' layout: 256 threads own 8 bins each (waves of 512), 1024 threads 2 each (waves of 128)"""
    kinds = {b: ((b + 1) % 512 == 0, (b + 1) % 8 == 0, (b + 1) % 128 == 0, (b + 1) % 2 == 0) for b in S.A_EDGES}
    assert kinds[1535] == (True, True, True, True)
    assert kinds[1663] == (False, True, True, True)
    assert kinds[1543] == (False, True, False, True)
    assert kinds[1537] == (False, False, False, True)
    assert kinds[1536] == (False, False, False, False) and not kinds[1539][1]     # inside one thread of the 256-thread finder
    assert kinds[1531][0] is False and 1531 < 1532 and 1527 < 1532               # the production range: under 1.0
    assert float(S.vals(S.mk(1536, 0, 0))[0]) == 2.0 and float(S.vals(S.mk(1664, 0, 0))[0]) == 2.0 ** 33
    assert float(S.vals(S.mk(511, 2047, 1023))[0]) == -2.0                        # 511 | 512 is -2.0
    names = {c["name"] for _, c in S.all_cases() if c["cls"] == "A"}
    assert {f"A_{s}_{b}" for s in ("pos", "neg") for b in S.A_EDGES} <= names


@pytest.mark.parametrize("name,case", every_case("A"), ids=lambda v: v["name"] if isinstance(v, dict) else v)
def test_class_A_populations_and_ranks(name, case):
    rows, _, two_eps = S.corpus(name)
    col = rows[:, case["col"]]
    keys = S.score_key(col)
    hi, a, m, c = case["promise"]["pop"]
    h1 = np.bincount(keys >> 21, minlength=2048)
    assert (h1[hi], h1[hi - 1], h1[hi - 2]) == (a, m, c) and h1[hi - 3] == 0
    lead = int(h1[hi + 1:].sum())
    assert lead == (S.A_LEAD if hi < 1024 else 0) and case["ks"] == [lead + a, lead + a + 1, lead + a + m, lead + a + m + 1]
    assert (col[case["rows"]] < 0).sum() == (a + m + c if hi < 1024 else 0)
    b2 = (keys[case["rows"]] >> 10) & 2047
    assert b2.min() >= 600 and b2.max() < 1400               # away from the floors: the band (below) cannot reach a neighbour
    for k in case["ks"]:
        for pl, dm in MODES.values():
            mo = S.model(col, k, two_eps, pl, dm)
            assert mo["bin1"] == case["promise"]["bin1"][k]
            assert mo["key_lo"] >> 21 in (mo["bin1"], mo["bin1"] - 1) and mo["count"] <= a + m + c + lead
            if mo["mode"] == S.DIRECT:
                assert mo["count"] == mo["n_ge"] == int(h1[mo["bin1"]:].sum())


@pytest.mark.parametrize("name,case", every_case("B"), ids=lambda v: v["name"] if isinstance(v, dict) else v)
def test_class_B_floors_and_counts(name, case):
    rows, _, two_eps = S.corpus(name)
    col = rows[:, case["col"]]
    band_ulps = float(two_eps) / 2.0 ** -23                  # the designed scores lie in [1, 2): one ulp is 2^-23
    assert band_ulps < 512 - S.MARGIN_ULPS, (name, band_ulps)
    for k, want in zip(case["ks"], (3, 7, 7, 10)):
        mo = S.model(col, k, two_eps, "split")
        assert (mo["bin1"], mo["bin2"]) == case["promise"]["floor"][k] and mo["count"] == want
        assert mo == S.model(col, k, two_eps, "fused", 0)
        top_case = case["promise"]["floor"][k][1] == 0
        assert S.model(col, k, two_eps, "fused")["count"] == (3 if top_case else 10)


def test_class_C_switches_between_64_and_65():
    rows, cases, two_eps = S.corpus("C")
    for c in cases:
        col = rows[:, c["col"]]
        k = c["ks"][0]
        mo = S.model(col, k, two_eps, *S.MODE64)
        assert mo["n_ge"] == c["promise"]["n_ge"] and mo["mode"] == c["promise"]["mode64"]
        direct, refine = S.model(col, k, two_eps, "fused", 4096), S.model(col, k, two_eps, "fused", 0)
        assert direct["mode"] == S.DIRECT and refine["mode"] == S.REFINE
        assert direct["count"] == mo["n_ge"] and refine["count"] == 50 and direct["count"] - refine["count"] == c["promise"]["between"] >= 14
        assert mo["count"] == (direct if mo["mode"] == S.DIRECT else refine)["count"]


def test_class_D_crosses_zero():
    rows, cases, two_eps = S.corpus("D")
    by = {c["name"]: c for c in cases}
    for c in cases:
        col = rows[:, c["col"]]
        for k in c["ks"]:
            for pl, dm in MODES.values():
                mo = S.model(col, k, two_eps, pl, dm)
                assert mo["bin1"] == c["promise"].get("bin1", {}).get(k, mo["bin1"])
                assert mo["count"] == c["promise"].get("count", {}).get(k, mo["count"]), (c["name"], k, pl, dm)
    zero = rows[:, by["D_zero"]["col"]]
    assert (zero == 0).sum() == 20 and ((zero > 0) & (zero < 2.0 ** -126)).sum() == 10 and zero.max() > 0.75
    mo = S.model(zero, 16, two_eps, "split")
    assert mo["kth"] == 0x80000000 and mo["key_lo"] < 0x80000000 == S.mk(1024, 0, 0)     # +0.0: the floor lies under zero
    sub = rows[:, by["D_neg_subnormal"]["col"]]
    assert ((sub < 0) & (sub > -2.0 ** -126)).sum() == 10
    tiny = rows[:, by["D_tiny"]["col"]]
    assert tiny.max() < 2.0 ** -20 < float(two_eps) and (tiny > 0).sum() == 600
    neg = rows[:, by["D_negatives"]["col"]]
    assert (neg < 0).all()
    mo = S.model(neg, 1, two_eps, "split")
    assert S.key_score(mo["key_lo"])[0] < S.key_score(mo["kth"])[0] < 0


def emit_branch(n_raw, k):
    """the branch of sort_emit_rows (ordered results) that n_raw candidates and k wanted rows take"""
    return "overflow" if n_raw > S.CAP else "rank" if n_raw <= 1024 else "select" if k <= 1024 else "bitonic"


def test_class_E_sizes_reach_every_branch_of_the_emit():
    rows, cases, two_eps = S.corpus("E")
    assert float(np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1).max())) == pytest.approx(S.E_ANCHOR[1], rel=1e-4)
    assert {c["promise"]["C"] for c in cases} == set(S.E_SIZES) and len(cases) == 2 * len(S.E_SIZES)
    seen = set()
    for c in cases:
        col, C = rows[:, c["col"]], c["promise"]["C"]
        assert c["ks"] == [1, 1024, 1025, min(C, S.CAP)]
        keys = S.score_key(col[c["rows"]])
        assert len(keys) == C and S.score_key(np.delete(col, c["rows"])).max() < keys.min() - (8 << 21)
        if c["promise"]["variant"] == "low":                 # one digit-2 bin; the low words all used, evenly
            assert len(np.unique(keys >> 10)) == 1 and np.ptp(np.bincount(keys & 1023, minlength=1024)) <= 1
        else:                                                # distinct, on both sides of bit 21 and of bit 10
            assert len(np.unique(keys)) == C and len(np.unique(keys >> 21)) == 2 and len(np.unique((keys >> 10) & 2047)) > 300
        assert S.model(col, min(C, S.CAP), two_eps, "split")["count"] == C
        for k in c["ks"]:
            for pl, dm in S.PIPELINES.values():
                mo = S.model(col, k, two_eps, pl, dm)
                seen.add(emit_branch(S.tail_report(mo, col, k, pl, dm)[0], k))
    assert seen == {"overflow", "rank", "select", "bitonic"}


def test_class_G_uses_the_last_rows():
    for name in ("G", "A_pos_f16", "A_neg_f16", "batch"):
        rows, cases, two_eps = S.corpus(name)
        n = len(rows)
        assert n % 4 == (0 if name == "batch" else 3)
        for c in [c for c in cases if c["cls"] == "G"]:
            col = rows[:, c["col"]]
            assert list(S.topk_rows(col, 4)) == c["promise"]["top"] and set(c["promise"]["top"][:3]) == {n - 1, n - 2, n - 3}
            for k in c["ks"]:
                assert S.model(col, k, two_eps)["bin1"] == c["promise"]["bin1"][k]


def test_class_F_holds_its_special_values():
    col = col_of("F_negzero", S.corpus("F_negzero")[1][0])
    assert (np.signbit(col) & (col == 0)).sum() == 10 and (~np.signbit(col) & (col == 0)).sum() == 10
    c = S.corpus("F_nan")[1][0]
    col = col_of("F_nan", c)
    assert max(c["ks"]) > (~np.isnan(col)).sum() == 99 in c["ks"]
    c = S.corpus("F_inf")[1][0]
    col = col_of("F_inf", c)
    order = S.topk_rows(col, 60)
    assert np.isposinf(col[order[1]]) and np.isneginf(col[order[52]]) and np.isneginf(col[order[56]]) and np.isnan(col[order[57]])
    assert {2, 53, 57} <= set(c["ks"])
    two_eps = S.corpus("F_inf")[2]
    assert S.model(col, 53, two_eps, "split")["key_lo"] == 0                      # a k-th score of -inf: everything is collected


# ---------------------------------------------------------------- 3: the margin
def test_no_score_near_a_floor():
    worst = 1 << 40
    for name, c in every_case():
        rows, _, two_eps = S.corpus(name)
        col = rows[:, c["col"]]
        for k in c["ks"]:
            for mode, (pl, dm) in MODES.items():
                g = S.margin(col, k, two_eps, pl, dm)
                assert g >= S.MARGIN_ULPS, (c["name"], k, mode, g)
                worst = min(worst, g)
    print(f"closest score to a floor: {worst} ulps")


# ---------------------------------------------------------------- 4: the mutation proof
def no_sign_flip(x):
    """the key map without the inversion of the negative half"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where((b & 0x7FFFFFFF) > 0x7F800000, np.uint32(0), b ^ np.uint32(0x80000000)).astype(np.uint32)


def affected(threads, pipelines=("fused", "split"), direct_max=0, names=None, **defect):
    """the cases whose candidate count or top-k changes under the defect, as {case name: [k, ...]}"""
    out = {}
    for name, c in every_case(f16=False):
        if names is not None and c["name"] not in names:
            continue
        rows, _, two_eps = S.corpus(name)
        col = rows[:, c["col"]]
        for k in c["ks"]:
            for pl in pipelines:
                want = S.model(col, k, two_eps, pl, direct_max)
                n, cand = S.select_with(col, k, two_eps, pl, direct_max, threads=threads, **defect)
                if n != want["count"] or not np.array_equal(S.topk_rows(col, k, cand), S.topk_rows(col, k)):
                    out.setdefault(c["name"], []).append(k)
    return out


@pytest.mark.parametrize("threads", [(256, 256), (256, 1024), (1024, 1024)])
def test_the_python_finders_agree_with_the_model(threads):
    """(256, 256): the split pipeline; (256, 1024): the fused tail's REFINE mode; (1024, 1024): the fused batch select"""
    for dm in (0, 64, S.DEFAULT_DIRECT_MAX, 4096):
        assert affected(threads, direct_max=dm) == {}


A_FEW = {"A_pos_1535", "A_pos_1663", "A_pos_1543", "A_pos_1537", "A_pos_1536", "A_pos_1531", "A_neg_1535", "A_neg_1663",
         "A_neg_1537", "A_neg_1531", "B_pos_7", "B_pos_127", "B_pos_511", "B_pos_1023", "B_pos_2047", "B_neg_511", "B_neg_127",
         "C_64", "C_65", "D_negatives", "D_zero", "G_neg"}


@pytest.mark.parametrize("threads,wave,caught", [
    (256, 3, {"A_pos_1535": [6, 11, 12]}),                   # the scores of bin 1536 and above, seen from bin 1535
    (256, 1, {"A_neg_1535": [6, 11, 12]}),                   # ... of bin 512, seen from bin 511
    (256, 2, {"A_neg_1535": [5, 6, 11, 12], "A_neg_1531": [5, 6, 11, 12]}),      # the positive scores in front of a negative k-th
    (256, 1, {"B_pos_511": [3, 7]}),                         # digit 2: bin 512 seen from bin 511
    (1024, 12, {"A_pos_1535": [6, 11, 12]}),
    (1024, 13, {"A_pos_1663": [6, 11, 12]}),
    (1024, 4, {"A_neg_1535": [6, 11, 12]}),
    (1024, 3, {"A_neg_1663": [6, 11, 12]}),
    (1024, 1, {"B_pos_127": [3, 7], "B_neg_127": [3, 7]}),
    (1024, 8, {"B_pos_1023": [3, 7]}),
])
def test_a_dropped_wave_total_is_caught(threads, wave, caught):
    got = affected((threads, threads), names=A_FEW, drop_wave=wave)
    for name, ks in caught.items():
        assert got.get(name) and set(ks) <= set(got[name]), (name, got.get(name))


@pytest.mark.parametrize("threads,defect,caught", [
    (256, "skip_top", {"A_pos_1535": 6, "A_pos_1543": 6, "A_neg_1535": 6, "B_pos_7": 4, "B_pos_511": 4}),
    (256, "skip_bottom", {"A_pos_1535": 5, "A_pos_1543": 5, "A_neg_1535": 5, "B_pos_7": 3, "B_pos_511": 3}),
    (1024, "skip_top", {"A_pos_1535": 6, "A_pos_1537": 6, "A_pos_1663": 6, "B_pos_127": 4}),
    (1024, "skip_bottom", {"A_pos_1535": 5, "A_pos_1537": 5, "A_pos_1663": 5, "B_pos_1023": 3}),
])
def test_a_thread_off_by_one_at_its_top_or_bottom_bin_is_caught(threads, defect, caught):
    got = affected((threads, threads), names=A_FEW, defect=defect)
    for name, k in caught.items():
        assert k in got.get(name, []), (name, got.get(name))


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("defect", ["lt", "le"])
def test_a_swapped_comparison_at_a_bins_last_rank_is_caught(threads, defect):
    got = affected((threads, threads), names=A_FEW, defect=defect)
    for name in ("A_pos_1531", "A_pos_1535", "A_neg_1531", "B_pos_511"):    # k = a (a + m): the last rank of a bin
        assert got.get(name), name
    assert 5 in got["A_pos_1531"] and 11 in got["A_pos_1531"]


def test_an_ignored_sign_flip_is_caught():
    got = affected((256, 256), names=A_FEW, key_of=no_sign_flip)
    for name in ("A_neg_1535", "A_neg_1531", "A_neg_1663", "D_negatives", "G_neg", "B_neg_511"):
        assert got.get(name), name
    assert not [n for n in got if n.startswith(("A_pos", "B_pos", "C_"))]


def test_the_wrong_mode_at_direct_max_is_caught():
    got = affected((256, 1024), pipelines=("fused",), direct_max=64, names=A_FEW, mode_le=False)
    assert got == {"C_64": [50]}


# ---------------------------------------------------------------- 5: nothing is left out
def test_every_case_but_class_F_is_count_asserted():
    classes = {}
    for name, c in S.all_cases():
        classes.setdefault(c["cls"], []).append(c)
        assert c["counted"] == (c["cls"] != "F"), c["name"]
        assert c["ks"] and min(c["ks"]) >= 1 and len(S.corpus(name)[0]) == S.N_SINGLE and S.corpus(name)[0].shape[1] == S.DIM_SINGLE
    assert set(classes) == set("ABCDEFG")
    assert len(classes["A"]) == 2 * len(S.A_EDGES) + 14 and len(classes["B"]) == 2 * len(S.B_EDGES)
    assert len(classes["E"]) == 12 and len(classes["G"]) == 4 and len(classes["F"]) == 3
    # what the GPU test asserts per counted case: the count itself up to 4096, one retry beyond
    over = [(c["name"], k, mode) for name, c in every_case() for k in c["ks"] for mode, (pl, dm) in S.PIPELINES.items()
            if S.tail_report(S.model(col_of(name, c), k, S.corpus(name)[2], pl, dm), col_of(name, c), k, pl, dm)[1]]
    assert {n for n, _, _ in over} >= {"E_low_4097", "E_wide_4097"} and all(n.startswith("E_") for n, _, _ in over)
    rows, cases, _ = S.corpus("batch")
    assert rows.shape == (S.N_BATCH, S.DIM_BATCH) and len(cases) == 16 and {tuple(c["ks"]) for c in cases if c["cls"] == "A"} == {(5, 6, 11, 12)}


def test_the_batch_corpora_stay_inside_the_batched_finish():
    """a query of the batch is handed back when the band under its k-th nominated score holds more than 2048 rows: the
    GPU test asserts zero hand-backs, so no designed column may come near that with the widest band it meets (binary16
    nomination of f32 rows)"""
    rows, cases, _ = S.corpus("batch")
    band = S.nomination_two_eps_of(rows)
    worst = 0
    for c in cases:
        col = rows[:, c["col"]]
        for k in (1, 3, 5, 6, 11, 12):
            kth = np.sort(col)[::-1][k - 1]
            worst = max(worst, int((col >= kth - 1.01 * band).sum()))
    assert worst <= 64, worst
    rows, cases = S.sampled_corpus()
    band = S.nomination_two_eps_of(rows)
    for c in cases:
        col = rows[:, c["col"]]
        kth = np.sort(col)[::-1][S.K_SAMPLED - 1]
        assert int((col >= kth - 1.01 * band).sum()) <= 64
        floor = np.sort(col[:S.SAMPLE])[::-1][S.K_SAMPLED - 1]                 # the sample's own k-th: the floor of the rest
        assert int((col >= floor - 0.01 * abs(floor) - 2.0 * band).sum()) <= 64
