"""Every nominating kernel held to its band at every row position and every query slot, with the ladder corpora of
ladder_vectors.py (test_ladder_vectors_cpu.py proves that a checked row nominated 5 eps low, or read without one 16-byte
unit, is lost).  In every test: the oracle's rows in the oracle's order, score bits equal, no tolerance; the profile
counters show that the intended path ran; and where the pipeline reports it, the candidate count of each query is exactly
the ladder's size W -- a row nominated too HIGH would show there.

What n_candidates counts (index.hip: run_search, filtered_query, note_search): the single-query pipelines -- the plain
scans, the scans over the image and the 8-bit copy, the masked scan, the device-resident begin / end pair -- report the
rows at or above (floor of the k-th nominated score's quarter-binade bin) - band; all of these corpora take the tail's
one-pass mode (64 scores in the k-th score's bin, far below its limit), which collects from exactly that floor.  The batched pipeline (the matrix-core batch,
the shared scans, coalesced groups) reports 0 by design; asserted as such.

Checked rows cover every residue of the row number modulo 256 once in the first 256 rows and once behind row 32 768
(131 072 for the packed scans and the shared scans) -- a later trip of every wave's grid-stride loop at the launch shapes
used here --, every row of the ragged last tile (n mod 8, mod 64, mod 256 all non-zero), row 0 and row n - 1.  Trips:
  scan_fixed_kernel 768-d f32, default plan (8-row groups, one workgroup per CU)    8 192 rows per sweep
  every other plain scan with RLR_SCAN_VARIANT = 0x100100 (16-row groups, one per CU) 16 384
  scan_packed_kernel (its launch ignores the workgroup field: 8 per CU)              131 072 -> a 135 037-row corpus
  scan_image_kernel (32-row slots, one workgroup per CU)                            32 768
  the 8-bit scans with RLR_Q8_VARIANT = 0x100 in a child (one per CU)                32 768 (128-d: 65 536)
  scan_multi_kernel / scan_multi_h_kernel (32-row groups, four per CU)              131 072 -> 135 037 rows at 256-d
  masked scans: dense shape 8 192 (a set of checked rows from row 20 480 on); sparse and generic shape 65 536 (first
  trip only at 36 923 rows)
The shards and the masked scans have layouts of their own (ladder_vectors.layout): a ladder per shard, and checked rows that
are the only allowed row of their unit.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ladder_vectors as L
from conftest import bits
from test_gpu_coalesce import run_threads

pytestmark = pytest.mark.gpu

ONE_PER_CU_16 = "0x100100"     # RLR_SCAN_VARIANT: one workgroup per CU, 16-row groups
ELEM_BYTES = {"f32": 4, "f16": 2}


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (exact scores [G, n], top-k rows [G, k], their scores [G, k]) of a corpus by the oracle's scan, computed once"""
    from oracle import oracle as O
    rows, qs, f = L.corpus(name)
    e = np.stack([O.scan(rows, q, 8) for q in qs])
    order = np.stack([np.lexsort((np.arange(e.shape[1]), -e[g].astype(np.float64)))[:f["k"]] for g in range(len(qs))])
    wr = order.astype(np.uint64)
    wc = np.take_along_axis(e, order, axis=1)
    for g in range(len(qs)):                                 # the case is the one the CPU test proved
        assert set(order[g]) == set(f["checked"][g]), (name, g)
    for a in (e, wr, wc):
        a.setflags(write=False)
    return e, wr, wc


def assert_exact(name, g, r, c, ctx):
    _, wr, wc = reference(name)
    assert np.array_equal(r, wr[g]), f"{ctx} query {g}: rows differ: got {r[:6]} want {wr[g][:6]}; " \
                                     f"missing {sorted(set(wr[g].tolist()) - set(r.tolist()))[:8]}"
    assert np.array_equal(bits(c), bits(wc[g])), f"{ctx} query {g}: scores differ"


def make_index(rlr, name, dtype=None):
    rows, qs, f = L.corpus(name)
    dtype = dtype or ("f16" if f["kind"] == "f16" else "f32")
    ix = rlr.GpuIndex(f["dim"], dtype)
    ix.upload(rows)                                          # as built: normalize_on_device = 0
    return ix


def single_queries(ix, name, scan_elem_bytes, ctx, search=None):
    """every ladder query alone through a single-query pipeline (`search(g)` -> rows, scores of query g; by default
    search_topk): exact, one scan launch over `scan_elem_bytes` per element, no batch, no retry, no fallback, exactly W
    candidates.  The one place where this file asserts what a single-query path must report."""
    rows, qs, f = L.corpus(name)
    search = search or (lambda g: tuple(a[0] for a in ix.search_topk(qs[g], f["k"])))
    ix.profile_enable(True)
    for g in range(len(qs)):
        ix.profile_read(reset=True)
        r, c = search(g)
        p = ix.profile_read()
        assert_exact(name, g, r, c, ctx)
        assert p.n_batches == 0 and p.n_scan_launches == 1 and p.n_f16_range_fallbacks == 0 and p.n_retries == 0, (ctx, g, p)
        assert p.scan_bytes == len(rows) * f["dim"] * scan_elem_bytes, (ctx, g, p)
        assert p.n_candidates == f["W"], f"{ctx} query {g}: {p.n_candidates} candidates, the ladder has {f['W']}"


# ---------------------------------------------------------------- single-query scans
@pytest.mark.parametrize("name,variant", [
    ("scan_f32_768", None),            # scan_fixed_kernel<3>, query in the launch arguments, 4 rows in flight
    ("scan_f32_256", ONE_PER_CU_16),   # scan_fixed_kernel<1>
    ("scan_f32_1024", ONE_PER_CU_16),  # scan_fixed_kernel<4>
    ("scan_f32_1536", ONE_PER_CU_16),  # scan_fixed_kernel<6>, two rows in flight
    ("scan_f16_1024", ONE_PER_CU_16),  # scan_fixed_kernel<2, F16>
    ("scan_f16_1536", ONE_PER_CU_16),  # scan_fixed_kernel<3, F16>, two rows in flight
    ("packed_f32_128", None),          # scan_packed_kernel<32, f32>
    ("packed_f16_256", None),          # scan_packed_kernel<32, F16>
    ("generic_f32_200", ONE_PER_CU_16),  # scan_generic_kernel
    ("generic_f16_72", ONE_PER_CU_16),   # scan_generic_kernel, F16
])
def test_plain_scans(rlr, monkeypatch, name, variant):
    monkeypatch.setenv("RLR_BATCH_MIN", "100000")            # (both read when the index is created)
    if variant:
        monkeypatch.setenv("RLR_SCAN_VARIANT", variant)
    else:
        monkeypatch.delenv("RLR_SCAN_VARIANT", raising=False)
    ix = make_index(rlr, name)
    try:
        single_queries(ix, name, ELEM_BYTES[L.corpus(name)[2]["kind"]], name)
    finally:
        ix.close()


def test_device_resident_results_report_the_ladder(rlr, monkeypatch):
    """rlr_search_topk_device_begin / _end: the same pipelines on the caller's stream, the k packed results left on the
    device ((score key << 32) | (2^32 - 1 - row), common.h: pack_result); the count goes through note_search in _end"""
    import torch
    monkeypatch.setenv("RLR_BATCH_MIN", "100000")
    monkeypatch.delenv("RLR_SCAN_VARIANT", raising=False)
    name = "scan_f32_768"
    rows, qs, f = L.corpus(name)
    ix = make_index(rlr, name)
    try:
        out = torch.zeros((1, f["k"]), dtype=torch.int64, device="cuda")

        def search(g):
            t = ix.search_topk_device_begin(qs[g], f["k"], out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert t, "the call ran synchronously: not the path under test"
            assert ix.search_topk_device_end(t) == 0
            torch.cuda.synchronize()
            packed = out.cpu().numpy().view(np.uint64)[0]
            key = (packed >> np.uint64(32)).astype(np.uint32)
            assert (key & np.uint32(0x80000000)).all()        # positive scores: the key is the bit pattern with the top bit set
            return np.uint64(0xFFFFFFFF) - (packed & np.uint64(0xFFFFFFFF)), (key & np.uint32(0x7FFFFFFF)).view(np.float32)

        single_queries(ix, name, 4, "device-resident results", search)
    finally:
        ix.close()


# ---------------------------------------------------------------- nomination copies
def test_scan_over_the_image(rlr, monkeypatch):
    """scan_image_kernel at 768-d: 32-row slots of 256-row tiles, one workgroup per CU -- rows from 32 768 on are a second trip"""
    monkeypatch.setenv("RLR_BATCH_MIN", "100000")
    ix = make_index(rlr, "image_768")
    try:
        ix.enable_batch_image(True, single_query=True)
        single_queries(ix, "image_768", 2, "image_768")
    finally:
        ix.close()


Q8_CHILD = r"""
import importlib, sys
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import ladder_vectors as L
import test_gpu_positions as T
rlr = importlib.import_module('rust-local-rag_amd')
name = sys.argv[1]
ix = T.make_index(rlr, name)
ix.enable_batch_image(False, q8=True)
T.single_queries(ix, name, 1, name)
ix.close()
print('ladder ok', len(L.corpus(name)[1]))
"""


@pytest.mark.parametrize("name", ["q8_768", "q8_128", "q8_400"])   # q8_scan_packed_kernel<4,3,2>, <8,1,8>; q8_scan_kernel<8,1>
def test_scan_over_the_8_bit_copy(name):
    """RLR_Q8_VARIANT is read once per process: a child, with one workgroup per CU, so that the later tile is a later trip"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RLR_Q8_VARIANT="0x100", RLR_BATCH_MIN="100000")
    out = subprocess.run([sys.executable, "-c", Q8_CHILD, name], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ladder ok" in out.stdout, (name, out.stdout[-1000:], out.stderr[-3000:])


# ---------------------------------------------------------------- shared scans
@pytest.mark.parametrize("name", ["scan_f32_768", "long_f32_256"])
def test_shared_f32_scan_every_slot(rlr, monkeypatch, name):
    """scan_multi_kernel with 8, 5, 2 and 3 ladder queries per call: every slot of every template (Q = 8, 4, 2) is a ladder
    query with its own class.  The batched pipeline reports no candidate count."""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    rows, qs, f = L.corpus(name)
    ix = make_index(rlr, name)
    try:
        ix.profile_enable(True)
        g0 = 0
        sizes = [8, 5, 2, 3] * (len(qs) // 18 + 1)
        for m in sizes:
            if g0 + m > len(qs):
                m = len(qs) - g0
            if m < 2:
                break
            ix.profile_read(reset=True)
            r, c = ix.search_topk(qs[g0:g0 + m], f["k"])
            p = ix.profile_read()
            for i in range(m):
                assert_exact(name, g0 + i, r[i], c[i], f"{name} shared scan of {m}, slot {i}")
            assert p.n_batches == 1 and p.n_batch_queries == m and p.n_batch_fallbacks == 0, (name, m, p)
            assert p.n_batches_without_image == 0 and p.n_f16_range_fallbacks == 0 and p.n_candidates == 0, (name, m, p)
            g0 += m
        assert g0 >= len(qs) - 1
    finally:
        ix.close()


def test_shared_binary16_scan_through_the_coalescer(rlr, monkeypatch):
    """scan_multi_h_kernel serves only groups of concurrent single-query calls over binary16 rows: six callers, three ladder
    queries each, released together with a linger of 20 ms.  Which slot of which group a query lands in depends on timing:
    whatever it is, the result must be the oracle's, and at least twelve of the 18 calls must have been served in a group"""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    name = "packed_f16_256"
    rows, qs, f = L.corpus(name)
    ix = make_index(rlr, name)
    try:
        ix.set_coalescing(8, 20000)
        ix.coalesce_stats(reset=True)
        got = run_threads(6, lambda t: [ix.search_topk(qs[t * 3 + i], f["k"]) for i in range(3)])
        st = ix.coalesce_stats()
        ix.set_coalescing(0)
        for t in range(6):
            for i in range(3):
                r, c = got[t][i]
                assert_exact(name, t * 3 + i, r[0], c[0], "coalesced binary16")
        assert st["n_calls"] == 18 and st["n_groups_f16"] > 0 and st["n_groups_f16"] == st["n_groups"], st
        assert st["n_handed_back"] == 0 and st["n_grouped_queries"] >= 12 and st["n_solo"] <= 6, st
    finally:
        ix.close()


# ---------------------------------------------------------------- the matrix-core batch
def batch(ix, name, qs, slots, k, want_without_image, ctx, chunk=None):
    """one batched call; qs[slots[i]] is ladder query i of the corpus.  -> the profile"""
    ix.profile_enable(True)
    ix.profile_read(reset=True)
    r, c = ix.search_topk(qs, k)
    p = ix.profile_read()
    for g, s in enumerate(slots):
        assert_exact(name, g, r[s], c[s], f"{ctx} slot {s}")
    assert p.n_batches == 1 and p.n_batch_queries == len(qs) and p.n_batch_fallbacks == 0, (ctx, p)
    assert p.n_f16_range_fallbacks == 0 and p.n_scan_launches == 0 and p.n_candidates == 0, (ctx, p)
    assert p.n_batches_without_image == want_without_image, (ctx, p)
    return p


@pytest.mark.parametrize("name,image,kernel", [
    ("gemm_768_q17", False, "gemm_nominate_kernel"),         # a ragged second block of 16 queries: slot 16
    ("gemm_f16_1024_q17", False, "gemm_nominate_kernel, binary16 rows"),
    ("gemm_768_q128", True, "gemm_resident_kernel"),
    ("gemm_768_q300", True, "gemm8_kernel"),                 # 256 + a ragged block of 44
])
def test_materialised_batch_every_slot(rlr, monkeypatch, name, image, kernel):
    """a corpus of a little over 4096 rows is its own sample: one materialising launch.  Every query of the batch is a
    ladder query; all of them are held to the oracle (the corpora are small)."""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    rows, qs, f = L.corpus(name)
    ix = make_index(rlr, name)
    try:
        if image:
            ix.enable_batch_image(True)
        f32_plain = not image and f["kind"] == "f32"
        batch(ix, name, qs, range(len(qs)), f["k"], 1 if f32_plain else 0, f"{name} ({kernel})")
    finally:
        ix.close()


@pytest.mark.parametrize("image,nq,kernel", [(False, 0, "gemm_nominate_kernel"), (True, 0, "gemm_resident_kernel"),
                                             (True, 300, "gemm8_kernel")])
def test_sampled_batch_behind_the_sample(rlr, oracle, monkeypatch, image, nq, kernel):
    """135 037 rows: the first 65 536 are the sample (materialised), the rest is filtered in the GEMM epilogue against the
    floor the sample set.  Each ladder's lower k rungs lie inside the sample and set that floor (rank = k at this size);
    its checked rows lie behind it, on every residue modulo 256 twice and on the ragged last tile.  nq = 0: the batch is the
    corpus' 20 ladder queries (a ragged second block of 16).  For the 300-query batch they sit on the first and last slot
    of both query blocks and 16 slots between; the other 280 slots carry ordinary queries, whose results must equal the
    single-query f32 scan of the same index (which test_plain_scans holds to the oracle at every position)."""
    monkeypatch.setenv("RLR_BATCH_MIN", "2")
    name = "sampled_768"
    rows, qs, f = L.corpus(name)
    if nq == 0:
        batch_q, slots = qs, list(range(len(qs)))
    else:
        slots = [0, 255, 256, nq - 1] + [17 + 13 * i for i in range(len(qs) - 4)]
        assert len(set(slots)) == len(qs) and max(slots) < nq
        batch_q = np.stack([oracle.normalize(oracle.synth_query(768, seed=9700 + i)) for i in range(nq)]).astype(np.float32)
        batch_q[slots] = qs
    ix = make_index(rlr, name)
    try:
        if image:
            ix.enable_batch_image(True)
        p = batch(ix, name, batch_q, slots, f["k"], 0 if image else 1, f"sampled ({kernel})")
        if nq:
            r, c = ix.search_topk(batch_q, f["k"])
            for i in sorted(set(range(nq)) - set(slots)):
                r1, c1 = ix.search_topk(batch_q[i], f["k"])  # one query: below RLR_BATCH_MIN, the f32 scan
                assert np.array_equal(r[i], r1[0]) and np.array_equal(bits(c[i]), bits(c1[0])), f"sampled ({kernel}) slot {i}"
        assert p.batch_main_bytes == (len(rows) - L.SAMPLE) * 768 * (2 if image else 4), p   # the filtered pass ran behind the sample
    finally:
        ix.close()


# ---------------------------------------------------------------- masked scans
@pytest.mark.parametrize("name,share,kernel", [
    ("masked_f32_768", 0.5, "scan_masked_fixed_kernel, dense shape"),      # 8-row units, one workgroup per CU
    ("masked_f32_768", 0.03, "scan_masked_fixed_kernel, sparse shape"),    # 16-row units, four per CU
    ("masked_f32_1024", 0.5, "scan_masked_generic_kernel"),
    ("masked_f32_1024", 0.03, "scan_masked_generic_kernel, few rows allowed"),
    ("masked_f16_72", 0.5, "scan_masked_generic_kernel, binary16"),
])
def test_masked_scans(rlr, monkeypatch, name, share, kernel):
    """Two sets of checked rows (ladder_vectors.masked_sets; test_ladder_vectors_cpu.py asserts the masks' shape).  ALONE: the
    only allowed row of its 16-row unit, so of its 8-row unit -- on every residue modulo 64 (the first and last bit of a
    mask word, every unit position) from row 1024 and again from row 20 480, and four rows of the last, partly filled word
    (n mod 64 = 59).  FULL: rows 0..255 with every neighbour allowed.  Every rung is allowed, so the expected result is the
    unfiltered one; every other row is allowed with probability `share`."""
    monkeypatch.setenv("RLR_BATCH_MIN", "100000")
    rows, qs, f = L.corpus(name)
    allowed = L.ladder_mask(name, share)
    dense = len(allowed) * 4 >= len(rows)
    assert dense == (share >= 0.25)
    ix = make_index(rlr, name)
    try:
        with ix.filter_rows(allowed) as flt:
            flt.set_path("scan")
            assert flt.info()["path"] == "scan" and flt.info()["n_allowed"] == len(allowed)
            single_queries(ix, name, ELEM_BYTES[f["kind"]], f"{name} masked ({kernel})",
                           lambda g: tuple(a[0] for a in ix.search_topk(qs[g], f["k"], filter=flt)))
    finally:
        ix.close()


# ---------------------------------------------------------------- shards
def test_three_shards_on_one_gpu(rlr):
    """MultiGpuIndex over [0, 0, 0]: shards of ceil(n / 3) rows, each running its own top-k with the full k over fewer than
    4096 rows -- the single-query pipelines, whatever the batch size.  So every ladder lives inside one shard (its lower
    rungs keep THAT shard's k-th nominated score in 0.75's bin); the checked rows are each shard's first 32 rows and last
    192: both sides of each cut and the whole ragged last tile of each shard.  Each top-k call is served by one exchange
    or one host merge of the shards' own results (rlr_multi_stats)."""
    name = "shards_768"
    rows, qs, f = L.corpus(name)
    bounds = [0] + L.shard_cuts(len(rows)) + [len(rows)]
    flat = f["checked"].ravel()
    assert all(c - 1 in flat and c in flat for c in bounds[1:-1]) and 0 in flat and len(rows) - 1 in flat
    for g in range(len(qs)):
        assert len({int(np.searchsorted(bounds, r, side="right")) for r in f["rungs"][g]}) == 1
    mi = rlr.MultiGpuIndex(768, [0, 0, 0], "f32")
    try:
        mi.upload(rows)
        mi.stats(reset=True)
        calls = 0
        for g0 in range(0, len(qs), 7):                      # the seven queries of one shard together ...
            r, c = mi.search_topk(qs[g0:g0 + 7], f["k"])
            calls += 1
            for i in range(len(r)):
                assert_exact(name, g0 + i, r[i], c[i], "three shards")
        for g in (0, 7, 14, 20):                             # ... and one of each shard alone
            r, c = mi.search_topk(qs[g], f["k"])
            calls += 1
            assert_exact(name, g, r[0], c[0], "three shards, one query")
        st = mi.stats()
        assert st["n_topk_rccl"] + st["n_topk_host_merge"] == calls, st
    finally:
        mi.close()
