"""The merge vectors (merge_vectors.py) checked without a GPU: the numpy packing equals the library's host-side
rlr_pack_result / rlr_unpack_result, the numpy reference merge equals sharded.merge_packed (the torch merge of the gloo
test) on every vector the GPU test runs -- the marker and unsorted variants excepted, which merge_packed does not define --
and the vectors hold what their description promises (fill counts, ties, NaN, the empty shard, rows next to 2^32)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import merge_vectors as V


def test_numpy_packing_equals_the_librarys(rlr):
    L = rlr.lib()
    rng = np.random.default_rng(5)
    scores = np.concatenate([V.LEVELS, np.array([-0.0, 1.0, -1.0, 1e-45, -1e-45, 3.4028235e38, -3.4028235e38], np.float32),
                             rng.standard_normal(200).astype(np.float32),
                             np.array([0x7F800001, 0xFFC00000, 0x7FFFFFFF, 0xFF800001], np.uint32).view(np.float32)])
    rows = np.concatenate([[0, 1, 0xFFFFFFFE, 0xFFFFFFFF, 0x80000000],
                           rng.integers(0, 2 ** 32, scores.size - 5)]).astype(np.uint64)
    want = V.pack(scores, rows)
    for i in range(scores.size):
        p = L.rlr_pack_result(C.c_float(scores[i]), C.c_uint32(int(rows[i])))
        assert p == int(want[i]), (i, scores[i], rows[i])
        s, r = C.c_float(), C.c_uint32()
        L.rlr_unpack_result(C.c_uint64(p), C.byref(s), C.byref(r))
        assert r.value == int(rows[i])
        got = np.array([s.value], np.float32).view(np.uint32)[0]
        assert got == V.key_bits(V.score_key(scores[i:i + 1]))[0], (i, scores[i])
        if not np.isnan(scores[i]):
            assert got == scores[i:i + 1].view(np.uint32)[0]          # every number travels bit for bit, -0.0 included
        else:
            assert got == V.PAD_BITS and (p >> 32) == 0
    # the key order is the score order, -0.0 strictly below +0.0, NaN below everything
    ladder = np.array([np.nan, -np.inf, -3e38, -1.0, -1e-40, -0.0, 0.0, 1e-40, 0.25, 0.5, 3e38, np.inf], np.float32)
    assert (np.diff(V.score_key(ladder).astype(np.int64)) > 0).all()


@pytest.mark.parametrize("world,k", V.SHAPES)
def test_reference_merge_equals_torch_merge(rlr, world, k):
    import torch
    sharded = importlib.import_module("rust-local-rag_amd.sharded")
    for nq in V.NQS:
        g, bases = V.make_vector(world, k, nq)
        rows, sbits, n = V.reference_merge(g, bases, k)
        t_rows, t_key = sharded.merge_packed(torch.from_numpy(g.view(np.int64)), torch.from_numpy(bases.astype(np.int64)), k)
        t_rows, t_key = t_rows.numpy(), t_key.numpy()
        assert t_rows.shape == (nq, k)
        for q in range(nq):
            m = int(n[q])
            assert np.array_equal(t_rows[q, :m].astype(np.uint64), rows[q, :m]), (world, k, nq, q)
            assert (t_rows[q, m:] == -1).all() and (rows[q, m:] == V.PAD_ROW).all()
            assert np.array_equal(sharded.key_to_score(t_key[q]).view(np.uint32), sbits[q]), (world, k, nq, q)
        # every variant of the vector holds the same entries, so the same merged result
        want = V.expected(world, k, nq, "unsorted")
        assert np.array_equal(want[0], rows) and np.array_equal(want[1], sbits) and np.array_equal(want[2], n)
        u, _ = V.make_vector(world, k, nq, "unsorted")
        assert np.array_equal(np.sort(u, axis=2), np.sort(g, axis=2))
        ur, us, un = V.reference_merge(u, bases, k)
        assert np.array_equal(ur, rows) and np.array_equal(us, sbits) and np.array_equal(un, n)


def test_vectors_hold_what_they_promise():
    n_all = sorted({w * k for w, k in V.SHAPES})
    assert n_all == [1, 16, 800, 1023, 1024, 1025, 8190, 8192]
    seen_counts, ties_within, ties_across, nan_runs = set(), 0, 0, 0
    unsorted_seen = 0
    for world, k in V.SHAPES:
        bases, sizes = V.make_bases(world, k)
        assert len(set(sizes[sizes > 0].tolist())) == int((sizes > 0).sum())         # unequal shard sizes
        assert int(bases[-1] + sizes[-1]) == 2 ** 32 - 2                              # last global row 2^32 - 3
        if world >= 3:
            assert sizes[1] == 0 and bases[1] == bases[2]                             # the empty shard shares its base
        for nq in V.NQS:
            g, _ = V.make_vector(world, k, nq)
            valid = g != 0
            counts = valid.sum(axis=2)
            assert np.isin(counts, [0, 1, k - 1, k]).all()
            if k > 2:
                seen_counts |= {{0: "0", 1: "1", k - 1: "k-1", k: "k"}[c] for c in counts.ravel().tolist()}
            assert ((g[valid] >> np.uint64(32)) != np.uint64(0x7FFFFFFF)).all()       # no -0.0 score
            assert (valid[:, :, :-1] >= valid[:, :, 1:]).all()                        # zeros behind the valid entries
            assert (g[:, :, :-1] >= g[:, :, 1:]).all()                                # every list descending
            local = V.M32 - (g & V.M32)
            assert (local[valid] < np.broadcast_to(sizes[:, None, None], g.shape)[valid]).all()
            rows, sbits, n = V.reference_merge(g, bases, k)
            assert (n == np.minimum(counts.sum(axis=0), k)).all()
            if world >= 3:
                assert counts[1].sum() == 0
            if nq == 5:
                assert counts[:, 2].sum() == 0 and n[2] == 0                          # all padding
                assert counts[:, 3].sum() < k and n[3] == counts[:, 3].sum()          # fewer than k in total
                owner = np.searchsorted(bases, rows[1], side="right") - 1             # every winner from one shard
                assert n[1] == k and len(set(owner.tolist())) == 1
                if world > 2 and k > 1:
                    assert counts[:, 1].sum() > k                                     # ... although others hold entries
                m, _ = V.make_vector(world, k, nq, "marker")
                diff = np.argwhere(m != g)
                assert sorted(diff[:, 1].tolist()) == list(V.MARKER_QUERIES) and (diff[:, 2] == 0).all()
                assert (m[m != g] == V.PAD_ROW).all()
            for q in range(nq):
                m = int(n[q])
                s = sbits[q, :m]
                nan = s == V.PAD_BITS
                if nan.any():                                                         # NaN last, ascending global row
                    first = int(np.argmax(nan))
                    assert nan[first:].all() and (np.diff(rows[q, first:m].astype(np.int64)) > 0).all()
                    nan_runs += int(nan.sum() > 1)
                same = s[1:] == s[:-1]
                assert (np.diff(rows[q, :m].astype(np.int64))[same] > 0).all()        # ties: ascending global row
                own = np.searchsorted(bases, rows[q, :m], side="right") - 1
                ties_within += int((same & (own[1:] == own[:-1])).sum())
                ties_across += int((same & (own[1:] != own[:-1])).sum())
            u, _ = V.make_vector(world, k, nq, "unsorted")
            unsorted_seen += int((u[:, :, :-1] < u[:, :, 1:]).any())
    assert seen_counts == {"0", "1", "k-1", "k"}
    assert ties_within >= 12 and ties_across >= 12 and nan_runs >= 5
    assert unsorted_seen >= 2 * len(V.SHAPES) - 4                                     # (k = 1 lists cannot be out of order)
    assert not np.signbit(V.LEVELS[V.LEVELS == 0]).any()
    assert sum(1 for _ in V.all_cases()) == len(V.SHAPES) * 5
