"""The Gram-based MMR restatement (mmr_restatement.py) pinned bit for bit against the oracle's literal loop, on pools of
up to 300 candidates with duplicated rows (similarity ties) and the awkward relevance the GPU tests use: ties, zeros of
both signs, NaN and both infinities; every lambda regime; k from 0 to the full drain."""
import numpy as np
import pytest

import mmr_restatement as R
from conftest import bits


@pytest.mark.parametrize("P,dim", [(1, 8), (2, 8), (3, 70), (17, 96), (64, 70), (65, 8), (128, 96), (300, 70), (300, 96)])
def test_restatement_equals_oracle_loop(oracle, P, dim):
    rng = np.random.default_rng([P, dim])
    rows = oracle.synth_rows(P + 20, dim, seed=4400 + P, n_clusters=4)
    if P > 12:
        rows[5:11] = rows[2]                                     # exact duplicates inside the pool
    big = P >= 300                                               # (a drain of 300 costs the literal loop ~0.5 s)
    for f16 in ((dim == 96,) if big else (False, True)):
        stored = oracle.round_f16(rows) if f16 else rows
        emb = stored[rng.permutation(P + 20)[:P]]
        g = R.gram(oracle, emb)
        assert np.array_equal(bits(g), bits(g.T))
        assert bits(g[0, P - 1]) == bits(np.float32(oracle.dot(emb[0], emb[P - 1])))
        drained = set()
        for lam in (0.0, 0.3, 0.7, 1.0):
            for nonfinite in ((lam != 0.3,) if big else (False, True)):
                sc = R.awkward_scores(rng, P, nonfinite)
                for k in sorted({5, P} if big else {0, 1, 5, P // 2, P}):
                    wo, wm = oracle.mmr(emb, sc, k, lam)
                    go, gm = R.mmr_from_gram(g, sc, k, lam)
                    assert np.array_equal(go, wo), (P, dim, f16, lam, nonfinite, k)
                    assert np.array_equal(bits(gm[1:]), bits(wm[1:])), (P, dim, f16, lam, nonfinite, k)
                    assert np.isnan(gm[0]) and np.isnan(wm[0])
                    if k == P:
                        drained.add(len(go) == P)
        if P >= 17:
            assert drained == {True, False}                      # both ends: remaining ran empty / no finite candidate left
