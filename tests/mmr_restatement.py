"""A Gram-based restatement of the oracle's MMR loop (oracle.mmr, rag_engine.rs:767-839) for the full drains of the GPU
tests, where the literal loop's k^2 * P * dim / 2 multiplications take minutes: the pairwise similarities are computed once
(oracle.scan: reference-order dot products) and the greedy loop runs over that matrix with the same bookkeeping -- the
`remaining` vector with swap_remove, fold(0.0, max) over the finite similarities, strict `>` in visiting order, the
finite checks, the break when no finite candidate is left.  test_mmr_restatement_cpu.py pins it bit for bit against
oracle.mmr before any GPU test relies on it.  Also the awkward relevance scores shared by those tests."""
import numpy as np


def gram(oracle, emb):
    """G[i, j] = the reference-order dot product of rows i and j (f32, bit-identical to oracle.dot)"""
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    g = np.empty((emb.shape[0], emb.shape[0]), dtype=np.float32)
    for i in range(emb.shape[0]):
        g[i] = oracle.scan(emb, emb[i])
    return g


def mmr_from_gram(g, scores, top_k, lam):
    """-> (order u32[n], mmr f32[n]) as oracle.mmr returns them"""
    rel = np.ascontiguousarray(scores, dtype=np.float32)
    P = rel.size
    if P == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.float32)
    lam = np.float32(lam)
    one_minus = np.float32(1.0) - lam
    rem = np.arange(P)
    order, logged = [0], [np.float32(np.nan)]                   # first = remaining.swap_remove(0), unconditional
    n_rem = P - 1
    rem[0] = rem[n_rem]
    max_sim = np.zeros(P, dtype=np.float32)
    rel_finite = np.isfinite(rel)
    with np.errstate(all="ignore"):
        while len(order) < top_k and n_rem > 0:
            c = rem[:n_rem].copy()                             # visiting order
            sim = g[order[-1], c]
            max_sim[c] = np.where(np.isfinite(sim), np.maximum(max_sim[c], sim), max_sim[c])
            m = one_minus * rel[c] - lam * max_sim[c]          # two rounded products, one rounded difference
            ok = rel_finite[c] & np.isfinite(m)
            if not ok.any():                                   # best stayed NEG_INFINITY
                break
            at = int(np.argmax(np.where(ok, m, -np.inf)))      # first of the largest: strict `>`, -0.0 == +0.0
            order.append(int(c[at]))
            logged.append(m[at])
            n_rem -= 1
            rem[at] = rem[n_rem]                               # swap_remove(best_idx)
    return np.array(order, dtype=np.uint32), np.array(logged, dtype=np.float32)


def awkward_scores(rng, P, nonfinite=True):
    """relevance with ties, zeros of both signs and (optionally) NaN / +Inf / -Inf, never in slot 0's favour: the first
    candidate is taken unconditionally whatever its score"""
    sc = (rng.standard_normal(P) * 0.2).astype(np.float32)
    sc[rng.integers(0, P, 12)] = sc[0]                         # relevance ties
    sc[rng.integers(0, P, 3)] = 0.0
    sc[rng.integers(0, P, 3)] = -0.0
    if nonfinite and P > 1:
        sc[rng.integers(1, P, 2)] = np.nan                     # non-finite relevance is never picked
        sc[rng.integers(1, P, 1)] = np.inf
        sc[rng.integers(1, P, 1)] = -np.inf
    return sc
