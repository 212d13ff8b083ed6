"""Designed inputs of the batched text search with a document scope PER QUERY (rlr_lexical_score_batch_scoped,
rlr_engine_search_text_batch_scoped), shared by tests/test_scoped_text_cpu.py -- which clears every engine vector on the
CPU -- and the two GPU test modules.  Corpora, weights, modes, top-ks, batch sizes and texts are those of
text_batch_filtered_vectors; what is new is the scope of each query."""
import numpy as np

import text_batch_filtered_vectors as V

# the six scopes of the one-filter vectors and four that put need_q, the pool size and |F_q| < top_k at different values
# inside one batch: 1, 10, 31 and 611 rows
SCOPES = V.SCOPES + [["doc0.pdf"], ["doc1.pdf", "doc5.pdf"], ["doc7.pdf"], ["doc10.pdf", "doc11.pdf"]]
SCOPE_ROWS = [200, 775, 1500, 0, 65, 0, 1, 10, 31, 611]
# query seeds the CPU test clears per corpus (the largest batch has 17 queries; the other corpora's 9)
N_SEEDS = {"f32_768": 17, "f32_256": 9, "f32_1024": 9, "f16_1024": 9}


def batch_scopes(n, rot):
    """query i of a batch searches inside SCOPES[(i + rot) % 10]"""
    return [(i + rot) % len(SCOPES) for i in range(n)]


def engine_grid(corpus):
    """(rot, weights index, lambda, stage, top_k, batch size, text shift): the full product of weights, modes and top-ks on
    the 768-d corpus with the batch size, the scope rotation and the text shift rotating through it (rot steps by 3, a unit
    of Z/10: every scope meets every slot); the reduced grid on the other corpora"""
    out, i = [], 0
    if corpus == "f32_768":
        for wi in range(len(V.WEIGHTS)):
            for lam, stage in V.MODES:
                for k in V.TOP_KS:
                    out.append(((3 * i) % len(SCOPES), wi, lam, stage, k, V.BATCHES[i % len(V.BATCHES)], i % len(V.TEXTS)))
                    i += 1
    else:
        for lam, stage in ((0.0, 1), (0.3, 0)):
            for n in (3, 9):
                for rot in (0, 6):
                    out.append((rot, 0, lam, stage, 7, n, i % len(V.TEXTS)))
                    i += 1
    return out


# ---- the lexical call: scopes confined to one 2048-row slice each, first allowed row = first or last row of the slice ---
def slice_scopes(n):
    """three scopes of an n-row index (4096 < n <= 6144), scope j inside slice j: from its first row on, or up to its last"""
    return [np.arange(0, 40), np.arange(4095 - 40, 4096), np.arange(4096, min(n, 4096 + 90)), np.array([2047]),
            np.array([2048]), np.arange(n - 30, n)]


SLICE_OF = [0, 1, 2, 0, 1, 2]   # the slice each scope of slice_scopes lies in
