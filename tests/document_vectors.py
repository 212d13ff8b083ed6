"""Designed inputs for the document column (rust-local-rag_amd/csrc/docs.hip) with their expected results, pure numpy:
per-row document ids, sets of documents to ask for, and for each pair the filter's mask words, its ascending row list
and the column a deletion leaves.  tests/test_document_vectors_cpu.py holds this generator to an independent restatement
(a Python loop over rows); tests/test_gpu_documents.py holds the device to the generator.

Row counts follow the kernels' scan hierarchy (docs.hip:15-18): a workgroup of the mask / scatter launches covers 4096
rows, a workgroup of the first scan launch covers 1024 of their counts = 4 194 304 rows, one workgroup scans the rest."""
import numpy as np

DOC_NONE = 0xFFFFFFFF
ROWS_PER_GROUP = 4096      # docs.hip:16  kDocsRowsPerGroup
SUMS_PER_GROUP = 1024      # docs.hip:17  kDocsSumsPerGroup
LDS_SET_MAX = 2048         # kernels.h    kDocsLdsMax: the LDS / global membership switch

SMALL_ROW_COUNTS = [1, 63, 64, 65, 127, 128, 129,
                    4095, 4096, 4097]                       # docs.hip:16: a second mask / scatter workgroup starts at 4097
LARGE_ROW_COUNTS = [(1 << 20) + 65,                         # 257 counts to scan
                    4194303, 4194304, 4194305]              # docs.hip:17-18: a second scan workgroup and the second scan
                                                            # level start at 1024 * 4096 + 1 rows
ROW_COUNTS = SMALL_ROW_COUNTS + LARGE_ROW_COUNTS

# "random over 1000 documents" uses ids BASE + 3 d: BASE + 3 d + 1 and + 2 tag nothing but sit between members, so a
# membership search that is off by one slot finds a wrong neighbour
BASE, STEP = 1000, 3


def member_of(ids, docs):
    """which rows belong to one of `docs` (DOC_NONE is never a document)"""
    ids = np.asarray(ids, dtype=np.uint32)
    docs = np.asarray(docs, dtype=np.uint32).ravel()
    return np.isin(ids, docs[docs != DOC_NONE]) & (ids != DOC_NONE)


def mask_words(member):
    """one bit per row, little-endian within a word, ceil(n / 64) uint64 words, tail bits zero"""
    n = member.size
    padded = np.zeros(((n + 63) // 64) * 64, dtype=bool)
    padded[:n] = member
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def expect(ids, docs):
    """-> dict: mask (u64 words), rows (ascending u32 list = the filter's list = a deletion's dead rows), column_after
    (the column once those rows are deleted)"""
    m = member_of(ids, docs)
    return {"mask": mask_words(m), "rows": np.flatnonzero(m).astype(np.uint32),
            "column_after": np.asarray(ids, dtype=np.uint32)[~m]}


def id_patterns(n, seed=0):
    """[(name, ids u32 [n], docs)] for n rows: every id pattern of the issue, each with the documents to ask for"""
    r = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed * 1_000_003 + n)
    out = []
    out.append(("all_one_document", np.full(n, 7, np.uint32), [7]))
    out.append(("no_row_matches", np.full(n, 7, np.uint32), [8]))
    alt = (r & 1).astype(np.uint32)
    out.append(("alternating_even", alt, [0]))               # mask words 0x5555...
    out.append(("alternating_odd", alt, [1]))                # mask words 0xAAAA...
    for start in (0, 1, 63, 64):
        for length in (1, 63, 64, 65):
            if start >= n:
                continue
            ids = np.full(n, 3, np.uint32)
            ids[start:start + length] = 4
            out.append((f"run_{length}_at_{start}", ids, [4]))
    for row in sorted({0, 63, 64, n - 1}):
        if row < n:
            ids = np.full(n, 3, np.uint32)
            ids[row] = 9
            out.append((f"single_row_{row}", ids, [9]))
    ids = np.where(r % 3 == 0, DOC_NONE, r % 2).astype(np.uint32)
    out.append(("none_interleaved", ids, [0, 1]))
    out.append(("none_interleaved_one", ids, [1]))
    out.append(("random_1_document", np.full(n, 11, np.uint32), [11]))
    out.append(("random_3_documents", rng.integers(0, 3, n).astype(np.uint32), [2, 0]))
    ids = (BASE + STEP * rng.integers(0, 1000, n)).astype(np.uint32)
    out.append(("random_1000_documents", ids, [BASE + STEP * d for d in (5, 17, 999, 0, 400)]))
    return out


def random_1000(n, seed=0):
    """the ids of the "random over 1000 documents" pattern alone"""
    return id_patterns(n, seed)[-1][1]


def query_sets(seed=0):
    """[(name, docs)] to ask of random_1000 ids: sizes 1, 2, either side of the LDS / global switch, 5000; unsorted, with
    repeats, with ids that tag nothing (BASE + 3 d + 1, BASE + 3 d + 2, ids below BASE, ids far above)"""
    rng = np.random.default_rng(seed + 77)
    real = BASE + STEP * np.arange(1000)

    def mixed(size):
        # a third real documents, the rest ids that tag nothing: between the real ones, below and above them
        n_real = min(size // 3 + 1, 1000)
        nothing = np.concatenate([real + 1, real + 2, np.arange(BASE), 10_000 + np.arange(8000)])
        docs = np.concatenate([rng.choice(real, n_real, replace=False), rng.choice(nothing, size - n_real, replace=False)])
        assert np.unique(docs).size == size
        return rng.permutation(docs).astype(np.uint32)      # unsorted

    out = [("one", np.array([BASE + STEP * 5], np.uint32)),
           ("two_unsorted", np.array([BASE + STEP * 900, BASE + STEP * 5], np.uint32)),
           ("lds_max", mixed(LDS_SET_MAX)),
           ("lds_max_plus_1", mixed(LDS_SET_MAX + 1)),
           ("five_thousand", mixed(5000))]
    rep = mixed(300)
    out.append(("repeats", np.concatenate([rep, rep[::-1], rep[:7]])))
    out.append(("repeats_past_the_switch", np.concatenate([mixed(LDS_SET_MAX - 10), real[:40].astype(np.uint32), real[:40].astype(np.uint32)])))
    out.append(("tags_nothing", np.array([BASE + 1, BASE + 2, 0, 999, 4_000_000_000], np.uint32)))
    out.append(("all_real_documents", rng.permutation(real).astype(np.uint32)))
    return out


def delete_patterns(n):
    """[(name, ids u32 [n], docs)]: first row, last row, everything, nothing, every other row, one run in the middle"""
    r = np.arange(n, dtype=np.int64)
    base = (20 + r // 50).astype(np.uint32)                  # documents of 50 rows: the surviving column is not constant
    out = []
    ids = base.copy(); ids[0] = 5
    out.append(("first_row", ids, [5]))
    ids = base.copy(); ids[n - 1] = 5
    out.append(("last_row", ids, [5]))
    out.append(("everything", np.where(r & 1, 5, 6).astype(np.uint32), [6, 5]))
    out.append(("nothing", base.copy(), [5]))
    ids = base.copy(); ids[::2] = 5
    out.append(("every_other_row", ids, [5]))
    ids = base.copy(); ids[n // 4: n // 4 + max(n // 8, 1)] = 5
    out.append(("one_run", ids, [5]))
    return out
