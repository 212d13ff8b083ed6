"""Partial top-k lists for the exchange step's merge (rlr_merge_topk), built on the host exactly as 1..16 ranks would
deliver them (test_merge_vectors_cpu.py holds the reference merge below to sharded.merge_packed and the packing to the
library's rlr_pack_result; test_gpu_exchange_merge.py runs every vector through the kernel).

A vector is `gathered` uint64 [world, nq, k] -- list (r, q) = the packed (score key << 32 | 0xFFFFFFFF - local row) results
of shard r for query q, sorted descending, zeros behind -- plus `bases` uint64 [world], the first global row of each shard.

  shapes   SHAPES: world * k = 1, 1023, 1024, 1025, 8190 and 8192 (the strided loops of the 1024-thread workgroup, the
           8192-entry limit)
  fill     every list holds 0, 1, k - 1 or k valid entries.  With nq = 5: query 1 has all k winners on ONE shard, query 2
           has only empty lists, query 3 fewer than k valid entries in total, query 4 one full list that is 60 % NaN beside lists of
           0 or 1 entries (NaN from several shards reaches the output); query 0 is drawn at random
  scores   standard normals mixed half and half with LEVELS (ties by the dozen inside and across shards; NaN = key 0
           comes out last, ascending global row).  No -0.0: the key order puts it below +0.0 while a host-side merge
           compares them equal, and a search cannot emit it (the reference sum starts at +0.0; the GPU test pins that)
  bases    unequal shard sizes, shard 1 (world >= 3) is EMPTY and shares its base with shard 2, the last shard ends at
           global row 2^32 - 3 (the 0xFFFFFFFF - row arithmetic near the top of the 32-bit row word)
  variants "sorted" as above; "unsorted": every list's k slots permuted, zeros in between (the bitonic fallback; same
           expected output); "marker": nq = 5, slot 0 of one shard's list is ~0 for queries 1 and 3
"""
import numpy as np

SHAPES = ((1, 1), (1, 8192), (2, 512), (3, 341), (5, 205), (7, 1170), (8, 100), (16, 1), (16, 512))
NQS = (1, 5)
VARIANTS = ("sorted", "unsorted", "marker")
MARKER_QUERIES = (1, 3)
LEVELS = np.array([0.5, 0.25, -0.25, 0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 3e38], dtype=np.float32)
LOW_LEVELS = np.array([0.5, 0.25, -0.25, 0.0, -np.inf, np.nan, 1e-40, -1e-40], dtype=np.float32)   # all below 100
PAD_ROW = np.uint64(0xFFFFFFFFFFFFFFFF)
PAD_BITS = np.uint32(0x7FC00000)
OVERFLOWED = np.uint32(0xFFFFFFFF)
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------- the packed format (csrc/common.h), in numpy
def score_key(s):
    """f32 -> u32 whose unsigned order is the score order; every NaN -> 0"""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0), key).astype(np.uint32)


def key_bits(key):
    """u32 key -> the f32 bit pattern it stands for (key 0 -> the quiet NaN 0x7FC00000)"""
    k = np.ascontiguousarray(key, dtype=np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return np.where(k == 0, PAD_BITS, b).astype(np.uint32)


def pack(scores, rows):
    return (score_key(scores).astype(np.uint64) << np.uint64(32)) | (M32 - np.ascontiguousarray(rows, dtype=np.uint64))


# ---------------------------------------------------------------- the reference merge
def reference_merge(gathered, bases, k):
    """per query: drop the zeros, rebase the low word to the global row, sort the u64 keys descending, take k.
    -> (rows u64 [nq, k] padded with ~0, score bits u32 [nq, k] padded with 0x7FC00000, n u32 [nq])"""
    world, nq, kk = gathered.shape
    rows = np.full((nq, k), PAD_ROW, dtype=np.uint64)
    sbits = np.full((nq, k), PAD_BITS, dtype=np.uint32)
    n = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        keys = []
        for r in range(world):
            p = gathered[r, q]
            p = p[p != 0]
            glob = np.uint64(bases[r]) + (M32 - (p & M32))
            assert (glob < M32).all()
            keys.append((p & ~M32) | (M32 - glob))
        keys = np.sort(np.concatenate(keys))[::-1][:k]
        n[q] = keys.size
        rows[q, :keys.size] = M32 - (keys & M32)
        sbits[q, :keys.size] = key_bits((keys >> np.uint64(32)).astype(np.uint32))
    return rows, sbits, n


# ---------------------------------------------------------------- the generator
def shard_sizes(world, k):
    """unequal, every non-empty shard holds at least k rows; shard 1 of three or more is empty"""
    sizes = np.array([k + 3 + 7 * r for r in range(world)], dtype=np.uint64)
    if world >= 3:
        sizes[1] = 0
    return sizes


def make_bases(world, k):
    sizes = shard_sizes(world, k)
    bases = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    bases[-1] = np.uint64(2 ** 32 - 2) - sizes[-1]
    if world >= 3:
        bases[1] = bases[2]                                       # (world 3: the next shard is the last one)
    assert (np.diff(bases.astype(np.int64)) >= 0).all()
    return bases, sizes


def _scores(rng, c, levels=LEVELS):
    s = rng.standard_normal(c).astype(np.float32)
    lvl = rng.random(c) < 0.5
    s[lvl] = levels[rng.integers(0, len(levels), int(lvl.sum()))]
    return s


def _list(rng, k, size, c, scores):
    """one sorted list of c valid entries over distinct local rows of a shard of `size` rows, zeros behind"""
    out = np.zeros(k, dtype=np.uint64)
    if c:
        local = rng.choice(int(size), size=c, replace=False).astype(np.uint64)
        out[:c] = np.sort(pack(scores, local))[::-1]
    return out


def make_vector(world, k, nq, variant="sorted", seed=0):
    """-> (gathered u64 [world, nq, k], bases u64 [world]); the sorted / unsorted / marker variants of one (world, k, nq,
    seed) hold the same entries"""
    rng = np.random.default_rng([world, k, nq, seed])
    bases, sizes = make_bases(world, k)
    live = np.flatnonzero(sizes)
    counts_of = sorted({0, 1, k - 1, k})
    g = np.zeros((world, nq, k), dtype=np.uint64)
    for q in range(nq):
        kind = {1: "one_shard", 2: "empty", 3: "short", 4: "nan_heavy"}.get(q, "random") if nq == 5 else "random"
        counts = np.zeros(world, dtype=np.int64)
        if kind == "random":
            counts[live] = rng.choice(counts_of, size=live.size)
            counts[live[rng.integers(0, live.size)]] = k          # at least one full list
        elif kind == "one_shard":
            counts[live] = rng.choice(counts_of, size=live.size)
            counts[live[q % live.size]] = k
        elif kind == "nan_heavy":
            counts[live] = rng.choice([0, 1], size=live.size)
            counts[live[rng.integers(0, live.size)]] = k
        elif kind == "short":
            some = live[: min(live.size, k - 1)]
            counts[some] = 1
        for r in range(world):
            c = int(counts[r])
            if kind == "one_shard" and r == live[q % live.size]:
                s = (np.abs(rng.standard_normal(c)) + 100.0).astype(np.float32)
                top = rng.random(c) < 0.3
                s[top] = np.array([np.inf, 3e38], np.float32)[rng.integers(0, 2, int(top.sum()))]
            else:
                s = _scores(rng, c, LOW_LEVELS if kind == "one_shard" else LEVELS)
                if kind == "nan_heavy":
                    s[rng.random(c) < 0.6] = np.nan
            g[r, q] = _list(rng, k, sizes[r], c, s)
    if variant == "unsorted":
        for r in range(world):
            for q in range(nq):
                g[r, q] = g[r, q][rng.permutation(k)]
    elif variant == "marker":
        assert nq == 5
        for q in MARKER_QUERIES:
            g[live[(q + 1) % live.size], q, 0] = PAD_ROW
    elif variant != "sorted":
        raise ValueError(variant)
    return g, bases


def expected(world, k, nq, variant="sorted", seed=0):
    """the merged result every variant must produce: the reference merge of the SORTED vector; marker queries report
    OVERFLOWED in n and their rows / scores are not defined (None in `defined`)"""
    g, bases = make_vector(world, k, nq, "sorted", seed)
    rows, sbits, n = reference_merge(g, bases, k)
    defined = np.ones(nq, dtype=bool)
    if variant == "marker":
        defined[list(MARKER_QUERIES)] = False
        n = n.copy()
        n[list(MARKER_QUERIES)] = OVERFLOWED
    return rows, sbits, n, defined


def all_cases():
    """(world, k, nq, variant) of every vector the GPU test runs"""
    for world, k in SHAPES:
        for nq in NQS:
            for variant in VARIANTS:
                if variant == "marker" and nq != 5:
                    continue
                yield world, k, nq, variant
