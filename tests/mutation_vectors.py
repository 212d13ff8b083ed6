"""The index's state machine as test vectors (test_mutation_vectors_cpu.py proves what they reach, test_gpu_mutations.py
runs them): a fixed plan of uploads, appends, deletes, reserves and copy toggles, a host mirror of what the index must
hold after every step, the probes that are sent after every step, and a model of a nomination copy (the binary16 image in
tiles of 256 rows, the 8-bit copy with its per-row scales) that a mutation may have left stale.

The mirror.  Every row the plan ever stores is one row of a pool (oracle.synth_rows, iid, no clusters, no row twice), so
the mirror after a step is an array of pool ids and `stored(O, dtype)[ids]` is the f32 content the index must return
(rounded through oracle.round_f16 for a binary16 index).  A position changed in a step iff its id changed.

The capacity model restates the library's rule (csrc/index.hip, ensure_rows / sync_q8 / sync_image): rows beyond the
allocation grow it to max(wanted, 1.5 x old, 1024); a copy buffer smaller than the row allocation is replaced and rebuilt
from row 0; an upload rebuilds from row 0; an append rebuilds from the old row count, a delete from the first deleted
row; the image rebuilds whole tiles, the 8-bit copy single rows, both up to the new row count.  It is the model of an
index whose copy was on before the first upload; the toggles move no rows and are steps without a rebuild rule.

The probes.  A stored row, normalised, as the query: its own position must come first (the largest cosine between two
pool rows is 0.39, its own is 1).  A copy position that holds anything but that row -- another row, zeros, another
row's bytes under this row's scale -- nominates it at <= 0.39 * 1.7 while the select collects from (bin floor of the
k-th nominated score) - band >= 0.75 - band, so the row is never re-scored and the result lacks it.

The superset argument.  `lost(...)` nominates with the exact (binary64) dot product of what the copy holds, selects with
band_vectors.select and the WIDEST band any path applies at this shape (`widest_band`: the binary16 bound and the 8-bit
bound, written out as test_band_vectors_cpu.py does, nothing read from the library).  A device path nominates with its
own, narrower or equal band around scores that differ from the model's by less than that band's half, so every row a
device path collects the model collects too: a winner the model loses is a winner the device loses.
"""
import numpy as np

import band_vectors as B

DIM = 256
TILE = 256                     # rows per image tile
BATCH_ROWS = 4096              # the batched paths need at least this many rows
POOL_SEED = 9100
MAX_QUERIES = 64               # per step: self-probes + N_ORDINARY
N_ORDINARY = 4
N_PREFIX = 8
SELF_KS = (1, 3)
ORDINARY_K = 25
FAULTS = ("F1_next_tile_edge", "F2_append_stops_at_old_count", "F3_delete_from_first_dead_plus_256",
          "F4_delete_rebuilds_nothing", "F5_grown_buffer_keeps_no_prefix", "F6a_q8_scales_not_rebuilt",
          "F6b_q8_bytes_not_rebuilt", "F7_last_partial_tile_skipped")

# (name, op, argument); a delete's argument is a function of the row count before it
SPEC = (
    ("toggle_on_before_upload", "toggle", "on_before_upload"),
    ("upload_17_tiles", "upload", 4352),
    ("append_outgrows_capacity", "append", 300),
    # (a reserve grows the row allocation only: the copy buffers are sized for it at the next sync, which therefore
    # rebuilds everything -- the append behind it is not the in-place one; the two appends after that are)
    ("reserve_8192", "reserve", 8192),
    ("append_into_reserved", "append", 200),
    ("append_completes_tile", "append", 12),
    ("append_opens_tile", "append", 1),
    ("append_over_many_tiles", "append", 1400),
    ("delete_tile_interior", "delete", lambda n: [1000, 1700, 2047, 2048, 3333, 4500]),
    ("toggle_on_after_step_5", "toggle", "on_after_step_5"),
    ("delete_on_tile_edge", "delete", lambda n: [1280, 1281, 2000, 4000]),
    ("toggle_drop", "toggle", "drop"),
    ("toggle_reenable", "toggle", "reenable"),
    ("delete_on_tile_last_row", "delete", lambda n: [1023, 1024, 3100]),
    ("toggle_widen_to_single_query", "toggle", "widen_to_single_query"),
    ("delete_whole_tile", "delete", lambda n: list(range(512, 768))),
    ("delete_last_row", "delete", lambda n: [n - 1]),
    # (only three changed rows are probed here, and a stale SCALE of another row moves a nominated score by a factor of
    # 0.6..1.7 only: of the offsets 2, 5, .. 38 this one lets a k = 3 probe see fault F6a, as the CPU test proves.  The
    # proof for this (step, fault) pair rests on that one probe: after a change of POOL_SEED or of an earlier step,
    # test_probes_see_fault[F6a_q8_scales_not_rebuilt] names this step if it no longer holds; then try the first offset
    # a in range(2, 200) with [a, a + 50, n - 1] until CopyModel.lost(step, probes, "q8", "F6a...") is not empty)
    ("delete_in_last_partial_tile", "delete", lambda n: [n // TILE * TILE + 35, n // TILE * TILE + 85, n - 1]),
    ("delete_run_over_three_edges", "delete", lambda n: list(range(2000, 2600))),
    ("delete_with_duplicates", "delete", lambda n: [700, 700, 2304, n - 1, 2304, 701]),
    ("upload_fewer_over_more", "upload", 4200),
    ("delete_every_row", "delete", lambda n: list(range(n))),
    ("append_after_empty", "append", 4300),
    ("delete_down_to_300", "delete", lambda n: list(range(300, n))),
    ("append_back_past_4096", "append", 4000),
)
STEP_NAMES = tuple(s[0] for s in SPEC)
TOGGLES = tuple(s[2] for s in SPEC if s[1] == "toggle")


class Step:
    """one step of the plan, with the state before and after it (ids: pool ids by row position)"""

    def __init__(self, index, name, op, arg):
        self.index, self.name, self.op, self.arg = index, name, op, arg
        self.ids_before = self.ids_after = None
        self.cap_before = self.cap_after = 0              # rows of the row allocation
        self.copy_cap_before = self.copy_cap_after = 0    # rows the copy buffers were sized for
        self.first_changed = None                         # the row the library rebuilds its copies from
        self.fresh = False                                # the copies are rebuilt from row 0
        self.changed = np.zeros(0, np.int64)              # live positions whose content differs from before
        self.tiles = np.zeros(0, np.int64)                # tiles of 256 those positions touch
        self.note = ""

    @property
    def n_before(self):
        return len(self.ids_before)

    @property
    def n_after(self):
        return len(self.ids_after)

    @property
    def dead(self):
        return np.unique(np.asarray(self.arg, np.int64)) if self.op == "delete" else np.zeros(0, np.int64)


def mirror_delete(ids, dead):
    """the mirror's delete: the rows named in `dead` (any order, duplicates ignored) leave, the others close up"""
    keep = np.ones(len(ids), bool)
    keep[np.asarray(dead, np.int64)] = False
    return ids[keep]


def grow(cap, want):
    return cap if want <= cap else max(want, cap + cap // 2, 1024)


def build_plan():
    steps, ids, cap, copy_cap, cursor = [], np.zeros(0, np.int64), 0, 0, 0
    for i, (name, op, arg) in enumerate(SPEC):
        st = Step(i, name, op, arg(len(ids)) if callable(arg) else arg)
        st.ids_before, st.cap_before, st.copy_cap_before = ids, cap, copy_cap
        sync = op in ("upload", "append", "delete")
        if op == "upload":
            ids = np.arange(cursor, cursor + st.arg)
            cursor += st.arg
            cap = grow(cap, st.arg)
            st.first_changed = 0
        elif op == "append":
            st.first_changed = len(ids)
            ids = np.concatenate([ids, np.arange(cursor, cursor + st.arg)])
            cursor += st.arg
            cap = grow(cap, len(ids))
        elif op == "delete":
            st.first_changed = int(st.dead.min())
            ids = mirror_delete(ids, st.arg)
        elif op == "reserve":
            cap = grow(cap, st.arg)
        if sync:
            if copy_cap < max(cap, len(ids), 1):
                copy_cap = max(cap, len(ids), 1)
                st.fresh = True
            st.fresh = st.fresh or st.first_changed == 0
            n0 = min(len(st.ids_before), len(ids))
            same = np.zeros(len(ids), bool)
            same[:n0] = st.ids_before[:n0] == ids[:n0]
            st.changed = np.flatnonzero(~same)
            st.tiles = np.unique(st.changed // TILE)
        st.ids_after, st.cap_after, st.copy_cap_after = ids, cap, copy_cap
        steps.append(st)
    return steps, cursor


_PLAN = None


def plan():
    """-> (steps, number of pool rows); built once"""
    global _PLAN
    if _PLAN is None:
        _PLAN = build_plan()
    return _PLAN


_STORED = {}


def stored(O, dtype="f32"):
    """the pool as an index of `dtype` stores it; shared, never changed"""
    if dtype not in _STORED:
        rows = O.synth_rows(plan()[1], DIM, seed=POOL_SEED, n_clusters=0)
        _STORED[dtype] = O.round_f16(rows) if dtype == "f16" else rows
        _STORED[dtype].setflags(write=False)
    return _STORED[dtype]


# ---------------------------------------------------------------- probes
def probe_positions(st):
    """-> (positions of the step's self-probes, note): the first and last changed row of every touched tile; the rows
    on either side of every seam; N_PREFIX rows of the unchanged prefix.  At most MAX_QUERIES - N_ORDINARY: the tile rows
    (two per tile) come first, then the prefix, then the seams, and the note says what did not fit."""
    n, n0 = st.n_after, st.n_before
    if n == 0:
        return np.zeros(0, np.int64), "empty index: ordinary queries only"
    tile_rows, seams = [], []
    for t in st.tiles:
        c = st.changed[st.changed // TILE == t]
        tile_rows += [int(c[0]), int(c[-1])]
    f = st.first_changed
    if f is not None:
        seams += [f - 1, f, f + 1]                       # the first dead / first appended row and its neighbours
        if len(st.changed):
            for e in range((f // TILE + 1) * TILE, int(st.changed[-1]) + 1, TILE):
                seams += [e - 1, e]                      # each tile edge inside the changed range
    seams += [n0 - 1, n - 1]                             # old and new n_rows - 1
    last_same = n if f is None else min(f, n)
    prefix = [int(p) for p in np.unique(np.linspace(0, last_same - 1, N_PREFIX).astype(np.int64))] if last_same > 0 else []
    out, note = [], ""
    for p in tile_rows + prefix + seams:
        if 0 <= p < n and p not in out:
            if len(out) == MAX_QUERIES - N_ORDINARY:
                note = "more probe rows than fit: two rows per touched tile and the prefix first, the seams cut short"
                break
            out.append(int(p))
    return np.array(out, np.int64), note


def ordinary_queries(O, st):
    return np.stack([O.normalize(O.synth_query(DIM, seed=7000 + N_ORDINARY * st.index + i)) for i in range(N_ORDINARY)])


def oracle_topk(scores, k, allowed=None):
    """the top-k of one oracle scan (over the ascending rows `allowed` only), score descending, row ascending: rows u64,
    scores f32"""
    e = np.asarray(scores, np.float32)
    rows = np.arange(len(e)) if allowed is None else np.asarray(allowed, np.int64)
    order = np.lexsort((rows, -e[rows].astype(np.float64)))[:k]
    return rows[order].astype(np.uint64), e[rows[order]]


class StepProbes:
    """the queries of one step and the oracle's scan of each over the mirror: computed once per (step, dtype), shared by
    every configuration and test, never changed"""

    def __init__(self, O, st, dtype):
        pool = stored(O, dtype)
        self.positions, self.note = probe_positions(st)
        self.n_self = len(self.positions)
        mirror = pool[st.ids_after]
        selfq = [O.normalize(mirror[p]) for p in self.positions]
        self.queries = np.ascontiguousarray(np.stack(selfq + list(ordinary_queries(O, st))), dtype=np.float32)
        self.scores = (np.stack([O.scan(mirror, q) for q in self.queries]) if st.n_after
                       else np.zeros((len(self.queries), 0), np.float32))
        for a in (self.queries, self.scores):
            a.setflags(write=False)

    def groups(self):
        """-> [(query indices, k)]: the self-probes at k = 1 and k = 3, the ordinary queries at k = 25"""
        g = [(np.arange(self.n_self), k) for k in SELF_KS] if self.n_self else []
        return g + [(np.arange(self.n_self, len(self.queries)), ORDINARY_K)]

    def expected(self, qi, k, allowed=None):
        """the oracle's top-k of query qi (over the ascending rows `allowed` only): rows u64, scores f32"""
        return oracle_topk(self.scores[qi], k, allowed)


_PROBES = {}


def step_probes(O, st, dtype="f32"):
    key = (st.index, dtype)
    if key not in _PROBES:
        _PROBES[key] = StepProbes(O, st, dtype)
    return _PROBES[key]


# ---------------------------------------------------------------- the bands, as specified
def scan_band(dim):
    return 2.0 * (dim + 64) * 2.0 ** -24 * 1.0625


def binary16_band(dim, f16_rows):
    op = 2.0 ** -11 if f16_rows else 2.0 ** -10
    return 2.0 * ((op * 1.001 + 2.0 * (dim + 64) * 2.0 ** -24) * 1.0 + 2.0 ** -25 * np.sqrt(dim) * 2.0) * 1.0625


def q8_band(dim, delta_max, scale_max, query_norm):
    qn = query_norm * 1.0001 + 1e-30
    arith = 32.0 * 2.0 ** -24 * 256.0 * np.sqrt(dim) * qn * scale_max * 1.0625
    return 2.0 * (delta_max * 1.001 * qn + arith + 0.5 * scan_band(dim))


def widest_band(delta_max, scale_max, query_norm=1.0, dim=DIM):
    """the widest band any path applies at this shape: the larger of the binary16 and the 8-bit bound"""
    return max(binary16_band(dim, False), q8_band(dim, delta_max, scale_max, query_norm))


# ---------------------------------------------------------------- a possibly stale copy
def fault_applies(st, fault):
    """is the fault's code path taken at all by this step?"""
    if st.op not in ("upload", "append", "delete"):
        return False
    return {"F2": st.op == "append", "F3": st.op == "delete", "F4": st.op == "delete",
            "F5": st.op == "append" and st.copy_cap_after > st.copy_cap_before}.get(fault[:2], True)


def copy_after(st, kind, fault=None):
    """-> (data ids, scale ids) per live position: the pool row whose values (whose scale) the copy of `kind` ("image":
    rebuilt in whole tiles; "q8": rebuilt row by row) holds at each position after the step, -1 for zeros.  The copy was
    right before the step (positions beyond the old row count: zeros).  fault None: the library's documented rule."""
    n, n0, f = st.n_after, st.n_before, st.first_changed
    prev = np.full(n, -1, np.int64)
    prev[:min(n, n0)] = st.ids_before[:min(n, n0)]
    begin = 0 if st.fresh else (f // TILE * TILE if kind == "image" else f)
    end = n
    tag = fault[:2] if fault else ""
    if tag == "F1" and not st.fresh:                      # the next tile edge, not the tile that holds the row
        begin = (f + TILE - 1) // TILE * TILE
    elif tag == "F2":                                     # an append's rebuild stops at the old row count
        end = min(n0, n)
    elif tag == "F3":
        begin = (f + TILE) // TILE * TILE if kind == "image" else f + TILE
    elif tag == "F4":
        begin = n
    elif tag == "F5":                                     # the new buffer: zeros below the first changed row
        prev[:] = -1
        begin = f // TILE * TILE if kind == "image" else f
    elif tag == "F7":
        end = n // TILE * TILE
    if st.copy_cap_after > st.copy_cap_before:            # replaced copy buffers hold nothing yet
        prev[:] = -1
    built = np.zeros(n, bool)
    built[begin:max(begin, end)] = True
    data = np.where(built, st.ids_after, prev)
    scale = data
    if tag == "F6":                                       # only the 8-bit copy has two parts to keep in step
        if kind != "q8":
            return st.ids_after.copy(), st.ids_after.copy()
        data, scale = (data, prev) if fault.startswith("F6a") else (prev, data)
    return data, scale


class CopyModel:
    """what the two copies hold per pool row, in binary64: the binary16 image (rows rounded by oracle.round_f16) and
    the 8-bit copy (band_vectors.q8_model: codes, scales, error norms)"""

    def __init__(self, O):
        pool = stored(O, "f32")
        self.O = O
        self.h = O.round_f16(pool)
        deq, self.delta, self.scale = B.q8_model(pool)
        self.codes = (deq / self.scale[:, None].astype(np.float64)).astype(np.float32)   # small integers: exact
        self.band = widest_band(float(self.delta.max()), float(self.scale.max()))

    def nominate(self, kind, data, scale, Q):
        """[queries, positions] nominated scores of a copy state"""
        out = np.zeros((len(Q), len(data)))
        live = np.flatnonzero((data >= 0) & (scale >= 0))
        if kind == "image":
            out[:, live] = self.O.round_f16(Q).astype(np.float64) @ self.h[data[live]].astype(np.float64).T
        else:
            out[:, live] = (Q.astype(np.float64) @ self.codes[data[live]].astype(np.float64).T) \
                * self.scale[scale[live]].astype(np.float64)[None, :]
        return out

    def lost(self, st, probes, kind, fault):
        """-> [(query index, k)] of the step's probes whose result under the fault differs from the oracle's"""
        data, scale = copy_after(st, kind, fault)
        good = self.nominate(kind, st.ids_after, st.ids_after, probes.queries)
        bad = np.flatnonzero((data != st.ids_after) | (scale != st.ids_after))
        nom = good.copy()
        if len(bad):
            nom[:, bad] = self.nominate(kind, data[bad], scale[bad], probes.queries)
        out = []
        np_err = np.seterr(divide="ignore", invalid="ignore")      # (a copy of zeros nominates 0: no bin, nothing collected)
        for idx, k in probes.groups():
            for qi in idx:
                if k > st.n_after:
                    continue
                want = probes.expected(qi, k)[0]
                assert np.array_equal(B.select(good[qi], probes.scores[qi], k, self.band).astype(np.uint64), want), \
                    (st.name, kind, qi, k, "the right copy must give the oracle's result")
                if not np.array_equal(B.select(nom[qi], probes.scores[qi], k, self.band).astype(np.uint64), want):
                    out.append((int(qi), k))
        np.seterr(**np_err)
        return out, len(bad)


# ---------------------------------------------------------------- the band case: the 8-bit statistic across an append
BAND_KS = (1, 10)
BAND_FORMS = ("append_into_reserved", "append_outgrows_capacity", "small_rows_appended_behind")


def band_case(O, k):
    """band_vectors.q8_rounding split: `base` is the filler alone (the special positions hold more filler), `tail` are
    X, its 150 decoys and its k - 1 champions, appended behind it.  -> (base, tail, query, facts); facts["x"] etc. are
    positions in concatenate([base, tail])."""
    rows, qs, f = B.q8_rounding(O, k)
    special = np.r_[f["x"], f["decoys"], f["champions"]].astype(np.int64)
    base = rows.copy()
    base[special] = O.synth_rows(len(special), rows.shape[1], seed=6300 + k, n_clusters=5)
    tail = rows[special].copy()
    n = len(base)
    facts = dict(k=k, x=n, decoys=n + 1 + np.arange(len(f["decoys"])),
                 champions=n + 1 + len(f["decoys"]) + np.arange(len(f["champions"])), edge=f["edge"],
                 query_norm=f["query_norm"], dim=rows.shape[1])
    return base, tail, qs[0].copy(), facts


def band_case_reversed(O, k):
    """the other direction: the index holds q8_rounding's whole corpus (X on row 50 owns the statistic) and `extra`, filler
    with a sixth of that error norm, is appended behind it in place: a statistic that a partial build starts from zero
    (or takes from the rows it builds alone) loses X.  -> (rows, extra, query, facts)"""
    rows, qs, f = B.q8_rounding(O, k)
    extra = O.synth_rows(200, rows.shape[1], seed=6400 + k, n_clusters=5)
    facts = dict(k=k, x=int(f["x"]), decoys=f["decoys"], champions=f["champions"], query_norm=f["query_norm"], dim=rows.shape[1])
    return rows, extra, qs[0].copy(), facts


# ---------------------------------------------------------------- the wide-row compaction case
WIDE_DIM, WIDE_ROWS, WIDE_SEED = 4096, 40000, 9400
WIDE_CHUNK = (256 << 20) // (WIDE_DIM * 4)      # rows one compaction chunk moves: 16 384


def wide_case():
    """-> (dead rows, surviving old rows by new position, positions to compare, two positions that moved across a seam)"""
    rng = np.random.default_rng(9401)
    first_dead = 100
    run = np.arange(first_dead + WIDE_CHUNK - 10, first_dead + WIDE_CHUNK + 10)
    dead = np.unique(np.r_[first_dead:first_dead + 5, rng.choice(np.arange(first_dead + 5, WIDE_ROWS), WIDE_ROWS // 100, replace=False), run])
    keep = np.delete(np.arange(WIDE_ROWS), dead)
    n = len(keep)
    seams = [first_dead + WIDE_CHUNK * j for j in range(1, (n - first_dead + WIDE_CHUNK - 1) // WIDE_CHUNK)]
    windows = [np.arange(0, 3), np.arange(first_dead - 2, first_dead + 3), np.arange(n - 5, n)]
    windows += [np.arange(s - 2, s + 3) for s in seams]
    sample = rng.choice(n, 1000, replace=False)
    positions = np.unique(np.concatenate(windows + [sample]))
    return dead, keep, positions, seams


def wide_expected(O, keep, positions):
    """the generator's rows that must stand at `positions` after the delete"""
    return np.concatenate([O.synth_rows(1, WIDE_DIM, seed=WIDE_SEED, row0=int(keep[p])) for p in positions])
