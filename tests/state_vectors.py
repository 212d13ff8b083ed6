"""Range, grouped and capped search across the index's state machine, as test vectors (test_state_vectors_cpu.py proves
what they reach, test_gpu_state_searches.py runs them).  The plan, the pool, the row mirror and the copy model are
mutation_vectors'; this file adds what the six entries read beside the rows:

The document mirror.  Every pool id has a document by a fixed rule (`doc_of`): of every 20 consecutive ids 13 belong to
one of N_BIG large documents (two thirds of any index: several rows of one document in every top-25 list), 5 to a small
document of their own block and 2 to none.  The column the index must hold after a step is a pure function of the plan
(`column`): `raw` straight after the mutation under the library's rules -- an append leaves its tail DOC_NONE, an upload
drops the column, delete_rows compacts it, a regrow keeps it -- and `tagged` after the walker's tagging (the appended
tail by tag_rows in runs of equal documents or the whole column by set_documents, in turn; the whole column after every
upload), which is doc_of(ids_after).  `buffer_before` is what the column's buffer holds beyond the row count: the
documents earlier deletes left behind.

The probes.  At most MAX_PROBES of mutation_vectors.step_probes' queries per step: the rows around the step's seam, a
spread of its changed and unchanged rows, and the ordinary queries.  Range: a self-probe asks tau = 0.75 (the largest
cosine between two pool rows is 0.39: the answer is its own row) and its own rank-25 score (25 hits: at cap 10 the single
entry hands the rows to the top-k path, which nominates over the copy that is on); an ordinary query asks the exact
score at ranks 1, 25 and about 300 and one ulp above each.  Grouped: GROUPED.  Capped: CAPPED, each probe with a lexical list of its own
(`lex_for`): none, the step's probe rows, or the live rows of a fixed residue class of pool ids.

Expectations come from range_vectors.expect, grouped_vectors.expect, capped_vectors.define (and oracle.mmr over the
pool) on oracle.scan over the mirror; nothing is read from the library.

Faults.  The copy faults of mutation_vectors.FAULTS, seen through the range GEMM over the image (`range_under_copy`;
the 8-bit faults F6a / F6b leave the image right) and, all eight, through the top-k hand-off of the rank-25 self-probes
(`groups` / `expected`: mutation_vectors.CopyModel.lost reads a StateProbes as it reads its own probes);
COLUMN_FAULTS, planted in `column`; STRIDE_FAULT, planted in `range_under_stride`.  The forms every batched call must
report are restated from the library's dispatch (`range_batch_forms`, `chunk_forms`)."""
import numpy as np

import capped_vectors as CV
import grouped_batch_vectors as GB
import grouped_vectors as G
import mutation_vectors as M
import range_batch_vectors as RB
import range_vectors as R

F32 = np.float32
DOC_NONE = G.DOC_NONE
MAX_PROBES = 16
N_SELF = MAX_PROBES - M.N_ORDINARY
N_BIG, SMALL_BASE = 5, 1000
SELF_TAU = F32(0.75)
RANKS = (1, 25, 300)
RANGE_CAPS = (10, 512)                         # below and above n_total at ranks 25 and 300
GROUPED = tuple((k, m) for k in (1, 3, 25) for m in (1, 3))
RAW_GROUPED = ((25, 1), (3, 1))                # what is asked before the walker tags
W_E, W_L = CV.W_EMBEDDING, CV.W_LEXICAL        # capped_vectors' weights
LAM = 0.7
# (need, per_doc, diversify, picks)
CAPPED = tuple((need, m, div, (need + 1) // 2 if div else need) for need in (3, 10) for m in (1, 2) for div in (False, True))
EPS_SCAN = M.scan_band(M.DIM) / 2.0
EPS_IMAGE = M.binary16_band(M.DIM, False) / 2.0
COLUMN_FAULTS = ("C1_delete_leaves_column", "C2_compaction_shifted_from_seam", "C3_append_tail_keeps_buffer",
                 "C4_regrow_loses_column", "C5_upload_keeps_column")
STRIDE_FAULT = "S1_score_stride_of_old_row_count"
IMAGE_FAULTS = tuple(f for f in M.FAULTS if not f.startswith("F6"))      # F6a / F6b touch the 8-bit copy alone
SHARING_STEPS = ("append_completes_tile", "delete_whole_tile", "append_back_past_4096")


# ---------------------------------------------------------------- documents
def doc_of(ids):
    """the document of every pool id"""
    ids = np.asarray(ids, np.int64)
    m, block = ids % 20, ids // 20
    return np.where(m < 13, block % N_BIG, np.where(m < 18, SMALL_BASE + block, DOC_NONE)).astype(np.uint32)


def runs(docs):
    """[(first, count, doc)] of the runs of equal tagged documents in `docs`"""
    docs = np.asarray(docs, np.uint32)
    if docs.size == 0:
        return []
    edges = np.r_[0, np.flatnonzero(docs[1:] != docs[:-1]) + 1, docs.size]
    return [(int(a), int(b - a), int(docs[a])) for a, b in zip(edges[:-1], edges[1:]) if docs[a] != DOC_NONE]


class Column:
    """the column of one step: raw (after the mutation), tagged (after the walker), how the walker tags"""

    def __init__(self, raw, tagged, tag):
        self.raw, self.tagged, self.tag = raw, tagged, tag

    @property
    def has_raw_phase(self):
        return self.tag is not None


_BUFFERS = None


def _buffers():
    """the column's buffer before every step under the library's rules (the walker's tagging included): u32 [cap]"""
    global _BUFFERS
    if _BUFFERS is None:
        out, buf = [], np.zeros(0, np.uint32)
        for st in M.plan()[0]:
            out.append(buf.copy())
            buf = _mutate(st, buf, None)
            buf[:st.n_after] = doc_of(st.ids_after)
        _BUFFERS = out
    return _BUFFERS


def buffer_before(st):
    return _buffers()[st.index]


def _mutate(st, buf, fault):
    """the buffer after the step's mutation alone"""
    tag = fault[:2] if fault else ""
    n0, n = st.n_before, st.n_after
    if st.cap_after > st.cap_before:                              # a regrow: a new buffer, the live part copied
        new = np.full(st.cap_after, DOC_NONE, np.uint32)
        if tag != "C4":
            new[:n0] = buf[:n0]
        buf = new
    else:
        buf = buf.copy()
    if st.op == "upload":
        if tag != "C5":
            buf[:] = DOC_NONE                                     # the column goes with the old rows
    elif st.op == "append":
        if tag != "C3":
            buf[n0:n] = DOC_NONE
    elif st.op == "delete":
        keep = np.setdiff1d(np.arange(n0), st.dead)
        moved = buf[keep]
        if tag == "C1":
            moved = buf[:n].copy()
        elif tag == "C2":                                         # one row off from the first seam behind the first dead row
            seam = (st.first_changed // M.TILE + 1) * M.TILE
            if seam < n:
                moved[seam:] = buf[np.minimum(keep[seam:] + 1, n0 - 1)]
        buf[:n] = moved
    return buf


def tag_mode(st):
    """how the walker tags after this step: None (nothing to tag), "rows" (tag_rows over the appended tail) or "whole" (set_documents)"""
    if st.op == "upload":
        return "whole"
    if st.op != "append":
        return None
    appends = [s.index for s in M.plan()[0] if s.op == "append"]
    return ("rows", "whole")[appends.index(st.index) % 2]


def column_fault_applies(st, fault):
    return {"C1": st.op == "delete", "C2": st.op == "delete", "C3": st.op == "append" and st.cap_after == st.cap_before,
            "C4": st.cap_after > st.cap_before and st.n_before > 0, "C5": st.op == "upload" and st.index > 1}[fault[:2]]


def column(st, fault=None):
    """-> Column of the step; the buffer was right before it.  fault None: the library's documented rule."""
    n0, n = st.n_before, st.n_after
    buf = _mutate(st, buffer_before(st), fault)
    raw = buf[:n].copy()
    mode = tag_mode(st)
    if mode == "rows":
        buf[n0:n] = doc_of(st.ids_after[n0:])
    elif mode == "whole":
        buf[:n] = doc_of(st.ids_after)
    return Column(raw, buf[:n].copy(), mode)


# ---------------------------------------------------------------- probes
def select(st, base):
    """indices into the step's probe queries: the seam rows first, then a spread of the others, then the ordinary ones"""
    pos, f = base.positions, st.first_changed
    first = [p for p in ((f - 1, f, f + 1) if f is not None else ()) + (st.n_after - 1, st.n_before - 1)]
    chosen = [i for i, p in enumerate(pos) if p in first][:N_SELF]
    rest = [i for i in range(len(pos)) if i not in chosen]
    room = N_SELF - len(chosen)
    if room and rest:
        chosen += [rest[j] for j in np.unique(np.linspace(0, len(rest) - 1, min(room, len(rest))).astype(np.int64))]
    return np.array(sorted(chosen) + list(range(base.n_self, len(base.queries))), np.int64)


class StateProbes:
    """the probes of one (step, dtype): queries, their oracle scans over the mirror, the range pairs, the lexical lists;
    built once, shared by every configuration and test, never changed"""

    def __init__(self, O, st, dtype):
        base = M.step_probes(O, st, dtype)
        idx = select(st, base)
        self.st, self.dtype, self.n = st, dtype, st.n_after
        self.n_self = int((idx < base.n_self).sum())
        self.positions = base.positions[idx[:self.n_self]]
        self.queries, self.scores = base.queries[idx], base.scores[idx]
        self.docs = doc_of(st.ids_after)
        pairs = [(i, SELF_TAU) for i in range(self.n_self)]
        self.cases = ["self"] * self.n_self
        for i in range(self.n_self if self.n else 0):               # more hits than RANGE_CAPS[0]: the single entry's hand-off
            t = min(RANKS[1], max(self.n // 2, 1))
            pairs.append((i, np.sort(self.scores[i])[::-1][t - 1]))
            self.cases.append(f"self rank {RANKS[1]}")
        for i in range(self.n_self, len(idx)):
            s = np.sort(self.scores[i])[::-1]
            for r in RANKS if self.n else ():
                t = min(r, max(self.n // 2, 1))
                pairs += [(i, s[t - 1]), (i, np.nextafter(s[t - 1], F32(np.inf)))]
                self.cases += [f"rank {r}", f"above rank {r}"]
            if not self.n:
                pairs.append((i, SELF_TAU))
                self.cases.append("empty")
        self.pair_query = np.array([p[0] for p in pairs], np.int64)
        self.taus = np.array([p[1] for p in pairs], np.float32)
        self.range_queries = self.queries[self.pair_query]
        self.lex = [self._lex(i) for i in range(len(idx))]
        self._cache = {}
        for a in (self.queries, self.scores, self.docs, self.taus, self.range_queries):
            a.setflags(write=False)

    def _lex(self, i):
        """-> (rows u64 ascending, scores f32, max_lex): positions of pool ids that are live in the mirror"""
        ids = self.st.ids_after
        if i % 4 == 0:
            rows = np.zeros(0, np.int64)
        elif i % 4 == 1:
            rows = np.unique(self.positions)
        else:
            rows = np.flatnonzero(ids % 97 == (11 * i) % 97)
        scores = (0.25 + (ids[rows] * 37 % 64) / 16.0).astype(np.float32)
        return rows.astype(np.uint64), scores, float(CV.max_lex_of(scores))

    def mask(self, allowed):
        return None if allowed is None else R._allowed_mask(self.n, allowed)

    # -- the top-k hand-off of a single range query, as mutation_vectors.CopyModel.lost reads its probes -------------
    def groups(self):
        """[(query indices, k)]: a self-probe that asks its own rank-25 score at cap RANGE_CAPS[0] has more hits than
        cap, and the single entry answers with the top-k path at k = cap -- over the nomination copy that is on"""
        return [(np.arange(self.n_self), RANGE_CAPS[0])]

    def expected(self, qi, k, allowed=None):
        return M.oracle_topk(self.scores[qi], k, allowed)

    @staticmethod
    def _key(allowed):
        return None if allowed is None else np.asarray(allowed, np.int64).tobytes()

    # -- the definitions ---------------------------------------------------------------------------------------------
    def range_expect(self, cap, allowed=None):
        """[(rows u64, scores f32, n_total)] per range pair (cached by cap and the allowed set)"""
        ck = ("range", cap, self._key(allowed))
        if ck not in self._cache:
            out = []
            for qi, tau in zip(self.pair_query, self.taus):
                rows, total = R.expect(self.scores[qi], tau, cap, allowed)
                out.append((rows, self.scores[qi][rows.astype(np.int64)], total))
            self._cache[ck] = out
        return self._cache[ck]

    def grouped_expect(self, k, per_doc, docs=None, allowed=None):
        """[(rows u64, scores f32, docs u32)] per probe; docs None: the tagged column (cached, by the allowed set too)"""
        ck = ("grouped", k, per_doc, self._key(allowed))
        cached = docs is None
        if not cached or ck not in self._cache:
            d = self.docs if docs is None else np.asarray(docs, np.uint32)
            out = []
            for e in self.scores:
                rows = G.expect(e, d, k, per_doc, self.mask(allowed)) if self.n else np.zeros(0, np.uint64)
                out.append((rows, e[rows.astype(np.int64)], d[rows.astype(np.int64)]))
            if not cached:
                return out
            self._cache[ck] = out
        return self._cache[ck]

    def topk(self, k):
        return [M.oracle_topk(e, k)[0] for e in self.scores]

    def capped_expect(self, O, combo, docs=None, allowed=None):
        """[dict(rows, comb, cos, lexn, docs)] per probe, in answer order (pick order when diversified)"""
        need, per_doc, diversify, picks = combo
        ck = ("capped", combo, self._key(allowed))
        cached = docs is None
        if not cached or ck not in self._cache:
            d = self.docs if docs is None else np.asarray(docs, np.uint32)
            mirror = M.stored(O, self.dtype)
            out = []
            for i, e in enumerate(self.scores):
                lr, ls, ml = self.lex[i]
                pool = CV.define(e, d, lr, ls, W_E, W_L, need, per_doc, self.mask(allowed), max_lex=ml)
                if diversify and pool["rows"].size:
                    order, _ = O.mmr(mirror[self.st.ids_after[pool["rows"].astype(np.int64)]], pool["comb"], picks, LAM)
                    pool = {name: v[order] for name, v in pool.items()}
                out.append(pool)
            if not cached:
                return out
            self._cache[ck] = out
        return self._cache[ck]


_PROBES = {}


def state_probes(O, st, dtype="f32"):
    key = (st.index, dtype)
    if key not in _PROBES:
        _PROBES[key] = StateProbes(O, st, dtype)
    return _PROBES[key]


def chunks(n, size=8):
    return [np.arange(a, min(a + size, n)) for a in range(0, n, size)]


# ---------------------------------------------------------------- the forms the batched entries must report (sharing mode 2)
def range_batch_forms(dtype, n, nq, list_path=False):
    """range_share_path of index_grouped.hip at 256 columns: 2..8 queries over f32 rows share a scan at any row count; anything
    else of two or more shares the GEMM from 4096 rows on; the rest goes by rule"""
    out = [0, 0, 0, 0]
    if n == 0 or nq == 0:
        return out
    if nq < 2 or list_path:
        out[3] = nq
    elif nq <= 8 and dtype == "f32":
        out[0] = nq
    elif n >= M.BATCH_ROWS:
        out[1] = nq
    else:
        out[3] = nq
    return out


def chunk_forms(dtype, n, n_allowed, per_doc, nq, list_path=False):
    """the grouped and the capped batch at 256 columns: f32 rows share a scan in chunks of the workspace rule's width
    (grouped_batch_vectors.chunk_width, split) at any row count; binary16 rows have no shared scan"""
    if n == 0 or n_allowed == 0 or nq == 0:
        return [0, 0, 0, 0]
    if nq < 2 or list_path or dtype != "f32":
        return [0, 0, 0, nq]
    shared, lone = GB.forms_by_rule(nq, GB.chunk_width(n, M.DIM * 4, n_allowed, per_doc))
    return [shared, 0, 0, lone]


# ---------------------------------------------------------------- the collect of the grouped tail, vectorised
def collect_count(a, docs, k, per_doc, eps):
    """the number of candidates the grouped collect keeps for one query (grouped_batch_vectors' heads / collect and
    capped_batch_vectors.collect, without their loops): ranks inside the document by nominated score, t_g the
    per_doc-th, heads the top per_doc of every document and the untagged rows, U the floor of the 22-bit bin of the k-th
    head, candidates a >= max(t_g, U) - 2 eps in f32"""
    a = np.asarray(a, np.float32)
    n = a.size
    docs = np.asarray(docs, np.uint32)
    order = np.lexsort((np.arange(n), -a.astype(np.float64), docs))
    d_sorted = docs[order]
    start = np.r_[0, np.flatnonzero(d_sorted[1:] != d_sorted[:-1]) + 1]
    sizes = np.diff(np.r_[start, n])
    first_of = np.repeat(start, sizes)
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) - first_of
    tagged = docs != DOC_NONE
    # the per_doc-th row of every document that has one
    t_doc = np.where(sizes >= per_doc, a[order[np.minimum(start + per_doc - 1, n - 1)]], F32(-np.inf)).astype(np.float32)
    tg = np.empty(n, np.float32)
    tg[order] = np.repeat(t_doc, sizes)
    tg[~tagged] = -np.inf
    head = ~tagged | (rank < per_doc)
    hv = np.sort(a[head])[::-1]
    U = CV.bin_floor(hv[k - 1]) if hv.size >= k else F32(-np.inf)
    thr = (np.maximum(tg, U) - F32(2.0 * eps)).astype(np.float32)
    return int((~(a < thr)).sum())


# ---------------------------------------------------------------- faults seen through the range entries
def differs(got, want):
    """two lists of (rows, scores, n_total): the indices at which they differ"""
    return [i for i, (g, w) in enumerate(zip(got, want))
            if g[2] != w[2] or not np.array_equal(g[0], w[0]) or not np.array_equal(np.asarray(g[1], np.float32).view(np.uint32),
                                                                                   np.asarray(w[1], np.float32).view(np.uint32))]


def range_under_copy(model, sp, fault, cap=RANGE_CAPS[1]):
    """every range pair of the step in ONE call behind the GEMM over the image the fault leaves (range_batch_vectors.
    device_path, path "gemm": a row whose nomination lies below lo is no candidate) -> (answers, stale positions)"""
    st = sp.st
    data, scale = M.copy_after(st, "image", fault)
    nominated = model.nominate("image", data, scale, sp.range_queries).astype(np.float32)
    exact = sp.scores[sp.pair_query]
    out = RB.device_path(nominated, exact, EPS_IMAGE, sp.taus, cap, path="gemm")
    return [(r, c, t) for r, c, t, _ in out], [s for _, _, _, s in out], int(((data != st.ids_after) | (scale != st.ids_after)).sum())


def stride_fault_applies(st):
    return st.n_after > 0 and st.n_before > 0 and RB.stride_of(st.n_before) != RB.stride_of(st.n_after)


def range_under_stride(sp, sel, cap, stride_read):
    """the range pairs `sel` (2..8) behind the shared scan whose collect reads query q's scores `stride_read` floats
    apart while the pass wrote them stride_of(n) apart: candidates from what it reads, membership on the exact score"""
    n, nq = sp.n, len(sel)
    stride = RB.stride_of(n)
    flat = np.zeros(nq * max(stride, stride_read) + n, np.float32)
    exact = sp.scores[sp.pair_query[sel]]
    for q in range(nq):
        flat[q * stride:q * stride + n] = exact[q]
    out = []
    for q in range(nq):
        a = flat[q * stride_read:q * stride_read + n]
        lo, _ = R.bounds(sp.taus[sel][q], F32(2.0) * F32(EPS_SCAN))
        with np.errstate(invalid="ignore"):
            cand = np.flatnonzero(~(a < lo))
            rows = cand[exact[q][cand] >= sp.taus[sel][q]]
        rows = rows[R.result_order(exact[q][rows], rows)]
        out.append((rows[:cap].astype(np.uint64), exact[q][rows[:cap]], int(rows.size)))
    return out
