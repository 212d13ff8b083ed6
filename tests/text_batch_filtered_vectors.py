"""Designed inputs of the batched text search inside a document scope (rlr_lexical_score_batch_filtered,
rlr_engine_search_text_batch_filtered), shared by tests/test_text_batch_filtered_cpu.py -- which clears every engine vector
on the CPU: the oracle alone must show that no query can be handed back -- and the two GPU test modules."""
import numpy as np

# ---- the engine call --------------------------------------------------------------------------------------------------
# corpora: the 1500-chunk, 12-document recipe of test_gpu_filter_engine.Corpus (DOC_LENGTHS, make_texts, synth_rows)
CORPORA = {"f32_768": (768, "f32", 11), "f32_256": (256, "f32", 12), "f32_1024": (1024, "f32", 13), "f16_1024": (1024, "f16", 31)}
DOC_LENGTHS = [1, 7, 64, 65, 200, 3, 128, 31, 300, 90, 411, 200]
SCOPES = [["doc4.pdf"], ["doc2.pdf", "doc8.pdf", "doc10.pdf"], [f"doc{d}.pdf" for d in range(12)], ["no-such.pdf"],
          ["doc3.pdf", "no-such.pdf"], []]
WEIGHTS = [(None, 0.7, 0.3), (dict(embedding=0.0, lexical=1.0), 0.0, 1.0), (dict(embedding=1.0, lexical=0.0), 1.0, 0.0)]
# (lambda, stage): `stage` only reaches search(), the lambda == 0 branch
MODES = [(0.0, 0), (0.0, 1), (0.3, 0), (1.0, 0)]
TOP_KS = [1, 7, 12]
# shared-pass instances with zeroed slots (2, 3, 5), a full one (8), a last chunk of one (9, 17), more than two chunks (17)
BATCHES = [2, 3, 5, 8, 9, 17]
# mixed within a batch: known and unknown words, a repeated word, an empty text, punctuation the tokenizer drops
TEXTS = ["w000x w001x common", "w017x frequent the", "", "w005x w006x w007x w008x w009x w010x", "the of", "zzunknown qqunknown",
         "w005x w005x, w040x;", "common frequent the of w000x w001x w002x"]
QUERY_SEED0 = 900  # query i of a batch: oracle.synth_query(dim, QUERY_SEED0 + i), text TEXTS[(i + shift) % len(TEXTS)]


def batch_texts(n, shift):
    return [TEXTS[(i + shift) % len(TEXTS)] for i in range(n)]


def engine_grid(corpus):
    """(scope index, weights index, lambda, stage, top_k, batch size, text shift) -- the full product on the 768-d corpus with the
    batch size and the texts rotating through it; the other widths and binary16 rows: what differs there is the cosine side"""
    out, i = [], 0
    if corpus == "f32_768":
        for s in range(len(SCOPES)):
            for wi in range(len(WEIGHTS)):
                for lam, stage in MODES:
                    for k in TOP_KS:
                        out.append((s, wi, lam, stage, k, BATCHES[i % len(BATCHES)], i % len(TEXTS)))
                        i += 1
    else:
        for s in (0, 1, 2, 4):
            for lam, stage in ((0.0, 1), (0.3, 0)):
                for n in (3, 9):
                    out.append((s, 0, lam, stage, 7, n, i % len(TEXTS)))
                    i += 1
    return out


def sizes(n_allowed, top_k, lam, stage):
    """(k_seen, BM25 limit, need) as rlr_engine_search_text_filtered computes them for a scope of n_allowed rows"""
    k_seen = max(top_k, 1) if lam == 0.0 else max(3 * top_k, top_k + 10)
    initial_k = min(n_allowed, 3 * k_seen)
    need = initial_k if (lam == 0.0 and stage) else min(initial_k, k_seen)
    return k_seen, min(5 * k_seen, 8192), need


# ---- the lexical call -------------------------------------------------------------------------------------------------
LEX_ROWS = 4200      # two full 2048-row slices of the accumulate kernel and a partial one
SMALL_INDEX = 4100   # an embedding index smaller than the lexical one: index_rows inside a slice and inside a mask word
LIMITS = [1, 5, 150, 8192]
# ("w000x" .. "w004x" are in more than half of the rows: idf 0, they score nothing; BROAD hits nine rows in ten)
BROAD = "w005x w006x w007x w008x w009x w010x w011x w012x"
LEX_TEXTS = [BROAD, "w017x w101x", "", "unknown words only", "the of", BROAD, "w399x w250x w250x w003x", "common w000x", "frequent w002x"]
MANY_TERMS = " ".join(f"w{i:03d}x" for i in range(129))   # 129 unique known terms: the single path (n_single = 1)


def lex_masks(n, texts=None):
    """name -> allowed rows of an n-row index (n >= 4200); texts: the rows' texts -- the one row is then the first row from
    the last row of slice 0 on that holds "w017x" (a row the second query hits), else that last row itself"""
    one = 2047
    if texts is not None:
        one = next(r for r in range(2047, n) if "w017x" in texts[r].split())
    return {
        "none": np.arange(0),
        "every_row": np.arange(n),
        "one_row": np.array([one]),
        "word_edge": np.array([63, 64]),
        "slice_edge": np.arange(2040, 2061),
        "slice_masked": np.concatenate([np.arange(0, 2048), np.arange(4096, n)]),
        "every_other": np.arange(n)[::2],
    }


def lex_batch(n):
    """n query texts: LEX_TEXTS in turn (an empty text, unknown words only and a repeated query among the first six)"""
    return [LEX_TEXTS[i % len(LEX_TEXTS)] for i in range(n)]
