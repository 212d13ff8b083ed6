"""The guard-band corpora (band_vectors.py) checked without a GPU: the oracle's strict scan ranks X where the builder says,
a binary64 model of each path's nomination ranks every decoy above X, and the distance between them is the stated
fraction of the path's band -- far enough that a band of half (or a quarter of) the width loses X.  The bands are written
out here from DESIGN.md section 4 and the comments of nomination_eps (gemm.hip) and q8_two_eps / q8_arith_eps (index.hip,
q8.hip); nothing is read from the library.  Each test prints the fractions it measured (pytest -s shows them).

Measured fractions of the band (smallest .. largest decoy gap; in brackets the part of the band the device needs to
reach X from the bin floor below the best decoy):
  (a) f32 / binary16 rows   128-d 0.305..0.308 [0.26]   768-d 0.347..0.432 [0.41]   1024-d 0.376..0.440 [0.42]
                            1536-d 0.406..0.449 [0.43]
  (b) f32 rows 0.508..0.521 [0.43]        (b) binary16 rows 0.419..0.476 [0.39]        (c) 0.991..0.995 [0.99]"""
import numpy as np
import pytest

import band_vectors as V
from conftest import bits

KS = (1, 10, 100)
ABSORPTION_SHAPES = ((768, 4096, V.N_DECOYS), (128, 1024, 2), (1024, 1024, V.N_DECOYS), (1536, 1024, V.N_DECOYS))


# ---------------------------------------------------------------- the bands, as specified
def scan_band(dim):
    """f32 scans: 2 eps, eps = (dim + 64) * 2^-24 * 1.0625 for unit-norm operands"""
    return 2.0 * (dim + 64) * 2.0 ** -24 * 1.0625


def binary16_band(dim, f16_rows):
    """binary16 nomination: operand rounding 2^-10 (both operands; 2^-11 when the rows are binary16 already) * 1.001, the
    MFMA chain's and the reference's accumulation (dim + 64) * 2^-24 each, the subnormal term 2^-25 sqrt(dim) * (norm sum
    = 2), all * 1.0625"""
    op = 2.0 ** -11 if f16_rows else 2.0 ** -10
    return 2.0 * ((op * 1.001 + 2.0 * (dim + 64) * 2.0 ** -24) * 1.0 + 2.0 ** -25 * np.sqrt(dim) * 2.0) * 1.0625


def q8_band(dim, delta_max, scale_max, query_norm):
    """8-bit copy: 2 * (delta_max * |q| + arith + eps_scan); delta_max = the largest |x - s k| rounded up by 1.001, |q|
    rounded up by 1.0001, arith = 32 roundings * 2^-24 * 256 sqrt(dim) |q| * the largest row scale * 1.0625"""
    qn = query_norm * 1.0001 + 1e-30
    arith = 32.0 * 2.0 ** -24 * 256.0 * np.sqrt(dim) * qn * scale_max * 1.0625
    return 2.0 * (delta_max * 1.001 * qn + arith + 0.5 * scan_band(dim)), arith


# ---------------------------------------------------------------- the common proof
def rank_of(e, row):
    order = np.lexsort((np.arange(len(e)), -e.astype(np.float64)))
    return int(np.flatnonzero(order == row)[0]) + 1


def prove(oracle, name, rows, q, f, nominated, band):
    """-> (smallest, largest) decoy gap as a fraction of the band, after asserting every fact the GPU test relies on"""
    k, x, D = f["k"], f["x"], f["decoys"]
    assert len(D) >= 150
    assert f["norm_product"] <= 1.0001 and f["norm_sum"] <= 2.0001, (name, f["norm_product"], f["norm_sum"])
    e = oracle.scan(rows, q)
    assert rank_of(e, x) == k, (name, k, rank_of(e, x))
    assert (e[D] < e[x]).all(), name                          # every decoy's exact score is below X's ...
    assert (e[D] > np.delete(e, np.r_[x, D, f["champions"]]).max()).all(), name      # ... and above all the filler
    gaps = nominated[D] - nominated[x]
    assert int((gaps > 0).sum()) >= max(k, 150), name         # every decoy nominates above X
    # the bin floor the device collects from lies between X and the best decoy
    assert nominated[x] < f["edge"] < nominated[D].max(), name
    assert V.bin_floor(nominated[D].max()) == f["edge"], name
    need = (f["edge"] - nominated[x]) / band
    lo, hi = gaps.min() / band, gaps.max() / band
    # mutation facts: the full band keeps X; half of it, or a quarter where half still covers the gap, loses X
    cut = 0.5 if hi > 0.5 and need > 0.5 else 0.25
    for bins in (True, False):
        assert x in V.select(nominated, e, k, band, bins), (name, "the full band must keep X")
        got = V.select(nominated, e, k, band * cut, bins)
        assert x not in got and set(got) <= set(D) | set(f["champions"]), (name, cut, bins)
    assert x not in V.select(nominated, e, k, 0.0)
    print(f"{name} k={k}: decoys {lo:.3f}..{hi:.3f} of the band {band:.4g}; from the bin floor {need:.3f}; "
          f"lost at {cut} of the band")
    return lo, hi


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("dim,n,span", ABSORPTION_SHAPES, ids=lambda v: str(v))
def test_absorption_rows_reach_the_scan_band(oracle, dim, n, span, f16):
    for k in KS:
        rows, qs, f = V.absorption(oracle, k, dim, n, f16, span)
        q = qs[0]
        assert rows.shape == (n, dim)
        if f16:
            assert np.array_equal(bits(rows), bits(oracle.round_f16(rows)))      # the rows are binary16 values
        else:
            assert np.array_equal(bits(oracle.normalize(f["raw_query"])), bits(q))
        # the construction itself: the reference adds one ulp per term of X and of D's large terms, nothing else
        e = oracle.scan(rows, q)
        lead = np.float32(f["lead"])
        assert e[f["x"]] == np.float32(float(lead) + (dim - 1) * V.ULP)
        want_d = (float(lead) + (dim - 1 - f["drops"]) * V.ULP).astype(np.float32)
        assert np.array_equal(bits(e[f["decoys"]]), bits(want_d))
        lo, hi = prove(oracle, f"(a) absorption {dim}-d {'f16' if f16 else 'f32'}", rows, q, f, V.true_dot(rows, q),
                       scan_band(dim))
        assert lo >= 0.30


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_operand_rounding_rows_reach_the_binary16_band(oracle, f16):
    for k in KS:
        rows, qs, f = V.operand_rounding(oracle, k, f16)
        q = qs[0]
        r16, q16 = oracle.round_f16(rows), oracle.round_f16(q)
        assert np.array_equal(bits(V.to_f16(rows)), bits(r16))                  # numpy's rounding is the oracle's
        if f16:
            assert np.array_equal(bits(rows), bits(r16))
        # direction of every rounding: the query down on M and up on P, X down, the decoys up (f32 rows)
        M, P = f["M"], f["P"]
        assert (q16[M] < q[M]).all() and (q16[P] > q[P]).all()
        if not f16:
            assert (r16[f["x"], M] < rows[f["x"], M]).all()
            assert ((r16[f["decoys"]][:, P] > rows[f["decoys"]][:, P]).sum(axis=1) >= len(P) - 1).all()
        lo, hi = prove(oracle, f"(b) operand rounding {'f16' if f16 else 'f32'} rows", rows, q, f, V.true_dot(r16, q16),
                       binary16_band(768, f16))
        # f32 rows: the issue's floor.  binary16 rows: 0.9 x the 0.419 measured here
        assert lo >= (0.377 if f16 else 0.40)


# ---------------------------------------------------------------- (c)
def test_q8_rows_reach_the_8_bit_band(oracle):
    for k in KS:
        rows, qs, f = V.q8_rounding(oracle, k)
        q = qs[0]
        deq, delta, scale = V.q8_model(rows)
        x, D = f["x"], f["decoys"]
        assert scale[x] == np.float32(V.Q8_STEP) and (scale[D] == np.float32(V.Q8_STEP)).all()
        assert int(np.argmax(delta)) in set(D) | {x}            # X or a decoy owns the index's delta_max
        assert delta[x] > 5.0 * np.delete(delta, np.r_[x, D]).max()
        # Cauchy-Schwarz with equality for X but for the pinned element, which has no error: q . e = |q| |e| sqrt(767 / 768)
        err = rows[x].astype(np.float64) - deq[x]
        cs = float(q.astype(np.float64) @ err) / (np.linalg.norm(q.astype(np.float64)) * delta[x])
        assert abs(cs - np.sqrt(767.0 / 768.0)) < 1e-6
        band, arith = q8_band(768, delta.max(), float(scale.max()), f["query_norm"])
        lo, hi = prove(oracle, "(c) 8-bit copy", rows, q, f, deq @ q.astype(np.float64), band)
        assert lo >= 0.89                                       # 0.9 x the 0.991 measured here
        print(f"    of which the arithmetic term {arith / (band / 2):.4f} and the scan term "
              f"{0.5 * scan_band(768) / (band / 2):.4f} of eps")


def test_engine_corpus_puts_x_on_the_pool_boundary(oracle):
    """the corpus test_gpu_guard_bands.py gives the engine: X is the last of the 30 stage-1 candidates of top_k = 10 and the
    last row of the 30-row MMR pool, and the diversified result holds it"""
    rows, qs, f = V.absorption(oracle, 30)
    raw = f["raw_query"]
    assert oracle.search(rows, raw, 10, stage=1)[0][-1] == f["x"]
    assert oracle.search(rows, raw, 30)[0][-1] == f["x"]
    assert f["x"] in oracle.search_with_diversity(rows, raw, 10, 0.7)[0]
