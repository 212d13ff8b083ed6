"""Concurrent single-query searches with coalescing off and on (rlr_index_set_coalescing).

    python tools/bench_concurrent.py [--rows 10000000] [--dim 768] [--seconds 1.5] [--reps 2] [--out FILE]

Caller threads issue rlr_search_topk calls with one query each (ctypes releases the GIL for the call), as the
reference's tokio workers do under the read lock.  For each index (f32, then binary16 rows; filled on the device by
rlr_index_fill_synthetic) and each thread count (1, 2, 4, 8, 16), coalescing is switched off and on in turn, `reps`
times each, every period after a warm-up; then rlr_engine_search_with_diversity (top_k 10, lambda 0.3) at 8 threads the
same way.  Reported per configuration: aggregate queries/s, p50 / p99 per call, the coalescer's group-size histogram,
and (coalescing on, 8 threads, one extra profiled period) where a shared pass spends its time.  One JSON line on stdout.
"""
from __future__ import annotations

import argparse
import ctypes as C
import importlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THREADS = (1, 2, 4, 8, 16)


def load():
    return importlib.import_module("rust-local-rag_amd")


def run_period(call, n_threads, seconds, warmup_s):
    """n_threads callers run call(thread, i) back to back; per-call latencies of the measured window"""
    stop_warm = time.perf_counter() + warmup_s
    stop = stop_warm + seconds
    lat = [[] for _ in range(n_threads)]
    barrier = threading.Barrier(n_threads)
    errs = []

    def body(t):
        try:
            barrier.wait()
            i = 0
            while True:
                t0 = time.perf_counter()
                if t0 >= stop:
                    break
                call(t, i)
                t1 = time.perf_counter()
                if t0 >= stop_warm:
                    lat[t].append(t1 - t0)
                i += 1
        except BaseException as e:  # noqa: BLE001 -- reported below
            errs.append(repr(e))

    ts = [threading.Thread(target=body, args=(t,)) for t in range(n_threads)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    if errs:
        raise RuntimeError(errs[0])
    all_lat = np.array([x for per in lat for x in per])
    return {"qps": round(len(all_lat) / seconds, 1), "calls": int(len(all_lat)),
            "p50_ms": round(float(np.percentile(all_lat, 50)) * 1e3, 3) if len(all_lat) else None,
            "p99_ms": round(float(np.percentile(all_lat, 99)) * 1e3, 3) if len(all_lat) else None}


def merge(periods):
    """several periods of one configuration: queries/s averaged, percentiles of the worst period"""
    return {"qps": round(sum(p["qps"] for p in periods) / len(periods), 1),
            "qps_each": [p["qps"] for p in periods],
            "p50_ms": max(p["p50_ms"] for p in periods), "p99_ms": max(p["p99_ms"] for p in periods)}


def bench_index(rlr, dtype, rows, dim, k, seconds, reps, warmup_s, threads=THREADS, linger_us=0):
    L = rlr.lib()
    ix = rlr.GpuIndex(dim, dtype)
    ix.fill_synthetic(rows, seed=20261016, n_clusters=64)
    rng = np.random.default_rng(7)
    qs = rng.standard_normal((512, dim)).astype(np.float32)
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    bufs = {}

    def topk(t, i):
        if t not in bufs:
            bufs[t] = (np.zeros(k, np.uint64), np.zeros(k, np.float32), np.zeros(1, np.uint32))
        r, c, n = bufs[t]
        q = qs[(t * 131 + i) % len(qs)]
        st = L.rlr_search_topk(ix.handle, q.ctypes.data_as(rlr._native.f32p), 1, k, -1.0,
                               r.ctypes.data_as(rlr._native.u64p), c.ctypes.data_as(rlr._native.f32p),
                               n.ctypes.data_as(rlr._native.u32p))
        if st != 0:
            raise RuntimeError(f"rlr_search_topk -> {st}")

    out = {"dtype": dtype, "rows": rows, "dim": dim, "k": k, "threads": {}}
    for nt in threads:
        res = {"off": [], "on": []}
        hist = [0] * 9
        for _ in range(reps):
            for mode in ("off", "on"):
                ix.set_coalescing(8 if mode == "on" else 0, linger_us)
                ix.coalesce_stats(reset=True)
                res[mode].append(run_period(topk, nt, seconds, warmup_s))
                if mode == "on":
                    st = ix.coalesce_stats()
                    hist = [a + b for a, b in zip(hist, st["group_size"])]
                    res.setdefault("solo", 0)
                    res["solo"] += st["n_solo"]
                    res.setdefault("handed_back", 0)
                    res["handed_back"] += st["n_handed_back"]
        ix.set_coalescing(0)
        off, on = merge(res["off"]), merge(res["on"])
        out["threads"][str(nt)] = {"off": off, "on": on, "speedup": round(on["qps"] / off["qps"], 3),
                                   "group_size_hist": hist, "n_solo": res.get("solo", 0),
                                   "n_handed_back": res.get("handed_back", 0)}
    # where a shared pass of 8 spends its time: one profiled period (HIP events around each stage; not in the rates above)
    ix.set_coalescing(8, linger_us)
    ix.profile_enable(True)
    ix.profile_read(reset=True)
    ix.coalesce_stats(reset=True)
    run_period(topk, 8, seconds, warmup_s)
    p = ix.profile_read()
    st = ix.coalesce_stats()
    ix.profile_enable(False)
    ix.set_coalescing(0)
    nb = max(p.n_batches, 1)
    out["profiled_8_threads"] = {
        "passes": p.n_batches, "queries": p.n_batch_queries,
        "shared_scan_ms_per_pass": round(p.batch_gemm_ms / nb, 4),
        "select_and_finish_ms_per_pass": round(p.batch_other_ms / nb, 4),
        "scan_gbps": round(p.batch_gemm_bytes / max(p.batch_gemm_ms, 1e-9) / 1e6, 1),
        "solo_calls": st["n_solo"], "solo_scan_ms_per_call": round(p.scan_ms / max(p.n_scan_launches, 1), 4),
        "group_size_hist": st["group_size"],
    }
    return ix, qs, out


def bench_engine(rlr, ix, qs, dim, seconds, reps, warmup_s, linger_us=0):
    L = rlr.lib()
    N = rlr._native
    bufs = {}

    def div(t, i):
        if t not in bufs:
            bufs[t] = ((N.SearchHitC * 64)(), C.c_uint32())
        hits, n = bufs[t]
        q = qs[(t * 131 + i) % len(qs)]
        st = L.rlr_engine_search_with_diversity(ix.handle, q.ctypes.data_as(N.f32p), dim, 10, 0.3, None, None, None, 0,
                                                hits, 64, C.byref(n))
        if st != 0:
            raise RuntimeError(f"rlr_engine_search_with_diversity -> {st}")

    res = {"off": [], "on": []}
    handbacks = 0
    for _ in range(reps):
        for mode in ("off", "on"):
            ix.set_coalescing(8 if mode == "on" else 0, linger_us)
            ix.coalesce_stats(reset=True)
            res[mode].append(run_period(div, 8, seconds, warmup_s))
            handbacks += ix.coalesce_stats()["n_engine_handbacks"]
    ix.set_coalescing(0)
    off, on = merge(res["off"]), merge(res["on"])
    return {"call": "rlr_engine_search_with_diversity", "top_k": 10, "lambda": 0.3, "threads": 8, "off": off, "on": on,
            "speedup": round(on["qps"] / off["qps"], 3), "n_engine_handbacks": handbacks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--warmup", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--linger", type=int, default=0, help="linger_us of rlr_index_set_coalescing")
    ap.add_argument("--threads", default=",".join(map(str, THREADS)), help="caller thread counts")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rlr = load()
    if rlr.device_count() < 1:
        raise SystemExit("bench_concurrent needs a GPU")
    result = {"tool": "bench_concurrent", "max_group": 8, "linger_us": a.linger, "indexes": []}
    for dt in a.dtypes.split(","):
        ix, qs, out = bench_index(rlr, dt, a.rows, a.dim, a.k, a.seconds, a.reps, a.warmup,
                                  tuple(int(t) for t in a.threads.split(",")), a.linger)
        if dt == "f32":
            out["engine_diversity"] = bench_engine(rlr, ix, qs, a.dim, a.seconds, a.reps, a.warmup, a.linger)
        ix.close()
        result["indexes"].append(out)
        print(f"# {dt}: " + ", ".join(f"{t}T off {v['off']['qps']} on {v['on']['qps']}" for t, v in out["threads"].items()),
              file=sys.stderr, flush=True)
    line = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
