#!/usr/bin/env python3
"""Host work per align pass, where it shows: one small batch (10 000 reads of
150 bp against 10 x 200 kb genomes, k = 31), pa_align called 200 times after a
warm-up; prints the median per call with the counters fetched and of the
enqueue alone, in microseconds, as one JSON line.

    [PA_LIBRARY=<libpa.so>] python scripts/small_batch.py
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)
import pa_native as N  # noqa: E402
import synth  # noqa: E402

gens = synth.family_genomes_fast(10, 200000, seed=5, family_size=5, sub_rate=0.01, conserved_len=2000)
index = N.Index(gens, 31)
reads = N.Reads.synthesize(index, 10000, 150, seed=3, sub_rate=0.005)
res = N.Result(index)
prm = N.Params.make()
for _ in range(20):
    N.align(index, reads, prm, 0, res)
    res.fetch()
full, enq = [], []
for _ in range(200):
    t0 = time.perf_counter()
    N.align(index, reads, prm, 0, res)
    t1 = time.perf_counter()
    res.fetch()
    t2 = time.perf_counter()
    enq.append(t1 - t0)
    full.append(t2 - t0)
stats = res.fetch()[0]


def q(v, p):
    return round(float(np.percentile(np.array(v) * 1e6, p)), 2)


print(json.dumps({"library": os.path.basename(os.environ.get("PA_LIBRARY", "libpa.so")), "reads": 10000, "calls": 200,
                  "call_us_median": q(full, 50), "call_us_p25": q(full, 25), "call_us_p75": q(full, 75),
                  "enqueue_us_median": q(enq, 50), "enqueue_us_p25": q(enq, 25), "enqueue_us_p75": q(enq, 75),
                  "stats_last": [int(x) for x in stats]}))
