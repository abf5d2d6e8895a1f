#!/usr/bin/env python3
"""Cost of a coverage pass on the C2 configuration (bench.py's: 50 x 2 Mbp
genomes, k = 31, synthesized 150-bp reads, 0.5 % substitutions).

    python scripts/coverage_rate.py --mode detail   [--reads N] [--runs R] > parent.json
    python scripts/coverage_rate.py --mode coverage [--reads N] [--runs R] [--baseline-json parent.json]
    python scripts/coverage_rate.py --mode assign   [--reads N] [--runs R] [--read-err E --rc-rate X --foreign-rate Y]
    python scripts/coverage_rate.py --mode bootstrap [--reads N] [--runs R] [--replicates B]
    python scripts/coverage_rate.py --mode lineage  [--reads N] [--runs R]
    python scripts/coverage_rate.py --mode containment [--reads N] [--runs R]
    python scripts/coverage_rate.py --mode trim     [--reads N] [--runs R]

--mode detail times one pa_align_detail call with its lists (the pass a
coverage add rides on); run it with PA_LIBRARY=<the parent commit's libpa.so>
PA_LIBRARY_PARTIAL=1 for the baseline, so that the ratio is never the new code
against itself.  --mode coverage times the same call on this library
(align_detail_branch_s), the positions view's build (and reports its bytes)
and pa_coverage_add with the view in place; with --baseline-json, the line of
a --mode detail run, it adds that run's figures (align_detail_parent_s,
parent_library) and ratio_coverage_add_over_align_detail = coverage_add_s /
align_detail_parent_s, so the record is one line of one command.  Every figure
is the median of --runs timed calls after one warm-up call; all calls return
when the device is done, so wall time is device time plus the call's own host
work.  One JSON line on stdout.

--mode assign times one pa_align_reads call (the assign pass, DESIGN.md section
11: types, counters, offsets and lists of every read in one call with room for
one list entry per read) next to pa_align_detail on the same library, and adds
the kernels' own times over profiled_calls such calls (pa_profile_read_kernels)
and the counter pass (pa_align + fetch) on the same batch.  --mode coverage rides the assign pass since
pa_coverage_add classifies through it (PA_ASSIGN=0: the exact pass, as before).
--mode pileup times pa_pileup_add next to pa_coverage_add
and pa_align_reads on the same library and batch, with the positions view in
place: the three share the assign pass, the two adds share k_place, so
coverage_add_s - align_reads_s bounds k_place (plus the depth atomics) and
pileup_add_s - coverage_add_s is k_pileup's cost over those atomics.  It adds
the align kernels' own times over profiled pileup adds, pa_pileup_variants over
the whole reference (its two passes and the copy of the records), and the stats.

--mode abundance times pa_abundance_add next to
pa_align_reads, pa_align_candidates, pa_coverage_add and pa_align_detail with
its lists on the same library and batch.  The add is the assign pass, the
candidate kernel over the ambiguous reads and the interning, and
pa_align_candidates is the first two plus the copy of the sets to the host, so
align_candidates_s - align_reads_s bounds the candidate kernel's two passes
from above and abundance_add_s - align_reads_s the candidate kernel plus the
interning.  It adds the align kernels' own times over one profiled add, the
accumulator's info (reads by type, classes) and pa_abundance_estimate for 200
iterations (tolerance 0) and with the default tolerance.

--mode bootstrap adds the reads once and times pa_abundance_bootstrap (DESIGN.md
section 16) at --replicates B (default 100), seed 1: 200 iterations with
tolerance 0 and with the default tolerance, each also under PA_BOOT_LDS=0, and
next to each one pa_abundance_estimate with the same settings.  The yardstick
is B x that estimate -- what a loop over pa_abundance_estimate would cost, with
no resampling at all -- so ratio_*_over_B_estimates is the call's time over it.
The draw / EM split comes from a kernel trace of this mode.

--mode lineage times pa_lineage_add next to pa_align_reads
and pa_abundance_add on the same batch, under a tree whose species are the
genome families, with and without the node array and under PA_LINEAGE_LDS=0
(global atomics instead of the LDS histogram).  With PA_LIBRARY naming the
parent's library (and PA_LIBRARY_PARTIAL=1), which has no pa_lineage_*, the
line holds the two yardsticks only.

--mode containment times pa_containment_add next to
pa_align_reads and pa_align_detail with its lists on the same batch: the first
add on clear bits, then the median of the later ones, the same under
PA_CONTAIN_LDS=0, and the reduction (pa_containment_counts, and
pa_containment_nodes under --mode lineage's tree).  One add runs with
PA_CONTAIN_STATS=1: the library prints the atomic ORs issued so far to stderr.

--mode pairs times pa_align_pairs on a both-strand C2
index: --reads pairs (default 1 000 000) made on the host -- fragments of 300 ..
500 bases, mates of 150, mate 2 the reverse complement of the fragment's last
150, --read-err substitutions -- and uploaded as two batches.  Next to it the
same call under PA_PAIR_COMBINE=0 (every pair to the pair-exact kernel),
pa_align_reads over mates 1 plus over mates 2 (the mates' pass the call rides
on), pa_align_detail with its lists over the 2 N mates, and the call without a
result (the difference is k_pair_count and the fetch-free counter pass).

--mode trim times pa_reads_trim next to pa_align (the
counter pass it stands in front of) and pa_align_reads on the same batch: the
C2 reads downloaded, given qualities and planted adapters on the host by the
recipe of tests/test_gpu_trim.py (an eighth each: clean, dim; bad 3' tail; bad
5' head; two eighths an adapter at a random insert, half with a substitution;
an adapter with four substitutions; all bad) and uploaded again, so that the
pass really trims.  With PA_TRIM_TIMING=1 the library prints the split of
every call (bounds kernel, offset scan, gather kernel) on stderr.

--read-err / --rc-rate / --foreign-rate give bench.py's c2mix reads (0.015, 0.2, 0.2).
"""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bioinformatics-project-for-shotgun-metagenomics-pseudo-alignment-shotgun-_amd"))

import numpy as np  # noqa: E402

import pa_native as N  # noqa: E402
import synth  # noqa: E402


def timed(fn, runs):
    fn()  # warm-up
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def time_detail(index, reads, prm, runs):
    """(median, runs, list entries) of pa_align_detail with its lists."""
    n = reads.n
    types = np.zeros(n, dtype=np.uint8)
    qf = np.zeros(n, dtype=np.uint32)
    hr = np.zeros(n, dtype=np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64)
    total = N.U64(0)
    N._check(N.lib().pa_align_detail(index.handle, reads.handle, ctypes.byref(prm), N._ptr(types), N._ptr(qf),
                                     N._ptr(hr), N._ptr(off), None, 0, ctypes.byref(total), None))
    lists = np.zeros(max(int(total.value), 1), dtype=np.uint32)

    def detail():
        N._check(N.lib().pa_align_detail(index.handle, reads.handle, ctypes.byref(prm), N._ptr(types),
                                         N._ptr(qf), N._ptr(hr), N._ptr(off), N._ptr(lists), lists.size,
                                         ctypes.byref(total), None))
    med, ts = timed(detail, runs)
    return med, ts, int(total.value)


def time_assign(index, reads, prm, runs):
    """(median, runs, list entries) of one pa_align_reads call with its lists
    (room for one entry per read; a longer total is learnt by a first call)."""
    n = reads.n
    types = np.zeros(n, dtype=np.uint8)
    qf = np.zeros(n, dtype=np.uint32)
    hr = np.zeros(n, dtype=np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64)
    total = N.U64(0)
    lists = np.zeros(max(n, 1), dtype=np.uint32)

    def call():
        return N.lib().pa_align_reads(index.handle, reads.handle, ctypes.byref(prm), N._ptr(types), N._ptr(qf),
                                      N._ptr(hr), N._ptr(off), N._ptr(lists), lists.size, ctypes.byref(total), None)
    st = call()
    if st == N.PA_EINVAL and total.value > lists.size:
        lists = np.zeros(int(total.value), dtype=np.uint32)
        st = call()
    N._check(st)
    med, ts = timed(lambda: N._check(call()), runs)
    return med, ts, int(total.value)


TRUSEQ = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


def make_trim_batch(reads, seed=22, chunk=1_000_000):
    """The batch's columns with the trim test's kinds of reads (read r is of kind r % 8), made chunk by
    chunk on the host; every read keeps its length L."""
    seq, qual, off = reads.download()
    n, L = reads.n, reads.max_len
    seq, qual = seq.reshape(n, L).copy(), qual.reshape(n, L).copy()
    rng = np.random.default_rng(seed)
    cols = np.arange(L)
    adapter = np.frombuffer(TRUSEQ, dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        kind = np.arange(a, b) % 8
        q = rng.integers(60, 74, (b - a, L), dtype=np.uint8)
        bad = rng.integers(35, 51, (b - a, L), dtype=np.uint8)
        at = rng.integers(0, L, b - a)
        low = ((kind == 1)[:, None] & (cols[None, :] >= at[:, None])) | \
              ((kind == 2)[:, None] & (cols[None, :] < (1 + at // 2)[:, None])) | (kind == 6)[:, None]
        q[low] = bad[low]
        dim = kind == 7
        q[dim] = rng.integers(56, 60, (int(dim.sum()), L), dtype=np.uint8)
        qual[a:b] = q
        s = seq[a:b]
        rows = np.flatnonzero((kind == 3) | (kind == 4) | (kind == 5))
        p = np.where(kind[rows] == 5, rng.integers(0, L - len(adapter) + 1, rows.size), at[rows])
        ad = np.broadcast_to(adapter, (rows.size, len(adapter))).copy()
        subs = np.where(kind[rows] == 5, 4, (rows % 2))  # (four: one over the three a whole adapter may hold)
        for j in range(4):
            hit = np.flatnonzero(subs > j)
            where = (rng.integers(0, 8, hit.size) + 8 * j) % len(adapter)
            ad[hit, where] = acgt[(np.searchsorted(acgt, ad[hit, where]) + rng.integers(1, 4, hit.size)) % 4]
        junk = acgt[rng.integers(0, 4, (rows.size, L))]
        c = cols[None, :] - p[:, None]
        tail = c >= 0
        body = tail & (c < len(adapter))
        s[rows[:, None], cols[None, :]] = np.where(body, ad[np.arange(rows.size)[:, None], np.clip(c, 0, len(adapter) - 1)],
                                                   np.where(tail & (kind[rows] != 5)[:, None], junk, s[rows]))
    return N.Reads.upload(seq.reshape(-1), qual.reshape(-1), off, device=reads.device)


def make_pairs(genomes, n, read_len, err, seed, chunk=250_000):
    """Two uploaded batches of n mates: fragments of 300 .. 500 bases drawn uniformly
    (genome, then start), mate 1 the first read_len bases, mate 2 the reverse
    complement of the last read_len; `err` substitutions per base; an N of the
    genome becomes a random base; qualities as synth.sample_reads draws them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = np.array([len(g) for g in genomes], dtype=np.int64)
    parts = ([], [], [], [])
    col = np.arange(read_len)[None, :]
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        origin = rng.integers(0, len(genomes), size=m)
        flen = rng.integers(300, 501, size=m)
        starts = (rng.random(m) * (lens[origin] - flen + 1)).astype(np.int64)
        s1 = np.empty((m, read_len), dtype=np.uint8)
        s2 = np.empty((m, read_len), dtype=np.uint8)
        for g in np.unique(origin):
            rows = np.flatnonzero(origin == g)
            s1[rows] = genomes[g][starts[rows, None] + col]
            s2[rows] = genomes[g][(starts[rows] + flen[rows] - read_len)[:, None] + col]
        s2 = synth.reverse_complement(s2)
        for s in (s1, s2):
            nmask = s == ord("N")
            if nmask.any():
                s[nmask] = synth.ACGT[rng.integers(0, 4, size=int(nmask.sum()))]
            if err > 0:
                emask = rng.random(s.shape) < err
                ne = int(emask.sum())
                if ne:
                    s[emask] = synth.ACGT[(np.searchsorted(synth.ACGT, s[emask]) + rng.integers(1, 4, size=ne)) % 4]
        for dst, s in ((0, s1), (2, s2)):
            parts[dst].append(np.ascontiguousarray(s).reshape(-1))
            q = np.clip(np.rint(rng.normal(60.0, 8.0, size=s.shape)), 35, 74).astype(np.uint8)
            parts[dst + 1].append(q.reshape(-1))
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(read_len)
    return (N.Reads.upload(np.concatenate(parts[0]), np.concatenate(parts[1]), off),
            N.Reads.upload(np.concatenate(parts[2]), np.concatenate(parts[3]), off))


def run_pairs(args, genomes, out):
    index = N.Index(genomes, 31, both_strands=True)
    index.prepare()
    m1, m2 = make_pairs(genomes, args.reads, 150, args.read_err, seed=2)
    prm = N.Params.make()
    n = args.reads
    res = N.Result(index)
    holder = {}

    def pairs(result):
        holder["r"] = N.align_pairs(index, m1, m2, prm, 0, result)
    os.environ.pop("PA_PAIR_COMBINE", None)
    med, ts = timed(lambda: pairs(res), args.runs)
    exact = int(holder["r"][5])
    types = holder["r"][0]
    out.update(align_pairs_s=med, align_pairs_runs_s=ts, pairs_per_s=n / med, exact_pairs=exact,
               exact_pairs_share=exact / n, list_entries=int(holder["r"][4].size),
               pair_types={name: int((types == t).sum()) for t, name in
                           ((2, "unique"), (3, "ambiguous"), (1, "unmapped"), (0, "dropped"))})
    med, ts = timed(lambda: pairs(None), args.runs)
    out.update(align_pairs_no_result_s=med, pair_count_s=out["align_pairs_s"] - med)
    os.environ["PA_PAIR_COMBINE"] = "0"
    med, ts = timed(lambda: pairs(res), args.runs)
    out.update(align_pairs_exact_only_s=med, align_pairs_exact_only_runs_s=ts,
               exact_pairs_exact_only=int(holder["r"][5]))
    del os.environ["PA_PAIR_COMBINE"]
    a1, _, e1 = time_assign(index, m1, prm, args.runs)
    a2, _, e2 = time_assign(index, m2, prm, args.runs)
    out.update(mates_assign_s=a1 + a2, mates_assign_each_s=[a1, a2], mates_list_entries=e1 + e2)
    d1, _, _ = time_detail(index, m1, prm, args.runs)
    d2, _, _ = time_detail(index, m2, prm, args.runs)
    out.update(mates_detail_s=d1 + d2, ratio_pairs_over_mates_assign=out["align_pairs_s"] / (a1 + a2))
    out["workload"] = (f"C2 both-strand index ({args.genomes} x {args.genome_len} bp, k=31), {n} pairs of 2 x 150 bp, "
                       "fragments of 300..500 bp, mate 2 reverse-complemented")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("detail", "coverage", "assign", "pileup", "abundance", "bootstrap", "pairs",
                                       "lineage", "containment", "trim"),
                    required=True)
    ap.add_argument("--replicates", type=int, default=100, help="bootstrap replicates of --mode bootstrap")
    ap.add_argument("--reads", type=int, default=None, help="reads (default 10 000 000); pairs with --mode pairs (1 000 000)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--genomes", type=int, default=50)
    ap.add_argument("--genome-len", type=int, default=2_000_000)
    ap.add_argument("--read-err", type=float, default=0.005)
    ap.add_argument("--rc-rate", type=float, default=0.0)
    ap.add_argument("--foreign-rate", type=float, default=0.0)
    ap.add_argument("--baseline-json", default=None, help="the line of a --mode detail run on the parent's library")
    args = ap.parse_args()
    if args.reads is None:
        args.reads = 1_000_000 if args.mode == "pairs" else 10_000_000
    genomes = synth.family_genomes(args.genomes, args.genome_len, seed=1, family_size=5, sub_rate=0.01,
                                   conserved_len=5000, n_rate=1e-4, n_run=10)
    if args.mode == "pairs":
        out = {"read_mix": {"err": args.read_err}, "mode": args.mode, "runs": args.runs,
               "library": N.lib().pa_version().decode()}
        run_pairs(args, genomes, out)
        print(json.dumps(out), flush=True)
        return
    index = N.Index(genomes, 31)
    index.prepare()
    reads = N.Reads.synthesize(index, args.reads, 150, first_read=0, seed=2, sub_rate=args.read_err,
                               rc_rate=args.rc_rate, foreign_rate=args.foreign_rate)
    prm = N.Params.make()
    out = {"workload": f"C2 index ({args.genomes} x {args.genome_len} bp, k=31), {args.reads} x 150 bp reads",
           "read_mix": {"err": args.read_err, "reverse_complement": args.rc_rate, "foreign": args.foreign_rate},
           "mode": args.mode, "runs": args.runs, "library": N.lib().pa_version().decode()}
    if args.mode == "detail":
        med, ts, entries = time_detail(index, reads, prm, args.runs)
        out.update(align_detail_s=med, align_detail_runs_s=ts, list_entries=entries)
    elif args.mode == "assign":
        med, ts, entries = time_assign(index, reads, prm, args.runs)
        out.update(align_reads_s=med, align_reads_runs_s=ts, list_entries=entries,
                   assign_reads_per_s=args.reads / med)
        index.profile_enable(True)
        index.profile_read_kernels()
        time_assign(index, reads, prm, 1)  # (three calls: the first, the warm-up and one timed)
        out["profiled_calls"] = 3
        out["kernels_ms_launches"] = index.profile_read_kernels()
        index.profile_enable(False)
        res = N.Result(index)
        N.align(index, reads, prm, 0, res)
        out["counter_pass_s"], _ = timed(lambda: (N.align(index, reads, prm, 0, res), res.fetch()), args.runs)
        dmed, dts, dentries = time_detail(index, reads, prm, args.runs)
        assert dentries == entries
        out.update(align_detail_s=dmed, align_detail_runs_s=dts, ratio_detail_over_assign=dmed / med)
    elif args.mode == "pileup":
        index.prepare_coverage()
        med, ts, entries = time_assign(index, reads, prm, args.runs)
        out.update(align_reads_s=med, align_reads_runs_s=ts, list_entries=entries)
        cov = N.Coverage(index)
        med, ts = timed(lambda: cov.add(reads, prm), args.runs)
        out.update(coverage_add_s=med, coverage_add_runs_s=ts)
        cov.close()
        pl = N.Pileup(index)
        med, ts = timed(lambda: pl.add(reads, prm), args.runs)
        out.update(pileup_add_s=med, pileup_add_runs_s=ts, pileup_reads_per_s=args.reads / med,
                   ratio_pileup_add_over_coverage_add=med / out["coverage_add_s"])
        med, ts = timed(lambda: pl.add(reads, prm, 60), args.runs)  # (synthesized qualities: normal(60, 8), so about half the bases)
        out.update(pileup_add_quality_s=med)
        index.profile_enable(True)
        index.profile_read_kernels()
        pl.add(reads, prm)
        out["profiled_calls"] = 1
        out["kernels_ms_launches"] = index.profile_read_kernels()
        index.profile_enable(False)
        pl.reset()
        pl.add(reads, prm)
        out["stats"] = pl.stats()
        for name, triple in (("variants_4_2_200", (4, 2, 200)), ("variants_1_1_0", (1, 1, 0))):
            holder = {}
            med, ts = timed(lambda: holder.update(v=pl.variants(*triple)), args.runs)
            out[name + "_s"] = med
            out[name + "_records"] = int(holder["v"].size)
        pl.close()
    elif args.mode == "abundance":
        med, ts, entries = time_assign(index, reads, prm, args.runs)
        out.update(align_reads_s=med, align_reads_runs_s=ts, list_entries=entries)
        holder = {}
        med, ts = timed(lambda: holder.update(c=N.align_candidates(index, reads, prm)), args.runs)
        out.update(align_candidates_s=med, align_candidates_runs_s=ts, set_entries=int(holder["c"][2].size))
        ab = N.Abundance(index)
        med, ts = timed(lambda: ab.add(reads, prm), args.runs)
        out.update(abundance_add_s=med, abundance_add_runs_s=ts, abundance_reads_per_s=args.reads / med)
        index.profile_enable(True)
        index.profile_read_kernels()
        ab.add(reads, prm)
        out["profiled_calls"] = 1
        out["kernels_ms_launches"] = index.profile_read_kernels()
        index.profile_enable(False)
        ab.reset()
        ab.add(reads, prm)
        info = ab.info()
        out["info"] = info
        amb = max(info["reads_ambiguous"], 1)
        out["candidate_passes_upper_s"] = out["align_candidates_s"] - out["align_reads_s"]
        out["candidates_and_interning_s"] = out["abundance_add_s"] - out["align_reads_s"]
        out["candidate_ns_per_ambiguous_read_upper"] = 1e9 * out["candidate_passes_upper_s"] / amb
        out["added_ns_per_ambiguous_read"] = 1e9 * out["candidates_and_interning_s"] / amb
        med, ts = timed(lambda: holder.update(e=ab.estimate(200, 0.0)), args.runs)
        out.update(estimate_200_s=med, estimate_200_runs_s=ts)
        med, ts = timed(lambda: holder.update(d=ab.estimate()), args.runs)
        out.update(estimate_default_s=med, estimate_default_iterations=holder["d"][2],
                   estimate_default_last_delta=holder["d"][3],
                   read_fraction_max=float(holder["e"][0].max()), read_fraction_min=float(holder["e"][0].min()))
        ab.close()
        index.prepare_coverage()
        cov = N.Coverage(index)
        med, ts = timed(lambda: cov.add(reads, prm), args.runs)
        out.update(coverage_add_s=med, coverage_add_runs_s=ts)
        cov.close()
        dmed, dts, dentries = time_detail(index, reads, prm, args.runs)
        out.update(align_detail_s=dmed, align_detail_runs_s=dts,
                   ratio_abundance_add_over_align_detail=out["abundance_add_s"] / dmed)
    elif args.mode == "bootstrap":
        ab = N.Abundance(index)
        ab.add(reads, prm)
        out["info"] = ab.info()
        B = args.replicates
        out["replicates"] = B
        holder = {}
        os.environ.pop("PA_BOOT_LDS", None)
        for tag, tol in (("200", 0.0), ("default", 1e-9)):
            med, ts = timed(lambda: holder.update(e=ab.estimate(200, tol)), args.runs)
            out.update({f"estimate_{tag}_s": med, f"estimate_{tag}_runs_s": ts,
                        f"estimate_{tag}_iterations": holder["e"][2]})
            for env, name in ((None, f"bootstrap_{tag}"), ("0", f"bootstrap_{tag}_global")):
                if env is not None:
                    os.environ["PA_BOOT_LDS"] = env
                med_b, ts = timed(lambda: holder.update(b=ab.bootstrap(B, 1, 200, tol)), args.runs)
                os.environ.pop("PA_BOOT_LDS", None)
                its = holder["b"][2]
                out.update({f"{name}_s": med_b, f"{name}_runs_s": ts,
                            f"{name}_iterations_min_max": [int(its.min()), int(its.max())],
                            f"ratio_{name}_over_B_estimates": med_b / (B * med)})
        share = holder["b"][1]
        out["abundance_sd_max"] = float(share.std(axis=0, ddof=1).max()) if B > 1 else 0.0
        ab.close()
    elif args.mode == "lineage":
        # families of five strains are species, the species hang off the root: an ambiguous read of a
        # family lands on its species node, so most of them share ten counters
        species = (args.genomes + 4) // 5
        parent = [0] + [0] * species + [1 + g // 5 for g in range(args.genomes)]
        genome_node = [1 + species + g for g in range(args.genomes)]
        med, ts, entries = time_assign(index, reads, prm, args.runs)
        out.update(align_reads_s=med, align_reads_runs_s=ts, list_entries=entries)
        ab = N.Abundance(index)
        med, ts = timed(lambda: ab.add(reads, prm), args.runs)
        out.update(abundance_add_s=med, abundance_add_runs_s=ts)
        ab.close()
        if not hasattr(N.lib(), "pa_lineage_create"):  # (the parent's library: the two yardsticks only)
            print(json.dumps(out), flush=True)
            return
        lin = N.Lineage(index, parent, genome_node)
        os.environ.pop("PA_LINEAGE_LDS", None)
        med, ts = timed(lambda: lin.add(reads, prm, nodes=False), args.runs)
        out.update(lineage_add_s=med, lineage_add_runs_s=ts, lineage_reads_per_s=args.reads / med,
                   ratio_lineage_add_over_abundance_add=med / out["abundance_add_s"])
        med, ts = timed(lambda: lin.add(reads, prm), args.runs)
        out.update(lineage_add_with_nodes_s=med)
        os.environ["PA_LINEAGE_LDS"] = "0"
        med, ts = timed(lambda: lin.add(reads, prm, nodes=False), args.runs)
        out.update(lineage_add_global_atomics_s=med, lineage_add_global_atomics_runs_s=ts)
        del os.environ["PA_LINEAGE_LDS"]
        lin.reset()
        nodes = lin.add(reads, prm)
        direct, clade, info = lin.counts()
        out.update(info=info, nodes=len(parent), reads_on_species_nodes=int(direct[1:1 + species].sum()),
                   reads_on_root=int(direct[0]), classified=int(clade[0]),
                   no_node=int((nodes == N.NO_NODE).sum()))
        lin.close()
    elif args.mode == "trim":
        batch = make_trim_batch(reads)
        reads.close()
        spec = N.TrimSpec.make(quality3=55, quality5=55, adapter=TRUSEQ)
        holder = {}

        def trim_call():
            if "out" in holder:
                holder.pop("out")[0].close()
            holder["out"] = batch.trim(spec)  # (ends in a synchronise: start / end come back to the host)
        med, ts = timed(trim_call, args.runs)
        trimmed, _, _, stats = holder["out"]
        out.update(trim_spec="quality3 = quality5 = 55, the 33-base TruSeq adapter, overlap 3, 100 permille",
                   reads_trim_s=med, reads_trim_runs_s=ts, trim_reads_per_s=args.reads / med, trim_stats=stats,
                   trim_bytes_moved=2 * 2 * stats["bases_out"], trim_input_bytes=2 * stats["bases_in"])
        res = N.Result(index)
        for name, b in (("untrimmed", batch), ("trimmed", trimmed)):
            N.align(index, b, prm, 0, res)
            cmed, cts = timed(lambda: (N.align(index, b, prm, 0, res), res.fetch()), args.runs)
            amed, ats, entries = time_assign(index, b, prm, args.runs)
            out.update({f"counter_pass_{name}_s": cmed, f"counter_pass_{name}_runs_s": cts,
                        f"align_reads_{name}_s": amed, f"list_entries_{name}": entries})
        out.update(ratio_trim_over_counter_pass_untrimmed=med / out["counter_pass_untrimmed_s"],
                   ratio_trim_over_counter_pass_trimmed=med / out["counter_pass_trimmed_s"],
                   ratio_trim_over_align_reads_trimmed=med / out["align_reads_trimmed_s"])
        trimmed.close()
        batch.close()
    elif args.mode == "containment":
        med, ts, entries = time_assign(index, reads, prm, args.runs)
        out.update(align_reads_s=med, align_reads_runs_s=ts, list_entries=entries)
        dmed, dts, _ = time_detail(index, reads, prm, args.runs)
        out.update(align_detail_s=dmed, align_detail_runs_s=dts)
        con = N.Containment(index)
        os.environ["PA_CONTAIN_STATS"] = "1"  # (stderr: the atomic ORs issued since the reset, after each add)
        t0 = time.perf_counter()
        con.add(reads, prm)
        out["containment_first_add_s"] = time.perf_counter() - t0  # (every k-mer's bit still clear)
        con.add(reads, prm)
        del os.environ["PA_CONTAIN_STATS"]
        med, ts = timed(lambda: con.add(reads, prm), args.runs)
        out.update(containment_add_s=med, containment_add_runs_s=ts, containment_reads_per_s=args.reads / med,
                   ratio_containment_add_over_align_detail=med / dmed,
                   ratio_containment_add_over_align_reads=med / out["align_reads_s"])
        os.environ["PA_CONTAIN_LDS"] = "0"
        med, ts = timed(lambda: con.add(reads, prm), args.runs)
        out.update(containment_add_global_atomics_s=med)
        del os.environ["PA_CONTAIN_LDS"]
        holder = {}
        med, ts = timed(lambda: holder.update(c=con.counts()), args.runs)
        out.update(counts_s=med, counts_runs_s=ts)
        species = (args.genomes + 4) // 5  # (--mode lineage's tree)
        parent = [0] + [0] * species + [1 + g // 5 for g in range(args.genomes)]
        lin = N.Lineage(index, parent, [1 + species + g for g in range(args.genomes)])
        med, ts = timed(lambda: holder.update(n=con.nodes(lin)), args.runs)
        out.update(nodes_s=med)
        arrays, info = holder["c"]
        out.update(info=info, kmers=int(arrays["kmers"].sum()), kmers_seen=int(arrays["kmers_seen"].sum()),
                   specific=int(arrays["specific"].sum()), specific_seen=int(arrays["specific_seen"].sum()),
                   n_kmers=int(index.info().n_kmers), clade_kmers_root=int(holder["n"][2][0]),
                   clade_seen_root=int(holder["n"][3][0]), table_slots=int(index.info().table_slots))
        lin.close()
        con.close()
    else:
        med, ts, entries = time_detail(index, reads, prm, args.runs)
        out.update(align_detail_branch_s=med, align_detail_branch_runs_s=ts, list_entries=entries)
        b0 = int(index.info().device_bytes)
        t0 = time.perf_counter()
        index.prepare_coverage()
        out["view_build_s"] = time.perf_counter() - t0
        out["view_bytes"] = int(index.info().device_bytes) - b0
        out["view_bytes_per_region_position"] = out["view_bytes"] / (args.genomes * args.genome_len)
        cov = N.Coverage(index)
        med, ts = timed(lambda: cov.add(reads, prm), args.runs)
        out.update(coverage_add_s=med, coverage_add_runs_s=ts)
        cov.reset()
        cov.add(reads, prm)
        t0 = time.perf_counter()
        cu, ca, su, sa = cov.summary(1)
        out["summary_s"] = time.perf_counter() - t0
        out["covered_bases_unique"] = int(cu.sum())
        out["sum_unique"] = int(su.sum())
        if args.baseline_json:
            with open(args.baseline_json) as f:
                base = json.loads(f.read().strip().splitlines()[-1])
            if base["workload"] != out["workload"] or base["mode"] != "detail":
                sys.exit("--baseline-json: not a --mode detail line of this workload")
            out.update(align_detail_parent_s=base["align_detail_s"],
                       align_detail_parent_runs_s=base["align_detail_runs_s"], parent_library=base["library"],
                       ratio_coverage_add_over_align_detail=out["coverage_add_s"] / base["align_detail_s"],
                       method=f"scripts/coverage_rate.py: median of {args.runs} timed calls after one warm-up call; "
                              "baseline = pa_align_detail (with lists) of the library in parent_library")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
