#!/usr/bin/env python3
"""Generate ``strand_cases.json``: the golden vectors of both-strand alignment
(``Index(..., both_strands=True)``, ``KmerReference(..., both_strands=True)``,
``main.py --both-strands``), by running the REFERENCE.

Run only in the build container, where ``/root/reference`` exists:

    python tests/golden/make_golden_strands.py

The reference has no both-strand mode.  A both-strand index of the genomes
``g`` is, by definition, a forward index of ``T(g) = g + "N" +
reverse_complement(g)`` (synth.both_strands_genome): windows holding the N are
not indexed (src/kmer.py:145), so every k-mer gets its own genomes and its
reverse complement's.  The file therefore holds the RAW genomes, and this
generator applies ``T`` before it calls the reference (imported from a scratch
copy, as make_golden.py does -- its helpers are reused).

* ``cases`` - unit-case format (see make_golden.py): the reference's k = 4
  fixtures with their reads and those reads' reverse complements, and seeded
  cases (k = 16, 31, 32, 63, 75, 150) of four genomes of 600-1500 bases plus
  one shorter than k, with N runs, an (ACGT)n run, a 100-base hairpin at a
  genome's end and a stretch whose reverse complement lies in another genome;
  about 60 reads of 40-272 bases, half of them reverse-complemented; five
  parameter sets each.  ``kmer_sets`` is a sample (every n-th k-mer in sorted
  order, about 50 per case);
* ``cli`` - the reference CLI's ``dumpalign`` stdout for four flag sets on the
  T-FASTA and the FASTQ text of the named case (its raw genomes and reads, as
  ``>header\nsequence\n`` and ``@id\nsequence\n+\nquality\n`` records).
"""

from __future__ import annotations

import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (copies the reference to a scratch directory and imports it from there)
import synth  # noqa: E402  (our own synthetic-data module, not the reference)

P = MG.P
PSETS = [P(), P(m=0, p=0), P(p=-1), P(mg=2), P(mrq=58, mkq=60, mg=2)]


def T(seq: str) -> str:
    return bytes(synth.both_strands_genome(seq)).decode()


def rc(seq: str) -> str:
    return bytes(synth.reverse_complement(np.frombuffer(seq.encode(), dtype=np.uint8))).decode()


def fixture_cases():
    """The reference's k = 4 fixtures (src/test_kmer.py), each read also reverse-complemented."""
    out = []
    for c in MG.fixture_cases():
        if c["k"] != 4:
            continue
        reads = []
        for rid, s, q in c["reads"]:
            reads += [(rid, s, q), (rid + "_rc", rc(s), q[::-1])]
        out.append({"name": "strand_" + c["name"], "genomes": c["genomes"], "k": 4, "reads": reads, "psets": PSETS})
    return out


def seeded_cases():
    out = []
    rng = np.random.Generator(np.random.PCG64(4242))
    for k in (16, 31, 32, 63, 75, 150):
        lens = [int(x) for x in rng.integers(600, 1501, size=4)]
        gens = [bytearray(synth.ACGT[rng.integers(0, 4, size=n)]) for n in lens]
        # genome 1: a relative of genome 0 (2 % substitutions over their common length)
        n01 = min(lens[0], lens[1])
        rel = bytearray(gens[0][:n01])
        for j in np.flatnonzero(rng.random(n01) < 0.02):
            rel[j] = int(synth.ACGT[rng.integers(0, 4)])
        gens[1][:n01] = rel
        # genome 3 holds the reverse complement of a stretch of genome 0: k-mers
        # whose reverse complement lies in another genome
        a = int(rng.integers(0, lens[0] - 300))
        gens[3][50:350] = rc(bytes(gens[0][a:a + 300]).decode()).encode()
        # an (ACGT)n run: its k-mers are their own reverse complements' neighbours
        gens[2][100:100 + 4 * 45] = b"ACGT" * 45
        # N runs
        for g in gens:
            for s in rng.integers(0, len(g) - 10, size=2):
                n = int(rng.integers(1, 6))
                g[int(s):int(s) + n] = b"N" * n
        # a 100-base hairpin at a genome's end: a stretch followed by its reverse complement
        stem = bytes(synth.ACGT[rng.integers(0, 4, size=50)]).decode()
        gens[1][-100:] = (stem + rc(stem)).encode()
        short = bytes(synth.ACGT[rng.integers(0, 4, size=k - 1)])  # shorter than k: no window on either strand
        seqs = [bytes(g).decode() for g in gens] + [short.decode()]
        genomes = [(f"g{i} k{k}", s) for i, s in enumerate(seqs)]
        reads = []
        for ri in range(60):
            L = int(rng.integers(40, 273))
            src = seqs[int(rng.integers(4))]
            if rng.random() < 0.9:
                st = int(rng.integers(0, len(src) - L + 1))
                s = bytearray(src[st:st + L].encode())
            else:
                s = bytearray(synth.ACGT[rng.integers(0, 4, size=L)])
            for j in range(L):
                if s[j] == ord("N") or rng.random() < 0.01:
                    s[j] = int(synth.ACGT[rng.integers(0, 4)])
            lvl = float(rng.uniform(54, 66))
            q = np.clip(np.rint(rng.normal(lvl, 6, size=L)), 33, 74).astype(np.uint8).tobytes().decode()
            text = s.decode()
            if ri % 2:
                text, q = rc(text), q[::-1]
            reads.append((f"r{ri}", text, q))
        out.append({"name": f"strand_k{k}", "genomes": genomes, "k": k, "reads": reads, "psets": PSETS})
    return out


def main():
    entries = []
    for case in fixture_cases() + seeded_cases():
        t_genomes = [(h, T(s)) for h, s in case["genomes"]]
        entry = {"name": case["name"], "k": case["k"], "genomes": case["genomes"], "reads": case["reads"],
                 "results": []}
        for ps in case["psets"]:
            res, ref = MG.run_case(t_genomes, case["k"], case["reads"], ps)
            entry["results"].append(res)
        entry["n_kmers"] = len(ref.kmers)
        gidx = {id(g): i for i, g in enumerate(ref.genomes)}
        allk = sorted(ref.kmers)
        step = max(1, len(allk) // 50)
        entry["kmer_sets"] = [[km, sorted(gidx[id(g)] for g in ref.kmers[km])] for km in allk[::step]]
        entries.append(entry)
    # the CLI: dumpalign on the T-FASTA of the k = 31 case
    c = next(x for x in entries if x["name"] == "strand_k31")
    fastq = MG.fastq_of(c["reads"])
    fa = os.path.join(MG.SCRATCH, "strand_t.fa")
    fq = os.path.join(MG.SCRATCH, "strand.fq")
    with open(fa, "w") as f:
        f.write(MG.fasta_of([(h, T(s)) for h, s in c["genomes"]]))
    with open(fq, "w") as f:
        f.write(fastq)
    runs = []
    for fl in ([], ["-p", "-1"], ["--max-genomes", "2"],
               ["--min-read-quality", "58", "--min-kmer-quality", "60", "--max-genomes", "2"]):
        cmd = [sys.executable, "main.py", "-t", "dumpalign", "-g", fa, "-k", "31", "--reads", fq] + fl
        r = subprocess.run(cmd, cwd=MG.REFDIR, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        runs.append({"flags": fl, "stdout": r.stdout})
    with open(os.path.join(HERE, "strand_cases.json"), "w") as f:
        json.dump({"cases": entries, "cli": {"case": c["name"], "k": 31, "runs": runs}}, f, separators=(",", ":"))
    print("strand cases:", len(entries), "reads x psets:", sum(len(c["reads"]) * len(c["results"]) for c in entries))


if __name__ == "__main__":
    try:
        main()
    finally:
        shutil.rmtree(MG.SCRATCH, ignore_errors=True)
