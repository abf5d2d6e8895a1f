#!/usr/bin/env python3
"""The extract job end to end on the C2 files (scripts/e2e_cli.py's), next to
the two routes a library without extraction offers.

    python scripts/extract_rate.py [--reads N] [--dir DIR] [--out-dir TMPFS] [--parent-library libpa_parent.so]

Writes the C2 genomes and N x 150 bp reads to DIR, then times whole
`main.py -t dumpalign` commands (the median of --runs):
  floor        plain dumpalign of the file (no per-read result)
  assignments  dumpalign --assignments FILE, the only route from a file to
               per-read results without --extract
  extract      dumpalign --extract FILE for four selections: the mapped reads
               (the default), everything (all four types), one type that is a
               fifth of C2's reads (ambiguous) and one that is next to none (unmapped)
With --parent-library the first two run on that library (PA_LIBRARY,
PA_LIBRARY_PARTIAL=1).  The outputs go to --out-dir (a tmpfs).  One more
extract run with PA_STREAM_TIMING=1 gives the per-window split (medians over
the windows) and the gather kernel's and the device-to-host copy's rates.
Prints one JSON line."""

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "bioinformatics-project-for-shotgun-metagenomics-pseudo-alignment-shotgun-_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(REPO, "scripts"))

import synth  # noqa: E402
from e2e_cli import write_fastq  # noqa: E402

WINDOW = re.compile(r"\[pa_extract\] window: (\d+) records, (\d+) text bytes, (\d+) bytes out: parse \+ counter pass "
                    r"([\d.]+) ms, assign ([\d.]+) ms, select \+ scan ([\d.]+) ms, gather ([\d.]+) ms, copy to host "
                    r"([\d.]+) ms, write ([\d.]+) ms")


def timed(cmd, runs, env=None):
    walls, last = [], None
    for _ in range(runs):
        time.sleep(2)  # (an idle device: the previous process's memory is reclaimed after it exits)
        t = time.perf_counter()
        last = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
        walls.append(time.perf_counter() - t)
        if last.returncode:
            raise SystemExit(f"command failed: {' '.join(cmd)}\n{last.stderr[-2000:]}")
    return statistics.median(walls), walls, last


def split_of(stderr):
    rows = [tuple(float(x) for x in m.groups()) for m in WINDOW.finditer(stderr)]
    full = [r for r in rows if r[1] >= max(x[1] for x in rows) * 0.9] or rows  # (the last window is short)
    med = lambda i: statistics.median(r[i] for r in full)  # noqa: E731
    out = {"windows": len(rows), "full_windows": len(full), "text_bytes": med(1), "bytes_out": med(2),
           "parse_counter_ms": med(3), "assign_ms": med(4), "select_scan_ms": med(5), "gather_ms": med(6),
           "copy_to_host_ms": med(7), "write_ms": med(8)}
    if out["gather_ms"] > 0:
        out["gather_out_GBps"] = out["bytes_out"] / out["gather_ms"] / 1e6
        out["copy_GBps"] = out["bytes_out"] / out["copy_to_host_ms"] / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--dir", default="/tmp/pa_e2e")
    ap.add_argument("--out-dir", default="/dev/shm")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-library", default=None)
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    fa, fq = os.path.join(args.dir, "c2.fa"), os.path.join(args.dir, "c2.fq")
    genomes = synth.family_genomes(50, 2_000_000, seed=1, family_size=5, sub_rate=0.01, conserved_len=5000,
                                   n_rate=1e-4, n_run=10)
    with open(fa, "w") as f:
        f.write(synth.fasta_text([f"genome_{i} synthetic C2" for i in range(50)], genomes, width=80))
    write_fastq(fq, genomes, args.reads)
    out_fq, out_txt = os.path.join(args.out_dir, "pa_extract_out.fq"), os.path.join(args.out_dir, "pa_assign_out.txt")
    base = [sys.executable, os.path.join(PKG, "main.py"), "-t", "dumpalign", "-g", fa, "-k", "31", "--reads", fq]
    penv = None
    if args.parent_library:
        penv = dict(os.environ, PA_LIBRARY=os.path.abspath(args.parent_library), PA_LIBRARY_PARTIAL="1")
    res = {"workload": f"dumpalign C2: 50 x 2 Mbp FASTA, {args.reads} x 150 bp FASTQ, k=31",
           "fastq_bytes": os.path.getsize(fq), "parent_library": args.parent_library, "runs": args.runs}
    floor, walls, plain = timed(base, args.runs, penv)
    res["floor"] = {"wall_s": floor, "runs_s": walls}
    t, walls, r = timed(base + ["--assignments", out_txt], max(1, args.runs - 1), penv)
    res["assignments"] = {"wall_s": t, "runs_s": walls, "bytes": os.path.getsize(out_txt),
                          "stdout_equals_floor": r.stdout == plain.stdout}
    os.remove(out_txt)
    for name, extra in (("extract_mapped", []), ("extract_everything", ["--extract-mapping",
                                                                         "unique,ambiguous,unmapped,filtered"]),
                        ("extract_ambiguous", ["--extract-mapping", "ambiguous"]),
                        ("extract_unmapped", ["--extract-mapping", "unmapped"])):
        t, walls, r = timed(base + ["--extract", out_fq] + extra, args.runs)
        res[name] = {"wall_s": t, "runs_s": walls, "bytes": os.path.getsize(out_fq),
                     "stdout_equals_floor": r.stdout == plain.stdout, "over_floor": t / floor,
                     "assignments_over_this": res["assignments"]["wall_s"] / t}
        env = dict(os.environ, PA_STREAM_TIMING="1")
        rt = subprocess.run(base + ["--extract", out_fq] + extra, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                            text=True, env=env)
        res[name]["per_window"] = split_of(rt.stderr)
        res[name]["stream_line"] = [x for x in rt.stderr.splitlines() if x.startswith("[pa_stream]")][-1:]
        os.remove(out_fq)
    print(json.dumps(res), flush=True)
    for p in (fa, fq):
        os.remove(p)


if __name__ == "__main__":
    main()
