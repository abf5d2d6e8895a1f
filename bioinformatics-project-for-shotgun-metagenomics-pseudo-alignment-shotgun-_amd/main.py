#!/usr/bin/env python3
"""Command-line interface, drop-in for the reference's src/main.py.

    python3 main.py -t dumpalign -g GENOMES.fa -k 31 --reads READS.fq [--reads2 MATES2.fq] [-m M] [-p P]
                    [--min-read-quality Q] [--min-kmer-quality QK] [--max-genomes MG]
                    [--filter-similar [--similarity-threshold T]]
                    [--coverage [--genomes a,b,c] [--min-coverage N] [--full-coverage]]
                    [--assignments FILE]
                    [--variants FILE [--variant-min-depth N] [--variant-min-count N]
                     [--variant-min-fraction F] [--variant-min-base-quality Q]]
                    [--abundance FILE [--abundance-iterations N] [--abundance-tolerance X]
                     [--abundance-bootstraps B [--abundance-seed S] [--abundance-confidence X]]]
                    [--lineages FILE [--lineage-report FILE]]
                    [--containment FILE]
                    [--extract FILE [--extract-mapping LIST] [--extract-genomes a,b] [--extract-invert]]
                    [--trim-quality Q] [--trim-quality5 Q] [--trim-adapter SEQ] [--trim-adapter2 SEQ]
                    [--trim-min-overlap N] [--trim-error-rate X] [--trim-report FILE]

Same tasks (reference | dumpref | align | dumpalign), flags, flag-combination
checks, default coercions and error exits as src/main.py:61-402:

* ``-m 0`` / ``-p 0`` / ``--similarity-threshold 0`` are falsy and coerced to
  their defaults (1, 1, 0.95), exactly like src/main.py:337-342;
* errors end the process with ``sys.exit(message)`` (non-zero, message on
  stderr).

The ``.kdb`` / ``.aln`` files are gzip pickles, loaded by a restricted
unpickler (kmer._KdbUnpickler) that admits only the classes such files hold;
the classes keep the reference's module and class names, so files written by
the reference load too (a loaded reference rebuilds its device index).
``dumpref`` streams its JSON from the device index (pa_index_dumpref).
"""

from __future__ import annotations

import argparse
import atexit
import gzip
import json
import os
import sys
import time
from typing import List, Optional

_T0 = time.perf_counter()

_EARLY_PREFETCH = None  # (path, native handle) of a FASTQ prefetch started at entry


_FQ_PLAIN_EXT = ".fq"  # (FASTAQFile.EXTENSIONS without ".fq.gz": the file types the prefetch takes)


_COVERAGE_FLAGS = ("--coverage", "--genomes", "--min-coverage", "--full-coverage")


def _has_coverage_flag(argv: List[str]) -> bool:
    """A coverage flag on the command line, in any spelling argparse accepts
    (`--flag=X`, an unambiguous prefix).  Read off argv before argparse; a
    prefix shared with another flag counts too, which only costs the early prefetch."""
    for a in argv:
        name = a.split("=", 1)[0]
        if len(name) > 2 and name.startswith("--") and any(f.startswith(name) for f in _COVERAGE_FLAGS):
            return True
    return False


def _has_assignments_flag(argv: List[str]) -> bool:
    """--assignments on the command line, in any spelling argparse accepts
    (`--assignments X`, `--assignments=X`, an unambiguous prefix; a prefix
    shared with another flag counts too, which only costs the early prefetch)."""
    for a in argv:
        name = a.split("=", 1)[0]
        if len(name) > 2 and name.startswith("--") and "--assignments".startswith(name):
            return True
    return False


_VARIANT_FLAGS = ("--variants", "--variant-min-depth", "--variant-min-count", "--variant-min-fraction",
                  "--variant-min-base-quality")


def _has_variants_flag(argv: List[str]) -> bool:
    """A --variants / --variant-* flag on the command line, in any spelling
    argparse accepts (as _has_coverage_flag)."""
    for a in argv:
        name = a.split("=", 1)[0]
        if len(name) > 2 and name.startswith("--") and any(f.startswith(name) for f in _VARIANT_FLAGS):
            return True
    return False


_ABUNDANCE_FLAGS = ("--abundance", "--abundance-iterations", "--abundance-tolerance", "--abundance-bootstraps",
                    "--abundance-seed", "--abundance-confidence")


def _has_abundance_flag(argv: List[str]) -> bool:
    """An --abundance* flag on the command line, in any spelling argparse accepts
    (as _has_coverage_flag)."""
    for a in argv:
        name = a.split("=", 1)[0]
        if len(name) > 2 and name.startswith("--") and any(f.startswith(name) for f in _ABUNDANCE_FLAGS):
            return True
    return False


_LINEAGE_FLAGS = ("--lineages", "--lineage-report")


def _has_lineage_flag(argv: List[str]) -> bool:
    """--lineages / --lineage-report on the command line, in any spelling argparse
    accepts (as _has_coverage_flag)."""
    for a in argv:
        name = a.split("=", 1)[0]
        if len(name) > 2 and name.startswith("--") and any(f.startswith(name) for f in _LINEAGE_FLAGS):
            return True
    return False


def _has_containment_flag(argv: List[str]) -> bool:
    """--containment on the command line, in any spelling the parser accepts
    (`--con` and longer: `--c` and `--co` are --coverage's)."""
    for a in argv:
        name = a.split("=", 1)[0]
        if name.startswith("--con") and "--containment".startswith(name):
            return True
    return False


_EXTRACT_FLAGS = ("--extract", "--extract-mapping", "--extract-genomes", "--extract-invert")


def _has_extract_flag(argv: List[str]) -> bool:
    """An --extract* flag on the command line, in any spelling argparse accepts
    (as _has_coverage_flag)."""
    for a in argv:
        name = a.split("=", 1)[0]
        if len(name) > 2 and name.startswith("--") and any(f.startswith(name) for f in _EXTRACT_FLAGS):
            return True
    return False


def _has_reads2_flag(argv: List[str]) -> bool:
    """--reads2 on the command line (`--reads2 X`, `--reads2=X`)."""
    return any(a.split("=", 1)[0] == "--reads2" for a in argv)


def _early_reads_path(argv: List[str]) -> Optional[str]:
    """The --reads file of a `-t dumpalign` command line, read off argv before
    argparse and the heavy imports (every spelling argparse accepts: `-t X`,
    `-tX`, `--task X`, `--task=X`, `--reads X`, `--reads=X`), when it is a file
    the later prefetch would take too (_prefetch_reads: a plain `.fq`, streaming
    and prefetch on).  A guess: main() still validates everything and ignores
    the early prefetch unless it names the same file."""
    task = reads = None
    i = 0
    while i < len(argv):
        a = argv[i]
        nxt = argv[i + 1] if i + 1 < len(argv) else None
        if a in ("-t", "--task"):
            task, i = nxt, i + 2
            continue
        if a == "--reads":
            reads, i = nxt, i + 2
            continue
        if a.startswith("--task="):
            task = a.split("=", 1)[1]
        elif a.startswith("-t") and not a.startswith("--") and len(a) > 2:
            task = a[2:]
        elif a.startswith("--reads="):
            reads = a.split("=", 1)[1]
        i += 1
    if task != "dumpalign" or not reads or not reads.endswith(_FQ_PLAIN_EXT):
        return None
    if _has_coverage_flag(argv):  # (a coverage job parses the reads on the host)
        return None
    if _has_assignments_flag(argv):  # (so does a job that writes every read's assignment)
        return None
    if _has_variants_flag(argv):  # (and a pileup job: the base counts need the read columns)
        return None
    if _has_abundance_flag(argv):  # (and an abundance job: the candidate pass needs the read columns)
        return None
    if _has_lineage_flag(argv):  # (and a lineage job, as an abundance job)
        return None
    if _has_containment_flag(argv):  # (and a containment job: its pass takes the read columns)
        return None
    if _has_extract_flag(argv):  # (an extract job streams the file in windows itself, records gathered per window)
        return None
    if _has_reads2_flag(argv):  # (and a paired job: both files are parsed on the host)
        return None
    if os.environ.get("PA_GPUS", "1") not in ("", "0", "1"):  # (read-sharded over GPUs: no whole-file prefetch)
        return None
    if os.environ.get("PA_STREAM", "1") == "0" or os.environ.get("PA_PREFETCH", "1") == "0":
        return None
    return reads


def _stream_window() -> int:
    """PA_STREAM_WINDOW (bytes; 0: the library's default), as pa_native reads it."""
    env = os.environ.get("PA_STREAM_WINDOW")
    return int(env) if env and env.isdigit() else 0


if __name__ == "__main__":  # the HIP runtime starts on a native thread while the modules below import
    try:
        import ctypes
        _here = os.path.dirname(os.path.abspath(__file__))
        _lib = ctypes.CDLL(os.environ.get("PA_LIBRARY", os.path.join(_here, "libpa.so")))
        _dev = int(os.environ.get("PA_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _lib.pa_runtime_start(_dev)
        # (a flag check may end the process at once: no way out leaves before the start is
        # over, or the runtime's exit handlers would run under the thread still starting it)
        import atexit
        atexit.register(_lib.pa_runtime_wait)
        # a plain FASTQ's copy into device memory starts now too (pa_fastq_prefetch_start
        # makes no HIP call on this thread): it overlaps the imports, not only the build
        _r = _early_reads_path(sys.argv[1:])
        if _r and os.path.isfile(_r) and os.environ.get("PA_EARLY_PREFETCH", "1") != "0":
            _n = len(os.sched_getaffinity(0))
            _omp = os.environ.get("OMP_NUM_THREADS", "")
            _thr = os.environ.get("PA_INGEST_THREADS", "")
            _threads = int(_thr) if _thr.isdigit() and int(_thr) > 0 else \
                max(1, min(min(_n, int(_omp)) if _omp.isdigit() and int(_omp) > 0 else _n, 16))
            _h = ctypes.c_void_p()
            _lib.pa_fastq_prefetch_start.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32,
                                                     ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]
            if (_lib.pa_fastq_prefetch_start(os.fsencode(_r), _dev, _threads, _stream_window(), ctypes.byref(_h)) == 0
                    and _h.value):
                _EARLY_PREFETCH = (os.path.abspath(_r), _h)

                def _free_early_prefetch():  # (an early exit: argument errors, another task)
                    if _EARLY_PREFETCH is not None:
                        _lib.pa_fastq_prefetch_free.argtypes = [ctypes.c_void_p]
                        _lib.pa_fastq_prefetch_free(_EARLY_PREFETCH[1])
                atexit.register(_free_early_prefetch)
    except (OSError, AttributeError, ValueError):
        pass  # (no library: pa_native raises at the first device call)

from constants import DEFAULT_AMBIGUOUS_THRESHOLD, DEFAULT_SIMILARITY_THRESHOLD, DEFAULT_UNIQUE_THRESHOLD
from data_file import FASTAFile, FASTAQFile, InvalidExtensionError, NoRecordsInDataFile
from kmer import (AddingExistingRead, KmerReference, NotValidatingUniqueMapping, PseudoAlignment,
                  extract_type_mask)
import trim as trimming

_TIMING = os.environ.get("PA_CLI_TIMING") == "1"  # stage times on stderr (diagnostic)


def _stage(name: str) -> None:
    if _TIMING:
        print(f"[pa_cli] {name}: {time.perf_counter() - _T0:.3f} s", file=sys.stderr, flush=True)


def validate_file_readable(filepath: str, description: str) -> None:
    if not os.path.isfile(filepath):
        sys.exit(f"Error: {description} file '{filepath}' does not exist or is not a file.")
    if not os.access(filepath, os.R_OK):
        sys.exit(f"Error: {description} file '{filepath}' is not readable.")


def validate_file_writable(filepath: str, description: str) -> None:
    dir_path = os.path.dirname(filepath) or "."
    if os.path.exists(filepath) and not os.access(filepath, os.W_OK):
        sys.exit(f"Error: {description} file '{filepath}' is not writable.")
    if not os.path.exists(filepath) and not os.access(dir_path, os.W_OK):
        sys.exit(f"Error: Directory '{dir_path}' is not writable to create {description} file '{filepath}'.")


def parse_arguments(args: Optional[List[str]] = None) -> argparse.Namespace:
    class _Parser(argparse.ArgumentParser):
        # --containment answers to `--con...` only: `--c` and `--co` stay --coverage's abbreviations
        def _get_option_tuples(self, option_string):
            found = super()._get_option_tuples(option_string)
            if len(found) > 1 and not option_string.split("=", 1)[0].startswith("--con"):
                found = [t for t in found if "--containment" not in t[0].option_strings]
            return found

    parser = _Parser(prog="Biosequence project")
    parser.add_argument("-t", "--task", required=True, help="Task to execute")
    parser.add_argument("-g", "--genomefile", help="Genome FASTA file (multiple records)")
    parser.add_argument("-k", "--kmer-size", type=int, help="Length of k-mers")
    parser.add_argument("-r", "--referencefile", help="KDB file (input/output)")
    parser.add_argument("-a", "--alignfile", help="aln file. Can be either input or name for output file")
    parser.add_argument("--reads", help="FASTQ reads file")
    parser.add_argument("--reads2", default=None, metavar="FILE",
                        help="FASTQ file of the second mates: record i of --reads and of --reads2 are one pair, "
                             "classified as one fragment (paired data wants --both-strands)")
    parser.add_argument("-m", "--unique-threshold", help="unique k-mer threshold", type=int)
    parser.add_argument("-p", "--ambiguous-threhold", help="ambiguous k-mer threshold", type=int)
    parser.add_argument("--reverse-complement", action="store_true")  # parsed, unused (as in the reference)
    # not in the reference: align against both strands (building from -g; with -r the file's property decides)
    parser.add_argument("--both-strands", action="store_true")
    parser.add_argument("--min-read-quality", type=int, default=None)
    parser.add_argument("--min-kmer-quality", type=int, default=None)
    parser.add_argument("--max-genomes", type=int, default=None)
    parser.add_argument("--filter-similar", action="store_true")
    parser.add_argument("--similarity-threshold", type=float)
    # EXTCOVERAGE (the course project's extension the reference leaves out): dumpalign with --reads
    parser.add_argument("--coverage", action="store_true", help="add per-genome read coverage to dumpalign's JSON")
    parser.add_argument("--genomes", default=None, help="comma-separated genome identifiers to report (default: all)")
    parser.add_argument("--min-coverage", type=int, default=None,
                        help="reads a position needs to count as covered (default: 1)")
    parser.add_argument("--full-coverage", action="store_true", help="also print the depth at every position")
    # not in the reference: read -> genome as text, dumpalign with --reads
    parser.add_argument("--assignments", default=None, metavar="FILE",
                        help="write one line per read (id, mapping, genomes) to FILE")
    # not in the reference: per-base pileup of the uniquely mapped reads and its SNV calls, dumpalign with --reads
    parser.add_argument("--variants", default=None, metavar="FILE",
                        help="write one line per called variant (genome, position, ref, alt, counts) to FILE")
    parser.add_argument("--variant-min-depth", type=int, default=None, help="counted bases a position needs (default: 4)")
    parser.add_argument("--variant-min-count", type=int, default=None,
                        help="reads the alternative base needs (default: 2)")
    parser.add_argument("--variant-min-fraction", type=float, default=None,
                        help="share of the depth the alternative base needs (default: 0.2)")
    parser.add_argument("--variant-min-base-quality", type=int, default=None,
                        help="count only bases whose quality byte is at least this (default: all)")
    # not in the reference: the genomes' shares of the sample (compatibility classes + EM), dumpalign with --reads
    parser.add_argument("--abundance", default=None, metavar="FILE",
                        help="write one line per genome (reads, estimated reads, read fraction, abundance) to FILE")
    parser.add_argument("--abundance-iterations", type=int, default=None, help="EM iterations at most (default: 200)")
    parser.add_argument("--abundance-tolerance", type=float, default=None,
                        help="stop once no read fraction moves by this much (default: 1e-9; 0: never)")
    parser.add_argument("--abundance-bootstraps", type=int, default=None, metavar="B",
                        help="add mean, sd and a confidence interval of the abundance over B bootstrap replicates")
    parser.add_argument("--abundance-seed", type=int, default=None, metavar="S",
                        help="seed of the bootstrap's resampling, 0 .. 2^64 - 1 (default: 1)")
    parser.add_argument("--abundance-confidence", type=float, default=None, metavar="X",
                        help="confidence level of the bootstrap interval (default: 0.95)")
    # not in the reference: reads and abundances rolled up a taxonomy tree, dumpalign with --reads
    parser.add_argument("--lineages", default=None, metavar="FILE",
                        help="the genomes' lineages, one line per genome: identifier<TAB>name;name;... (root first)")
    parser.add_argument("--lineage-report", default=None, metavar="FILE",
                        help="write one line per node of the lineage tree (reads in the clade, on the node) to FILE")
    # not in the reference: the selected reads written back out as FASTQ, dumpalign with --reads
    parser.add_argument("--containment", default=None, metavar="FILE",
                        help="write one line per genome (its distinct k-mers, those the reads hold, the containment "
                             "and identity from them) to FILE")
    parser.add_argument("--extract", default=None, metavar="FILE",
                        help="write the selected reads' FASTQ records to FILE, in file order")
    parser.add_argument("--extract-mapping", default=None, metavar="LIST",
                        help="read types to select, a comma list of unique, ambiguous, unmapped, filtered "
                             "(default: unique,ambiguous)")
    parser.add_argument("--extract-genomes", default=None,
                        help="comma-separated genome identifiers: select only mapped reads that name one of them")
    parser.add_argument("--extract-invert", action="store_true", help="select every read the selection leaves out")
    # not in the reference: the reads trimmed on the device before anything else sees them, align / dumpalign with --reads
    parser.add_argument("--trim-quality", type=int, default=None, metavar="Q",
                        help="cut the 3' end where the qualities fall below Q (a raw quality byte, as --min-read-quality)")
    parser.add_argument("--trim-quality5", type=int, default=None, metavar="Q", help="the same for the 5' end")
    parser.add_argument("--trim-adapter", default=None, metavar="SEQ",
                        help="cut a 3' adapter (1 .. 64 letters of ACGT) and everything after it")
    parser.add_argument("--trim-adapter2", default=None, metavar="SEQ",
                        help="the adapter of the second mates (--reads2; default: --trim-adapter's)")
    parser.add_argument("--trim-min-overlap", type=int, default=None, metavar="N",
                        help="bases of the adapter a read's end must hold (default: 3)")
    parser.add_argument("--trim-error-rate", type=float, default=None, metavar="X",
                        help="mismatches allowed per compared base, 0 .. 0.5 (default: 0.1)")
    parser.add_argument("--trim-report", default=None, metavar="FILE",
                        help="write the trim statistics (reads and bases in, out and cut) to FILE")
    return parser.parse_args(args)


def _load_reference(reference_file: str) -> KmerReference:
    try:
        return KmerReference.load(reference_file)
    except gzip.BadGzipFile:
        sys.exit("Error: Incorrect format of input file.")


def compact_for_job(reads_file: Optional[str], container, shards: int = 1) -> bool:
    """The reference of a one-FASTQ job gets the compact k-mer table
    (PA_BUILD_COMPACT) when the job has fewer than PA_COMPACT_READS_PER_BASE
    reads per genome base -- the reads counted high, one per 64 bytes of the
    file (4x that for gzip), over `shards` replicas."""
    env = os.environ.get("PA_COMPACT_TABLE")  # (A/B: 0 / 1 overrides the policy)
    if env in ("0", "1"):
        return env == "1"
    if not reads_file:
        return False
    import pa_native as N
    try:
        size = os.path.getsize(reads_file)
    except OSError:
        return False
    reads = (size * (4 if reads_file.endswith(".gz") else 1)) // 64 // max(shards, 1)
    bases = sum(len(g["genome"]) for g in container)
    return reads < N.PA_COMPACT_READS_PER_BASE * bases


def create_reference(fasta_file: str, kmer_size: int, filter_similar: bool = False,
                     similarity_threshold: float = 0.95, reads_file: Optional[str] = None,
                     both_strands: bool = False) -> KmerReference:
    container = FASTAFile(fasta_file).container
    _stage("fasta parsed")
    return KmerReference(kmer_size, container, filter_similar=filter_similar,
                         similarity_threshold=similarity_threshold,
                         compact_table=compact_for_job(reads_file, container), both_strands=both_strands)


def _check_strands(args: argparse.Namespace, ref) -> None:
    """--both-strands with -r: the stored property decides, and a forward-only
    file cannot serve the request."""
    if args.both_strands and not getattr(ref, "_both_strands", False):
        sys.exit(f"Error: --both-strands was given, but reference file '{args.referencefile}' is forward-only; "
                 "rebuild it with -t reference --both-strands.")


def _prefetch_reads(reads_file: str):
    """Start moving a plain FASTQ file into device memory (pa_fastq_prefetch_start)
    so that the copy overlaps the reference build; None where the file takes
    another path (a .gz or wrong extension, PA_STREAM=0 / PA_PREFETCH=0)."""
    if os.environ.get("PA_STREAM", "1") == "0" or os.environ.get("PA_PREFETCH", "1") == "0":
        return None
    if reads_file.endswith(".gz") or not any(reads_file.endswith(e) for e in FASTAQFile.EXTENSIONS):
        return None
    try:
        import pa_native as N
        global _EARLY_PREFETCH
        early = _EARLY_PREFETCH
        if early is not None and early[0] == os.path.abspath(reads_file):  # started at entry
            _EARLY_PREFETCH = None  # (owned by pf from here on)
            pf = N.FastqPrefetch.adopt(early[1], reads_file)
        else:
            pf = N.FastqPrefetch(reads_file)
    except Exception:  # (no device, unreadable file: the exact path reports it in the reference's order)
        return None
    atexit.register(pf.close)
    return pf


def create_alignment_from_reference(kmer_reference: KmerReference, reads_file: str, m: int, p: int,
                                    min_read_quality, min_kmer_quality, max_genomes,
                                    prefetch=None, per_read: bool = False,
                                    coverage: bool = False, assignments: bool = False,
                                    pileup: bool = False, min_base_quality=None,
                                    abundance: bool = False, lineages=None, extract=None,
                                    containment: bool = False, trim=None) -> PseudoAlignment:
    # the FASTQ file goes straight to the device (parsed there, aligned in
    # windows); a file outside that subset of the grammar is parsed the exact
    # way (FASTAQFile), which also raises the reference's errors.  per_read
    # (task 'align': the .aln file holds every read's result): the host parse,
    # whose records the per-read results are made from -- the device parse
    # would only have to be repeated on the host for them
    FASTAQFile.check_extension(reads_file)
    _stage("reference built")
    # coverage: the reads are parsed on the host and aligned on one device (align_reads_from_file
    # then takes its exact path: the placements need the read columns)
    # pileup: likewise (the base counts need the read columns); abundance: likewise (the candidate pass does)
    # lineages: likewise (its pass is the candidate pass); the tree is made over the index's genomes, now,
    # so that a genome without a lineage ends the job before a read is aligned
    # containment: likewise (the mark pass takes the read columns)
    # trim: every path below trims first -- the stream per window, the host-parsed ones per batch
    alignment = (PseudoAlignment(kmer_reference, coverage=coverage, pileup=pileup, min_base_quality=min_base_quality,
                                 abundance=abundance, lineages=lineages, containment=containment, trim=trim)
                 if coverage or pileup or abundance or lineages is not None or containment or trim is not None
                 else PseudoAlignment(kmer_reference))
    if lineages is not None:
        try:
            alignment._lineage_tree()
        except ValueError as err:
            sys.exit(f"Error: {err} in lineage file.")
    # extract: (out_file, mapping, genomes, invert) -- the selected records gathered on the device from the
    # device-parsed stream; with a per-read job above (or --assignments) the host-parsed records are selected
    if extract is not None:
        out_file, mapping, genomes, invert = extract
        stats = alignment.extract_reads_from_file(reads_file, out_file, mapping, genomes, invert, m, p,
                                                  min_read_quality, min_kmer_quality, max_genomes,
                                                  host_parsed=per_read or assignments)
        if _TIMING:
            print(f"[pa_cli] extract: {stats}", file=sys.stderr, flush=True)
    # assignments: the host parse too -- every read's line needs its id and the read columns
    elif per_read or assignments:
        alignment.align_reads_from_container(FASTAQFile(reads_file).container, m, p, min_read_quality,
                                             min_kmer_quality, max_genomes)
    else:
        alignment.align_reads_from_file(reads_file, m, p, min_read_quality, min_kmer_quality, max_genomes,
                                        prefetch=prefetch)
    _stage("reads aligned")
    return alignment


def create_alignment_from_pairs(kmer_reference: KmerReference, reads_file: str, reads2_file: str, m: int, p: int,
                                min_read_quality, min_kmer_quality, max_genomes, trim=(None, None)) -> PseudoAlignment:
    # a paired job: both files parsed on the host, one device, one entry per pair
    FASTAQFile.check_extension(reads_file)
    FASTAQFile.check_extension(reads2_file)
    _stage("reference built")
    alignment = (PseudoAlignment(kmer_reference) if trim == (None, None)
                 else PseudoAlignment(kmer_reference, trim=trim[0], trim2=trim[1] or trimming.Spec()))
    try:
        alignment.align_pairs_from_containers(FASTAQFile(reads_file).container, FASTAQFile(reads2_file).container,
                                              m, p, min_read_quality, min_kmer_quality, max_genomes)
    except ValueError as err:  # (unequal record counts, a pair whose ids differ, the reference's argument errors)
        sys.exit(f"Error: {err}")
    _stage("pairs aligned")
    return alignment


def _load_lineages(args: argparse.Namespace):
    """The --lineages file, parsed once (main() reads it before any device work); None without the flag."""
    if args.lineages is None:
        return None
    if getattr(args, "_lineages", None) is None:
        from lineage import Lineages
        try:
            args._lineages = Lineages.from_file(args.lineages)
        except ValueError as err:
            sys.exit(f"Error: {err}")
    return args._lineages


def _extract_job(args: argparse.Namespace):
    """(out_file, mapping, genomes, invert) of --extract; None without the flag."""
    if args.extract is None:
        return None
    genomes = None if args.extract_genomes is None else [x for x in args.extract_genomes.split(",") if x]
    return (args.extract, "unique,ambiguous" if args.extract_mapping is None else args.extract_mapping, genomes,
            args.extract_invert)


_TRIM_WHAT = "--trim-quality, --trim-quality5, --trim-adapter or --trim-adapter2"


def _trim_specs(args: argparse.Namespace):
    """(mate 1's trim.Spec, mate 2's) of the --trim-* flags, each None when it
    trims nothing; ValueError for an adapter or a number out of range."""
    if (args.trim_quality is None and args.trim_quality5 is None and args.trim_adapter is None
            and args.trim_adapter2 is None):
        return None, None
    overlap = trimming.DEFAULT_MIN_OVERLAP if args.trim_min_overlap is None else args.trim_min_overlap
    permille = trimming.DEFAULT_ERROR_PERMILLE
    if args.trim_error_rate is not None:
        if not 0 <= args.trim_error_rate <= 0.5:  # (false for NaN too)
            raise ValueError("the trim error rate must be between 0 and 0.5")
        permille = int(round(1000 * args.trim_error_rate))
    specs = []
    for adapter in (args.trim_adapter, args.trim_adapter if args.trim_adapter2 is None else args.trim_adapter2):
        spec = trimming.Spec(args.trim_quality, args.trim_quality5, adapter, overlap, permille)
        specs.append(spec if spec.active else None)
    return specs[0], specs[1]


def _write_trim_report(alignment: PseudoAlignment, args: argparse.Namespace) -> None:
    """--trim-report: one line of values, a second one for the second mates of a paired job."""
    if args.trim_report is None:
        return
    stats = [alignment.get_trim_stats(1) or trimming.new_stats()]
    if args.reads2 is not None:
        stats.append(alignment.get_trim_stats(2) or trimming.new_stats())
    with open(args.trim_report, "w") as fh:
        fh.write(trimming.report_text(stats))


def _print_json(obj) -> None:
    print(json.dumps(obj, indent=4))


def _dump_reference(ref: KmerReference) -> None:
    """print(json.dumps(ref.get_summary(), indent=4)) (src/main.py:121-127), the
    text streamed to stdout from the device index instead of built as a dict."""
    if not isinstance(ref, KmerReference):  # (another object in the file: its own summary, as the reference)
        _print_json(ref.get_summary())
        return
    sys.stdout.flush()
    fd = sys.stdout.fileno()
    ref.write_summary(fd)
    os.write(fd, b"\n")


def _check_task(args: argparse.Namespace) -> None:
    """Flag combinations (src/main.py:321-334), truthiness-based like the reference."""
    extra = (args.reads or args.alignfile or args.unique_threshold or args.ambiguous_threhold
             or args.min_read_quality or args.min_kmer_quality or args.max_genomes)
    if args.reads2 is not None:
        if not args.reads:
            sys.exit("Error: --reads2 needs --reads (the first mates' file).")
        if args.task not in ("align", "dumpalign"):
            sys.exit("Error: --reads2 is only allowed for tasks 'align' and 'dumpalign'.")
        if args.coverage or args.variants is not None or args.abundance is not None:
            sys.exit("Error: --reads2 cannot be combined with --coverage, --variants or --abundance "
                     "(those take single reads).")
    if not args.coverage and (args.genomes is not None or args.min_coverage is not None or args.full_coverage):
        sys.exit("Error: --genomes, --min-coverage and --full-coverage need --coverage.")
    if args.coverage:
        if args.task != "dumpalign" or not args.reads:
            sys.exit("Error: --coverage is only allowed for task 'dumpalign' with --reads.")
        if args.min_coverage is not None and args.min_coverage < 1:
            sys.exit("Error: --min-coverage must be at least 1.")
    if args.assignments is not None:
        if args.task != "dumpalign" or not args.reads:
            sys.exit("Error: --assignments is only allowed for task 'dumpalign' with --reads.")
        validate_file_writable(args.assignments, "Assignments output")
    if args.variants is None and any(v is not None for v in (args.variant_min_depth, args.variant_min_count,
                                                             args.variant_min_fraction,
                                                             args.variant_min_base_quality)):
        sys.exit("Error: --variant-min-depth, --variant-min-count, --variant-min-fraction and "
                 "--variant-min-base-quality need --variants.")
    if args.variants is not None:
        if args.task != "dumpalign" or not args.reads:
            sys.exit("Error: --variants is only allowed for task 'dumpalign' with --reads.")
        if args.variant_min_depth is not None and args.variant_min_depth < 1:
            sys.exit("Error: --variant-min-depth must be at least 1.")
        if args.variant_min_count is not None and args.variant_min_count < 1:
            sys.exit("Error: --variant-min-count must be at least 1.")
        if args.variant_min_fraction is not None and not 0 <= args.variant_min_fraction <= 1:
            sys.exit("Error: --variant-min-fraction must be in 0 .. 1.")
        if args.variant_min_base_quality is not None and args.variant_min_base_quality < 0:
            sys.exit("Error: --variant-min-base-quality must be at least 0.")
        validate_file_writable(args.variants, "Variants output")
    if args.abundance is None and (args.abundance_iterations is not None or args.abundance_tolerance is not None):
        sys.exit("Error: --abundance-iterations and --abundance-tolerance need --abundance.")
    if args.abundance is None and (args.abundance_bootstraps is not None or args.abundance_seed is not None
                                   or args.abundance_confidence is not None):
        sys.exit("Error: --abundance-bootstraps, --abundance-seed and --abundance-confidence need --abundance.")
    if args.abundance is not None:
        if args.task != "dumpalign" or not args.reads:
            sys.exit("Error: --abundance is only allowed for task 'dumpalign' with --reads.")
        if args.abundance_iterations is not None and not 1 <= args.abundance_iterations <= 10000:
            sys.exit("Error: --abundance-iterations must be in 1 .. 10000.")
        if args.abundance_tolerance is not None and not args.abundance_tolerance >= 0:
            sys.exit("Error: --abundance-tolerance must be at least 0.")
        if args.abundance_bootstraps is None and (args.abundance_seed is not None
                                                  or args.abundance_confidence is not None):
            sys.exit("Error: --abundance-seed and --abundance-confidence need --abundance-bootstraps.")
        if args.abundance_bootstraps is not None and not 1 <= args.abundance_bootstraps <= 10000:
            sys.exit("Error: --abundance-bootstraps must be in 1 .. 10000.")
        if args.abundance_seed is not None and not 0 <= args.abundance_seed <= 2 ** 64 - 1:
            sys.exit("Error: --abundance-seed must be in 0 .. 2^64 - 1.")
        if args.abundance_confidence is not None and not (  # (false for NaN too)
                0 < args.abundance_confidence < 1 and 1 <= int(round(1000 * args.abundance_confidence)) <= 999):
            sys.exit("Error: --abundance-confidence must be in 0.001 .. 0.999.")
        validate_file_writable(args.abundance, "Abundance output")
    if args.lineage_report is not None and args.lineages is None:
        sys.exit("Error: --lineage-report needs --lineages.")
    if args.lineages is not None:
        if args.lineage_report is None and args.assignments is None:
            sys.exit("Error: --lineages needs --lineage-report (or --assignments, whose lines then gain the taxon).")
        if args.task != "dumpalign" or not args.reads:
            sys.exit("Error: --lineages is only allowed for task 'dumpalign' with --reads.")
        if args.reads2 is not None:
            sys.exit("Error: --reads2 cannot be combined with --lineages (the lineage pass takes single reads).")
        validate_file_readable(args.lineages, "Lineages")
        if args.lineage_report is not None:
            validate_file_writable(args.lineage_report, "Lineage report output")
    if args.containment is not None:
        if args.task != "dumpalign" or not args.reads:
            sys.exit("Error: --containment is only allowed for task 'dumpalign' with --reads.")
        if args.reads2 is not None:
            sys.exit("Error: --reads2 cannot be combined with --containment (the containment pass takes single reads).")
        if args.alignfile:
            sys.exit("Error: --containment cannot be combined with -a.")
        validate_file_writable(args.containment, "Containment output")
    if args.extract is None and (args.extract_mapping is not None or args.extract_genomes is not None
                                 or args.extract_invert):
        sys.exit("Error: --extract-mapping, --extract-genomes and --extract-invert need --extract.")
    if args.extract is not None:
        try:
            extract_type_mask("unique,ambiguous" if args.extract_mapping is None else args.extract_mapping)
        except ValueError as err:
            sys.exit(f"Error: {err}.")
        if args.task != "dumpalign" or not args.reads:
            sys.exit("Error: --extract is only allowed for task 'dumpalign' with --reads.")
        if args.reads2 is not None:
            sys.exit("Error: --extract cannot be combined with --reads2 (pairs are not extracted).")
        if args.alignfile:
            sys.exit("Error: --extract cannot be combined with -a.")
        if os.path.exists(args.extract) and os.path.samefile(args.extract, args.reads) or (
                os.path.abspath(args.extract) == os.path.abspath(args.reads)):
            sys.exit("Error: --extract FILE is the --reads file.")
        validate_file_writable(args.extract, "Extract output")
    trim_flag = (args.trim_quality is not None or args.trim_quality5 is not None or args.trim_adapter is not None
                 or args.trim_adapter2 is not None)
    if not trim_flag and (args.trim_min_overlap is not None or args.trim_error_rate is not None):
        sys.exit(f"Error: --trim-min-overlap and --trim-error-rate need {_TRIM_WHAT}.")
    if not trim_flag and args.trim_report is not None:
        sys.exit(f"Error: --trim-report needs {_TRIM_WHAT}.")
    if trim_flag:
        if args.task not in ("align", "dumpalign") or not args.reads:
            sys.exit("Error: the --trim-* flags are only allowed for tasks 'align' and 'dumpalign' with --reads.")
        if args.trim_adapter2 is not None and args.reads2 is None:
            sys.exit("Error: --trim-adapter2 needs --reads2 (the second mates' file).")
        try:
            _trim_specs(args)
        except ValueError as err:
            sys.exit(f"Error: {err}.")
        if args.trim_report is not None:
            validate_file_writable(args.trim_report, "Trim report output")
    if args.task == "reference":
        if extra:
            sys.exit("Error: For task 'reference', only -g, -k, -r, --filter-similar, and --similarity-threshold "
                     "are allowed.")
    elif args.task == "dumpref":
        if extra:
            sys.exit("Error: For task 'dumpref', only -r or (-g and -k) with --filter-similar and "
                     "--similarity-threshold are allowed.")
    elif args.task == "align":
        if not ((args.referencefile and args.reads and args.alignfile)
                or (args.genomefile and args.kmer_size and args.reads and args.alignfile)):
            sys.exit("Error: For task 'align', provide either -r (reference file) or -g and -k (genome file and "
                     "kmer size) along with --reads and -a.")
    elif args.task == "dumpalign":
        if not ((args.referencefile and args.reads) or (args.genomefile and args.kmer_size and args.reads)
                or args.alignfile):
            sys.exit("Error: For task 'dumpalign', provide either -r and --reads, or -g, -k, and --reads, or -a.")
    else:
        sys.exit("Error: Unsupported task.")


def _dumpalign_sharded(args: argparse.Namespace, filt) -> Optional[PseudoAlignment]:
    """PA_GPUS=N > 1: the dumpalign job read-sharded over N devices (pa_shard:
    one index replica per device, one byte range of the FASTQ file each, the
    counters reduced on the host); None where it does not apply -- one GPU,
    a .gz or non-canonical file, a duplicate id across ranges -- and the
    one-GPU path runs (and raises the reference's errors)."""
    import pa_shard
    n, share = pa_shard.gpus_from_env()
    if n < 2 or args.reads.endswith(".gz"):
        return None
    FASTAQFile.check_extension(args.reads)
    devices = pa_shard.devices_for(n, share)
    if len(devices) < 2:
        return None
    container = FASTAFile(args.genomefile).container
    _stage("fasta parsed")
    refs = pa_shard.build_replicas(args.kmer_size, container, devices, args.filter_similar,
                                   args.similarity_threshold,
                                   compact_table=compact_for_job(args.reads, container, len(devices)),
                                   both_strands=args.both_strands)
    _stage(f"{len(refs)} references built")
    pa = pa_shard.align_sharded(refs, args.reads, *filt)
    _stage("reads aligned (sharded)" if pa is not None else "sharded path not taken")
    if pa is None:
        return None
    if _TIMING:
        print(f"[pa_cli] shards (offset, bytes, records): {pa._shards}", file=sys.stderr, flush=True)
    return pa


def _print_alignment(alignment: PseudoAlignment, args: argparse.Namespace) -> None:
    """The dumpalign JSON; with --coverage the "Coverage" (and "Details") objects after "Summary"."""
    out = alignment.get_summary()
    if args.coverage:
        genomes = None if args.genomes is None else [x for x in args.genomes.split(",") if x]
        out.update(alignment.get_coverage(genomes, args.min_coverage or 1, args.full_coverage))
    _print_json(out)
    if args.assignments is not None:
        with open(args.assignments, "w") as fh:
            alignment.write_assignments(fh)
    if args.variants is not None:
        with open(args.variants, "w") as fh:
            alignment.write_variants(fh, 4 if args.variant_min_depth is None else args.variant_min_depth,
                                     2 if args.variant_min_count is None else args.variant_min_count,
                                     0.2 if args.variant_min_fraction is None else args.variant_min_fraction)
    em = (200 if args.abundance_iterations is None else args.abundance_iterations,
          1e-9 if args.abundance_tolerance is None else args.abundance_tolerance,
          args.abundance_bootstraps or 0,
          1 if args.abundance_seed is None else args.abundance_seed,
          0.95 if args.abundance_confidence is None else args.abundance_confidence)
    if args.abundance is not None:
        with open(args.abundance, "w") as fh:
            alignment.write_abundance(fh, *em)
    if args.lineage_report is not None:  # (with --abundance: its estimates rolled up the tree, under the same settings)
        with open(args.lineage_report, "w") as fh:
            alignment.write_lineage_report(fh, *em)
    if args.containment is not None:
        with open(args.containment, "w") as fh:
            alignment.write_containment(fh)
    _write_trim_report(alignment, args)


def _run(args: argparse.Namespace) -> None:
    filt = (args.unique_threshold, args.ambiguous_threhold, args.min_read_quality, args.min_kmer_quality,
            args.max_genomes)
    trim = _trim_specs(args)
    if args.task == "reference":
        validate_file_readable(args.genomefile, "Genome FASTA")
        validate_file_writable(args.referencefile, "Reference database output")
        create_reference(args.genomefile, args.kmer_size, args.filter_similar,
                         args.similarity_threshold, both_strands=args.both_strands).save(args.referencefile)
    elif args.task == "dumpref":
        if args.referencefile:
            validate_file_readable(args.referencefile, "Reference database")
            _dump_reference(_load_reference(args.referencefile))
        elif args.genomefile and args.kmer_size:
            validate_file_readable(args.genomefile, "Genome FASTA")
            _dump_reference(create_reference(args.genomefile, args.kmer_size, args.filter_similar,
                                             args.similarity_threshold))
    elif args.task == "align":
        validate_file_readable(args.reads, "FASTQ reads")
        validate_file_writable(args.alignfile, "Alignment output")
        if args.referencefile and args.reads and args.alignfile:
            validate_file_readable(args.referencefile, "Reference database")
            ref = _load_reference(args.referencefile)
            _check_strands(args, ref)
        else:
            validate_file_readable(args.genomefile, "Genome FASTA")
            ref = create_reference(args.genomefile, args.kmer_size, args.filter_similar, args.similarity_threshold,
                                   reads_file=args.reads, both_strands=args.both_strands)
            # saved unconditionally, as src/main.py:370 does: without -r that is
            # gzip.open(None), a TypeError the reference does not catch
            # (src/main.py:401), so the command ends with a traceback and exit
            # status 1 before any alignment is written -- reproduced, not fixed
            ref.save(args.referencefile)
        if args.reads2 is not None:
            validate_file_readable(args.reads2, "FASTQ second-mate reads")
            alignment = create_alignment_from_pairs(ref, args.reads, args.reads2, *filt, trim=trim)
            alignment.save(args.alignfile)
            _write_trim_report(alignment, args)
            return
        alignment = create_alignment_from_reference(ref, args.reads, *filt, per_read=True, trim=trim[0])
        alignment.save(args.alignfile)
        _write_trim_report(alignment, args)
    elif args.task == "dumpalign":
        if args.referencefile and args.reads:
            validate_file_readable(args.reads, "FASTQ reads")
            if args.reads2 is not None:
                validate_file_readable(args.reads2, "FASTQ second-mate reads")
                ref = _load_reference(args.referencefile)
                _check_strands(args, ref)
                _print_alignment(create_alignment_from_pairs(ref, args.reads, args.reads2, *filt, trim=trim), args)
                return
            host_parsed = (args.coverage or args.assignments is not None or args.variants is not None
                           or args.abundance is not None or args.lineages is not None
                           or args.containment is not None)
            pf = None if host_parsed or args.extract is not None else _prefetch_reads(args.reads)
            ref = _load_reference(args.referencefile)
            _check_strands(args, ref)
            _print_alignment(create_alignment_from_reference(ref, args.reads, *filt, prefetch=pf,
                                                             coverage=args.coverage,
                                                             assignments=args.assignments is not None,
                                                             pileup=args.variants is not None,
                                                             min_base_quality=args.variant_min_base_quality,
                                                             abundance=args.abundance is not None,
                                                             lineages=_load_lineages(args),
                                                             extract=_extract_job(args),
                                                             containment=args.containment is not None,
                                                             trim=trim[0]), args)
        elif args.genomefile and args.kmer_size and args.reads:
            validate_file_readable(args.reads, "FASTQ reads")
            validate_file_readable(args.genomefile, "Genome FASTA")
            if args.reads2 is not None:  # (a paired job runs on one device, both files parsed on the host)
                validate_file_readable(args.reads2, "FASTQ second-mate reads")
                ref = create_reference(args.genomefile, args.kmer_size, args.filter_similar,
                                       args.similarity_threshold, reads_file=args.reads,
                                       both_strands=args.both_strands)
                _print_alignment(create_alignment_from_pairs(ref, args.reads, args.reads2, *filt, trim=trim), args)
                return
            # (a coverage job runs on one device: the depth arrays of read shards are not reduced;
            # an assignments job too: its lines come from one host-parsed batch; a pileup job and an
            # abundance job, as coverage)
            host_parsed = (args.coverage or args.assignments is not None or args.variants is not None
                           or args.abundance is not None or args.lineages is not None
                           or args.containment is not None)
            # (an extract job too: its output is written by one device, window after window)
            # (and a job with trim flags: the byte-range shards have no trimming form)
            sharded = (None if host_parsed or args.extract is not None or trim != (None, None)
                       else _dumpalign_sharded(args, filt))
            if sharded is not None:
                _print_json(sharded.get_summary())
                return
            pf = None if host_parsed or args.extract is not None else _prefetch_reads(args.reads)
            ref = create_reference(args.genomefile, args.kmer_size, args.filter_similar, args.similarity_threshold,
                                   reads_file=args.reads, both_strands=args.both_strands)
            _print_alignment(create_alignment_from_reference(ref, args.reads, *filt, prefetch=pf,
                                                             coverage=args.coverage,
                                                             assignments=args.assignments is not None,
                                                             pileup=args.variants is not None,
                                                             min_base_quality=args.variant_min_base_quality,
                                                             abundance=args.abundance is not None,
                                                             lineages=_load_lineages(args),
                                                             extract=_extract_job(args),
                                                             containment=args.containment is not None,
                                                             trim=trim[0]), args)
        elif args.alignfile:
            validate_file_readable(args.alignfile, "Alignment output")
            try:
                alignment = PseudoAlignment.load(args.alignfile)
            except gzip.BadGzipFile:
                sys.exit("Error: Incorrect format of input file.")
            _print_json(alignment.get_summary())
        else:
            sys.exit("Error: Provide either -g and -k with --reads, or -r with --reads, or -a.")
    else:
        sys.exit("Error: Unsupported task.")


def main(argv: Optional[List[str]] = None) -> None:
    _stage("imports done")
    args = parse_arguments(argv)
    _check_task(args)
    _load_lineages(args)  # (a file the parser refuses ends the job here)
    # falsy -> default, as src/main.py:337-342 (so -m 0 and -p 0 become 1)
    if not args.unique_threshold:
        args.unique_threshold = DEFAULT_UNIQUE_THRESHOLD
    if not args.ambiguous_threhold:
        args.ambiguous_threhold = DEFAULT_AMBIGUOUS_THRESHOLD
    if not args.similarity_threshold:
        args.similarity_threshold = DEFAULT_SIMILARITY_THRESHOLD
    try:
        _run(args)
        _stage("printed")
    except gzip.BadGzipFile:
        sys.exit("Error: Incorrect format of input file.")
    except (InvalidExtensionError, NoRecordsInDataFile, NotValidatingUniqueMapping, AddingExistingRead,
            ValueError) as err:
        sys.exit(err)


if __name__ == "__main__":
    main()
    # done: the output is flushed and the process ends without releasing the
    # device index allocation by allocation (the driver reclaims it at exit);
    # PA_FAST_EXIT=0 keeps the normal interpreter exit (profilers write their
    # results from exit handlers)
    if os.environ.get("PA_FAST_EXIT", "1") != "0":
        _stage("exit")
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
