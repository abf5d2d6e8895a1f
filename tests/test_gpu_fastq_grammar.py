"""The device FASTQ parser (csrc/pa_fastq.hip) against the reference grammar.

Truth for a file: its text as data_file.load_file reads it (text mode, UTF-8,
universal newlines; gzip.open for .gz), parsed by the regex grammar
(FASTAQRecordContainer._parse_regex -- the host native parser is not part of
the oracle) and aligned by align_reads_from_container: the summary as JSON
text, or the exception's type name.  Every file then goes through
align_reads_from_file -- the windowed stream, the prefetched form
(N.FastqPrefetch, 4 KiB copy chunks) and, as BGZF, the gzip stream -- and must
(a) give the truth and (b) report the verdict the CPU model of the
device-parsed subset (fastq_cases.in_device_subset) predicts:
_streamed_records == the model's record count, or None when the model rejects.

The index and the reads (fastq_cases) make every parsed byte count: a wrong
base unmaps a read, a wrong quality byte moves filtered_quality_reads.
tests/test_fastq_model_host.py holds the CPU side: the model against the regex
grammar, and what the generated files cover."""

import gzip
import hashlib
import json
import time

import numpy as np
import pytest

import fastq_cases as C
import pa_native as N
import records as R
import synth
from data_file import FASTAQFile, NoRecordsInDataFile
from kmer import KmerReference, PseudoAlignment

pytestmark = pytest.mark.gpu

W = C.WINDOW
GRAMMAR_ERRORS = (R.NoRecordsInData, R.InvalidRecordData, R.DuplicateRecordError, R.UnparsedDataError,
                  NoRecordsInDataFile, UnicodeDecodeError)
PATHS = ("window", "prefetch", "bgzf")


@pytest.fixture(scope="module")
def ref():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible (no CPU fallback exists)")
    c = R.FASTARecordContainer()
    c.parse_records(C.genomes_fasta())
    return KmerReference(C.K, c)


@pytest.fixture(scope="module")
def ref_long():
    """Genomes long enough to cut reads of 20 000 bases from (k = 31)."""
    gens = synth.family_genomes(4, 30000, seed=5, family_size=2, sub_rate=0.02, conserved_len=800)
    c = R.FASTARecordContainer()
    c.parse_records(synth.fasta_text([f"L{i} long genome" for i in range(len(gens))], gens, width=70))
    return gens, KmerReference(31, c)


@pytest.fixture(autouse=True)
def small_windows(monkeypatch):
    monkeypatch.setenv("PA_STREAM_WINDOW", str(W))
    monkeypatch.setenv("PA_PREFETCH_CHUNK", "4096")


_PARSED = {}  # text digest -> the regex grammar's container, or its exception's type name
_TRUTH = {}   # (reference, text digest, arguments) -> outcome


def truth(ref, path, **kw) -> str:
    try:
        with (gzip.open if path.endswith(".gz") else open)(path, "rt", encoding="utf-8") as f:
            text = f.read()
    except UnicodeDecodeError:
        with pytest.raises(Exception) as ei:
            FASTAQFile(path)
        return type(ei.value).__name__
    digest = hashlib.sha1(text.encode("utf-8")).digest()
    key = (id(ref), digest, tuple(sorted(kw.items())))
    if key in _TRUTH:
        return _TRUTH[key]
    if digest not in _PARSED:
        c = R.FASTAQRecordContainer()
        try:
            c._parse_regex(text)
            _PARSED[digest] = c
        except GRAMMAR_ERRORS as e:
            name = type(e).__name__
            _PARSED[digest] = "NoRecordsInDataFile" if name == "NoRecordsInData" else name
    c = _PARSED[digest]
    if isinstance(c, str):
        out = c
    else:
        a = PseudoAlignment(ref)
        a.align_reads_from_container(c, **kw)
        out = json.dumps(a.get_summary(), indent=4)
    _TRUTH[key] = out
    return out


def outcome(ref, path, prefetch, **kw):
    """(summary text or exception name, _streamed_records or None) of align_reads_from_file."""
    a = PseudoAlignment(ref)
    try:
        a.align_reads_from_file(path, prefetch=N.FastqPrefetch(path) if prefetch else None, **kw)
    except GRAMMAR_ERRORS as e:
        return type(e).__name__, None
    return json.dumps(a.get_summary(), indent=4), getattr(a, "_streamed_records", None)


def write_case(tmp_path, name, data, how):
    """The bytes as a file for one of PATHS ("gzip": one gzip member); returns (path, prefetch?)."""
    if how == "bgzf":
        p = tmp_path / (name + ".fq.gz")
        p.write_bytes(synth.bgzf_bytes(data, level=1, block=W))  # members of one window of text
    elif how == "gzip":
        p = tmp_path / (name + ".fq.gz")
        p.write_bytes(gzip.compress(data, compresslevel=1))
    else:
        p = tmp_path / (name + ".fq")
        p.write_bytes(data)
    return str(p), how == "prefetch"


def check(ref, tmp_path, name, data, how, verdict=True, **kw):
    path, prefetch = write_case(tmp_path, name, data, how)
    want = truth(ref, path, **kw)
    got, streamed = outcome(ref, path, prefetch, **kw)
    assert got == want, (name, how, kw)
    if verdict:
        model = C.in_device_subset(data)
        assert streamed == (None if model is None else len(model)), (name, how, kw)
    return streamed


# ---- 1. differential fuzz -----------------------------------------------------------

def test_differential_fuzz(ref, tmp_path):
    """N_FUZZ small random and mutated files (the seeds whose shares
    test_fastq_model_host.py asserts), the windowed and the prefetched path in
    turn.  Prints the measured cost per file of align_reads_from_file."""
    spent = 0.0
    for i in range(C.N_FUZZ):
        data = C.fuzz_case(i)
        path, prefetch = write_case(tmp_path, f"fuzz{i}", data, PATHS[i % 2])
        want = truth(ref, path, **C.KW)
        t = time.perf_counter()
        got, streamed = outcome(ref, path, prefetch, **C.KW)
        spent += time.perf_counter() - t
        assert got == want, (i, PATHS[i % 2], data)
        model = C.in_device_subset(data)
        assert streamed == (None if model is None else len(model)), (i, PATHS[i % 2], data)
    print(f"fuzz: {C.N_FUZZ} files, {1e3 * spent / C.N_FUZZ:.2f} ms per file in align_reads_from_file")


# ---- 2. boundary sweep --------------------------------------------------------------

@pytest.mark.parametrize("how", PATHS)
def test_boundary_sweep(ref, tmp_path, how):
    """About 2.3 windows of sensitive records, the first id padded byte by byte
    so that offset 65536 walks over a whole record and every 16-byte phase,
    with and without the final line feed in turn
    (test_sweep_covers_every_structural_position_at_the_window_edge)."""
    t = time.perf_counter()
    pads = C.sweep_pads()
    for pad in pads:
        data = C.sweep_case(pad)
        at = (C.structure_at(data, W - 1), C.structure_at(data, W))
        path, prefetch = write_case(tmp_path, "sweep", data, how)
        want = truth(ref, path, **C.KW)
        got, streamed = outcome(ref, path, prefetch, **C.KW)
        assert got == want, (pad, how, at)
        assert streamed == len(C.sweep_records(pad)), (pad, how, at)
    print(f"sweep[{how}]: {len(pads)} files, {1e3 * (time.perf_counter() - t) / len(pads):.2f} ms per file with its truth")


# ---- 3. late violations -------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.VIOLATIONS))
def test_late_violation(ref, tmp_path, name):
    """A violation first seen after window 0 has been aligned: the partial
    result must be discarded and the exact path's outcome returned; a clean
    file parsed next on the same reference streams and equals its truth."""
    n = 0
    for placement in C.PLACEMENTS:
        data, _ = C.late_case(name, placement)
        for how in PATHS:
            assert check(ref, tmp_path, f"{name}_{placement}", data, how, **C.KW) is None
            clean = C.clean_case(n % 3)
            assert check(ref, tmp_path, "clean", clean, how, **C.KW) == 120
            n += 1


# ---- 4. extremes --------------------------------------------------------------------

@pytest.mark.parametrize("how", PATHS)
def test_dense_windows(ref, tmp_path, how):
    """20 000 records of nine to twelve bytes: thousands of records in every
    64 KiB window (the multi-block record scan, the id set near its load)."""
    assert check(ref, tmp_path, "dense", C.dense_case(), how, **C.KW) == 20000


def _long_reads_text(gens, lens, seed):
    parts = []
    for i, n_b in enumerate(lens):
        seq, qual, _ = synth.sample_reads(gens, 1, n_b, seed=seed * 1000 + i, err_rate=0.02)
        parts.append(b"@L%d len=%d\n%s\n+\n%s\n" % (i, n_b, bytes(seq[0]), bytes(qual[0])))
    return b"".join(parts)


LONG_KW = [dict(), dict(m=2, p=0, min_read_quality=58, min_kmer_quality=60, max_genomes=2)]


@pytest.mark.parametrize("window", [None, W])
def test_long_reads(ref_long, tmp_path, monkeypatch, window):
    """Reads of 177, 700, 1500 and 20 000 bases among reads of 150, at the
    default window and at 64 KiB (no record is longer than a window)."""
    gens, r = ref_long
    if window is None:
        monkeypatch.delenv("PA_STREAM_WINDOW")
    data = _long_reads_text(gens, [150, 177, 150, 700, 150, 1500, 150, 20000] * 4, seed=81)
    for kw in LONG_KW:
        for how in PATHS:
            assert check(r, tmp_path, "long", data, how, **kw) == 32


@pytest.mark.parametrize("n_bases", [70_000, 1_200_000])
def test_one_over_long_record(ref_long, tmp_path, n_bases):
    """A record longer than a window (and, at 1.2 M bases, than the longest
    carried tail) in mid-file: whichever parser takes the file, the outcome is
    the truth.  The verdict depends on where the record starts
    (parse_align_window: R == 0 && !last; align_fastq_file: kCarryMax) and is
    not asserted."""
    gens, r = ref_long
    rng = np.random.default_rng(n_bases)
    seq = np.tile(gens[1], n_bases // len(gens[1]) + 1)[:n_bases]
    qual = rng.integers(40, 75, size=n_bases).astype(np.uint8)
    data = (_long_reads_text(gens, [150] * 300, seed=82)
            + b"@over-long\n%s\n+\n%s\n" % (bytes(seq), bytes(qual))
            + _long_reads_text(gens, [150] * 300, seed=83).replace(b"@L", b"@M"))
    for how in PATHS:
        check(r, tmp_path, "overlong", data, how, verdict=False, **LONG_KW[1])


@pytest.mark.parametrize("size,final_lf", [(2 * W, True), (2 * W, False), (3 * W, True), (3 * W, False),
                                           (2 * W + 1, True)])
def test_text_length_at_the_window_edge(ref, tmp_path, size, final_lf):
    """Texts that end exactly with a window (or one line feed after it): for a
    gzip stream the end of the file is learnt one read late, so the last
    window is empty or holds only the carried tail."""
    data = C.sized_case(size, final_lf)
    n = len(C.in_device_subset(data))
    for how in PATHS + ("gzip",):
        assert check(ref, tmp_path, "sized", data, how, **C.KW) == n


@pytest.mark.parametrize("how", ["window", "prefetch"])
def test_empty_and_single_record_files(ref, tmp_path, how):
    assert check(ref, tmp_path, "empty", b"", how, **C.KW) is None
    assert check(ref, tmp_path, "lf_only", b"\n", how, **C.KW) is None
    one = C.sensitive_records(1, 91)
    for final_lf in (True, False):
        assert check(ref, tmp_path, "one", C.join_records(one, final_lf), how, **C.KW) == 1


THRESHOLDS = [None, C.Q - 1, C.Q, C.Q + 1]


@pytest.mark.parametrize("mrq", THRESHOLDS)
def test_q_min_at_the_threshold(ref, tmp_path, mrq):
    """Every quality byte is at least Q except one byte Q - 1 in a record of
    the last window: the parser's own q_min, from which the align layer elides
    the quality thresholds, must see that byte."""
    data, _ = C.threshold_case()
    n = len(C.in_device_subset(data))
    for mkq in THRESHOLDS:
        kw = {k: v for k, v in dict(min_read_quality=mrq, min_kmer_quality=mkq).items() if v is not None}
        for how in ("window", "prefetch") + (("bgzf",) if mkq == mrq else ()):
            assert check(ref, tmp_path, "threshold", data, how, **kw) == n
