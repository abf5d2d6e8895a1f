"""Read trimming on the device (pa_reads_trim, the pa_*_fastq_*_ex streams,
csrc/pa_trim.hip) against the plain-Python model of
trim.py (checked on its own in tests/test_trim_host.py) and the unchanged CPU
oracle fed with the model-trimmed columns.  Every comparison is for exact
equality.  The yardstick: everything downstream sees the trimmed read as if the
file had held it.

The world: the eight family genomes of test_gpu_extract.py (k = 31); 3000 reads
of twelve lengths and two of 5000 bases, in kinds -- clean, a bad 3' tail, a bad
5' head, an adapter planted at a random insert (half with one substitution,
some cut off by the read's end), an adapter with one mismatch too many, all
bad, dim (above the trim cutoff, below the quality filters) -- and 200 chimeric
reads (75 + 75 bases of two genomes) whose second half has bad qualities.  The populations the comparisons stand on are asserted from
the model and the oracle alone before anything is compared.
"""

import functools
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pa_native as N
import pa_oracle as O
import synth
import test_pairs_host as M
import trim as T
from kmer import KmerReference, PseudoAlignment
from records import FASTARecordContainer
from test_extract_host import AMBIGUOUS, MAIN, MAPPED, UNMAPPED, extract_model, lists_of, records_of, spec_of

pytestmark = pytest.mark.gpu

K = 31
LENS = (1, 20, 31, 63, 64, 65, 100, 129, 150, 176, 250, 1000)
KINDS = ("clean", "tail", "head", "adapter", "adapter", "too_many", "all_bad", "dim")
TRUSEQ = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
ADAPTER2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
QCUT = 55
FULL = T.Spec(QCUT, QCUT, TRUSEQ)
QUALITY = dict(min_read_quality=58, min_kmer_quality=60, max_genomes=2)  # (test_gpu_extract.QUALITY)
STREAM_ENV = {"PA_STREAM_WINDOW": "65536"}
TRIM_FLAGS = ["--trim-quality", str(QCUT), "--trim-quality5", str(QCUT), "--trim-adapter", TRUSEQ.decode()]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- the world ------------------------------------------------------------------------------------

def substitute(rng, a, at):
    a[at] = int(ACGT[(b"ACGT".index(a[at]) + int(rng.integers(1, 4))) % 4])


def mismatches(read, p, limit):
    """Mismatches of the whole adapter at p, counted up to `limit`."""
    mm = 0
    for j in range(len(TRUSEQ)):
        if read[p + j] != TRUSEQ[j]:
            mm += 1
            if mm >= limit:
                break
    return mm


def make_records(gens, allow_empty, seed=2200):
    """[(id, sequence, qualities)] as bytes.  allow_empty False: a read the full spec would empty is
    replaced by an untouched one (a FASTQ record cannot hold an empty read)."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(3002):
        n = 5000 if i >= 3000 else LENS[i % len(LENS)]
        kind = "tail" if i >= 3000 else KINDS[(i // len(LENS)) % len(KINDS)]
        g, at = int(rng.integers(0, 8)), int(rng.integers(0, 30000 - n))
        seq = bytearray(bytes(gens[g][at:at + n]).replace(b"N", b"A"))
        qual = bytearray(rng.integers(60, 74, n, dtype=np.uint8))
        if kind == "tail":
            t = int(rng.integers(0, n))
            qual[t:] = bytes(rng.integers(35, 51, n - t, dtype=np.uint8))
        elif kind == "head":
            h = int(rng.integers(1, max(2, n // 2)))
            qual[:h] = bytes(rng.integers(35, 51, h, dtype=np.uint8))
        elif kind == "adapter":
            p = int(rng.integers(0, n))
            a = bytearray(TRUSEQ)
            if i % 2 and n - p >= 10:  # one substitution inside the part the read keeps
                substitute(rng, a, int(rng.integers(0, min(n - p, len(a)))))
            seq[p:] = (a + bytearray(rng.choice(ACGT, size=n)))[:n - p]
        elif kind == "too_many" and n >= 63:  # four substitutions in a whole adapter: three are allowed
            p = int(rng.integers(0, n - len(TRUSEQ) + 1))
            a = bytearray(TRUSEQ)
            for at2 in rng.choice(len(a), size=4, replace=False):
                substitute(rng, a, int(at2))
            seq[p:p + len(a)] = a
        elif kind == "all_bad":
            qual = bytearray(rng.integers(35, 51, n, dtype=np.uint8))
        elif kind == "dim":  # above the trim cutoff, below QUALITY's thresholds: untouched, then filtered
            qual = bytearray(rng.integers(56, 60, n, dtype=np.uint8))
        recs.append((b"r%d %s len=%d" % (i, kind.encode(), n), bytes(seq), bytes(qual)))
    for i in range(200):
        a = int(rng.integers(0, 8))
        b = (a + 4) % 8
        pa, pb = int(rng.integers(0, 30000 - 75)), int(rng.integers(0, 30000 - 75))
        seq = (bytes(gens[a][pa:pa + 75]) + bytes(gens[b][pb:pb + 75])).replace(b"N", b"A")
        recs.append((b"chim%d %d+%d" % (i, a, b), seq, bytes([70]) * 75 + bytes([40]) * 75))
    if not allow_empty:
        for i, (rid, seq, qual) in enumerate(recs):
            s, e, _ = T.trim_read(seq, qual, FULL)
            if s == e:
                recs[i] = (rid, b"C" * len(seq), bytes([70]) * len(seq))
    return recs


def columns(recs):
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    np.cumsum([len(r[1]) for r in recs], out=off[1:])
    return b"".join(r[1] for r in recs), b"".join(r[2] for r in recs), off


def fastq(recs):
    return b"".join(b"@%s\n%s\n+\n%s\n" % r for r in recs)


def oracle_kw(kw):
    return dict(m=kw.get("m", 1), p=kw.get("p", 1), mrq=kw.get("min_read_quality"), mkq=kw.get("min_kmer_quality"),
                mg=kw.get("max_genomes"))


@functools.lru_cache(maxsize=None)
def genomes():
    return synth.family_genomes(8, 30000, seed=5, family_size=4, sub_rate=0.02, conserved_len=800)


class World:
    def __init__(self):
        self.gens = genomes()
        self.names = [f"g{i}" for i in range(8)]
        self.oracle = O.OracleIndex(self.gens, K)
        self.recs = make_records(self.gens, True)
        self.seq, self.qual, self.off = columns(self.recs)
        self._model, self._oracle = {}, {}

    def model(self, spec=FULL, key="full"):
        """trim.trim_columns of the world under the spec: (seq, qual, off, start, end, stats)."""
        if key not in self._model:
            self._model[key] = T.trim_columns(self.seq, self.qual, self.off, spec)
        return self._model[key]

    def aligned(self, kw, trimmed=True):
        """The oracle's result on the model-trimmed (or the original) columns."""
        key = (json.dumps(kw, sort_keys=True), trimmed)
        if key not in self._oracle:
            s, q, o = self.model()[:3] if trimmed else (self.seq, self.qual, self.off)
            self._oracle[key] = self.oracle.align(s, q, np.asarray(o, dtype=np.uint64), **oracle_kw(kw))
        return self._oracle[key]

    def populations(self):
        """The reads per population, from the model and the oracle alone."""
        ms, mq, moff, starts, ends, _ = self.model()
        pop = dict.fromkeys(("q3", "q5", "inside", "end_only", "with_mismatch", "rejected_by_one", "empty",
                             "below_k", "untouched"), 0)
        for (rid, seq, qual), s, e in zip(self.recs, starts, ends):
            n = len(seq)
            start, cut = T.quality_bounds(qual, QCUT, QCUT)
            pop["q3"] += T.quality_bounds(qual, QCUT, None)[1] < n
            pop["q5"] += T.quality_bounds(qual, None, QCUT)[0] > 0
            pop["empty"] += n > 0 and s == e
            pop["below_k"] += n >= K and e - s < K
            pop["untouched"] += n > 0 and e - s == n
            if start >= cut:
                continue
            read = seq[start:cut]
            if e < cut:  # a hit at p
                p = e - s
                ov = min(len(read) - p, len(TRUSEQ))
                pop["inside" if ov == len(TRUSEQ) else "end_only"] += 1
                pop["with_mismatch"] += any(read[p + j] != TRUSEQ[j] for j in range(ov))
            elif len(read) >= len(TRUSEQ):  # no hit: a whole-adapter candidate one mismatch over the limit?
                allowed = FULL.max_error_permille * len(TRUSEQ) // 1000
                pop["rejected_by_one"] += any(mismatches(read, p, allowed + 2) == allowed + 1
                                              for p in range(len(read) - len(TRUSEQ) + 1))
        before, after = self.aligned({}, False), self.aligned({})
        pop["type_changed"] = int((before.types != after.types).sum())
        return pop


@functools.lru_cache(maxsize=None)
def the_world():
    w = World()
    pop = w.populations()
    print("populations:", pop)
    for name, count in pop.items():
        assert count >= (50 if name == "type_changed" else 100), (name, count, pop)
    return w


@pytest.fixture(scope="module")
def world():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible (no CPU fallback exists)")
    return the_world()


@pytest.fixture(scope="module")
def ref(world):
    c = FASTARecordContainer()
    c.parse_records(synth.fasta_text(world.names, world.gens, width=70))  # (the headers of files["fa"])
    return KmerReference(K, c)


@pytest.fixture(scope="module")
def files(world, tmp_path_factory):
    """The files of the command-line checks: the genomes, the world's reads, and the variant without
    emptied reads next to the FASTQ file the model wrote pre-trimmed."""
    d = tmp_path_factory.mktemp("trim")
    fa = d / "g.fa"
    fa.write_text(synth.fasta_text(world.names, world.gens, width=70))
    (d / "reads.fq").write_bytes(fastq(world.recs))
    with gzip.open(d / "reads.fq.gz", "wb") as f:
        f.write(fastq(world.recs))
    kept = make_records(world.gens, False)
    (d / "kept.fq").write_bytes(fastq(kept))
    seq, qual, off = columns(kept)
    ts, tq, toff, _, _, stats = T.trim_columns(seq, qual, off, FULL)
    assert stats["reads_empty"] == 0 and stats["reads_trimmed"] >= 1500
    pre = [(r[0], ts[toff[i]:toff[i + 1]], tq[toff[i]:toff[i + 1]]) for i, r in enumerate(kept)]
    (d / "pretrimmed.fq").write_bytes(fastq(pre))
    return {"dir": d, "fa": str(fa), "reads": str(d / "reads.fq"), "gz": str(d / "reads.fq.gz"),
            "kept": str(d / "kept.fq"), "pretrimmed": str(d / "pretrimmed.fq"), "kept_stats": stats}


def upload(seq, qual, off, device=None):
    return N.Reads.upload(np.frombuffer(seq, dtype=np.uint8), np.frombuffer(qual, dtype=np.uint8),
                          np.asarray(off, dtype=np.uint64), device=device)


def run_main(argv, env=None):
    return subprocess.run([sys.executable, MAIN] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                          env=dict(os.environ, **(env or {})))


def ok(run):
    assert run.returncode == 0, run.stderr.decode(errors="replace")
    return run


# ---- 1. pa_reads_trim against the model -------------------------------------------------------------

SPECS = {
    "identity": T.Spec(),
    "quality3": T.Spec(quality3=QCUT),
    "quality5": T.Spec(quality5=QCUT),
    "adapter": T.Spec(adapter=TRUSEQ),
    "full": FULL,
    "adapter_1": T.Spec(QCUT, QCUT, TRUSEQ[:1], 1),
    "adapter_3": T.Spec(QCUT, QCUT, TRUSEQ[:3]),
    "adapter_64": T.Spec(QCUT, QCUT, (TRUSEQ + ADAPTER2)[:64]),
    "overlap_1": T.Spec(QCUT, QCUT, TRUSEQ, 1),
    "overlap_12": T.Spec(QCUT, QCUT, TRUSEQ, 12),
    "permille_0": T.Spec(QCUT, QCUT, TRUSEQ, 3, 0),
    "permille_500": T.Spec(QCUT, QCUT, TRUSEQ, 3, 500),
}


def check_trim(reads, spec, want):
    ms, mq, moff, starts, ends, stats = want
    out, st, en, got = reads.trim(spec.native())
    try:
        ds, dq, doff = out.download()
        assert doff.tolist() == list(moff)
        assert ds.tobytes() == ms and dq.tobytes() == mq
        assert st.tolist() == starts and en.tolist() == ends
        assert got == stats
        assert (out.n, out.n_bases, out.max_len) == (len(starts), len(ms), max(np.diff(moff), default=0))
    finally:
        out.close()


@pytest.mark.parametrize("name", list(SPECS))
def test_reads_trim_equals_the_model(world, name):
    reads = upload(world.seq, world.qual, world.off)
    try:
        check_trim(reads, SPECS[name], world.model(SPECS[name], name))
    finally:
        reads.close()
    if name == "identity":
        ms, mq, moff = world.model(SPECS[name], name)[:3]
        assert (ms, mq, list(moff)) == (world.seq, world.qual, world.off.tolist())


def test_non_acgt_bytes_and_a_long_read(world):
    """N (and any other byte) inside the overlap always mismatches; a read of 70000 bases whose only hit
    lies past the first thousand chunks, behind a bad 5' head longer than a chunk."""
    rng = np.random.default_rng(5)
    recs, planted = [], []
    for i in range(300):
        n = int(rng.integers(40, 200))
        seq = bytearray(rng.choice(ACGT, size=n))
        p = int(rng.integers(0, n - 20))
        a = bytearray(TRUSEQ)
        for at in rng.choice(20, size=1 + i % 5, replace=False):  # (three mismatches pass a whole adapter)
            a[int(at)] = ord("N") if i % 2 else ord("n")
        seq[p:] = (a + bytearray(rng.choice(ACGT, size=n)))[:n - p]
        recs.append((b"", bytes(seq), bytes([70]) * n))
        planted.append(p)
    long_seq = bytearray(b"C" * 70000)
    long_seq[66001:66001 + 33] = TRUSEQ
    long_qual = bytearray([70]) * 70000
    long_qual[:200] = bytes([36]) * 200
    long_qual[69000:] = bytes([36]) * 1000
    recs.append((b"", bytes(long_seq), bytes(long_qual)))
    seq, qual, off = columns(recs)
    want = T.trim_columns(seq, qual, off, FULL)
    assert (want[3][-1], want[4][-1]) == (200, 66001)
    accepted = sum(e == p for e, p in zip(want[4], planted))
    assert accepted >= 50 and len(planted) - accepted >= 50  # (an adapter with such bytes taken, and refused)
    reads = upload(seq, qual, off)
    try:
        check_trim(reads, FULL, want)
    finally:
        reads.close()


def test_three_batches_add_up(world):
    """The statistics are sums over reads: three batches accumulate to the one-batch values."""
    want = world.model()
    total = N.TrimStats()
    cuts = [0, 1000, 1001, len(world.recs)]
    parts = []
    for a, b in zip(cuts, cuts[1:]):
        lo, hi = int(world.off[a]), int(world.off[b])
        reads = upload(world.seq[lo:hi], world.qual[lo:hi], world.off[a:b + 1] - world.off[a])
        try:
            out, _, _, _ = reads.trim(FULL.native(), stats=total)
            parts.append(out.download()[0].tobytes())
            out.close()
        finally:
            reads.close()
    assert total.as_dict() == want[5]
    assert b"".join(parts) == want[0]


def test_empty_batch_and_einval(world):
    reads = upload(b"", b"", [0])
    out, st, en, stats = reads.trim(FULL.native())
    assert (out.n, out.n_bases, len(st), len(en)) == (0, 0, 0, 0) and stats == T.new_stats()
    out.close()
    reads.close()
    reads = upload(b"ACGT", b"IIII", [0, 4])
    try:
        def spec(**kw):
            s = FULL.native()
            for k, v in kw.items():
                setattr(s, k, v)
            return s
        bad_adapter = FULL.native()
        bad_adapter.adapter = TRUSEQ[:10] + b"N" + TRUSEQ[11:]
        for bad in (spec(flags=8), spec(flags=0x80000007), spec(adapter_len=0), spec(adapter_len=65), bad_adapter,
                    spec(min_overlap=0), spec(max_error_permille=501), spec(quality3=256), spec(quality5=256),
                    spec(flags=0, min_overlap=0), spec(flags=0, max_error_permille=501), spec(flags=0, quality3=256)):
            with pytest.raises(ValueError):
                reads.trim(bad)
        # what the flags do not ask for is not looked at
        out, st, en, _ = reads.trim(spec(flags=N.PA_TRIM_QUALITY3, adapter_len=0))
        assert (st.tolist(), en.tolist()) == ([0], [4])
        out.close()
    finally:
        reads.close()


# ---- 2. everything downstream sees the trimmed read -------------------------------------------------

@pytest.mark.parametrize("kw", [{}, QUALITY], ids=["default", "quality"])
def test_align_on_the_trimmed_batch(world, ref, kw):
    want = world.aligned(kw)
    index = ref.index
    reads = upload(world.seq, world.qual, world.off, index.device)
    out, _, _, _ = reads.trim(FULL.native())
    try:
        prm = N.Params.make(**kw)
        res = N.Result(index)
        N.align(index, out, prm, 0, res)
        stats, uq, am, fk = res.fetch()
        res.close()
        assert stats.tolist() == want.stats.tolist()
        assert uq.tolist() == want.unique.tolist() and am.tolist() == want.ambiguous.tolist()
        types, qf, hr, loff, lists = N.align_reads(index, out, prm)
        assert types.tolist() == want.types.tolist()
        assert qf.tolist() == want.qf.tolist() and hr.tolist() == want.hr.tolist()
        assert lists_of(loff, lists) == lists_of(want.list_off, want.lists)
        empty = np.flatnonzero(np.diff(np.asarray(world.model()[2])) == 0)
        assert len(empty) >= 100 and set(types[empty].tolist()) == {UNMAPPED}  # (kept, no windows)
    finally:
        out.close()
        reads.close()


def test_containment_on_the_trimmed_batch(world, ref):
    """One accumulator fed the device-trimmed batch against the same one fed the model-trimmed columns."""
    index = ref.index
    prm = N.Params.make(**QUALITY)
    reads = upload(world.seq, world.qual, world.off, index.device)
    out, _, _, _ = reads.trim(FULL.native())
    model = upload(*world.model()[:3], index.device)
    a, b = N.Containment(index), N.Containment(index)
    try:
        a.add(out, prm)
        b.add(model, prm)
        def plain(counts):
            arrays, info = counts
            return {n: v.tolist() for n, v in arrays.items()}, info
        ca, cb = plain(a.counts()), plain(b.counts())
        assert ca == cb and ca[1]["windows_retained"] > 100000
        c = N.Containment(index)
        c.add(reads, prm)  # (the untrimmed reads hold other windows: the comparison can fail)
        cc = plain(c.counts())
        c.close()
        assert cc != ca
    finally:
        a.close()
        b.close()
        out.close()
        model.close()
        reads.close()


# ---- 3. the stream path ------------------------------------------------------------------------------

def summary_text(world, kw):
    return json.dumps(O.summary_by_walk(world.aligned(kw), world.names, **{k: v for k, v in oracle_kw(kw).items()
                                                                           if k in ("mrq", "mkq", "mg")}), indent=4) + "\n"


def quality_flags(kw):
    return [x for k, v in kw.items() for x in ("--" + k.replace("_", "-"), str(v))]


TIMED_ENV = dict(STREAM_ENV, PA_STREAM_TIMING="1")  # (the library names the stream it ran, on stderr)


def streamed(run, records):
    """The device-parsed stream read the whole file (its own line on stderr says so, for the windowed
    and for the prefetched form): the command did not fall back to the host parser, whose batches are
    trimmed by pa_reads_trim instead."""
    return any(b"[pa_stream] %s%d records:" % (how, records) in run.stderr for how in (b"", b"prefetched "))


@pytest.mark.parametrize("variant", ["plain", "no_prefetch", "gz"])
def test_stream_dumpalign(world, files, variant):
    kw = QUALITY if variant == "plain" else {}
    report = files["dir"] / f"report_{variant}.tsv"
    run = ok(run_main(["-t", "dumpalign", "-g", files["fa"], "-k", str(K), "--reads",
                       files["gz" if variant == "gz" else "reads"], "--trim-report", str(report)] + TRIM_FLAGS
                      + quality_flags(kw),
                      dict(TIMED_ENV, **({"PA_PREFETCH": "0"} if variant == "no_prefetch" else {}))))
    assert streamed(run, len(world.recs)), run.stderr
    assert run.stdout.decode() == summary_text(world, kw)
    assert report.read_text() == T.report_text([world.model()[5]])


def test_stream_took_the_device_path(world, ref, files, monkeypatch):
    monkeypatch.setenv("PA_STREAM_WINDOW", "65536")
    a = PseudoAlignment(ref, trim=FULL)
    a.align_reads_from_file(files["reads"], **QUALITY)
    assert getattr(a, "_streamed_records", None) == len(world.recs)
    assert json.dumps(a.get_summary(), indent=4) + "\n" == summary_text(world, QUALITY)
    assert a.get_trim_stats() == world.model()[5] == a.get_trim_stats(1)
    # per-read results parse the file again, and trim again: the statistics do not move
    want = world.aligned(QUALITY)
    reads = a.reads
    assert len(reads) == int((want.types != 0).sum())
    assert a.get_trim_stats() == world.model()[5]


def test_refused_late_window_leaves_the_callers_statistics(world, ref, files):
    """pa_align_fastq_file_ex adds the file's sums only when it returns PA_OK: a "+." line in the last
    record is refused at a late window, after earlier windows were trimmed, and the caller's struct
    (which a C caller hands on to the host-parsed fallback) is as it was."""
    import ctypes
    text = fastq(world.recs)
    at = text.rfind(b"\n+\n")
    path = files["dir"] / "late.fq"
    path.write_bytes(text[:at] + b"\n+.\n" + text[at + 3:])
    spec = FULL.native()
    stats = N.TrimStats()
    stats.reads, stats.bases_out = 7, 11
    opts = N.FastqOpts(ctypes.pointer(spec), ctypes.pointer(stats))
    res = N.Result(ref.index)
    n = N.U64(0)
    prm = N.Params.make()
    try:
        st = N.lib().pa_align_fastq_file_ex(ref.index.handle, os.fsencode(str(path)), ctypes.byref(prm), 0, res.handle,
                                            4, 65536, None, ctypes.byref(n), ctypes.byref(opts))
        assert st == N.PA_ENOTCANON
        assert stats.as_dict() == dict(T.new_stats(), reads=7, bases_out=11)
        res.reset()
        path.write_bytes(text)
        st = N.lib().pa_align_fastq_file_ex(ref.index.handle, os.fsencode(str(path)), ctypes.byref(prm), 0, res.handle,
                                            4, 65536, None, ctypes.byref(n), ctypes.byref(opts))
        assert st == N.PA_OK and n.value == len(world.recs)
        want = dict(world.model()[5])
        want["reads"] += 7
        want["bases_out"] += 11
        assert stats.as_dict() == want
    finally:
        res.close()


def test_stream_equals_the_pretrimmed_file(files):
    """stdout with the trim flags is byte for byte the stdout without them on the file the model trimmed."""
    base = ["-t", "dumpalign", "-g", files["fa"], "-k", str(K)] + quality_flags(QUALITY)
    report = files["dir"] / "kept_report.tsv"
    a = ok(run_main(base + ["--reads", files["kept"], "--trim-report", str(report)] + TRIM_FLAGS, TIMED_ENV))
    b = ok(run_main(base + ["--reads", files["pretrimmed"]], TIMED_ENV))
    assert streamed(a, 3202) and streamed(b, 3202), (a.stderr, b.stderr)
    assert a.stdout == b.stdout and len(a.stdout) > 100
    assert report.read_text() == T.report_text([files["kept_stats"]])
    c = ok(run_main(base + ["--reads", files["kept"]], STREAM_ENV))
    assert c.stdout != a.stdout  # (the flags change the answer: the untrimmed reads give another)


# ---- 4. the host-parsed consumers --------------------------------------------------------------------

def test_assignments_coverage_variants(files):
    d = files["dir"]
    base = ["-t", "dumpalign", "-g", files["fa"], "-k", str(K), "--coverage"]
    outs = []
    for tag, reads, extra in (("t", files["kept"], TRIM_FLAGS), ("p", files["pretrimmed"], [])):
        names = [str(d / f"{tag}_{x}") for x in ("assignments.tsv", "variants.tsv")]
        run = ok(run_main(base + ["--reads", reads, "--assignments", names[0], "--variants", names[1],
                                  "--variant-min-depth", "2", "--variant-min-count", "1"] + extra))
        outs.append([run.stdout] + [open(n, "rb").read() for n in names])
    assert outs[0] == outs[1]
    assert all(len(x) > 100 for x in outs[0][:2])


# ---- 5. extraction: the selection from the trimmed read, the bytes from the file ---------------------

@pytest.mark.parametrize("host_parsed", [False, True], ids=["device_parsed", "host_parsed"])
def test_extract_writes_the_original_records(world, files, host_parsed):
    out = files["dir"] / f"extract_{int(host_parsed)}.fq"
    extra = ["--assignments", str(files["dir"] / "extract_assignments.tsv")] if host_parsed else []
    run = ok(run_main(["-t", "dumpalign", "-g", files["fa"], "-k", str(K), "--reads", files["reads"], "--extract",
                       str(out), "--extract-genomes", "g0,g5"] + TRIM_FLAGS + extra, STREAM_ENV))
    want = world.aligned({})
    lists = lists_of(want.list_off, want.lists)
    recs = records_of(fastq(world.recs))
    expected = extract_model(recs, want.types.tolist(), lists, spec_of(MAPPED, (0, 5)))
    assert out.read_bytes() == expected and len(expected) > 10000
    assert run.stdout.decode() == summary_text(world, {})
    before = world.aligned({}, False)
    other = extract_model(recs, before.types.tolist(), lists_of(before.list_off, before.lists), spec_of(MAPPED, (0, 5)))
    assert other != expected  # (the untrimmed reads select other records)


# ---- 6. pairs ------------------------------------------------------------------------------------------

def pair_records(gens):
    """300 pairs: two forward ends of one fragment, each with its own adapter at a random insert (some at
    0: the mate is emptied) or none, and mate 2 with a bad tail."""
    rng = np.random.default_rng(66)
    m1, m2 = [], []
    for i in range(300):
        g = int(rng.integers(0, 8))
        at = int(rng.integers(0, 30000 - 400))
        mates = []
        for j, adapter in enumerate((TRUSEQ, ADAPTER2)):
            seq = bytearray(bytes(gens[g][at + 200 * j:at + 200 * j + 120]).replace(b"N", b"A"))
            if i % 3:
                p = 0 if i % 50 == 1 else int(rng.integers(20, 120))
                seq[p:] = (adapter + bytes(rng.choice(ACGT, size=120)))[:120 - p]
            qual = bytearray(rng.integers(60, 74, 120, dtype=np.uint8))
            if j == 1 and i % 4 == 0:
                t = int(rng.integers(30, 120))
                qual[t:] = bytes(rng.integers(35, 51, 120 - t, dtype=np.uint8))
            mates.append((bytes(seq), bytes(qual)))
        m1.append((b"p%d/1" % i,) + mates[0])
        m2.append((b"p%d/2" % i,) + mates[1])
    return m1, m2


def test_pairs_trim_each_mate_by_its_own_spec(world, files):
    d = files["dir"]
    m1, m2 = pair_records(world.gens)
    (d / "m1.fq").write_bytes(fastq(m1))
    (d / "m2.fq").write_bytes(fastq(m2))
    spec1, spec2 = T.Spec(QCUT, None, TRUSEQ), T.Spec(QCUT, None, ADAPTER2)
    t1 = T.trim_columns(*columns(m1), spec1)
    t2 = T.trim_columns(*columns(m2), spec2)
    assert t1[5]["reads_adapter"] >= 150 and t2[5]["reads_adapter"] >= 150 and t2[5]["reads_quality"] >= 50
    assert t1[5]["reads_empty"] >= 3 and t1[5] != t2[5]

    def mate(t, i):
        return t[0][t[2][i]:t[2][i + 1]].decode(), t[1][t[2][i]:t[2][i + 1]].decode("latin-1")
    pairs = [mate(t1, i) + mate(t2, i) for i in range(len(m1))]
    gens = [bytes(g).decode() for g in world.gens]
    results = M.model_all(M.kmer_sets(gens, False, K), K, pairs, m=1, p=1)
    report = d / "pairs_report.tsv"
    run = ok(run_main(["-t", "dumpalign", "-g", files["fa"], "-k", str(K), "--reads", str(d / "m1.fq"), "--reads2",
                       str(d / "m2.fq"), "--trim-quality", str(QCUT), "--trim-adapter", TRUSEQ.decode(),
                       "--trim-adapter2", ADAPTER2.decode(), "--trim-report", str(report)]))
    assert json.loads(run.stdout) == M.summary_of(results, world.names)
    assert run.stdout.decode() == json.dumps(M.summary_of(results, world.names), indent=4) + "\n"
    assert report.read_text() == T.report_text([t1[5], t2[5]])
    untrimmed = M.model_all(M.kmer_sets(gens, False, K), K,
                            [(a[1].decode(), a[2].decode("latin-1"), b[1].decode(), b[2].decode("latin-1"))
                             for a, b in zip(m1, m2)], m=1, p=1)
    assert [r[:2] for r in untrimmed] != [r[:2] for r in results]


# ---- 7. the Python interface ---------------------------------------------------------------------------

def test_pseudo_alignment_sees_trimmed_reads(world, ref, files):
    from data_file import FASTAQFile
    want = world.aligned(QUALITY)
    a = PseudoAlignment(ref, trim=FULL)
    a.align_reads_from_container(FASTAQFile(files["reads"]).container, **QUALITY)
    assert getattr(a, "_streamed_records", None) is None
    assert json.dumps(a.get_summary(), indent=4) + "\n" == summary_text(world, QUALITY)
    assert a.get_trim_stats() == world.model()[5]
    reads = a.reads
    ids = [r[0].decode() for r in world.recs]
    kept = [i for i, t in enumerate(want.types) if t != 0]
    assert list(reads) == [ids[i] for i in kept]
    lists = lists_of(want.list_off, want.lists)
    for i in kept[::7]:
        entry = reads[ids[i]]
        assert entry["mapping_type"].value == int(want.types[i])
        assert entry["genomes_mapped_to"] == [world.names[g] for g in lists[i]]
    assert PseudoAlignment(ref).get_trim_stats() is None
    # -t align writes an .aln of the trimmed reads; dumpalign -a prints their summary
    aln = files["dir"] / "trimmed.aln"
    kdb = files["dir"] / "ref.kdb"
    ok(run_main(["-t", "reference", "-g", files["fa"], "-k", str(K), "-r", str(kdb)]))
    ok(run_main(["-t", "align", "-r", str(kdb), "--reads", files["reads"], "-a", str(aln)] + TRIM_FLAGS
                + quality_flags(QUALITY)))
    run = ok(run_main(["-t", "dumpalign", "-a", str(aln)]))
    assert run.stdout.decode() == summary_text(world, QUALITY)
