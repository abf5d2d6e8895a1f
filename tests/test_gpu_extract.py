"""Read extraction on the device (pa_extract_fastq_file, pa_reads_select,
csrc/pa_extract.hip) against the plain-Python model of
tests/test_extract_host.py fed with the unchanged CPU oracle's types and lists.
Every comparison is for exact equality of bytes and integers: the output file,
the statistics, the summary next to a run without extraction.

The main file is test_gpu_fastq.py's (3000 reads of six lengths) with 200
chimeric reads appended (75 bases of genome a + 75 of genome (a + 4) % 8), which
give ambiguous reads whose lists hold two or more genomes.  Small windows
(PA_STREAM_WINDOW=65536: some fifteen windows) carry records across window
boundaries.  The third-line variant the exact grammar accepts is "+" followed
by dots (records.py: r"\\+(\\.*)"); a literal "+id" line is refused by it, so
both are tested: the first for the canonical four lines, the second for the
reference's error and an empty output file."""

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
from data_file import FASTAQFile
from kmer import KmerReference, PseudoAlignment
from records import FASTARecordContainer
from test_extract_host import (ALL, AMBIGUOUS, DROPPED, MAIN, MAPPED, UNIQUE, UNMAPPED, extract_flags, extract_model,
                               extract_model_stats, lists_of, records_of, spec_of)
from test_gpu_abundance import large_case
from test_gpu_fastq import PARAMS, reads_text

pytestmark = pytest.mark.gpu

K = 31
PARAM_SETS = PARAMS + ([dict(m=2, p=0)] if dict(m=2, p=0) not in PARAMS else [])
QUALITY = dict(min_read_quality=58, min_kmer_quality=60, max_genomes=2)
WORDS = {DROPPED: "filtered", UNMAPPED: "unmapped", UNIQUE: "unique", AMBIGUOUS: "ambiguous"}
# each type alone, mapped, mapped with genome_keep = {g0}, {g0, g5}, all and none (each also inverted by the tests)
SPECS = [(1 << DROPPED, None), (1 << UNMAPPED, None), (1 << UNIQUE, None), (1 << AMBIGUOUS, None), (MAPPED, None),
         (MAPPED, (0,)), (MAPPED, (0, 5)), (MAPPED, tuple(range(8))), (MAPPED, ())]


def words_of(mask):
    return [WORDS[t] for t in range(4) if (mask >> t) & 1]


def oracle_kw(kw):
    return dict(m=kw.get("m", 1), p=kw.get("p", 1), mrq=kw.get("min_read_quality"), mkq=kw.get("min_kmer_quality"),
                mg=kw.get("max_genomes"))


def oracle_align(oracle, recs, kw):
    """(types, lists per read) of the records under the parameters kw, from the CPU oracle."""
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    np.cumsum([len(r[1]) for r in recs], out=off[1:])
    o = oracle.align(b"".join(r[1] for r in recs), b"".join(r[2] for r in recs), off, **oracle_kw(kw))
    return [int(t) for t in o.types], lists_of(o.list_off, o.lists)


@pytest.fixture(scope="module")
def world():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible (no CPU fallback exists)")
    gens = synth.family_genomes(8, 30000, seed=5, family_size=4, sub_rate=0.02, conserved_len=800)
    names = [f"g{i}" for i in range(len(gens))]
    c = FASTARecordContainer()
    c.parse_records(synth.fasta_text([f"{n} test genome" for n in names], gens, width=70))
    text = reads_text(gens, 3000, seed=11, lens=(150, 100, 31, 20, 176, 250))
    rng = np.random.default_rng(2011)
    chim = []
    for i in range(200):
        a = int(rng.integers(0, 8))
        b = (a + 4) % 8
        pa, pb = int(rng.integers(0, 30000 - 75)), int(rng.integers(0, 30000 - 75))
        seq = (bytes(gens[a][pa:pa + 75]) + bytes(gens[b][pb:pb + 75])).replace(b"N", b"A")
        chim.append(b"@chim%d %d+%d\n%s\n+\n%s\n" % (i, a, b, seq, bytes([70]) * 150))
    text = text.encode() + b"".join(chim)
    ref = KmerReference(K, c)
    w = {"gens": gens, "names": [g.identifier for g in ref.genomes], "ref": ref,
         "oracle": O.OracleIndex(gens, K), "text": text, "records": records_of(text), "memo": {}, "summary": {},
         "container": c}
    # what the comparisons below stand on, from the oracle, before anything is compared
    types, lists = classified(w, QUALITY)
    for t in range(4):
        assert sum(1 for x in types if x == t) >= 100, (t, "too few reads of this type")
    assert sum(1 for t, l in zip(types, lists) if t == AMBIGUOUS and not l) >= 100
    types, lists = classified(w, dict(m=2, p=0))
    assert sum(1 for l in lists if len(l) >= 2) >= 20
    return w


def classified(world, kw):
    key = json.dumps(kw, sort_keys=True)
    if key not in world["memo"]:
        world["memo"][key] = oracle_align(world["oracle"], world["records"], kw)
    return world["memo"][key]


def summary_without(world, path, kw):
    """get_summary() of the run without extraction (the device-parsed stream), as JSON text."""
    key = json.dumps(kw, sort_keys=True)
    if key not in world["summary"]:
        a = PseudoAlignment(world["ref"])
        a.align_reads_from_file(path, **kw)
        world["summary"][key] = json.dumps(a.get_summary(), indent=4)
    return world["summary"][key]


def names_of(world, keep):
    return None if keep is None else [world["names"][g] for g in keep]


def run_extract(ref, path, out, mask, genomes, invert, kw, streamed=True, alignment=None):
    a = alignment if alignment is not None else PseudoAlignment(ref)
    stats = a.extract_reads_from_file(path, out, words_of(mask), genomes, invert, **kw)
    assert (getattr(a, "_streamed_records", None) is not None) == streamed
    with open(out, "rb") as f:
        return f.read(), stats, a


def merged_is_input(part, rest, flags, records):
    """The spec's records and its inverse's, merged in file order, are the input."""
    from test_extract_host import record_bytes
    at = [0, 0]
    for s, rec in zip(flags, records):
        b = record_bytes(rec)
        src = part if s else rest
        i = 0 if s else 1
        if src[at[i]:at[i] + len(b)] != b:
            return False
        at[i] += len(b)
    return at[0] == len(part) and at[1] == len(rest)


# ---- the main case ----------------------------------------------------------------------------

@pytest.mark.parametrize("spec", range(len(SPECS)), ids=lambda i: f"spec{i}")
@pytest.mark.parametrize("window", [0, 65536])
@pytest.mark.parametrize("kw", PARAM_SETS, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "default")
def test_main_case(world, tmp_path, monkeypatch, kw, window, spec):
    monkeypatch.setenv("PA_STREAM_WINDOW", str(window))
    path = str(tmp_path / "reads.fq")
    with open(path, "wb") as f:
        f.write(world["text"])
    types, lists = classified(world, kw)
    recs = world["records"]
    mask, keep = SPECS[spec]
    outs = []
    for invert in (False, True):
        sp = spec_of(mask, keep, invert)
        got, stats, a = run_extract(world["ref"], path, str(tmp_path / f"out{int(invert)}.fq"), mask,
                                    names_of(world, keep), invert, kw)
        assert got == extract_model(recs, types, lists, sp)
        assert stats == extract_model_stats(recs, types, lists, sp)
        assert json.dumps(a.get_summary(), indent=4) == summary_without(world, path, kw)
        outs.append(got)
    assert merged_is_input(outs[0], outs[1], extract_flags(types, lists, spec_of(mask, keep)), recs)
    if keep is not None and 0 < len(keep) < 8 and kw == dict(m=2, p=0):  # (the restriction restricts, here)
        assert 0 < len(outs[0]) < len(extract_model(recs, types, lists, spec_of(mask)))


# ---- edges, one small file each ---------------------------------------------------------------

def check_file(world, tmp_path, text, specs, kw=None, ref=None, oracle=None, name="reads.fq", streamed=True):
    """Every spec (mask, keep, invert) on the file `text`: output and statistics equal the model's."""
    kw = kw or {}
    path = str(tmp_path / name)
    if name.endswith(".gz"):
        with gzip.open(path, "wb") as f:
            f.write(text)
    else:
        with open(path, "wb") as f:
            f.write(text)
    recs = records_of(text)
    types, lists = oracle_align(oracle or world["oracle"], recs, kw)
    outs = []
    for i, (mask, keep, invert) in enumerate(specs):
        sp = spec_of(mask, keep, invert)
        got, stats, _ = run_extract(ref or world["ref"], path, str(tmp_path / f"out{i}.fq"), mask,
                                    names_of(world, keep), invert, kw, streamed=streamed)
        assert got == extract_model(recs, types, lists, sp), (mask, keep, invert)
        assert stats == extract_model_stats(recs, types, lists, sp), (mask, keep, invert)
        outs.append(got)
    return types, lists, outs


def genome_read(world, g, at, n):
    return bytes(world["gens"][g][at:at + n]).replace(b"N", b"A")


def fq(recs):
    return b"".join(b"@%s\n%s\n+\n%s\n" % r for r in recs)


def test_nine_byte_records(world, tmp_path):
    """Records of 9 bytes ("@a", one base): several records per 16-byte chunk, selected alternately
    (every second one fails --min-read-quality), all and none."""
    ids = [bytes([c]) for c in range(0x21, 0x7F)]
    text = fq([(rid, b"ACGT"[i % 4:i % 4 + 1], b"I" if i % 2 else b"!") for i, rid in enumerate(ids)])
    assert len(text) == 9 * len(ids)
    kw = dict(min_read_quality=50)
    types, _, outs = check_file(world, tmp_path, text, [(1 << DROPPED, None, False), (1 << UNMAPPED, None, False),
                                                        (ALL, None, False), (ALL, None, True)], kw)
    assert types == [DROPPED if i % 2 == 0 else UNMAPPED for i in range(len(ids))]
    assert len(outs[0]) == len(outs[1]) == len(text) // 2 and outs[2] == text and outs[3] == b""


def test_long_reads(world, tmp_path):
    """A read of 5000 bases and one of 20000 (past a 4096-byte tile, inside a window) between short ones."""
    recs = []
    for i, (g, at, n) in enumerate([(0, 100, 150), (1, 2000, 5000), (2, 50, 31), (3, 5000, 20000), (4, 7, 150)]):
        s = genome_read(world, g, at, n)
        recs.append((b"r%d" % i, s, b"I" * n))
    recs.insert(2, (b"noise", b"ACGT" * 40, b"I" * 160))
    text = fq(recs)
    types, _, outs = check_file(world, tmp_path, text,
                                [(1 << t, None, inv) for t in range(4) for inv in (False, True)] + [(ALL, None, False)])
    assert types[2] == UNMAPPED and types[1] in (UNIQUE, AMBIGUOUS) and types[4] in (UNIQUE, AMBIGUOUS)
    assert outs[-1] == text


def test_alternating(world, tmp_path):
    """Selected and not selected records in turn: genome reads between reads of no genome."""
    rng = np.random.default_rng(777)  # (not the genomes' seed: that stream starts with their shared stretch)
    recs = []
    for i in range(301):
        if i % 2 == 0:
            n = 100 + i % 50
            s = genome_read(world, i % 8, 15000 + 31 * i, n)
        else:
            n = 40 + i % 7
            s = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))
        recs.append((b"alt%d" % i, s, b"I" * n))
    text = fq(recs)
    types, _, outs = check_file(world, tmp_path, text, [(MAPPED, None, False), (MAPPED, None, True)])
    assert all((t in (UNIQUE, AMBIGUOUS)) == (i % 2 == 0) for i, t in enumerate(types))
    assert len(outs[0]) + len(outs[1]) == len(text)


@pytest.mark.parametrize("last_mapped", [True, False])
def test_no_final_line_feed(world, tmp_path, last_mapped):
    """A file without a final line feed, the last record selected and not selected:
    the record gets its line feed, and no byte past the text is needed for it."""
    recs = [(b"a", genome_read(world, 0, 10, 150), b"I" * 150), (b"b", b"ACGT" * 20, b"I" * 80),
            (b"c", genome_read(world, 1, 10, 97), b"I" * 97)]
    if not last_mapped:
        recs.append((b"d", b"TGCA" * 13, b"I" * 52))
    text = fq(recs)[:-1]
    types, _, outs = check_file(world, tmp_path, text, [(MAPPED, None, False), (MAPPED, None, True), (ALL, None, False)])
    assert (types[-1] in (UNIQUE, AMBIGUOUS)) == last_mapped
    assert outs[2] == text + b"\n"
    assert outs[0 if last_mapped else 1].endswith(recs[-1][2] + b"\n")


def test_nothing_and_everything(world, tmp_path):
    text = world["text"][:40000]
    text = text[:text.rfind(b"\n@r") + 1]
    _, _, outs = check_file(world, tmp_path, text, [(ALL, None, True), (ALL, None, False)])
    assert outs[0] == b"" and os.path.exists(tmp_path / "out0.fq")  # (an empty file is created)
    assert outs[1] == text


def test_gz_input(world, tmp_path, monkeypatch):
    monkeypatch.setenv("PA_STREAM_WINDOW", "65536")
    text = world["text"][:300000]
    text = text[:text.rfind(b"\n@r") + 1]
    check_file(world, tmp_path, text, [(MAPPED, (0, 5), False), (1 << UNMAPPED, None, False), (ALL, None, False)],
               name="reads.fq.gz")


def test_both_strand_index(world, tmp_path):
    ref = KmerReference(K, world["container"], both_strands=True)
    oracle = O.OracleIndex([synth.both_strands_genome(g) for g in world["gens"]], K)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    recs = []
    for i in range(200):
        s = genome_read(world, i % 8, 1000 + 97 * i, 120)
        recs.append((b"s%d" % i, s.translate(comp)[::-1] if i % 3 else s, b"I" * 120))
    types, _, _ = check_file(world, tmp_path, fq(recs), [(MAPPED, (1, 2), False), (MAPPED, (1, 2), True),
                                                         (1 << UNIQUE, None, False)], ref=ref, oracle=oracle)
    assert sum(1 for t in types if t in (UNIQUE, AMBIGUOUS)) > 150  # (the reverse-complement reads map)


def test_without_the_lane_path(world, tmp_path, monkeypatch):
    """PA_ASSIGN=0: every read classified by the exact kernel."""
    monkeypatch.setenv("PA_ASSIGN", "0")
    monkeypatch.setenv("PA_STREAM_WINDOW", "65536")
    text = world["text"][-200000:]
    text = text[text.find(b"\n@r") + 1:]
    check_file(world, tmp_path, text, [(MAPPED, (0,), False), (1 << AMBIGUOUS, None, False), (MAPPED, None, True)],
               dict(m=2, p=0))


# ---- pa_reads_select ----------------------------------------------------------------------------

def upload(recs, device=None):
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    np.cumsum([len(r[1]) for r in recs], out=off[1:])
    seq = np.frombuffer(b"".join(r[1] for r in recs), dtype=np.uint8)
    qual = np.frombuffer(b"".join(r[2] for r in recs), dtype=np.uint8)
    return N.Reads.upload(seq, qual, off, device=device)


@pytest.mark.parametrize("kw", [QUALITY, dict(m=2, p=0)], ids=["quality", "m2p0"])
def test_reads_select(world, kw):
    recs = world["records"]
    types, lists = classified(world, kw)
    index = world["ref"].index
    reads = upload(recs, index.device)
    prm = N.Params.make(**kw)
    try:
        for mask, keep in SPECS:
            for invert in (False, True):
                k8 = None if keep is None else np.isin(np.arange(8), keep).astype(np.uint8)
                got = N.reads_select(index, reads, prm, N.ExtractSpec.make(mask, k8, invert))
                assert got.tolist() == extract_flags(types, lists, spec_of(mask, keep, invert)), (mask, keep, invert)
        for bad in (0, 16, 1 << 31, 0x1F):
            with pytest.raises(ValueError):
                N.reads_select(index, reads, prm, N.ExtractSpec.make(bad))
    finally:
        reads.close()


def test_reads_select_many_genomes():
    """300 genomes that share one stretch, genome_keep set on genomes above 64: the byte array is read
    at every genome number, past a wave's width."""
    genomes, seqs, quals = large_case(300, 500, 200, 31, 90)
    recs = [(b"r%d" % i, s.encode(), q.encode()) for i, (s, q) in enumerate(zip(seqs, quals))]
    types, lists = oracle_align(O.OracleIndex(genomes, 31), recs, {})
    listed = sorted({g for l in lists for g in l})
    high = [g for g in listed if g > 64]
    assert len(high) >= 20 and any(t == AMBIGUOUS and not l for t, l in zip(types, lists))
    index = N.Index(genomes, 31)
    reads = upload(recs, index.device)
    try:
        for keep in ((high[0],), (high[1], high[-1]), tuple(high[::2]), tuple(range(65, 300)), (65,)):
            k = np.isin(np.arange(300), keep).astype(np.uint8)
            for mask in (MAPPED, ALL, 1 << AMBIGUOUS):
                for invert in (False, True):
                    got = N.reads_select(index, reads, N.Params.make(), N.ExtractSpec.make(mask, k, invert))
                    assert got.tolist() == extract_flags(types, lists, spec_of(mask, keep, invert))
        some = extract_flags(types, lists, spec_of(MAPPED, (high[0],)))
        assert 0 < sum(some) < sum(extract_flags(types, lists, spec_of(MAPPED)))  # (the restriction restricts)
    finally:
        reads.close()
        index.close()


# ---- the host path against the device path ----------------------------------------------------

@pytest.fixture(scope="module")
def small(world):
    text = world["text"][-120000:]
    return text[text.find(b"\n@r") + 1:]


@pytest.mark.parametrize("variant", ["crlf", "plus_dots"])
def test_host_path_gives_the_canonical_lines(world, tmp_path, small, variant):
    """A CRLF copy and a "+.." copy take the host path and give the four canonical lines of the LF file."""
    text = small.replace(b"\n", b"\r\n") if variant == "crlf" else small.replace(b"\n+\n", b"\n+..\n")
    specs = [(MAPPED, (0, 5), False), (MAPPED, None, True), (ALL, None, False)]
    _, _, outs = check_file(world, tmp_path, text, specs, dict(m=2, p=0), streamed=False)
    assert outs[2] == small
    (tmp_path / "lf").mkdir()
    _, _, lf = check_file(world, tmp_path / "lf", small, specs, dict(m=2, p=0))
    assert outs == lf  # (the result does not depend on the path that ran)


def late_error_file(world, bad_line):
    """The main file with one bad "+" line in its last record: the window that holds it comes late."""
    text = world["text"]
    at = text.rfind(b"\n+\n")
    return text[:at] + b"\n" + bad_line + b"\n" + text[at + 3:]


def test_late_bad_record_accepted_by_the_grammar(world, tmp_path, monkeypatch):
    monkeypatch.setenv("PA_STREAM_WINDOW", "65536")
    text = late_error_file(world, b"+.")
    path = str(tmp_path / "late.fq")
    with open(path, "wb") as f:
        f.write(text)
    # the entry point itself: earlier windows are written, and the statistics say how much
    ref = world["ref"]
    with open(tmp_path / "partial.fq", "wb") as fh:
        n, stats = N.extract_fastq_file(ref.index, path, N.Params.make(), N.ExtractSpec.make(ALL), fh.fileno())
    assert n is None
    assert 65536 < stats["bytes"] < len(text) and stats["records"] == stats["selected"] > 0
    assert (tmp_path / "partial.fq").read_bytes() == text[:stats["bytes"]]
    # the Python layer: the file truncated, the host path's output
    types, lists, outs = check_file(world, tmp_path, text, [(MAPPED, None, False), (ALL, None, False)],
                                    name="late.fq", streamed=False)
    assert outs[1] == world["text"]  # (the canonical lines: the "+." line written as "+")


def test_late_bad_record_refused_by_the_grammar(world, tmp_path, monkeypatch):
    monkeypatch.setenv("PA_STREAM_WINDOW", "65536")
    path = str(tmp_path / "late.fq")
    with open(path, "wb") as f:
        f.write(late_error_file(world, b"+chim199"))
    with pytest.raises(Exception) as want:
        FASTAQFile(path).container
    out = tmp_path / "out.fq"
    a = PseudoAlignment(world["ref"])
    with pytest.raises(type(want.value)) as got:
        a.extract_reads_from_file(path, str(out))
    assert str(got.value) == str(want.value)
    assert out.exists() and out.stat().st_size == 0


def test_abundance_job_takes_the_host_path(world, tmp_path, small):
    path = str(tmp_path / "reads.fq")
    with open(path, "wb") as f:
        f.write(small)
    recs = records_of(small)
    kw = dict(m=2, p=0)
    types, lists = oracle_align(world["oracle"], recs, kw)
    a = PseudoAlignment(world["ref"], abundance=True)
    got, stats, _ = run_extract(world["ref"], path, str(tmp_path / "out.fq"), MAPPED, [world["names"][0]], False, kw,
                                streamed=False, alignment=a)
    sp = spec_of(MAPPED, (0,))
    assert got == extract_model(recs, types, lists, sp) and stats == extract_model_stats(recs, types, lists, sp)
    assert a.get_abundance()  # (the accumulator was fed)
    with pytest.raises(ValueError, match="unknown genome identifier: nope"):
        PseudoAlignment(world["ref"]).extract_reads_from_file(path, str(tmp_path / "o2.fq"), genomes=["nope"])


# ---- the CLI ------------------------------------------------------------------------------------

def test_cli(world, tmp_path, small):
    fa, fq_path, out = tmp_path / "g.fa", tmp_path / "reads.fq", tmp_path / "host_depleted.fq"
    fa.write_text(synth.fasta_text(world["names"], world["gens"], width=70))
    fq_path.write_bytes(small)
    base = [sys.executable, MAIN, "-t", "dumpalign", "-g", str(fa), "-k", str(K), "--reads", str(fq_path)]
    plain = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    run = subprocess.run(base + ["--extract", str(out), "--extract-genomes", f"{world['names'][0]},{world['names'][5]}",
                                 "--extract-invert"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert plain.returncode == 0 and run.returncode == 0, (plain.stderr, run.stderr)
    assert run.stdout == plain.stdout and len(plain.stdout) > 0
    recs = records_of(small)
    types, lists = oracle_align(world["oracle"], recs, {})
    assert out.read_bytes() == extract_model(recs, types, lists, spec_of(MAPPED, (0, 5), True))
