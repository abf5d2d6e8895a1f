"""The consumers of the assign pass: PseudoAlignment.reads,
Coverage, align_placements and the CLI's --assignments.  PA_ASSIGN=0 sends
them back to the exact pass; both settings must give the same results."""

import io
import os
import subprocess
import sys

import numpy as np
import pytest

import pa_native as N
import synth
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

MAIN = os.path.join(PKG, "main.py")
FA, FQ = os.path.join(GOLDEN, "config1.fa"), os.path.join(GOLDEN, "config1.fq")
ALN_FLAGS = ["-p", "3", "--min-kmer-quality", "58", "--max-genomes", "2"]  # (tests/golden/make_golden.py: config1.aln)
WORDS = {"UNIQUELY_MAPPED": "unique", "AMBIGUOUSLY_MAPPED": "ambiguous", "UNMAPPED": "unmapped"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


def config1_alignment(**kw):
    from data_file import FASTAFile, FASTAQFile
    from kmer import KmerReference, PseudoAlignment
    ref = KmerReference(21, FASTAFile(FA).container)
    pa = PseudoAlignment(ref)
    pa.align_reads_from_container(FASTAQFile(FQ).container, **kw)
    return pa


def test_reads_equal_under_both_settings(monkeypatch):
    monkeypatch.delenv("PA_ASSIGN", raising=False)
    new = config1_alignment(p=3, min_kmer_quality=58, max_genomes=2).reads
    monkeypatch.setenv("PA_ASSIGN", "0")
    old = config1_alignment(p=3, min_kmer_quality=58, max_genomes=2).reads
    assert len(new) > 0 and list(new.items()) == list(old.items())  # (dict order included)


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
def test_coverage_and_placements(both, monkeypatch):
    gens = synth.family_genomes(10, 30000, seed=311, family_size=5, sub_rate=0.01, conserved_len=500, n_rate=2e-4,
                                n_run=8)
    seq, qual, _ = synth.sample_reads(gens, 5000, 150, seed=470, err_rate=0.015)
    if both:
        seq = seq.copy()
        seq[::2] = synth.reverse_complement(seq[::2])
    off = np.arange(len(seq) + 1, dtype=np.uint64) * 150
    index = N.Index(gens, 31, both_strands=both)
    reads = N.Reads.upload(seq.reshape(-1), qual.reshape(-1), off)
    out = {}
    for setting in (None, "0"):
        if setting is None:
            monkeypatch.delenv("PA_ASSIGN", raising=False)
        else:
            monkeypatch.setenv("PA_ASSIGN", setting)
        for ps in (dict(), dict(max_genomes=2)):
            prm = N.Params.make(**ps)
            cov = N.Coverage(index)
            cov.add(reads, prm)
            depths = [np.concatenate(cov.depth(g)) for g in range(len(gens))]
            cov.close()
            out[(setting, tuple(ps))] = (depths, N.align_placements(index, reads, prm))
    reads.close()
    for ps in ((), ("max_genomes",)):
        (d_new, p_new), (d_old, p_old) = out[(None, ps)], out[("0", ps)]
        assert sum(int(d.sum()) for d in d_new) > 0
        for a, b in zip(d_new, d_old):
            assert a.tolist() == b.tolist()
        for a, b in zip(p_new, p_old):
            assert a.tolist() == b.tolist()


# ---- the CLI ---------------------------------------------------------------------------------

def run_cli(flags, cwd):
    cmd = [sys.executable, MAIN, "-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ] + flags
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=str(cwd))
    assert r.returncode == 0, r.stderr
    return r.stdout


def fastq_ids():
    from data_file import FASTAQFile
    return [r.identifier for r in FASTAQFile(FQ).container]


def parse(path):
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[0] == "#read\tmapping\tgenomes" and lines[-1] == ""
    return [tuple(l.split("\t")) for l in lines[1:-1]]


def lines_of(reads, ids):
    """The file's lines from a ``reads`` dict; ids missing from it were filtered."""
    out = []
    for rid in ids:
        if rid not in reads:
            out.append((rid, "filtered", ""))
            continue
        e = reads[rid]
        listed = ",".join(e["genomes_mapped_to"]) if e["mapping_type"].name != "UNMAPPED" else ""
        out.append((rid, WORDS[e["mapping_type"].name], listed))
    return out


def test_cli_assignments(tmp_path):
    plain = run_cli(ALN_FLAGS, tmp_path)
    tsv = tmp_path / "a.tsv"
    assert run_cli(ALN_FLAGS + ["--assignments", str(tsv)], tmp_path) == plain  # stdout: byte for byte
    got = parse(tsv)
    ids = fastq_ids()
    assert [g[0] for g in got] == ids  # one line per record, in file order
    assert got == lines_of(config1_alignment(p=3, min_kmer_quality=58, max_genomes=2).reads, ids)
    # the reference's own alignment of the same flags (tests/golden/make_golden.py)
    from kmer import PseudoAlignment
    assert got == lines_of(PseudoAlignment.load(os.path.join(GOLDEN, "config1.aln")).reads, ids)
    assert {g[1] for g in got} >= {"unique", "ambiguous"}


def test_cli_assignments_filtered_lines(tmp_path):
    flags = ["--min-read-quality", "58"]
    plain = run_cli(flags, tmp_path)
    tsv = tmp_path / "b.tsv"
    assert run_cli(flags + ["--assignments=" + str(tsv), "--coverage"], tmp_path) != ""
    assert run_cli(flags + ["--assignments", str(tsv)], tmp_path) == plain
    got = parse(tsv)
    ids = fastq_ids()
    reads = config1_alignment(min_read_quality=58).reads
    assert 0 < len(reads) < len(ids)  # (the threshold drops some reads, not all)
    assert got == lines_of(reads, ids)
    assert sum(g[1] == "filtered" for g in got) == len(ids) - len(reads)


def test_write_assignments_api():
    pa = config1_alignment()
    fh = io.StringIO()
    pa.write_assignments(fh)
    ids = fastq_ids()
    lines = fh.getvalue().split("\n")
    assert lines[0] == "#read\tmapping\tgenomes" and len(lines) == len(ids) + 2
    assert [tuple(l.split("\t")) for l in lines[1:-1]] == lines_of(pa.reads, ids)
