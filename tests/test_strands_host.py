"""Both-strand alignment, host side (no GPU).  A both-strand index of genomes g
is a forward index of T(g) = g + "N" + reverse_complement(g)
(synth.both_strands_genome); tests/golden/strand_cases.json
(make_golden_strands.py) holds the raw genomes and the REFERENCE's results on
T(genomes)."""

import json
import os
import re

import pytest

import pa_native as N
import pa_oracle as O
import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")

with open(os.path.join(GOLD, "strand_cases.json")) as _f:
    STRAND = json.load(_f)


def test_strand_transform():
    assert bytes(synth.both_strands_genome("AACGN")) == b"AACGNNNCGTT"
    assert bytes(synth.both_strands_genome("")) == b"" and bytes(synth.both_strands_genome(b"A")) == b"ANT"


def test_header_constant_matches_binding():
    text = open(os.path.join(REPO, "include", "pa.h")).read()
    m = re.search(r"#define PA_BUILD_BOTH_STRANDS (\d+)u", text)
    assert m and int(m.group(1)) == N.PA_BUILD_BOTH_STRANDS == 4
    assert "pa_index_strands" in N.EXPORTS


def test_cli_flag_parses_and_reverse_complement_stays_inert():
    import main
    base = ["-t", "dumpalign", "-g", "g.fa", "-k", "5", "--reads", "r.fq"]
    a = main.parse_arguments(base)
    assert a.both_strands is False and a.reverse_complement is False
    a = main.parse_arguments(base + ["--both-strands"])
    assert a.both_strands is True and a.reverse_complement is False
    a = main.parse_arguments(base + ["--reverse-complement"])
    assert a.reverse_complement is True and a.both_strands is False
    src = open(os.path.join(os.path.dirname(os.path.abspath(main.__file__)), "main.py")).read()
    assert "reverse_complement" not in src  # parsed (the add_argument line, with dashes), and nothing reads it
    for task in ("reference", "align"):
        assert main.parse_arguments(["-t", task, "-g", "g.fa", "-k", "5", "--both-strands"]).both_strands is True


def test_pickled_property_defaults_to_forward(monkeypatch):
    """A .kdb without the key, and one written by the reference, load as
    forward-only; a both-strand one keeps the property."""
    import kmer
    built = []
    monkeypatch.setattr(kmer.KmerReference, "_build",
                        lambda self: (built.append(getattr(self, "_both_strands", None)), setattr(self, "_view", None)))
    ref = kmer.KmerReference.__new__(kmer.KmerReference)
    ref.__setstate__({"genomes": [], "kmer_len": 5, "_all_genomes": None, "_ref_kmers": None, "_device": 0,
                      "_compact": False})
    assert ref._both_strands is False and built[-1] is False
    ref._both_strands = True
    again = kmer.KmerReference.__new__(kmer.KmerReference)
    again.__setstate__(ref.__getstate__())
    assert again._both_strands is True and built[-1] is True
    old = kmer.KmerReference.load(os.path.join(GOLD, "config1.kdb"))  # written by the reference
    assert old._both_strands is False and built[-1] is False


@pytest.mark.parametrize("case", STRAND["cases"], ids=[c["name"] for c in STRAND["cases"]])
def test_oracle_on_t_genomes_reproduces_strand_cases(case):
    """The unchanged oracle, run forward-only on T(genomes), gives the reference's
    results on T(genomes): this pins the fixture on the CPU."""
    idents = [g[0] for g in case["genomes"]]
    ix = O.OracleIndex([bytes(synth.both_strands_genome(g[1])) for g in case["genomes"]], case["k"])
    assert ix.n_kmers == case["n_kmers"]
    got = ix.export()
    exp_sets = {km: gl for km, gl in case["kmer_sets"]}
    assert {km: got.get(km) for km in exp_sets} == exp_sets
    for km, gl in list(got.items())[:200]:  # the index is symmetric
        assert got[O.reverse_complement(km)] == gl, km
    seq, off = O.concat([r[1] for r in case["reads"]])
    qual, _ = O.concat([r[2] for r in case["reads"]])
    for res in case["results"]:
        ps = res["params"]
        out = ix.align(seq, qual, off, m=ps["m"], p=ps["p"], mrq=ps["mrq"], mkq=ps["mkq"], mg=ps["mg"])
        for r, (rid, tname, glist, qf, hr) in enumerate(res["reads"]):
            assert O.TYPE_NAMES[int(out.types[r])] == tname, (rid, ps)
            assert [idents[g] for g in out.genomes_of(r)] == glist, (rid, ps)
            assert int(out.qf[r]) == qf and int(out.hr[r]) == hr, (rid, ps)
        summ = O.summary_by_walk(out, idents, ps["mrq"], ps["mkq"], ps["mg"])
        assert summ == res["summary"]
        assert json.dumps(summ, indent=4) == res["summary_text"]
