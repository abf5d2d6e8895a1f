"""Both-strand pseudo-alignment (PA_BUILD_BOTH_STRANDS, Index(both_strands=True),
KmerReference(both_strands=True), main.py --both-strands) on the GPU.

The acceptance rule: every result of a both-strand index over genomes g equals,
bit for bit, the result of the reference -- and of the unchanged CPU oracle --
run forward-only on T(g) = g + "N" + reverse_complement(g) with the same
headers (synth.both_strands_genome).  tests/golden/strand_cases.json holds the
reference's results on T(genomes) (make_golden_strands.py; pinned on the CPU by
test_strands_host.py); the larger cases below use the oracle on T(genomes).
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

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "bioinformatics-project-for-shotgun-metagenomics-pseudo-alignment-shotgun-_amd")
GOLD = os.path.join(REPO, "tests", "golden")
MAIN = os.path.join(PKG, "main.py")
TYPE = {0: "DROPPED", 1: "UNMAPPED", 2: "UNIQUELY_MAPPED", 3: "AMBIGUOUSLY_MAPPED"}

with open(os.path.join(GOLD, "strand_cases.json")) as _f:
    STRAND = json.load(_f)
with open(os.path.join(GOLD, "lookup_cases.json")) as _f:
    LOOKUP = json.load(_f)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


def T(genomes):
    return [synth.both_strands_genome(g) for g in genomes]


def reads_of(reads):
    seq, off = N.concat([r[1] for r in reads])
    qual, _ = N.concat([r[2] for r in reads])
    return seq, qual, off


def counters(index, reads, prm, base=0):
    res = N.Result(index)
    N.align(index, reads, prm, base, res)
    out = [a.tolist() for a in res.fetch()]
    res.close()
    return out


def oracle_counters(o):
    ofk = np.where(o.first_key == np.iinfo(np.uint64).max, N.NO_FIRST_KEY, o.first_key)
    return [o.stats.tolist(), o.unique.tolist(), o.ambiguous.tolist(), ofk.tolist()]


def summary_from_counters(idents, stats, uq, am, fk, ps):
    """get_summary from per-genome counters + first-appearance keys (as kmer.py does)."""
    st = {"unique_mapped_reads": int(stats[0]), "ambiguous_mapped_reads": int(stats[1]),
          "unmapped_reads": int(stats[2])}
    if ps["mrq"] is not None:
        st["filtered_quality_reads"] = int(stats[3])
    if ps["mkq"] is not None:
        st["filtered_quality_kmers"] = int(stats[4])
    if ps["mg"] is not None:
        st["filtered_hr_kmers"] = int(stats[5])
    counts, first = {}, {}
    for g in np.flatnonzero(np.asarray(fk, dtype=np.uint64) != N.NO_FIRST_KEY):
        name = idents[g]
        c = counts.setdefault(name, [0, 0])
        c[0] += int(uq[g])
        c[1] += int(am[g])
        first[name] = min(first.get(name, 1 << 64), int(fk[g]))
    return {"Statistics": st, "Summary": {n: {"unique_reads": counts[n][0], "ambiguous_reads": counts[n][1]}
                                          for n in sorted(first, key=first.get)}}


# ---- 1. golden: the reference on T(genomes) -----------------------------------------

@pytest.mark.parametrize("case", STRAND["cases"], ids=[c["name"] for c in STRAND["cases"]])
def test_golden_strand_cases(case):
    """Per-read results and summaries of a both-strand index of the RAW genomes
    vs the reference's on T(genomes)."""
    idents = [g[0] for g in case["genomes"]]
    index = N.Index([g[1] for g in case["genomes"]], case["k"], both_strands=True)
    assert index.n_kmers == case["n_kmers"]
    kms = [km for km, _ in case["kmer_sets"]]
    cls, size = index.lookup(kms)
    for (km, gl), c, s in zip(case["kmer_sets"], cls, size):
        assert c >= 0 and int(s) == len(gl), km
        assert index.class_genomes(int(c)) == gl, km
    seq, qual, off = reads_of(case["reads"])
    reads = N.Reads.upload(seq, qual, off)
    for res in case["results"]:
        ps = res["params"]
        prm = N.Params.make(ps["m"], ps["p"], ps["mrq"], ps["mkq"], ps["mg"])
        types, qf, hr, loff, lists = N.align_detail(index, reads, prm)
        for r, (rid, tname, glist, eqf, ehr) in enumerate(res["reads"]):
            assert TYPE[int(types[r])] == tname, (rid, ps)
            assert [idents[g] for g in lists[loff[r]:loff[r + 1]]] == glist, (rid, ps)
            assert (int(qf[r]), int(hr[r])) == (eqf, ehr), (rid, ps)
        stats, uq, am, fk = counters(index, reads, prm)
        summ = summary_from_counters(idents, stats, uq, am, fk, ps)
        assert json.dumps(summ, indent=4) == res["summary_text"], ps
    reads.close()
    index.close()


# ---- 2. the align kernels against the oracle on T(genomes) ---------------------------

MID_PSETS = [dict(), dict(m=0, p=0), dict(mrq=58, mkq=60, mg=2)]


@functools.lru_cache(maxsize=None)
def mid_genomes():
    gens = synth.family_genomes(10, 30000, seed=81, family_size=3, sub_rate=0.01, conserved_len=500,
                                n_rate=2e-4, n_run=8)
    rng = np.random.default_rng(82)
    for g in gens:  # inverted repeats and an (ACGT)16 run, as test_reverse_strand_walk_vs_oracle
        for _ in range(20):
            ln = int(rng.integers(40, 400))
            a0 = int(rng.integers(0, len(g) - 2 * ln - 1))
            b0 = int(rng.integers(a0 + ln, len(g) - ln))
            g[b0:b0 + ln] = synth.reverse_complement(g[a0:a0 + ln])
        p0 = int(rng.integers(0, len(g) - 64))
        g[p0:p0 + 64] = np.frombuffer(b"ACGT" * 16, dtype=np.uint8)
    for g in gens:  # a hairpin at every genome's end: k-mers repeat within 255 positions across the join
        g[-300:] = synth.reverse_complement(g[-700:-400])
    return tuple(gens)


@functools.lru_cache(maxsize=None)
def mid_reads():
    seq, qual, _ = synth.sample_reads(mid_genomes(), 20000, 150, seed=5, err_rate=0.006)
    seq[1::2] = synth.reverse_complement(seq[1::2])
    qual[1::2] = qual[1::2, ::-1]
    return seq.tobytes(), qual.tobytes(), np.arange(20001, dtype=np.uint64) * 150


@functools.lru_cache(maxsize=None)
def mid_oracle(k, strands):
    """The oracle's counters for every parameter set, computed once per k:
    strands = 2 on T(genomes), 1 on the genomes themselves."""
    gens = mid_genomes()
    oix = O.OracleIndex(T(gens) if strands == 2 else list(gens), k)
    s, q, off = mid_reads()
    out = []
    for ps in (MID_PSETS if strands == 2 else MID_PSETS[:1]):
        out.append(oracle_counters(oix.align(s, q, off, read_base=7, detail=False, **ps)))
    return oix.n_kmers, out


@pytest.mark.parametrize("variant", ["default", "compact", "prepared", "large"])
@pytest.mark.parametrize("k", [31, 32, 63, 75])
def test_align_kernels_vs_oracle_on_t_genomes(k, variant, monkeypatch):
    """20 000 reads of 150 bases, every second one on the reverse strand, against
    a both-strand index built four ways (default; compact table, tiles without
    neighbour bits; tiles with neighbour bits; the large-reference layout):
    counters and first keys equal the oracle's on T(genomes)."""
    if variant == "large":
        monkeypatch.setenv("PA_LAYOUT", "large")
    n_kmers, expect = mid_oracle(k, 2)
    s, q, off = mid_reads()
    n = len(off) - 1
    if variant == "compact":
        index = N.Index(list(mid_genomes()), k, both_strands=True, defer_tiles=True, compact=True)
        index.prepare(expected_reads=n)
    elif variant == "prepared":
        index = N.Index(list(mid_genomes()), k, both_strands=True, defer_tiles=True)
        index.prepare()
    else:
        index = N.Index(list(mid_genomes()), k, both_strands=True)
    assert index.n_kmers == n_kmers
    reads = N.Reads.upload(np.frombuffer(s, dtype=np.uint8), np.frombuffer(q, dtype=np.uint8), off)
    for ps, exp in zip(MID_PSETS, expect):
        prm = N.Params.make(ps.get("m", 1), ps.get("p", 1), ps.get("mrq"), ps.get("mkq"), ps.get("mg"))
        assert counters(index, reads, prm, base=7) == exp, ps
    reads.close()
    index.close()


@pytest.mark.parametrize("k", [31, 32])
def test_reverse_reads_map_on_both_strands_only(k):
    """What the feature is for, stated on the ORACLE's numbers (never libpa's):
    forward-only leaves the reverse-strand half mostly unmapped (measured 5417 /
    5467 of 20 000), both strands leave almost none (measured 0)."""
    fwd_unmapped = mid_oracle(k, 1)[1][0][0][2]
    both_unmapped = mid_oracle(k, 2)[1][0][0][2]
    print(f"k={k}: forward oracle unmapped {fwd_unmapped}, both-strand oracle unmapped {both_unmapped}")
    assert fwd_unmapped >= 5000
    assert both_unmapped <= 100


# ---- 3. reduce ---------------------------------------------------------------------

@pytest.mark.parametrize("inplace", [False, True], ids=["gather", "inplace"])
def test_reduce_keeps_both_strands(inplace, monkeypatch):
    """A deferred both-strand index reduced to its even genomes equals the oracle
    on T of the kept genomes (whole regions are gathered; PA_REDUCE_INPLACE=1:
    compacted inside the old codes buffer)."""
    if inplace:
        monkeypatch.setenv("PA_REDUCE_INPLACE", "1")
    k = 31
    gens = list(mid_genomes())
    sel = list(range(0, len(gens), 2))
    index = N.Index(gens, k, both_strands=True, defer_tiles=True)
    # strandness is fixed at the build: the bit is not one of reduce's flags
    assert N.lib().pa_index_reduce(index.handle, None, 0, N.PA_BUILD_BOTH_STRANDS, None) == N.PA_EINVAL
    index.reduce(sel)
    assert index.both_strands and index.strands() == 1 and index.n_genomes == len(sel)
    kept = [gens[i] for i in sel]
    oix = O.OracleIndex(T(kept), k)
    info = index.info()
    assert info.n_kmers == oix.n_kmers and info.n_genomes == len(sel)
    assert info.total_windows == 2 * sum(len(g) - k + 1 for g in kept)
    s, q, off = mid_reads()
    reads = N.Reads.upload(np.frombuffer(s, dtype=np.uint8), np.frombuffer(q, dtype=np.uint8), off)
    for ps in MID_PSETS[:2]:
        exp = oracle_counters(oix.align(s, q, off, read_base=7, detail=False, **ps))
        assert counters(index, reads, N.Params.make(ps.get("m", 1), ps.get("p", 1)), base=7) == exp, ps
    # forward views still speak the kept genomes' coordinates
    fwd = N.Index(kept, k)
    kms = [bytes(g[p:p + k]).decode() for g in gens[:4] for p in (0, 100, len(g) - k)]
    for rev in (False, True):
        assert index.positions(kms, reverse=rev).tolist() == fwd.positions(kms, reverse=rev).tolist()
    for h in (reads, index, fwd):
        h.close()


# ---- 4. edge genomes -----------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 31])
def test_edge_genomes(k):
    """Genomes of 0, 1, k-1, k, k+1 and 2k bases, one of N only and a pure (ACGT)n
    one: n_kmers and every k-mer's genome list equal the T-oracle's export()."""
    rng = np.random.default_rng(900 + k)
    gens = [synth.ACGT[rng.integers(0, 4, size=n)] for n in (0, 1, k - 1, k, k + 1, 2 * k)]
    gens += [np.frombuffer(b"N" * (k + 3), dtype=np.uint8), np.frombuffer(b"ACGT" * (k + 2), dtype=np.uint8)]
    # (ACGT)n windows also occur in a random genome's tail, so that sets of two genomes exist
    gens.append(np.concatenate([synth.ACGT[rng.integers(0, 4, size=3 * k)], np.frombuffer(b"ACGT" * k, np.uint8)]))
    index = N.Index(gens, k, both_strands=True)
    got_o = O.OracleIndex(T(gens), k).export()
    info = index.info()
    assert info.n_kmers == len(got_o)
    assert info.total_windows == 2 * sum(len(g) - k + 1 for g in gens if len(g) >= k)
    kms = list(got_o)
    cls, size = index.lookup(kms)
    for km, c, s in zip(kms, cls, size):
        assert c >= 0 and index.class_genomes(int(c)) == got_o[km] and int(s) == len(got_o[km]), km
    # the windows across the join hold its N: not indexed
    absent = [bytes(synth.both_strands_genome(g))[len(g) - k + 1 + i:len(g) + 1 + i].decode()
              for g in gens if len(g) >= k for i in (0, k - 1)]
    cls, _ = index.lookup(absent)
    assert all(c < 0 for c in cls)
    index.close()


def test_bad_byte_offset_is_the_callers():
    """The PA_EINVAL message names the bad byte's offset in the caller's text, on
    either path of the expansion kernel (inside a 16-byte run, at a genome's end)."""
    rng = np.random.default_rng(5)
    for at in (0, 37, 999, 1000, 1663):
        gens = [bytearray(synth.ACGT[rng.integers(0, 4, size=n)]) for n in (1000, 0, 664)]
        text = bytearray(b"".join(gens))
        text[at] = ord("x")
        with pytest.raises(ValueError, match=rf"\(byte {at}\)"):
            N.Index([bytes(text[:1000]), b"", bytes(text[1000:])], 21, both_strands=True)


# ---- 5. forward views unchanged ---------------------------------------------------------

@pytest.mark.parametrize("case", LOOKUP, ids=[c["name"] for c in LOOKUP])
def test_positions_are_forward(case):
    seqs = [g[1] for g in case["genomes"]]
    both = N.Index(seqs, case["k"], both_strands=True)
    fwd = N.Index(seqs, case["k"])
    assert (both.strands(), fwd.strands()) == (1, 0)
    kms = [q[0] for q in case["queries"]]
    for rev in (False, True):
        a, b = both.positions(kms, reverse=rev), fwd.positions(kms, reverse=rev)
        assert a.tolist() == b.tolist()
    assert len(fwd.positions(kms, reverse=True)) > 0
    both.close()
    fwd.close()


def test_synthesized_reads_are_forward():
    gens = list(mid_genomes())[:4] + [np.frombuffer(b"ACGT" * 20, dtype=np.uint8)]
    both = N.Index(gens, 31, both_strands=True, defer_tiles=True)
    fwd = N.Index(gens, 31, defer_tiles=True)
    for kw in (dict(), dict(rc_rate=0.4, foreign_rate=0.1)):
        for read_len in (150, 80):  # (80: the short genome is eligible too)
            a = N.Reads.synthesize(both, 3000, read_len, first_read=11, seed=83, sub_rate=0.01, **kw)
            b = N.Reads.synthesize(fwd, 3000, read_len, first_read=11, seed=83, sub_rate=0.01, **kw)
            for x, y in zip(a.download(), b.download()):
                assert np.array_equal(x, y)
            a.close()
            b.close()
    with pytest.raises(ValueError):  # longer than every forward half (though not than every region)
        N.Reads.synthesize(both, 10, 40000, seed=1)
    both.close()
    fwd.close()


# ---- 6. EXTSIM -------------------------------------------------------------------------

def _container(genomes):
    from records import FASTARecordContainer
    c = FASTARecordContainer()
    c.parse_records("".join(f">{h}\n{s}\n" for h, s in genomes))
    return c


@functools.lru_cache(maxsize=None)
def extsim_genomes():
    gens = synth.family_genomes(8, 3000, seed=100, family_size=4, sub_rate=0.002, conserved_len=200, n_rate=0.0,
                                n_run=0)
    gens[5][:] = synth.reverse_complement(gens[4])  # a genome given on the other strand: similar only on both
    return tuple((f"sim_{i} family", bytes(g).decode()) for i, g in enumerate(gens))


def test_extsim_on_both_strands():
    from kmer import KmerReference
    genomes = extsim_genomes()
    idents = [h for h, _ in genomes]  # (a record's identifier is its whole header line)
    seqs = [s for _, s in genomes]
    k = 21
    oix = O.OracleIndex(T(seqs), k)
    index = N.Index(seqs, k, both_strands=True, defer_tiles=True)
    group_of = list(range(len(seqs)))
    for a, b in zip(index.extsim_stats(group_of, len(seqs)), oix.extsim_stats(group_of, len(seqs))):
        assert a.tolist() == b.tolist()
    index.close()
    kept, info = O.extsim(idents, [len(s) for s in seqs], oix, 0.9)
    ref = KmerReference(k, _container(genomes), filter_similar=True, similarity_threshold=0.9, both_strands=True)
    assert json.dumps(ref.similarity_info, indent=4) == json.dumps(info, indent=4)
    assert [g.identifier for g in ref.genomes] == [idents[i] for i in kept]
    assert ref.index.both_strands and ref.index.strands() == 1  # (reduce kept it)
    assert ref.n_kmers == O.OracleIndex(T([seqs[i] for i in kept]), k).n_kmers
    # the reverse-strand copy is dropped only when both strands are compared
    fwd_kept, _ = O.extsim(idents, [len(s) for s in seqs], O.OracleIndex(seqs, k), 0.9)
    assert (4 in fwd_kept and 5 in fwd_kept) and not (4 in kept and 5 in kept)


# ---- 7. dumpref ------------------------------------------------------------------------

def test_dumpref_is_of_the_forward_database(tmp_path):
    from kmer import KmerReference
    genomes = [("dup x", "ACGTTGCAACGTAACNNACGTTG"), ("other", "TTGCAACGTAACGGT"), ("dup x", "CAACGTAACGGTTTT"),
               ("short", "ACG"), ("rc", O.reverse_complement("TTGCAACGTAACGGT"))]
    both = KmerReference(5, _container(genomes), both_strands=True)
    fwd = KmerReference(5, _container(genomes))
    with open(tmp_path / "kmers.json", "wb") as f:
        with pytest.raises(N.PaUnsupported, match="both-strand"):
            N.index_dumpref(both.index, None, np.zeros(len(genomes), dtype=np.uint32), ['"d"'], f.fileno())
    a, b = both.get_summary(), fwd.get_summary()
    assert json.dumps(a["Kmers"], indent=4) == json.dumps(b["Kmers"], indent=4) and len(b["Kmers"]) > 0
    assert a == b
    assert both.n_kmers > fwd.n_kmers == len(fwd.kmers) == len(both.kmers)

    def named(refs):  # (the two references hold records of their own)
        return [(g["description"], g["genome"], sorted(p)) for g, p in refs.items()]
    assert named(both.get_kmer_references("ACGTT")) == named(fwd.get_kmer_references("ACGTT")) != []
    assert named(both.get_kmer_and_reverse_references("ACGTT")) == named(fwd.get_kmer_and_reverse_references("ACGTT"))
    assert len(named(fwd.get_kmer_and_reverse_references("ACGTT"))) > len(named(fwd.get_kmer_references("ACGTT")))
    # with EXTSIM: the dump of the kept genomes, in the full build's order
    sim = extsim_genomes()
    both = KmerReference(21, _container(sim), filter_similar=True, similarity_threshold=0.9, both_strands=True)
    kept = {g.identifier for g in both.genomes}
    assert len(kept) < len(sim)
    exp = O.dumpref_summary([(h, s) for h, s in sim], 21, kept, both.similarity_info)
    assert json.dumps(both.get_summary(), indent=4) == json.dumps(exp, indent=4)


# ---- 8. CLI ----------------------------------------------------------------------------

def _cli(args, gpus=1):
    env = dict(os.environ, PA_CLI_TIMING="1")
    env.pop("PA_GPUS", None)
    if gpus > 1:
        env.update(PA_GPUS=str(gpus), PA_GPUS_SHARE="1")
    return subprocess.run([sys.executable, MAIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=300, env=env)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("strands")
    case = next(c for c in STRAND["cases"] if c["name"] == STRAND["cli"]["case"])
    fastq = "".join(f"@{i}\n{s}\n+\n{q}\n" for i, s, q in case["reads"])
    (d / "raw.fa").write_text("".join(f">{h}\n{s}\n" for h, s in case["genomes"]))
    (d / "reads.fq").write_text(fastq)
    with gzip.open(d / "reads.fq.gz", "wt") as f:
        f.write(fastq)
    return d


@pytest.mark.parametrize("how", ["fq", "gz", "sharded"])
def test_cli_dumpalign_both_strands(cli_files, how):
    """dumpalign --both-strands on the RAW FASTA prints, byte for byte, what the
    reference CLI prints for the T-FASTA."""
    cli = STRAND["cli"]
    reads = cli_files / ("reads.fq.gz" if how == "gz" else "reads.fq")
    for run in cli["runs"]:
        r = _cli(["-t", "dumpalign", "-g", str(cli_files / "raw.fa"), "-k", str(cli["k"]), "--reads", str(reads),
                  "--both-strands"] + run["flags"], gpus=2 if how == "sharded" else 1)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout == run["stdout"], run["flags"]
        if how == "sharded":
            assert "reads aligned (sharded)" in r.stderr, r.stderr[-2000:]
    # without the flag the reverse-strand half stays unmapped: the flag is what changes the output
    r = _cli(["-t", "dumpalign", "-g", str(cli_files / "raw.fa"), "-k", str(cli["k"]), "--reads", str(reads),
              "--reverse-complement"])
    assert r.returncode == 0 and r.stdout != cli["runs"][0]["stdout"]


def test_cli_reference_file_carries_the_property(cli_files):
    cli = STRAND["cli"]
    fa, fq = str(cli_files / "raw.fa"), str(cli_files / "reads.fq")
    both, fwd = str(cli_files / "both.kdb"), str(cli_files / "fwd.kdb")
    r = _cli(["-t", "reference", "-g", fa, "-k", str(cli["k"]), "-r", both, "--both-strands"])
    assert r.returncode == 0, r.stderr[-2000:]
    r = _cli(["-t", "reference", "-g", fa, "-k", str(cli["k"]), "-r", fwd])
    assert r.returncode == 0, r.stderr[-2000:]
    for extra in ([], ["--both-strands"]):  # with -r the stored property decides
        r = _cli(["-t", "dumpalign", "-r", both, "--reads", fq] + extra)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout == cli["runs"][0]["stdout"]
    r = _cli(["-t", "dumpalign", "-r", fwd, "--reads", fq, "--both-strands"])
    assert r.returncode != 0 and r.stdout == ""
    err = [ln for ln in r.stderr.splitlines() if not ln.startswith("[pa_")]
    assert len(err) == 1 and "forward-only" in err[0] and "rebuild" in err[0] and "--both-strands" in err[0]
