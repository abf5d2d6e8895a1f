"""K-mer containment on the GPU (pa_containment_*, Containment,
PseudoAlignment(containment=True), main.py --containment).

The reference has no such code.  The model is tests/test_containment_host.py's:
plain Python from the genome texts, nothing of libpa in it.  Every comparison
is exact integer equality (the derived ratios are compared as the text the
model formats from its own integers).
"""

import functools
import io

import numpy as np
import pytest

import pa_native as N
import test_abundance_host as M
import test_containment_host as CM
import test_gpu_abundance as A
import test_gpu_coverage as TC
import test_gpu_index_variants as V
import test_gpu_lineage as GL
import test_lineage_host as L

pytestmark = pytest.mark.gpu

ARRAYS, INFO = CM.ARRAYS, CM.INFO
WINDOW_COUNTERS = ("windows_retained", "windows_filtered_quality", "windows_filtered_hr", "windows_absent")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


def lists(arrays):
    return {n: [int(x) for x in arrays[n]] for n in ARRAYS}


def check_info(info):
    assert sum(info[n] for n in WINDOW_COUNTERS) == info["windows"], info


def check_device(index, dev, ps, want):
    """A fresh accumulator after one add of `dev`: the arrays and the info against the model's (arrays, info)."""
    con = N.Containment(index)
    con.add(dev, A.params(ps))
    got, info = con.counts()
    assert info == want[1]
    check_info(info)
    assert lists(got) == want[0]
    return con


def check_totals(index, arrays):
    """kmers / specific are pa_index_extsim_stats' total / uniq under the identity grouping."""
    G = index.n_genomes
    total, uniq, _ = index.extsim_stats(list(range(G)), G)
    assert [int(x) for x in total] == arrays["kmers"] and [int(x) for x in uniq] == arrays["specific"]


# ---- 1. hand-built ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hand_case(k):
    """test_gpu_abundance's hand-built genomes and reads, plus a read of exactly k
    bases and one that holds the same k-mers twice."""
    genomes, reads = A.hand_case(k)
    S3 = genomes[0][k + 70:k + 70 + 2 * k + 140]
    more = [("exactly_k", S3[7:7 + k]), ("twice", S3[3:k + 9] + S3[3:k + 9])]
    return genomes, list(reads) + [(n, s, "I" * len(s)) for n, s in more]


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
@pytest.mark.parametrize("k", [31, 32, 63, 64, 127])  # the key-width edges; 32 and 64: a top word of zero bits
def test_hand_built(k, both):
    genomes, reads = hand_case(k)
    names, seqs, quals = [r[0] for r in reads], [r[1] for r in reads], [r[2] for r in reads]
    kd = M.kmer_sets(genomes, both, k)
    want = CM.model(genomes, both, k, seqs, quals, A.HAND_PS, kd)
    arrays, info = want
    # the corners are what they are named for
    alone = {n: CM.mark(kd, k, 3, [s], [q], **A.HAND_PS) for n, s, q in reads}
    one = {n: v[2] for n, v in alone.items()}
    assert one["short"]["windows"] == 0 and one["exactly_k"]["windows"] == one["exactly_k"]["windows_retained"] == 1
    assert one["dropped"]["reads_dropped"] == 1 and one["dropped"]["windows"] == 0
    assert one["with_n"]["windows_absent"] == k
    assert one["twice"]["windows_retained"] >= 14 and one["twice"]["windows_absent"] >= k - 10
    assert one["twice"]["windows_retained"] >= len(alone["twice"][0]) + 7   # seven k-mers met twice
    assert one["reverse"]["windows_retained"] == (one["reverse"]["windows"] if both else 0)
    assert all(arrays["kmers"][g] > arrays["kmers_seen"][g] > arrays["specific_seen"][g] > 0 for g in range(3))
    assert info["reads"] == len(reads) and info["reads_dropped"] == 1
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, k, both_strands=both)
    con = check_device(index, dev, A.HAND_PS, want)
    check_totals(index, arrays)
    for x in (con, dev, index):
        x.close()


# ---- 2. window-count edges -------------------------------------------------------------------

@pytest.mark.parametrize("ps", [dict(), dict(mkq=62)], ids=["plain", "mkq"])
@pytest.mark.parametrize("k", [31, 127])
def test_window_counts(k, ps):
    """63 / 64 / 65 windows (one wave of lanes), 128 / 129 (the align pass's quality masks), 256 / 257 (one
    staging of the mark kernel), and a read of 5000 bases; with mkq the window sums cross every one of them."""
    rng = np.random.default_rng(40 + k)
    genomes = [TC.rand_dna(rng, 6000), TC.rand_dna(rng, 700)]
    seqs, quals = [], []
    for extra in (62, 63, 64, 127, 128, 255, 256):
        for rep in range(3):
            ln = k + extra
            a = int(rng.integers(0, len(genomes[0]) - ln + 1))
            seqs.append(TC.mutate(rng, genomes[0][a:a + ln], 0.01))
    seqs.append(TC.mutate(rng, genomes[0][400:5400], 0.002))
    seqs.append(genomes[0][0:5000])
    for s in seqs:
        quals.append(bytes(rng.integers(50, 75, len(s), dtype=np.uint8)).decode())
    want = CM.model(genomes, False, k, seqs, quals, ps)
    assert want[1]["windows"] == sum(len(s) - k + 1 for s in seqs)
    if ps:
        assert 0.2 * want[1]["windows"] < want[1]["windows_filtered_quality"] < 0.8 * want[1]["windows"]
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, k)
    con = check_device(index, dev, ps, want)
    for x in (con, dev, index):
        x.close()


# ---- 3. filters ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rand_kd(both):
    return A.rand_kd() if not both else M.kmer_sets(A.rand_strains(), True, A.RAND_K)


@pytest.mark.parametrize("ps", [dict(mkq=61), dict(mg=2), dict(mrq=62, mkq=58, mg=2)], ids=["mkq", "mg", "all"])
def test_filters_count_what_pa_align_counts(ps):
    seqs, quals = A.rand_reads()
    seqs, quals = list(seqs[:1500]), list(quals[:1500])
    want = CM.model(A.rand_strains(), False, A.RAND_K, seqs, quals, ps, rand_kd(False))
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(A.rand_strains(), A.RAND_K)
    con = check_device(index, dev, ps, want)
    res = N.Result(index)
    N.align(index, dev, A.params(ps), 0, res)
    stats = [int(x) for x in res.fetch()[0]]
    _, info = con.counts()
    assert info["reads_dropped"] == stats[3]
    assert info["windows_filtered_quality"] == stats[4] and info["windows_filtered_hr"] == stats[5]
    assert stats[4] + stats[5] > 0 and ("mrq" not in ps or stats[3] > 100)
    for x in (con, res, dev, index):
        x.close()


# ---- 4. shared bitset words ------------------------------------------------------------------

def test_marks_in_shared_words():
    """40 distinct k-mers in a table of a few bitset words, 4000 reads over them at once: a mark made with a
    plain store would lose bits of a word that two lanes write."""
    k = 31
    rng = np.random.default_rng(77)
    genomes = [TC.rand_dna(rng, k + 29), TC.rand_dna(rng, k + 9)]
    seqs = []
    for i in range(4000):
        g = genomes[i % 2]
        ln = int(rng.integers(k, len(g) + 1))
        a = int(rng.integers(0, len(g) - ln + 1))
        seqs.append(g[a:a + ln])
    quals = ["I" * len(s) for s in seqs]
    want = CM.model(genomes, False, k, seqs, quals)
    assert want[0]["kmers"] == want[0]["kmers_seen"] == [30, 10]   # every k-mer is met
    dev, _ = TC.upload(seqs, quals)
    for compact in (False, True):
        index = N.Index(genomes, k, compact=compact)
        assert int(index.info().table_slots) <= 256
        con = check_device(index, dev, {}, want)
        con.close()
        index.close()
    dev.close()


# ---- 5. many genomes -------------------------------------------------------------------------

@pytest.mark.parametrize("lds", [True, False], ids=["lds_histogram", "global_atomics"])
@pytest.mark.parametrize("G, length, stretch, k, n_reads", [(300, 500, 200, 31, 90), (2100, 70, 40, 21, 60)],
                         ids=["300_genomes", "2100_genomes"])
def test_many_genomes(G, length, stretch, k, n_reads, lds, monkeypatch):
    """A class of every genome (300: larger than a wave and a workgroup), and a genome count past the LDS
    histograms (2100 x 2 counters in the scan; PA_CONTAIN_LDS=0: the global atomics below that count too)."""
    if not lds:
        monkeypatch.setenv("PA_CONTAIN_LDS", "0")
    genomes, seqs, quals = A.large_case(G, length, stretch, k, n_reads)
    want = CM.model(genomes, False, k, seqs, quals)
    assert min(want[0]["kmers_seen"]) > 0 and sum(want[0]["hits_specific"]) > 0
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, k)
    con = check_device(index, dev, {}, want)
    check_totals(index, want[0])
    for x in (con, dev, index):
        x.close()


# ---- 6. random strains -----------------------------------------------------------------------

@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
@pytest.mark.parametrize("i", range(len(A.RAND_PS)),
                         ids=[",".join(f"{a}={b}" for a, b in ps.items()) for ps in A.RAND_PS])
def test_random_strains(i, both):
    seqs, quals = A.rand_reads()
    ps = {n: v for n, v in A.RAND_PS[i].items() if n in ("mrq", "mkq", "mg")}   # (m and p are ignored)
    want = CM.model(A.rand_strains(), both, A.RAND_K, seqs, quals, ps, rand_kd(both))
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(A.rand_strains(), A.RAND_K, both_strands=both)
    con = N.Containment(index)
    con.add(dev, A.params(A.RAND_PS[i]))   # with the set's own m and p: the result must not depend on them
    got, info = con.counts()
    assert info == want[1] and lists(got) == want[0]
    check_info(info)
    for x in (con, dev, index):
        x.close()


# ---- 7. batches and lifetime -----------------------------------------------------------------

def test_batches_reset_and_errors():
    genomes = A.rand_strains()
    seqs, quals = A.rand_reads()
    seqs, quals = list(seqs[:1800]), list(quals[:1800])
    ps = dict(mkq=58, mg=2)
    prm = A.params(ps)
    index, other = N.Index(genomes, A.RAND_K), N.Index(genomes, A.RAND_K)
    whole, _ = TC.upload(seqs, quals)
    parts = [TC.upload(seqs[a:b], quals[a:b])[0] for a, b in ((0, 500), (500, 1300), (1300, 1800))]
    one, three = N.Containment(index), N.Containment(index)
    b0 = int(index.info().device_bytes)
    one.add(whole, prm)
    for p in parts:
        three.add(p, prm)
    assert int(index.info().device_bytes) == b0   # the accumulator's bytes are not the index's
    a1, i1 = one.counts()
    a3, i3 = three.counts()
    assert lists(a1) == lists(a3) == CM.model(genomes, False, A.RAND_K, seqs, quals, ps, rand_kd(False))[0]
    assert i1 == i3
    # the same batch again: the hits and the counters double, what is seen stays
    one.add(whole, prm)
    a2, i2 = one.counts()
    assert i2 == {n: 2 * v for n, v in i1.items()}
    assert [int(x) for x in a2["hits_specific"]] == [2 * int(x) for x in a1["hits_specific"]]
    for n in ("kmers", "kmers_seen", "specific", "specific_seen"):
        assert a2[n].tolist() == a1[n].tolist()
    # reset
    three.reset()
    a0, i0 = three.counts()
    assert i0 == dict.fromkeys(INFO, 0) and a0["kmers"].tolist() == a1["kmers"].tolist()
    assert not a0["kmers_seen"].any() and not a0["specific_seen"].any() and not a0["hits_specific"].any()
    three.add(whole, prm)
    assert lists(three.counts()[0]) == lists(a1)
    # NULL outputs
    lib = N.lib()
    assert lib.pa_containment_counts(one.handle, None, None, None, None, None, None, None) == N.PA_OK
    seen = np.zeros(len(genomes), dtype=np.uint64)
    assert lib.pa_containment_counts(one.handle, None, N._ptr(seen), None, None, None, None, None) == N.PA_OK
    assert seen.tolist() == a1["kmers_seen"].tolist()
    # another index; its own index after a reduce
    assert lib.pa_containment_add(other.handle, whole.handle, prm, one.handle, None) == N.PA_EINVAL
    index.reduce([0, 2, 3, 5])
    with pytest.raises(ValueError):
        one.add(whole, prm)
    with pytest.raises(ValueError):
        one.counts()
    for x in [one, three, whole, index, other] + parts:
        x.close()


# ---- 8. layouts ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def layout_batch(k, both):
    seqs, quals = A.rand_reads()
    seqs, quals = list(seqs[:300]), list(quals[:300])
    ps = dict(mkq=58, mg=2)
    return seqs, quals, ps, CM.model(A.rand_strains(), both, k, seqs, quals, ps)


def layout_cells():
    out = []
    for variant in V.VARIANTS:
        out.append((variant, 31, False))
        if variant in V.BOTH_TOO:
            out.append((variant, 31, True))
        if variant in V.WIDE:
            out.append((variant, 63, False))
    return out


@pytest.mark.parametrize("variant, k, both", layout_cells(), ids=[f"{v}-k{k}-{'both' if b else 'fwd'}"
                                                                   for v, k, b in layout_cells()])
def test_layouts(variant, k, both):
    seqs, quals, ps, want = layout_batch(k, both)
    dev, _ = TC.upload(seqs, quals)
    with V.variant_env(variant):
        index, snap = V.make(variant, A.rand_strains(), k, both, len(seqs))
        before = int(index.info().device_bytes)
        con = check_device(index, dev, ps, want)
        check_totals(index, want[0])
        # the pass made no align-side view: a deferred index is still deferred
        assert int(index.info().device_bytes) == before
        if variant == "deferred":
            index.prepare()
            assert int(index.info().device_bytes) > before
            got, info = con.counts()   # (the view changes no slot: the accumulator stays valid)
            assert lists(got) == want[0] and info == want[1]
    for x in (con, dev, index):
        x.close()


# ---- 9. nodes --------------------------------------------------------------------------------

NODE_K = 21


@functools.lru_cache(maxsize=None)
def node_genomes():
    """test_gpu_lineage's genome count; all genomes share one stretch, every seven consecutive ones another."""
    rng = np.random.default_rng(31)
    S = TC.rand_dna(rng, NODE_K + 4)
    out, block = [], ""
    for g in range(GL.LCA_G):
        if g % 7 == 0:
            block = TC.rand_dna(rng, NODE_K + 5)
        out.append(TC.rand_dna(rng, NODE_K + 8) + (S if g % 3 else "") + TC.rand_dna(rng, 3) + block)
    return out


@functools.lru_cache(maxsize=None)
def node_world():
    genomes = node_genomes()
    kd = M.kmer_sets(genomes, False, NODE_K)
    rng = np.random.default_rng(37)
    seqs = []
    for i in range(300):
        g = genomes[int(rng.integers(0, len(genomes)))]
        ln = int(rng.integers(NODE_K, len(g) + 1))
        a = int(rng.integers(0, len(g) - ln + 1))
        seqs.append(g[a:a + ln])
    quals = ["I" * len(s) for s in seqs]
    seen, hits, info = CM.mark(kd, NODE_K, len(genomes), seqs, quals)
    return kd, seqs, quals, seen


@pytest.fixture(scope="module")
def node_index():
    index = N.Index(node_genomes(), NODE_K)
    seqs, quals = node_world()[1:3]
    dev, _ = TC.upload(seqs, quals)
    con = N.Containment(index)
    con.add(dev, A.params({}))
    dev.close()
    yield index, con
    con.close()
    index.close()


@pytest.mark.parametrize("kind", ["flat", "chain", "balanced", "random"])
def test_nodes(kind, node_index):
    index, con = node_index
    kd, _, _, seen = node_world()
    parent, genome_node = GL.lca_tree(kind)
    want = CM.per_node(kd, seen, parent, genome_node)
    assert sum(1 for x in want[0] if x) >= 3 and want[3][0] == len(seen) > 100
    lin = N.Lineage(index, parent, genome_node)
    got = con.nodes(lin)
    for g, w in zip(got, want):
        assert [int(x) for x in g] == w
    assert int(got[2][0]) == int(index.info().n_kmers) == len(kd)
    assert lib_nodes_null(con, lin) == N.PA_OK
    lin.close()


def lib_nodes_null(con, lin):
    return N.lib().pa_containment_nodes(con.handle, lin.handle, None, None, None, None, None)


def test_nodes_refuse_a_lineage_of_another_index(node_index):
    index, con = node_index
    other = N.Index(node_genomes()[:50], NODE_K)
    lin = N.Lineage(other, [0, 0], [1] * 50)
    with pytest.raises(ValueError):
        con.nodes(lin)
    lin.close()
    other.close()


# ---- 10. drop-in API and CLI -----------------------------------------------------------------

CLI_CASES, FA, FQ = TC.CLI_CASES, TC.FA, TC.FQ


@functools.lru_cache(maxsize=None)
def config1_model(both=False):
    gen, reads = TC.config1()
    gs = [g for _, g in gen]
    seqs, quals = [s for s, _ in reads], [q for _, q in reads]
    kd = M.kmer_sets(gs, both, 21)
    seen, hits, info = CM.mark(kd, 21, len(gs), seqs, quals)
    arrays = CM.per_genome(kd, len(gs), seen, hits)
    return kd, seen, arrays, info, CM.file_text([n for n, _ in gen], [len(g) for g in gs], 21, arrays, info)


def test_cli_containment(tmp_path):
    from data_file import FASTAFile
    from kmer import KmerReference, PseudoAlignment
    f = str(tmp_path / "c.tsv")
    r = TC.run_cli(["--containment", f])
    assert r.returncode == 0, r.stderr
    assert r.stdout == CLI_CASES[0]["stdout"]   # stdout: what is pinned without the flag
    kd, seen, arrays, info, text = config1_model()
    assert open(f).read() == text
    assert info["windows_retained"] > 0 and sum(arrays["kmers_seen"]) > 0
    r = TC.run_cli(["--both-strands", "--containment", f])
    assert r.returncode == 0 and open(f).read() == config1_model(True)[4]
    # the API
    ref = KmerReference(21, FASTAFile(FA).container)
    plain = PseudoAlignment(ref)
    for fn in (plain.get_containment, lambda: plain.write_containment(io.StringIO())):
        with pytest.raises(ValueError):
            fn()
    pa = PseudoAlignment(ref, containment=True)
    pa.align_reads_from_file(FQ)
    buf = io.StringIO()
    pa.write_containment(buf)
    assert buf.getvalue() == text
    rep = pa.get_containment()
    names = [n for n, _ in TC.config1()[0]]
    assert [g["genome"] for g in rep["genomes"]] == names and rep["info"] == info
    assert [g["genome"] for g in pa.get_containment([names[2], names[0]])["genomes"]] == [names[0], names[2]]
    with pytest.raises(ValueError):
        pa.get_containment(["not a genome"])
    assert not any("ontainment" in key for key in pa.__getstate__())   # (never part of an .aln file)
    with pytest.raises(ValueError):
        PseudoAlignment(ref, containment=True).align_pairs_from_containers([], [])


def test_cli_lineage_report_gains_the_clades_kmers(tmp_path):
    lf = GL.write_lineages(tmp_path / "lin.tsv")
    rep, rep0, f = str(tmp_path / "rep.tsv"), str(tmp_path / "rep0.tsv"), str(tmp_path / "c.tsv")
    r = TC.run_cli(["--lineages", lf, "--lineage-report", rep, "--containment", f])
    plain = TC.run_cli(["--lineages", lf, "--lineage-report", rep0])
    assert r.returncode == 0 and plain.returncode == 0, r.stderr + plain.stderr
    assert r.stdout == plain.stdout
    kd, seen, arrays, info, text = config1_model()
    assert open(f).read() == text
    ids = [n for n, _ in TC.config1()[0]]
    parent, names, genome_node = L.model_tree(ids, GL.config1_lineages())
    dk, ds, ck, cs = CM.per_node(kd, seen, parent, genome_node)
    got, base = open(rep).read().split("\n"), open(rep0).read().split("\n")
    assert len(got) == len(base) == len(parent) + 3
    assert got[0] == base[0] + "\tkmers_clade\tkmers_seen_clade\tkmer_containment"
    for line, line0, v in zip(got[1:-2], base[1:-2], L.preorder(parent)):
        assert line == line0 + f"\t{ck[v]}\t{cs[v]}\t{CM.f9(cs[v] / ck[v] if ck[v] else 0.0)}"
    assert got[-2:] == base[-2:]
    assert ck[0] == len(kd) and cs[0] == len(seen) and len({c for c in ck}) >= 3


def test_cli_containment_composes(tmp_path):
    lf = GL.write_lineages(tmp_path / "lin.tsv")

    def flags(tag):
        return ["--abundance", str(tmp_path / f"ab{tag}.tsv"), "--lineages", lf, "--lineage-report",
                str(tmp_path / f"rep{tag}.tsv"), "--coverage", "--assignments", str(tmp_path / f"as{tag}.tsv"),
                "--extract", str(tmp_path / f"x{tag}.fq")]
    f = str(tmp_path / "c.tsv")
    r, plain = TC.run_cli(flags(1) + ["--containment", f]), TC.run_cli(flags(2))
    assert r.returncode == 0 and plain.returncode == 0, r.stderr + plain.stderr
    assert r.stdout == plain.stdout
    for name in ("ab{}.tsv", "as{}.tsv", "x{}.fq"):
        assert open(str(tmp_path / name.format(1))).read() == open(str(tmp_path / name.format(2))).read()
    cut = [ln.rsplit("\t", 3)[0] for ln in open(str(tmp_path / "rep1.tsv")).read().split("\n")[:-2]]
    assert cut == open(str(tmp_path / "rep2.tsv")).read().split("\n")[:-2]
    assert open(f).read() == config1_model()[4]
    # the three filters and --filter-similar: the file's lines are the kept genomes', the counters pa_align's
    fs = ["--filter-similar", "--similarity-threshold", "0.5", "--min-read-quality", "40", "--min-kmer-quality",
          "45", "--max-genomes", "2"]
    r, plain = TC.run_cli(fs + ["--containment", f]), TC.run_cli(fs)
    assert r.returncode == 0 and plain.returncode == 0, r.stderr + plain.stderr
    assert r.stdout == plain.stdout
    lines = open(f).read().splitlines()
    assert lines[0].startswith("#genome\t") and lines[-1].startswith("#reads\t") and 3 <= len(lines) <= 5
