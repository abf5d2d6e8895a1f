"""Lineages on the GPU (pa_lineage_*, Lineage, PseudoAlignment(lineages=...),
main.py --lineages / --lineage-report).

The reference has no such code.  The model is tests/test_lineage_host.py's: a
read's node from the root paths of its compatibility set's genomes, no preorder
numbers in it; types and sets are tests/test_abundance_host.py's model, checked
against the CPU oracle on every batch (test_gpu_abundance.model_of).  Nodes and
counts are integers and are compared for exact equality.  The rolled-up
estimates of the CLI test are compared with sums of the abundance file's own
numbers: both files print format(x, ".9g"), a relative error of 5e-10 per
number, so a sum over g genomes is within (g + 1) * 5e-10 * (the largest term
or the sum) -- the bound used below is (g + 1) * 1e-9.
"""

import collections
import functools
import io
import os

import numpy as np
import pytest

import pa_native as N
import test_abundance_host as M
import test_gpu_abundance as A
import test_gpu_coverage as TC
import test_lineage_host as L

pytestmark = pytest.mark.gpu

UNIQUE, AMBIGUOUS, NO_NODE = M.UNIQUE, M.AMBIGUOUS, L.NO_NODE


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


def check_counts(lin, parent, nodes, types):
    """direct, clade and info of the accumulator against the model's per-read nodes."""
    direct, clade, info = lin.counts()
    md, mc = L.counts_of(parent, nodes)
    assert direct.tolist() == md and clade.tolist() == mc
    assert int(clade[0]) == types.count(UNIQUE) + types.count(AMBIGUOUS) == info["reads_unique"] + info["reads_ambiguous"]
    assert [info[n] for n in ("reads_unique", "reads_ambiguous", "reads_unmapped", "reads_dropped")] == \
        [types.count(x) for x in (UNIQUE, AMBIGUOUS, M.UNMAPPED, M.DROPPED)]
    assert info["n_nodes"] == len(parent)
    want = collections.Counter(v for v in nodes if v != NO_NODE)
    assert {v: int(c) for v, c in enumerate(direct) if c} == dict(want)
    return direct, clade, info


# ---- 1. pa_lineage_lca alone -----------------------------------------------------------------

LCA_G = 2200
LCA_SIZES = (0, 1, 2, 63, 64, 65, 300, 2100)   # both sides of the lane / wave threshold, of a wave, of a workgroup


@functools.lru_cache(maxsize=None)
def lca_genomes():
    rng = np.random.default_rng(17)
    return [TC.rand_dna(rng, 40) for _ in range(LCA_G)]


@pytest.fixture(scope="module")
def lca_index():
    index = N.Index(lca_genomes(), 21)
    yield index
    index.close()


def lca_tree(kind):
    """(parent, genome_node) over LCA_G genomes."""
    rng = np.random.default_rng(23)
    G = LCA_G
    if kind == "flat":
        return [0] * (G + 1), [g + 1 for g in range(G)]
    if kind == "chain":       # depth 300, genomes at every level (the root's included)
        return [max(i - 1, 0) for i in range(301)], [g % 301 for g in range(G)]
    if kind == "balanced":    # a complete binary tree of 4095 nodes, the genomes on its 2048 leaves
        n = 4095
        return [max((i - 1) // 2, 0) for i in range(n)], [n - 1 - (g % 2048) for g in range(G)]
    n = 1500                  # random: more genomes than nodes (shared nodes), most of them internal
    parent = [0] + [int(rng.integers(max(0, i - 40), i)) for i in range(1, n)]
    return parent, [int(x) for x in rng.integers(0, n, G)]


def lca_sets(parent, genome_node):
    """Sets of every size in LCA_SIZES: random members, and members from one stretch of the genomes
    ordered by node (a deeper answer); then the sets whose answers the issue names."""
    rng = np.random.default_rng(29)
    G = len(genome_node)
    by_node = sorted(range(G), key=lambda g: (L.root_path(parent, genome_node[g]), g))
    sets = []
    for size in LCA_SIZES:
        for rep in range(4):
            sets.append(tuple(sorted(int(x) for x in rng.choice(G, size, replace=False))))
            a = int(rng.integers(0, G - size + 1))
            sets.append(tuple(sorted(by_node[a:a + size])))
    kids = set(parent[1:])
    internal = [g for g in range(G) if genome_node[g] in kids and genome_node[g] != 0]
    leaves = collections.defaultdict(list)
    for g in range(G):
        if genome_node[g] not in kids:
            leaves[genome_node[g]].append(g)
    shared = [gs for gs in leaves.values() if len(gs) >= 2]
    if internal:
        sets.append((internal[0],))
        below = [g for g in range(G) if genome_node[g] != genome_node[internal[0]]
                 and genome_node[internal[0]] in L.root_path(parent, genome_node[g])]
        if below:
            sets.append(tuple(sorted((internal[0], below[0]))))   # a node and its own ancestor
    if shared:
        sets.append(tuple(sorted(shared[0][:2])))                  # genomes sharing a leaf
    sets.append(tuple(range(G)))                                   # every genome: the root
    return sets


@pytest.mark.parametrize("kind", ["flat", "chain", "balanced", "random"])
def test_lca_alone(kind, lca_index):
    parent, genome_node = lca_tree(kind)
    sets = lca_sets(parent, genome_node)
    want = [L.lca(parent, sorted({genome_node[g] for g in C})) if C else NO_NODE for C in sets]
    # what the batch must hold, on the model's side
    kids = set(parent[1:])
    assert 0 in want and NO_NODE in want
    assert any(v != NO_NODE and v not in kids for v in want)                      # a leaf
    if kind in ("chain", "random"):
        assert any(v in kids and v != 0 and v in set(genome_node) for v in want)  # an internal genome node
    assert {len(C) for C in sets} >= set(LCA_SIZES)
    off = np.zeros(len(sets) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(C) for C in sets])
    flat = np.array([g for C in sets for g in C], dtype=np.uint32)
    lin = N.Lineage(lca_index, parent, genome_node)
    got = lin.lca(off, flat)
    assert got.tolist() == want
    assert lin.lca(off, flat).tolist() == want              # twice: the same
    assert not lin.counts()[0].any()                        # the accumulator's counts are not touched
    assert lin.lca(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32)).size == 0
    assert lin.lca([0, 0, 0], []).tolist() == [NO_NODE, NO_NODE]
    with pytest.raises(ValueError):
        lin.lca([0, 2], [0, LCA_G])                         # a genome the index does not hold
    lin.close()


# ---- 2. hand-built ---------------------------------------------------------------------------

# root -> species A -> g0, g1; root -> species B -> g2
HAND_PARENT = [0, 0, 1, 1, 0, 4]
HAND_GENOME_NODE = [2, 3, 5]
ROOT, SP_A, SP_B = 0, 1, 4


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
@pytest.mark.parametrize("k", [31, 63, 127])
def test_hand_built(k, both):
    genomes, reads = A.hand_case(k)
    names, seqs, quals = [r[0] for r in reads], [r[1] for r in reads], [r[2] for r in reads]
    types, sets, _ = A.model_of(genomes, both, k, seqs, quals, A.HAND_PS)
    nodes = L.nodes_of(HAND_PARENT, HAND_GENOME_NODE, types, sets)
    got = dict(zip(names, nodes))
    for n in ("in3_a", "in3_b", "in3_c", "substitution", "in12", "p_demoted"):
        assert got[n] == ROOT, n             # all three genomes, or g1 and g2: across the species
    for n in ("in2_a", "in2_b", "with_n", "subset"):
        assert got[n] == SP_A, n             # g0 and g1: an unambiguous species-A read
    assert got["boundary0"] == HAND_GENOME_NODE[0] and got["boundary2"] == HAND_GENOME_NODE[2]
    assert got["private1"] == HAND_GENOME_NODE[1]
    assert got["short"] == NO_NODE and got["dropped"] == NO_NODE
    assert got["reverse"] == (ROOT if both else NO_NODE)
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, k, both_strands=both)
    lin = N.Lineage(index, HAND_PARENT, HAND_GENOME_NODE)
    read_node = lin.add(dev, A.params(A.HAND_PS))
    assert read_node.dtype == np.uint32 and read_node.tolist() == nodes
    check_counts(lin, HAND_PARENT, nodes, types)
    for x in (lin, dev, index):
        x.close()


# ---- 3. random strains -----------------------------------------------------------------------

# rand_strains: four ancestors, three strains each (genomes 3a, 3a + 1, 3a + 2): root -> ancestor -> strain
# for the last three ancestors; the first one's strains have no lineage and hang off the root, so the reads
# that are ambiguous among them land there (no read of this batch is ambiguous across ancestors)
RAND_PARENT = [0] + [0, 0, 0] + [0, 4, 4, 4] + [0, 8, 8, 8] + [0, 12, 12, 12]
RAND_GENOME_NODE = [1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15]


def test_random_batch_conditions():
    """What the batch must hold, on the model's side, before any device result is looked at."""
    types, sets, _ = A.rand_model(0)
    nodes = L.nodes_of(RAND_PARENT, RAND_GENOME_NODE, types, sets)
    leaves = set(RAND_GENOME_NODE)
    assert types.count(AMBIGUOUS) >= 0.2 * len(types)
    assert len({v for v in nodes if v != NO_NODE and v not in leaves}) >= 3
    assert nodes.count(0) >= 1
    assert all((v == NO_NODE) == (t not in (UNIQUE, AMBIGUOUS)) for v, t in zip(nodes, types))


@pytest.mark.parametrize("i", range(len(A.RAND_PS)),
                         ids=[",".join(f"{a}={b}" for a, b in ps.items()) for ps in A.RAND_PS])
def test_random_strains(i):
    types, sets, _ = A.rand_model(i)
    nodes = L.nodes_of(RAND_PARENT, RAND_GENOME_NODE, types, sets)
    seqs, quals = A.rand_reads()
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(A.rand_strains(), A.RAND_K)
    prm = A.params(A.RAND_PS[i])
    lin = N.Lineage(index, RAND_PARENT, RAND_GENOME_NODE)
    read_node = lin.add(dev, prm)
    assert read_node.tolist() == nodes
    direct, clade, info = check_counts(lin, RAND_PARENT, nodes, types)
    # section 14's classes of the same reads (the unique reads are in their {g}), rolled up by the model's LCA
    ab = N.Abundance(index)
    ab.add(dev, prm)
    rolled = [0] * len(RAND_PARENT)
    for C, n in A.classes_list(ab):
        rolled[L.lca(RAND_PARENT, [RAND_GENOME_NODE[g] for g in C])] += n
    assert rolled == direct.tolist()
    for x in (ab, lin, dev, index):
        x.close()


# ---- 4. large sets, both sides of PA_LINEAGE_LDS_NODES ----------------------------------------

def large_tree(G, above):
    """Groups of 16 genomes under the root.  Below the constant: the genomes share
    N.LINEAGE_LDS_NODES // 4 nodes at most; above it: a chain of unused nodes
    takes the tree past the constant."""
    groups = (G + 15) // 16
    parent = [0] + [0] * groups
    slots = max(1, min(G, N.LINEAGE_LDS_NODES // 4 - groups - 1))
    first = len(parent)
    for s in range(slots):
        parent.append(1 + (s // 16) % groups)
    genome_node = [first + g % slots for g in range(G)]
    if above:
        while len(parent) <= N.LINEAGE_LDS_NODES + 7:
            parent.append(len(parent) - 1 if len(parent) > first + slots else 0)
    assert (len(parent) > N.LINEAGE_LDS_NODES) == above
    return parent, genome_node


@pytest.mark.parametrize("above", [False, True], ids=["lds_histogram", "global_atomics"])
@pytest.mark.parametrize("G, length, stretch, k, n_reads", [(300, 500, 200, 31, 90), (2100, 70, 40, 21, 60)],
                         ids=["300_genomes", "2100_genomes"])
def test_large_sets(G, length, stretch, k, n_reads, above):
    genomes, seqs, quals = A.large_case(G, length, stretch, k, n_reads)
    ps = dict(m=1, p=1)
    types, sets, _ = A.model_of(genomes, False, k, seqs, quals, ps)
    parent, genome_node = large_tree(G, above)
    nodes = L.nodes_of(parent, genome_node, types, sets)
    inside = [v for v, C in zip(nodes, sets) if len(C) == G]
    assert len(inside) >= n_reads // 3 and set(inside) == {0}   # the shared stretch: all on one node, the root
    assert len({v for v in nodes if v not in (0, NO_NODE)}) >= 5
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, k)
    lin = N.Lineage(index, parent, genome_node)
    assert lin.add(dev, A.params(ps)).tolist() == nodes
    check_counts(lin, parent, nodes, types)
    for x in (lin, dev, index):
        x.close()


# ---- 5. protocol -----------------------------------------------------------------------------

def test_batches_reset_and_determinism(monkeypatch):
    seqs, quals = A.rand_reads()
    seqs, quals = list(seqs[:1800]), list(quals[:1800])
    prm = A.params(A.RAND_PS[0])
    index = N.Index(A.rand_strains(), A.RAND_K)
    whole, _ = TC.upload(seqs, quals)
    cuts = ((0, 500), (500, 1300), (1300, 1800))
    parts = [TC.upload(seqs[a:b], quals[a:b])[0] for a, b in cuts]
    one, three = (N.Lineage(index, RAND_PARENT, RAND_GENOME_NODE) for _ in range(2))
    ref = one.add(whole, prm)
    got = np.concatenate([three.add(p, prm) for p in parts])
    assert np.array_equal(ref, got) and len(set(ref.tolist())) >= 8

    def state(lin):
        d, c, info = lin.counts()
        return d.tobytes(), c.tobytes(), info
    assert state(one) == state(three)                       # the same reads in three batches: the same counts
    base = state(one)
    # read_node == NULL: counted all the same
    three.reset()
    d, c, info = three.counts()
    assert not d.any() and not c.any() and not any(info[n] for n in info if n != "n_nodes")
    assert three.add(whole, prm, nodes=False) is None and state(three) == base
    # a second run: equal arrays
    three.reset()
    assert np.array_equal(three.add(whole, prm), ref) and state(three) == base
    # the LDS histogram and the global atomics count the same
    monkeypatch.setenv("PA_LINEAGE_LDS", "0")
    three.reset()
    assert np.array_equal(three.add(whole, prm), ref) and state(three) == base
    monkeypatch.delenv("PA_LINEAGE_LDS")
    # every read through the exact kernel
    monkeypatch.setenv("PA_ASSIGN", "0")
    three.reset()
    assert np.array_equal(three.add(whole, prm), ref) and state(three) == base
    monkeypatch.delenv("PA_ASSIGN")
    # an all-dropped batch
    drop = N.Params.make(1, 1, 200, None, None)
    three.reset()
    nodes = three.add(parts[0], drop)
    d, c, info = three.counts()
    assert (nodes == NO_NODE).all() and not d.any() and info["reads_dropped"] == 500 and info["reads_unique"] == 0
    for x in [one, three, whole, index] + parts:
        x.close()


def test_errors():
    genomes = A.rand_strains()
    seqs, quals = A.rand_reads()
    dev, _ = TC.upload(list(seqs[:300]), list(quals[:300]))
    prm = A.params(A.RAND_PS[0])
    index, other = N.Index(genomes, A.RAND_K), N.Index(genomes, A.RAND_K)
    lib, G = N.lib(), len(genomes)
    b0 = int(index.info().device_bytes)

    def create(parent, genome_node, n_nodes=None):
        par = np.array(parent, dtype=np.uint32)
        gn = np.array(genome_node, dtype=np.uint32)
        h = N.P()
        st = lib.pa_lineage_create(index.handle, N._ptr(par), len(parent) if n_nodes is None else n_nodes, N._ptr(gn),
                                   N.ctypes.byref(h))
        assert (st == N.PA_OK) == bool(h.value)
        if h.value:
            lib.pa_lineage_free(h)
        return st
    assert create([0, 0], [1] * G) == N.PA_OK
    assert create([0], [0] * G, n_nodes=0) == N.PA_EINVAL            # n_nodes == 0
    assert create([1, 0], [0] * G) == N.PA_EINVAL                    # parent[0] != 0
    assert create([0, 1], [0] * G) == N.PA_EINVAL                    # parent[i] >= i
    assert create([0, 0, 3, 0], [0] * G) == N.PA_EINVAL
    assert create([0, 0], [0] * (G - 1) + [2]) == N.PA_EINVAL        # genome_node[g] >= n_nodes
    assert create([0], [0] * G, n_nodes=0xFFFFFFFF) == N.PA_EUNSUPPORTED
    for bad in ([1, 0], [0, 1]):
        with pytest.raises(ValueError):
            N.Lineage(index, bad, [0] * G)
    with pytest.raises(ValueError):
        N.Lineage(index, [0, 0], [0] * (G + 1))                      # not one node per genome
    # NULL arguments
    h = N.P()
    par, gn = np.zeros(1, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
    assert lib.pa_lineage_create(None, N._ptr(par), 1, N._ptr(gn), N.ctypes.byref(h)) == N.PA_EINVAL
    assert lib.pa_last_error() == b"NULL argument"
    assert lib.pa_lineage_create(index.handle, N._ptr(par), 1, N._ptr(gn), None) == N.PA_EINVAL
    assert lib.pa_lineage_create(index.handle, None, 1, N._ptr(gn), N.ctypes.byref(h)) == N.PA_EINVAL
    assert lib.pa_lineage_create(index.handle, N._ptr(par), 1, None, N.ctypes.byref(h)) == N.PA_EINVAL
    assert not h.value
    lin = N.Lineage(index, RAND_PARENT, RAND_GENOME_NODE)
    assert int(index.info().device_bytes) == b0                      # the accumulator's bytes are not the index's
    assert lib.pa_lineage_reset(None, None) == N.PA_EINVAL
    assert lib.pa_lineage_counts(None, None, None, None, None) == N.PA_EINVAL
    assert lib.pa_lineage_counts(lin.handle, None, None, None, None) == N.PA_OK   # (every output may be NULL)
    assert lib.pa_lineage_lca(None, None, None, 0, None, None) == N.PA_EINVAL
    assert lib.pa_lineage_lca(lin.handle, None, None, 0, None, None) == N.PA_OK
    assert lib.pa_lineage_lca(lin.handle, None, None, 1, None, None) == N.PA_EINVAL
    assert lib.pa_lineage_add(None, dev.handle, prm, lin.handle, None, None) == N.PA_EINVAL
    assert lib.pa_lineage_add(index.handle, None, prm, lin.handle, None, None) == N.PA_EINVAL
    assert lib.pa_lineage_add(index.handle, dev.handle, None, lin.handle, None, None) == N.PA_EINVAL
    assert lib.pa_lineage_add(index.handle, dev.handle, prm, None, None, None) == N.PA_EINVAL
    lib.pa_lineage_free(None)
    off = np.array([0, 2, 1], dtype=np.uint64)                        # descending offsets
    out = np.zeros(2, dtype=np.uint32)
    assert lib.pa_lineage_lca(lin.handle, N._ptr(off), N._ptr(np.zeros(2, dtype=np.uint32)), 2, N._ptr(out),
                              None) == N.PA_EINVAL
    # another index; its own index after a reduce
    ref = lin.add(dev, prm)
    held = [a.tolist() for a in lin.counts()[:2]]
    assert lib.pa_lineage_add(other.handle, dev.handle, prm, lin.handle, None, None) == N.PA_EINVAL
    index.reduce([0, 2, 3, 5])
    with pytest.raises(ValueError):
        lin.add(dev, prm)
    assert [a.tolist() for a in lin.counts()[:2]] == held             # (what it holds stays readable)
    assert len(ref) == 300
    for x in (lin, dev, index, other):
        x.close()


def test_alloc_failures_leave_the_index_usable():
    """PA_ENOMEM from every device allocation of pa_lineage_create and pa_lineage_add (libpa's test
    hook, as tests/test_gpu_alloc_paths.py): nothing leaks, and the index and the accumulator go on working."""
    seqs, quals = A.rand_reads()
    dev, _ = TC.upload(list(seqs[:600]), list(quals[:600]))
    prm = A.params(A.RAND_PS[0])
    index = N.Index(A.rand_strains(), A.RAND_K)
    first = N.Lineage(index, RAND_PARENT, RAND_GENOME_NODE)
    ref = first.add(dev, prm)                      # (also makes the index's align-side view and scratch)
    want = [a.tolist() for a in first.counts()[:2]]
    first.close()
    live0, c0 = N.test_alloc_live(), N.test_alloc_calls()
    N.Lineage(index, RAND_PARENT, RAND_GENOME_NODE).close()
    K = N.test_alloc_calls() - c0
    assert K >= 4 and N.test_alloc_live() == live0
    for i in range(1, K + 1):
        N.test_alloc_fail_at(i)
        try:
            with pytest.raises(MemoryError):
                N.Lineage(index, RAND_PARENT, RAND_GENOME_NODE)
        finally:
            N.test_alloc_fail_at(0)
        assert N.test_alloc_live() == live0, f"allocation {i} of pa_lineage_create leaked"
    lin = N.Lineage(index, RAND_PARENT, RAND_GENOME_NODE)
    live1, c0 = N.test_alloc_live(), N.test_alloc_calls()
    assert np.array_equal(lin.add(dev, prm), ref)
    K = N.test_alloc_calls() - c0
    assert K >= 4 and N.test_alloc_live() == live1
    nomem = 0
    for i in range(1, K + 1):
        lin.reset()                                 # (after an error the accumulator may hold a part of the batch)
        N.test_alloc_fail_at(i)
        try:
            got = lin.add(dev, prm)
            assert np.array_equal(got, ref), f"a tolerated failure of allocation {i} changed the result"
        except MemoryError:
            nomem += 1
        finally:
            N.test_alloc_fail_at(0)
        assert N.test_alloc_live() == live1, f"allocation {i} of pa_lineage_add leaked"
    assert nomem >= 1
    lin.reset()
    assert np.array_equal(lin.add(dev, prm), ref) and [a.tolist() for a in lin.counts()[:2]] == want
    for x in (lin, dev, index):
        x.close()


# ---- 6. drop-in API and CLI ------------------------------------------------------------------

CLI_CASES, FA, FQ = TC.CLI_CASES, TC.FA, TC.FQ


@functools.lru_cache(maxsize=None)
def config1_lineages():
    """{identifier: lineage}: the first two genomes one species of one family, the third a family of its own."""
    ids = [n for n, _ in TC.config1()[0]]
    assert len(ids) == 3
    return {ids[0]: ["FamA", "SpX"], ids[1]: ["FamA", "SpX"], ids[2]: ["FamB"], "not in the index": ["FamC", "SpZ"]}


def write_lineages(path):
    with open(path, "w") as fh:
        fh.write("# genome\tlineage\n\n")
        for ident, names in config1_lineages().items():
            fh.write(f"{ident}\t{';'.join(names)}\n")
    return str(path)


@functools.lru_cache(maxsize=None)
def config1_model(both=False):
    gen, reads = TC.config1()
    ids, gs = [n for n, _ in gen], [g for _, g in gen]
    seqs, quals = [s for s, _ in reads], [q for _, q in reads]
    types, sets, _ = A.model_of(gs, both, 21, seqs, quals, dict(m=1, p=1))
    parent, names, genome_node = L.model_tree(ids, config1_lineages())
    return types, sets, parent, names, genome_node, L.nodes_of(parent, genome_node, types, sets)


def fastq_ids():
    from data_file import FASTAQFile
    return [r.identifier for r in FASTAQFile(FQ).container]


def test_cli_lineage_report(tmp_path):
    lf = write_lineages(tmp_path / "lin.tsv")
    rep, a = str(tmp_path / "rep.tsv"), str(tmp_path / "as.tsv")
    r = TC.run_cli(["--lineages", lf, "--lineage-report", rep, "--assignments", a])
    assert r.returncode == 0, r.stderr
    assert r.stdout == CLI_CASES[0]["stdout"]      # stdout: what is pinned without the flags
    types, sets, parent, names, genome_node, nodes = config1_model()
    want = L.report_text(parent, names, genome_node, nodes, types.count(M.UNMAPPED), types.count(M.DROPPED))
    assert open(rep).read() == want
    assert len({v for v in nodes if v != NO_NODE}) >= 3
    # the assignments file's fourth column: the path of the read's node
    lines = open(a).read().split("\n")
    assert lines[0] == "#read\tmapping\tgenomes\ttaxon" and lines[-1] == ""
    got = [ln.split("\t") for ln in lines[1:-1]]
    assert all(len(g) == 4 for g in got) and [g[0] for g in got] == fastq_ids()
    paths = ["root" if v == 0 else ";".join(names[x] for x in L.root_path(parent, v)[1:]) for v in range(len(parent))]
    assert [g[3] for g in got] == ["" if v == NO_NODE else paths[v] for v in nodes]
    words = {M.DROPPED: "filtered", M.UNMAPPED: "unmapped", UNIQUE: "unique", AMBIGUOUS: "ambiguous"}
    assert [g[1] for g in got] == [words[t] for t in types]
    # --lineages with --assignments alone
    r = TC.run_cli(["--lineages", lf, "--assignments", str(tmp_path / "as2.tsv")])
    assert r.returncode == 0 and open(str(tmp_path / "as2.tsv")).read() == open(a).read()


def test_api_lineage_report_with_bootstraps():
    from data_file import FASTAFile
    from kmer import ABUNDANCE_BOOTSTRAP_COLUMNS, KmerReference, PseudoAlignment, bootstrap_summary
    from lineage import Lineages
    types, sets, parent, names, genome_node, nodes = config1_model()
    ref = KmerReference(21, FASTAFile(FA).container)
    plain = PseudoAlignment(ref)
    for fn in (plain.get_lineage_report, lambda: plain.write_lineage_report(io.StringIO())):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(ValueError):
        PseudoAlignment(ref, lineages={"x": ["A"]})
    pa = PseudoAlignment(ref, abundance=True, lineages=Lineages(config1_lineages()))
    pa.align_reads_from_file(FQ)
    assert pa._batches[0].read_node.dtype == np.uint32 and pa._batches[0].read_node.tolist() == nodes
    rep = pa.get_lineage_report(50, 0.0, 20, 7, 0.9)
    a = pa.get_abundance(50, 0.0, 20, 7, 0.9)
    tree = pa._lineage_tree()
    assert (tree.parent, tree.names, tree.genome_node) == (parent, names, genome_node)
    assert [r["node"] for r in rep["rows"]] == L.preorder(parent)
    matrix = pa._abundance().bootstrap(20, 7, 50, 0.0)[1]
    below = {v: [g for g, gv in enumerate(genome_node) if v in L.root_path(parent, gv)] for v in range(len(parent))}

    def total(values, v):   # ascending genome index, in double
        s = 0.0
        for g in below[v]:
            s += float(values[g])
        return s
    rolled = [[total(rep_b, v) for v in range(len(parent))] for rep_b in matrix]
    summary = bootstrap_summary(rolled, 0.9)
    for r in rep["rows"]:
        v = r["node"]
        assert r["read_fraction"] == total([g["read_fraction"] for g in a["genomes"]], v)
        assert r["abundance"] == total([g["abundance"] for g in a["genomes"]], v)
        assert tuple(r[c] for c in ABUNDANCE_BOOTSTRAP_COLUMNS) == summary[v]
    root = rep["rows"][0]
    assert abs(root["read_fraction"] - 1) <= 1e-12 and abs(root["abundance"] - 1) <= 1e-12
    assert (rep["iterations"], rep["bootstraps"], rep["seed"], rep["confidence"]) == (50, 20, 7, 0.9)
    assert rep["reads"] == len(types) and rep["classified"] == types.count(UNIQUE) + types.count(AMBIGUOUS)
    buf = io.StringIO()
    pa.write_lineage_report(buf, 50, 0.0, 20, 7, 0.9)
    text = buf.getvalue().splitlines()
    assert text[0].split("\t")[6:] == ["read_fraction", "abundance"] + list(ABUNDANCE_BOOTSTRAP_COLUMNS)
    assert text[-1].endswith("\titerations\t50\tlast_delta\t" + format(a["last_delta"], ".9g")
                             + f"\tclasses\t{a['classes']}\tbootstraps\t20\tseed\t7\tconfidence\t0.9")
    assert not any("ineage" in key for key in pa.__getstate__())   # (never part of an .aln file)
    # pairs: refused, as with abundance
    with pytest.raises(ValueError):
        PseudoAlignment(ref, lineages=Lineages(config1_lineages())).align_pairs_from_containers([], [])


def test_cli_lineage_report_with_abundance(tmp_path):
    lf = write_lineages(tmp_path / "lin.tsv")
    rep, f = str(tmp_path / "rep.tsv"), str(tmp_path / "a.tsv")
    flags = ["--abundance", f, "--abundance-bootstraps", "20", "--abundance-seed", "7", "--abundance-confidence", "0.9"]
    r = TC.run_cli(flags + ["--lineages", lf, "--lineage-report", rep])
    assert r.returncode == 0, r.stderr
    assert r.stdout == CLI_CASES[0]["stdout"]
    types, sets, parent, names, genome_node, nodes = config1_model()
    plain = L.report_text(parent, names, genome_node, nodes, types.count(M.UNMAPPED), types.count(M.DROPPED))
    got = [ln.split("\t") for ln in open(rep).read().splitlines()]
    ab = [ln.split("\t") for ln in open(f).read().splitlines()]
    assert got[0][6:] == ab[0][5:] == ["read_fraction", "abundance", "abundance_mean", "abundance_sd", "abundance_lo",
                                       "abundance_hi"]
    assert ["\t".join(g[:6]) for g in got[:-1]] == plain.splitlines()[:-1]      # the first six columns: the plain report
    assert "\t".join(got[-1][:10]) == plain.splitlines()[-1]
    assert got[-1][10:] == ["iterations"] + ab[-1][1:]                           # the settings, as the abundance file's
    genome_rows = ab[1:-1]
    order = L.preorder(parent)
    assert len(got) == len(order) + 2
    for row, v in zip(got[1:-1], order):
        below = [g for g, gv in enumerate(genome_node) if v in L.root_path(parent, gv)]
        tol = (len(below) + 1) * 1e-9
        for col in range(3):          # read_fraction, abundance and abundance_mean are sums over the subtree
            want = sum(float(genome_rows[g][5 + col]) for g in below)
            assert abs(float(row[6 + col]) - want) <= tol, (row, col)
        if len(below) == 1:           # a genome's own node: its line of the abundance file, digit for digit
            assert row[6:] == genome_rows[below[0]][5:]
        assert float(row[10]) <= float(row[11])   # lo <= hi (sd, lo and hi of the inner nodes: the API test above)


def test_cli_lineage_filter_similar(tmp_path):
    """After --filter-similar the tree is built over the kept genomes; one lineage file serves both runs."""
    from data_file import FASTAFile
    from kmer import KmerReference
    lf = write_lineages(tmp_path / "lin.tsv")
    rep = str(tmp_path / "rep.tsv")
    flags = ["--filter-similar", "--similarity-threshold", "0.5"]
    r, plain = TC.run_cli(flags + ["--lineages", lf, "--lineage-report", rep]), TC.run_cli(flags)
    assert r.returncode == 0 and plain.returncode == 0, r.stderr + plain.stderr
    assert r.stdout == plain.stdout
    ref = KmerReference(21, FASTAFile(FA).container, filter_similar=True, similarity_threshold=0.5)
    kept = [g.identifier for g in ref.genomes]
    parent, names, genome_node = L.model_tree(kept, config1_lineages())
    lines = open(rep).read().splitlines()
    assert [ln.split("\t")[0].split(";")[-1] for ln in lines[1:-1]] == [names[v] for v in L.preorder(parent)]
    assert lines[1].split("\t")[:3] == ["root", "0", str(len(kept))] and 1 <= len(kept) <= 3
    assert lines[-1].split("\t")[-2:] == ["nodes", str(len(parent))]
    # a genome of the index without a line
    short = tmp_path / "short.tsv"
    short.write_text("nobody\tA;B\n")
    bad = TC.run_cli(["--lineages", str(short), "--lineage-report", rep])
    err = bad.stderr.strip()
    assert bad.returncode != 0 and bad.stdout == "" and err.startswith("Error: no lineage for genome") \
        and len(err.splitlines()) == 1


def test_cli_files_without_lineages_are_unchanged(tmp_path):
    """--abundance and --assignments without --lineages: the files of the format as it was."""
    f, a = str(tmp_path / "a.tsv"), str(tmp_path / "as.tsv")
    r = TC.run_cli(["--abundance", f, "--assignments", a])
    assert r.returncode == 0, r.stderr
    assert r.stdout == CLI_CASES[0]["stdout"]
    assert open(f).read() == A.config1_text()
    gen, reads = TC.config1()
    ids = [n for n, _ in gen]
    seq, off = TC.O.concat([s for s, _ in reads])
    qual, _ = TC.O.concat([q for _, q in reads])
    o = TC.oracle_lists([g for _, g in gen], False, 21, (seq, qual, off), dict(m=1, p=1))
    words = {M.DROPPED: "filtered", M.UNMAPPED: "unmapped", UNIQUE: "unique", AMBIGUOUS: "ambiguous"}
    want = "#read\tmapping\tgenomes\n" + "".join(
        f"{rid}\t{words[int(t)]}\t{','.join(ids[int(g)] for g in o.genomes_of(i)) if int(t) >= 2 else ''}\n"
        for i, (rid, t) in enumerate(zip(fastq_ids(), o.types)))
    assert open(a).read() == want
