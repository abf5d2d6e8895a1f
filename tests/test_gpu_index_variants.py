"""Layouts x consumers: everything built on the per-read
pass -- align_reads, candidates / classes / EM, coverage and placements, pileup,
pairs, lineage, positions / lookup, dumpref / EXTSIM statistics -- on every way
the index can be laid out, and the pair-exact kernel past the membership masks.

The worlds, models and check functions are the existing modules' (imported, not
restated): the models know nothing of the layout, so one model per (consumer,
strands, k, parameter set) serves every variant, and a cell costs an index build
and the passes.  Every comparison is exact equality.

Variants (VARIANTS below): the build flags (compact, defer_tiles), the order of
prepare() and the passes, the switches csrc/pa_index.hip reads at build or
prepare time, and an index reduced from a larger one.  A cell sets its variant's
environment before the build and keeps it until its last pass has run.  Every
variant is built once per world -- except compact_job, deferred and
prepared_late, whose state the first pass consumes: those are built per cell.

Witnesses (witness() below; test_witnesses_reject_a_build_without_the_switch
shows each one fails on a default build): table_slots for default, compact and
large; device_bytes against the default, no_nb and compact builds of the same
genomes for compact_job, deferred, prepared_late, no_nb, nb_half, no_tile and
no_bloom (no_tile also by k_align_lane not running); n_genomes / n_kmers
against a build of the kept genomes for reduced.

Unwitnessed -- no API tells them from the build they are compared with, they
stay in the matrix all the same:
  * nb_split (the neighbour words in two allocations: the same bytes);
  * tpos_local (genome-local first occurrences: the same bytes and slots);
  * large_hi1 against large_hi0 (both are witnessed as `large`; PA_TPOS_HI only
    chooses the first occurrences' form);
  * reduced_inplace against reduced_gather (both are witnessed as reduced;
    PA_REDUCE_INPLACE only chooses how the kept codes are moved);
  * no_nb at k = 97: four key words have no tiles, so there is nothing to leave out.

Refusal by design, asserted as such: pa_index_dumpref on a both-strand index
(PaUnsupported, include/pa.h: the dump is of the forward k-mer database).
"""

import contextlib
import functools
import json
import os
import tempfile

import numpy as np
import pytest

import pa_native as N
import pa_oracle as O
import test_abundance_host as AM
import test_gpu_abundance as A
import test_gpu_coverage as TC
import test_gpu_lineage as LG
import test_gpu_pairs as GP
import test_gpu_pileup as P
import test_lineage_host as L
import test_pairs_host as PM

pytestmark = pytest.mark.gpu

ENV_KEYS = ("PA_NO_NB", "PA_NB_SPLIT", "PA_NB_HALF", "PA_LAYOUT", "PA_TPOS_HI", "PA_TPOS_LOCAL", "PA_NO_TILE",
            "PA_BLOOM_MB", "PA_REDUCE_INPLACE")
VARIANTS = {
    "default": {},
    "compact": {},                # compact=True
    "compact_job": {},            # compact=True, defer_tiles=True, prepare(expected_reads=n): tiles, no neighbour bits
    "deferred": {},               # defer_tiles=True, nothing prepared
    "prepared_late": {},          # defer_tiles=True, prepare(expected_reads=1), half the batch, prepare(), the rest
    "no_nb": {"PA_NO_NB": "1"},
    "nb_split": {"PA_NB_SPLIT": "1"},
    "nb_half": {"PA_NB_SPLIT": "1", "PA_NB_HALF": "1"},
    "large_hi1": {"PA_LAYOUT": "large", "PA_TPOS_HI": "1"},
    "large_hi0": {"PA_LAYOUT": "large", "PA_TPOS_HI": "0"},
    "tpos_local": {"PA_TPOS_LOCAL": "1"},
    "no_tile": {"PA_NO_TILE": "1"},
    "no_bloom": {"PA_BLOOM_MB": "0"},
    "reduced_gather": {},         # built with decoys interleaved, then reduce(keep)
    "reduced_inplace": {"PA_REDUCE_INPLACE": "1"},
}
STATEFUL = ("compact_job", "deferred", "prepared_late")  # the first pass changes them: built per cell
BOTH_TOO = ("default", "compact_job", "large_hi1", "reduced_inplace")
WIDE = ("no_nb", "large_hi1", "reduced_gather")  # (the compact table is single-word only)
UNWITNESSED = ("nb_split", "tpos_local")
EXPECTED_READS = {"cov": 3000, "abd": 4000, "pair": 4000}  # far below the neighbour bits' break-even (2.5 per base)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


@contextlib.contextmanager
def set_env(values, clear=()):
    saved = {name: os.environ.get(name) for name in tuple(clear) + tuple(values)}
    try:
        for name in clear:
            os.environ.pop(name, None)
        for name, v in values.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
        yield
    finally:
        for name, v in saved.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v


def variant_env(variant):
    return set_env(VARIANTS[variant], clear=ENV_KEYS)


# ---- 1. the variants ---------------------------------------------------------------------------

def roundup4(x):
    return (x + 3) // 4 * 4


def snapshot(index, **stages):
    i = index.info()
    s = dict(slots=int(i.table_slots), bytes=int(i.device_bytes), windows=int(i.total_windows),
             n_genomes=int(i.n_genomes), n_kmers=int(i.n_kmers))
    s.update(bytes_built=s["bytes"], genomes_built=s["n_genomes"])  # (before prepare / before reduce)
    s.update(stages)
    return s


def with_decoys(genomes):
    """(genomes with a 1 % mutated copy after every second one, the originals' numbers)."""
    rng = np.random.default_rng(len(genomes))
    out, keep = [], []
    for i, g in enumerate(genomes):
        keep.append(len(out))
        out.append(g)
        if i % 2 == 0 and i + 1 < len(genomes):
            out.append(TC.mutate(rng, g, 0.01))
    runs = 1 + sum(b != a + 1 for a, b in zip(keep, keep[1:]))
    assert runs >= 3 and len(out) > len(genomes), (runs, keep)
    return out, keep


def make(variant, genomes, k, both, expected_reads):
    """(index, snapshot) of one variant, under the environment the caller has set."""
    kw = dict(both_strands=both, compact=variant in ("compact", "compact_job"), defer_tiles=variant in STATEFUL)
    if variant.startswith("reduced"):
        full, keep = with_decoys(genomes)
        index = N.Index(full, k, **kw)
        built = snapshot(index)
        index.reduce(keep)
        return index, snapshot(index, genomes_built=built["n_genomes"])
    index = N.Index(list(genomes), k, **kw)
    snap = snapshot(index)
    if variant == "compact_job":
        index.prepare(expected_reads=expected_reads)
        snap = snapshot(index, bytes_built=snap["bytes"])
    if variant == "prepared_late":
        index.prepare(expected_reads=1)
        snap = snapshot(index, bytes_built=snap["bytes"])
    return index, snap


def witness(variant, s, ref, tiled=True):
    """The variant is what its name says: its snapshot against the snapshots ref(name) of other builds of
    the same genomes.  tiled: k <= 95 (wider keys have no align-side view to leave out)."""
    if variant in UNWITNESSED:
        return
    if variant == "default":
        assert s["slots"] == roundup4(4 * s["windows"] + 64), s
        return
    d = ref("default")
    if variant in ("compact", "compact_job"):
        assert s["slots"] == roundup4(2 * s["windows"] + 64), (s, d)
        if variant == "compact_job":  # prepare made the tiles, and not the neighbour bits a compact build holds
            assert s["bytes_built"] < s["bytes"] < ref("compact")["bytes"], (s, ref("compact"))
    elif variant in ("deferred", "no_tile"):  # less than an index that lacks only the neighbour bits
        assert s["slots"] == d["slots"] and s["bytes"] < ref("no_nb")["bytes"], (s, ref("no_nb"))
    elif variant == "prepared_late":  # prepare(expected_reads=1) made tiles, not all a default build holds
        assert s["slots"] == d["slots"] and s["bytes_built"] < s["bytes"] < d["bytes"], (s, d)
    elif variant == "no_nb":
        assert s["slots"] == d["slots"], (s, d)
        assert s["bytes"] < d["bytes"] if tiled else s["bytes"] == d["bytes"], (s, d)
    elif variant == "nb_half":  # 12 B per base where the default holds 24
        assert 0 < d["bytes"] - s["bytes"] and 2 * (d["bytes"] - s["bytes"]) == d["bytes"] - ref("no_nb")["bytes"], \
            (s, d, ref("no_nb"))
    elif variant in ("large_hi1", "large_hi0"):
        assert 2 * s["slots"] < d["slots"], (s, d)
    elif variant == "no_bloom":
        assert s["slots"] == d["slots"] and s["bytes"] < d["bytes"], (s, d)
    elif variant.startswith("reduced"):  # (the default build is the build of the kept genomes)
        assert s["genomes_built"] > s["n_genomes"] == d["n_genomes"] and s["n_kmers"] == d["n_kmers"], (s, d)
    else:
        raise KeyError(variant)


class Factory:
    """The module's indices, device batches and default-variant results."""

    def __init__(self):
        self.indices, self.snaps, self.devs, self.memo = {}, {}, {}, {}

    def build(self, variant, genomes, k, both, expected_reads=0):
        """The N.Index of `variant` over `genomes` (call inside variant_env(variant)); cached unless stateful."""
        genomes = tuple(genomes)
        key = (variant, genomes, k, both)
        if variant not in STATEFUL and key in self.indices:
            return self.indices[key]
        assert all(os.environ.get(e) == VARIANTS[variant].get(e) for e in ENV_KEYS), "not inside variant_env"
        index, snap = make(variant, genomes, k, both, expected_reads)
        self.snaps[key] = snap
        if variant not in STATEFUL:
            self.indices[key] = index
        try:
            witness(variant, snap, lambda name: self.snap(name, genomes, k, both), tiled=k <= 95)
        except AssertionError as e:
            raise AssertionError(f"variant {variant} (k={k}, both={both}) is not what its name says: {e}") from e
        return index

    def snap(self, name, genomes, k, both):
        key = (name, tuple(genomes), k, both)
        if key not in self.snaps:
            with variant_env(name):
                index = self.build(name, genomes, k, both)
                if name in STATEFUL:
                    index.close()
        return self.snaps[key]

    def reads(self, key, seqs, quals):
        if key not in self.devs:
            self.devs[key] = (TC.upload(list(seqs), list(quals))[0],)
        return self.devs[key][0]

    def pairs(self, key, pairs):
        if key not in self.devs:
            self.devs[key] = tuple(GP.upload(list(pairs)))
        return self.devs[key]

    def close(self):
        for x in list(self.indices.values()) + [d for ds in self.devs.values() for d in ds]:
            x.close()


@pytest.fixture(scope="module")
def factory():
    f = Factory()
    yield f
    f.close()


# ---- 2. the worlds and models ------------------------------------------------------------------

def world_genomes(world, k):
    if world == "cov":       # 6 x 3-5 kb (pileup's reference genomes are the same texts)
        return TC.rand_genomes(TC.pair_len(k))[0]
    if world == "abd":       # 12 x 2 kb
        return A.rand_strains()
    return PM.rand_genomes()  # 4 x 3.8 kb


@functools.lru_cache(maxsize=None)
def cov_model(k, both, psi):
    return TC.rand_model(k, both, TC.RAND_PS[psi])


@functools.lru_cache(maxsize=None)
def pile_model(both, psi):
    return P.rand_model(31, both, P.RAND_PS[psi])


@functools.lru_cache(maxsize=None)
def abd_kd(k, both):
    return AM.kmer_sets(A.rand_strains(), both, k)


@functools.lru_cache(maxsize=None)
def abd_model(k, both, psi):
    if k == A.RAND_K and not both:
        return A.rand_model(psi)
    seqs, quals = A.rand_reads()
    return A.model_of(A.rand_strains(), both, k, seqs, quals, A.RAND_PS[psi], abd_kd(k, both))


@functools.lru_cache(maxsize=None)
def lineage_tree():
    return LG.lca_tree("random")


@functools.lru_cache(maxsize=None)
def abd_nodes(k, both, psi, G):
    parent, node = lineage_tree()
    types, sets, _ = abd_model(k, both, psi)
    return L.nodes_of(parent, node[:G], types, sets)


def pair_list(k):
    return PM.rand_pairs(k if k in PM.RAND_SHAPES else 63)  # (k = 97: the 150-base mates of k = 63)


@functools.lru_cache(maxsize=None)
def pair_model(k, both, psi):
    if k in PM.RAND_SHAPES:
        return PM.rand_model(k, both, psi)[0]
    genomes, pairs, ps = PM.rand_genomes(), pair_list(k), PM.RAND_PS[psi]
    res = PM.model_all(PM.kmer_sets(genomes, both, k), k, pairs, **ps)
    PM.oracle_check(genomes, both, k, pairs, res, ps)
    return res


@functools.lru_cache(maxsize=None)
def cov_kmer_dict(k):
    return O.kmer_dict(world_genomes("cov", k), k)


@functools.lru_cache(maxsize=None)
def cov_kmer_sets(k, both):
    return PM.kmer_sets(world_genomes("cov", k), both, k)


@functools.lru_cache(maxsize=None)
def pos_queries(k):
    """k-mers of the genomes, reverse complements of some, random ones, and two that can be no key."""
    rng = np.random.default_rng(k)
    keys = list(cov_kmer_dict(k))
    pick = [keys[int(i)] for i in rng.integers(0, len(keys), 300)]
    queries = pick + [O.reverse_complement(q) for q in pick[:100]]
    queries += ["".join(rng.choice(list("ACGT"), k)) for _ in range(50)]
    return queries + ["N" * k, ("ACGT" * k)[:k]]


# ---- 3. the consumers --------------------------------------------------------------------------

def rows(per_read, off=None, flats=()):
    """One tuple per read: the per-read columns, then read r's slice of every flat list."""
    cols = [np.asarray(c).tolist() for c in per_read]
    if off is not None:
        off = [int(x) for x in off]
        for f in flats:
            f = np.asarray(f).tolist()
            cols.append([tuple(f[off[i]:off[i + 1]]) for i in range(len(off) - 1)])
    return list(zip(*cols))


def same_rows(what, got, want, unit="reads"):
    assert len(got) == len(want), f"{what}: {len(got)} {unit} from the device, {len(want)} in the model"
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:5]
    assert not bad, (f"{what}: first differing {unit} {bad}: device {[got[i] for i in bad]}, "
                     f"model {[want[i] for i in bad]}")


class Cell:
    """One (variant, consumer, k, strands, parameter set): the index and how the batch is fed to it."""

    def __init__(self, factory, consumer, variant, world, k, both, pss, psi):
        self.factory, self.consumer, self.variant, self.world, self.k, self.both = factory, consumer, variant, world, k, both
        self.genomes = world_genomes(world, k)
        self.psi = None if pss is None else psi % len(pss)
        self.ps = None if pss is None else pss[self.psi]
        self.prm = None if pss is None else A.params(self.ps)
        self.late = variant == "prepared_late"
        self.index = None
        self.label = (f"variant {variant}, consumer {consumer}, k={k}, {'both strands' if both else 'forward'}, "
                      f"parameters {self.ps}")

    def open(self):
        self.index = self.factory.build(self.variant, self.genomes, self.k, self.both, EXPECTED_READS[self.world])
        self.completed = False

    def renew(self):
        """A fresh index where the passes so far have changed it."""
        if self.variant in STATEFUL:
            self.close()
            self.open()

    def close(self):
        if self.variant in STATEFUL and self.index is not None:
            self.index.close()
        self.index = None

    def cuts(self, n):
        return [0, n // 2, n] if self.late else [0, n]

    def batches(self, tag, seqs, quals):
        c = self.cuts(len(seqs))
        return [self.factory.reads((tag, a, b), seqs[a:b], quals[a:b]) for a, b in zip(c, c[1:])]

    def between(self, j):
        """prepared_late: after the first half, prepare() makes the neighbour bits."""
        if self.late and j == 0 and not self.completed:
            b1 = int(self.index.info().device_bytes)
            self.index.prepare()
            b2 = int(self.index.info().device_bytes)
            assert b2 > b1, f"prepare() after prepare(expected_reads=1) made nothing: {b1} -> {b2} device bytes"
            self.completed = True

    def baseline(self, art):
        """`art` equals what the default variant gives for the same consumer, k, strands and parameters."""
        key = (self.consumer, self.k, self.both, self.psi)
        memo = self.factory.memo
        if self.variant == "default":
            memo[key] = art
            return
        if key not in memo:
            run_cell(self.factory, self.consumer, "default", self.k, self.both)
        assert art == memo[key], "differs from the default variant's result"


def c_reads(c):
    seqs, quals = TC.rand_reads(c.k)
    o = cov_model(c.k, c.both, c.psi)[0]
    got = []
    for j, dev in enumerate(c.batches(("cov", c.k), seqs, quals)):
        t, qf, hr, off, lists = N.align_reads(c.index, dev, c.prm)
        got += rows((t, qf, hr), off, (lists,))
        c.between(j)
    same_rows("align_reads (type, filtered k-mers, redundant k-mers, list)", got,
              rows((o.types, o.qf, o.hr), o.list_off, (o.lists,)))


def c_coverage(c):
    seqs, quals = TC.rand_reads(c.k)
    o, model = cov_model(c.k, c.both, c.psi)
    starts, du, da = model[0], model[1], model[2]
    cov = N.Coverage(c.index)
    got = []
    devs = c.batches(("cov", c.k), seqs, quals)
    for j, dev in enumerate(devs):
        t, loff, lists, st = N.align_placements(c.index, dev, c.prm)
        got += rows((t,), loff, (lists, st))
        cov.add(dev, c.prm)
        c.between(j)
    same_rows("align_placements (type, list, starts)", got, rows((o.types,), o.list_off, (o.lists, starts)))
    for g in range(len(c.genomes)):
        u, a = cov.depth(g)
        same_rows(f"unique depth of genome {g}", u.tolist(), du[g].tolist(), "positions")
        same_rows(f"ambiguous depth of genome {g}", a.tolist(), da[g].tolist(), "positions")
    for mc in (1, 2):
        cu, ca, su, sa = cov.summary(mc)
        mu, ma = TC.summarize(du, c.genomes, mc), TC.summarize(da, c.genomes, mc)
        assert (cu.tolist(), su.tolist(), ca.tolist(), sa.tolist()) == (mu[0], mu[1], ma[0], ma[1]), ("summary", mc)
    cov.close()
    if len(devs) == 1:
        TC.check_device(c.index, devs[0], c.prm, c.genomes, (o, model))


def c_pileup(c):
    seqs, quals = P.rand_reads(31, c.both)
    o, model = pile_model(c.both, c.psi)
    pl = N.Pileup(c.index)
    for j, dev in enumerate(c.batches(("pile", c.both), seqs, quals)):
        pl.add(dev, c.prm, 0)
        c.between(j)
    for g in range(len(c.genomes)):
        same_rows(f"pileup counts of genome {g}", pl.counts(g).tolist(), model[0][g].tolist(), "positions")
    P.check_device(pl, c.genomes, model)
    art = pl.variants(4, 2, 500).tobytes()
    pl.close()
    c.baseline(art)


def c_candidates(c):
    seqs, quals = A.rand_reads()
    types, sets, _ = abd_model(c.k, c.both, c.psi)
    ab = N.Abundance(c.index)
    got = []
    devs = c.batches(("abd",), seqs, quals)
    for j, dev in enumerate(devs):
        t, off, flat = N.align_candidates(c.index, dev, c.prm)
        got += rows((t,), off, (flat,))
        ab.add(dev, c.prm)
        c.between(j)
    same_rows("align_candidates (type, set)", got, list(zip(types, sets)))
    want = AM.classes_of(sets)
    same_rows("Abundance.classes (set, reads)", A.classes_list(ab), want, "classes")
    info = ab.info()
    assert [info[n] for n in ("reads_unique", "reads_ambiguous", "reads_unmapped", "reads_dropped")] == \
        [types.count(x) for x in (AM.UNIQUE, AM.AMBIGUOUS, AM.UNMAPPED, AM.DROPPED)], info
    assert (info["n_classes"], info["class_entries"]) == (len(want), sum(len(s) for s, _ in want)), info
    art = A.bits(ab.estimate(60, 0.0))
    ab.close()
    if len(devs) == 1:
        A.check_device(c.index, devs[0], c.prm, types, sets).close()
    c.baseline(art)


def c_lineage(c):
    seqs, quals = A.rand_reads()
    types, _, _ = abd_model(c.k, c.both, c.psi)
    parent, node = lineage_tree()
    G = len(c.genomes)
    nodes = abd_nodes(c.k, c.both, c.psi, G)
    lin = N.Lineage(c.index, parent, node[:G])
    got = []
    for j, dev in enumerate(c.batches(("abd",), seqs, quals)):
        got += lin.add(dev, c.prm).tolist()
        c.between(j)
    same_rows("Lineage.add (node)", got, nodes)
    LG.check_counts(lin, parent, nodes, types)
    lin.close()


def c_pairs(c):
    pairs = pair_list(c.k)
    results = pair_model(c.k, c.both, c.psi)
    cuts = c.cuts(len(pairs))
    for n, mode in enumerate((None, "0")):
        if n:
            c.renew()
        with set_env({"PA_PAIR_COMBINE": mode}):
            for j, (a, b) in enumerate(zip(cuts, cuts[1:])):
                m1, m2 = c.factory.pairs(("pair", c.k, a, b), pairs[a:b])
                try:
                    GP.check_pairs(c.index, m1, m2, c.prm, results[a:b], base=a, combine=mode is None)
                except AssertionError as e:
                    raise AssertionError(f"PA_PAIR_COMBINE={mode}, pairs {a}..{b}: {e}") from e
                c.between(j)


def c_positions(c):
    kmers, sets, queries = cov_kmer_dict(c.k), cov_kmer_sets(c.k, c.both), pos_queries(c.k)
    for j in range(2 if c.late else 1):
        for reverse in (False, True):
            hits = c.index.positions(queries, reverse=reverse)
            assert reverse or not (hits["query"] >> 31).any()
            got = {}
            for q, g, p in hits.tolist():
                got.setdefault(q & 0x7FFFFFFF, {}).setdefault(g, []).append(p)
            same_rows(f"positions(reverse={reverse})",
                      [sorted((g, sorted(p)) for g, p in got.get(qi, {}).items()) for qi in range(len(queries))],
                      [sorted(O.kmer_references(kmers, q, reverse)) for q in queries], "queries")
        cls, size = c.index.lookup(queries)
        same_rows("lookup / class_genomes (set size, set)",
                  [(int(s), tuple(c.index.class_genomes(int(x))) if x >= 0 else ()) for x, s in zip(cls, size)],
                  [(len(sets.get(q, ())), sets.get(q, ())) for q in queries], "queries")
        c.between(j)


def dump(index, genomes, keep=None):
    """pa_index_dumpref of `index` as the dict KmerReference.get_summary builds from it (without "Similarity")."""
    names = [f"genome_{i}" for i in range(len(genomes))]
    with tempfile.TemporaryFile() as f:
        uniq, multi, order, last, nk = N.index_dumpref(index, keep, np.arange(len(names), dtype=np.uint32),
                                                       [json.dumps(n) for n in names], f.fileno())
        f.seek(0)
        kmers = json.loads(f.read())
    assert nk == len(kmers)
    present = sorted((d for d in range(len(names)) if int(order[d]) != N.NO_ORDER), key=lambda d: int(order[d]))
    summary = {names[d]: {"total_bases": len(genomes[int(last[d])]), "unique_kmers": int(uniq[d]),
                          "multi_mapping_kmers": int(multi[d])} for d in present}
    return {"Kmers": kmers, "Summary": summary}, names


def same_dump(what, got, want):
    same_rows(what + ": Kmers", list(got["Kmers"].items()), list(want["Kmers"].items()), "k-mers")
    same_rows(what + ": Summary", list(got["Summary"].items()), list(want["Summary"].items()), "genomes")


def c_dumpref(c):
    G = len(c.genomes)
    group_of = [g // 2 for g in range(G)]
    ng = group_of[-1] + 1
    want = O.OracleIndex(TC.regions_of(c.genomes, c.both), c.k).extsim_stats(group_of, ng)
    for j in range(2 if c.late else 1):
        for name, a, b in zip(("total", "unique", "intersections"), c.index.extsim_stats(group_of, ng), want):
            assert a.tolist() == b.tolist(), ("extsim_stats", name)
        if c.both:  # the dump is of the forward k-mer database: refused on a both-strand index (include/pa.h)
            with pytest.raises(N.PaUnsupported):
                dump(c.index, c.genomes)
        else:
            got, names = dump(c.index, c.genomes)
            same_dump("dumpref", got, O.dumpref_summary(list(zip(names, c.genomes)), c.k))
        c.between(j)
    if c.variant.startswith("reduced") and not c.both:
        # what KmerReference dumps after EXTSIM: an index of every original genome, the kept ones as a mask
        full, keep = with_decoys(c.genomes)
        mask = np.zeros(len(full), dtype=np.uint8)
        mask[keep] = 1
        index = N.Index(full, c.k, defer_tiles=True)
        got, names = dump(index, full, mask)
        index.close()
        same_dump("masked dumpref", got, O.dumpref_summary(list(zip(names, full)), c.k, {names[i] for i in keep}))


CONSUMERS = {  # name: (function, world, the module's parameter sets or None)
    "reads": (c_reads, "cov", TC.RAND_PS),
    "candidates": (c_candidates, "abd", A.RAND_PS),
    "coverage": (c_coverage, "cov", TC.RAND_PS),
    "pileup": (c_pileup, "cov", P.RAND_PS),
    "pairs": (c_pairs, "pair", PM.RAND_PS),
    "lineage": (c_lineage, "abd", A.RAND_PS),
    "positions": (c_positions, "cov", None),
    "dumpref": (c_dumpref, "cov", None),
}
WIDE_CONSUMERS = ("candidates", "coverage", "pairs", "positions")
assert all(pss[0] == dict(m=1, p=1) for _, _, pss in CONSUMERS.values() if pss)


def run_cell(factory, consumer, variant, k, both):
    fn, world, pss = CONSUMERS[consumer]
    with variant_env(variant):
        for psi in ((0, -1) if pss else (None,)):  # m=1, p=1 and the module's last set (quality filter, --max-genomes)
            c = Cell(factory, consumer, variant, world, k, both, pss, psi)
            print(c.label)
            try:
                c.open()
                fn(c)
            except AssertionError as e:
                raise AssertionError(f"{c.label}: {e}") from e
            finally:
                c.close()


def cells():
    out = []
    for consumer in CONSUMERS:
        out += [(consumer, v, 31, False) for v in VARIANTS] + [(consumer, v, 31, True) for v in BOTH_TOO]
    for consumer in WIDE_CONSUMERS:  # two key words; four (no lane path: the view must still serve it)
        out += [(consumer, v, 63, both) for v in WIDE for both in (False, True)] + [(consumer, v, 97, False) for v in WIDE]
    return out


@pytest.mark.parametrize("consumer, variant, k, both", cells(),
                         ids=[f"{c}-{v}-k{k}-{'both_strands' if b else 'forward'}" for c, v, k, b in cells()])
def test_cell(consumer, variant, k, both, factory):
    run_cell(factory, consumer, variant, k, both)


# ---- 4. the cells are not the exact kernel doing all the work ------------------------------------

def world_batch(factory, world):
    if world == "cov":
        return factory.reads((("cov", 31), 0, 2000), *TC.rand_reads(31))
    if world == "abd":
        return factory.reads((("abd",), 0, 4000), *A.rand_reads())
    pairs = pair_list(31)
    return factory.pairs(("pair", 31, 0, len(pairs)), pairs)[0]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("world", ["cov", "abd", "pair"])
def test_lane_kernel_ran(world, variant, factory):
    """On every variant that has tiles k_align_lane runs in the assign pass of the world's batch; on no_tile it
    does not (its second witness).  Prints the figures of DESIGN.md section 18."""
    genomes = world_genomes(world, 31)
    with variant_env(variant):
        index = factory.build(variant, genomes, 31, False, EXPECTED_READS[world])
        dev = world_batch(factory, world)
        index.profile_enable(True)
        try:
            index.profile_read_kernels()
            N.align_reads(index, dev, N.Params.make(1, 1))
            launched = {name: n for name, (_, n) in index.profile_read_kernels().items()}
        finally:
            index.profile_enable(False)
        if variant in STATEFUL:
            index.close()
    s = factory.snaps[(variant, tuple(genomes), 31, False)]  # (as built: before any pass made a view of its own)
    print(f"\nlayout {world} {variant}: table_slots {s['slots']}, device_bytes {s['bytes']}, "
          f"assign pass launches {launched}")
    if variant == "no_tile":
        assert launched["k_align_lane"] == 0 and launched["k_align_exact"] >= 1, launched
    else:
        assert launched["k_align_lane"] >= 1, launched


def test_witnesses_reject_a_build_without_the_switch(factory):
    """Every witness fails on a build made without its variant's flags and environment (the default build;
    for `default` itself, the compact one)."""
    genomes = world_genomes("cov", 31)

    def ref(name):
        return factory.snap(name, genomes, 31, False)
    for variant in VARIANTS:
        if variant in UNWITNESSED:
            continue
        wrong = ref("compact" if variant == "default" else "default")
        with pytest.raises(AssertionError):
            witness(variant, wrong, ref)
        witness(variant, ref(variant), ref)


# ---- 5. the positions view before and after the first pass ----------------------------------------

@pytest.mark.parametrize("order", ["view_first", "pass_first"])
@pytest.mark.parametrize("consumer", ["coverage", "pileup"])
def test_deferred_view_order(consumer, order, factory):
    """prepare_coverage() on a deferred build before anything ran, and after the consumer's first pass made
    the align-side view and the positions view itself: the model's results either way."""
    fn, world, pss = CONSUMERS[consumer]
    with variant_env("deferred"):
        c = Cell(factory, consumer, "deferred", world, 31, False, pss, -1)
        c.label += f", {order}"
        c.baseline = lambda art: None
        try:
            c.open()
            if order == "pass_first":
                fn(c)
            c.index.prepare_coverage()
            fn(c)
        except AssertionError as e:
            raise AssertionError(f"{c.label}: {e}") from e
        finally:
            c.close()


# ---- 6. pairs outside the mask regime --------------------------------------------------------------

LARGE_IDS = [f"{s[0]}_genomes" for s in PM.LARGE_SHAPES]


def large_pairs_cell(factory, shape, both, variant):
    genomes, pairs = PM.large_pairs(shape)
    k = shape[3]
    with variant_env(variant):
        index = factory.build(variant, genomes, k, both)
        m1, m2 = factory.pairs(("large", shape), pairs)
        for i, ps in enumerate(PM.LARGE_PS):
            results = PM.large_model(shape, both, i)
            kept = sum(r[0] != PM.DROPPED for r in results)
            for mode in (None, "0"):
                label = (f"variant {variant}, consumer pairs, G={shape[0]}, k={k}, "
                         f"{'both strands' if both else 'forward'}, parameters {ps}, PA_PAIR_COMBINE={mode}")
                print(label)
                with set_env({"PA_PAIR_COMBINE": mode}):
                    try:
                        exact = GP.check_pairs(index, m1, m2, A.params(ps), results, base=7 * i, combine=mode is None)
                        if mode is None:
                            assert 0 < exact < len(pairs), f"exact_pairs {exact} of {len(pairs)}"
                        else:
                            assert exact == kept, f"exact_pairs {exact}, kept {kept}"
                    except AssertionError as e:
                        raise AssertionError(f"{label}: {e}") from e


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
@pytest.mark.parametrize("shape", PM.LARGE_SHAPES, ids=LARGE_IDS)
def test_pairs_many_genomes(shape, both, factory):
    """k_align_pair_exact over 70 genomes (class records, LDS counters), 300 and 2100 (the global workspace)."""
    large_pairs_cell(factory, shape, both, "default")


@pytest.mark.parametrize("variant", ["compact", "large_hi1"])
@pytest.mark.parametrize("shape", PM.LARGE_SHAPES, ids=LARGE_IDS)
def test_pairs_many_genomes_on_variants(shape, variant, factory):
    large_pairs_cell(factory, shape, False, variant)
