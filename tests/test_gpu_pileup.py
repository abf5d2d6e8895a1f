"""Per-base pileup and SNV calls (pa_pileup_*, Pileup, PseudoAlignment(pileup=True),
main.py --variants) on the GPU.

The reference has no such code, so the definition is
restated here as a small pure-Python model: mapping types and genome lists from
the CPU oracle (never from libpa), placements from the coverage model's votes
(tests/test_gpu_coverage.py) with "one distinct diagonal" as the consistency
test.  Everything the device returns -- all counts of all genomes, the stats,
the variant records -- is compared with the model for exact equality;
tests/test_pileup_host.py pins the model itself on the CPU.
"""

import collections
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import pa_native as N
import pa_oracle as O
import test_gpu_coverage as TC

pytestmark = pytest.mark.gpu

UNIQUE, AMBIGUOUS = TC.UNIQUE, TC.AMBIGUOUS
TRIPLES = [(1, 1, 0), (4, 2, 500), (8, 3, 200)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


# ---- the model ------------------------------------------------------------------------

def diagonals(first, seq, g, k):
    """The diagonals the windows of `seq` vote for on genome g, with their votes (TC.place's count)."""
    votes = collections.Counter()
    for j in range(len(seq) - k + 1):
        p = first.get(seq[j:j + k], {}).get(g)
        if p is not None:
            votes[p - j] += 1
    return votes


_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def pile(genomes, both, k, seqs, quals, types, list_off, lists, min_base_quality=0, first=None, memo=None):
    """The model: (counts per genome, (n, 4) uint32; stats dict)."""
    regions = TC.regions_of(genomes, both)
    first = TC.first_occurrences(regions, k) if first is None else first
    memo = {} if memo is None else memo
    counts = [np.zeros((len(g), 4), dtype=np.uint32) for g in genomes]
    piled = skipped = bases = 0
    for r, (seq, qual) in enumerate(zip(seqs, quals)):
        if types[r] != UNIQUE:
            continue
        gl = [int(x) for x in lists[int(list_off[r]):int(list_off[r + 1])]]
        assert len(gl) == 1, "a uniquely mapped read's list is exactly [g]"
        g = gl[0]
        if (r, g) not in memo:
            memo[r, g] = diagonals(first, seq, g, k)
        votes = memo[r, g]
        assert votes, "a listed genome without a voting window"
        if len(votes) > 1:
            skipped += 1
            continue
        piled += 1
        s = next(iter(votes))
        n, R = len(genomes[g]), len(regions[g])
        code = _CODE[np.frombuffer(seq.encode("latin-1"), dtype=np.uint8)]
        ql = np.frombuffer(qual.encode("latin-1"), dtype=np.uint8)
        q = s + np.arange(len(seq), dtype=np.int64)
        keep = (q >= 0) & (q < R) & (code < 4) & (ql >= min_base_quality)
        x, b = q.copy(), code.astype(np.int64)
        if both:
            keep &= q != n
            rev = q > n
            x[rev] = 2 * n - q[rev]
            b[rev] = 3 - b[rev]
        np.add.at(counts[g], (x[keep], b[keep]), 1)
        bases += int(keep.sum())
    return counts, {"reads_piled": piled, "reads_skipped": skipped, "bases_counted": bases}


def call(genomes, counts, min_depth, min_alt_count, min_alt_permille):
    """The records (genome, position, ref, alt, depth, alt_count, (A, C, G, T)) in the ABI's order."""
    recs = []
    for g, (text, c) in enumerate(zip(genomes, counts)):
        depth = c.sum(axis=1, dtype=np.int64)
        for x in np.flatnonzero(depth >= min_depth):
            ref = "ACGT".find(text[x])
            if ref < 0:
                continue
            D = int(depth[x])
            for b in range(4):
                cb = int(c[x, b])
                if b != ref and cb >= min_alt_count and 1000 * cb >= min_alt_permille * D:
                    recs.append((g, int(x), ref, b, D, cb, tuple(int(v) for v in c[x])))
    return recs


def records_of(arr):
    """Pileup.variants' structured array as the model's tuples."""
    return [(int(v["genome"]), int(v["position"]), int(v["ref"]), int(v["alt"]), int(v["depth"]),
             int(v["alt_count"]), tuple(int(x) for x in v["acgt"])) for v in arr]


def check_device(pile_dev, genomes, model, triples=TRIPLES):
    counts, stats = model
    for g in range(len(genomes)):
        got = pile_dev.counts(g)
        assert got.shape == (len(genomes[g]), 4) and got.dtype == np.uint32
        assert np.array_equal(got, counts[g]), g
    assert pile_dev.stats() == stats
    for t in triples:
        assert records_of(pile_dev.variants(*t)) == call(genomes, counts, *t), t


# ---- 1. hand-built corner cases ------------------------------------------------------------

HAND_PS = dict(m=1, p=1)
HAND_MBQ = 40
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


class _DeadEnd(Exception):
    pass


def _grow(rng, seq, n, k, used):
    """seq + n bases, every new k-mer and its reverse complement new to `used` (and added to it)."""
    for _ in range(n):
        for b in rng.permutation(4):
            cand = seq + "ACGT"[b]
            w = cand[-k:]
            if len(cand) < k or (w not in used and O.reverse_complement(w) not in used
                                 and w != O.reverse_complement(w)):
                break
        else:
            raise _DeadEnd
        if len(cand) >= k:
            used.update((w, O.reverse_complement(w)))
        seq = cand
    return seq


def _absent(text, k, used):
    return all(text[j:j + k] not in used for j in range(len(text) - k + 1))


def _filler(left, right, ns, k, used):
    """n bases (n in `ns`) between `left` and `right` such that no window touching them is a k-mer of a region."""
    for n in ns:
        for t in itertools.product("ACGT", repeat=n):
            t = "".join(t)
            if _absent(left[-(k - 1):] + t + right[:k - 1], k, used):
                return t
    raise _DeadEnd


def lay(exp, g, x0, text, times=1):
    """`text` lies at forward positions x0.. of genome g, `times` reads deep (non-ACGT bytes count nothing)."""
    for i, ch in enumerate(text):
        if ch in "ACGT":
            exp[g][x0 + i, "ACGT".index(ch)] += times


@functools.lru_cache(maxsize=None)
def hand_case(k):
    """Five genomes of 0-48 bases whose k-mers -- reverse complements included --
    are all distinct, except a stretch g1 and g2 share; g2 holds an N.  Returns
    (genomes, reads [(name, seq, qual)], expected(both) -> (counts, piled reads),
    position and bases of the two-alternative site)."""
    for seed in range(200):
        rng = np.random.default_rng(100 * k + seed)
        used = set()
        try:
            g0 = _grow(rng, "", 44, k, used)
            g1 = _grow(rng, "", 44, k, used)
            S = k + 9
            shared = g1[20:20 + S]
            for _ in range(40):  # a head whose junction with the shared stretch makes new k-mers only
                trial = set(used)
                head = _grow(rng, "", 12, k, trial)
                joint = head[-(k - 1):] + shared[:k - 1]
                if _absent(joint, k, trial):
                    break
            else:
                raise _DeadEnd
            used = trial
            for j in range(k - 1):
                used.update((joint[j:j + k], O.reverse_complement(joint[j:j + k])))
            g2_full = _grow(rng, head + shared, 12, k, used)
            g2 = g2_full[:5] + "N" + g2_full[6:]
            g3 = _grow(rng, "", 48, k, used)
            j1 = _filler("", g0[:12], [3], k, used)
            j2 = _filler(g0[32:], "", [3], k, used)
            rc0 = O.reverse_complement(g0[0:12])
            j3 = _filler(rc0, "", [3], k, used)
            sep = g1[35:44]
            x1 = _filler(sep, O.reverse_complement(sep), [1], k, used)
            junk = _filler("", "", [14], k, used)
            amb_a, amb_b = g0[20:20 + k + 2], g1[0:k + 2]
            amb = amb_a + _filler(amb_a, amb_b, [1, 2, 3], k, used) + amb_b
            dem = g0[0:k + 3] + _filler(g0[0:k + 3], shared, [1, 2, 3], k, used) + shared
            inc_a, inc_b = g3[2:2 + k + 1], g3[24:24 + k + 1]
            inc = inc_a + _filler(inc_a, inc_b, [1, 2, 3], k, used) + inc_b
            for a0 in range(48 - (2 * k + 3) + 1):  # a site both of whose changed bases make no k-mer of a region
                pos = a0 + k + 1
                plain = g3[a0:a0 + 2 * k + 3]
                alts = [b for b in "ACGT" if b != g3[pos]
                        and _absent(plain[2:k + 1] + b + plain[k + 2:2 * k + 1], k, used)]
                if len(alts) >= 2:
                    break
            else:
                raise _DeadEnd
        except _DeadEnd:
            continue
        break
    else:
        raise AssertionError("no seed gives the hand-built genomes")
    genomes = [g0, g1, g2, g3, ""]
    hi = "I"
    nm = g0[10:15] + "N" + g0[16:22] + "." + g0[23:30]
    qread = g1[0:20]
    qq = hi * 3 + chr(HAND_MBQ - 1) + hi * 5 + chr(HAND_MBQ) + hi * 10
    mut = [plain[:pos - a0] + b + plain[pos - a0 + 1:] for b in alts[:2]]
    once = g0[5:25]
    reads = [
        ("start_overhang", j1 + g0[0:12]),                         # s = -3
        ("end_overhang", g0[32:44] + j2),                          # runs out of g0 (into the N and the reverse half)
        ("region_end_overhang", rc0 + j3),                         # runs out of the both-strand region
        ("reverse_half", O.reverse_complement(g1[0:18])),
        ("across_separator", sep + x1 + O.reverse_complement(sep)),
        ("n_and_other_byte", nm),
        ("base_quality", qread),
        ("short", g0[0:k - 1]),
        ("unmapped", junk),
        ("ambiguous", amb),
        ("p_demoted", dem),
        ("inconsistent", inc),                                     # two diagonals
        ("reference_n", g2_full[0:15]),                            # over g2's N
        ("alt_plain", plain), ("alt_1", mut[0]), ("alt_2", mut[1]),
    ] + [("copy", once)] * 300
    reads = [(n, s, qq if n == "base_quality" else hi * len(s)) for n, s in reads]

    def expected(both):
        exp = [np.zeros((len(g), 4), dtype=np.uint32) for g in genomes]
        lay(exp, 0, 0, g0[0:12])
        lay(exp, 0, 32, g0[32:44])
        piled = 2
        if both:  # j2[0] falls on the N between the strands, j2[1], j2[2] on the reverse half's first bases
            lay(exp, 0, 43, COMP[j2[1]])
            lay(exp, 0, 42, COMP[j2[2]])
            lay(exp, 0, 0, g0[0:12])      # region_end_overhang
            lay(exp, 1, 0, g1[0:18])      # reverse_half
            lay(exp, 1, 35, sep)          # across_separator: its second half
            piled += 2
        lay(exp, 1, 35, sep)
        lay(exp, 0, 10, nm)
        lay(exp, 1, 0, qread[0:3])
        lay(exp, 1, 4, qread[4:20])
        lay(exp, 2, 0, g2_full[0:15])
        for t in [plain] + mut:
            lay(exp, 3, a0, t)
        lay(exp, 0, 5, once, 300)
        return exp, piled + 7 + 300

    return genomes, reads, expected, (pos, g3[pos], alts[:2])


def hand_model(k, both):
    """(oracle result, model) of the hand-built case, its corners asserted on the model's side."""
    genomes, reads, _, _ = hand_case(k)
    names, seqs, quals = ([r[i] for r in reads] for i in range(3))
    seq, off = O.concat(seqs)
    qual, _ = O.concat(quals)
    o = TC.oracle_lists(genomes, both, k, (seq, qual, off), HAND_PS)
    ty = {n: int(t) for n, t in zip(names, o.types)}
    for n in ("start_overhang", "end_overhang", "across_separator", "n_and_other_byte", "base_quality",
              "inconsistent", "reference_n", "alt_plain", "alt_1", "alt_2", "copy"):
        assert ty[n] == UNIQUE, n
    for n in ("region_end_overhang", "reverse_half"):
        assert ty[n] == (UNIQUE if both else 1), n
    assert ty["short"] == 1 and ty["unmapped"] == 1 and ty["ambiguous"] == AMBIGUOUS
    gl = o.genomes_of(names.index("p_demoted"))
    assert ty["p_demoted"] == AMBIGUOUS and len(gl) > 1 and gl.count(gl[0]) == 2
    first = TC.first_occurrences(TC.regions_of(genomes, both), k)
    assert len(diagonals(first, seqs[names.index("inconsistent")], 3, k)) == 2
    assert next(iter(diagonals(first, seqs[0], 0, k))) == -3
    return o, pile(genomes, both, k, seqs, quals, o.types, o.list_off, o.lists, HAND_MBQ, first)


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
@pytest.mark.parametrize("k", [5, 7])
def test_hand_built(k, both):
    genomes, reads, expected, (pos, ref, alts) = hand_case(k)
    o, model = hand_model(k, both)
    exp, piled = expected(both)
    dev, _ = TC.upload([r[1] for r in reads], [r[2] for r in reads])
    index = N.Index(genomes, k, both_strands=both)
    pl = N.Pileup(index)
    pl.add(dev, N.Params.make(**HAND_PS), HAND_MBQ)
    for g in range(len(genomes)):
        assert np.array_equal(pl.counts(g), exp[g]), g          # the hand-written counts
    assert pl.counts(4).shape == (0, 4)                         # the empty genome
    assert pl.stats() == {"reads_piled": piled, "reads_skipped": 1,
                          "bases_counted": int(sum(int(e.sum(dtype=np.uint64)) for e in exp))}
    assert int(pl.counts(0, 24, 1)[0, "ACGT".index(genomes[0][24])]) == 300 + 1  # the copies and n_and_other_byte
    check_device(pl, genomes, model)                            # and the model agrees
    recs = records_of(pl.variants(1, 1, 0))
    here = [r for r in recs if r[0] == 3 and r[1] == pos]
    assert [(r[2], r[3], r[4], r[5]) for r in here] == [("ACGT".index(ref), "ACGT".index(a), 3, 1)
                                                        for a in sorted(alts, key="ACGT".index)]
    assert not any(r[0] == 2 and r[1] == 5 for r in recs)      # the reference N: counted, never called
    assert int(pl.counts(2, 5, 1).sum()) == 1
    for x in (pl, dev, index):
        x.close()


# ---- 2. randomised against the model ---------------------------------------------------------

RAND_KS = [15, 31, 33, 75]
RAND_PS = [dict(m=1, p=1), dict(m=1, p=1, mkq=61, mg=2)]
# Seeds: the strains' and the reads'.  At k = 75 few reads keep clean windows on both sides of a
# repeat boundary (18-62 skipped reads over the seeds tried, against 84-143 at the shorter k);
# strain seed 19 with read seed 10 gives at least 50 there for both kinds of index.
RAND_SEED = 19
READ_SEED = {15: 1, 31: 10, 33: 10, 75: 10}  # (10 at k = 15 gives 6 records off the planted sites, one too many)


@functools.lru_cache(maxsize=None)
def rand_strains():
    """TC.rand_genomes with one substitution planted every 100-199 bases, the
    first at 20-119: (reference genomes, strains, planted sites {(g, x)})."""
    genomes = TC.rand_genomes()[0]
    rng = np.random.default_rng(RAND_SEED)
    strains, sites = [], set()
    for g, text in enumerate(genomes):
        s = list(text)
        x = int(rng.integers(20, 120))
        while x < len(s):
            s[x] = "ACGT"[("ACGT".index(s[x]) + int(rng.integers(1, 4))) % 4]
            sites.add((g, x))
            x += int(rng.integers(100, 200))
        strains.append("".join(s))
    return genomes, strains, sites


@functools.lru_cache(maxsize=None)
def rand_reads(k, both):
    """3 000 reads of max(40, k + 10)..272 bases drawn from the strains, 1 % substitutions."""
    _, strains, _ = rand_strains()
    rng = np.random.default_rng(READ_SEED[k] * 1000 + 2 * k + both)
    return TC.sample_reads(rng, strains, 3000, max(40, k + 10), 272, sub=0.01, rc=0.3 if both else 0.0)


@functools.lru_cache(maxsize=None)
def rand_shared(k, both):
    return TC.first_occurrences(TC.regions_of(rand_strains()[0], both), k), {}


def rand_model(k, both, ps, mbq=0):
    genomes = rand_strains()[0]
    seqs, quals = rand_reads(k, both)
    seq, off = O.concat(seqs)
    qual, _ = O.concat(quals)
    o = TC.oracle_lists(genomes, both, k, (seq, qual, off), ps)
    first, memo = rand_shared(k, both)
    return o, pile(genomes, both, k, seqs, quals, o.types, o.list_off, o.lists, mbq, first, memo)


def rand_conditions(o, model):
    """The inputs exercise the feature (asserted on the model's side)."""
    genomes, _, sites = rand_strains()
    counts, stats = model
    assert int((o.types == UNIQUE).sum()) >= 1000
    assert stats["reads_skipped"] >= 50
    deep = {(g, x) for g, x in sites if int(counts[g][x].sum()) >= 4}
    assert len(deep) >= 80
    recs = call(genomes, counts, 4, 2, 500)
    called = {(r[0], r[1]) for r in recs}
    assert len(called & deep) >= 0.9 * len(deep)
    assert sum(1 for r in recs if (r[0], r[1]) not in sites) <= 5


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both_strands"])
@pytest.mark.parametrize("k", RAND_KS)
def test_random_vs_model(k, both):
    genomes = rand_strains()[0]
    models = [rand_model(k, both, ps) for ps in RAND_PS]
    rand_conditions(*models[0])
    half = rand_model(k, both, RAND_PS[0], 62)
    full, cut = models[0][1][1]["bases_counted"], half[1][1]["bases_counted"]
    assert 0.4 * full <= cut <= 0.6 * full  # (qualities uniform in 50..74: 62 cuts about half)
    seqs, quals = rand_reads(k, both)
    assert max(len(s) for s in seqs) > 192 and min(len(s) for s in seqs) < 128  # 2 to 5 rounds of the lane stride
    dev, _ = TC.upload(seqs, quals)
    index = N.Index(genomes, k, both_strands=both)
    pl = N.Pileup(index)
    for ps, mbq, (o, model) in [(RAND_PS[0], 0, models[0]), (RAND_PS[1], 0, models[1]), (RAND_PS[0], 62, half)]:
        pl.reset()
        pl.add(dev, N.Params.make(ps["m"], ps["p"], None, ps.get("mkq"), ps.get("mg")), mbq)
        check_device(pl, genomes, model)
    for x in (pl, dev, index):
        x.close()


# ---- 3. more than 64 genomes (k_place's class records) ---------------------------------------------

def test_more_than_64_genomes():
    genomes, (seqs, quals) = TC.many_case()
    dev, host = TC.upload(seqs, quals)
    ps = dict(m=1, p=1)
    o = TC.oracle_lists(genomes, False, 21, host, ps)
    model = pile(genomes, False, 21, seqs, quals, o.types, o.list_off, o.lists)
    assert model[1]["reads_piled"] >= 100
    index = N.Index(genomes, 21)
    pl = N.Pileup(index)
    pl.add(dev, N.Params.make(1, 1))
    check_device(pl, genomes, model)
    for x in (pl, dev, index):
        x.close()


# ---- 4. the invariant against coverage -------------------------------------------------------------

def test_invariant_against_coverage():
    """ACGT-only reads, no base-quality threshold: the unique depth of a
    position is at least the sum of its four counts, and equal to it when the
    batch holds no inconsistent unique read."""
    genomes = rand_strains()[0]
    seqs, quals = rand_reads(31, False)
    seqs, quals = list(seqs[:1200]), list(quals[:1200])
    seq, off = O.concat(seqs)
    qual, _ = O.concat(quals)
    o = TC.oracle_lists(genomes, False, 31, (seq, qual, off), RAND_PS[0])
    first, _ = rand_shared(31, False)
    bad = {r for r in range(len(seqs)) if o.types[r] == UNIQUE
           and len(diagonals(first, seqs[r], o.genomes_of(r)[0], 31)) > 1}
    assert len(bad) >= 10
    keep = [r for r in range(len(seqs)) if r not in bad]
    index = N.Index(genomes, 31)
    prm = N.Params.make(1, 1)
    for pick, equal in ((range(len(seqs)), False), (keep, True)):
        dev, _ = TC.upload([seqs[r] for r in pick], [quals[r] for r in pick])
        pl, cov = N.Pileup(index), N.Coverage(index)
        pl.add(dev, prm)
        cov.add(dev, prm)
        assert pl.stats()["reads_skipped"] == (0 if equal else len(bad))
        strict = 0
        for g in range(len(genomes)):
            du = cov.depth(g)[0].astype(np.int64)
            tot = pl.counts(g).sum(axis=1, dtype=np.int64)
            assert (du >= tot).all(), g
            strict += int((du > tot).sum())
        assert (strict == 0) if equal else (strict > 0)
        for x in (pl, cov, dev):
            x.close()
    index.close()


# ---- 5. accumulation and lifetime ------------------------------------------------------------------

def all_counts(pl, n):
    return [pl.counts(g).tolist() for g in range(n)]


def test_accumulation_and_lifetime():
    genomes = rand_strains()[0]
    seqs, quals = rand_reads(31, False)
    seqs, quals = seqs[:600], quals[:600]
    prm = N.Params.make(1, 1)
    index, other = N.Index(genomes, 31), N.Index(genomes, 31)
    whole, _ = TC.upload(seqs, quals)
    h1, _ = TC.upload(seqs[:250], quals[:250])
    h2, _ = TC.upload(seqs[250:], quals[250:])
    one, two = N.Pileup(index), N.Pileup(index)
    b0 = int(index.info().device_bytes)
    one.add(whole, prm)
    two.add(h1, prm)
    two.add(h2, prm)
    ref = all_counts(one, 6)
    assert any(any(any(p) for p in c) for c in ref)
    assert all_counts(two, 6) == ref and two.stats() == one.stats()
    assert records_of(two.variants(4, 2, 500)) == records_of(one.variants(4, 2, 500))
    part = one.counts(2, 100, 250)
    assert part.tolist() == ref[2][100:350] and one.counts(2, len(genomes[2]), 0).shape == (0, 4)
    two.reset()
    assert not any(any(any(p) for p in c) for c in all_counts(two, 6))
    assert two.stats() == {"reads_piled": 0, "reads_skipped": 0, "bases_counted": 0}
    assert two.variants(1, 1, 0).size == 0  # zero records
    two.add(whole, prm)  # (and it accumulates again after a reset)
    assert all_counts(two, 6) == ref
    # the short-capacity protocol
    lib = N.lib()
    n = N.U64(0)
    assert lib.pa_pileup_variants(one.handle, 4, 2, 500, None, 0, N.ctypes.byref(n), None) == N.PA_EINVAL
    total = int(n.value)
    assert total == len(one.variants(4, 2, 500)) and total >= 2
    buf = np.zeros(total, dtype=N.VARIANT_DTYPE)
    buf["genome"] = 77
    assert lib.pa_pileup_variants(one.handle, 4, 2, 500, N._ptr(buf), total - 1, N.ctypes.byref(n), None) == N.PA_EINVAL
    assert int(n.value) == total and (buf["genome"] == 77).all()  # nothing written
    assert lib.pa_pileup_variants(one.handle, 4, 2, 500, N._ptr(buf), total, N.ctypes.byref(n), None) == N.PA_OK
    assert records_of(buf) == records_of(one.variants(4, 2, 500))
    # the argument checks
    for bad in ((0, 1, 0), (1, 0, 0), (1, 1, 1001)):
        assert lib.pa_pileup_variants(one.handle, *bad, None, 0, N.ctypes.byref(n), None) == N.PA_EINVAL
        with pytest.raises(ValueError):
            one.variants(*bad)
    assert lib.pa_pileup_counts(one.handle, 6, 0, 0, None, None) == N.PA_EINVAL
    assert lib.pa_pileup_counts(one.handle, 1, len(genomes[1]), 1, N._ptr(buf), None) == N.PA_EINVAL
    # another index; its own index after a reduce
    assert lib.pa_pileup_add(other.handle, whole.handle, prm, 0, one.handle, None) == N.PA_EINVAL
    assert int(index.info().device_bytes) >= b0  # (the accumulators are not the index's: only the view was added)
    index.reduce([0, 2, 3, 5])
    with pytest.raises(ValueError):
        one.add(whole, prm)
    assert all_counts(one, 6) == ref  # (what it holds stays readable)
    for x in (one, two, whole, h1, h2, index, other):
        x.close()


def test_device_bytes_unchanged_by_pileup():
    genomes = rand_strains()[0][:3]
    index = N.Index(genomes, 31)
    index.prepare_coverage()
    b1 = int(index.info().device_bytes)
    pl = N.Pileup(index)
    seqs, quals = rand_reads(31, False)
    dev, _ = TC.upload(seqs[:50], quals[:50])
    pl.add(dev, N.Params.make(1, 1))
    assert int(index.info().device_bytes) == b1
    for x in (pl, dev, index):
        x.close()


# ---- 6. drop-in API and CLI ------------------------------------------------------------------------

CLI_CASES, FA, FQ, MAIN = TC.CLI_CASES, TC.FA, TC.FQ, TC.MAIN


def config1_records(both=False, triple=(4, 2, 200), mbq=0):
    gen, reads = TC.config1()
    gs = [g for _, g in gen]
    seqs, quals = [s for s, _ in reads], [q for _, q in reads]
    seq, off = O.concat(seqs)
    qual, _ = O.concat(quals)
    o = TC.oracle_lists(gs, both, 21, (seq, qual, off), dict(m=1, p=1))
    first, _ = TC.config1_first(both)
    counts, _ = pile(gs, both, 21, seqs, quals, o.types, o.list_off, o.lists, mbq, first)
    return [n for n, _ in gen], call(gs, counts, *triple)


def variants_text(names, recs):
    out = ["#genome\tposition\tref\talt\tdepth\talt_count\tA\tC\tG\tT\n"]
    for g, x, ref, alt, depth, ac, acgt in recs:
        out.append("\t".join([names[g], str(x), "ACGT"[ref], "ACGT"[alt], str(depth), str(ac)]
                             + [str(v) for v in acgt]) + "\n")
    return "".join(out)


def test_cli_variants(tmp_path):
    from data_file import FASTAFile
    from kmer import KmerReference, PseudoAlignment
    import io
    f = str(tmp_path / "v.tsv")
    r = TC.run_cli(["--variants", f])
    assert r.returncode == 0, r.stderr
    assert r.stdout == CLI_CASES[0]["stdout"]  # stdout: what is pinned without the flag
    text = open(f).read()
    ref = KmerReference(21, FASTAFile(FA).container)
    plain = PseudoAlignment(ref)
    for fn in (plain.get_variants, lambda: plain.write_variants(io.StringIO())):
        with pytest.raises(ValueError):
            fn()
    pa = PseudoAlignment(ref, pileup=True)
    pa.align_reads_from_file(FQ)
    buf = io.StringIO()
    pa.write_variants(buf)
    assert text == buf.getvalue()
    names, recs = config1_records()
    assert text == variants_text(names, recs)
    assert [(names.index(v["genome"]), v["position"], "ACGT".index(v["ref"]), "ACGT".index(v["alt"]), v["depth"],
             v["alt_count"], (v["A"], v["C"], v["G"], v["T"])) for v in pa.get_variants()] == recs
    assert not any("ileup" in key for key in pa.__getstate__())  # (never part of an .aln file)
    # looser thresholds, so that the file holds records whatever the defaults give
    r = TC.run_cli(["--variants", f, "--variant-min-depth", "1", "--variant-min-count", "1",
                    "--variant-min-fraction", "0.05", "--variant-min-base-quality", "40"])
    assert r.returncode == 0, r.stderr
    names, recs = config1_records(triple=(1, 1, 50), mbq=40)
    assert len(recs) >= 1 and open(f).read() == variants_text(names, recs)


def test_cli_variants_both_strands(tmp_path):
    f = str(tmp_path / "v.tsv")
    plain = TC.run_cli(["--both-strands"])
    r = TC.run_cli(["--both-strands", "--variants", f, "--variant-min-depth", "1", "--variant-min-count", "1",
                    "--variant-min-fraction", "0"])
    assert r.returncode == 0 and plain.returncode == 0, r.stderr + plain.stderr
    assert r.stdout == plain.stdout
    names, recs = config1_records(both=True, triple=(1, 1, 0))
    assert len(recs) >= 1 and open(f).read() == variants_text(names, recs)


def test_cli_variants_composes(tmp_path):
    f, a = str(tmp_path / "v.tsv"), str(tmp_path / "a.tsv")
    r = TC.run_cli(["--coverage", "--assignments", a, "--variants", f])
    both = TC.run_cli(["--coverage", "--assignments", str(tmp_path / "a2.tsv")])
    assert r.returncode == 0 and both.returncode == 0, r.stderr + both.stderr
    assert r.stdout == both.stdout and open(a).read() == open(str(tmp_path / "a2.tsv")).read()
    names, recs = config1_records()
    assert open(f).read() == variants_text(names, recs)


@pytest.mark.parametrize("argv", [
    ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--variant-min-depth", "2"],
    ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--variant-min-count", "2"],
    ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--variant-min-fraction", "0.5"],
    ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--variant-min-base-quality", "30"],
    ["-t", "dumpalign", "-a", "x.aln", "--variants", "v.tsv"],
    ["-t", "dumpref", "-g", FA, "-k", "21", "--variants", "v.tsv"],
    ["-t", "reference", "-g", FA, "-k", "21", "-r", "x.kdb", "--variants", "v.tsv"],
    ["-t", "align", "-g", FA, "-k", "21", "--reads", FQ, "-a", "x.aln", "-r", "x.kdb", "--variants", "v.tsv"],
    ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--variants", "no_such_dir/v.tsv"],
    ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--variants", "v.tsv", "--variant-min-depth", "0"],
    ["-t", "dumpalign", "-g", FA, "-k", "21", "--reads", FQ, "--variants", "v.tsv", "--variant-min-fraction", "1.5"],
], ids=["min_depth", "min_count", "min_fraction", "min_base_quality", "alignfile", "dumpref", "reference", "align",
        "unwritable", "min_depth_0", "fraction_above_1"])
def test_cli_variants_misuse(argv, tmp_path):
    r = subprocess.run([sys.executable, MAIN] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0 and r.stdout == ""
    assert r.stderr.strip().startswith("Error:") and len(r.stderr.strip().splitlines()) == 1
    assert not os.path.exists(str(tmp_path / "v.tsv"))
