"""k_align_lane's reads that are walked again:
a read whose walk already shows present specific neighbours against too few
walked specific k-mers probes one of them for its new anchor, and is given up
unprobed if its second walk shows the same (PA_LANE_SURE).  Against the CPU
oracle: stats, unique, ambiguous and first keys bit for bit, with a nonzero
read base.

The index is 10 genomes x 30 kb in families of 5, so most reads of a genome
but the first of its family are first walked on a sibling.  The engineered
cases are selected on the host from a k-mer table of the genomes (asserted
before the GPU runs):
  * sibling walks: error-free 170-bp reads of the last member of a family
    whose own substitutions lie only at the bases no seed window covers (seeds
    start at bases 0, 34, 69, 104, 139), every seed k-mer shared with a sibling;
  * second-walk give-ups: 170-bp chimeras of two non-first members at the
    same coordinates which, walked on the first half's genome, again have
    more present specific neighbours than walked specific k-mers.
"""

import numpy as np
import pytest

import pa_native as N
import pa_oracle as O
import synth

pytestmark = pytest.mark.gpu

K = 31
BASE = 54321
FAM = 5
RLEN = 170
SEEDS = (0, 34, 69, 104, 139)
GAPS = (31, 32, 33, 65, 66, 67, 68, 100, 101, 102, 103, 135, 136, 137, 138)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i
PARAMS = {"default": dict(), "m0p0": dict(m=0, p=0), "m3": dict(m=3), "pneg": dict(p=-1), "mg2": dict(mg=2),
          "mg1": dict(mg=1), "mkq": dict(mkq=58)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


def make_genomes():
    return synth.family_genomes(10, 30000, seed=311, family_size=FAM, sub_rate=0.01, conserved_len=500,
                                n_rate=2e-4, n_run=8)


# ---- host k-mer table ---------------------------------------------------------

def kmer_codes(seq, k=K):
    """2-bit codes of every window of the last axis (uint64, k <= 32) and
    whether the window holds only ACGT."""
    c = CODE[np.asarray(seq, dtype=np.uint8)]
    n = c.shape[-1] - k + 1
    kc = np.zeros(c.shape[:-1] + (n,), dtype=np.uint64)
    bad = np.zeros(c.shape[:-1] + (n,), dtype=bool)
    for j in range(k):
        cj = c[..., j:j + n]
        bad |= cj == 255
        kc = (kc << np.uint64(2)) | (cj & 3).astype(np.uint64)
    return kc, ~bad


class KmerTable:
    """Every k-mer of the genomes: in how many genomes it lies, and the first."""

    def __init__(self, gens):
        keys, owner = [], []
        for g, s in enumerate(gens):
            kc, ok = kmer_codes(s)
            u = np.unique(kc[ok])
            keys.append(u)
            owner.append(np.full(u.size, g, dtype=np.int64))
        keys, owner = np.concatenate(keys), np.concatenate(owner)
        order = np.argsort(keys, kind="stable")
        keys, owner = keys[order], owner[order]
        self.keys, first, self.count = np.unique(keys, return_index=True, return_counts=True)
        self.owner = owner[first]

    def lookup(self, kc):
        """(number of genomes holding each k-mer -- 0: absent --, the first of them)"""
        i = np.minimum(np.searchsorted(self.keys, kc), self.keys.size - 1)
        hit = self.keys[i] == kc
        return np.where(hit, self.count[i], 0), np.where(hit, self.owner[i], -1)


def sibling_walk_reads(gens, table):
    """Reads of the last member of each family (module docstring)."""
    reads = []
    gaps = np.array(GAPS)
    for last in range(FAM - 1, len(gens), FAM):
        fam = np.stack(gens[last - FAM + 1:last + 1])
        votes = np.stack([(fam == b).sum(0) for b in ACGT])
        own = (fam[-1] != ACGT[votes.argmax(0)]) | (fam[-1] == ord("N"))
        cum = np.concatenate([[0], np.cumsum(own)])
        starts = np.arange(fam.shape[1] - RLEN + 1)
        total = cum[starts + RLEN] - cum[starts]
        in_gaps = own[starts[:, None] + gaps[None, :]].sum(1)
        starts = starts[(total == in_gaps) & (in_gaps >= 1)]
        seq = fam[-1][starts[:, None] + np.arange(RLEN)[None, :]]
        keep = ~(seq == ord("N")).any(1)
        seq = seq[keep]
        kc, ok = kmer_codes(seq)
        cnt, owner = table.lookup(kc)
        shared_seeds = (cnt[:, list(SEEDS)] >= 2).all(1)                  # (first occurrence: an earlier member)
        specific = ((cnt == 1) & (owner == last) & ok).any(1)             # (a k-mer of this member alone)
        reads.append(seq[shared_seeds & specific])
    return np.concatenate(reads)


def sibling_chimeras(gens, table):
    """Chimeras that meet the rule again when walked on the first half's genome."""
    half = RLEN // 2
    out = []
    for f0 in range(0, len(gens), FAM):
        members = range(f0 + 1, f0 + FAM)
        for ga in members:
            for gb in members:
                if ga == gb:
                    continue
                starts = np.arange(0, len(gens[ga]) - RLEN + 1, 20)
                idx = starts[:, None] + np.arange(RLEN)[None, :]
                sa, sb = gens[ga][idx], gens[gb][idx]
                seq = np.concatenate([sa[:, :half], sb[:, half:]], axis=1)
                clean = ~((sa == ord("N")) | (sb == ord("N"))).any(1)
                seq, sa = seq[clean], sa[clean]
                kc, _ = kmer_codes(seq)
                cnt, owner = table.lookup(kc)
                cum = np.concatenate([np.zeros((len(seq), 1), dtype=np.int64), np.cumsum(seq != sa, axis=1)], axis=1)
                mis = cum[:, K:] - cum[:, :-K]                              # mismatches against ga per window
                nspec = ((mis == 0) & (cnt == 1)).sum(1)                    # (specific: of ga alone)
                sure = ((mis == 1) & (cnt == 1)).sum(1)                     # present, specific, one mismatch
                # the first walk must lead there: a specific k-mer of ga in the first half
                leads = ((cnt == 1) & (owner == ga))[:, :half - K + 1].any(1)
                out.append(seq[(sure > 0) & (nspec < sure + 1) & leads])
    return np.concatenate(out)


# ---- the world ----------------------------------------------------------------

@pytest.fixture(scope="module")
def world():
    gens = make_genomes()
    return {"gens": gens, "index": N.Index(gens, K), "oracle": O.OracleIndex(gens, K), "memo": {},
            "table": KmerTable(gens)}


def offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return off


def oracle_of(world, key, s, q, off, ps):
    """The oracle's result of a batch, computed once per (batch, parameters)."""
    memo = world["memo"]
    if key not in memo:
        full = {"m": 1, "p": 1, "mrq": None, "mkq": None, "mg": None, **ps}
        memo[key] = world["oracle"].align(s.tobytes(), q.tobytes(), off, m=full["m"], p=full["p"], mrq=full["mrq"],
                                          mkq=full["mkq"], mg=full["mg"], read_base=BASE, detail=False)
    return memo[key]


def gpu_of(index, s, q, off, ps):
    full = {"m": 1, "p": 1, "mrq": None, "mkq": None, "mg": None, **ps}
    res = N.Result(index)
    N.align(index, N.Reads.upload(s, q, off), N.Params.make(full["m"], full["p"], full["mrq"], full["mkq"], full["mg"]),
            BASE, res)
    return res.fetch()


def assert_equal(got, o, what):
    stats, uq, am, fk = got
    assert stats.tolist() == o.stats.tolist(), what
    assert uq.tolist() == o.unique.tolist() and am.tolist() == o.ambiguous.tolist(), what
    ofk = np.where(o.first_key == np.iinfo(np.uint64).max, N.NO_FIRST_KEY, o.first_key)
    assert fk.tolist() == ofk.tolist(), what


def engineered(world, which):
    """(reads, flat bases, qualities, offsets) of an engineered batch, made once."""
    memo = world["memo"]
    if ("reads", which) not in memo:
        make = {"sibling": sibling_walk_reads, "chimera": sibling_chimeras}[which]
        seq = make(world["gens"], world["table"])[:4000]
        memo[("reads", which)] = seq
    seq = memo[("reads", which)]
    s = seq.reshape(-1)
    return seq, s, np.full(s.size, ord("I"), dtype=np.uint8), offsets([RLEN] * len(seq))


def both_grids(world, key, index, s, q, off, ps, monkeypatch, w=None):
    """One block's four waves take every chunk (their lists of reads to walk
    again fill up and drain), then the uncapped grid."""
    o = oracle_of(w or world, key, s, q, off, ps)
    monkeypatch.setenv("PA_LANE_GRID", "1")
    assert_equal(gpu_of(index, s, q, off, ps), o, (key, "grid1"))
    monkeypatch.delenv("PA_LANE_GRID")
    assert_equal(gpu_of(index, s, q, off, ps), o, (key, "uncapped"))
    return o


# ---- case 1: natural reads ----------------------------------------------------

@pytest.mark.parametrize("ps", list(PARAMS), ids=list(PARAMS))
@pytest.mark.parametrize("err", [0.005, 0.015], ids=["e0.5", "e1.5"])
def test_natural_reads(world, err, ps, monkeypatch):
    memo = world["memo"]
    if ("natural", err) not in memo:
        memo[("natural", err)] = synth.sample_reads(world["gens"], 20000, 150, seed=int(err * 1e4) + 320, err_rate=err)
    seq, qual, origin = memo[("natural", err)]
    assert np.count_nonzero(origin % FAM) > 10000  # (reads of non-first members: first walked on a sibling)
    s, q, off = seq.reshape(-1), qual.reshape(-1), offsets([150] * len(seq))
    o = both_grids(world, ("natural", err, ps), world["index"], s, q, off, PARAMS[ps], monkeypatch)
    assert int(o.stats[0]) > 5000 and int(o.stats[1]) > 0  # (unique and ambiguous reads both)
    if ps == "mkq":
        assert int(o.stats[4]) > 0  # (the threshold filters some windows)


# ---- case 2: engineered sibling walks -----------------------------------------

@pytest.mark.parametrize("ps", ["default", "m3", "mg2"])
def test_sibling_walks(world, ps, monkeypatch):
    """No walked specific k-mer and at least one present specific neighbour."""
    seq, s, q, off = engineered(world, "sibling")
    assert len(seq) >= 50
    o = both_grids(world, ("sibling", ps), world["index"], s, q, off, PARAMS[ps], monkeypatch)
    if ps == "default":  # (error-free reads holding a k-mer of their genome alone)
        assert int(o.stats[0]) == len(seq)


# ---- case 3: second-walk give-ups ---------------------------------------------

@pytest.mark.parametrize("ps", ["default", "m0p0", "mg2"])
def test_second_walk_give_ups(world, ps, monkeypatch):
    seq, s, q, off = engineered(world, "chimera")
    assert len(seq) >= 10
    both_grids(world, ("chimera", ps), world["index"], s, q, off, PARAMS[ps], monkeypatch)


# ---- case 4: the path switched off by the data --------------------------------

def all_reads(world):
    """The engineered batches and 2000 natural reads at 1.5 % in one batch."""
    sib, chim = engineered(world, "sibling")[0], engineered(world, "chimera")[0]
    nat, _, _ = synth.sample_reads(world["gens"], 2000, 150, seed=330, err_rate=0.015)
    reads = list(sib) + list(chim) + list(nat)
    s = np.concatenate(reads)
    return s, np.full(s.size, ord("I"), dtype=np.uint8), offsets([len(r) for r in reads])


def test_without_neighbour_bits(world, monkeypatch):
    """An index prepared for so few reads that it has no neighbour bits."""
    s, q, off = all_reads(world)
    index = N.Index(world["gens"], K, defer_tiles=True)
    index.prepare(expected_reads=1)
    for ps in ("default", "mg2"):
        both_grids(world, ("all", ps), index, s, q, off, PARAMS[ps], monkeypatch)
    assert int(index.info().device_bytes) < int(world["index"].info().device_bytes)  # (still without them)
    # and the serving index on the same batch
    both_grids(world, ("all", "default"), world["index"], s, q, off, {}, monkeypatch)


def test_two_word_keys(world, monkeypatch):
    """k = 63: neighbour words without the specific half."""
    s, q, off = all_reads(world)
    w = {"oracle": O.OracleIndex(world["gens"], 63), "memo": {}}
    both_grids(world, ("all63", "default"), N.Index(world["gens"], 63), s, q, off, {}, monkeypatch, w=w)
