"""k_align_lane's scheduling (chunks claimed from a device
counter, the next chunk's offsets fetched an iteration ahead, the queue
segments under claimed chunks), its mismatch scan and its validity test while
packing, against the CPU oracle: stats, unique, ambiguous and first keys bit
for bit, with a nonzero read base.

PA_LANE_GRID=<blocks> caps the lane kernel's grid, so that a small batch runs
many chunks per wave.  Every case's reads fall into at least two of unique,
ambiguous and unmapped on the oracle's side (asserted before the GPU runs).
"""

import numpy as np
import pytest

import pa_native as N
import pa_oracle as O
import synth

pytestmark = pytest.mark.gpu

K = 31
BASE = 12345
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    COMP[_a] = _b
PARAMS = {"default": dict(), "m0p0": dict(m=0, p=0), "mg2": dict(mg=2)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


def make_genomes():
    """Ten 30-kb genomes in families of three, with N runs and two inverted
    repeats each (a stretch copied reverse-complemented further on: the few
    reverse-strand reads of it map)."""
    gens = synth.family_genomes(10, 30000, seed=181, family_size=3, sub_rate=0.01, conserved_len=500,
                                n_rate=2e-4, n_run=8)
    rng = np.random.default_rng(182)
    for g in gens:
        for _ in range(2):
            ln = int(rng.integers(60, 200))
            a0 = int(rng.integers(0, len(g) - 2 * ln - 1))
            b0 = int(rng.integers(a0 + ln, len(g) - ln))
            g[b0:b0 + ln] = COMP[g[a0:a0 + ln][::-1]]
    return gens


@pytest.fixture(scope="module")
def world():
    gens = make_genomes()
    return {"gens": gens, "index": N.Index(gens, K), "oracle": O.OracleIndex(gens, K), "memo": {}}


def offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return off


def oracle_of(world, key, s, q, off, ps):
    """The oracle's result of a batch, computed once per (batch, parameters)."""
    memo = world["memo"]
    if key not in memo:
        full = {"m": 1, "p": 1, "mrq": None, "mkq": None, "mg": None, **ps}
        o = world["oracle"].align(s.tobytes(), q.tobytes(), off, m=full["m"], p=full["p"], mrq=full["mrq"],
                                  mkq=full["mkq"], mg=full["mg"], read_base=BASE, detail=False)
        assert sum(int(x) > 0 for x in o.stats[:3]) >= 2, (key, o.stats.tolist())  # (the case is worth running)
        memo[key] = o
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


def mixed_reads(gens, n, seed):
    """150-bp reads at 1 % substitutions; every tenth reverse-complemented,
    every tenth of a random (unindexed) organism."""
    seq, _, _ = synth.sample_reads(gens, n, 150, seed=seed, err_rate=0.01)
    rng = np.random.default_rng(seed + 1)
    kind = rng.integers(0, 10, n)
    rc = kind == 0
    seq[rc] = COMP[seq[rc][:, ::-1]]
    fg = kind == 1
    seq[fg] = ACGT[rng.integers(0, 4, (int(fg.sum()), 150))]
    return seq


# ---- chunk claiming ---------------------------------------------------------

@pytest.mark.parametrize("grid", [1, 2, None], ids=["grid1", "grid2", "uncapped"])
def test_chunk_claiming(world, grid, monkeypatch):
    """Batches of 1, 63, 64, 65, 64 W - 1 and 64 W + 1 reads (W: the capped
    grid's waves), and one that gives every wave tens of chunks, so that waves
    claim past their first two chunks, finish at different times and drain
    their lists of reads to walk again after the last claim; the same batch
    twice gives the same counters (the claim counter is reset per pass)."""
    if grid is not None:
        monkeypatch.setenv("PA_LANE_GRID", str(grid))
    w = 4 * (grid or 2)
    sizes = [1, 63, 64, 65, 64 * w - 1, 64 * w + 1, 64 * w * 20 + 17]
    if grid is None:
        sizes[-1] = 20000  # (more blocks than a capped grid: some waves get no chunk, some one)
    if "mixed" not in world["memo"]:  # (one batch: every size is a prefix of it)
        world["memo"]["mixed"] = mixed_reads(world["gens"], 20000, 190)
    seq = world["memo"]["mixed"]
    qual = np.full_like(seq, ord("I"))
    for n in sizes:
        # (a single read: two classes cannot be; the batch of 63 holds it)
        s, q, off = seq[:n].reshape(-1), qual[:n].reshape(-1), offsets([150] * n)
        if n == 1:
            full = world["oracle"].align(s.tobytes(), q.tobytes(), off, m=1, p=1, mrq=None, mkq=None, mg=None,
                                         read_base=BASE, detail=False)
        else:
            full = oracle_of(world, ("claim", n), s, q, off, {})
        got = gpu_of(world["index"], s, q, off, {})
        assert_equal(got, full, (grid, n))
        if n == sizes[-1]:
            again = gpu_of(world["index"], s, q, off, {})
            for x, y in zip(got, again):
                assert x.tolist() == y.tolist(), (grid, n)


@pytest.mark.parametrize("variant", ["mkq", "mrq_mkq_mg", "k63"])
@pytest.mark.parametrize("grid", [1, 2], ids=["grid1", "grid2"])
def test_chunk_claiming_other_kernels(world, grid, variant, monkeypatch):
    """Claimed chunks in the other instantiations that run them: the window
    quality masks (qualities spread so that the filters fire), with
    --max-genomes too, and two-word keys (k = 63); tens of chunks per wave."""
    monkeypatch.setenv("PA_LANE_GRID", str(grid))
    n = 64 * 4 * grid * 20 + 17
    if "mixed" not in world["memo"]:
        world["memo"]["mixed"] = mixed_reads(world["gens"], 20000, 190)
    seq = world["memo"]["mixed"][:n]
    qual = np.clip(np.random.default_rng(191).normal(60, 8, seq.shape).round(), 35, 74).astype(np.uint8)
    s, q, off = seq.reshape(-1), qual.reshape(-1), offsets([150] * n)
    ps = {"mkq": dict(mkq=58), "mrq_mkq_mg": dict(mrq=53, mkq=58, mg=10), "k63": dict()}[variant]
    w = world
    if variant == "k63":
        if "k63" not in world["memo"]:
            world["memo"]["k63"] = {"index": N.Index(world["gens"], 63), "oracle": O.OracleIndex(world["gens"], 63),
                                    "memo": {}}
        w = world["memo"]["k63"]
    o = oracle_of(w, ("claim", variant, n), s, q, off, ps)
    assert_equal(gpu_of(w["index"], s, q, off, ps), o, (grid, variant))


# ---- queue segments under claimed chunks ------------------------------------

def seedless_batch(gens, which):
    """20 000 reads none of which has a seed in the index: reverse-complemented
    ones (a few, of the inverted repeats, map all the same) or a random
    organism's, the latter followed by one chunk of plain reads."""
    if which == "rc":
        seq, _, _ = synth.sample_reads(gens, 20000, 150, seed=201, err_rate=0.005)
        return COMP[seq[:, ::-1]]
    rng = np.random.default_rng(202)
    seq = ACGT[rng.integers(0, 4, (20000, 150))]
    tail, _, _ = synth.sample_reads(gens, 64, 150, seed=203, err_rate=0.005)
    return np.concatenate([seq, tail])


@pytest.mark.parametrize("ps", list(PARAMS), ids=list(PARAMS))
@pytest.mark.parametrize("rcwalk", ["1", "0"], ids=["rcwalk", "norcwalk"])
@pytest.mark.parametrize("seg", ["1", "0"], ids=["seg", "flat"])
@pytest.mark.parametrize("which", ["rc", "foreign"])
def test_segments_under_claims(world, which, seg, rcwalk, ps, monkeypatch):
    """Every read seedless and one block's four waves taking all 313 chunks:
    a wave that runs ahead fills its queue segment and must stop claiming, the
    others take the rest; no read lost, none written past a segment."""
    monkeypatch.setenv("PA_NA_MIN", "0")
    monkeypatch.setenv("PA_LANE_GRID", "1")
    monkeypatch.setenv("PA_NA_SEG", seg)
    monkeypatch.setenv("PA_NA_RCWALK", rcwalk)
    memo = world["memo"]
    if ("seedless", which) not in memo:
        memo[("seedless", which)] = seedless_batch(world["gens"], which)
    seq = memo[("seedless", which)]
    s, q, off = seq.reshape(-1), np.full(seq.size, ord("I"), dtype=np.uint8), offsets([150] * len(seq))
    o = oracle_of(world, ("seedless", which, ps), s, q, off, PARAMS[ps])
    assert o.stats[2] >= 18000  # (unmapped: the seedless reads)
    assert_equal(gpu_of(world["index"], s, q, off, PARAMS[ps]), o, (which, seg, rcwalk, ps))


# ---- the walk's mismatch scan -----------------------------------------------

def mismatch_reads(gens):
    """Reads cut from genome 0 (and one across an N run) with substitutions
    placed by hand, at lengths 31, 32, 150, 160 and 176."""
    g = gens[0]
    code = np.zeros(256, dtype=np.int64)
    for i, c in enumerate(b"ACGT"):
        code[c] = i
    clean = np.flatnonzero(np.convolve((g == ord("N")).astype(np.int64), np.ones(176, dtype=np.int64))[175:] == 0)
    rng = np.random.default_rng(210)
    reads = []

    def cut(start, length, subs):
        r = g[start:start + length].copy()
        for p in subs:
            r[p] = ACGT[(code[r[p]] + 1 + p % 3) % 4] if r[p] != ord("N") else ord("A")
        r[r == ord("N")] = ord("A")  # (a read holds no N: some base against the genome's N run)
        reads.append(r)

    for length in (31, 32, 150, 160, 176):
        last, last_whole = length - 1, 32 * (length // 32) - 1
        spread = lambda n: sorted({int(x) for x in np.linspace(0, last, n).round()})  # noqa: E731
        patterns = [[], [0], [31], [32], [63], [64], [last], [last_whole], [3, 17], [40, 45], [30, 33], [62, 65],
                    spread(8), spread(9), spread(40), spread(41)]
        for subs in patterns:
            subs = sorted({p for p in subs if p < length})
            for _ in range(3):  # (three places of the genome each: conserved and specific stretches)
                cut(int(clean[rng.integers(0, len(clean))]), length, subs)
    # a mismatch inside an N run of the genome: reads across the first N runs, with and without
    # substitutions next to the run
    nruns = np.flatnonzero((g[1:] == ord("N")) & (g[:-1] != ord("N"))) + 1
    for st in nruns[:4]:
        for length in (150, 176):
            lo = max(0, int(st) - length // 2)
            if lo + length <= len(g):
                cut(lo, length, [])
                cut(lo, length, [int(st) - lo - 1])
    return reads


@pytest.mark.parametrize("nb", ["serving", "no_nb"])
def test_mismatch_scan(world, nb):
    """Substitutions at the word boundaries of the walk's XOR words, two in
    one word and across a boundary, at the neighbour-bit budget (8, 9) and
    the walk's cap (40, 41), and against an N run of the genome -- on a
    serving index (neighbour bits) and on one prepared for so few reads that
    none exist (every mismatch window probed)."""
    reads = mismatch_reads(world["gens"])
    s = np.concatenate(reads)
    q, off = np.full(s.size, ord("I"), dtype=np.uint8), offsets([len(r) for r in reads])
    index = world["index"]
    if nb == "no_nb":
        index = N.Index(world["gens"], K, defer_tiles=True)
        index.prepare(expected_reads=1)
    for ps in PARAMS:
        o = oracle_of(world, ("mismatch", ps), s, q, off, PARAMS[ps])
        assert_equal(gpu_of(index, s, q, off, PARAMS[ps]), o, (nb, ps))
    if nb == "no_nb":  # (still without the bits after these few reads)
        assert int(index.info().device_bytes) < int(world["index"].info().device_bytes)


# ---- the validity test while packing ----------------------------------------

def test_validity_while_packing(world):
    """N, a lower-case base and a zero byte at the first, a middle and the last
    base of a read; clean reads whose neighbours in the buffer end and start
    with N stay clean; the last read of the batch runs against the padding."""
    seq, _, _ = synth.sample_reads(world["gens"], 400, 150, seed=220, err_rate=0.005)
    reads = [r.copy() for r in seq]
    i = 0
    for bad in (ord("N"), ord("a"), ord("c"), ord("g"), ord("t"), 0):
        for pos in (0, 77, 149):
            reads[3 * i + 1][pos] = bad  # (read 3 i + 1 bad, its neighbours 3 i and 3 i + 2 clean)
            i += 1
    # clean reads between reads ending and starting with N, at every alignment of the 16-B chunks
    for j in range(100, 132, 2):
        reads[j] = reads[j][:150 - (j - 100) // 2]  # (shifts the following reads byte by byte)
        reads[j][-1] = ord("N")
        reads[j + 2][0] = ord("N")
    lens = [len(r) for r in reads]
    s = np.concatenate(reads)
    q, off = np.full(s.size, ord("I"), dtype=np.uint8), offsets(lens)
    for ps in PARAMS:
        o = oracle_of(world, ("validity", ps), s, q, off, PARAMS[ps])
        assert_equal(gpu_of(world["index"], s, q, off, PARAMS[ps]), o, ps)
    # the batch's last read alone against the padding, clean and with a bad last base
    for bad in (None, ord("N")):
        tail = [r.copy() for r in seq[200:265]]
        if bad is not None:
            tail[-1][149] = bad
        s = np.concatenate(tail)
        q, off = np.full(s.size, ord("I"), dtype=np.uint8), offsets([150] * len(tail))
        o = oracle_of(world, ("validity-tail", bad), s, q, off, {})
        assert_equal(gpu_of(world["index"], s, q, off, {}), o, bad)
