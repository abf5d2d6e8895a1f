"""pa_align_reads (the assign pass): the lane kernels
write the per-read result of every read they settle, the exact kernel in
detail mode takes the lane chain's queue.  Its five arrays must equal
pa_align_detail's on every batch -- that path is pinned to the oracle by the
rest of the suite -- and the natural batches are compared with the oracle's
per-read results directly.

The world is test_gpu_reanchor.py's: 10 genomes x 30 kb in families of 5, k = 31,
20 000 natural 150-bp reads at 0.5 % and 1.5 % errors with varying qualities."""

import numpy as np
import pytest

import pa_native as N
import pa_oracle as O
import synth

pytestmark = pytest.mark.gpu

K = 31
BASE = 54321
FAM = 5
PARAMS = {"default": dict(), "m0p0": dict(m=0, p=0), "m3": dict(m=3), "pneg": dict(p=-1), "mg2": dict(mg=2),
          "mg1": dict(mg=1), "mkq": dict(mkq=58), "mrq": dict(mrq=60)}
UNIQUE, AMBIGUOUS, UNMAPPED, DROPPED = 2, 3, 1, 0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


def make_genomes():
    return synth.family_genomes(10, 30000, seed=311, family_size=FAM, sub_rate=0.01, conserved_len=500,
                                n_rate=2e-4, n_run=8)


def offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return off


def natural(gens, err, n=20000, rlen=150):
    seq, qual, _ = synth.sample_reads(gens, n, rlen, seed=int(err * 1e4) + 320, err_rate=err)
    return seq.reshape(-1), qual.reshape(-1), offsets([rlen] * len(seq))


@pytest.fixture(scope="module")
def world():
    gens = make_genomes()
    return {"gens": gens, "index": N.Index(gens, K), "oracle": O.OracleIndex(gens, K), "memo": {}}


def batch(world, err):
    memo = world["memo"]
    if ("natural", err) not in memo:
        memo[("natural", err)] = natural(world["gens"], err)
    return memo[("natural", err)]


def params_of(ps):
    full = {"m": 1, "p": 1, "mrq": None, "mkq": None, "mg": None, **ps}
    return full, N.Params.make(full["m"], full["p"], full["mrq"], full["mkq"], full["mg"])


def oracle_of(world, key, s, q, off, ps, oracle=None):
    memo = world["memo"]
    if key not in memo:
        full, _ = params_of(ps)
        memo[key] = (oracle or world["oracle"]).align(s.tobytes(), q.tobytes(), off, m=full["m"], p=full["p"],
                                                      mrq=full["mrq"], mkq=full["mkq"], mg=full["mg"],
                                                      read_base=BASE, detail=True)
    return memo[key]


def same(got, want, what):
    names = ("types", "filtered_kmers", "redundant_kmers", "list_off", "lists")
    for name, a, b in zip(names, got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (what, name, bad[:5].tolist(), a[bad[:5]].tolist(), b[bad[:5]].tolist())


def assign_vs_detail(index, reads, ps, what):
    """align_reads against align_detail on an uploaded batch; returns the assign pass's arrays."""
    _, prm = params_of(ps)
    got = N.align_reads(index, reads, prm)
    same(got, N.align_detail(index, reads, prm), what)
    return got


def vs_oracle(got, o, what):
    same(got, (o.types, o.qf, o.hr, o.list_off, o.lists), (what, "oracle"))


def both_grids(index, s, q, off, ps, what, monkeypatch, o=None):
    reads = N.Reads.upload(s, q, off)
    monkeypatch.setenv("PA_LANE_GRID", "1")
    got = assign_vs_detail(index, reads, ps, (what, "grid1"))
    if o is not None:
        vs_oracle(got, o, (what, "grid1"))
    monkeypatch.delenv("PA_LANE_GRID")
    got = assign_vs_detail(index, reads, ps, (what, "uncapped"))
    if o is not None:
        vs_oracle(got, o, (what, "uncapped"))
    reads.close()
    return got


def list_lengths(o):
    return np.diff(o.list_off.astype(np.int64))


def demoted(o):
    """Reads whose list repeats its first genome (a p-demoted G*)."""
    ll, lo = list_lengths(o), o.list_off.astype(np.int64)
    return [r for r in np.flatnonzero(ll >= 2) if o.lists[lo[r]] in o.lists[lo[r] + 1:lo[r + 1]]]


# ---- parameter sets, both grids, against the oracle ----------------------------

@pytest.mark.parametrize("ps", list(PARAMS), ids=list(PARAMS))
@pytest.mark.parametrize("err", [0.005, 0.015], ids=["e0.5", "e1.5"])
def test_natural_reads(world, err, ps, monkeypatch):
    s, q, off = batch(world, err)
    o = oracle_of(world, ("natural", err, ps), s, q, off, PARAMS[ps])
    if ps == "mkq":
        assert int(o.qf.sum()) > 0  # (the threshold filters some windows)
    if ps == "mrq":
        assert 0 < int((o.types == DROPPED).sum()) < len(o.types)  # (and this one some reads)
    if ps in ("mg1", "mg2"):
        assert int(o.hr.sum()) > 0
    if ps == "default" and err == 0.015:
        ll = list_lengths(o)
        assert int((o.types == UNIQUE).sum()) > 5000
        assert int(((o.types == AMBIGUOUS) & (ll == 0)).sum()) > 0
        assert int(((o.types == AMBIGUOUS) & (ll >= 2)).sum()) > 0
        assert len(demoted(o)) > 0
    both_grids(world["index"], s, q, off, PARAMS[ps], ("natural", err, ps), monkeypatch, o)


def test_kernels_of_the_pass(world, monkeypatch):
    """The lane kernel runs, the wave kernel does not, the exact kernel runs twice
    (types, then lists) -- and under PA_ASSIGN=0 or PA_NO_LANE=1 the exact kernel alone."""
    s, q, off = batch(world, 0.015)
    reads = N.Reads.upload(s, q, off)
    index = world["index"]
    index.profile_enable(True)
    try:
        index.profile_read_kernels()
        want = N.align_reads(index, reads, N.Params.make())
        k = index.profile_read_kernels()
        assert k["k_align_lane"][1] == 1 and k["k_align_fast"][1] == 0 and k["k_align_exact"][1] == 2, k
        for env in ("PA_ASSIGN", "PA_NO_LANE"):
            monkeypatch.setenv(env, "0" if env == "PA_ASSIGN" else "1")
            same(N.align_reads(index, reads, N.Params.make()), want, env)
            k = index.profile_read_kernels()
            assert k["k_align_lane"][1] == 0 and k["k_align_fast"][1] == 0 and k["k_align_exact"][1] == 2, (env, k)
            monkeypatch.delenv(env)
    finally:
        index.profile_enable(False)
        reads.close()


# ---- the seedless chain ---------------------------------------------------------

@pytest.mark.parametrize("na_min", ["0", None], ids=["lane_na", "handed_on"])
def test_seedless_chain(world, na_min, monkeypatch):
    """Reverse-strand and foreign reads: k_align_lane_na, k_rc_seeds and
    k_align_lane_rc settle them (PA_NA_MIN=0), or hand the few on to the remainder."""
    reads = N.Reads.synthesize(world["index"], 5000, 150, seed=7, sub_rate=0.005, rc_rate=0.4, foreign_rate=0.2)
    if na_min is not None:
        monkeypatch.setenv("PA_NA_MIN", na_min)
    for ps in ("default", "mg2", "mkq"):
        got = assign_vs_detail(world["index"], reads, PARAMS[ps], ("mix", na_min, ps))
        assert int((got[0] == UNMAPPED).sum()) > 500 and int((got[0] == UNIQUE).sum()) > 500
    reads.close()


# ---- key widths -------------------------------------------------------------------

@pytest.mark.parametrize("k", [63, 75, 127])
def test_key_widths(world, k, monkeypatch):
    """Two- and three-word keys (k_align_lane_naw), and k = 127: no lane path, every read to the exact kernel."""
    s, q, off = batch(world, 0.005)
    n = 5000
    s, q, off = s[:150 * n], q[:150 * n], off[:n + 1]
    index = N.Index(world["gens"], k)
    o = oracle_of(world, ("k", k), s, q, off, {}, oracle=O.OracleIndex(world["gens"], k))
    both_grids(index, s, q, off, {}, ("k", k), monkeypatch, o)
    monkeypatch.setenv("PA_NA_MIN", "0")
    reads = N.Reads.upload(s, q, off)
    assign_vs_detail(index, reads, PARAMS["mkq"], ("k", k, "mkq", "na"))
    reads.close()


# ---- read shapes --------------------------------------------------------------------

@pytest.mark.parametrize("rlen", [250, 170])
def test_long_shapes(world, rlen, monkeypatch):
    s, q, off = natural(world["gens"], 0.01, n=5000, rlen=rlen)
    for ps in ("default", "mg2", "mrq"):
        both_grids(world["index"], s, q, off, PARAMS[ps], ("len", rlen, ps), monkeypatch)


def test_mixed_batch(world, monkeypatch):
    """A length-0 read, reads shorter than k, one of exactly k bases, reads with
    N, uniform random reads, a 400-bp read (overlong: deferred), among natural ones."""
    rng = np.random.default_rng(5)
    g = world["gens"][3]
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    withn = g[1000:1150].copy()
    withn[70] = ord("N")
    reads = [np.zeros(0, dtype=np.uint8), g[10:20].copy(), g[100:130].copy(), g[500:500 + K].copy(), withn,
             acgt[rng.integers(0, 4, 150)], acgt[rng.integers(0, 4, 150)], g[2000:2400].copy(),
             np.full(150, ord("N"), dtype=np.uint8)]
    ns, nq, _ = batch(world, 0.015)
    for i in range(300):
        reads.insert(int(rng.integers(0, len(reads) + 1)), ns[150 * i:150 * (i + 1)])
    s = np.concatenate(reads)
    q = rng.integers(40, 75, s.size).astype(np.uint8)
    off = offsets([len(r) for r in reads])
    for ps in ("default", "mkq", "mrq", "mg1"):
        o = oracle_of(world, ("mixed", ps), s, q, off, PARAMS[ps])
        both_grids(world["index"], s, q, off, PARAMS[ps], ("mixed", ps), monkeypatch, o)


# ---- indexes ------------------------------------------------------------------------

def test_both_strand_index(world, monkeypatch):
    s, q, off = batch(world, 0.015)
    n = 5000
    s, q, off = s[:150 * n].copy(), q[:150 * n], off[:n + 1]
    rows = s.reshape(n, 150)
    rows[::2] = synth.reverse_complement(rows[::2])  # (every other read from the reverse strand)
    index = N.Index(world["gens"], K, both_strands=True)
    oracle = O.OracleIndex([synth.both_strands_genome(g) for g in world["gens"]], K)
    o = oracle_of(world, ("both",), s, q, off, {}, oracle=oracle)
    assert int((o.types == UNIQUE).sum()) > 2500
    both_grids(index, s, q, off, {}, ("both",), monkeypatch, o)


def test_without_neighbour_bits(world, monkeypatch):
    s, q, off = batch(world, 0.015)
    index = N.Index(world["gens"], K, defer_tiles=True)
    index.prepare(expected_reads=1)
    for ps in ("default", "mg2"):
        o = oracle_of(world, ("natural", 0.015, ps), s, q, off, PARAMS[ps])
        both_grids(index, s, q, off, PARAMS[ps], ("no_nb", ps), monkeypatch, o)


def test_compact_table(world, monkeypatch):
    s, q, off = batch(world, 0.015)
    o = oracle_of(world, ("natural", 0.015, "default"), s, q, off, {})
    both_grids(N.Index(world["gens"], K, compact=True), s, q, off, {}, ("compact",), monkeypatch, o)


def test_many_genomes(monkeypatch):
    """600 genomes: above the lane kernel's 512-genome cap of LDS counters."""
    gens = synth.family_genomes(600, 2000, seed=17, family_size=5, sub_rate=0.02, conserved_len=200)
    seq, qual, _ = synth.sample_reads(gens, 5000, 150, seed=18, err_rate=0.01)
    s, q, off = seq.reshape(-1), qual.reshape(-1), offsets([150] * len(seq))
    o = O.OracleIndex(gens, K).align(s.tobytes(), q.tobytes(), off, read_base=BASE, detail=True)
    both_grids(N.Index(gens, K), s, q, off, {}, ("g600",), monkeypatch, o)


# ---- ties to the counter path ---------------------------------------------------------

@pytest.mark.parametrize("ps", ["default", "mkq", "mg2", "mrq"])
def test_counters_from_assignments(world, ps):
    """stats, unique[g], ambiguous[g] and the first keys recomputed from the
    per-read arrays equal pa_align's on the same batch (read base != 0)."""
    s, q, off = batch(world, 0.015)
    _, prm = params_of(PARAMS[ps])
    reads = N.Reads.upload(s, q, off)
    types, qf, hr, loff, lists = N.align_reads(world["index"], reads, prm)
    res = N.Result(world["index"])
    N.align(world["index"], reads, prm, BASE, res)
    reads.close()
    stats, uq, am, fk = res.fetch()
    G = len(world["gens"])
    want = [int((types == t).sum()) for t in (UNIQUE, AMBIGUOUS, UNMAPPED, DROPPED)] + [int(qf.sum()), int(hr.sum())]
    assert stats.tolist() == want
    loff = loff.astype(np.int64)
    owner = np.repeat(np.arange(len(types)), np.diff(loff))
    pos = np.arange(len(lists)) - loff[owner]
    is_u = types[owner] == UNIQUE
    assert np.bincount(lists[is_u], minlength=G).tolist() == uq.tolist()
    assert np.bincount(lists[~is_u], minlength=G).tolist() == am.tolist()
    first = np.full(G, int(N.NO_FIRST_KEY), dtype=np.uint64)
    keys = ((owner.astype(np.uint64) + np.uint64(BASE)) << np.uint64(20)) | pos.astype(np.uint64)
    np.minimum.at(first, lists, keys)
    assert first.tolist() == fk.tolist()


# ---- the call's protocol ------------------------------------------------------------------

def test_list_cap_too_small(world):
    s, q, off = batch(world, 0.015)
    _, prm = params_of({})
    reads = N.Reads.upload(s, q, off)
    want = N.align_detail(world["index"], reads, prm)
    total = int(want[3][-1])
    assert total > 1
    for cap in (0, 1, total - 1):
        st, types, qf, hr, loff, _, got_total = N.align_reads_call(world["index"], reads, prm, cap)
        assert st == N.PA_EINVAL and got_total == total
        same((types, qf, hr, loff), want[:4], ("cap", cap))
    st, types, qf, hr, loff, lists, got_total = N.align_reads_call(world["index"], reads, prm, total)
    assert st == N.PA_OK and got_total == total
    same((types, qf, hr, loff, lists[:total]), want, "second call")
    reads.close()


def test_nullable_counters(world):
    s, q, off = batch(world, 0.005)
    _, prm = params_of(PARAMS["mkq"])
    reads = N.Reads.upload(s, q, off)
    want = N.align_detail(world["index"], reads, prm)
    st, types, qf, hr, loff, lists, total = N.align_reads_call(world["index"], reads, prm, len(types_of(want)),
                                                                counters=False)
    assert st == N.PA_OK and qf is None and hr is None
    same((types, loff, lists[:total]), (want[0], want[3], want[4]), "no counters")
    reads.close()


def types_of(arrays):
    return arrays[0]


def test_no_reads(world):
    e = np.zeros(0, dtype=np.uint8)
    reads = N.Reads.upload(e, e, np.zeros(1, dtype=np.uint64))
    types, qf, hr, loff, lists = N.align_reads(world["index"], reads, N.Params.make())
    assert len(types) == len(qf) == len(hr) == len(lists) == 0 and loff.tolist() == [0]
    reads.close()


def test_callers_result_untouched(world):
    """The lane kernels' counters of an assign pass go to scratch, never to a result of the caller's."""
    s, q, off = batch(world, 0.005)
    _, prm = params_of({})
    reads = N.Reads.upload(s, q, off)
    res = N.Result(world["index"])
    N.align(world["index"], reads, prm, BASE, res)
    before = [a.copy() for a in res.fetch()]
    N.align_reads(world["index"], reads, prm)
    after = res.fetch()
    for a, b in zip(before, after):
        assert a.tolist() == b.tolist()
    reads.close()
