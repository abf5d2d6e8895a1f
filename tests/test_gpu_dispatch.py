"""The launch layer's selection matrix, walked once on
the smallest world that reaches every kernel family: key widths NW 1, 2, 3
(k = 31, 45, 75), the 150-bp and the 250-bp read shape (NM 2, 4), the filter
sets (none; --min-read-quality; both quality filters) each with and without
--max-genomes 2, in the counter pass (pa_align) and the assign pass
(pa_align_reads).  Every cell is compared with the oracle, and the per-kernel
launch counts show that the lane chain -- not the wave or exact kernel alone
-- did the work.

World: 6 genomes x 6 kb in families of 3 (1 % substitutions, 500 conserved
bases); per k one index and one oracle; 1024 synthesized 150-bp reads (0.5 %
errors, 30 % reverse strand, 20 % foreign), at k = 31 also 512 of 250 bp.  An
index of this size has a Bloom filter and, at k = 31, a reverse-complement
plane, so the genomes need no enlarging.  PA_NA_MIN=0: the seedless chain
takes its reads however few they are.  The read seeds are chosen so that every
oracle batch holds UNIQUE, AMBIGUOUS and UNMAPPED reads and, with
--min-read-quality, DROPPED ones (the 250-bp batch has exactly one at 58)."""

import numpy as np
import pytest

import pa_native as N
import pa_oracle as O
import synth
from test_gpu_assign import params_of, same

pytestmark = pytest.mark.gpu

BASE = 54321
UNIQUE, AMBIGUOUS, UNMAPPED, DROPPED = 2, 3, 1, 0
BATCHES = {150: (1024, 7), 250: (512, 22)}  # read length: (reads, seed)
SHAPES = [(31, 150), (31, 250), (45, 150), (75, 150)]
FILTERS = {"none": dict(), "mrq": dict(mrq=60), "mrq_mkq": dict(mrq=58, mkq=60)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X (no CPU fallback exists)")


@pytest.fixture(scope="module")
def world():
    """The genomes and a memo: per k the index and the oracle, per (k, read
    length) the batch on the device and on the host.  All made once, on demand."""
    gens = synth.family_genomes(6, 6000, seed=1, family_size=3, sub_rate=0.01, conserved_len=500)
    return {"gens": gens, "memo": {}}


def index_of(world, k):
    memo = world["memo"]
    if ("index", k) not in memo:
        memo[("index", k)] = (N.Index(world["gens"], k), O.OracleIndex(world["gens"], k))
    return memo[("index", k)]


def batch_of(world, k, rlen):
    memo = world["memo"]
    if ("batch", k, rlen) not in memo:
        n, seed = BATCHES[rlen]
        reads = N.Reads.synthesize(index_of(world, k)[0], n, rlen, seed=seed, sub_rate=0.005, rc_rate=0.3,
                                   foreign_rate=0.2)
        memo[("batch", k, rlen)] = (reads, reads.download())
    return memo[("batch", k, rlen)]


def launches(kernels):
    return {name: n for name, (_, n) in kernels.items()}


@pytest.mark.parametrize("mg", [None, 2], ids=["nomg", "mg2"])
@pytest.mark.parametrize("filters", list(FILTERS))
@pytest.mark.parametrize("k,rlen", SHAPES, ids=[f"k{k}_len{r}" for k, r in SHAPES])
def test_cell(world, k, rlen, filters, mg, monkeypatch):
    monkeypatch.setenv("PA_NA_MIN", "0")
    ps = dict(FILTERS[filters], **({"mg": mg} if mg else {}))
    full, prm = params_of(ps)
    index, oracle = index_of(world, k)
    reads, (s, q, off) = batch_of(world, k, rlen)
    o = oracle.align(s.tobytes(), q.tobytes(), off, m=full["m"], p=full["p"], mrq=full["mrq"], mkq=full["mkq"],
                     mg=full["mg"], read_base=BASE, detail=True)
    # the inputs reach every outcome (a condition on the batch, by the oracle alone)
    for t in (UNIQUE, AMBIGUOUS, UNMAPPED) + ((DROPPED,) if "mrq" in ps else ()):
        assert int((o.types == t).sum()) > 0, (t, np.bincount(o.types, minlength=4).tolist())

    res = N.Result(index)
    index.profile_enable(True)
    try:
        index.profile_read_kernels()
        N.align(index, reads, prm, BASE, res)
        counter = launches(index.profile_read_kernels())
        got = N.align_reads(index, reads, prm)
        assign = launches(index.profile_read_kernels())
    finally:
        index.profile_enable(False)
    stats, uq, am, fk = res.fetch()
    res.close()
    print(k, rlen, ps, "counter pass", counter, "assign pass", assign)

    assert stats.tolist() == o.stats.tolist()
    assert uq.tolist() == o.unique.tolist() and am.tolist() == o.ambiguous.tolist()
    assert fk.tolist() == o.first_key.tolist()
    same(got, (o.types, o.qf, o.hr, o.list_off, o.lists), (k, rlen, ps))

    assert counter["k_align_fast"] == 1 and assign["k_align_fast"] == 0, (counter, assign)
    if rlen == 250 and "mkq" in ps:
        return  # (window masks cover 128 windows: these reads go to the wave kernel by design)
    for what, n in (("counter", counter), ("assign", assign)):
        assert n["k_align_lane"] == 1 and n["k_align_lane_na"] == 1, (what, n)
        if k == 31:  # the reverse-strand walk: single-word keys only
            assert n["k_rc_seeds"] == 1 and n["k_align_lane_rc"] == 1, (what, n)
